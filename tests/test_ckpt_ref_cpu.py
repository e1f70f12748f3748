"""tests/ckpt_ref.py, the numpy reference of the checkpoint's view coding (include/gx_ckpt.h): round
trips on the shapes the device coder is checked at, and the stored size by the formula."""
import numpy as np
import pytest

from tests import ckpt_ref
from tests.ckpt_ref import BLOCK, U64, decode_views, encode_views, nblk_of, pw_of, view_section_bytes

# R: below a block; odd; one block exactly; one slot into the next; a ragged last block; three blocks
SIZES = [(5, 4), (33, 99), (16, 512), (19, 513), (70, 770), (96, 1536)]


def words(rng, shape):
    """Packed slot words: (time << 3) | status, like the engine's."""
    return (rng.integers(1, 1 << 40, size=shape, dtype=np.uint64) << U64(3)) | rng.integers(0, 4, size=shape, dtype=np.uint64)


def cases(Hl, R, seed=0):
    rng = np.random.default_rng(seed + R)
    base = words(rng, R)
    equal = np.tile(base, (Hl, 1))
    yield "all_equal", equal
    S = max(1, R // Hl)  # each view differs only in "its own" S records
    own = equal.copy()
    for v in range(Hl):
        lo = (v * S) % R
        own[v, lo:lo + S] -= U64(8)
    yield "own_records", own
    yield "random", words(rng, (Hl, R))
    edges = equal.copy()  # a differing slot at a block's first and last index, in every second view
    for v in range(0, Hl, 2):
        b = v % nblk_of(R)
        edges[v, b * BLOCK] -= U64(8)
        edges[v, min(R, (b + 1) * BLOCK) - 1] -= U64(8)
    yield "block_edges", edges
    raw = equal.copy()  # view 1 differs everywhere: it must go raw; the others stay coded
    raw[1 % Hl] -= U64(8)
    yield "one_raw", raw


@pytest.mark.parametrize("Hl,R", SIZES)
def test_round_trip_and_size(Hl, R):
    for name, v in cases(Hl, R):
        data = encode_views(v)
        assert len(data) == view_section_bytes(v), name
        assert np.array_equal(decode_views(data, Hl, R), v), name


@pytest.mark.parametrize("Hl,R", SIZES)
def test_size_formula(Hl, R):
    c = dict(cases(Hl, R))
    rec0 = 8 * (1 + pw_of(R))
    # all equal: base and one empty record per view
    assert len(encode_views(c["all_equal"])) == 8 * R + Hl * rec0
    # one raw view: 8 + 8 R for it
    coded = 1 + pw_of(R) + 8 * nblk_of(R) + R
    assert coded >= R
    assert len(encode_views(c["one_raw"])) == 8 * R + (Hl - 1) * rec0 + 8 * (1 + R)
    # block edges: every second view one present block, two literals (one where the block has one slot)
    n = 8 * R + (Hl // 2) * rec0
    for v in range(0, Hl, 2):
        b = v % nblk_of(R)
        lits = 1 if min(R, (b + 1) * BLOCK) - 1 == b * BLOCK else 2
        w = 1 + pw_of(R) + 8 + lits
        n += 8 * (1 + R) if w >= R else 8 * w
    assert len(encode_views(c["block_edges"])) == n


def test_raw_exactly_when_not_smaller():
    """A view goes raw exactly when its coded record would reach 8 R bytes."""
    R, Hl = 1536, 3
    rng = np.random.default_rng(1)
    base = words(rng, R)
    PW, nb = pw_of(R), nblk_of(R)
    for nl in (R - 1 - PW - 8 * nb - 1, R - 1 - PW - 8 * nb):  # coded = R - 1 words; coded = R words
        v = np.tile(base, (Hl, 1))
        v[2, :nl] -= U64(8)  # (nl > 2 * BLOCK: every block present)
        assert ckpt_ref.coded_words(v[2], base)[2] == 1 + PW + 8 * nb + nl
        data = encode_views(v)
        at = 8 * R + 2 * 8 * (1 + PW)
        first = int(np.frombuffer(data[at:at + 8], dtype="<u8")[0])
        assert (first == ckpt_ref.MAXU64) == (1 + PW + 8 * nb + nl >= R)
        assert np.array_equal(decode_views(data, Hl, R), v)


def test_decoder_rejects_bad_records():
    R, Hl = 770, 4
    v = dict(cases(Hl, R))["block_edges"]
    data = bytearray(encode_views(v))
    at = 8 * R  # view 0's n_lit
    data[at] += 1
    with pytest.raises(AssertionError):
        decode_views(bytes(data), Hl, R)


def test_checksum_properties():
    rng = np.random.default_rng(2)
    data = rng.integers(0, 256, size=1001, dtype=np.uint8).tobytes()
    s = ckpt_ref.checksum(data)
    for i in (0, 500, 1000):
        b = bytearray(data)
        b[i] ^= 0x40
        assert ckpt_ref.checksum(bytes(b)) != s
    assert ckpt_ref.checksum(data[:-1]) != s and ckpt_ref.checksum(data + b"\0") != s
    assert ckpt_ref.checksum(b"") == 0
