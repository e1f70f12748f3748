"""A numpy reader and writer of the checkpoint file, written from include/gx_ckpt.h alone (FILE and
VIEW SECTION): the reference the engine's view coder and file writer are checked against."""
import struct

import numpy as np

MAGIC = 0x31304B4358474B43
FORMAT = 1
HEADER_BYTES = 40
RAW, VIEWS = 0, 1
CK_VIEW = 1
BLOCK = 512
U64 = np.uint64
MAXU64 = (1 << 64) - 1


def pad8(n):
    return (n + 7) & ~7


def checksum(data: bytes) -> int:
    n = len(data)
    w = np.frombuffer(data + b"\0" * (pad8(n) - n), dtype="<u8")
    with np.errstate(over="ignore"):
        m = w ^ (np.arange(1, w.size + 1, dtype=U64) * U64(0x9E3779B97F4A7C15))
        m ^= m >> U64(32)
        m *= U64(0xD6E8FEB86659FD93)
        m ^= m >> U64(32)
        s = int(m.sum(dtype=U64)) if w.size else 0
    return s ^ n


def nblk_of(R):
    return (R + BLOCK - 1) // BLOCK


def pw_of(R):
    return (nblk_of(R) + 63) // 64


def coded_words(row: np.ndarray, base: np.ndarray):
    """(present blocks, literals, words of the coded record) of one view."""
    ne = row != base
    nl = int(ne.sum())
    R = row.size
    padded = np.zeros(nblk_of(R) * BLOCK, dtype=bool)
    padded[:R] = ne
    np_ = int(padded.reshape(-1, BLOCK).any(axis=1).sum())
    return np_, nl, 1 + pw_of(R) + 8 * np_ + nl


def _bits_to_words(bits: np.ndarray) -> np.ndarray:
    """bool[64 k] -> k u64 words, bit i of word j = bits[64 j + i]."""
    b = bits.reshape(-1, 64).astype(U64)
    return (b << np.arange(64, dtype=U64)).sum(axis=1, dtype=U64)


def encode_views(views: np.ndarray) -> bytes:
    """The view section of views[Hl][R] (uint64)."""
    views = np.ascontiguousarray(views, dtype=U64)
    Hl, R = views.shape
    nblk, PW = nblk_of(R), pw_of(R)
    base = views.max(axis=0)
    out = [base.astype("<u8").tobytes()]
    for row in views:
        np_, nl, words = coded_words(row, base)
        if words >= R:
            out.append(struct.pack("<Q", MAXU64) + row.astype("<u8").tobytes())
            continue
        ne = np.zeros(nblk * BLOCK, dtype=bool)
        ne[:R] = row != base
        blocks = ne.reshape(nblk, BLOCK)
        present = np.zeros(PW * 64, dtype=bool)
        present[:nblk] = blocks.any(axis=1)
        rec = [np.array([nl], dtype=U64), _bits_to_words(present)]
        for b in np.nonzero(present[:nblk])[0]:
            rec.append(_bits_to_words(blocks[b]))
        rec.append(row[ne[:R]])
        rec = np.concatenate(rec).astype("<u8")
        assert rec.size == words
        out.append(rec.tobytes())
    return b"".join(out)


def view_section_bytes(views: np.ndarray) -> int:
    """The stored size by the formula of gx_ckpt.h, without encoding."""
    views = np.asarray(views, dtype=U64)
    Hl, R = views.shape
    base = views.max(axis=0)
    n = 8 * R
    for row in views:
        words = coded_words(row, base)[2]
        n += 8 * (1 + R) if words >= R else 8 * words
    return n


def decode_views(data: bytes, Hl: int, R: int) -> np.ndarray:
    w = np.frombuffer(data, dtype="<u8")
    nblk, PW = nblk_of(R), pw_of(R)
    base = w[:R]
    at = R
    out = np.empty((Hl, R), dtype=U64)
    for v in range(Hl):
        nl = int(w[at])
        if nl == MAXU64:
            out[v] = w[at + 1:at + 1 + R]
            at += 1 + R
            continue
        present = np.unpackbits(w[at + 1:at + 1 + PW].view(np.uint8), bitorder="little").astype(bool)
        assert not present[nblk:].any(), "present bits past the last block"
        pb = np.nonzero(present[:nblk])[0]
        masks = w[at + 1 + PW:at + 1 + PW + 8 * pb.size]
        ne = np.zeros(nblk * BLOCK, dtype=bool)
        if pb.size:
            mb = np.unpackbits(masks.view(np.uint8), bitorder="little").astype(bool).reshape(pb.size, BLOCK)
            assert mb.any(axis=1).all(), "a present block without a differing slot"
            ne.reshape(nblk, BLOCK)[pb] = mb
        assert not ne[R:].any(), "mask bits past R"
        assert int(ne.sum()) == nl, "n_lit disagrees with the masks"
        lit = w[at + 1 + PW + 8 * pb.size:at + 1 + PW + 8 * pb.size + nl]
        row = base.copy()
        row[ne[:R]] = lit
        out[v] = row
        at += 1 + PW + 8 * pb.size + nl
    assert at == w.size, "the records do not fill the section"
    return out


class CkptFile:
    """A parsed checkpoint: params (raw bytes), round, sections {id: (coding, raw_bytes, stored bytes)}."""

    def __init__(self, params: bytes, round_: int, sections):
        self.params, self.round, self.sections = params, round_, dict(sections)

    @classmethod
    def read(cls, path, verify=True):
        data = open(path, "rb").read()
        magic, fmt, abi, psz, nsec, round_, hsum = struct.unpack_from("<QIIIIqQ", data, 0)
        assert magic == MAGIC and fmt == FORMAT
        tab = HEADER_BYTES + pad8(psz)
        hb = tab + 32 * nsec
        if verify:
            head = bytearray(data[:hb])
            head[32:40] = b"\0" * 8
            assert checksum(bytes(head)) == hsum, "header checksum"
        f = cls(data[HEADER_BYTES:HEADER_BYTES + psz], round_, {})
        f.abi = abi
        f.offsets = {}  # id -> where the section's stored bytes begin in the file
        at = hb
        for i in range(nsec):
            sid, coding, raw, stored, ssum = struct.unpack_from("<IIQQQ", data, tab + 32 * i)
            body = data[at:at + stored]
            assert len(body) == stored, "short file"
            if verify:
                assert checksum(body) == ssum, f"section {sid} checksum"
            f.sections[sid] = (coding, raw, body)
            f.offsets[sid] = at
            at += pad8(stored)
        assert at == len(data)
        return f

    def write(self, path):
        ids = sorted(self.sections)
        head = bytearray(struct.pack("<QIIIIqQ", MAGIC, FORMAT, self.abi, len(self.params), len(ids), self.round, 0))
        head += self.params + b"\0" * (pad8(len(self.params)) - len(self.params))
        body = bytearray()
        for sid in ids:
            coding, raw, stored = self.sections[sid]
            head += struct.pack("<IIQQQ", sid, coding, raw, len(stored), checksum(stored))
            body += stored + b"\0" * (pad8(len(stored)) - len(stored))
        head[32:40] = struct.pack("<Q", checksum(bytes(head)))
        with open(path, "wb") as f:
            f.write(head + body)
