"""A numpy reader and writer of the checkpoint file's FIFO SECTION, written from include/gx_ckpt.h
alone: u32 n[Hl] zero-padded to 8 bytes, then each host's n[v] stored jobs of 16 bytes (u64 a, u32 c,
u32 meta) in queue order. The reference the engine's FIFO coder is checked against."""
import numpy as np

JOB = np.dtype([("a", "<u8"), ("c", "<u4"), ("meta", "<u4")])
assert JOB.itemsize == 16


def pad8(n):
    return (n + 7) & ~7


def encode(queues) -> bytes:
    """queues[v]: host v's stored jobs as (a, c, meta) tuples, in queue order."""
    n = np.array([len(q) for q in queues], dtype="<u4").tobytes()
    out = [n + b"\0" * (pad8(len(n)) - len(n))]
    for q in queues:
        out.append(np.array([tuple(j) for j in q], dtype=JOB).tobytes())
    return b"".join(out)


def stored_bytes(counts) -> int:
    return pad8(4 * len(counts)) + 16 * int(sum(counts))


def decode(data: bytes, Hl: int, Q: int, windows=None):
    """The queues of a section for Hl hosts with rings of Q jobs. windows: per host fifo_stored -
    fifo_head (mod 2^32) of the host states the file restores; a count that disagrees is refused."""
    tb = pad8(4 * Hl)
    assert len(data) >= tb, "short table"
    n = np.frombuffer(data[:4 * Hl], dtype="<u4")
    assert data[4 * Hl:tb] == b"\0" * (tb - 4 * Hl), "padding"
    assert (n <= Q).all(), "a count above Q"
    assert tb + 16 * int(n.sum(dtype=np.uint64)) == len(data), "table and jobs do not fill the section"
    if windows is not None:
        assert [int(x) for x in n] == [int(w) & 0xFFFFFFFF for w in windows], "a count disagrees with the host state"
    jobs = np.frombuffer(data[tb:], dtype=JOB)
    out, at = [], 0
    for k in n:
        out.append([(int(j["a"]), int(j["c"]), int(j["meta"])) for j in jobs[at:at + int(k)]])
        at += int(k)
    return out


def with_counts(data: bytes, Hl: int, counts) -> bytes:
    """The section with its count table replaced (the jobs stay): for the refusal tests."""
    n = np.array(counts, dtype="<u4").tobytes()
    assert len(counts) == Hl
    return n + b"\0" * (pad8(len(n)) - len(n)) + data[pad8(4 * Hl):]


def windows_of(hosts):
    return [(h.fifo_stored - h.fifo_head) & 0xFFFFFFFF for h in hosts]
