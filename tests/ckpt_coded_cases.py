"""The schedules of the coded-checkpoint tests (include/gx_ckpt.h gx_ckpt_save_coded: ROW CODING of
the server times, FIFO SECTION). They were picked with the oracle so that the saved states hold every
shape the two coders meet (tests/test_ckpt_coded_cases_cpu.py checks it on the CPU):
  FIFO windows  empty, partial, full (n = Q), wrapped round the ring's end, with deferred jobs behind
                the stored window
  server times  rows stored raw, rows coded with literals, rows equal to base; W = 2 H of one full
                block (512), two blocks with a ragged last one (514), far below a block (8, 66, 128)"""
import numpy as np

from sidecar_amd.abi import INIT_OWN, INIT_WARM, Engine, default_params
from tests import ckpt_ref

CASES = {
    # Q = 8 is below k_send's head prefetch; Hl = 33: the count table needs its padding
    "q8": dict(n_hosts=33, n_services=3, init_mode=INIT_OWN, churn_ppm=100000, alive_interval_rounds=2,
               tombstone_interval_rounds=7, ae_period_rounds=5, queue_cap=8, storm_round=5, fanout=1, packet_cap=1),
    "q16": dict(n_hosts=64, n_services=8, init_mode=INIT_OWN, churn_ppm=50000, alive_interval_rounds=2,
                tombstone_interval_rounds=7, ae_period_rounds=5, queue_cap=16, storm_round=5),
    # W = 514: two blocks, the last with 2 slots
    "warm257": dict(n_hosts=257, n_services=1, init_mode=INIT_WARM, churn_ppm=50000, ae_period_rounds=5, queue_cap=32),
    # W = 512: exactly one full block
    "warm256": dict(n_hosts=256, n_services=2, init_mode=INIT_WARM, churn_ppm=20000, ae_period_rounds=5, queue_cap=32),
    # W = 8
    "h4": dict(n_hosts=4, n_services=1, init_mode=INIT_WARM, churn_ppm=200000, queue_cap=8),
}
# (case, saved round) of the continuity runs
SAVES = [("q8", 6), ("q8", 12), ("q16", 6), ("warm257", 20), ("warm257", 40), ("warm256", 12), ("h4", 6)]
FIFO_SHAPES = ("empty", "partial", "full", "wrapped", "deferred")


def engine(lib, name, **kw):
    return Engine(default_params(lib, **dict(CASES[name], **kw)), lib=lib)


def srvt_table(e, stored=False) -> np.ndarray:
    """The engine's server times as a table of u64 [Hl][2 H]: as gx_read_server_times returns them
    (absolute), or, stored, as the engine keeps them and the file holds them: relative to gx_epoch,
    0 staying 0 (time.Unix(0, 0))."""
    t = np.stack([e.server_times(v).reshape(-1) for v in range(e.lo, e.hi)])
    if stored:
        t = np.where(t != 0, t - np.int64(e.epoch), 0).astype(np.int64)
    return t.view(np.uint64)


def queues(e):
    """Every held host's stored jobs as (a, c, meta) tuples, in queue order."""
    return [[(j.a, j.c, j.meta) for j in e.queue(v)] for v in range(e.lo, e.hi)]


def fifo_shapes(e):
    """Of FIFO_SHAPES, how many of the engine's hosts have each."""
    Q = e.params.queue_cap
    n = dict.fromkeys(FIFO_SHAPES, 0)
    for h in e.hosts():
        k = (h.fifo_stored - h.fifo_head) & 0xFFFFFFFF
        n["empty"] += k == 0
        n["partial"] += 0 < k < Q
        n["full"] += k == Q
        n["wrapped"] += k > 0 and h.fifo_head % Q + k > Q
        n["deferred"] += h.fifo_tail != h.fifo_stored
    return n


def srvt_rows(table: np.ndarray):
    """(rows stored raw, rows coded with literals, rows equal to base, literals of the coded rows)."""
    base = table.max(axis=0)
    raw = coded = equal = lits = 0
    for row in table:
        _, nl, words = ckpt_ref.coded_words(row, base)
        if words >= row.size:
            raw += 1
        elif nl:
            coded += 1
            lits += nl
        else:
            equal += 1
    return raw, coded, equal, lits
