"""Spread latencies from a record watch's log (include/gx_watch.h; Engine.watch_read,
ShardRounds.watch_read), and the owners' current versions of watched keys.

A watch entry names a record and a version (a threshold on Updated). The log holds, per round and
entry, how many live views hold the version (`holds`) and how many hold an older one (`older`),
and per round the live views counted (`live`). A version has reached every view at the end of the
first round with holds == live; no view is left behind on an older one at the first with older == 0
(views that hold no record of the key at all are not behind).
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from .abi import ABSENT, TS_SHIFT


def spread_rounds(counts, live, first_round: int, born_round) -> Tuple[List[Optional[int]], List[Optional[int]]]:
    """counts [rounds, n, 2] (holds, older), live [rounds]: log rows of rounds first_round,
    first_round + 1, ...; born_round: per entry (or one for all), the round the version was stamped
    in. Returns (full, clean), per entry the rounds from born_round to the first logged round, not
    before born_round, at whose end holds == live (full) and older == 0 (clean): 0 when the round
    the version was born in already ends that way, None where the log never shows it. The
    definition is bench.py's `dissemination` latency. Rows without live views (rounds jumped over by
    gx_set_round) show nothing."""
    counts = np.asarray(counts)
    live = np.asarray(live)
    rounds, n = counts.shape[0], counts.shape[1]
    born = np.broadcast_to(np.asarray(born_round, dtype=np.int64), (n,))
    rnd = first_round + np.arange(rounds, dtype=np.int64)
    seen = (rnd[:, None] >= born[None, :]) & (live[:, None] > 0)
    out = []
    for ok in (counts[:, :, 0] == live[:, None], counts[:, :, 1] == 0):
        ok = ok & seen
        first = ok.argmax(axis=0) if rounds else np.zeros(n, dtype=np.int64)
        hit = ok.any(axis=0) if rounds else np.zeros(n, dtype=bool)
        out.append([int(rnd[first[i]] - born[i]) if hit[i] else None for i in range(n)])
    return out[0], out[1]


def owner_versions(cluster, keys: Sequence[int]) -> np.ndarray:
    """The Updated (absolute ns) each watched key's owner holds now, from the owner's own view:
    int64 [len(keys)], -1 where the owner holds no record. `cluster` is an Engine, or a ShardRounds
    whose process holds every key's owning shard: each key is read from the shard that owns it."""
    engines = getattr(cluster, "engines", None) or [cluster]
    S = engines[0].S
    out = np.full(len(keys), -1, dtype=np.int64)
    rows = {}  # owner -> its own view's words
    for i, key in enumerate(keys):
        o = int(key) // S
        if o not in rows:
            e = next(x for x in engines if x.lo <= o < x.hi)
            rows[o] = (e, e.read_views(o, o + 1)[0])
        e, row = rows[o]
        w = int(row[int(key)])
        if w & 7 != ABSENT:
            out[i] = (w >> TS_SHIFT) + e.epoch
    return out
