"""Reference for the record watch (include/gx_watch.h), shared by tests/test_watch_ref_cpu.py and the
GPU watch tests: an unsharded oracle engine runs in lockstep with the engine under test, and after
every round its views (read_view of every host) and, with the failure detector, its departures
(fd_hosts) give the expected holds, older and live in numpy. Nothing here calls the watch.

Also the schedules and watch entries of those tests. The first two schedules are
tests/lock_pool_cases.BASE with one change each and a seed; a watch is armed after ARM rounds and
logs ROUNDS[name] more. Seeds and rounds are the first tried (seeds 0x5EED, 1, 2, 3; rounds in steps
of 5) with which the oracle alone shows what tests/test_watch_ref_cpu.py asks for: BASE's contended
lock lets a version reach every view only after 50 to 150 rounds.
"""
import numpy as np

from sidecar_amd.abi import ABSENT, INIT_OWN, WATCH_ANY, WATCH_OFF
from tests.lock_pool_cases import BASE

ARM = 5
ROUNDS = {"odd_rows": 80, "storm": 125, "fd": 40}

SCHEDULES = {
    # R = 99: odd rows (the scalar row paths), 70 entries: past one wave, not a multiple of 64
    "odd_rows": dict(BASE, n_hosts=33, n_services=3, seed=2),
    # BASE itself: the ExpireServer storm in the first watched round
    "storm": dict(BASE, seed=3),
    # departures inside the window, found by the failure detector: a tests/fd_cases.py schedule from
    # empty views (INIT_OWN), without the lock model (with it no version reaches 64 views in 40 rounds)
    "fd": dict(n_hosts=64, n_services=8, init_mode=INIT_OWN, fd_enable=1, depart_round=12, depart_ppm=100000,
               ae_period_rounds=10, queue_cap=4096, churn_ppm=20000, lock_model=0),
}


class OracleWatch:
    """The expected log of a watch of n entries over the unsharded oracle engine `orc`: entries are
    set like the watch's, run_round() runs one oracle round and appends its row."""

    def __init__(self, orc, n):
        self.orc = orc
        self.keys = np.full(n, WATCH_OFF, dtype=np.uint32)
        self.thr = np.zeros(n, dtype=np.int64)
        self.first_round = orc.round
        self.counts, self.live, self.views = [], [], []

    def set(self, first, keys, thr):
        self.keys[first:first + len(keys)] = keys
        self.thr[first:first + len(thr)] = thr

    def _live(self):
        """Hosts that have not departed in the oracle's current round."""
        o = self.orc
        if not o.params.fd_enable:
            assert o.params.depart_round < 0 or not o.params.depart_ppm
            return np.ones(o.H, dtype=bool)
        return np.array([not h.departed for h in o.fd_hosts()])

    def run_round(self):
        o = self.orc
        live = self._live()  # by the round that ends, before the round number moves
        o.run_rounds(1)
        got = [o.read_view(v) for v in range(o.H)]
        ts = np.stack([g[0] for g in got])
        st = np.stack([g[1] for g in got])
        self.views.append((ts, st, live))
        self.counts.append(counts_of(ts, st, live, self.keys, self.thr))
        self.live.append(int(live.sum()))

    def run(self, n):
        for _ in range(n):
            self.run_round()

    def log(self):
        """(counts uint32 [rounds, n, 2], live uint32 [rounds])"""
        return np.stack(self.counts).astype(np.uint32), np.array(self.live, dtype=np.uint32)


def counts_of(ts, st, live, keys, thr):
    """[n, 2] holds and older of every entry over the live views of ts, st [H, R]."""
    out = np.zeros((len(keys), 2), dtype=np.int64)
    rows = np.flatnonzero(live)
    for i, (k, t) in enumerate(zip(keys, thr)):
        if k == WATCH_OFF:
            continue
        present = st[rows, k] != ABSENT
        held = ts[rows, k] >= t  # (WATCH_ANY is INT64_MIN: every present slot)
        out[i] = ((present & held).sum(), (present & ~held).sum())
    return out


def owner_version(orc, key):
    """Updated of `key` in its owner's own view (WATCH_ANY if the owner holds none)."""
    ts, st = orc.read_view(int(key) // orc.S)
    return int(ts[key]) if st[key] != ABSENT else WATCH_ANY


def entries(name, orc):
    """The watch entries of schedule `name`, from the oracle as it stands at the arm round:
    (keys uint32 [n], thresholds int64 [n])."""
    R, S = orc.H * orc.S, orc.S
    if name == "odd_rows":
        keys = [7 * S, 7 * S + 1, 7 * S + 2,  # all three records of owner 7
                7 * S,                       # a duplicate key, with another threshold
                WATCH_OFF, 50, 51] + [(7 * i + 3) % R for i in range(7, 70)]
        thr = [owner_version(orc, k) if k != WATCH_OFF else 0 for k in keys]
        thr[3] = thr[0] + 1              # the version after the one entry 0 watches
        thr[5] = WATCH_ANY
        thr[6] = orc.now() + 10 ** 12    # a version nobody holds inside the test: every present slot is older
    elif name == "storm":
        keys = list(range(R))
        # even keys: the storm's tombstones (Updated = the storm round's now) and everything later;
        # odd keys: the owners' versions at the arm round
        storm_now = orc.params.t0_ns + orc.params.storm_round * orc.params.round_ns
        thr = [storm_now if k % 2 == 0 else owner_version(orc, k) for k in keys]
    elif name == "fd":
        keys = [(5 * i + 1) % R for i in range(100)]
        thr = [owner_version(orc, k) for k in keys]
        thr[::10] = [t + 1 if t != WATCH_ANY else t for t in thr[::10]]  # the owners' next versions
    else:
        raise KeyError(name)
    return np.array(keys, dtype=np.uint32), np.array(thr, dtype=np.int64)


def spread_direct(views, keys, thr, first_round, born_round):
    """Per entry, rounds from born_round until every live view holds the version / none holds an
    older one, straight from the per-round oracle views (OracleWatch.views); None: never."""
    full, clean = [], []
    for k, t in zip(keys, thr):
        f = c = None
        for j, (ts, st, live) in enumerate(views):
            rnd = first_round + j
            if rnd < born_round or not live.any():
                continue
            if k == WATCH_OFF:
                hold = old = np.zeros(int(live.sum()), dtype=bool)
            else:
                present = st[live, k] != ABSENT
                hold = present & (ts[live, k] >= t)
                old = present & (ts[live, k] < t)
            if f is None and hold.all():
                f = rnd - born_round
            if c is None and not old.any():
                c = rnd - born_round
        full.append(f)
        clean.append(c)
    return full, clean
