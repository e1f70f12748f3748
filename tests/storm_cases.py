"""The ExpireServer storm's contract (k_storm_p2 for S | 64, k_storm otherwise; DESIGN.md "Storm
contract"): sparse views written with gx_write_views, a numpy restatement of what one viewer's storm
does to them, and the parameter sets whose row lengths reach each seam of the kernels' pipeline.

Shared by tests/test_storm_model_cpu.py (the model and the guards against the oracle alone) and
tests/test_gpu_storm.py (the HIP engine against the oracle and the model)."""
import ctypes as C
import functools

import numpy as np

from sidecar_amd.abi import (ALIVE, DRAINING, INIT_OWN, INIT_WARM, JOB_EXPIRE, SLOT_ABSENT, TOMBSTONE, TS_SHIFT,
                             UNHEALTHY, Engine, GxJob, check, default_params)

M64 = (1 << 64) - 1
ST_DEPART = 11  # the departure stream of the engines' seeded generator (gx_oracle_fd.c)

# cell palette of build_views: what one viewer holds of one owner
(P_ABSENT, P_TOMB, P_ALIVE, P_SPARSE, P_FIRST, P_LAST, P_MIXED, P_SICK, P_PRETOMB) = range(9)
# about half the owners live: the two dead kinds weigh a quarter each
P_WEIGHT = np.array([0.25, 0.25] + [0.5 / 7] * 7)

SEAM_VIEWERS = 8      # per half: up to 6 seam viewers, then "no live owner", then "every owner live"
LISTENERS = ((20, 4096), (21, 7), (-20, 300), (-21, 1))  # (viewer: offset into the first / from the end of
#                                                           the second half, capacity): two per half


def other_half(H, v):
    """[lo, hi): the owners viewer v expires in the storm (ph_storm)."""
    half = H // 2
    return (half, H) if v < half else (0, half)


def is_p2(S):
    return S >= 2 and 64 % S == 0


def seam_positions(S, nw):
    """{seam name: word offsets p (0 < p < nw, owner-aligned) into a viewer's stretch} where the
    kernel's job ranks pass from one unit to the next. k_storm_p2: a wave's 128-word chunk, a block's
    512-word chunk, the 1024-word unit, the tile (1024 * GX_STORM_TM = 2048) and the PF * TW = 4096
    words in flight. k_storm: the tile of 1024 / S owners, and the 256th owner inside it (the second
    pass of the block-wide scan)."""
    if is_p2(S):
        return {m: np.arange(m, nw, m) for m in (128, 512, 1024, 2048, 4096) if m < nw}
    ot = 1024 // S
    tiles = np.arange(0, nw, ot * S)
    out = {"tile": tiles[1:]}
    if ot > 256:
        p = tiles + 256 * S
        out["scan256"] = p[p < nw]
    return out


def listener_views(H):
    return [(v if v >= 0 else H + v, cap) for v, cap in LISTENERS]


def _cells(rng, n, S, t0, tomb_now, kinds=None):
    """n owner cells of S words each, kinds drawn from the palette (or given)."""
    if kinds is None:
        kinds = rng.choice(len(P_WEIGHT), size=n, p=P_WEIGHT).astype(np.uint8)
    k = kinds[:, None]
    bits = rng.integers(0, 256, size=(n, S), dtype=np.uint8)
    some, dead, drain = (bits & 1).astype(bool), (bits & 2).astype(bool), (bits & 4).astype(bool)
    pick = rng.integers(0, S, size=n)
    pick = np.where(kinds == P_FIRST, 0, np.where(kinds == P_LAST, S - 1, pick))
    one = np.arange(S)[None, :] == pick[:, None]
    nxt = np.arange(S)[None, :] == ((pick + 1) % S)[:, None]
    # fresh timestamps, within a second before t0; the tombstones of P_MIXED older than its live records
    ts = t0 - 1 - rng.integers(0, 400_000_000, size=(n, S), dtype=np.int64)
    present = np.select([k == P_ABSENT, (k == P_TOMB) | (k == P_ALIVE) | (k == P_MIXED), k == P_PRETOMB],
                        [False, True, one | nxt], one | some)
    st = np.select([k == P_TOMB, k == P_ALIVE, (k == P_SPARSE) | (k == P_MIXED), k == P_SICK],
                   [TOMBSTONE, ALIVE, np.where(one | ~dead, ALIVE, TOMBSTONE),
                    np.where(one, np.where(drain, DRAINING, UNHEALTHY), TOMBSTONE)],
                   np.where(one, ALIVE, TOMBSTONE)).astype(np.int64)
    ts = np.where((k == P_MIXED) & (st == TOMBSTONE), ts - 500_000_000, ts)
    w = np.where(present, (ts << TS_SHIFT) | st, SLOT_ABSENT).astype(np.uint64)
    return np.where((k == P_PRETOMB) & nxt, np.uint64(tomb_now), w)


def build_views(engine, seed, storm_now):
    """The engine's current views with every viewer's other-half columns replaced: each (viewer,
    owner) cell a seeded draw from the palette, then per half the hand-made viewers (the first SEAM_VIEWERS
    of the half): one per seam of seam_positions whose only live owners are the last owner before and
    the first owner after every seam position, one with no live owner, one with every owner live."""
    H, S = engine.H, engine.S
    words = engine.read_views()
    t0 = engine.params.t0_ns - engine.epoch
    tomb_now = ((storm_now - engine.epoch) << TS_SHIFT) | TOMBSTONE
    rng = np.random.default_rng(seed)
    half = H // 2
    for v0, v1 in ((0, half), (half, H)):
        lo, hi = other_half(H, v0)
        no, nw = hi - lo, (hi - lo) * S
        n = (v1 - v0) * no  # the cells are drawn from a pool of 2^16 seeded ones (one gather fills the half)
        pool = _cells(rng, min(n, 1 << 16), S, t0, tomb_now)
        words[v0:v1, lo * S:hi * S] = pool[rng.integers(0, len(pool), size=n)].reshape(v1 - v0, nw)
        seams = list(seam_positions(S, nw).values())
        assert len(seams) + 2 <= SEAM_VIEWERS < v1 - v0
        fix = np.random.default_rng(1)  # the hand-made rows do not depend on the seed
        for i in range(len(seams) + 2):
            kinds = np.where(np.arange(no) % 3 == 0, P_TOMB, P_ABSENT).astype(np.uint8)  # no live owner
            live = np.arange(no) if i == len(seams) + 1 else np.array([], dtype=np.int64) if i == len(seams) \
                else np.unique(np.concatenate([seams[i] // S - 1, seams[i] // S]))
            kinds[live] = fix.integers(P_ALIVE, P_PRETOMB + 1, size=len(live))
            words[v0 + i, lo * S:hi * S] = _cells(fix, no, S, t0, tomb_now, kinds).reshape(nw)
    return words


def storm_model(views_before, H, S, v, storm_now, epoch):
    """expire_server (oracle/gx_oracle.c) for every owner of viewer v's other half, in vector form.
    Returns a dict: cols (the other-half words after), jobs [(mask, owner)] in owner order, calls
    (ServiceChanged calls), written (words that change), live (owners whose server times become
    storm_now), events [(owner, svc, storm_now, TOMBSTONE, previous status)] in owner, then service
    order."""
    lo, hi = other_half(H, v)
    w = np.asarray(views_before[v, lo * S:hi * S]).reshape(hi - lo, S)
    st = w & np.uint64(7)
    present = st != SLOT_ABSENT
    live = (present & (st != TOMBSTONE)).any(axis=1)
    tomb = np.uint64(((storm_now - epoch) << TS_SHIFT) | TOMBSTONE)
    hit = present & live[:, None]  # Tombstone() + ServiceChanged for every record of a live owner
    mask = (present.astype(np.uint64) << np.arange(S, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    owners = lo + np.nonzero(live)[0]
    o, s = np.nonzero(hit)
    ev = np.stack([lo + o, s, np.full(len(o), storm_now), np.full(len(o), TOMBSTONE), st[o, s].astype(np.int64)], axis=1)
    return dict(cols=np.where(hit, tomb, w).reshape(-1), jobs=np.stack([mask[live], owners.astype(np.uint64)], axis=1),
                calls=int(hit.sum()), written=int((hit & (w != tomb)).sum()), live=owners, events=ev.astype(np.int64))


# ------------------------------------------------------------------------------------ cases --
def _case(S, H, min_nw, reaches, storm_round=1, listeners=False, seed=1, **kw):
    p = dict(n_hosts=H, n_services=S, init_mode=INIT_WARM, lock_model=0, storm_round=storm_round,
             partition_start=0, partition_end=storm_round + 6, ae_period_rounds=10,
             ae_phase=(storm_round + 6) % 10, queue_cap=H // 2 + 257)
    p.update(kw)
    half = H // 2
    return dict(S=S, H=H, nw=(half * S, (H - half) * S), min_nw=min_nw, reaches=reaches, params=p,
                storm_round=storm_round, listeners=listeners, seed=seed)


THREE = "both refills, third outer pass, q[] reuse"
CASES = {
    "s2_refill": _case(2, 4102, 4096, "first refill, 2nd outer pass, LPO 1"),
    "s4_refill": _case(4, 2054, 4096, "first refill, 2nd outer pass, LPO 2"),
    "s8_three": _case(8, 2054, 8192, THREE, listeners=True),
    "s16_three": _case(16, 1030, 8192, THREE + "; the headline's S", listeners=True),
    "s32_three": _case(32, 518, 8192, THREE + "; S = 32", listeners=True),
    "s64_three": _case(64, 262, 8192, THREE + "; LPO 32 / omask, 64-bit masks", listeners=True),
    "s16_odd": _case(16, 1031, 8192, "odd H: the halves differ in length"),
    "s16_wrap": _case(16, 300, 2048, "ring wrap, room < jobs, deferred counts", storm_round=8, queue_cap=24),
    "s8_lock": _case(8, 1100, 4096, "lock_model 1: locked viewers defer; pexp bits with lo, hi not multiples of 32",
                     storm_round=12, lock_model=1, init_mode=INIT_OWN, alive_interval_rounds=2,
                     tombstone_interval_rounds=3, churn_ppm=100000, ae_period_rounds=5, ae_phase=0,
                     partition_start=0, partition_end=0, queue_cap=2048),
    "s16_depart": _case(16, 600, 4096, "departed viewers skipped", depart_round=0, depart_ppm=150000),
    "s3_generic": _case(3, 1400, 2048, "k_storm: LDS masks over more than two tiles, 341 owners per tile + remainder",
                        listeners=True),
    "s12_generic": _case(12, 360, 2048, "k_storm: 85 owners per tile + remainder", listeners=True),
}
# (case, with listeners): every case without (EV = false); the "three" and generic ones again with
RUNS = [(n, ev) for n, c in CASES.items() for ev in ((False, True) if c["listeners"] else (False,))]


def run_id(run):
    return run[0] + ("-ev" if run[1] else "")


# ------------------------------------------------------------------------------ the harness --
def mix64(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def departed(p, v):
    """departed_at (gx_oracle_fd.c) at any round >= depart_round."""
    if p.depart_round < 0 or not p.depart_ppm:
        return False
    h = mix64(p.seed ^ ((ST_DEPART * 0xD1B54A32D192ED03) & M64))
    for x in (v, 0, 0):
        h = mix64(h ^ x)
    return (h % 1000000) & 0xFFFFFFFF < p.depart_ppm


JOB_DT = np.dtype([("a", "<u8"), ("c", "<u4"), ("meta", "<u4")])


def queue_array(e, v):
    """queue(v) as a structured array (a, c, meta)."""
    n = C.c_uint32()
    check(e.lib.gx_read_queue(e.h, v, None, 0, C.byref(n)))
    out = (GxJob * max(1, n.value))()
    check(e.lib.gx_read_queue(e.h, v, out, n.value, C.byref(n)))
    return np.frombuffer(out, dtype=JOB_DT, count=n.value).copy()


def make_engine(lib, name, **extra):
    return Engine(default_params(lib, **dict(CASES[name]["params"], **extra)), lib=lib)


def storm_now(e, case):
    return e.params.t0_ns + case["storm_round"] * e.params.round_ns


@functools.lru_cache(maxsize=1)
def case_views(name):
    """The case's views at its storm round, built once on the oracle (the warm rounds before the
    storm included) and shared, unchanged, by every test of the case."""
    from tests.oracle_lib import load_oracle
    case = CASES[name]
    o = make_engine(load_oracle(omp=True), name)
    o.run_rounds(case["storm_round"])
    words = build_views(o, case["seed"], storm_now(o, case))
    words.setflags(write=False)
    o.close()
    return words


def add_listeners(e):
    for v, cap in listener_views(e.H):
        e.add_listener(v, 1, cap)


def before_state(e):
    """What the checks need of the engine before the storm round's round_send()."""
    r = e.round
    hosts = e.hosts()
    lm = e.params.lock_model
    return dict(round=r, stats=e.stats(), locked=np.array([bool(lm and h.locked_at(r)) for h in hosts]),
                head=np.array([h.fifo_head for h in hosts], dtype=np.int64),
                departed=np.array([departed(e.params, v) for v in range(e.H)]),
                times=np.stack([e.server_times(v) for v in range(e.H)]))


def check_against_model(e, name, words, before, viewers=None, events=None):
    """The model's statements (storm_model) on engine e after the storm round's round_send():
    views, server times, counters for every viewer; the queued EXPIRE jobs for `viewers` (all when
    None); the drained listener events in `events` {viewer: [tup]}. Returns the per-viewer figures
    the guards read."""
    case = CASES[name]
    H, S, p = e.H, e.S, e.params
    now = storm_now(e, case)
    tomb_round = case["storm_round"]
    after = e.read_views()
    hosts = e.hosts()
    st0, st1 = before["stats"], e.stats()
    runs = ~before["locked"] & ~before["departed"]
    n_jobs = np.zeros(H, dtype=np.int64)
    calls = 0
    deferred = 0
    fig = dict(jobs=n_jobs, runs=runs, tail0=np.zeros(H, dtype=np.int64), room=np.zeros(H, dtype=np.int64),
               live=[None] * H, models={})
    burst = p.fanout * max(1, p.gossip_messages)  # GetBroadcasts calls of the round's sends
    for v in range(H):
        lo, hi = other_half(H, v)
        m = storm_model(words, H, S, v, now, e.epoch)
        got = after[v, lo * S:hi * S]
        times = e.server_times(v, lo, hi)
        if not runs[v]:
            deferred += (hi - lo) if before["locked"][v] else 0
            assert np.array_equal(got, words[v, lo * S:hi * S]), f"{name}: viewer {v} did not run, its row changed"
            assert np.array_equal(times, before["times"][v, lo:hi]), f"{name}: viewer {v} server times"
            continue
        fig["live"][v] = m["live"]
        n_jobs[v] = len(m["jobs"])
        calls += m["calls"]
        bad = np.nonzero(got != m["cols"])[0]
        assert not len(bad), f"{name}: viewer {v} other-half words differ from the model at {bad[:5].tolist()}"
        want_t = before["times"][v, lo:hi].copy()
        want_t[m["live"] - lo] = now
        assert np.array_equal(times, want_t), f"{name}: viewer {v} server times differ from the model"
        if viewers is None or v in viewers or (events and v in events):
            fig["models"][v] = m
        if viewers is not None and v not in viewers:
            continue
        # the stored EXPIRE jobs of this round: the model's jobs [a, b), b cut where the ring was full
        # (the rest keep their place and lose their contents), a <= the sends' dequeues
        h = hosts[v]
        n = len(m["jobs"])
        tail0 = h.fifo_tail - n  # nothing is pushed behind the storm's jobs in the same round_send()
        room = max(p.queue_cap - (tail0 - int(before["head"][v])), 0) if h.fifo_stored >= tail0 else 0
        b = min(n, room)
        fig["tail0"][v], fig["room"][v] = tail0, room
        if room and h.fifo_head <= tail0 + b:
            assert h.fifo_stored == tail0 + b, f"{name}: viewer {v} stored {h.fifo_stored - tail0} of {n} jobs, room {room}"
        q = queue_array(e, v)
        q = q[((q["meta"] & 7) == JOB_EXPIRE) & (q["c"] == tomb_round)]
        a = b - len(q)
        assert 0 <= a <= burst, f"{name}: viewer {v} holds {len(q)} EXPIRE jobs, stored {b} of {n}"
        meta = JOB_EXPIRE | (p.tombstone_count << 9) | (m["jobs"][a:b, 1].astype(np.uint32) << 15)
        assert np.array_equal(q["a"], m["jobs"][a:b, 0]), f"{name}: viewer {v} job masks differ from the model"
        assert np.array_equal(q["meta"], meta.astype(np.uint32)), f"{name}: viewer {v} job owners differ from the model"
    assert st1["expire_server"] - st0["expire_server"] == n_jobs.sum(), name
    assert st1["expire_deferred"] - st0["expire_deferred"] == deferred, name
    fig["calls"], fig["deferred"] = calls, deferred
    for v, evs in (events or {}).items():
        cap = dict(listener_views(H))[v]
        lo, hi = other_half(H, v)
        k = next((i for i, t in enumerate(evs) if lo <= t[0] < hi), len(evs))  # the owner phase's own events first
        want = fig["models"][v]["events"] if runs[v] else np.zeros((0, 5), dtype=np.int64)
        assert len(evs) == min(cap, k + len(want)), f"{name}: listener of {v} drained {len(evs)} events"
        tail = np.array([t[:5] for t in evs[k:]], dtype=np.int64).reshape(-1, 5)
        assert np.array_equal(tail, want[:len(tail)]), f"{name}: listener of {v} events differ from the model"
        assert all(t[5] == now for t in evs[k:]), f"{name}: listener of {v} event times"
    return fig


# The receive phase's counters of the packets a round_send() gathered: the HIP engine's senders count
# them (k_send filters each record against the receiver's slot), the oracle's receivers do in
# round_merge(). Between the two calls they are the only state that may differ; from round_end() on
# parity.assert_same compares them like every other counter.
RECEIVE_COUNTERS = ("gossip_merges", "stale_drops", "locked_merges", "first_locked_round")


def assert_same_after_send(g, o, what):
    """parity.assert_same between round_send() and round_merge()."""
    from tests.parity import _dict_diff, snapshot
    sa, sb = snapshot(g), snapshot(o)
    for s in (sa, sb):
        for k in RECEIVE_COUNTERS:
            del s["stats"][k]
    assert sa["stats"] == sb["stats"], f"{what}: stats differ\n{_dict_diff(sa['stats'], sb['stats'])}"
    assert sa["hosts"] == sb["hosts"], f"{what}: host states differ"
    for k in ("views", "digests", "last_changed", "times"):
        bad = np.argwhere(sa[k] != sb[k])
        assert not len(bad), f"{what}: {len(bad)} {k} differ, first {bad[:5].tolist()}"


def drain_all(e):
    return {v: [x.tup() for x in e.drain_listener(v, 1, 8192)] for v, _ in listener_views(e.H)}
