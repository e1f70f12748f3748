"""The push-pull contract (ae_pair in gx_kernels.hpp, behind k_ae, k_ae_ev, k_ae_chunk, k_merge_views and
the k_ae_plan kernels; DESIGN.md "Push-pull contract"): views written with gx_write_views between the
push-pull round's round_merge() and ae_merge(), a numpy restatement of what one exchange does to its
two rows, and the parameter sets whose row lengths and pair counts reach each seam of the kernel.

Every pair of the round's matching gets two rows drawn from a seeded pool: a common base row (about
1/4 absent, 1/2 fresh, 1/8 stale) with seeded edits on each side at a density of 0.1 %, 2 %, 30 % or
100 % of the slots. The first pairs of the round, in pair order, are hand-made (HAND).

Shared by tests/test_ae_model_cpu.py (the model and the guards, on the oracle alone) and
tests/test_gpu_ae.py (the HIP engine against the oracle and the model)."""
import functools

import numpy as np

from sidecar_amd.abi import (ABSENT, ALIVE, DRAINING, INIT_OWN, INIT_WARM, JOB_RETX, SLOT_ABSENT, TOMBSTONE,
                             TS_SHIFT, UNHEALTHY, UNKNOWN, Engine, default_params)
from sidecar_amd.dist import LocalShards
from tests.storm_cases import departed, queue_array
from tests.test_wire_format import BLK, ae_pairs, digest, leads, own_ok

TILE, WAVE = 1024, 128                # ae_pair's slot geometry: 256 threads x 4 slots, two 512-slot halves
SEAMS = (128, 512, 1024, 2048)        # wave, half tile, tile, two tiles in flight (PF = 2)
STATUSES = np.array([ALIVE, TOMBSTONE, UNHEALTHY, DRAINING], dtype=np.uint64)
DENSITIES = (0.001, 0.02, 0.3, 1.0)
N_BASE, N_EDIT = 6, 6                 # pool: base rows x densities x edited variants
RETX_META = JOB_RETX | (1 << 9)       # gx.h gx_job meta: kind | pass << 3 | n_passes << 9 | owner << 15
LISTENER_CAPS = (4096, 7, 1)
U = np.uint64

# hand-made pairs, in pair order
HAND = ("seam128", "seam512", "seam1024", "seam2048", "same", "insert_all", "odd_keys", "even_keys",
        "last_is_older", "last_keeps_status", "own_records")
# hand-made cross pairs of the sharded cases: the first cross pairs in pair order
CROSS_HAND = ("block1", "tile_orders", "edge_literals", "tail_block", "lead_both", "same")


def pack(ts, st):
    return (np.asarray(ts).astype(U) << U(TS_SHIFT)) | np.asarray(st).astype(U)


def ts_of(w):
    return (w >> U(TS_SHIFT)).astype(np.int64)


def st_of(w):
    return (w & U(7)).astype(np.int64)


def stale_cut(now, p):
    """Slot time below which a record IsStale (add_entry)."""
    return now - p.tombstone_lifespan_ns - p.stale_fudge_ns


# ------------------------------------------------------------------------------------ the model --
def _merge(old, inc, v, S, cut):
    """x.Merge(inc) on row `old` of host v: add_entry(..., SRC_AE) for every present word of `inc` in
    key order, in vector form (no key is touched twice, so the order only shows in what is 'last')."""
    so, si = st_of(old), st_of(inc)
    to, ti = ts_of(old), ts_of(inc)
    pres = si != ABSENT
    stale = pres & (ti < cut)
    live = pres & ~stale
    ins = live & (so == ABSENT)
    newer = live & (so != ABSENT) & (ti > to)
    acc = ins | newer
    st_new = np.where(newer & (so == DRAINING) & (si == ALIVE), DRAINING, si)
    row = np.where(acc, pack(ti, st_new), old)
    chg = ins | (newer & (so != st_new))
    keys = np.nonzero(acc)[0]
    ckeys = np.nonzero(chg)[0]
    H = len(old) // S
    lu, lc = np.full(H, -1, dtype=np.int64), np.full(H, -1, dtype=np.int64)
    np.maximum.at(lu, keys // S, keys)   # the last accepted key of each owner, in key order
    np.maximum.at(lc, ckeys // S, ckeys)
    tn = ts_of(row)
    retx = keys[keys // S != v]
    prev = np.where(ins, UNKNOWN, so)
    return dict(row=row, ae_merges=int(pres.sum()), stale_drops=int(stale.sum()), ae_accepts=len(keys),
                change_events=len(ckeys), acc=acc, chg=chg, retx=retx,
                owners_updated=np.nonzero(lu >= 0)[0], last_updated=tn[lu[lu >= 0]],
                owners_changed=np.nonzero(lc >= 0)[0], last_changed=tn[lc[lc >= 0]],
                state_last_changed=int(tn[ckeys[-1]]) if len(ckeys) else None,
                events=np.stack([ckeys // S, ckeys % S, tn[ckeys], st_of(row[ckeys]), prev[ckeys], tn[ckeys]], axis=1))


def exchange_model(Va, Vb, a, b, now, p, both=True):
    """a.Merge(b) and b.Merge(a's snapshot) (ae_exchange, oracle/gx_oracle.c) on the 'before' rows Va,
    Vb; now = slot time of the round. both=False: gx_merge(dst = a, src = b) alone. Returns one dict
    per side (see _merge): row, the four counters, retx (the retransmitted keys in key order: accepted
    and not the side's own), per-owner last_updated / last_changed (slot times, for the owners in
    owners_updated / owners_changed), state_last_changed, events (owner, svc, slot time, status,
    previous status, event time) in key order."""
    S, cut = p.n_services, stale_cut(now, p)
    ma = _merge(Va, Vb, a, S, cut)
    return (ma, _merge(Vb, Va, b, S, cut)) if both else (ma,)


# -------------------------------------------------------------------------------------- the rows --
def _base_rows(rng, n, R, now, p):
    """n seeded base rows: 1/4 absent, 1/2 fresh, 1/8 stale, 1/8 old but not stale; every status."""
    cut = stale_cut(now, p)
    kind = rng.choice(4, size=(n, R), p=[0.25, 0.5, 0.125, 0.125])
    ts = np.select([kind == 1, kind == 2], [now - rng.integers(10**9, 5 * 10**10, size=(n, R)),
                                            cut - rng.integers(10**9, 10**12, size=(n, R))],
                   cut + rng.integers(10**9, 10**12, size=(n, R)))
    return np.where(kind == 0, U(SLOT_ABSENT), pack(ts, STATUSES[rng.integers(0, 4, size=(n, R))]))


def _edited(rng, base, density, now, p):
    """One side of a pair: `base` with seeded edits at `density` of its slots: newer, older, an equal
    timestamp with another status, absent, stale (newer than a stale base word), an older DRAINING
    (the other side's ALIVE is then newer than a DRAINING word)."""
    R, cut = len(base), stale_cut(now, p)
    mask = rng.random(R) < density
    kind = rng.integers(0, 6, size=R)
    d = rng.integers(1, 10**8, size=R)
    bp, bt, bs = st_of(base) != ABSENT, ts_of(base), st_of(base)
    ref = np.where(bp, bt, now - 2 * 10**9)
    nxt = np.array([TOMBSTONE, UNHEALTHY, DRAINING, ALIVE, ALIVE, ALIVE, ALIVE, ALIVE])[bs]
    stx = STATUSES[rng.integers(0, 4, size=R)]
    w = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                  [pack(ref + d, stx), pack(ref - d, stx), pack(ref, nxt), np.full(R, SLOT_ABSENT, dtype=U),
                   pack(np.where(bp & (bt < cut), bt + d, cut - d), stx)], pack(ref - d, DRAINING))
    return np.where(mask, w, base)


def _fresh_row(R, now):
    """All present, all fresh, every word distinct."""
    k = np.arange(R)
    return pack(now - 3 * 10**9 - 1000 * (k * 7919 % R), STATUSES[k % 4])


def _bump(w, by=500, st=None):
    """The same records `by` ns newer (with status st)."""
    return pack(ts_of(w) + by, st_of(w) if st is None else st)


def seam_slots(R, m):
    """The last slot before and the first slot after every multiple of m inside the row."""
    p = np.arange(m, R, m)
    return np.sort(np.concatenate([p - 1, p]))


def hand_rows(kind, a, b, R, S, now, p, seeded):
    """The two rows of a hand-made pair (HAND, CROSS_HAND)."""
    base = _fresh_row(R, now)
    Va, Vb = base.copy(), base.copy()
    k = np.arange(R)
    own_a, own_b = k // S == a, k // S == b
    if kind.startswith("seam"):
        # a newer at one seam slot and b at the next, alternating; a key of one of the two hosts is
        # newer on its owner's side, so that every accept here is also retransmitted
        s = seam_slots(R, int(kind[4:]))
        a_newer = (np.arange(len(s)) % 2 == 0)
        a_newer = np.where(own_a[s], True, np.where(own_b[s], False, a_newer))
        Va[s[a_newer]] = _bump(base[s[a_newer]])
        Vb[s[~a_newer]] = _bump(base[s[~a_newer]])
    elif kind == "same":
        Va = Vb = seeded.copy()  # stale and absent slots included: the shortcut alone
    elif kind == "insert_all":
        Va[:] = SLOT_ABSENT
    elif kind in ("odd_keys", "even_keys"):
        sel = k % 2 == (kind == "odd_keys")
        a_newer = sel & (k // 2 % 2 == 0)
        Va[a_newer] = _bump(base[a_newer])
        Vb[sel & ~a_newer] = _bump(base[sel & ~a_newer])
    elif kind == "last_is_older":
        # every owner: two accepted keys (its first and its last), the later one with the smaller
        # timestamp; even owners accept on side a, odd owners on side b
        first, last = k % S == 0, k % S == S - 1
        new = np.where(first, pack(now - 10**9, ALIVE), pack(now - 2 * 10**9, ALIVE))
        ea, eb = (first | last) & (k // S % 2 == 0), (first | last) & (k // S % 2 == 1)
        Vb[ea] = new[ea]
        Va[eb] = new[eb]
    elif kind == "last_keeps_status":
        # every owner: its first key changes the status, its last is only newer
        first, last = k % S == 0, (k % S == S - 1) & (S > 1)
        new = np.where(first, _bump(base, 700, (st_of(base) + 1) % 3), _bump(base, 300))
        ea, eb = (first | last) & (k // S % 2 == 0), (first | last) & (k // S % 2 == 1)
        Vb[ea] = new[ea]
        Va[eb] = new[eb]
    elif kind == "own_records":
        Vb[own_a] = _bump(base[own_a])  # accepted by a, not retransmitted
        Va[own_b] = _bump(base[own_b])
    # cross pairs: digest blocks of 512 slots
    elif kind == "block1":
        sel = (k // BLK == 1) & (k % 3 == 0)
        Vb[sel] = _bump(base[sel])
    elif kind == "tile_orders":
        # tile 0 = (differs, matched), tile 1 = (matched, differs)
        for blk, V in ((0, Va), (3, Vb)):
            sel = (k // BLK == blk) & (k % 5 == 0)
            V[sel] = _bump(base[sel])
    elif kind == "edge_literals":
        # one differing slot per block, the block's first (block 1) or last (block 2) slot, newer on
        # side b: a leads both blocks (equal literal counts: the pair's first host), and b's return
        # block has its only literal there
        Vb[BLK] = _bump(base[BLK])
        Vb[3 * BLK - 1] = _bump(base[3 * BLK - 1])
    elif kind == "tail_block":
        # newer on side b, which follows: the short block comes back as a return block with literals
        sel = (k // BLK == (R - 1) // BLK) & (k % 2 == 0)
        Vb[sel] = _bump(base[sel])
    elif kind == "lead_both":
        # tile 0: block 0 is one run on side a (a leads it), block 1 one run on side b (b leads it);
        # tile 1 (blocks 2, 3): matched beside a block b leads
        Va[k // BLK == 0] = pack(now - 10**9, ALIVE)
        Vb[k // BLK == 1] = pack(now - 10**9, UNHEALTHY)
        Vb[k // BLK == 3] = pack(now - 10**9, ALIVE)
    else:
        raise KeyError(kind)
    return Va, Vb


def build_views(engine, case, seed=1):
    """Every host's row for the push-pull round the engine is in: per pair of the matching two rows
    of the seeded pool, the first pairs hand-made; a host without a partner gets a pool row too. With
    case["cross"] (G shards) the first cross-shard pairs are the CROSS_HAND ones."""
    H, S, p = engine.H, engine.S, engine.params
    R = H * S
    now = engine.now() - engine.epoch
    rng = np.random.default_rng(seed)
    base = _base_rows(rng, N_BASE, R, now, p)
    pool = np.stack([[[_edited(rng, base[i], d, now, p) for _ in range(N_EDIT)] for d in DENSITIES]
                     for i in range(N_BASE)])  # [base, density, variant, R]
    pairs = ae_pairs(p, engine.round)
    words = np.empty((H, R), dtype=U)
    words[:] = base[rng.integers(0, N_BASE, size=H)]  # the hosts without a partner
    pick = np.stack([rng.integers(0, N_BASE, size=len(pairs)), rng.integers(0, len(DENSITIES), size=len(pairs)),
                     rng.integers(0, N_EDIT, size=len(pairs)), rng.integers(1, N_EDIT, size=len(pairs))], axis=1)
    pa, pb = np.array(pairs).T
    words[pa] = pool[pick[:, 0], pick[:, 1], pick[:, 2]]
    words[pb] = pool[pick[:, 0], pick[:, 1], (pick[:, 2] + pick[:, 3]) % N_EDIT]
    hand = dict(zip(range(len(HAND)), HAND))
    G = case.get("cross", 0)
    if G:
        cross = [t for t, (a, b) in enumerate(pairs) if a * G // H != b * G // H and t >= len(HAND)]
        hand.update(zip(cross, CROSS_HAND))
    assert len(hand) == len(HAND) + (len(CROSS_HAND) if G else 0) <= len(pairs)
    for t, kind in hand.items():
        a, b = pairs[t]
        words[a], words[b] = hand_rows(kind, a, b, R, S, now, p, base[t % N_BASE])
    return words, hand


# ------------------------------------------------------------------------------------ the cases --
def _case(S, H, runs, ae_round=2, listeners=False, big=False, cross=0, **kw):
    p = dict(n_hosts=H, n_services=S, init_mode=INIT_WARM, lock_model=0, storm_round=-1, partition_start=0,
             partition_end=0, ae_period_rounds=10, ae_phase=ae_round % 10)
    p.update(kw)
    return dict(S=S, H=H, R=S * H, runs=runs, params=p, ae_round=ae_round, listeners=listeners, big=big, cross=cross)


LOCK = dict(lock_model=1, init_mode=INIT_OWN, alive_interval_rounds=2, tombstone_interval_rounds=3, churn_ppm=100000,
            ae_period_rounds=5, queue_cap=2048)
CASES = {
    "s16_off": _case(16, 200, "k_ae<true>, NT; tail of 128 slots; the headline's S", listeners=True),
    "s2_off": _case(2, 1537, "k_ae<true>; lpo 1; tail of one lane; one host unpaired"),
    "s64_off": _case(64, 50, "k_ae<true>; lpo 32"),
    "s12_book": _case(12, 260, "k_ae<true> through ae_book; owners straddle tiles", listeners=True),
    "s3_odd": _case(3, 1025, "k_ae<false>: scalar path, odd tail", listeners=True),
    "s32_lock": _case(32, 100, "k_ae_chunk; lock_model 1, some hosts locked", ae_round=4, ae_phase=4,
                      **dict(LOCK, alive_interval_rounds=4, tombstone_interval_rounds=5)),
    "s1_chunk2": _case(1, 8200, "k_ae_chunk, 2 pairs per block; ae_book with 1024 owners per tile", big=True,
                       ae_round=5, ae_phase=0, **LOCK),
    "s16_room": _case(16, 200, "k_ae<true>; windows cut inside a tile, full from the start, across the ring's end",
                      ae_round=8, queue_cap=24, init_mode=INIT_OWN, churn_ppm=100000, alive_interval_rounds=2),
    "s8_depart": _case(8, 400, "pairs with a departed member skipped", depart_round=0, depart_ppm=150000),
    "s16_split": _case(16, 203, "partition active: two groups, two keys, halves 101 / 102", partition_end=3),
    "s8_initiate": _case(8, 400, "k_ae_plan, PF 1, batches (push_pull_mode 1)", push_pull_mode=1),
}
MODELLED = [n for n in CASES if n != "s8_initiate"]  # GX_PP_INITIATE: parity with the oracle only
RUNS = [(n, ev) for n in MODELLED for ev in ((False, True) if CASES[n]["listeners"] else (False,))]
SHARDED = {
    "x_s16_g3": _case(16, 200, "k_ae_plan_pf2; Hl does not divide H; R % 512 = 128", cross=3),
    "x_s3_odd_g2": _case(3, 1025, "k_ae_plan_pf2, scalar path", cross=2),
    "x_s16_ev_g2": _case(16, 200, "k_ae_plan_ev (listeners)", cross=2, listeners=True),
    "x_s2_pf1_g2": _case(2, 4100, "k_ae_plan, PF 1 (>= 1024 cross pairs per shard)", cross=2, big=True, ae_round=8),
}
ALL = dict(CASES, **SHARDED)
N_SEEDED = 16  # seeded pairs checked in detail beside the hand-made ones


def run_id(run):
    return run[0] + ("-ev" if run[1] else "")


def make_engine(lib, name, **extra):
    return Engine(default_params(lib, **dict(ALL[name]["params"], **extra)), lib=lib)


def at_ae_round(lib, name, words=None, ev=False, **extra):
    """An engine between the push-pull round's round_merge() and ae_merge(), holding `words`."""
    case = ALL[name]
    e = make_engine(lib, name, **extra)
    e.run_rounds(case["ae_round"])
    assert e.is_ae_round()
    e.round_send()
    e.round_merge()
    if words is not None:
        e.write_views(words)
    if ev:
        add_listeners(e, name)
    return e


@functools.lru_cache(maxsize=2)
def case_views(name):
    """(words, hand) of the case, built once on the oracle and shared, unchanged, by every test."""
    from tests.oracle_lib import load_oracle
    o = at_ae_round(load_oracle(omp=True), name)
    words, hand = build_views(o, ALL[name])
    words.setflags(write=False)
    o.close()
    return words, hand


def detail_pairs(name, n_pairs):
    """Pair indices checked in detail: the hand-made pairs and N_SEEDED seeded others."""
    hand = case_views(name)[1]
    rest = [t for t in range(n_pairs) if t not in hand]
    rng = np.random.default_rng(3)
    return sorted(hand) + sorted(int(t) for t in rng.choice(rest, size=min(N_SEEDED, len(rest)), replace=False))


def listener_hosts(e, name):
    """(host, capacity) of the listeners: both hosts of every hand-made pair (at most 64 listeners)."""
    pairs = ae_pairs(e.params, ALL[name]["ae_round"])
    hosts = [h for t in sorted(case_views(name)[1]) for h in pairs[t]]
    return [(h, LISTENER_CAPS[i % len(LISTENER_CAPS)]) for i, h in enumerate(hosts)]


def _holder(e, v):
    """The engine that holds host v: e itself, or the shard of a Sharded."""
    return e.engine_of(v) if hasattr(e, "engine_of") else e


def add_listeners(e, name):
    for v, cap in listener_hosts(e, name):
        _holder(e, v).add_listener(v, 1, cap)


def drain_all(e, name):
    return {v: [x.tup() for x in _holder(e, v).drain_listener(v, 1, 8192)] for v, _ in listener_hosts(e, name)}


def before_state(e, hosts=None):
    """What the checks need of engine e before ae_merge(): counters, FIFO fields, locks, departures,
    and for `hosts` (all when None) the server times and state.LastChanged."""
    r, p = e.round, e.params
    hs = e.hosts()
    hosts = range(e.H) if hosts is None else hosts
    return dict(round=r, stats=e.stats(), pairs=ae_pairs(p, r),
                locked=np.array([bool(h.locked_at(r)) for h in hs]),
                departed=np.array([departed(p, v) for v in range(e.H)]),
                head=np.array([h.fifo_head for h in hs], dtype=np.int64),
                tail=np.array([h.fifo_tail for h in hs], dtype=np.int64),
                stored=np.array([h.fifo_stored for h in hs], dtype=np.int64),
                times={v: e.server_times(v) for v in hosts}, last_changed=e.last_changed())


def pair_runs(before, p, t):
    a, b = before["pairs"][t]
    if before["departed"][a] or before["departed"][b]:
        return False
    return not (p.lock_model and (before["locked"][a] or before["locked"][b]))


def room_of(before, v, Q):
    """Jobs host v's stored window can still take (push_job's rule: nothing behind a deferred job)."""
    if before["stored"][v] != before["tail"][v]:
        return 0
    return max(int(Q - (before["stored"][v] - before["head"][v])), 0)


COUNTERS = ("ae_merges", "stale_drops", "ae_accepts", "change_events")


def check_against_model(e, name, words, before, detail=None, events=None, every_pair=True):
    """The model's statements on engine e after ae_merge(). every_pair: the words of every pair's
    rows, untouched rows of pairs that must not run and of unpaired hosts, and the engine-wide counter
    deltas; else only the pairs in `detail`. For the pairs in `detail` (all when None): every owner's
    server times, state.LastChanged, the queue tail job for job, fifo_tail, fifo_stored. `events`
    {host: drained tuples}: the model's ChangeEvents, cut at the listener's capacity. Returns the
    per-pair figures the guards read."""
    p, H, S = e.params, e.H, e.S
    R, Q = H * S, p.queue_cap
    now = e.now() - e.epoch
    pairs = before["pairs"]
    detail = range(len(pairs)) if detail is None else detail
    after = e.read_views()
    hs = e.hosts()
    lc_after = e.last_changed()
    tot = dict.fromkeys(COUNTERS + ("retransmits", "queue_deferred", "ae_slots", "ae_exchanges"), 0)
    fig = dict(runs=np.zeros(len(pairs), dtype=bool), sides={}, accepted=0, slots=0)
    paired = np.zeros(H, dtype=bool)
    for t, (a, b) in enumerate(pairs):
        paired[[a, b]] = True
        if not every_pair and t not in detail:
            continue
        runs = fig["runs"][t] = pair_runs(before, p, t)
        if not runs:
            for v in (a, b):
                assert np.array_equal(after[v], words[v]), f"{name}: pair {t} must not run, row {v} changed"
            continue
        sides = exchange_model(words[a], words[b], a, b, now, p)
        tot["ae_slots"] += 2 * R
        tot["ae_exchanges"] += 1
        fig["accepted"] += sides[0]["ae_accepts"] + sides[1]["ae_accepts"]
        fig["slots"] += 2 * R
        for v, m in zip((a, b), sides):
            bad = np.nonzero(after[v] != m["row"])[0]
            assert not len(bad), f"{name}: pair {t} ({a}, {b}), row {v} differs from the model at keys {bad[:5].tolist()}"
            n, room = len(m["retx"]), room_of(before, v, Q)
            k = min(n, room)
            for c in COUNTERS:
                tot[c] += m[c]
            tot["retransmits"] += n
            tot["queue_deferred"] += n - k
            if t not in detail:
                continue
            fig["sides"][v] = dict(t=t, n=n, room=room, tail0=int(before["tail"][v]), model=m)
            what = f"{name}: pair {t} ({a}, {b}), host {v}"
            want = before["times"][v].copy()
            want[m["owners_updated"], 0] = m["last_updated"] + e.epoch
            want[m["owners_changed"], 1] = m["last_changed"] + e.epoch
            got = e.server_times(v)
            bad = np.argwhere(got != want)
            assert not len(bad), f"{what}: server times differ from the model, first (owner, field) {bad[:5].tolist()}"
            slc = m["state_last_changed"]
            assert lc_after[v] == (before["last_changed"][v] if slc is None else slc + e.epoch), f"{what}: state.LastChanged"
            grew, kept = hs[v].fifo_tail - before["tail"][v], hs[v].fifo_stored - before["stored"][v]
            assert grew == n, f"{what}: fifo_tail grew by {grew}, model {n}"
            assert kept == k, f"{what}: stored {kept} of {n}, room {room}"
            q = queue_array(_holder(e, v), v)
            assert len(q) >= k, f"{what}: queue holds {len(q)} jobs, {k} stored now"
            q = q[len(q) - k:]
            keys = m["retx"][:k]
            assert np.array_equal(q["c"], keys.astype(np.uint32)), f"{what}: retransmit keys differ from the model"
            assert np.array_equal(q["a"], m["row"][keys]), f"{what}: retransmit words differ from the model"
            assert (q["meta"] == RETX_META).all(), f"{what}: retransmit job meta"
    if every_pair:
        for v in np.nonzero(~paired)[0]:
            assert np.array_equal(after[v], words[v]), f"{name}: host {v} has no partner, its row changed"
        st0, st1 = before["stats"], e.stats()
        for c, want in tot.items():
            assert st1[c] - st0[c] == want, f"{name}: {c} grew by {st1[c] - st0[c]}, the model says {want}"
    for v, evs in (events or {}).items():
        cap = dict(listener_hosts(e, name))[v]
        m = fig["sides"][v]["model"] if v in fig["sides"] else None
        want = m["events"] if m is not None else np.zeros((0, 6), dtype=np.int64)
        want = want + np.array([0, 0, e.epoch, 0, 0, e.epoch])
        got = np.array(evs, dtype=np.int64).reshape(-1, 6)
        assert len(got) == min(cap, len(want)), \
            f"{name}: listener of {v} drained {len(got)} events, model {len(want)}, capacity {cap}"
        assert np.array_equal(got, want[:len(got)]), f"{name}: listener of {v}: events differ from the model"
    return fig


# -------------------------------------------------------------------------------- sharded cases --
class Sharded:
    """LocalShards behind the part of Engine's interface check_against_model reads."""

    def __init__(self, sh):
        self.sh = sh
        e = sh.engines[0]
        self.H, self.S, self.params, self.epoch, self.lib = e.H, e.S, e.params, e.epoch, e.lib
        self.now, self.stats = e.now, sh.stats

    round = property(lambda self: self.sh.engines[0].round)

    def engine_of(self, v):
        return next(e for e in self.sh.engines if e.lo <= v < e.hi)

    def read_views(self):
        return np.concatenate([e.read_views() for e in self.sh.engines])

    def hosts(self):
        return sum((e.hosts() for e in self.sh.engines), [])

    def last_changed(self):
        return np.concatenate([e.last_changed() for e in self.sh.engines])

    def server_times(self, v):
        return self.engine_of(v).server_times(v)


def sharded_at_ae_round(lib, name, words, device="cpu", ev=False):
    case = SHARDED[name]
    sh = LocalShards(lib, case["cross"], device=device, **case["params"])
    sh.run_rounds(case["ae_round"])
    assert sh.round_gossip()
    for e in sh.engines:
        e.write_views(words[e.lo:e.hi], e.lo)
    if ev:
        add_listeners(Sharded(sh), name)
    return sh


# ------------------------------------------------------------------ what the guards read (CPU) --
def wave_classes(Va, Vb, acc):
    """Per (tile, wave of the block): the wave's slots are the same on both sides / some are accepted.
    A wave holds slots [128 w, 128 w + 128) of both halves of its tile (4 slots per lane)."""
    R = len(Va)
    nt = (R + TILE - 1) // TILE
    pad = nt * TILE - R
    same = np.pad(Va == Vb, (0, pad), constant_values=True).reshape(nt, 2, 4, WAVE)
    accp = np.pad(acc, (0, pad)).reshape(nt, 2, 4, WAVE)
    return same.all(axis=(1, 3)), accp.any(axis=(1, 3))


def block_classes(Va, Vb, a_first=True):
    """Per digest block of a cross pair, as side a sees it: 0 matched, 1 the partner leads, 2 a leads."""
    R = len(Va)
    out = []
    for blk in range((R + BLK - 1) // BLK):
        if digest(Va, blk) == digest(Vb, blk):
            out.append(0)
        else:
            out.append(2 if leads(Va, Vb, blk, R, a_first) else 1)
    return out


def return_literals(Va, Vb, blk, now, p, a_first=True):
    """The slots of differing block blk that its follower's return block carries as literals (gx.h
    "return": every slot where merging the follower's word into the leader's is not a no-op); the
    other slots are the return block's own mask. None when the digests match."""
    R = len(Va)
    if digest(Va, blk) == digest(Vb, blk):
        return None
    X, Y = (Va, Vb) if leads(Va, Vb, blk, R, a_first) else (Vb, Va)  # leader, follower
    lo = blk * BLK
    return [i - lo for i in range(lo, min(R, lo + BLK)) if not own_ok(int(X[i]), int(Y[i]), now, p)]
