"""The expiry scan contract (TombstoneOthersServices: expiry_word, scan_view, scan_chunk_waves, k_scan,
k_scan_split, k_scan_join, k_bt_finish, the scan prologue of k_send and gx_tombstone_others; DESIGN.md
"Expiry scan contract"): rows written with gx_write_views at the start of one round, a numpy
restatement of what one BroadcastTombstones tick's scan does to a row (scan_model), and the
parameter sets whose rows put expirations next to each seam of the kernels.

A case runs `warm` quiet rounds, writes every local row, and runs the scan round phase by phase. The
first ticking views of the shard, in order, are hand-made (one kind each, hand_kinds); the others get
a seeded row with a few expirations. Every row also holds records whose deadlines fall exactly on the
scan round, and 3, 5 and 7 rounds later, on keys no row of the case expires in the scan round (QUIET
keys), so that the follow-up rounds check the expiry bound the scan left behind.

Shared by tests/test_scan_model_cpu.py (the model and the guards, on the oracle alone) and
tests/test_gpu_scan.py (the HIP engine against the oracle and the model)."""
import functools

import numpy as np

from sidecar_amd.abi import (ALIVE, DRAINING, INIT_WARM, JOB_SEND, SLOT_ABSENT, TOMBSTONE, TS_SHIFT, UNHEALTHY,
                             UNKNOWN, Engine, default_params)
from tests.ae_cases import pack, st_of, ts_of
from tests.storm_cases import departed, queue_array

U = np.uint64
TILE, HALF, WAVE = 1024, 512, 128     # scan_view: 256 threads x 4 slots, two 512-slot halves of 4 waves
WTILE, WHALF = 256, 128               # scan_chunk_waves: a wave's tile of 64 lanes x 4 slots, two halves
SCAN_ITEMS = 2048                     # scan_chunks: blocks a split scan aims at
EXP_ST = np.array([ALIVE, UNHEALTHY, UNKNOWN, DRAINING], dtype=np.int64)
N_SEEDED = 8                          # seeded views checked in detail beside the hand-made ones
LISTENER_CAPS = (8192, 5)             # roomy, and smaller than the events of most hand-made rows
FOLLOW_UP = 12                        # rounds after the scan round
LATER = (3, 5, 7)                     # rounds after the scan round at which the later deadlines fall


# ------------------------------------------------------------------------------------ the model --
def life_of(st, p):
    """The lifespan the scan applies to status st (vector)."""
    return np.where(st == TOMBSTONE, p.tombstone_lifespan_ns,
                    np.where(st == DRAINING, p.draining_lifespan_ns, p.alive_lifespan_ns)).astype(np.int64)


def scan_model(row, v, now, p, L, departed_owners):
    """scan_view (oracle/gx_oracle.c) on viewer v's row at slot time `now`, and what bt_tick does with
    its result. departed_owners: bool [H]. The rule is strict: a non-tombstone with ts < now - life
    becomes pack(ts + tombstone_bump_ns, TOMBSTONE); a tombstone with ts < now - tombstone_lifespan_ns
    becomes absent and counts in gc only. Returns row, expired, gc, false_expiries, written (slots that
    change), keys (every expired key, in key order), list (the first min(n, L) of them, (key, new
    word)), times {owner: slot time of its last expired key}, state_last_changed (None without an
    expiry), events [owner, svc, slot time, TOMBSTONE, previous status, event time], deadline (the
    minimum over the present slots of the new row of timestamp + lifespan; None for an empty row)."""
    S = p.n_services
    row = np.asarray(row, dtype=U)
    st, ts = st_of(row), ts_of(row)
    present = row != U(SLOT_ABSENT)
    tomb = present & (st == TOMBSTONE)
    gc = tomb & (ts < now - p.tombstone_lifespan_ns)
    exp = present & ~tomb & (ts < now - life_of(st, p))
    new = np.where(exp, pack(ts + p.tombstone_bump_ns, TOMBSTONE), np.where(gc, U(SLOT_ABSENT), row))
    keys = np.nonzero(exp)[0]
    tn = ts_of(new)
    own = np.arange(v * S, (v + 1) * S)
    assert not exp[own].any() and not gc[own].any(), "the model leaves the viewer's own slots out"
    times = {int(o): int(t) for o, t in zip(keys // S, tn[keys])}  # key order: the last one stays
    pres2 = new != U(SLOT_ABSENT)
    dl = tn[pres2] + life_of(st_of(new[pres2]), p)
    ev = np.stack([keys // S, keys % S, tn[keys], np.full(len(keys), TOMBSTONE), st[keys], tn[keys]], axis=1)
    return dict(row=new, expired=len(keys), gc=int(gc.sum()), written=int((new != row).sum()),
                false_expiries=int((~np.asarray(departed_owners)[keys // S]).sum()), keys=keys,
                list=[(int(k), int(new[k])) for k in keys[:L]], times=times,
                state_last_changed=int(tn[keys[-1]]) if len(keys) else None, events=ev.astype(np.int64),
                deadline=int(dl.min()) if len(dl) else None)


# ------------------------------------------------------------------------------- scan geometry --
def scan_nch(R, S):
    """gx_engine.hip: the most chunks a row takes, fixed at create (the stride of the chunk tables)."""
    if R >= 65536 and S >= 2 and 128 % S == 0:
        return min(R // 32768, 16)
    return 1


def scan_chunks(R, n, nch):
    """scan_chunks (gx_kernels.hpp): (chunks, clen) of a round whose worklist holds n views."""
    c = min((SCAN_ITEMS + n - 1) // n if n else 1, nch)
    clen = (R // c + 1023) // 1024 * 1024
    return (R + clen - 1) // clen, clen


def wave_quarter(clen_actual):
    """scan_chunk_waves: a wave's range inside a chunk of clen_actual slots."""
    return (clen_actual // 4 + 255) // 256 * 256


def path_of(case, ev):
    """The scan's code path: (placement, kernel) as gx_engine.hip's round_send_impl selects them."""
    S, R = case["S"], case["R"]
    vec = R % 2 == 0
    if case["place"] == "send":
        return ("send", "fused" if S <= 16 else "prologue")
    if vec and not ev and scan_nch(R, S) > 1:
        return ("scan", "split")
    wave_times = vec and S >= 2 and 128 % S == 0
    return ("scan", "block-wave" if wave_times else "block-lds" if vec else "scalar")


# --------------------------------------------------------------------------------- row builders --
def around(points, R):
    """The keys p-2, p-1, p, p+1 of every point p, one of the four (in turn) as a GC-only tombstone:
    (expiring keys, gc keys). Points may equal R (the row's end)."""
    points = np.unique(np.asarray(points, dtype=np.int64))
    points = points[(points >= 2) & (points <= R)]
    k = points[:, None] + np.array([-2, -1, 0, 1])[None, :]
    is_gc = np.arange(4)[None, :] == (np.arange(len(points)) % 4)[:, None]
    ok = k < R
    return k[ok & ~is_gc], k[ok & is_gc]


class Ctx:
    """What a row is built from: the viewer, the sizes, the slot time of the scan round, the case's
    QUIET keys and chunk geometry."""

    def __init__(self, v, case, now, p, quiet, geo, seed):
        self.v, self.S, self.H, self.R, self.now, self.p = v, case["S"], case["H"], case["R"], now, p
        self.quiet, self.geo = quiet, geo
        self.L = p.packet_cap + p.pending_cap
        self.rng = np.random.default_rng(seed)
        self.qset = np.sort(quiet.reshape(-1))

    def free(self, keys):
        """The keys that are neither the viewer's own nor QUIET."""
        keys = np.asarray(keys, dtype=np.int64)
        return keys[(keys // self.S != self.v) & ~np.isin(keys, self.qset)]

    def run_to(self, m, n_back, n_fwd):
        """n_back free keys ending at the last free key below m, and n_fwd from m on, in key order."""
        pad = self.S + 64 + (n_back + n_fwd) // 8
        free = self.free(np.arange(max(m - n_back - pad, 0), min(m + n_fwd + pad, self.R)))
        i = np.searchsorted(free, m)
        assert i >= n_back and i + n_fwd <= len(free)
        return free[i - n_back:i + n_fwd]


def base_row(R, now, seed=11):
    """Nothing can expire for 50 s: every status and absent slots, fresh timestamps. One per case: the
    rows differ in the viewer's own slots (the engine's) and in what place() writes."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(6, size=R, p=[0.3, 0.15, 0.1, 0.15, 0.15, 0.15])
    st = np.array([ALIVE, UNHEALTHY, UNKNOWN, DRAINING, TOMBSTONE, 0])[kind]
    ts = now - rng.integers(10**9, 30 * 10**9, size=R)
    return np.where(kind == 5, U(SLOT_ABSENT), pack(ts, st))


def place(c, row, exp, gc, deadlines=True):
    """Writes expiring records at the free keys of `exp` and GC-only tombstones at those of `gc`; the
    first two expiring keys and the first gc key sit exactly one tick past their lifespan. With
    `deadlines`: on the row's QUIET keys the three records exactly on their lifespan (they stay), the
    three later deadlines (LATER) and a tombstone that already equals the word the first expiry
    becomes. Returns the last expiring key (or -1)."""
    p, now = c.p, c.now
    exp, gc = c.free(exp), c.free(gc)
    gc = np.setdiff1d(gc, exp)
    n = len(exp)
    st = EXP_ST[c.rng.integers(0, 4, size=n)]
    if n:
        st[0] = ALIVE
    if n > 1:
        st[1] = DRAINING
    late = c.rng.integers(0, 5 * 10**8, size=n)
    late[:2] = 0
    row[exp] = pack(now - life_of(st, p) - 1 - late, st)
    late = c.rng.integers(0, 5 * 10**8, size=len(gc))
    late[:1] = 0
    row[gc] = pack(now - p.tombstone_lifespan_ns - 1 - late, np.full(len(gc), TOMBSTONE))
    last = int(exp.max()) if n else -1
    if deadlines:
        q = quiet_for(c, last)
        r = p.round_ns
        al, dl, tl = p.alive_lifespan_ns, p.draining_lifespan_ns, p.tombstone_lifespan_ns
        for key, w in ((q[0][0], pack(now - al, UNKNOWN)), (q[1][0], pack(now - dl, DRAINING)),
                       (q[2][0], pack(now - tl, TOMBSTONE)),
                       (q[0][1], pack(now - al - 1 + LATER[0] * r, UNHEALTHY)),
                       (q[1][1], pack(now - tl - 1 + LATER[1] * r, TOMBSTONE)),
                       (q[2][1], pack(now - dl - 1 + LATER[2] * r, DRAINING)),
                       (q[0][2], pack(now - al - 1 + p.tombstone_bump_ns, TOMBSTONE))):
            if key // c.S != c.v:  # (the viewer's own slots stay the engine's)
                row[key] = w
    return last


def quiet_for(c, last):
    """[3][3] QUIET keys of a row whose last expiring key is `last`: with chunks, each triple from a
    chunk other than that key's."""
    nc = len(c.quiet)
    lc = chunk_of(c.geo, last)
    ch = [(lc + 1 + j) % nc for j in range(3)]
    ch = [x if x != lc or nc == 1 else (lc + 1) % nc for x in ch]
    return [c.quiet[x][3 * j:3 * j + 3] for j, x in enumerate(ch)]


def later_keys(c, last):
    """The keys of the row's three later deadlines, as place() chose them."""
    q = quiet_for(c, last)
    return [int(q[0][1]), int(q[1][1]), int(q[2][1])]


def chunk_of(geo, key):
    return int(key) // geo["clen"] if key >= 0 else 0


def owner_last(c, odd):
    """Every second owner expires at its slot 0 and at its last even (odd) slot."""
    S = c.S
    o = np.arange(0, c.H, 2)
    last = S - 1 if odd else max(S - 2, 0)
    if S % 2 == 1 and S > 1:
        last = S - 2 if odd else S - 1  # (key parity follows the owner's base for odd S: both occur)
    return np.unique(np.concatenate([o * S, o * S + last]))


def straddlers(c, side):
    """The owners that straddle a tile seam expire on both sides of it, before it only, after it only."""
    S, out = c.S, []
    for m in range(TILE, c.R, TILE):
        o = m // S
        if o * S == m:
            continue
        ks = np.arange(o * S, min((o + 1) * S, c.R))
        out.append(ks if side == "both" else ks[ks < m] if side == "first" else ks[ks >= m])
    return np.concatenate(out)


def pair_keys(R):
    """Within the first 600 keys and the last 64: of four pairs in turn the even slot, the odd slot,
    both, none."""
    k = np.concatenate([np.arange(0, 600), np.arange(R - 64, R)])
    return k[np.isin(k // 2 % 4 * 2 + k % 2, (0, 3, 4, 5))]


def hand_kinds(case, geo=None):
    """The hand-made rows of a case, in order: [(kind, f(c) -> (expiring keys, gc keys))]."""
    S, R = case["S"], case["R"]
    nch = case["nch"]
    none = np.array([], dtype=np.int64)

    def mult(m):
        return np.arange(m, R + 1, m)
    kinds = []
    if nch > 1:
        geo = geo or case_geo(case, 1)
        nc, clen = geo["nc"], geo["clen"]
        starts = np.arange(nc) * clen
        lens = np.minimum(starts + clen, R) - starts
        quarters = np.concatenate([s + np.arange(1, 4) * wave_quarter(n) for s, n in zip(starts, lens)])
        kinds += [("chunks", lambda c: around(starts[1:], R)),
                  ("quarters", lambda c: around(quarters[quarters < R], R)),
                  ("tiles256", lambda c: around(mult(WTILE), R)),
                  ("halves128", lambda c: around(mult(WHALF)[::2], R)),
                  # the second of a wave's two tiles in flight: odd multiples of 256 from each wave's start
                  ("second_tile", lambda c: around(np.concatenate([quarters, starts]) + WTILE, R)),
                  # a chunk without an expiry between two that have some, and none in the final chunk
                  ("chunk_gap", lambda c: around([5, clen // 2] + ([2 * clen + 300] if nc > 3 else []), R)),
                  ("last_slot", lambda c: (np.array([R - 1]), none)),
                  ("gc_only", lambda c: (none, mult(4096) - 1)),
                  ("cap_quarter", lambda c: (c.run_to(int(quarters[0]), c.L, c.L + 1), none)),
                  ("cap_chunk", lambda c: (c.run_to(clen, c.L, 2 * c.L + 5), none)),
                  ("cap_exact", lambda c: (c.run_to(clen, c.L, 0), none)),
                  ("cap_less", lambda c: (c.run_to(clen, c.L - 1, 0), none))]
        return kinds
    kinds += [("pairs", lambda c: (pair_keys(R), none)),
              ("seam128", lambda c: around(mult(WAVE), R)),
              ("seam512", lambda c: around(mult(HALF), R)),
              ("seam1024", lambda c: around(mult(TILE), R)),
              ("row_end", lambda c: (np.array([R - 1]), np.array([R - 3]))),
              ("gc_only", lambda c: (none, mult(200) - 1))]
    if S > 1:
        kinds += [("owner_even", lambda c: (owner_last(c, False), none)),
                  ("owner_odd", lambda c: (owner_last(c, True), none))]
    if TILE % S:
        kinds += [("straddle_" + side, lambda c, side=side: (straddlers(c, side), none))
                  for side in ("both", "first", "second")]
    # the list's capacity crossed inside a pair, inside a wave, between the halves of a tile and between
    # tiles (the L-th expiry at the last free key below m, the next at m); L - 1, L, L + 1, 3 L + 5
    for cross, m in (("pair", 2 * TILE + 31), ("wave", 2 * TILE + 32), ("half", TILE + HALF), ("tile", TILE)):
        for n in ("less", "exact", "plus1", "three"):
            def f(c, m=m, n=n):
                L = c.L
                back, fwd = {"less": (L - 1, 0), "exact": (L, 0), "plus1": (L, 1), "three": (L, 2 * L + 5)}[n]
                fits = m - back >= 2 * c.S + 16 and m + fwd + 16 <= R
                return (c.run_to(m, back, fwd) if fits else none, none)
            if case["caps"] or (cross, n) in (("tile", "plus1"), ("half", "three")):
                kinds.append((f"cap_{cross}_{n}", f))
    return kinds


def seeded_row(c, row, dense=False):
    """A few expirations and GC tombstones at seeded free keys."""
    n = int(c.rng.integers(1 if dense else 0, max(2, min(c.R // 200, 400))))
    keys = np.unique(c.rng.integers(0, c.R, size=2 * n))
    keys = c.rng.permutation(keys)
    n = len(keys) // 2
    return place(c, row, keys[:n], keys[n:])


# ------------------------------------------------------------------------------------ the cases --
def _case(S, H, runs, G=1, g=0, place="scan", warm=2, listeners=False, caps=False, model=True, model_all=True, dense=False,
          **kw):
    p = dict(n_hosts=H, n_services=S, init_mode=INIT_WARM, tombstone_interval_rounds=1, alive_interval_rounds=1000,
             ae_period_rounds=0, storm_round=-1, partition_start=0, partition_end=0)
    p.update(kw)
    R = S * H
    return dict(S=S, H=H, R=R, G=G, g=g, runs=runs, params=p, place=place, warm=warm, listeners=listeners, caps=caps,
                model=model, model_all=model_all, dense=dense, nch=scan_nch(R, S))


SEND_WARM = 10  # quiet rounds, one call each, before a k_send-placement case's scan round (scan_probe_begin)
CASES = {
    # block path, server times from ballots (S | 128, R even): rows of two tiles and a part
    "w_s2": _case(2, 1300, "S = 2: one lane per owner; row end 2600 = 2 tiles + 552", G=10, g=3),
    "w_s16": _case(16, 170, "S = 16, the headline's; every list-capacity crossing at L = 132", listeners=True, caps=True),
    "w_s64": _case(64, 43, "S = 64: one owner over 32 lanes", listeners=True),
    # block path, server times through LDS (S does not divide 128, or S = 1)
    "l_s3": _case(3, 900, "S = 3, R even: owners straddle tile seams", G=4, g=1, listeners=True),
    "l_s12": _case(12, 230, "S = 12", listeners=True),
    "l_s1": _case(1, 2600, "S = 1, R even: 1024 owners in a tile", G=10, g=9),
    # scalar path (R odd)
    "o_s3": _case(3, 901, "S = 3, R odd: the last slot alone in its pair", G=4, g=3, listeners=True),
    "o_s5": _case(5, 541, "S = 5, R odd", G=2, g=0),
    "o_s1": _case(1, 2601, "S = 1, R odd", G=10, g=0),
    # list capacities
    "cap1": _case(16, 170, "L = 1", caps=True, listeners=True, packet_cap=1, pending_cap=0),
    "cap8": _case(16, 170, "L = 8", caps=True, listeners=True, packet_cap=4, pending_cap=4),
    "cap512": _case(16, 230, "L = 512", caps=True, listeners=True, packet_cap=256, pending_cap=256),
    # split path (S | 128, R >= 65536): one shard of a larger cluster
    "x_64k": _case(32, 2048, "R = 65536: 2 chunks; with a listener the block path over 64 tiles", G=64, g=5,
                   listeners=True),
    "x_128k": _case(64, 2048, "R = 131072: 4 chunks", G=64, g=63),
    "x_256k": _case(64, 4096, "R = 262144: 8 chunks", G=64, g=40),
    "x_few": _case(64, 4096, "R = 262144, 300 listed views: 7 chunks in tables strided by scan_nch = 8", G=13, g=6,
                   model_all=False, dense=True),
    "x_dep": _case(32, 2048, "R = 65536 with departures: false_expiries of the split path", G=64, g=9, depart_round=0,
                   depart_ppm=150000),
    "x_1026": _case(64, 1026, "R = 65664: clen rounded up, the last chunk short", G=38, g=7),
    "x_cap8": _case(64, 1024, "R = 65536, L = 8: the capacity between waves and chunks", G=32, g=0, packet_cap=4,
                    pending_cap=4),
    # placements: the scan in k_send (no view scanned in the rounds before)
    "p_s2": _case(2, 1300, "k_send, owner class S <= 4", G=10, g=3, place="send", warm=SEND_WARM),
    "p_s8": _case(8, 340, "k_send, owner class S <= 8", place="send", warm=SEND_WARM),
    "p_s16": _case(16, 170, "k_send, owner class S <= 16", place="send", warm=SEND_WARM, listeners=True),
    "p_s64": _case(64, 43, "k_send, the tick == 2 prologue (S > 16)", place="send", warm=SEND_WARM, listeners=True),
    "p_s3": _case(3, 901, "k_send, scalar rows", G=4, g=3, place="send", warm=SEND_WARM),
    # k_bt_finish apart
    "b_fd": _case(16, 170, "fd_enable: the list queued before the detector's jobs", fd_enable=1),
    "b_storm": _case(16, 170, "the storm round: the list queued before the storm's jobs", model=False, warm=2,
                     storm_round=2, partition_end=8, lock_model=0),
    # departures: false_expiries
    "d_s16": _case(16, 170, "departed owners and viewers", depart_round=0, depart_ppm=150000),
}
RUNS = [(n, ev) for n in CASES for ev in ((False, True) if CASES[n]["listeners"] else (False,))]
API_CASES = ("w_s16", "l_s12", "o_s3", "w_s64")


def run_id(run):
    return run[0] + ("-ev" if run[1] else "")


def make_engine(lib, case, device=None):
    p = default_params(lib, **case["params"])
    if case["G"] > 1:
        p.n_shards, p.shard_id = case["G"], case["g"]
    if device is not None:
        p.device = device
    return Engine(p, lib=lib)


def gossip_round(e):
    e.round_send()
    e.round_merge()
    e.round_end()


def warm_up(e, case):
    """The case's quiet rounds, one call and one synchronizing read each."""
    for _ in range(case["warm"]):
        gossip_round(e)
        e.stats()


def ticking(e):
    """Which local views' BroadcastTombstones looper ticks in the round that runs next (ph_owner), when
    no BroadcastServices tick is due: bool [Hl], and the local views where one is (they are left out:
    their rows hold nothing that can expire)."""
    r, lm, p = e.round, e.params.lock_model != 0, e.params
    out, unknown = [], []
    for i, h in enumerate(e.hosts()):
        gone = p.depart_round >= 0 and r >= p.depart_round and departed(p, e.lo + i)
        if h.bs_next <= r and not gone:  # its BroadcastServices tick comes first and may block this one
            unknown.append(i)
        out.append(h.bs_next > r and not gone and not (h.flags & 2) and not (lm and h.flags & 1) and h.bt_next <= r)
    return np.array(out), unknown


def case_geo(case, n_work):
    nc, clen = scan_chunks(case["R"], n_work, case["nch"])
    return dict(nc=nc, clen=clen)


def quiet_keys(case, geo):
    """[chunk][9] keys that no row of the case expires in the scan round, apart from every multiple of
    128: nine per chunk (per third of an unsplit row)."""
    R, split = case["R"], case["nch"] > 1
    nc = geo["nc"] if split else 3
    span = geo["clen"] if split else R // 3
    rng = np.random.default_rng(5)
    out = []
    for c in range(nc):
        k = np.arange(c * span, min((c + 1) * span, R))
        k = k[(k % WAVE >= 40) & (k % WAVE < 90) & (k % 4 == 1)]
        out.append(np.sort(rng.choice(k, size=9, replace=False)))
    return np.array(out, dtype=np.int64)


class Built:
    """A case's scan round: words (the shard's rows), tick (bool per local view), hand {view: kind},
    last {view: its last expiring key or -1}, quiet, geo, now (slot time)."""


def build_round(e, case):
    S, R, p = case["S"], case["R"], e.params
    now = e.now() - e.epoch
    b = Built()
    b.tick, b.skip = ticking(e)
    b.now = now
    cur = e.read_views()
    b.geo = case_geo(case, int(b.tick.sum()))
    kinds = hand_kinds(case, b.geo)
    b.quiet = quiet_keys(case, b.geo)
    b.words = np.empty((e.hi - e.lo, R), dtype=U)
    base = base_row(R, now)
    b.hand, b.last = {}, {}
    n_hand = 0
    for i in range(e.hi - e.lo):
        v = e.lo + i
        c = Ctx(v, case, now, p, b.quiet, b.geo, seed=1000 + i)
        row = b.words[i]
        row[:] = base
        row[v * S:(v + 1) * S] = cur[i, v * S:(v + 1) * S]
        if b.tick[i] and n_hand < len(kinds):
            kind, f = kinds[n_hand]
            n_hand += 1
            b.hand[v] = kind
            exp, gc = f(c)
            b.last[v] = place(c, row, exp, gc)
        elif (i % 7 == 6 and not case["dense"]) or i in b.skip:
            b.last[v] = place(c, row, [], [], deadlines=False)  # nothing to expire: the view is not scanned
        else:
            b.last[v] = seeded_row(c, row, case["dense"])
    b.n_kinds = len(kinds)
    b.words.setflags(write=False)
    return b


@functools.lru_cache(maxsize=2)
def case_round(name):
    """The case's Built, made once on the oracle and shared, unchanged, by every test."""
    from tests.oracle_lib import load_oracle
    case = CASES[name]
    o = make_engine(load_oracle(omp=True), case)
    warm_up(o, case)
    b = build_round(o, case)
    o.close()
    return b


def ctx_of(e, case, b, v):
    return Ctx(v, case, b.now, e.params, b.quiet, b.geo, seed=0)


def detail_views(b, lo):
    """The views checked in detail: the hand-made ones and N_SEEDED ticking others."""
    rest = [lo + i for i in np.nonzero(b.tick)[0] if lo + i not in b.hand]
    rng = np.random.default_rng(3)
    return sorted(b.hand) + sorted(int(v) for v in rng.choice(rest, size=min(N_SEEDED, len(rest)), replace=False))


def listener_views(b):
    """(view, capacity) of the listeners: the first 16 hand-made views, capacities in turn."""
    return [(v, LISTENER_CAPS[i % 2]) for i, v in enumerate(sorted(b.hand)[:16])]


def drain_all(e, b):
    return {v: [x.tup() for x in e.drain_listener(v, 1, 16384)] for v, _ in listener_views(b)}


def before_state(e, views):
    return dict(stats=e.stats(), times={v: e.server_times(v) for v in views}, last_changed=e.last_changed(),
                launches=e.timing()["scan"]["launches"])


def scan_round_on(lib, name, ev, device=None):
    """An engine of the case after the scan round's round_send(), and what was read before it."""
    case = CASES[name]
    b = case_round(name)
    e = make_engine(lib, case, device)
    warm_up(e, case)
    detail = detail_views(b, e.lo)
    e.write_views(b.words, e.lo)
    if ev:
        for v, cap in listener_views(b):
            e.add_listener(v, 1, cap)
    before = before_state(e, detail)
    e.round_send()
    events = drain_all(e, b) if ev else None
    return e, b, before, detail, events


def sent_list(e, v):
    """The list of view v's BroadcastTombstones SendServices job of this round, [(updated_ns, host, svc,
    status)]: the job is in the queue, or, sent once already, among the sleepers."""
    jobs = [(int(j["c"]), int(j["meta"])) for j in queue_array(e, v)] + [(s.job.c, s.job.meta) for s in e.sleepers(v)]
    mine = [c for c, meta in jobs if meta & 7 == JOB_SEND and (meta >> 9) & 63 == e.params.tombstone_count]
    assert len(mine) == 1, f"view {v}: {len(mine)} SendServices jobs of a BroadcastTombstones tick"
    got = [s.tup() for s in e.read_list(v, mine[0] & 0xFFFF)]
    assert len(got) == mine[0] >> 16
    return got


def check_against_model(e, name, b, before, detail, events=None):
    """scan_model's statements on engine e after the scan round's round_send(): every local row outside
    the viewer's own slots (a view that does not tick keeps its row), the counters' growth summed over
    the ticking views; for the views in `detail` every owner's server times, state.LastChanged and the
    sent list; `events`: the ChangeEvents, cut at the listener's capacity. Returns {view: model}."""
    case = CASES[name]
    S, p, lo = case["S"], e.params, e.lo
    L = p.packet_cap + p.pending_cap
    after = e.read_views()
    lc = e.last_changed()
    gone = np.array([p.depart_round >= 0 and departed(p, o) for o in range(e.H)])
    tot = dict(expired=0, gc=0, false_expiries=0, scan_slots=0)
    models = {}
    for i in range(e.hi - lo):
        v = lo + i
        what = f"{name}: view {v} ({b.hand.get(v, 'seeded')})"
        other = np.ones(case["R"], dtype=bool)
        other[v * S:(v + 1) * S] = False
        if not case["model_all"] and v not in detail:
            continue
        if not b.tick[i]:
            assert np.array_equal(after[i][other], b.words[i][other]), f"{what} did not tick, its row changed"
            continue
        m = models[v] = scan_model(b.words[i], v, b.now, p, L, gone)
        for k in ("expired", "gc", "false_expiries"):
            tot[k] += m[k]
        tot["scan_slots"] += case["R"]
        bad = np.nonzero((after[i] != m["row"]) & other)[0]
        assert not len(bad), f"{what}: row differs from the model at keys {bad[:5].tolist()}"
        if v not in detail:
            continue
        want = before["times"][v].copy()
        for o, ts in m["times"].items():
            want[o] = ts + e.epoch
        got = e.server_times(v)
        got[v], want[v] = 0, 0
        bad = np.argwhere(got != want)
        assert not len(bad), f"{what}: server times differ from the model, first (owner, field) {bad[:5].tolist()}"
        slc = m["state_last_changed"]
        assert lc[i] == (before["last_changed"][i] if slc is None else slc + e.epoch), f"{what}: state.LastChanged"
        if m["expired"]:
            want = [(w >> TS_SHIFT) + e.epoch for _, w in m["list"]]
            got = sent_list(e, v)
            assert [(t[1] * S + t[2], t[3]) for t in got] == [(k, TOMBSTONE) for k, _ in m["list"]], f"{what}: the list's keys"
            assert [t[0] for t in got] == want, f"{what}: the list's timestamps"
    st0, st1 = before["stats"], e.stats()
    if b.skip:
        del tot["scan_slots"]
    for k, want in tot.items() if case["model_all"] else ():
        assert st1[k] - st0[k] == want, f"{name}: {k} grew by {st1[k] - st0[k]}, the model says {want}"
    caps = dict(listener_views(b))
    for v, evs in (events or {}).items():
        if v not in models:
            continue
        want = models[v]["events"] + np.array([0, 0, e.epoch, 0, 0, e.epoch])
        got = np.array(evs, dtype=np.int64).reshape(-1, 6)
        assert len(got) == min(caps[v], len(want)), \
            f"{name}: listener of {v} drained {len(got)} events, model {len(want)}, capacity {caps[v]}"
        assert np.array_equal(got, want[:len(got)]), f"{name}: listener of {v}: events differ from the model"
    return models


def finish_round(e):
    e.round_merge()
    e.round_end()


def follow_up(e):
    for _ in range(FOLLOW_UP):
        gossip_round(e)


# --------------------------------------------------------------------------------- the API call --
def api_caps(n, L):
    """The capacities gx_tombstone_others is called with for a row of n expirations."""
    return sorted({0, 1, max(n - 1, 0), n, n + 1, L + 3})


def api_calls(e, name):
    """gx_tombstone_others on every hand-made view of the case's scan round, capacities from api_caps in
    turn. Returns [(view, cap, records as tuples, n_out)]."""
    b = case_round(name)
    L = e.params.packet_cap + e.params.pending_cap
    gone = np.zeros(e.H, dtype=bool)
    out = []
    for j, v in enumerate(sorted(b.hand)):
        n = scan_model(b.words[v - e.lo], v, b.now, e.params, L, gone)["expired"]
        caps = api_caps(n, L)
        cap = caps[j % len(caps)]
        recs, n_out = e.tombstone_others(v, cap)
        out.append((v, cap, [r.tup() for r in recs], n_out))
    return out
