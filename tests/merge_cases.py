"""The gossip merge contract (k_inbox_unpack, k_merge_seg, merge_seg<16>, merge_seg<32>, merge_receiver,
merge_inbox_serial and lock_append_seg in gx_kernels.hpp; DESIGN.md "Gossip merge contract"): one
engine created as shard g of G with no partner shards, whose inbox the test writes record by record in
the packet wire format of gx.h and hands to gx_inbox_unpack; a sequential restatement of what the
receive phase does to one receiver (inbox_model); and the parameter sets whose inboxes reach each seam
of the kernels.

Modelled cases (CASES): a warm, quiescent cluster (no churn, empty queues, no owner tick due in the
round), sparse rows written with gx_write_views after round_send(), then inbox_unpack(crafted) and
round_merge(). The first receivers of the shard, in order, are hand-made (HAND); the others get 0-6
seeded packets of the same edit classes. Lock and queue cases (LOCK_CASES): local traffic present, the
views not rewritten, crafted records built relative to the slots they meet; oracle parity only.

Shared by tests/test_merge_model_cpu.py (the model and the guards, on the oracle alone) and
tests/test_gpu_merge.py (the HIP engine against the oracle and the model)."""
import functools

import numpy as np

from sidecar_amd.abi import (ABSENT, ALIVE, DRAINING, INIT_WARM, SLOT_ABSENT, TOMBSTONE, UNHEALTHY, UNKNOWN, Engine,
                             default_params)
from tests import ae_cases as ac
from tests.ae_cases import pack, stale_cut
from tests.storm_cases import M64, mix64, queue_array

U = np.uint64
SLOT_EMPTY = 0xFFFFFFFF          # gx.h GX_SLOT_EMPTY: a slot gx_inbox_unpack skips
NR = 16                          # receivers per k_merge_seg block below 16,384 local hosts (GX_MERGE_SMALL_HL)
MERGE_WAVES, MSET, TILE = 4, 512, 64
N_SEEDED = 16                    # seeded receivers checked in detail beside the hand-made ones
SEEDED_BLOCKS = (1, 2, 3, 4, 7)  # k_merge_seg blocks whose free receivers get seeded packets
LONE_BLOCK, EMPTY_BLOCK = 5, 6   # one receiver of the 16-lane class alone in its block; a block without any

# hand-made receivers, in receiver order: block 0 holds ten whole-wave receivers (a third pass of the
# item loop), three of the 16-lane and three of the 32-lane class
HAND = ("live33", "live64", "live65", "live130", "pk33x1", "pk64", "pk65", "pk200", "mset_tiles", "mset_full",
        "live1", "live16", "live17", "live32", "pk16x1", "pk17x1",
        "dup_asc", "dup_desc", "dup_equal", "dup_draining", "dup_back", "filter_mix", "all_dropped", "gc_window",
        "own_records", "owner_desc", "last_keeps_status", "insert_absent")
# the hand-made receivers that also run with a listener (capacities as ac.LISTENER_CAPS, in turn)
LISTEN = ("live16", "live17", "live33", "live65", "live130", "pk65", "mset_tiles", "dup_asc", "dup_desc", "dup_equal",
          "dup_draining", "dup_back", "own_records", "owner_desc", "last_keeps_status", "insert_absent", "gc_window")


# ------------------------------------------------------------------------------------ the model --
def inbox_model(row, packets, v, now, p, room, tail):
    """The receive phase of receiver v on round-start row `row` (ph_receive, oracle/gx_oracle.c):
    add_entry(..., SRC_GOSSIP) record by record in arrival order, ascending sender key and then record
    order inside the packet. packets: [(sender key, [(record key, word), ...])]. room: jobs the stored
    window can still take (ac.room_of); tail: fifo_tail before. Returns row, the six counters, jobs (the
    retransmits [(key, word)] in arrival order, one per accepted record v does not own; the first
    `stored` = min(n, room) are stored and fifo_tail grows by n), last_updated / last_changed {owner:
    slot time} of the owner's last accepted / last status-changing record in arrival order,
    state_last_changed, events [owner, svc, slot time, status, previous status, event time]."""
    S, cut = p.n_services, int(stale_cut(now, p))
    row = [int(x) for x in row]
    c = dict.fromkeys(("gossip_merges", "stale_drops", "gossip_accepts", "change_events"), 0)
    jobs, events, lu, lc, slc = [], [], {}, {}, None
    for _, recs in sorted(packets, key=lambda x: x[0]):
        for key, w in recs:
            c["gossip_merges"] += 1
            ts, st = w >> 3, w & 7
            if ts < cut:  # IsStale
                c["stale_drops"] += 1
                continue
            old = row[key]
            so = old & 7
            if so == ABSENT:
                prev, changed = UNKNOWN, True
            elif ts > old >> 3:
                if so == DRAINING and st == ALIVE:
                    st = DRAINING
                prev, changed = so, so != st
            else:
                continue  # equal or older: the first arrival stays
            nw = ts << 3 | st
            row[key] = nw
            c["gossip_accepts"] += 1
            o = key // S
            lu[o] = ts
            if changed:
                lc[o] = slc = ts
                c["change_events"] += 1
                events.append([o, key % S, ts, st, prev, ts])
            if o != v:
                jobs.append((key, nw))
    n = len(jobs)
    k = min(n, room)
    return dict(c, row=np.array(row, dtype=U), jobs=jobs, retransmits=n, stored=k, queue_deferred=n - k,
                fifo_tail=tail + n, last_updated=lu, last_changed=lc, state_last_changed=slc,
                events=np.array(events, dtype=np.int64).reshape(-1, 6))


def unpack_filter(row, recs, now, p):
    """k_inbox_unpack's filter on one packet against the round-start row: the records it keeps (not
    stale, and the slot absent, older, or a tombstone past tombstone_lifespan)."""
    cut, t_gc = stale_cut(now, p), now - p.tombstone_lifespan_ns
    keep = []
    for key, w in recs:
        w0 = int(row[key])
        gc = w0 & 7 == TOMBSTONE and w0 >> 3 < t_gc
        if w >> 3 >= cut and (w0 & 7 == ABSENT or w >> 3 > w0 >> 3 or gc):
            keep.append((key, w))
    return keep


def inbox_class(row, packets, now, p, DI):
    """(deg, live, class) of a receiver as k_merge_seg routes it: deg registered packets (a packet
    without a live record is not registered), live records, and none / seg16 / seg32 / wave / wide
    (a whole wave with more than 64 headers) / serial (more packets than inbox slots)."""
    lens = [len(unpack_filter(row, recs, now, p)) for _, recs in packets]
    deg, live = sum(1 for n in lens if n), sum(lens)
    cls = "none" if not live else "serial" if deg > DI else "wide" if deg > 64 else \
        "seg16" if live <= 16 else "seg32" if live <= 32 else "wave"
    return deg, live, cls


# ---------------------------------------------------------------------------- hand-made inboxes --
class Ctx:
    """What a hand-made receiver is built from: its id, the cluster's sizes, the slot time, its row
    (all present, all fresh, every word distinct; a kind may edit it) and seeded keys."""

    def __init__(self, v, S, H, now, p, seed):
        self.v, self.S, self.H, self.R, self.now, self.p = v, S, H, S * H, now, p
        self.cut, self.t_gc = int(stale_cut(now, p)), now - p.tombstone_lifespan_ns
        k = np.arange(self.R)
        self.row = pack(now - 3 * 10**9 - 1000 * (k * 7919 % self.R), ac.STATUSES[k % 4])
        self.rng = np.random.default_rng(seed)
        foreign = k[k // S != v]
        self._keys = iter(self.rng.permutation(foreign).tolist())

    def keys(self, n):
        """n keys v does not own, distinct from every key drawn before."""
        return [next(self._keys) for _ in range(n)]

    def ts(self, k):
        return int(self.row[k]) >> 3

    def st(self, k):
        return int(self.row[k]) & 7

    def rec(self, k, d=1000, st=None):
        """Key k's record d ns newer than its slot (with status st); a fresh ALIVE one for an absent slot."""
        if self.st(k) == ABSENT:
            return (k, (self.now - 2 * 10**9 + d) << 3 | (ALIVE if st is None else st))
        return (k, (self.ts(k) + d) << 3 | (self.st(k) if st is None else st))

    def other(self, k):
        """A status that differs from key k's slot and stays what it is when it is merged."""
        return {ALIVE: UNHEALTHY, TOMBSTONE: ALIVE, UNHEALTHY: TOMBSTONE, DRAINING: TOMBSTONE}[self.st(k)]

    def owners(self, n):
        """n owners other than v with S distinct keys each (drawn apart from keys())."""
        o = self.rng.permutation(np.delete(np.arange(self.H), self.v))[:n]
        return [int(x) for x in o]


def chunks(recs, sizes):
    out, i = [], 0
    for n in sizes:
        out.append(recs[i:i + n])
        i += n
    assert i == len(recs)
    return out


def _live(c, n, cap):
    """n newer records of distinct keys, in packets of `cap` and a rest."""
    recs = [c.rec(k) for k in c.keys(n)]
    return chunks(recs, [cap] * (n // cap) + ([n % cap] if n % cap else []))


def rand_rec(c, k):
    """A seeded record for key k, relative to the slot it meets: newer, much newer, older, an equal
    timestamp with another status, stale, an older DRAINING, in the stale_fudge window."""
    kind = int(c.rng.choice(7, p=[0.3, 0.15, 0.15, 0.1, 0.1, 0.1, 0.1]))
    d = int(c.rng.integers(1, 10**8))
    ref = c.ts(k) if c.st(k) != ABSENT else c.now - 2 * 10**9
    stx = int(ac.STATUSES[c.rng.integers(0, 4)])
    if kind == 0:
        return (k, (ref + d) << 3 | stx)
    if kind == 1:
        return (k, (ref + 10 * d) << 3 | stx)
    if kind == 2:
        return (k, (ref - d) << 3 | stx)
    if kind == 3:
        return (k, ref << 3 | (ALIVE if c.st(k) != ALIVE else TOMBSTONE))
    if kind == 4:
        return (k, (c.cut - d) << 3 | stx)
    if kind == 5:
        return (k, (ref - d) << 3 | DRAINING)
    return (k, (c.cut + int(c.rng.integers(0, c.p.stale_fudge_ns))) << 3 | stx)


def _packets_of(c, lens, sure=True):
    """Packets of the given lengths on seeded keys, drawn from half as many keys as there are records,
    so that keys repeat: with `sure` the first record of each is newer than its slot, so the packet is
    registered whatever the others do."""
    out = []
    some = c.rng.integers(0, c.R, size=max(1, sum(lens) // 2))
    for n in lens:
        ks = some[c.rng.integers(0, len(some), size=n)].tolist()
        out.append([c.rec(ks[0], 10**8 + int(c.rng.integers(1, 10**6))) if sure else rand_rec(c, ks[0])] +
                   [rand_rec(c, k) for k in ks[1:]])
    return out


def hand_packets(kind, c, cap):
    """The packets of hand-made receiver `kind`, in arrival order (c.row edited where the kind says)."""
    S, v = c.S, c.v
    if kind.startswith("live"):     # routing by live count: distinct keys, every record accepted
        return _live(c, int(kind[4:]), cap)
    if kind in ("pk16x1", "pk17x1", "pk33x1"):  # header ranks: one record per packet
        return _live(c, int(kind[2:4]), 1)
    if kind == "pk64":              # the last narrow inbox: 64 headers
        return _packets_of(c, [2] * 64)
    if kind == "pk65":              # the wide header path (L.pst)
        return _packets_of(c, c.rng.integers(1, cap + 1, size=65).tolist())
    if kind == "pk200":
        return _packets_of(c, c.rng.integers(1, 4, size=200).tolist())
    if kind == "mset_tiles":
        # tile 0: 64 keys accepted at +1000. tile 1: 32 of them again, 16 at +500 (between the round-start
        # word and the accepted one: refused) and 16 at +1500 (accepted), then 32 new keys. tile 2: the 16
        # accepted twice at +1200 (refused) and +1800 (accepted, 8 each), 16 of tile 1's new keys at +500
        # (refused), 8 of tile 0's untouched keys at +700 (refused)
        k0, k1 = c.keys(64), c.keys(32)
        t1 = [c.rec(k, 500) for k in k0[:16]] + [c.rec(k, 1500) for k in k0[16:32]] + [c.rec(k) for k in k1]
        t2 = [c.rec(k, 1200) for k in k0[16:24]] + [c.rec(k, 1800) for k in k0[24:32]] + \
            [c.rec(k, 500) for k in k1[:16]] + [c.rec(k, 700) for k in k0[32:40]]
        order = c.rng.permutation(64).tolist()
        return chunks([c.rec(k) for k in k0] + [t1[i] for i in order] + t2, [cap] * 16 + [cap] * 5)
    if kind == "mset_full":
        # 40 packets of 8 distinct accepted keys (the set stops taking keys past MSET / 2 = 256), then
        # repeats of keys of the first and of the last tile, below and above the accepted word
        ks = c.keys(40 * cap)
        rep = ks[:4] + ks[-4:]
        return chunks([c.rec(k) for k in ks] + [c.rec(k, 500 if i % 2 else 1500) for i, k in enumerate(rep)],
                      [cap] * 40 + [len(rep)])
    if kind == "dup_asc":           # ascending timestamps: every copy accepted, every copy retransmitted
        a, b = c.keys(2)
        return [[c.rec(a, 100)], [c.rec(a, 200), c.rec(b, 100), c.rec(b, 200), c.rec(b, 300)], [c.rec(a, 300)],
                [c.rec(a, 400, c.other(a))]]
    if kind == "dup_desc":          # descending: only the first accepted
        a, b = c.keys(2)
        return [[c.rec(a, 400)], [c.rec(a, 300), c.rec(b, 300), c.rec(b, 200), c.rec(b, 100)], [c.rec(a, 200)],
                [c.rec(a, 100, c.other(a))]]
    if kind == "dup_equal":         # an equal timestamp with another status: the first arrival wins
        a, b = c.keys(2)
        return [[c.rec(a, 100, ALIVE)], [c.rec(a, 100, TOMBSTONE), c.rec(b, 100, UNHEALTHY), c.rec(b, 100, ALIVE)],
                [c.rec(a, 100, UNHEALTHY)]]
    if kind == "dup_draining":      # slot DRAINING, a newer ALIVE (stays DRAINING), then a newer TOMBSTONE
        a, b = c.keys(2)
        for k in (a, b):
            c.row[k] = pack(c.ts(k), DRAINING)
        return [[c.rec(a, 100, ALIVE), c.rec(b, 100, ALIVE)], [c.rec(a, 200, TOMBSTONE)], [c.rec(b, 200, ALIVE)],
                [c.rec(a, 300, ALIVE), c.rec(b, 300, UNHEALTHY)]]
    if kind == "dup_back":          # a status change and a change back: prev of both events
        a, b = c.keys(2)
        sa, sb = c.st(a), c.st(b)
        return [[c.rec(a, 100, c.other(a))], [c.rec(a, 200, sa), c.rec(b, 100, c.other(b)), c.rec(b, 200, sb)],
                [c.rec(a, 300, sa)]]
    if kind == "filter_mix":        # what the unpack filter drops, between live records of the same packet
        ks = c.keys(12)
        dropped = [(ks[0], (c.cut - 5) << 3 | ALIVE), c.rec(ks[1], -100), c.rec(ks[2], 0, c.other(ks[2])),
                   (ks[3], (c.cut - 10**9) << 3 | TOMBSTONE), c.rec(ks[4], -1), c.rec(ks[5], 0)]
        return [[dropped[0], c.rec(ks[6]), dropped[1], dropped[2], c.rec(ks[7]), dropped[3]],
                dropped[3:] + dropped[:3],      # every record dropped: counted, never registered
                [c.rec(ks[8]), dropped[4], c.rec(ks[9], 1)], [dropped[5]], [c.rec(ks[10]), c.rec(ks[11])]]
    if kind == "all_dropped":       # no packet registered at all
        ks = c.keys(6)
        return [[c.rec(ks[0], -1), (ks[1], (c.cut - 1) << 3 | ALIVE)], [c.rec(k, 0, c.other(k)) for k in ks[2:]]]
    if kind == "gc_window":
        # slots inside the stale_fudge window (older than tombstone_lifespan, not stale yet). Tombstones:
        # the filter's garbage-collection clause keeps an older record, and the fold refuses it; other
        # statuses: the filter drops it. Newer records are accepted over both
        ks = c.keys(8)
        for i, k in enumerate(ks):
            c.row[k] = pack(c.t_gc - 10**9 - 1000 * i, TOMBSTONE if i < 6 else ALIVE)
        return [[c.rec(ks[0], -500, ALIVE), c.rec(ks[1], 0, ALIVE), c.rec(ks[2], 500, ALIVE)],
                [c.rec(ks[3], -500, TOMBSTONE), c.rec(ks[6], -500), c.rec(ks[7], 500, TOMBSTONE)],
                [(ks[4], c.cut << 3 | ALIVE), (ks[5], (c.cut - 1) << 3 | ALIVE), c.rec(ks[0], -400, UNHEALTHY)]]
    if kind == "own_records":       # v's own records: accepted, never retransmitted, its own server times
        own = [v * S + s for s in range(S)]
        f = c.keys(3)
        recs = [c.rec(own[-1], 300, c.other(own[-1]))] + [c.rec(f[0])] + [c.rec(k, 200) for k in own[:-1]] + \
            [c.rec(f[1]), c.rec(own[0], 100), c.rec(f[2])]
        return chunks(recs, [2] + [1] * (len(recs) - 2))
    if kind == "owner_desc":
        # per owner two keys, the larger key first and with the larger timestamp: last_updated is the
        # smaller key's (arrival order, not key order, and not the larger timestamp). S = 1: one key twice
        out = []
        for o in c.owners(5):
            hi, lo = o * S + S - 1, o * S
            d = max(900, c.ts(lo) - c.ts(hi) + 10**6)  # the first arrival's timestamp is the larger one
            out.append([c.rec(hi, d)] + ([c.rec(lo, 300)] if S > 1 else [c.rec(lo, d + 50)]))
        return [[r[0] for r in out], [r[1] for r in out]]
    if kind == "last_keeps_status":
        # per owner: the first accept changes the status, the last keeps it: last_changed != last_updated
        first, last = [], []
        for o in c.owners(5):
            a, b = o * S, o * S + S - 1
            first.append(c.rec(a, 300, c.other(a)))
            last.append(c.rec(b, 700) if S > 1 else c.rec(a, 700, first[-1][1] & 7))
        return [first[:3], first[3:] + last[:2], last[2:]]
    if kind == "insert_absent":     # inserts: events with prev UNKNOWN, then a newer copy with the same status
        ks = c.keys(6)
        for k in ks:
            c.row[k] = SLOT_ABSENT
        ins = [(k, (c.now - 10**9 - i) << 3 | int(ac.STATUSES[i % 4])) for i, k in enumerate(ks)]
        return [ins[:4], ins[4:] + [(ins[0][0], ins[0][1] + (50 << 3))], [(ins[1][0], ins[1][1] - (50 << 3))]]
    raise KeyError(kind)


# ----------------------------------------------------------------------------- seeded receivers --
def seeded_row(rng, R, now, p):
    """1/4 absent, 1/2 fresh, 1/8 stale, 1/16 old, 1/16 inside the stale_fudge window; every status."""
    cut = stale_cut(now, p)
    kind = rng.choice(5, size=R, p=[0.25, 0.5, 0.125, 0.0625, 0.0625])
    ts = np.select([kind == 1, kind == 2, kind == 3],
                   [now - rng.integers(10**9, 5 * 10**10, size=R), cut - rng.integers(10**9, 10**12, size=R),
                    now - p.tombstone_lifespan_ns + rng.integers(10**9, 10**12, size=R)],
                   cut + rng.integers(1, p.stale_fudge_ns, size=R))
    return np.where(kind == 0, U(SLOT_ABSENT), pack(ts, ac.STATUSES[rng.integers(0, 4, size=R)]))


# ------------------------------------------------------------------------------------ the cases --
def _case(S, H, runs, listeners=False, g=1, G=4, **kw):
    p = dict(n_hosts=H, n_services=S, fanout=3, gossip_messages=4, packet_cap=8, init_mode=INIT_WARM,
             ae_period_rounds=0, alive_interval_rounds=1000, tombstone_interval_rounds=1000, storm_round=-1,
             partition_start=0, partition_end=0)
    p.update(kw)
    return dict(S=S, H=H, R=S * H, G=G, g=g, runs=runs, params=p, listeners=listeners)


CASES = {
    "s16": _case(16, 500, "every class; wide inboxes (DI 256); the headline's S", listeners=True),
    "s1": _case(1, 500, "S = 1: an owner is one key"),
    "s3_odd": _case(3, 501, "S = 3, odd R; the last shard but one", listeners=True, g=2),
    "s16_slots2": _case(16, 500, "inbox_slots 2 (DR 2): three packets and more fold in merge_inbox_serial", inbox_slots=2),
    "s16_gm1": _case(16, 500, "gossip_messages 1 (DI 64): 65 and 200 packets fold in merge_inbox_serial", g=0,
                     gossip_messages=1),
}
RUNS = [(n, ev) for n in CASES for ev in ((False, True) if CASES[n]["listeners"] else (False,))]


def run_id(run):
    return run[0] + ("-ev" if run[1] else "")


def inbox_slots(p):
    """DI (gx_engine.hip): inbox header slots per receiver."""
    return p.inbox_slots or (256 if p.gossip_messages > 1 else 64)


def make_engine(lib, case, device=None):
    p = default_params(lib, **case["params"])
    p.n_shards, p.shard_id = case["G"], case["g"]
    if device is not None:
        p.device = device
    return Engine(p, lib=lib)


def tick_due(e):
    return any(h.bs_next <= e.round or h.bt_next <= e.round for h in e.hosts())


def gossip_round(e, buf=None):
    """One round of a lone shard, phase by phase; buf: (address, bytes) of received packet slots."""
    e.round_send()
    if buf is not None:
        e.inbox_unpack(*buf)
    e.round_merge()
    e.round_end()


def at_quiet_round(lib, name, device=None):
    """An engine of the case after round_send() of its first round without an owner tick."""
    e = make_engine(lib, CASES[name], device)
    while tick_due(e):
        gossip_round(e)
    e.round_send()
    return e


def sender_keys(e, rng):
    """Every packet key of a sender on another shard (sender * KE + j), shuffled."""
    KE = e.params.fanout * max(1, e.params.gossip_messages)
    s = np.concatenate([np.arange(0, e.lo), np.arange(e.hi, e.H)])
    return rng.permutation((s[:, None] * KE + np.arange(KE)[None, :]).reshape(-1)).tolist()


def slot_buffer(p, inboxes, rng, n_empty=3):
    """The packet slots of `inboxes` {receiver: [(sender key, records)]} in shuffled order (gx.h
    "packet": u32 key, u32 receiver, u32 len, u32 0, then packet_cap x {u64 word, u32 key, u32 0}),
    with n_empty unused slots (GX_SLOT_EMPTY) among them. Returns the bytes as a uint8 array."""
    cap = p.packet_cap
    dt = np.dtype([("key", "<u4"), ("dst", "<u4"), ("len", "<u4"), ("nfd", "<u4"),
                   ("rec", [("w", "<u8"), ("r", "<u4"), ("pad", "<u4")], (cap,))])
    assert dt.itemsize == 16 + 16 * cap
    slots = [(key, v, recs) for v, pk in inboxes.items() for key, recs in pk] + [(SLOT_EMPTY, 0, [])] * n_empty
    buf = np.zeros(len(slots), dtype=dt)
    for i, j in enumerate(rng.permutation(len(slots)).tolist()):
        key, v, recs = slots[j]
        assert len(recs) <= cap and (key == SLOT_EMPTY or recs)
        buf["key"][i], buf["dst"][i], buf["len"][i] = key, v, len(recs)
        for y, (r, w) in enumerate(recs):
            buf["rec"]["w"][i, y], buf["rec"]["r"][i, y] = w, r
    return buf.view(np.uint8).reshape(-1)


def with_keys(packets, pool):
    """Arrival order -> ascending sender keys, taken from the shuffled pool."""
    keys = sorted(pool.pop() for _ in packets)
    return list(zip(keys, packets))


class Built:
    """A case's crafted round: words (the shard's rows), inboxes {receiver: [(sender key, records)]} in
    arrival order, hand {receiver: kind}, buf (the packet slots, uint8)."""


def build_round(e, case, seed=1):
    S, H, p = e.S, e.H, e.params
    now = e.now() - e.epoch
    Hl, cap = e.hi - e.lo, p.packet_cap
    rng = np.random.default_rng(seed)
    pool = sender_keys(e, rng)
    b = Built()
    b.words = np.empty((Hl, H * S), dtype=U)
    b.inboxes, b.hand = {}, {}
    for i in range(Hl):
        v = e.lo + i
        c = Ctx(v, S, H, now, p, seed=1000 + i)
        if i < len(HAND):
            b.hand[v] = HAND[i]
            pk = hand_packets(HAND[i], c, cap)
        elif i == LONE_BLOCK * NR:
            pk = _live(c, 3, cap)
        else:
            c.row = seeded_row(c.rng, c.R, now, p)
            n = int(c.rng.integers(0, 7)) if i // NR in SEEDED_BLOCKS else 0
            pk = _packets_of(c, c.rng.integers(1, cap + 1, size=n).tolist(), sure=False)
        b.words[i] = c.row
        b.inboxes[v] = with_keys(pk, pool)
    b.buf = slot_buffer(p, b.inboxes, rng)
    b.words.setflags(write=False)
    b.buf.setflags(write=False)
    return b


@functools.lru_cache(maxsize=2)
def case_round(name):
    """The case's Built, made once on the oracle and shared, unchanged, by every test."""
    from tests.oracle_lib import load_oracle
    o = at_quiet_round(load_oracle(), name)
    b = build_round(o, CASES[name])
    o.close()
    return b


def detail_hosts(b):
    """The receivers checked in detail: the hand-made ones and N_SEEDED seeded others with packets."""
    rest = [v for v, pk in b.inboxes.items() if pk and v not in b.hand]
    rng = np.random.default_rng(3)
    return sorted(b.hand) + sorted(int(v) for v in rng.choice(rest, size=min(N_SEEDED, len(rest)), replace=False))


def listener_hosts(b):
    """(receiver, capacity) of the listeners: the LISTEN hand-made receivers."""
    hosts = [v for v, kind in sorted(b.hand.items()) if kind in LISTEN]
    return [(v, ac.LISTENER_CAPS[i % len(ac.LISTENER_CAPS)]) for i, v in enumerate(hosts)]


def drain_all(e, b):
    return {v: [x.tup() for x in e.drain_listener(v, 1, 8192)] for v, _ in listener_hosts(b)}


def host_buffer(buf):
    """(address, bytes) of the slots in host memory (the oracle), and what keeps them alive."""
    a = np.array(buf)
    return (a.ctypes.data, a.size), a


def device_buffer(buf, device=0):
    """The same in device memory (the HIP engine)."""
    import torch
    t = torch.from_numpy(np.array(buf)).to(f"cuda:{device}")
    torch.cuda.synchronize(device)
    return (t.data_ptr(), t.numel()), t


def before_state(e, hosts):
    """What the checks need of engine e after round_send(): counters, the local hosts' FIFO fields, and
    for `hosts` the server times; every local view's state.LastChanged."""
    hs = e.hosts()
    return dict(stats=e.stats(), lo=e.lo,
                head=np.array([h.fifo_head for h in hs], dtype=np.int64),
                tail=np.array([h.fifo_tail for h in hs], dtype=np.int64),
                stored=np.array([h.fifo_stored for h in hs], dtype=np.int64),
                times={v: e.server_times(v) for v in hosts}, last_changed=e.last_changed())


def received(e, b, ev, buf):
    """write_views, listeners, inbox_unpack, round_merge on engine e (after round_send())."""
    e.write_views(b.words, e.lo)
    if ev:
        for v, cap in listener_hosts(b):
            e.add_listener(v, 1, cap)
    e.inbox_unpack(*buf)
    e.round_merge()


COUNTERS = ("gossip_merges", "stale_drops", "gossip_accepts", "retransmits", "queue_deferred", "change_events")


def check_against_model(e, name, b, before, detail, events=None):
    """The model's statements on engine e after round_merge(): every local row, the engine-wide counter
    deltas since `before`; for the receivers in `detail` every owner's server times, state.LastChanged,
    the queue job for job, fifo_tail and fifo_stored; `events` {receiver: drained tuples}: the model's
    ChangeEvents, cut at the listener's capacity. Returns {receiver: model}."""
    p, lo = e.params, e.lo
    now = e.now() - e.epoch
    after = e.read_views()
    hs = e.hosts()
    lc_after = e.last_changed()
    tot = dict.fromkeys(COUNTERS, 0)
    models = {}
    for v, pk in b.inboxes.items():
        i = v - lo
        room = ac.room_of(before, i, p.queue_cap)
        m = models[v] = inbox_model(b.words[i], pk, v, now, p, room, int(before["tail"][i]))
        for c in COUNTERS:
            tot[c] += m[c]
        what = f"{name}: receiver {v} ({b.hand.get(v, 'seeded')})"
        bad = np.nonzero(after[i] != m["row"])[0]
        assert not len(bad), f"{what}: row differs from the model at keys {bad[:5].tolist()}"
        if v not in detail:
            continue
        want = before["times"][v].copy()
        for o, ts in m["last_updated"].items():
            want[o, 0] = ts + e.epoch
        for o, ts in m["last_changed"].items():
            want[o, 1] = ts + e.epoch
        bad = np.argwhere(e.server_times(v) != want)
        assert not len(bad), f"{what}: server times differ from the model, first (owner, field) {bad[:5].tolist()}"
        slc = m["state_last_changed"]
        assert lc_after[i] == (before["last_changed"][i] if slc is None else slc + e.epoch), f"{what}: state.LastChanged"
        grew, kept = hs[i].fifo_tail - before["tail"][i], hs[i].fifo_stored - before["stored"][i]
        assert grew == m["retransmits"], f"{what}: fifo_tail grew by {grew}, model {m['retransmits']}"
        assert kept == m["stored"], f"{what}: stored {kept} of {m['retransmits']}, room {room}"
        q = queue_array(e, v)
        k = m["stored"]
        assert len(q) >= k, f"{what}: queue holds {len(q)} jobs, {k} stored now"
        q = q[len(q) - k:]
        assert q["c"].tolist() == [r for r, _ in m["jobs"][:k]], f"{what}: retransmit keys differ from the model"
        assert q["a"].tolist() == [w for _, w in m["jobs"][:k]], f"{what}: retransmit words differ from the model"
        assert (q["meta"] == ac.RETX_META).all(), f"{what}: retransmit job meta"
    st0, st1 = before["stats"], e.stats()
    for c, want in tot.items():
        assert st1[c] - st0[c] == want, f"{name}: {c} grew by {st1[c] - st0[c]}, the model says {want}"
    caps = dict(listener_hosts(b))
    for v, evs in (events or {}).items():
        want = models[v]["events"] + np.array([0, 0, e.epoch, 0, 0, e.epoch])
        got = np.array(evs, dtype=np.int64).reshape(-1, 6)
        assert len(got) == min(caps[v], len(want)), \
            f"{name}: listener of {v} drained {len(got)} events, model {len(want)}, capacity {caps[v]}"
        assert np.array_equal(got, want[:len(got)]), f"{name}: listener of {v}: events differ from the model"
    return models


# ------------------------------------------------------------------------ lock and queue cases --
# Local traffic is present and the views are not rewritten: every crafted record is built relative to
# the slot it meets after round_send() (read from the oracle), for W rounds in a row, so that a
# pipeline filled in one crafted round is full, or drains, in a later one. Oracle parity only.
def _lock_case(runs, first, **kw):
    c = _case(16, 500, runs, **dict(ac.LOCK, ae_period_rounds=0, **kw))
    return dict(c, first=first, window=6, drain=16)


LOCK_CASES = {
    "lock40": _lock_case("lock_buffer 40: pipelines that fill inside a packet, and full ones", 1, lock_buffer=40),
    "lock150": dict(_lock_case("lock_buffer 150: more than 64 records appended (two SEG * LOCK_RPL passes)", 1,
                               lock_buffer=150), drain=28),
    "lock_off": _lock_case("lock_model 0: locked receivers merge, counted", 1, lock_model=0, lock_buffer=40),
    "s16_room": _lock_case("queue_cap 24: room cut inside the retransmits, room 0, the ring's end", 8, lock_model=0,
                           queue_cap=24),
}
LOCKED_KINDS = ("fits", "cut", "many17", "big72", "nine")
ST_PEER = 1  # the peer stream of the engines' seeded generator (oracle/gx_oracle.c)


def sample_peers(p, rnd, u):
    """sample_peers (oracle/gx_oracle.c) outside a partition: host u's gossip targets of round rnd, in
    target order (packet entry j of u goes to target j // max(1, gossip_messages))."""
    H, peers, a = p.n_hosts, [], 0
    while len(peers) < min(p.fanout, H - 1) and a < 64 * p.fanout:
        h = mix64(p.seed ^ ((ST_PEER * 0xD1B54A32D192ED03) & M64))
        for x in (rnd, u, a):
            h = mix64(h ^ x)
        idx = ((h >> 32) * (H - 1)) >> 32
        q = idx + 1 if idx >= u else idx
        if q not in peers:
            peers.append(q)
        a += 1
    return peers


def local_targets(e):
    """The hosts some host of engine e's shard may send a packet to in e's round."""
    return {q for u in range(e.lo, e.hi) for q in sample_peers(e.params, e.round, u)}


def lock_lens(kind, room, cap):
    """Packet lengths of a locked receiver with `room` places left in its pipeline."""
    if kind == "fits":     # room for all of its records
        return [3, 3]
    if kind == "cut":      # room ends inside a packet (with no local packet: no prefix sum equals room)
        first = 5 if (room - 5) % cap else 3
        return [first] + [cap] * ((room - first) // cap + 2)
    if kind == "many17":   # more than SEG packets: the whole-wave fallback of lock_append_seg
        return [1] * 17
    if kind == "big72":    # more than 64 records appended, from more than 8 packets (past the inline DR slots)
        return [cap] * 9
    if kind == "nine":     # more than 8 packets, few records
        return [2] * 9
    if kind == "full":     # dropped at unpack
        return [4, 4]
    raise KeyError(kind)


def build_lock_round(o, name):
    """The crafted inbox of the round oracle `o` is in (after its round_send()): Built with inboxes,
    kinds {receiver: kind}, buf, and pre (the local hosts' bookkeeping the kinds were chosen from)."""
    S, H, p, r = o.S, o.H, o.params, o.round
    now = o.now() - o.epoch
    rows, hs = o.read_views(), o.hosts()
    rng = np.random.default_rng(100 + r)
    pool = sender_keys(o, rng)
    b = Built()
    b.inboxes, b.kinds, b.pre, b.rows, b.targets = {}, {}, hs, rows, local_targets(o)
    nl = nu = 0
    for i, h in enumerate(hs):
        v = o.lo + i
        c = Ctx(v, S, H, now, p, seed=r * 1000 + i)
        c.row = rows[i]
        locked, nb = bool(h.locked_at(r)), h.lock_buffered
        if name == "s16_room":
            kind, pk = "retx", _live(c, 12, 6)
        elif locked and p.lock_model and nb >= p.lock_buffer:
            kind = "full"
        elif locked:
            kind = LOCKED_KINDS[nl % len(LOCKED_KINDS)]
            nl += 1
            if kind == "big72" and p.lock_buffer - nb < 80:
                kind = "fits"
        elif nb:
            kind = ("drain_packets", "drain_alone")[nu % 2]
            nu += 1
        else:
            kind = "seeded"
        if kind == "seeded":
            pk = _packets_of(c, c.rng.integers(1, p.packet_cap + 1, size=int(c.rng.integers(2, 7))).tolist(), sure=False)
        elif kind.startswith("drain"):
            pk = _packets_of(c, [4, 4, 4] if kind == "drain_packets" else [])
        elif kind != "retx":
            pk = _packets_of(c, lock_lens(kind, p.lock_buffer - nb, p.packet_cap), sure=False)
        b.kinds[v] = kind
        b.inboxes[v] = with_keys(pk, pool)
    b.buf = slot_buffer(p, b.inboxes, rng)
    return b


def make_lock_engine(lib, name, device=None):
    return make_engine(lib, LOCK_CASES[name], device)


def lock_rounds(o, others, name):
    """Steps oracle `o` and the engines `others` [(engine, buffer maker)] through the case's crafted
    rounds; yields (round, Built) after every crafted round's round_merge(). The round's round_end()
    follows when the walk goes on, the last round's too: a walk run to its end leaves every engine
    between two rounds."""
    case = LOCK_CASES[name]
    es = [(o, host_buffer)] + list(others)
    for e, _ in es:
        while e.round < case["first"]:
            gossip_round(e)
    for _ in range(case["window"]):
        for e, _ in es:
            e.round_send()
        b = build_lock_round(o, name)
        keep = []
        for e, mk in es:
            buf, t = mk(b.buf)
            keep.append(t)
            e.inbox_unpack(*buf)
        for e, _ in es:
            e.round_merge()
        yield o.round, b
        for e, _ in es:
            e.stats()  # waits for the device before the buffer goes
            e.round_end()
        del keep
