"""The gossip merge contract on the oracle alone (tests/merge_cases.py): inbox_model equals the oracle's
receive phase on every modelled case, and each case's inboxes reach what the case names (the vacuity
guards, computed from the written rows, the crafted packets and the hosts' bookkeeping), so the GPU
tests that import the same cases cannot quietly stop testing it. The lock and queue cases pick their
round by walking the oracle; their guards assert what the crafted inboxes meet at that round."""
import time
from collections import Counter

import numpy as np
import pytest

from sidecar_amd.abi import ABSENT, ALIVE, DRAINING, TOMBSTONE, UNHEALTHY, UNKNOWN, GxParams
from tests import ae_cases as ac
from tests import merge_cases as mc
from tests.oracle_lib import load_oracle


def merge_round_on(lib, name, ev, device=None):
    """An engine of the case after the crafted round's round_merge(), and what was read before."""
    b = mc.case_round(name)
    e = mc.at_quiet_round(lib, name, device)
    detail = mc.detail_hosts(b)
    before = mc.before_state(e, detail)
    buf, keep = (mc.host_buffer if device is None else mc.device_buffer)(b.buf)
    mc.received(e, b, ev, buf)
    events = mc.drain_all(e, b) if ev else None
    return e, b, before, detail, events, keep


@pytest.mark.parametrize("run", mc.RUNS, ids=mc.run_id)
def test_merge_model_and_guards(run):
    name, ev = run
    case = mc.CASES[name]
    S, H = case["S"], case["H"]
    t0 = time.time()
    e, b, before, detail, events, _ = merge_round_on(load_oracle(), name, ev)
    models = mc.check_against_model(e, name, b, before, detail, events)
    p = e.params
    now = e.now() - e.epoch
    Hl, DI = e.hi - e.lo, mc.inbox_slots(p)
    hs = e.hosts()
    # the rig: a lone shard, a quiescent round (no local packet, no job, no sleeper, nobody locked, no
    # owner tick due), the hand-made receivers first, sender keys of other shards, each at most once
    assert Hl % mc.NR and case["G"] > 1 and p.ae_period_rounds == 0 and p.init_mode == mc.INIT_WARM and not p.churn_ppm
    assert before["stats"]["packets"] == 0 and (before["head"] == before["tail"]).all() and not mc.tick_due(e)
    assert all(h.lock == 0 and h.sleep_head == h.sleep_tail and h.dq_len == 0 for h in hs)
    assert [b.hand[e.lo + i] for i in range(len(mc.HAND))] == list(mc.HAND)
    KE = p.fanout * max(1, p.gossip_messages)
    keys = [k for pk in b.inboxes.values() for k, _ in pk]
    assert len(set(keys)) == len(keys) and all(k < H * KE and not e.lo <= k // KE < e.hi for k in keys)
    assert any(k // KE < e.lo for k in keys) or e.lo == 0
    assert any(k // KE >= e.hi for k in keys)
    for v, pk in b.inboxes.items():
        assert [k for k, _ in pk] == sorted(k for k, _ in pk)  # the lists are in arrival order
    # routing: (deg, live, class) of every receiver, from the filter restated on the round-start rows
    cls = {v: mc.inbox_class(b.words[v - e.lo], pk, now, p, DI) for v, pk in b.inboxes.items()}
    kind = {k: v for v, k in b.hand.items()}
    K = {k: cls[v] for k, v in kind.items()}
    M = {k: models[v] for k, v in kind.items()}
    big = "serial" if name == "s16_slots2" else "wave"
    wide = "serial" if DI < 256 else "wide"
    assert K["live1"] == (1, 1, "seg16") and K["live16"] == (2, 16, "seg16")
    seg32 = "seg32" if DI >= 17 else "serial"
    assert K["live17"] == (3, 17, seg32) and K["live32"] == (4, 32, seg32)
    assert K["live33"] == (5, 33, big) and K["live64"] == (8, 64, big) and K["live65"] == (9, 65, big)
    assert K["live130"] == (17, 130, big)
    assert K["pk16x1"] == (16, 16, "seg16" if DI >= 16 else "serial") and K["pk17x1"] == (17, 17, seg32)
    assert K["pk33x1"] == (33, 33, big)
    assert K["pk64"][0] == 64 and K["pk64"][2] == big and K["pk65"][0] == 65 and K["pk65"][2] == wide
    assert K["pk200"][0] == 200 and K["pk200"][2] == wide and K["pk200"][1] > 3 * mc.TILE
    for k in ("live1", "live16", "live17", "live32", "live33", "live64", "live65", "live130", "pk16x1", "pk17x1", "pk33x1"):
        n = K[k][1]  # every record accepted and retransmitted, in an order that is not key order
        assert M[k]["gossip_accepts"] == M[k]["retransmits"] == n and M[k]["change_events"] == 0
        assert n < 3 or [r for r, _ in M[k]["jobs"]] != sorted(r for r, _ in M[k]["jobs"])
    # block layout: ten whole-wave receivers in block 0 (three passes of MERGE_WAVES items), the lone
    # 16-lane receiver (an item with three MERGE_NONE slots), the block without any, the partial block
    by_blk = [Counter(cls[e.lo + i][2] for i in range(blk * mc.NR, min(Hl, (blk + 1) * mc.NR)))
              for blk in range((Hl + mc.NR - 1) // mc.NR)]
    if name in ("s16", "s1", "s3_odd"):
        assert by_blk[0]["wave"] + by_blk[0]["wide"] >= 2 * mc.MERGE_WAVES + 1
        assert by_blk[0]["seg16"] == 3 and by_blk[0]["seg32"] == 3
    assert by_blk[mc.LONE_BLOCK] == Counter({"none": mc.NR - 1, "seg16": 1})
    assert by_blk[mc.EMPTY_BLOCK] == Counter({"none": mc.NR})
    assert sum(by_blk[-1].values()) == Hl % mc.NR and sum(n for c, n in by_blk[-1].items() if c != "none") >= 3
    tot = Counter(c for _, _, c in cls.values())
    if name in ("s16", "s1", "s3_odd"):
        assert tot["seg16"] >= 40 and tot["seg32"] >= 3 and tot["wave"] >= 8 and tot["wide"] == 2 and not tot["serial"]
    if name == "s16_slots2":
        assert tot["serial"] >= 30 and K["dup_asc"][2] == "serial"
    if name == "s16_gm1":
        assert tot["serial"] == 2 and K["pk64"][2] == "wave"
    # one key several times
    assert M["dup_asc"]["gossip_accepts"] == M["dup_asc"]["retransmits"] == 7 == M["dup_asc"]["gossip_merges"]
    assert M["dup_asc"]["change_events"] == 1
    assert M["dup_desc"]["gossip_accepts"] == 2 and M["dup_desc"]["gossip_merges"] == 7 and K["dup_desc"][1] == 7
    assert M["dup_equal"]["gossip_accepts"] == 2 and K["dup_equal"][1] == 5
    m = M["dup_draining"]
    assert m["gossip_accepts"] == 6 and [x[3] for x in m["events"]] == [TOMBSTONE, ALIVE, UNHEALTHY] and \
        [x[4] for x in m["events"]] == [DRAINING, TOMBSTONE, DRAINING]
    m = M["dup_back"]
    assert m["gossip_accepts"] == 5 and m["change_events"] == 4 and [x[4] for x in m["events"]][1] == m["events"][0][3]
    # the written-key set: records of later tiles refused against a word an earlier tile wrote
    m = M["mset_tiles"]
    assert K["mset_tiles"][1] == 168 and m["gossip_accepts"] == 64 + 16 + 32 + 8 and m["stale_drops"] == 0
    m = M["mset_full"]
    assert K["mset_full"][1] == 40 * 8 + 8 and 40 * 8 > mc.MSET // 2 and m["gossip_accepts"] == 40 * 8 + 4
    # the unpack filter
    v = kind["filter_mix"]
    lens = [len(mc.unpack_filter(b.words[v - e.lo], recs, now, p)) for _, recs in b.inboxes[v]]
    assert lens == [2, 0, 2, 0, 2] and M["filter_mix"]["gossip_merges"] == 18 and M["filter_mix"]["stale_drops"] == 4
    assert M["filter_mix"]["gossip_accepts"] == 6
    m = M["all_dropped"]
    assert K["all_dropped"] == (0, 0, "none") and m["gossip_merges"] == 6 and m["gossip_accepts"] == 0
    # ... and its garbage-collection clause: records the filter keeps and the fold refuses
    v = kind["gc_window"]
    no_gc = GxParams.from_buffer_copy(p)
    no_gc.tombstone_lifespan_ns = 1 << 57  # no slot is past it
    kept = sum(len(mc.unpack_filter(b.words[v - e.lo], recs, now, p)) for _, recs in b.inboxes[v])
    kept_no_gc = sum(len(mc.unpack_filter(b.words[v - e.lo], recs, now, no_gc)) for _, recs in b.inboxes[v])
    assert (kept, kept_no_gc) == (7, 2) and M["gc_window"]["gossip_accepts"] == 2 and M["gc_window"]["stale_drops"] == 1
    # owners
    m = M["own_records"]
    v = kind["own_records"]
    assert m["gossip_accepts"] == S + 3 and m["retransmits"] == 3 and v in m["last_updated"] and v in m["last_changed"]
    for k in ("owner_desc", "last_keeps_status"):
        m = M[k]
        assert len(m["last_updated"]) == 5 and m["gossip_accepts"] == 10
    m, v = M["owner_desc"], kind["owner_desc"]
    acc_ts = {}
    for r, w in m["jobs"]:
        acc_ts.setdefault(r // S, []).append(w >> 3)
    assert all(m["last_updated"][o] == t[-1] and (S == 1 or t[-1] < t[0]) for o, t in acc_ts.items())
    m = M["last_keeps_status"]
    assert sorted(m["last_changed"]) == sorted(m["last_updated"])
    assert all(m["last_changed"][o] != m["last_updated"][o] for o in m["last_changed"])
    m = M["insert_absent"]
    assert m["gossip_accepts"] == 7 and m["change_events"] == 6 and (m["events"][:, 4] == UNKNOWN).all()
    assert K["insert_absent"][1] == 8
    # the seeded receivers: every rule occurs
    seeded = [v for v in b.inboxes if v not in b.hand and b.inboxes[v]]
    recs = [(v, r, w) for v in seeded for _, pk in b.inboxes[v] for r, w in pk]
    w0 = np.array([b.words[v - e.lo][r] for v, r, _ in recs])
    w = np.array([x for _, _, x in recs], dtype=np.uint64)
    cut = ac.stale_cut(now, p)
    pres = ac.st_of(w0) != ABSENT
    assert len(seeded) >= 40 and (~pres).sum() > 20 and (ac.ts_of(w) < cut).sum() > 20
    assert (pres & (ac.ts_of(w) == ac.ts_of(w0)) & (w != w0)).sum() > 10
    assert (pres & (ac.ts_of(w) < ac.ts_of(w0))).sum() > 20
    assert ((ac.st_of(w0) == DRAINING) & (ac.st_of(w) == ALIVE) & (ac.ts_of(w) > ac.ts_of(w0)) & (ac.ts_of(w) >= cut)).sum() > 0
    assert ((ac.st_of(w0) == TOMBSTONE) & (ac.ts_of(w0) < now - p.tombstone_lifespan_ns) & (ac.ts_of(w) >= cut)
            & (ac.ts_of(w) <= ac.ts_of(w0))).sum() > 0  # the filter's gc clause among the seeded records
    rkeys = {v: [r for _, pk in b.inboxes[v] for r, _ in pk] for v in seeded}
    assert sum(1 for v in seeded if len(set(rkeys[v])) < len(rkeys[v])) >= 10  # a key several times in one inbox
    if ev:  # a listener overflows, one takes every event of its receiver
        caps = dict(mc.listener_hosts(b))
        assert len(caps) >= 6 and any(len(x) == caps[v] < len(models[v]["events"]) for v, x in events.items())
        assert any(0 < len(x) < caps[v] for v, x in events.items())
    for k in mc.HAND:
        print(f"MERGE-CASE {mc.run_id(run)} {k}: deg={K[k][0]} live={K[k][1]} class={K[k][2]} "
              f"accepted={M[k]['gossip_accepts']} retx={M[k]['retransmits']} events={M[k]['change_events']}")
    print(f"MERGE-CASE {mc.run_id(run)}: S={S} H={H} shard {case['g']}/{case['G']} Hl={Hl} DI={DI} packets={len(keys)} "
          f"records={sum(m['gossip_merges'] for m in models.values())} classes={dict(sorted(tot.items()))} "
          f"seconds={time.time() - t0:.1f}")


def test_inbox_model_by_hand():
    """The model on hand-written words: receiver 1 of 3 hosts, S = 2, every rule once."""
    p = GxParams(n_hosts=3, n_services=2, tombstone_lifespan_ns=1000, stale_fudge_ns=100)
    now = 10_000  # stale below 8900

    def w(ts, st):
        return (ts << 3) | st
    A = 7
    row = [w(9000, ALIVE), A, w(9000, DRAINING), w(9000, ALIVE), w(9500, TOMBSTONE), w(8950, TOMBSTONE)]
    packets = [(40, [(0, w(9200, ALIVE)), (1, w(8000, ALIVE)), (2, w(9100, ALIVE))]),   # arrives second
               (7, [(0, w(9300, UNHEALTHY)), (1, w(9100, UNHEALTHY)), (4, w(9500, ALIVE)), (5, w(8900, ALIVE))]),
               (41, [(3, w(9400, ALIVE)), (1, w(9200, UNHEALTHY)), (0, w(9400, UNHEALTHY))])]
    m = mc.inbox_model(np.array(row, dtype=np.uint64), packets, 1, now, p, room=2, tail=5)
    # key 0: 9300 UNHEALTHY accepted (a change), 9200 refused, 9400 UNHEALTHY accepted (no change). key 1:
    # inserted at 9100, 8000 stale, 9200 accepted (no change). key 2 (own): ALIVE onto DRAINING stays
    # DRAINING. key 3 (own): newer, same status. key 4: an equal timestamp. key 5: older, not stale
    assert m["row"].tolist() == [w(9400, UNHEALTHY), w(9200, UNHEALTHY), w(9100, DRAINING), w(9400, ALIVE),
                                 w(9500, TOMBSTONE), w(8950, TOMBSTONE)]
    assert (m["gossip_merges"], m["stale_drops"], m["gossip_accepts"], m["change_events"]) == (10, 1, 6, 2)
    assert m["jobs"] == [(0, w(9300, UNHEALTHY)), (1, w(9100, UNHEALTHY)), (1, w(9200, UNHEALTHY)), (0, w(9400, UNHEALTHY))]
    assert (m["retransmits"], m["stored"], m["queue_deferred"], m["fifo_tail"]) == (4, 2, 2, 9)
    assert m["last_updated"] == {0: 9400, 1: 9400} and m["last_changed"] == {0: 9100} and m["state_last_changed"] == 9100
    assert m["events"].tolist() == [[0, 0, 9300, UNHEALTHY, ALIVE, 9300], [0, 1, 9100, UNHEALTHY, UNKNOWN, 9100]]
    # the filter keeps the records of key 5's packet that the garbage-collection clause names
    assert mc.unpack_filter(row, packets[1][1], now, p) == [(0, w(9300, UNHEALTHY)), (1, w(9100, UNHEALTHY)),
                                                            (5, w(8900, ALIVE))]


# ------------------------------------------------------------------------ lock and queue cases --
def test_sample_peers_restated(oracle_lib):
    """merge_cases.sample_peers equals the oracle's targets: every packet slot two oracle shards pack
    for each other names the receiver the restatement gives for its sender and entry."""
    from sidecar_amd.abi import Engine, default_params
    kw = dict(n_hosts=40, n_services=4, fanout=3, gossip_messages=2, packet_cap=8, init_mode=1, alive_interval_rounds=1)
    n = 0
    es = []
    for g in range(2):
        p = default_params(oracle_lib, **kw)
        p.n_shards, p.shard_id = 2, g
        es.append(Engine(p, lib=oracle_lib))
    for _ in range(3):
        for e in es:
            e.round_send()
            sizes = e.outbox_bytes()
            buf = np.zeros(int(sizes.sum()), dtype=np.uint8)
            e.outbox_pack(buf.ctypes.data, buf.size)
            hdr = buf.reshape(-1, 16 + 16 * 8)[:, :16].copy().view("<u4")
            for key, dst, ln, _ in hdr.tolist():
                assert ln and mc.sample_peers(e.params, e.round, key // 6)[key % 6 // 2] == dst and e.lo <= key // 6 < e.hi
                n += 1
            e.round_merge()
            e.round_end()
    assert n > 50


def lock_guard_walk(lib, name):
    """Walks the oracle through the case's crafted rounds; returns per line of the case's list the
    receivers that met it [(round, receiver)], and the engine at the window's end."""
    case = mc.LOCK_CASES[name]
    o = mc.make_lock_engine(lib, name)
    p = o.params
    C, Q, cap = p.lock_buffer, p.queue_cap, p.packet_cap
    met = {k: [] for k in ("fits", "cut", "full", "over16", "over64", "over8", "drain_packets", "drain_alone",
                           "drain_stale", "drain_both", "locked_merge", "room_cut", "room0", "ring")}
    st0 = o.stats()
    # pipe[v]: the records in v's pipeline, in order, while they are known: it was empty, and since then
    # no local packet could reach v, so what it holds are the crafted records that fitted
    pipe = {}
    for r, b in mc.lock_rounds(o, [], name):
        post, st = o.hosts(), o.stats()
        now = o.now() - o.epoch
        after = o.read_views()
        drops = drained = 0
        for i, (h0, h1) in enumerate(zip(b.pre, post)):
            v = o.lo + i
            kind, lens = b.kinds[v], [len(recs) for _, recs in b.inboxes[v]]
            alone = v not in b.targets  # no local packet can reach v this round: its inbox is the crafted one
            locked, nb0, nb1 = bool(h0.locked_at(r)), h0.lock_buffered, h1.lock_buffered
            if nb0 == 0:
                pipe[v] = []
            if locked and p.lock_model:
                room = C - nb0
                flat = [x for _, recs in b.inboxes[v] for x in recs]
                pipe[v] = pipe[v] + flat[:nb1 - nb0] if alone and pipe.get(v) is not None else None
                if kind == "full":
                    assert nb0 >= C and nb1 == nb0
                    met["full"].append((r, v))
                    drops += sum(lens)
                    continue
                if nb1 < C and nb1 - nb0 >= sum(lens):
                    met["fits"].append((r, v))
                if alone and sum(lens) > room > 0 and room not in np.cumsum(lens) and nb1 == C:
                    met["cut"].append((r, v))
                    drops += sum(lens) - room
                if len(lens) > 16 and nb1 - nb0 >= min(sum(lens), room) > 0:
                    met["over16"].append((r, v))  # ... and what fitted was appended
                if nb1 - nb0 > 64:
                    met["over64"].append((r, v))
                if len(lens) > 8 and nb1 - nb0 >= sum(lens):
                    met["over8"].append((r, v))  # every packet's records were kept: the ones past the inline slots too
            elif locked:
                if lens:
                    met["locked_merge"].append((r, v))
            elif nb0 and p.lock_model:
                assert nb1 == 0
                drained += nb0
                if lens:
                    met["drain_packets"].append((r, v))
                elif alone:
                    met["drain_alone"].append((r, v))
                known = pipe.pop(v, None)
                if alone and known is not None:
                    # the fold is the pipeline first, then the packets: the model on both, in that order
                    assert len(known) == nb0
                    room = ac.room_of(dict(head=[h0.fifo_head], tail=[h0.fifo_tail], stored=[h0.fifo_stored]), 0, Q)
                    m = mc.inbox_model(b.rows[i], [(-1, known)] + b.inboxes[v], v, now, p, room, h0.fifo_tail)
                    assert np.array_equal(after[i], m["row"]) and h1.fifo_tail == m["fifo_tail"], (r, v)
                    k = m["stored"]
                    q = mc.queue_array(o, v)
                    assert q["c"][len(q) - k:].tolist() == [x for x, _ in m["jobs"][:k]], (r, v)
                    assert q["a"][len(q) - k:].tolist() == [x for _, x in m["jobs"][:k]], (r, v)
                    first = mc.inbox_model(b.rows[i], [(-1, known)], v, now, p, room, h0.fifo_tail)
                    if first["stale_drops"]:
                        met["drain_stale"].append((r, v))  # a stale drop counted among the drained records
                    if first["retransmits"] and m["retransmits"] > first["retransmits"]:
                        met["drain_both"].append((r, v))  # jobs from the pipeline, then jobs from the packets
            if name == "s16_room" and alone and not (locked and p.lock_model):
                # no local packet: the model holds on the row round_send() left, and names the queue's end
                room = ac.room_of(dict(head=[h0.fifo_head], tail=[h0.fifo_tail], stored=[h0.fifo_stored]), 0, Q)
                m = mc.inbox_model(b.rows[i], b.inboxes[v], v, now, p, room, h0.fifo_tail)
                assert h1.fifo_tail == m["fifo_tail"] and h1.fifo_stored - h0.fifo_stored == m["stored"], (r, v)
                q = mc.queue_array(o, v)
                k = m["stored"]
                assert q["c"][len(q) - k:].tolist() == [x for x, _ in m["jobs"][:k]], (r, v)
                n = m["retransmits"]
                if 0 < room < n:
                    met["room_cut"].append((r, v))
                if room == 0 and n:
                    met["room0"].append((r, v))
                if k and h0.fifo_tail % Q + k > Q:
                    met["ring"].append((r, v))
        assert st["lock_drops"] - st0["lock_drops"] >= drops
        assert st["lock_drained"] - st0["lock_drained"] == drained
        st0 = st
    return met, o


@pytest.mark.parametrize("name", list(mc.LOCK_CASES))
def test_lock_case_guards(oracle_lib, name):
    case = mc.LOCK_CASES[name]
    met, o = lock_guard_walk(oracle_lib, name)
    n = {k: len(x) for k, x in met.items()}
    if name in ("lock40", "lock150"):
        assert min(n[k] for k in ("fits", "cut", "full", "over16", "over8", "drain_packets", "drain_alone", "drain_stale",
                                  "drain_both")) >= 3, n
        assert (n["over64"] >= 3) == (name == "lock150") and o.params.lock_buffer >= (130 if name == "lock150" else 1), n
    if name == "lock_off":
        assert n["locked_merge"] >= 10 and o.stats()["locked_merges"] > 100 and o.stats()["lock_buffered"] == 0, n
    if name == "s16_room":
        assert n["room_cut"] >= 3 and n["room0"] >= 3 and n["ring"] >= 3 and o.stats()["queue_deferred"] > 0, n
    # the locked receivers drain inside the tested window
    for _ in range(case["drain"]):  # (the walk has ended the last crafted round)
        mc.gossip_round(o)
    assert all(h.lock_buffered == 0 for h in o.hosts())
    if o.params.lock_model:
        st = o.stats()
        assert st["lock_drained"] == st["lock_buffered"] > 0
    print(f"MERGE-CASE {name}: rounds {case['first']}..{case['first'] + case['window'] - 1} {n} "
          f"lock_buffered={o.stats()['lock_buffered']} lock_drops={o.stats()['lock_drops']} "
          f"locked_merges={o.stats()['locked_merges']} queue_deferred={o.stats()['queue_deferred']}")
