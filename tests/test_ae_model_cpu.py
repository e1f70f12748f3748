"""The push-pull contract on the oracle alone (tests/ae_cases.py): exchange_model equals the oracle's
ae_merge() on every unsharded case, and each case's inputs reach what the case names (the vacuity
guards, computed from the words, the pair list and the hosts' FIFO fields), so the GPU tests that
import the same cases cannot quietly stop testing it."""
import time

import numpy as np
import pytest

from sidecar_amd.abi import ABSENT, ALIVE, DRAINING, TOMBSTONE, UNKNOWN, GxParams, default_params
from tests import ae_cases as ac
from tests.oracle_lib import load_oracle
from tests.test_shards_cpu import assert_sharded_equal

AE_GRID = 4096  # gx_kernels.hpp


def gx_epoch_of(t0_ns):
    """gx.h gx_epoch_of: the absolute time of slot time 0."""
    half = 1 << 60
    return 0 if t0_ns < half else (t0_ns - half) // 10**9 * 10**9


def ae_grid(np_, lock_model):
    """ae_grid (gx_kernels.hpp) restated: blocks of a push-pull launch."""
    if not lock_model:
        return np_
    g = min(np_, AE_GRID)
    return max(g, (np_ + 255) // 256)


def ae_round_on(lib, name, ev):
    words, hand = ac.case_views(name)
    e = ac.at_ae_round(lib, name, words, ev)
    case = ac.CASES[name]
    detail = ac.detail_pairs(name, len(ac.ae_pairs(e.params, e.round))) if case["big"] else None
    hosts = None if detail is None else [h for t in detail for h in ac.ae_pairs(e.params, e.round)[t]]
    before = ac.before_state(e, hosts)
    e.ae_merge()
    return e, words, hand, before, detail, (ac.drain_all(e, name) if ev else None)


@pytest.mark.parametrize("run", ac.RUNS, ids=ac.run_id)
def test_ae_model_and_guards(run):
    name, ev = run
    case = ac.CASES[name]
    S, H, R = case["S"], case["H"], case["R"]
    t0 = time.time()
    e, words, hand, before, detail, events = ae_round_on(load_oracle(omp=True), name, ev)
    fig = ac.check_against_model(e, name, words, before, detail, events, every_pair=not case["big"])
    p, Q = e.params, e.params.queue_cap
    pairs = before["pairs"]
    now = e.now() - e.epoch
    runs = np.array([ac.pair_runs(before, p, t) for t in range(len(pairs))])
    # the row is three tiles and a tail at least, and the hand-made pairs are the first of the round
    assert R > 3 * ac.TILE and R % ac.TILE and sorted(hand) == list(range(len(ac.HAND)))
    kinds = {k: t for t, k in hand.items()}
    models = {t: ac.exchange_model(words[a], words[b], a, b, now, p) for t, (a, b) in enumerate(pairs) if t in hand}
    # (a) every seam pair: accepts directly before and after every multiple of m, on one side each, and
    # nowhere else; every accept of a seam pair is retransmitted
    for m in ac.SEAMS:
        ma, mb = models[kinds[f"seam{m}"]]
        s = ac.seam_slots(R, m)
        assert len(s) >= 2 and np.array_equal(np.nonzero(ma["acc"] | mb["acc"])[0], s) and not (ma["acc"] & mb["acc"]).any()
        assert ma["acc"].any() and mb["acc"].any()
        assert len(ma["retx"]) == ma["ae_accepts"] and len(mb["retx"]) == mb["ae_accepts"]
    # (b) the other hand-made pairs do what they are named for
    ma, mb = models[kinds["same"]]
    a, b = pairs[kinds["same"]]
    assert ma["ae_accepts"] == mb["ae_accepts"] == 0 and ma["stale_drops"] > 0 and (ac.st_of(words[a]) == ABSENT).any()
    ma, mb = models[kinds["insert_all"]]
    assert ma["ae_accepts"] == ma["change_events"] == R and mb["ae_merges"] == 0 and (ma["events"][:, 4] == UNKNOWN).all()
    for kind, par in (("odd_keys", 1), ("even_keys", 0)):
        ma, mb = models[kinds[kind]]
        for m in (ma, mb):
            k = np.nonzero(m["acc"])[0]
            assert len(k) > R // 8 and (k % 2 == par).all()
    if S >= 2:
        ma, mb = models[kinds["last_is_older"]]
        a, b = pairs[kinds["last_is_older"]]
        for m, v, par in ((ma, a, 0), (mb, b, 1)):
            own = np.arange(H)[np.arange(H) % 2 == par]
            assert np.array_equal(m["owners_updated"], own)
            acc_ts = np.where(m["acc"], ac.ts_of(m["row"]), 0).reshape(H, S)[own]
            assert ((acc_ts > 0).sum(axis=1) == 2).all()
            assert (m["last_updated"] < acc_ts.max(axis=1)).all()  # the last key's timestamp is not the largest
        ma, mb = models[kinds["last_keeps_status"]]
        for m in (ma, mb):
            assert len(m["owners_changed"]) >= H // 2 and np.array_equal(m["owners_changed"], m["owners_updated"])
            assert (m["last_changed"] != m["last_updated"]).all()
    ma, mb = models[kinds["own_records"]]
    assert ma["ae_accepts"] == mb["ae_accepts"] == S and not len(ma["retx"]) and not len(mb["retx"])
    # (c) a seeded pair that runs has a tile with both an all-same wave and an accepting wave; statuses
    # and rules all occur among the seeded pairs that run
    mixed = drain_alive = stale_newer = equal_ts = 0
    for t, (a, b) in enumerate(pairs[:400]):
        if t in hand or not runs[t]:
            continue
        Va, Vb = words[a], words[b]
        ma, mb = ac.exchange_model(Va, Vb, a, b, now, p)
        same, acc = ac.wave_classes(Va, Vb, ma["acc"] | mb["acc"])
        mixed += bool((same.any(axis=1) & acc.any(axis=1)).any())
        pres = (ac.st_of(Va) != ABSENT) & (ac.st_of(Vb) != ABSENT)
        drain_alive += int((ma["acc"] & (ac.st_of(Va) == DRAINING) & (ac.st_of(Vb) == ALIVE)).sum())
        stale_newer += int((pres & (ac.ts_of(Vb) > ac.ts_of(Va)) & (ac.ts_of(Vb) < ac.stale_cut(now, p))).sum())
        equal_ts += int((pres & (ac.ts_of(Vb) == ac.ts_of(Va)) & (Va != Vb)).sum())
    assert mixed >= 4 and drain_alive and stale_newer and equal_ts, (mixed, drain_alive, stale_newer, equal_ts)
    sides = fig["sides"]
    cut_in = sum(1 for s in sides.values() if 0 < s["room"] < s["n"]
                 and s["model"]["retx"][s["room"] - 1] // ac.TILE == s["model"]["retx"][s["room"]] // ac.TILE)
    full = sum(1 for s in sides.values() if s["room"] == 0 and s["n"] > 0)
    ring = sum(1 for s in sides.values() if min(s["n"], s["room"]) > 0 and s["tail0"] % Q + min(s["n"], s["room"]) > Q)
    if name == "s16_room":  # (d)
        assert cut_in >= 10 and full >= 1 and ring >= 10, (cut_in, full, ring)
        assert e.stats()["queue_deferred"] > before["stats"]["queue_deferred"]
    if name == "s32_lock":  # (e)
        assert 4 * runs.sum() >= len(pairs) and 4 * (~runs).sum() >= len(pairs), runs.sum()
    if name == "s8_depart":
        assert sum(1 for a, b in pairs if before["departed"][a] or before["departed"][b]) >= 5
    if name == "s2_off":
        assert H % 2 == 1 and len(pairs) == H // 2
    if name == "s16_split":
        half = H // 2
        assert len(pairs) == half // 2 + (H - half) // 2 and all((a < half) == (b < half) for a, b in pairs)
    if name in ("s12_book", "s3_odd", "s1_chunk2") and S > 1:  # (f) an owner with accepted keys in two tiles
        n = 0
        for s in sides.values():
            k = np.nonzero(s["model"]["acc"])[0]
            o, tl = k // S, k // ac.TILE
            n += int(((o[1:] == o[:-1]) & (tl[1:] != tl[:-1])).sum())  # ... the later tile's key deciding its times
        assert n > 0
    if name == "s1_chunk2":  # (g) two pairs per block
        grid = ae_grid(len(pairs), p.lock_model)
        assert p.lock_model and R % 2 == 0 and (len(pairs) + grid - 1) // grid == 2
    if ev:  # (h) a listener overflows, one takes every event of its row
        caps = dict(ac.listener_hosts(e, name))
        assert any(len(x) == caps[v] for v, x in events.items()) and any(0 < len(x) < caps[v] for v, x in events.items())
    print(f"AE-CASE {ac.run_id(run)}: R={R} pairs={len(pairs)} run={int(runs.sum())} "
          f"accepted share={fig['accepted'] / max(1, fig['slots']):.4f} cut-in-tile={cut_in} room0={full} "
          f"ring-end={ring} locked={int(before['locked'].sum())} departed={int(before['departed'].sum())} "
          f"seconds={time.time() - t0:.1f}")


def test_case_table_matches_the_kernel_selection():
    """Each case's parameters select the kernel its row names (ae_whole_impl's rules, restated)."""
    for name, c in ac.CASES.items():
        p, vec = c["params"], c["R"] % 2 == 0
        chunk = vec and bool(p["lock_model"])
        assert chunk == ("k_ae_chunk" in c["runs"]), name
        assert ("k_ae<false>" in c["runs"]) == (not vec), name
        if "ae_book" in c["runs"]:
            assert c["S"] < 2 or 128 % c["S"] or not vec, name
        elif "k_ae<true>" in c["runs"]:
            assert 128 % c["S"] == 0 and c["S"] >= 2, name


@pytest.mark.parametrize("name", ["s16_off", "s3_odd"])
def test_merge_model(oracle_lib, name):
    """exchange_model(both=False) equals gx_merge(dst, src) on the oracle: the hand-made pairs one way
    each, then seeded (dst, src), each on the rows the merges before it left."""
    words, hand = ac.case_views(name)
    e = ac.at_ae_round(oracle_lib, name, words, ev=True)
    want = run_merges(e, e, name, np.array(words))
    check_merge_events(e, name, want, ac.drain_all(e, name))


def run_merges(g, o, name, cur, n_seeded=100):
    """gx_merge on engines g and o (the same engine twice on the CPU) against the model: views and
    counters of g. Returns {dst: the model's events of its merges, in call order}."""
    p = o.params
    now = o.now() - o.epoch
    pairs = ac.ae_pairs(p, o.round)
    rng = np.random.default_rng(11)
    todo = [pairs[t] for t in sorted(ac.case_views(name)[1])] + \
        [tuple(int(x) for x in rng.choice(o.H, size=2, replace=False)) for _ in range(n_seeded)]
    st0 = g.stats()
    tot = dict.fromkeys(ac.COUNTERS + ("retransmits", "ae_slots"), 0)
    want_ev = {}
    for dst, src in todo:
        for e in {id(g): g, id(o): o}.values():
            e.merge(dst, src)
        (m,) = ac.exchange_model(cur[dst], cur[src], dst, src, now, p, both=False)
        cur[dst] = m["row"]
        for c in ac.COUNTERS:
            tot[c] += m[c]
        tot["retransmits"] += len(m["retx"])
        tot["ae_slots"] += len(m["row"])
        want_ev.setdefault(dst, []).append(m["events"])
    assert np.array_equal(g.read_views(), cur), f"{name}: views after {len(todo)} gx_merge calls differ from the model"
    st1 = g.stats()
    for c, want in tot.items():
        assert st1[c] - st0[c] == want, f"{name}: {c} grew by {st1[c] - st0[c]}, the model says {want}"
    assert tot["ae_accepts"] > 1000 and tot["stale_drops"] > 1000
    return want_ev


def check_merge_events(e, name, want_ev, events):
    """The drained events {host: tuples} of run_merges' calls equal the model's, cut at the capacity."""
    assert any(events.values())
    for v, evs in events.items():
        cap = dict(ac.listener_hosts(e, name))[v]
        want = np.concatenate(want_ev.get(v, []) + [np.zeros((0, 6), dtype=np.int64)]) + np.array([0, 0, e.epoch, 0, 0, e.epoch])
        got = np.array(evs, dtype=np.int64).reshape(-1, 6)
        assert len(got) == min(cap, len(want)) and np.array_equal(got, want[:len(got)]), f"{name}: listener of {v}"


def test_exchange_model_by_hand():
    """The model on hand-written words: one owner pair, S = 4, every rule once."""
    p = GxParams(n_hosts=3, n_services=4, tombstone_lifespan_ns=1000, stale_fudge_ns=100)
    now = 10_000  # stale below 8900

    def w(ts, st):
        return (ts << 3) | st
    A = 7
    #          host 0 (a's own)                    host 1 (b's own)                     host 2
    Va = [w(9000, 0), A, w(9500, 4), w(9100, 1), w(9000, 0), w(9000, 0), A, A, w(9300, 0), w(9200, 2), w(5000, 0), A]
    Vb = [w(9100, 0), w(9000, 2), w(9600, 0), w(9100, 0), w(9000, 1), A, A, w(8000, 0), w(9200, 1), w(9400, 2), w(6000, 0), A]
    ma, mb = ac.exchange_model(np.array(Va, dtype=np.uint64), np.array(Vb, dtype=np.uint64), 0, 1, now, p)
    # a: key 0 newer (own), key 1 insert (own), key 2 ALIVE onto DRAINING stays DRAINING, key 3 equal
    # timestamp, key 4 equal, key 7 stale, key 8 older, key 9 newer with the same status, key 10 stale
    assert ma["row"].tolist() == [w(9100, 0), w(9000, 2), w(9600, 4), w(9100, 1), w(9000, 0), w(9000, 0), A, A,
                                  w(9300, 0), w(9400, 2), w(5000, 0), A]
    assert (ma["ae_merges"], ma["stale_drops"], ma["ae_accepts"], ma["change_events"]) == (9, 2, 4, 1)
    assert ma["retx"].tolist() == [9]
    assert ma["owners_updated"].tolist() == [0, 2] and ma["last_updated"].tolist() == [9600, 9400]
    assert ma["owners_changed"].tolist() == [0] and ma["last_changed"].tolist() == [9000]
    assert ma["state_last_changed"] == 9000 and ma["events"].tolist() == [[0, 1, 9000, 2, UNKNOWN, 9000]]
    # b reads a's words as they were: key 5 insert (own), key 8 newer with another status; key 10 stale
    assert mb["row"].tolist() == [w(9100, 0), w(9000, 2), w(9600, 0), w(9100, 0), w(9000, 1), w(9000, 0), A, w(8000, 0),
                                  w(9300, 0), w(9400, 2), w(6000, 0), A]
    assert (mb["ae_merges"], mb["stale_drops"], mb["ae_accepts"], mb["change_events"]) == (8, 1, 2, 2)
    assert mb["retx"].tolist() == [8] and mb["state_last_changed"] == 9300
    assert mb["events"].tolist() == [[1, 1, 9000, 0, UNKNOWN, 9000], [2, 0, 9300, 0, TOMBSTONE, 9300]]


# -------------------------------------------------------------------------------- sharded cases --
def plan_launches(pairs, H, G):
    """Per shard (cross, local): the entries of its two push-pull launches, the cross pairs' sides it
    holds (launched by gx_ae_merge) and its local pairs (gx_ae_merge_local)."""
    n = [[0, 0] for _ in range(G)]
    for a, b in pairs:
        ga, gb = a * G // H, b * G // H
        if ga == gb:
            n[ga][1] += 1
        else:
            n[ga][0] += 1
            n[gb][0] += 1
    return n


@pytest.mark.parametrize("name", [n for n, c in ac.SHARDED.items() if not c["big"]])
def test_sharded_cases_on_the_oracle(oracle_lib, name):
    """Oracle shards against the unsharded oracle and the model on the cases' written views."""
    case = ac.SHARDED[name]
    H, G, R = case["H"], case["cross"], case["R"]
    words, hand = ac.case_views(name)
    whole = ac.at_ae_round(oracle_lib, name, words)
    sh = ac.sharded_at_ae_round(oracle_lib, name, words)
    sx = ac.Sharded(sh)
    pairs = ac.ae_pairs(whole.params, whole.round)
    detail = sorted(hand)
    before = ac.before_state(sx, [h for t in detail for h in pairs[t]])
    whole.ae_merge()
    whole.round_end()
    sh.round_finish(True)
    assert_sharded_equal(whole, sh, f"{name} after the push-pull round")
    ac.check_against_model(sx, name, words, before, detail, every_pair=False)
    print(f"AE-CASE {name}: R={R} G={G} pairs={len(pairs)} launches (cross, local)={plan_launches(pairs, H, G)} "
          f"cross={sum(1 for a, b in pairs if a * G // H != b * G // H)}")


@pytest.mark.parametrize("name", list(ac.SHARDED))
def test_cross_pairs_reach_their_blocks(name):
    """The hand-made cross pairs of every sharded case, from the written words alone (digest, leads and
    own_ok of tests/test_wire_format.py, which that file pins to the engines' messages): their tiles
    hold every mix of block classes named, and their return blocks the literal positions named."""
    case = ac.SHARDED[name]
    H, G, R = case["H"], case["cross"], case["R"]
    words, hand = ac.case_views(name)
    p = default_params(load_oracle(), **case["params"])
    pairs = ac.ae_pairs(p, case["ae_round"])
    now = p.t0_ns + case["ae_round"] * p.round_ns - gx_epoch_of(p.t0_ns)
    # per cross pair (a's view; b's mirrors it): the class of each digest block, the return literals
    cls, lits = {}, {}
    for t, kind in hand.items():
        if kind in ac.CROSS_HAND and t >= len(ac.HAND):
            a, b = pairs[t]
            assert a * G // H != b * G // H
            cls[kind] = ac.block_classes(words[a], words[b])
            lits[kind] = [ac.return_literals(words[a], words[b], blk, now, p) for blk in range(len(cls[kind]))]
    assert sorted(cls) == sorted(ac.CROSS_HAND)
    nblk = (R + ac.BLK - 1) // ac.BLK
    tail = R - (nblk - 1) * ac.BLK
    assert 0 < tail < ac.BLK and nblk >= 6  # a last block shorter than 512 slots
    tiles = {k: [tuple(c[i:i + 2]) for i in range(0, nblk, 2)] for k, c in cls.items()}
    led = {k: [bool(x) for x in c] for k, c in cls.items()}
    assert led["block1"] == [False, True] + [False] * (nblk - 2)           # equal except block 1: tile (matched, differs)
    assert led["tile_orders"][:4] == [True, False, False, True] and sum(led["tile_orders"]) == 2  # and (differs, matched)
    assert (0, 0) in tiles["block1"] and (0, 0) in tiles["tile_orders"]   # a tile with both blocks matched
    # own masks with the only literal at the block's first / last slot
    assert led["edge_literals"] == [False, True, True] + [False] * (nblk - 3)
    assert lits["edge_literals"][1] == [0] and lits["edge_literals"][2] == [ac.BLK - 1]
    # the short last block as a return block with literals, up to its last even slot
    assert led["tail_block"] == [False] * (nblk - 1) + [True]
    assert lits["tail_block"][-1] == list(range(0, tail, 2))
    # return blocks with no literal (the all-own mask) and with many
    assert lits["tile_orders"][0] == [] and len(lits["tile_orders"][3]) > 100 and len(lits["block1"][1]) > 100
    # led by this side beside led by the partner, and matched beside led by the partner (side b sees
    # every class mirrored: 1 <-> 2)
    assert tiles["lead_both"][0] == (2, 1) and tiles["lead_both"][1] == (0, 1)
    assert not any(cls["same"])


def test_pf1_case_fills_the_plan():
    """x_s2_pf1_g2: every shard has a launch of at least 1024 plan entries (k_ae_plan with PF = 1; below
    that k_ae_plan_pf2), counted from the pair list and the shard bounds; every launch of the smaller
    sharded cases stays below."""
    lib = load_oracle()
    for name, case in ac.SHARDED.items():
        p = default_params(lib, **case["params"])
        n = plan_launches(ac.ae_pairs(p, case["ae_round"]), case["H"], case["cross"])
        assert all(max(x) >= 1024 for x in n) if case["big"] else all(max(x) < 1024 for x in n), (name, n)
