"""The expiry scan contract on the oracle alone (tests/scan_cases.py): scan_model equals the oracle's
scan_view and bt_tick on every case, and each case's rows reach what the case names (the vacuity
guards, computed from the written rows, the model and the hosts' bookkeeping), so the GPU tests that
import the same cases cannot quietly stop testing it."""
import time

import numpy as np
import pytest

from sidecar_amd.abi import ALIVE, DRAINING, SLOT_ABSENT, TOMBSTONE, UNHEALTHY, UNKNOWN, GxParams
from tests import scan_cases as sc
from tests.ae_cases import pack, st_of, ts_of
from tests.oracle_lib import load_oracle


def crossing(case, geo, a, b):
    """Where two consecutive list positions fall relative to the scan's units."""
    if case["nch"] > 1:
        ca, cb = a // geo["clen"], b // geo["clen"]
        if ca != cb:
            return "chunk"
        n = min((ca + 1) * geo["clen"], case["R"]) - ca * geo["clen"]
        q = sc.wave_quarter(n)
        return "quarter" if (a - ca * geo["clen"]) // q != (b - cb * geo["clen"]) // q else "inside"
    if a // sc.TILE != b // sc.TILE:
        return "tile"
    if a // sc.HALF != b // sc.HALF:
        return "half"
    if a // sc.WAVE != b // sc.WAVE:
        return "waves"
    return "pair" if a // 2 == b // 2 else "wave"


def seam_guard(case, b, kind, m, L, v):
    """What hand-made kind `kind` must hold, from its model m."""
    S, R, keys = case["S"], case["R"], m["keys"]
    n = m["expired"]
    hit = np.zeros(R + 2, dtype=bool)
    hit[keys] = True
    if kind in ("seam128", "seam512", "seam1024", "tiles256", "halves128"):
        step = {"seam128": 128, "seam512": 512, "seam1024": 1024, "tiles256": 256, "halves128": 256}[kind]
        pts = np.arange(128 if kind == "halves128" else step, R - 2, step)
        pts = pts[((pts - 2) // S != v) & ((pts + 1) // S != v)]  # (not the seams inside the viewer's own slots)
        # at least three of the four keys around every inner seam expire (one is the GC tombstone, one
        # may be the viewer's own), on both sides of it, and nothing else in the row does
        near = hit[pts - 2].astype(int) + hit[pts - 1] + hit[pts] + hit[pts + 1]
        assert (near >= 2).all() and (near >= 3).mean() > 0.9, kind
        assert ((hit[pts - 2] | hit[pts - 1]) & (hit[pts] | hit[pts + 1])).mean() > 0.9, kind
        assert n <= 3 * (len(pts) + 1) and m["gc"] >= len(pts) // 2, kind
    if kind == "pairs":
        pr = hit[:600].reshape(-1, 2)
        assert pr[:, 0].any() and pr[:, 1].any() and (pr[:, 0] & pr[:, 1]).any() and (pr[:, 0] & ~pr[:, 1]).any() \
            and (~pr[:, 0] & pr[:, 1]).any() and hit[R - 64:R].any()
    if kind in ("row_end", "last_slot"):
        assert keys.tolist() == [R - 1]
    if kind == "gc_only":
        assert n == 0 and m["gc"] > 3
    if kind in ("owner_even", "owner_odd"):
        last = {}
        for k in keys.tolist():
            last[k // S] = k
        par = np.array(list(last.values())) % 2
        assert len(last) > case["H"] // 3 and (par == (kind == "owner_odd")).mean() > (0.45 if S % 2 else 0.95), kind
    if kind.startswith("straddle"):
        ms = np.array([x for x in range(sc.TILE, R, sc.TILE) if x % S])
        lo_side = np.array([hit[x // S * S:x].any() for x in ms])
        hi_side = np.array([hit[x:(x // S + 1) * S].any() for x in ms])
        want = {"both": (True, True), "first": (True, False), "second": (False, True)}[kind.split("_")[1]]
        assert len(ms) and (lo_side == want[0]).all() and (hi_side == want[1]).all(), kind
    if kind.startswith("cap_") and case["nch"] == 1:
        _, cross, cnt = kind.split("_")
        assert n == {"less": L - 1, "exact": L, "plus1": L + 1, "three": 3 * L + 5}[cnt], (kind, n, L)
        if n > L:
            assert crossing(case, b.geo, int(keys[L - 1]), int(keys[L])) == cross, kind
    if case["nch"] > 1:
        nc, clen = b.geo["nc"], b.geo["clen"]
        per = np.bincount(keys // clen, minlength=nc)
        if kind == "chunks":
            assert (per > 0).all() and n <= 3 * (nc - 1) and all(hit[c * clen - 1] or hit[c * clen - 2] for c in range(1, nc))
        if kind in ("quarters", "second_tile", "tiles256", "halves128"):
            assert (per > 0).all()
        if kind == "chunk_gap":
            assert per[0] > 0 and per[1] == 0 and per[-1] == 0 and (nc < 4 or per[2] > 0)
        if kind == "last_slot":
            assert per[-1] == 1 and per.sum() == 1
        if kind == "cap_quarter":
            assert n == 2 * L + 1 and crossing(case, b.geo, int(keys[L - 1]), int(keys[L])) == "quarter"
        if kind == "cap_chunk":
            assert n == 3 * L + 5 and crossing(case, b.geo, int(keys[L - 1]), int(keys[L])) == "chunk"
        if kind == "cap_exact":
            assert n == L and keys[-1] == clen - 1
        if kind == "cap_less":
            assert n == L - 1


@pytest.mark.parametrize("run", sc.RUNS, ids=sc.run_id)
def test_scan_model_and_guards(run):
    name, ev = run
    case = sc.CASES[name]
    S, R = case["S"], case["R"]
    t0 = time.time()
    e, b, before, detail, events = sc.scan_round_on(load_oracle(omp=True), name, ev)
    p = e.params
    L = p.packet_cap + p.pending_cap
    Hl = e.hi - e.lo
    gone = np.array([p.depart_round >= 0 and sc.departed(p, o) for o in range(e.H)])
    if case["model"]:
        models = sc.check_against_model(e, name, b, before, detail, events)
    else:
        models = {v: sc.scan_model(b.words[v - e.lo], v, b.now, p, L, gone) for v in detail}
    # the rig: every hand-made kind has a ticking view, three quarters of the local views tick, the
    # path the case names follows from its sizes
    assert len(b.hand) == b.n_kinds and all(b.tick[v - e.lo] for v in b.hand)
    assert b.tick.sum() * 4 >= 3 * Hl
    place, kernel = sc.path_of(case, ev)
    assert place == case["place"]
    assert kernel == {"w": "block-wave", "l": "block-lds", "o": "scalar", "c": "block-wave", "b": "block-wave",
                      "d": "block-wave"}.get(name[0], kernel)
    if name[0] == "x":
        assert kernel == ("block-wave" if ev else "split") and case["nch"] >= 2
        listed = sum(1 for v, k in b.last.items() if k >= 0 and b.tick[v - e.lo])  # the round's worklist
        assert b.geo == sc.case_geo(case, listed)
        # fewer chunks than the tables' stride only where the case says so (a long worklist)
        assert (b.geo["nc"] < case["nch"]) == (name == "x_few") and (name != "x_few" or b.geo["nc"] >= 3)
        assert b.geo["nc"] * b.geo["clen"] >= R > (b.geo["nc"] - 1) * b.geo["clen"]
        if name == "x_1026":
            assert R % (1024 * b.geo["nc"]) and R - (b.geo["nc"] - 1) * b.geo["clen"] < b.geo["clen"]
    if name[0] == "p":
        assert kernel == ("fused" if S <= 16 else "prologue") and case["warm"] >= 8
        # nothing expired in the warm rounds (their rows are the warm start's): no view was scanned
        assert before["stats"]["expired"] == 0 and before["stats"]["gc"] == 0
    if name[0] in "wlo":
        assert R > 2 * sc.TILE and R % sc.HALF and (R % 2 == 1) == (name[0] == "o")
    # the seams, kind by kind; the values every hand-made row holds
    kind_of = {k: v for v, k in b.hand.items()}
    for kind, v in kind_of.items():
        m = models[v]
        seam_guard(case, b, kind, m, L, v)
        row = b.words[v - e.lo]
        other = np.ones(R, dtype=bool)
        other[v * S:(v + 1) * S] = False
        st, ts = st_of(row[other]), ts_of(row[other])
        assert {ALIVE, UNHEALTHY, UNKNOWN, DRAINING, TOMBSTONE} <= set(np.unique(st[row[other] != SLOT_ABSENT]).tolist())
        assert (row[other] == SLOT_ABSENT).any()
        c = sc.ctx_of(e, case, b, v)
        q = sc.quiet_for(c, b.last[v])
        lk = sc.later_keys(c, b.last[v])
        for life, stays, goes in ((p.alive_lifespan_ns, q[0][0], 0), (p.draining_lifespan_ns, q[1][0], 1),
                                  (p.tombstone_lifespan_ns, q[2][0], None)):
            if stays // S != v:  # exactly on the lifespan: stays, and bounds the row's next deadline
                assert ts_of(row[stays:stays + 1])[0] == b.now - life and m["row"][stays] == row[stays]
        if m["expired"] >= 2 and not kind.startswith("straddle"):
            k0, k1 = m["keys"][:2]  # one tick past the lifespan: goes
            assert ts_of(row[k0:k0 + 1])[0] == b.now - p.alive_lifespan_ns - 1
            assert row[k1] == pack(b.now - p.draining_lifespan_ns - 1, DRAINING)
        if m["expired"] and q[0][2] // S != v:  # a record that already equals the first expiry's new word
            assert row[q[0][2]] == m["row"][m["keys"][0]] or st_of(row[m["keys"][:1]])[0] != ALIVE
        if all(k // S != v for k in lk) and all(k // S != v for k in (q[0][0], q[1][0], q[2][0])):
            assert m["deadline"] == b.now  # the records exactly on their lifespan: the row is scanned next round
        if case["nch"] > 1 and b.last[v] >= 0:  # the later deadlines sit in other chunks than the last expiry
            assert all(k // b.geo["clen"] != b.last[v] // b.geo["clen"] for k in lk), kind
    # list capacity: crossed and not crossed among the hand-made rows; the count-only tail
    ns = [models[v]["expired"] for v in b.hand]
    assert any(n > L for n in ns) and any(0 < n <= L for n in ns)
    if name in ("d_s16", "x_dep"):  # departed and live owners' records expire, on both sides of some seam
        assert gone.sum() > 10 and gone[e.lo:e.hi].any() and not b.tick[np.nonzero(gone[e.lo:e.hi])[0]].any()
        m = models[kind_of["seam128" if name == "d_s16" else "halves128"]]
        go = gone[m["keys"] // S]
        assert go.any() and not go.all() and m["false_expiries"] == (~go).sum()
        pts = np.arange(128, R - 2, 128)
        assert (gone[(pts - 1) // S] != gone[pts // S]).any()
    if ev:
        caps = dict(sc.listener_views(b))
        evs = {v: len(models[v]["events"]) for v in caps}
        assert any(evs[v] > caps[v] for v in caps) and any(0 < evs[v] <= caps[v] for v in caps)
        if case["model"]:
            assert all(len(events[v]) == min(caps[v], evs[v]) for v in caps)
    # the round's end and the follow-up rounds: the later deadlines fall
    sc.finish_round(e)
    sc.follow_up(e)
    after = e.read_views()
    hs = e.hosts()
    fell, lagged = 0, []
    for v in b.hand if name != "b_storm" else ():
        c = sc.ctx_of(e, case, b, v)
        row, ok = after[v - e.lo], True
        for k, want in zip(sc.later_keys(c, b.last[v]), (TOMBSTONE, None, TOMBSTONE)):
            if k // S == v:
                continue
            # (every row holds these records, so a peer's tombstone, up to tombstone_count passes of
            # pass_increment_ns later, may have replaced the view's own)
            d = ts_of(row[k:k + 1])[0] - ts_of(b.words[v - e.lo][k:k + 1])[0] - p.tombstone_bump_ns
            ok &= row[k] == SLOT_ABSENT if want is None else \
                bool(st_of(row[k:k + 1])[0] == want and 0 <= d <= p.tombstone_count * p.pass_increment_ns)
        # a looper whose nil waits behind a long queue does not tick: only such a view may lag
        h = hs[v - e.lo]
        assert ok or (h.flags & 3 and h.fifo_tail != h.fifo_head), (name, v, b.hand[v])
        fell += ok
        if not ok:
            lagged.append(b.hand[v])
    assert name == "b_storm" or fell * 4 >= 3 * len(b.hand), (name, fell)
    # the kinds whose expiry bound has to survive a seam never lag: only rows with long lists may
    # (cap512: lists of 512 records keep every view's queue long, whatever its own row holds)
    assert name == "cap512" or \
        not [k for k in lagged if not k.startswith(("cap_", "owner_", "pairs", "tiles256", "halves128"))], lagged
    n_hand = {b.hand[v]: models[v]["expired"] for v in sorted(b.hand)}
    print(f"SCAN-CASE {sc.run_id(run)}: S={S} H={case['H']} R={R} shard {case['g']}/{case['G']} Hl={Hl} L={L} "
          f"path={place}/{kernel} chunks={b.geo['nc']} clen={b.geo['clen']} ticking={int(b.tick.sum())} "
          f"expirations={n_hand} lagged={lagged} seconds={time.time() - t0:.1f}")


def test_scan_model_by_hand():
    """The model on hand-written words: viewer 0 of 3 hosts, S = 2, every rule once."""
    p = GxParams(n_hosts=3, n_services=2, alive_lifespan_ns=100, draining_lifespan_ns=1000, tombstone_lifespan_ns=5000,
                 tombstone_bump_ns=10, packet_cap=1, pending_cap=1)
    now = 10_000

    def w(ts, st):
        return (ts << 3) | st
    A = SLOT_ABSENT
    #      own         owner 1                                  owner 2
    row = [w(9990, ALIVE), A, w(9900, ALIVE), w(9899, UNHEALTHY), w(8999, DRAINING), w(4999, TOMBSTONE)]
    m = sc.scan_model(np.array(row, dtype=np.uint64), 0, now, p, 2, [False, False, True])
    assert m["row"].tolist() == [w(9990, ALIVE), A, w(9900, ALIVE), w(9909, TOMBSTONE), w(9009, TOMBSTONE), A]
    assert (m["expired"], m["gc"], m["false_expiries"], m["written"]) == (2, 1, 1, 3)
    assert m["list"] == [(3, w(9909, TOMBSTONE)), (4, w(9009, TOMBSTONE))] and m["times"] == {1: 9909, 2: 9009}
    assert m["state_last_changed"] == 9009 and m["deadline"] == 10_000  # key 2: 9900 + 100
    assert m["events"].tolist() == [[1, 1, 9909, TOMBSTONE, UNHEALTHY, 9909], [2, 0, 9009, TOMBSTONE, DRAINING, 9009]]
    m1 = sc.scan_model(np.array(row, dtype=np.uint64), 0, now, p, 1, [False] * 3)
    assert m1["list"] == [(3, w(9909, TOMBSTONE))] and m1["expired"] == 2 and m1["state_last_changed"] == 9009
    # UNKNOWN takes the alive lifespan; one tick later key 2 goes
    m2 = sc.scan_model(np.array([A, A, w(9900, UNKNOWN), A, A, A], dtype=np.uint64), 0, now + 1, p, 2, [False] * 3)
    assert m2["keys"].tolist() == [2] and m2["deadline"] == 9910 + 5000


def test_scan_geometry_restated():
    """scan_chunks and the wave quarters for the row lengths of the split cases; a chunk is never short
    enough for an empty wave quarter (DESIGN.md "Expiry scan contract")."""
    assert sc.scan_nch(65536, 16) == 2 and sc.scan_nch(65535 * 2, 2) == 3 and sc.scan_nch(524288, 64) == 16
    assert sc.scan_nch(65536, 3) == 1 and sc.scan_nch(65536, 1) == 1 and sc.scan_nch(65534, 2) == 1
    assert sc.scan_chunks(65664, 13, 2) == (2, 33792) and sc.scan_chunks(131072, 683, 4) == (3, 44032)
    assert sc.scan_chunks(131072, 682, 4) == (4, 32768) and sc.scan_chunks(65536, 2048, 2) == (1, 65536)
    for R in range(65536, 65536 * 17, 4096 + 64):
        for nch in range(1, sc.scan_nch(R, 64) + 1):
            nc, clen = sc.scan_chunks(R, max(1, sc.SCAN_ITEMS // nch), sc.scan_nch(R, 64))
            last = R - (nc - 1) * clen
            assert 0 < last <= clen and 3 * sc.wave_quarter(last) < last


@pytest.mark.parametrize("name", sc.API_CASES)
def test_api_model(oracle_lib, name):
    """gx_tombstone_others on the hand-made rows: n_out, the records cut at the caller's cap (not at L),
    the row."""
    case = sc.CASES[name]
    b = sc.case_round(name)
    e = sc.make_engine(oracle_lib, case)
    sc.warm_up(e, case)
    e.write_views(b.words, e.lo)
    p = e.params
    L = p.packet_cap + p.pending_cap
    calls = sc.api_calls(e, name)
    after = e.read_views()
    seen = set()
    for v, cap, recs, n_out in calls:
        m = sc.scan_model(b.words[v - e.lo], v, b.now, p, max(cap, 1), np.zeros(e.H, dtype=bool))
        assert n_out == m["expired"] and len(recs) == min(cap, n_out), (name, v, cap)
        want = [((w >> 3) + e.epoch, k // case["S"], k % case["S"], TOMBSTONE) for k, w in m["list"][:cap]]
        assert recs == want, (name, v, cap)
        assert np.array_equal(after[v - e.lo], m["row"]), (name, v)
        seen.add("below" if cap < n_out else "at" if cap == n_out else "above")
        if cap > L and n_out > L:
            seen.add("past L")
    assert seen >= {"below", "at", "above"}, seen
    assert "past L" in seen or name != "w_s16"
