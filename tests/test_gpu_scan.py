"""The lifespan scan (expiry_word, scan_view, scan_chunk_waves, k_scan, k_scan_split, k_scan_join,
k_bt_finish, the scan prologue of k_send, gx_tombstone_others) on hand-made rows: the cases of
tests/scan_cases.py (DESIGN.md "Expiry scan contract"), compared with the oracle bit for bit and with
the numpy restatement scan_cases.scan_model, in the scan round, at its end and 12 rounds later. Every
case asserts the placement that ran from gx_timing.launches. tests/test_scan_model_cpu.py holds the
guards that keep each case on the seams it names."""
import numpy as np
import pytest

from sidecar_amd.abi import TOMBSTONE
from tests import scan_cases as sc
from tests.oracle_lib import load_oracle
from tests.parity import assert_same
from tests.storm_cases import assert_same_after_send, queue_array

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc_lib():
    return load_oracle(omp=True)


def same_queues(g, o, hosts, what):
    for v in hosts:
        assert np.array_equal(queue_array(g, v), queue_array(o, v)), f"{what}: queue of host {v}"


@pytest.mark.parametrize("run", sc.RUNS, ids=sc.run_id)
def test_scan_case(gx_lib, orc_lib, run):
    name, ev = run
    case = sc.CASES[name]
    what = sc.run_id(run)
    g, b, before, detail, g_ev = sc.scan_round_on(gx_lib, name, ev, device=0)
    o, _, _, _, o_ev = sc.scan_round_on(orc_lib, name, ev)
    # the placement: one launch of the k_scan class (k_scan, or k_scan_split + k_scan_join), or none
    # and the scan in k_send
    launched = g.timing()["scan"]["launches"] - before["launches"]
    assert launched == (1 if sc.path_of(case, ev)[0] == "scan" else 0), f"{what}: {launched} k_scan launches"
    assert_same_after_send(g, o, f"{what} after round_send")
    if ev:
        for v in g_ev:
            assert g_ev[v] == o_ev[v], f"{what}: listener of host {v}: {len(g_ev[v])} events, the oracle {len(o_ev[v])}"
    same_queues(g, o, detail, what)
    if case["model"]:
        sc.check_against_model(g, name, b, before, detail, g_ev)
    for e in (g, o):
        sc.finish_round(e)
    assert_same(g, o, f"{what} at the scan round's end")
    # the later deadlines (3, 5 and 7 rounds on) fall only if the scan left the exact expiry bound
    for e in (g, o):
        sc.follow_up(e)
    assert_same(g, o, f"{what} {sc.FOLLOW_UP} rounds after the scan round")
    same_queues(g, o, detail, what + " later rounds")
    if ev:
        ge, oe = sc.drain_all(g, b), sc.drain_all(o, b)
        for v in ge:
            assert ge[v] == oe[v], f"{what} later rounds: listener of host {v}"


@pytest.mark.parametrize("name", sc.API_CASES)
def test_tombstone_others(gx_lib, orc_lib, name):
    """gx_tombstone_others on the hand-made rows, capacities below, at and above the expirations: the
    returned records and n_out against the oracle and the model (cut at the caller's cap, not at L), a
    listener's events, and parity of the state after the calls and 12 rounds on."""
    case = sc.CASES[name]
    b = sc.case_round(name)
    es = []
    for lib, dev in ((gx_lib, 0), (orc_lib, None)):
        e = sc.make_engine(lib, case, dev)
        sc.warm_up(e, case)
        e.write_views(b.words, e.lo)
        for v, cap in sc.listener_views(b)[:4]:
            e.add_listener(v, 1, cap)
        es.append(e)
    g, o = es
    calls, want = sc.api_calls(g, name), sc.api_calls(o, name)
    assert calls == want, f"{name}: gx_tombstone_others differs from the oracle"
    S, p = case["S"], g.params
    after = g.read_views()
    for v, cap, recs, n_out in calls:
        m = sc.scan_model(b.words[v - g.lo], v, b.now, p, max(cap, 1), np.zeros(g.H, dtype=bool))
        assert n_out == m["expired"] and len(recs) == min(cap, n_out), (name, v, cap)
        assert recs == [((w >> 3) + g.epoch, k // S, k % S, TOMBSTONE) for k, w in m["list"][:cap]], (name, v, cap)
        assert np.array_equal(after[v - g.lo], m["row"]), (name, v)
    for v, _ in sc.listener_views(b)[:4]:
        ge = [x.tup() for x in g.drain_listener(v, 1, 16384)]
        assert ge == [x.tup() for x in o.drain_listener(v, 1, 16384)], f"{name}: listener of host {v}"
    assert_same(g, o, f"{name} after gx_tombstone_others")
    for e in es:
        sc.follow_up(e)
    assert_same(g, o, f"{name} {sc.FOLLOW_UP} rounds after gx_tombstone_others")
