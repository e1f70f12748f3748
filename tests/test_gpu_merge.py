"""The gossip receive phase (k_inbox_unpack, k_merge_seg, merge_seg<16>, merge_seg<32>, merge_receiver,
merge_inbox_serial, lock_append_seg) on hand-made inboxes: the cases of tests/merge_cases.py, one shard
whose received packets the test writes record by record (DESIGN.md "Gossip merge contract"), compared
with the oracle bit for bit and with the sequential model of merge_cases.inbox_model.
tests/test_merge_model_cpu.py holds the guards that keep each case on the paths it names."""
import numpy as np
import pytest

from tests import merge_cases as mc
from tests.oracle_lib import load_oracle
from tests.parity import assert_same
from tests.storm_cases import queue_array
from tests.test_merge_model_cpu import merge_round_on

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def orc_lib():
    return load_oracle()


def same_events(g, o, b, what):
    ge, oe = mc.drain_all(g, b), mc.drain_all(o, b)
    for v in ge:
        assert ge[v] == oe[v], f"{what}: listener of host {v}: {len(ge[v])} events, the oracle {len(oe[v])}"
    return ge


def same_queues(g, o, hosts, what):
    for v in hosts:
        assert np.array_equal(queue_array(g, v), queue_array(o, v)), f"{what}: queue of host {v}"


@pytest.mark.parametrize("run", mc.RUNS, ids=mc.run_id)
def test_merge_case(gx_lib, orc_lib, run):
    name, ev = run
    what = mc.run_id(run)
    g, b, before, detail, g_ev, keep = merge_round_on(gx_lib, name, ev, device=0)
    o, _, _, _, o_ev, _ = merge_round_on(orc_lib, name, ev)
    assert_same(g, o, f"{what} after round_merge")
    if ev:
        for v in g_ev:
            assert g_ev[v] == o_ev[v], f"{what}: listener of host {v}: {len(g_ev[v])} events, the oracle {len(o_ev[v])}"
    # the hand-made receivers and 16 seeded others: the queues, tuple for tuple
    same_queues(g, o, detail, what)
    # every receiver's row and the counters; the receivers in detail: times, queue, events
    mc.check_against_model(g, name, b, before, detail, g_ev)
    del keep
    # a wrong job only shows once it is sent
    for e in (g, o):
        e.round_end()
        for _ in range(12):
            mc.gossip_round(e)
    assert_same(g, o, f"{what} 12 rounds after the crafted round")
    same_queues(g, o, detail, what + " later rounds")
    if ev:
        same_events(g, o, b, what + " later rounds")


@pytest.mark.parametrize("name", list(mc.LOCK_CASES))
def test_lock_case(gx_lib, orc_lib, name):
    """The lock and queue cases: local traffic present, crafted inboxes for six rounds in a row built
    from the oracle's state after round_send(); parity after every crafted round (the pipeline records
    are part of the host digests), the crafted receivers' queues tuple for tuple, and again once the
    locked receivers have drained."""
    case = mc.LOCK_CASES[name]
    g, o = mc.make_lock_engine(gx_lib, name, device=0), mc.make_lock_engine(orc_lib, name)
    for r, b in mc.lock_rounds(o, [(g, mc.device_buffer)], name):
        what = f"{name} round {r}"
        assert_same(g, o, what + " after round_merge")
        same_queues(g, o, [v for v, kind in b.kinds.items() if kind != "seeded"], what)
    for e in (g, o):  # (the walk has ended the last crafted round)
        for _ in range(case["drain"]):
            mc.gossip_round(e)
    assert_same(g, o, f"{name} after the drain")
    assert all(h.lock_buffered == 0 for h in g.hosts())
    same_queues(g, o, range(g.lo, g.hi), name + " after the drain")
