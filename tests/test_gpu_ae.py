"""The push-pull kernels (ae_pair behind k_ae, k_ae_ev, k_ae_chunk, k_merge_views and the k_ae_plan
kernels) on sparse pairs: the cases of tests/ae_cases.py, whose rows cross every seam of the kernel
(DESIGN.md "Push-pull contract"), compared with the oracle bit for bit and with the numpy model of
ae_cases.exchange_model. tests/test_ae_model_cpu.py holds the guards that keep each case on the paths
it names."""
import numpy as np
import pytest

from tests import ae_cases as ac
from tests.oracle_lib import load_oracle
from tests.parity import assert_same
from tests.test_ae_model_cpu import check_merge_events, run_merges
from tests.test_shards_cpu import assert_sharded_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def omp_lib():
    return load_oracle(omp=True)


def same_events(g, o, name, what):
    ge, oe = ac.drain_all(g, name), ac.drain_all(o, name)
    for v in ge:
        assert ge[v] == oe[v], f"{what}: listener of host {v}: {len(ge[v])} events, the oracle {len(oe[v])}"
    return ge


def detail_of(name, e):
    """(the pairs checked in detail: the hand-made ones and 16 seeded others; their hosts)."""
    pairs = ac.ae_pairs(e.params, e.round)
    detail = ac.detail_pairs(name, len(pairs))
    return detail, [h for t in detail for h in pairs[t]]


@pytest.mark.parametrize("run", ac.RUNS, ids=ac.run_id)
def test_ae_case(gx_lib, omp_lib, run):
    name, ev = run
    what = ac.run_id(run)
    words, _ = ac.case_views(name)
    g = ac.at_ae_round(gx_lib, name, words, ev)
    o = ac.at_ae_round(omp_lib, name, words, ev)
    detail, hosts = detail_of(name, g)
    before = ac.before_state(g, hosts)
    g.ae_merge()
    o.ae_merge()
    assert_same(g, o, f"{what} after ae_merge")
    events = same_events(g, o, name, what) if ev else None
    # the hand-made pairs and 16 seeded others: the queues, tuple for tuple
    for v in hosts:
        assert np.array_equal(ac.queue_array(g, v), ac.queue_array(o, v)), f"{what}: queue of host {v}"
    # every pair's words and the counters (the two large cases: the pairs in detail only)
    ac.check_against_model(g, name, words, before, detail, events, every_pair=not ac.ALL[name]["big"])
    # a wrong job only shows once it is sent
    for e in (g, o):
        e.round_end()
        e.run_rounds(12)
    assert_same(g, o, f"{what} 12 rounds after the push-pull round")
    if ev:
        same_events(g, o, name, what + " later rounds")


def test_ae_initiate(gx_lib, omp_lib):
    """GX_PP_INITIATE (k_ae_plan with PF = 1, one launch per batch) on the written views: parity with
    the oracle alone (an exchange of a later batch reads what an earlier one wrote)."""
    name = "s8_initiate"
    words, _ = ac.case_views(name)
    g = ac.at_ae_round(gx_lib, name, words)
    o = ac.at_ae_round(omp_lib, name, words)
    st0 = g.stats()
    g.ae_merge()
    o.ae_merge()
    assert g.stats()["ae_exchanges"] - st0["ae_exchanges"] > ac.ALL[name]["H"] // 2  # more than a matching has
    assert_same(g, o, f"{name} after ae_merge")
    for e in (g, o):
        e.round_end()
        e.run_rounds(12)
    assert_same(g, o, f"{name} 12 rounds after the push-pull round")


@pytest.mark.parametrize("ev", [False, True], ids=["", "ev"])
@pytest.mark.parametrize("name", ["s16_off", "s3_odd"])
def test_merge_views(gx_lib, oracle_lib, name, ev):
    """gx_merge(dst, src), all four k_merge_views variants: the hand-made pairs one way each and 100
    seeded (dst, src), against the oracle and exchange_model(both=False)."""
    words, _ = ac.case_views(name)
    g = ac.at_ae_round(gx_lib, name, words, ev)
    o = ac.at_ae_round(oracle_lib, name, words, ev)
    want = run_merges(g, o, name, np.array(words))
    assert_same(g, o, f"{name} after the gx_merge calls")
    if ev:
        check_merge_events(g, name, want, same_events(g, o, name, name))


@pytest.mark.parametrize("name", list(ac.SHARDED))
def test_ae_sharded(gx_lib, omp_lib, name):
    """Shards on one device against the unsharded HIP engine and the oracle, after the push-pull round
    and 12 rounds later; the model on the hand-made pairs, the cross pairs among them."""
    case = ac.SHARDED[name]
    ev = case["listeners"]
    words, hand = ac.case_views(name)
    whole = ac.at_ae_round(gx_lib, name, words, ev)
    orc = ac.at_ae_round(omp_lib, name, words, ev)
    sh = ac.sharded_at_ae_round(gx_lib, name, words, device="cuda:0", ev=ev)
    sx = ac.Sharded(sh)
    pairs = ac.ae_pairs(whole.params, whole.round)
    detail = sorted(hand)
    before = ac.before_state(sx, [h for t in detail for h in pairs[t]])
    for e in (whole, orc):
        e.ae_merge()
        e.round_end()
    sh.round_finish(True)
    assert_sharded_equal(whole, sh, f"{name} vs the unsharded engine after the push-pull round")
    assert_sharded_equal(orc, sh, f"{name} vs the oracle after the push-pull round")
    events = None
    if ev:
        events, we, oe = (ac.drain_all(x, name) for x in (sx, whole, orc))
        assert events == oe and we == oe, f"{name}: listener events differ (shards, unsharded, oracle)"
    ac.check_against_model(sx, name, words, before, detail, events, every_pair=False)
    for x in (whole, orc, sh):
        x.run_rounds(12)
    assert_sharded_equal(whole, sh, f"{name} vs the unsharded engine 12 rounds later")
    assert_sharded_equal(orc, sh, f"{name} vs the oracle 12 rounds later")
