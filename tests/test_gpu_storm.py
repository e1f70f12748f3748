"""The ExpireServer storm kernels (k_storm_p2 for S | 64, k_storm otherwise) on sparse views: the
cases of tests/storm_cases.py, whose row lengths cross every seam of the kernels' pipeline (DESIGN.md
"Storm contract"), compared with the oracle bit for bit and with the numpy model of
storm_cases.storm_model. tests/test_storm_model_cpu.py holds the guards that keep each case on the
paths it names."""
import numpy as np
import pytest

from sidecar_amd.dist import LocalShards
from tests import storm_cases as sc
from tests.oracle_lib import load_oracle
from tests.parity import assert_same
from tests.test_shards_cpu import assert_sharded_equal

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def omp_lib():
    return load_oracle(omp=True)


def at_storm_round(lib, name, words, ev=False, **extra):
    case = sc.CASES[name]
    e = sc.make_engine(lib, name, **extra)
    e.run_rounds(case["storm_round"])
    e.write_views(words)
    if ev:
        sc.add_listeners(e)
    return e


def same_events(g, o, what):
    ge, oe = sc.drain_all(g), sc.drain_all(o)
    for v in ge:
        assert ge[v] == oe[v], f"{what}: listener of viewer {v}: {len(ge[v])} events, the oracle {len(oe[v])}"
    return ge


@pytest.mark.parametrize("run", sc.RUNS, ids=sc.run_id)
def test_storm_case(gx_lib, omp_lib, run):
    name, ev = run
    case = sc.CASES[name]
    H = case["H"]
    words = sc.case_views(name)
    g = at_storm_round(gx_lib, name, words, ev)
    o = at_storm_round(omp_lib, name, words, ev)
    before = sc.before_state(g)
    g.round_send()
    o.round_send()
    what = sc.run_id(run)
    sc.assert_same_after_send(g, o, f"{what} after the storm's round_send")
    events = same_events(g, o, what) if ev else None
    # the seam viewers of both halves and 16 seeded others: the queued jobs, tuple for tuple
    half = H // 2
    rng = np.random.default_rng(case["seed"])
    viewers = set(range(sc.SEAM_VIEWERS)) | set(range(half, half + sc.SEAM_VIEWERS)) | \
        set(int(v) for v in rng.choice(H, size=16, replace=False))
    for v in sorted(viewers):
        gq, oq = sc.queue_array(g, v), sc.queue_array(o, v)
        assert np.array_equal(gq, oq), f"{what}: queue of viewer {v} differs from the oracle's"
    sc.check_against_model(g, name, words, before, viewers, events)
    # a wrong job or mask only shows once it is sent
    for e in (g, o):
        e.round_merge()
        e.ae_merge()
        e.round_end()
    assert_same(g, o, f"{what} at the end of the storm round")
    for e in (g, o):
        e.run_rounds(12)
    assert_same(g, o, f"{what} 12 rounds after the storm")
    if ev:
        same_events(g, o, what + " later rounds")


def test_storm_sharded(gx_lib, omp_lib):
    """s16_three's views written shard by shard (d.lo != 0, Hl not dividing H): 3 shards against
    the unsharded HIP engine and the oracle through the storm and 12 rounds more."""
    name = "s16_three"
    case = sc.CASES[name]
    words = sc.case_views(name)
    whole = at_storm_round(gx_lib, name, words)
    orc = at_storm_round(omp_lib, name, words)
    sh = LocalShards(gx_lib, 3, device="cuda:0", **case["params"])
    sh.run_rounds(case["storm_round"])
    for e in sh.engines:
        e.write_views(words[e.lo:e.hi], e.lo)
    for x in (whole, orc, sh):
        x.run_rounds(13)
    assert whole.stats()["expire_server"] > 0
    assert_sharded_equal(whole, sh, "s16_three G=3 vs the unsharded engine")
    assert_sharded_equal(orc, sh, "s16_three G=3 vs the oracle")


@pytest.mark.parametrize("name", ["s64_three", "s3_generic"])
def test_notify_leave_on_sparse_rows(gx_lib, oracle_lib, name):
    """The single-call path (gx_notify_leave, the API kernel) on the same sparse rows."""
    case = sc.CASES[name]
    H = case["H"]
    words = sc.case_views(name)
    g = at_storm_round(gx_lib, name, words, storm_round=-1)
    o = at_storm_round(oracle_lib, name, words, storm_round=-1)
    rng = np.random.default_rng(7)
    before = o.stats()["expire_server"]
    for v in rng.integers(0, H, size=200):
        lo, hi = sc.other_half(H, int(v))
        owner = int(rng.integers(lo, hi))
        g.notify_leave(int(v), owner)
        o.notify_leave(int(v), owner)
    n = o.stats()["expire_server"] - before
    assert 50 < n < 150, n  # about half the owners are live
    assert_same(g, o, f"{name} after 200 NotifyLeave calls")
