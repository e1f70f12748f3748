"""Which kernel variant a round launches: small clusters chosen so that every input of the host's
variant selection (gx_engine.hip: launch_send, launch_merge, with_flags) takes every value, each
compared bit-exact with the CPU oracle like tests/test_gpu_parity.py.

The inputs: the owner class of S (<= 4, <= 8, <= 16: owner ticks fused into k_send; above: apart),
the parity of R = H * S (VEC), a listener on some view (EV), retransmit_rounds (planned sends),
departures (X), a storm round or the failure detector (sends without the expiry scans),
GossipMessages and the lock model (the merge). The first rounds of every engine run the k_scan
placement (scan_heavy until the first snapshots arrive), the later ones k_send's own scans; the
cases with expiry-age records (CHURN) have views that do get scanned, in either placement.
"""
import pytest

from sidecar_amd.abi import INIT_OWN, INIT_WARM, Engine, default_params
from tests.fd_parity import assert_same_fd
from tests.parity import assert_same

pytestmark = pytest.mark.gpu

DEPART = dict(depart_round=2, depart_ppm=100000)
CHURN = dict(churn_ppm=80000, aged_ppm=60000)
STORM = dict(init_mode=INIT_WARM, partition_start=0, partition_end=12, storm_round=5, queue_cap=1024)

# name -> (parameters, [(view, listener id, capacity)])
CASES = {
    # owner class 1; R = 111 is odd
    "s3_odd_plan": (dict(n_hosts=37, n_services=3, **CHURN, ae_period_rounds=5), []),
    "s3_odd_ev_rt0": (dict(n_hosts=37, n_services=3, retransmit_rounds=0, **CHURN, ae_period_rounds=5),
                      [(0, 1, 4096), (36, 1, 50)]),
    "s4_ev_depart": (dict(n_hosts=40, n_services=4, **DEPART, **CHURN), [(3, 1, 4096)]),
    # owner class 2
    "s6_ev_plan_gm3": (dict(n_hosts=32, n_services=6, gossip_messages=3), [(0, 1, 4096), (31, 2, 64)]),
    "s8_rt0_depart": (dict(n_hosts=30, n_services=8, retransmit_rounds=0, **DEPART, ae_period_rounds=4), []),
    # owner class 4
    "s12_plan_lock_off": (dict(n_hosts=48, n_services=12, lock_model=0, gossip_messages=4, ae_period_rounds=6), []),
    "s16_ev_depart": (dict(n_hosts=32, n_services=16, **DEPART), [(5, 1, 4096)]),
    "s16_rt0": (dict(n_hosts=35, n_services=16, retransmit_rounds=0, **CHURN), []),
    # S > 16: k_owner apart, the scans in k_send
    "s24_plan": (dict(n_hosts=30, n_services=24, ae_period_rounds=5), []),
    "s24_ev_rt0": (dict(n_hosts=33, n_services=24, retransmit_rounds=0, churn_ppm=80000), [(1, 1, 4096)]),
    "s24_depart_lock_off": (dict(n_hosts=30, n_services=24, lock_model=0, **DEPART), []),
    # the storm round and the detector: BroadcastTombstones finished apart, k_send without scans
    "storm_s8_ev_plan": (dict(n_hosts=40, n_services=8, **STORM), [(0, 1, 4096), (39, 1, 100)]),
    "storm_s3_odd_rt0": (dict(n_hosts=45, n_services=3, retransmit_rounds=0, **STORM, ae_period_rounds=4), []),
    "fd_s8_depart": (dict(n_hosts=40, n_services=8, init_mode=INIT_WARM, fd_enable=1, **DEPART, queue_cap=4096,
                          ae_period_rounds=5), []),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_send_variant_parity(oracle_lib, gx_lib, name):
    kw, listen = CASES[name]
    kw = dict(dict(init_mode=INIT_OWN), **kw)
    g = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    o = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    for v, lid, cap in listen:
        g.add_listener(v, lid, cap)
        o.add_listener(v, lid, cap)
    assert_same(g, o, f"{name} init")
    for chunk in (1, 3, 10):
        g.run_rounds(chunk)
        o.run_rounds(chunk)
        assert_same(g, o, f"{name} round {g.round}")
        if kw.get("fd_enable"):
            assert_same_fd(g, o, f"{name} round {g.round}")
        for v, lid, cap in listen:
            ge = [x.tup() for x in g.drain_listener(v, lid, cap)]
            oe = [x.tup() for x in o.drain_listener(v, lid, cap)]
            assert ge == oe, f"{name} view {v} listener {lid} round {g.round}"
    assert g.converged() == o.converged()
