"""Per-node push-pull (push_pull_mode = GX_PP_INITIATE) and the sharded round driver, without a
GPU: the binding's push-pull round predicate follows the engines' (with staggered timers some
host's timer fires every round, which the sized gossip path relies on), and the driver does not
hide that the CPU oracle has no sharded initiate protocol (the HIP engine has; the unsharded oracle
is its ground truth, tests/test_gpu_shards_initiate.py)."""
import pytest

from sidecar_amd.abi import PP_INITIATE, Engine, GxError, default_params
from sidecar_amd.dist import LocalShards

KW = dict(n_hosts=24, n_services=4, init_mode=2, push_pull_mode=PP_INITIATE, ae_period_rounds=4, ae_phase=1)


def test_is_ae_round_every_round_with_staggered_timers(oracle_lib):
    e = Engine(default_params(oracle_lib, push_pull_stagger=1, **KW), lib=oracle_lib)
    for _ in range(9):
        assert e.is_ae_round(), e.round
        e.run_rounds(1)


def test_is_ae_round_follows_the_period_without_stagger(oracle_lib):
    e = Engine(default_params(oracle_lib, **KW), lib=oracle_lib)
    for _ in range(9):
        assert e.is_ae_round() == (e.round % 4 == 1), e.round
        e.run_rounds(1)


@pytest.mark.parametrize("stagger", [0, 1])
def test_oracle_shards_refuse_initiate_mode(oracle_lib, stagger):
    with pytest.raises(GxError):
        LocalShards(oracle_lib, 2, push_pull_stagger=stagger, **KW)
