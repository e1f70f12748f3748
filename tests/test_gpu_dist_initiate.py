"""Per-node push-pull (GX_PP_INITIATE) on the multi-process sharded path (DistShard, what bench.py
runs at N > 1): processes on the one GPU of the test box, collectives over gloo staged through the
host. Every rank derives the round's batches itself and makes one chain of collectives per batch;
views, per-host bookkeeping, queue digests, summed counters and the convergence verdict must equal
the unsharded CPU oracle's."""
import numpy as np
import pytest

from sidecar_amd.abi import Engine, default_params
from tests.parity import host_tuples
from tests.ranks import run_ranks
from tests.test_gpu_dist import _worker
from tests.test_gpu_shards_initiate import SCEN

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,world", [("pp_storm", 2), ("pp_stagger_ragged", 3), ("pp_departures", 3)])
def test_gpu_dist_gloo_initiate_matches_oracle(oracle_lib, name, world):
    kw, rounds = SCEN[name], 40
    res = run_ranks(_worker, world, (kw, rounds), timeout=100)
    whole = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    whole.run_rounds(rounds)
    assert whole.stats()["ae_exchanges"] > 0
    assert np.array_equal(np.concatenate([r[1] for r in res]), whole.read_views())
    assert sum((r[2] for r in res), []) == host_tuples(whole)
    assert np.array_equal(np.concatenate([r[3] for r in res]), whole.digests())
    assert res[0][4] == whole.stats()
    assert res[0][5][0] == whole.converged()
