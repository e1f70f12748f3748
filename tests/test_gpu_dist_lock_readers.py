"""Push-pull with a read-locked side (gx.h lock_readers = 1) on the multi-process sharded path
(DistShard): processes on the one GPU of the test box, collectives over gloo staged through the host.
Every run of the push-pull chain makes one more collective, the MIN reduction that arbitrates the
cluster-wide pool's slots; views, per-host bookkeeping, queue digests, summed counters and the
convergence verdict must equal the unsharded CPU oracle's, losses included."""
import numpy as np
import pytest

from sidecar_amd.abi import Engine, default_params
from tests.parity import host_tuples
from tests.ranks import run_ranks
from tests.test_gpu_dist import _worker
from tests.test_gpu_shards_lock_readers import _kw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,world", [("matching_p8", 2), ("ragged_init_p8", 3)])
def test_gpu_dist_gloo_lock_readers_matches_oracle(oracle_lib, name, world):
    kw, rounds = _kw(name), 40
    res = run_ranks(_worker, world, (kw, rounds), timeout=100)
    whole = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    whole.run_rounds(rounds)
    st = whole.stats()
    assert st["ae_deferred"] >= 4 and st["ae_defer_lost"] >= 2, st
    assert np.array_equal(np.concatenate([r[1] for r in res]), whole.read_views())
    assert sum((r[2] for r in res), []) == host_tuples(whole)
    assert np.array_equal(np.concatenate([r[3] for r in res]), whole.digests())
    assert res[0][4] == st
    assert res[0][5][0] == whole.converged()
