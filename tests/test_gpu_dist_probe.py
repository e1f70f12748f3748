"""Probe-traffic piggybacking (gx.h probe_piggyback) on the multi-process sharded path (DistShard):
processes on the one GPU of the test box, collectives over gloo staged through the host. Pings and
acks to hosts of other ranks ride in the planned exchange, in slots k_xplan counted and k_probe
wrote; no collective is added. Views, per-host bookkeeping, queue digests, summed counters and the
convergence verdict must equal the unsharded CPU oracle's."""
import numpy as np
import pytest

from sidecar_amd.abi import Engine, default_params
from tests.parity import host_tuples
from tests.ranks import run_ranks
from tests.test_gpu_dist import _worker
from tests.test_gpu_shards_probe import _kw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,world", [("probe_storm_partition", 2), ("probe_uneven", 3)])
def test_gpu_dist_gloo_probe_matches_oracle(oracle_lib, name, world):
    kw, rounds = _kw(name), 40
    res = run_ranks(_worker, world, (kw, rounds), timeout=100)
    whole = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    whole.run_rounds(rounds)
    st = whole.stats()
    off = Engine(default_params(oracle_lib, **_kw(name, probe=0)), lib=oracle_lib)
    off.run_rounds(rounds)
    assert st["packets"] != off.stats()["packets"]
    if name == "probe_storm_partition":  # pings across the partition, counted by the sender's rank
        assert st["lost_packets"] > 0
    assert np.array_equal(np.concatenate([r[1] for r in res]), whole.read_views())
    assert sum((r[2] for r in res), []) == host_tuples(whole)
    assert np.array_equal(np.concatenate([r[3] for r in res]), whole.digests())
    assert res[0][4] == st
    assert res[0][5][0] == whole.converged()
