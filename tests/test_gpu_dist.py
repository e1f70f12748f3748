"""The multi-process sharded path (sidecar_amd.dist.DistShard, what bench.py runs at N > 1) on the
HIP engine: two processes on the one GPU of the test box, collectives over gloo staged through
the host (RCCL refuses two ranks on one device). Everything the ranks do on the device — outbox
plan and pack, inbox unpack, cross-shard push-pull digests, lead and return blocks, merges — is
the RCCL path's; the views, per-host bookkeeping, queue digests and summed counters must equal
the unsharded CPU oracle's."""
import numpy as np
import pytest

from sidecar_amd.abi import Engine, default_params
from tests.parity import host_tuples
from tests.ranks import run_ranks
from tests.test_shards_cpu import SCEN

pytestmark = pytest.mark.gpu


def _worker(rank, world, kw, rounds):
    import torch
    import torch.distributed as dist
    from sidecar_amd.abi import load_product
    from sidecar_amd.dist import DistShard
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sh = DistShard(load_product(), rank, world, "cuda:0", **kw)
    assert sh.stage
    sh.run_rounds(rounds)
    st = sh.stats()
    conv = sh.converged()
    fd = sh.e.fd_converged()[1] if kw.get("fd_enable") else 0
    out = (rank, sh.e.read_views(), host_tuples(sh.e), sh.e.digests(), st, (conv, fd))
    dist.barrier()
    sh.close()
    dist.destroy_process_group()
    return out


@pytest.mark.parametrize("name,world", [("storm", 2), ("blocks3", 2), ("fd", 2), ("departures", 3)])
def test_gpu_dist_gloo_matches_oracle(oracle_lib, name, world):
    kw, rounds = SCEN[name], 40
    res = run_ranks(_worker, world, (kw, rounds), timeout=100)
    whole = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    whole.run_rounds(rounds)
    assert np.array_equal(np.concatenate([r[1] for r in res]), whole.read_views())
    assert sum((r[2] for r in res), []) == host_tuples(whole)
    assert np.array_equal(np.concatenate([r[3] for r in res]), whole.digests())
    assert res[0][4] == whole.stats()
    (c, n), fd = res[0][5][0], [r[5][1] for r in res]
    cw, nw = whole.converged()
    if nw == 0 and kw.get("fd_enable"):
        cw, nw = whole.fd_converged()
        # a node misjudged in several shards counts once per shard in the sharded sum
        assert max(fd) <= nw <= sum(fd) and n == sum(fd)
    else:
        assert n == nw
    assert c == cw
