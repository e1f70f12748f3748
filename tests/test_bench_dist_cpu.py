"""bench.py's N>1 path (Cluster over DistShard, run_converge) rehearsed on the CPU oracle over
gloo with two ranks: the sharded cluster must report the unsharded cluster's counters and
rounds-to-converge, and the exchange byte accounting must add up."""
import pytest

from tests.ranks import run_ranks


def _worker(rank, world, cfg):
    import torch.distributed as dist
    import bench
    from tests.oracle_lib import load_oracle
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lib = load_oracle()
        c = bench.Cluster(lib, cfg, 0x5EED, rank, 2, rank, dist.barrier, device="cpu")
        c.run_rounds(45)
        st, x = c.stats(), c.exchange_bytes()
        c.close()
        conv = bench.run_converge(lib, cfg, 0x5EED, rank, 2, rank, dist.barrier, 600, 10, device="cpu")
        return rank, st, x, conv[0]
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("cfg", ["cfg1", "cfg1fd"])
def test_bench_cluster_gloo_world2(oracle_lib, cfg):
    import bench
    res = run_ranks(_worker, 2, (cfg,), timeout=300)
    whole = bench.make_engine(oracle_lib, cfg, 0x5EED, 0)
    whole.run_rounds(45)
    ref = whole.stats()
    whole.close()
    (_, st0, x0, conv0), (_, st1, x1, conv1) = res
    assert st0 == st1 == ref
    assert x0 == x1 and x0["packets"] > 0
    assert conv0 == conv1
    ref_conv = bench.run_converge(oracle_lib, cfg, 0x5EED, 0, 1, 0, lambda: None, 600, 10)
    assert conv0 == ref_conv[0]
