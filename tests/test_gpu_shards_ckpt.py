"""Checkpoints of sharded HIP engines (include/gx_ckpt.h; sidecar_amd.dist ShardRounds.save,
LocalShards.load): every shard saves its own file with no collective; a cluster restored from the
files continues bit for bit as the unsharded engine and the oracle, on the lock_readers schedules of
tests/test_gpu_shards_lock_readers.py (read-locked exchanges across shards, the waiting merges' pool,
the sized and the planned gossip path)."""
import pytest

from sidecar_amd.abi import GX_EINVAL, Engine, GxError, ckpt_params
from sidecar_amd.dist import LocalShards, ShardRounds
from tests.test_gpu_shards_lock_readers import CHUNKS, _kw, _trio
from tests.test_shards_cpu import assert_sharded_equal

pytestmark = pytest.mark.gpu

PREFIX, REST = CHUNKS[:3], CHUNKS[3:]  # (1, 4, 10) before the save, (15, 30) after the load


@pytest.mark.parametrize("G", [2, 3, 5])
@pytest.mark.parametrize("name", ["matching_p8", "ragged_init_p8", "gm4_p8"])
def test_gpu_shards_save_load_continue(gx_lib, oracle_lib, tmp_path, name, G):
    whole, orc, sh = _trio(gx_lib, oracle_lib, _kw(name), G)
    for chunk in PREFIX:
        for e in (whole, orc, sh):
            e.run_rounds(chunk)
    infos = sh.save(tmp_path)
    assert len(infos) == G
    for g in range(G):
        p, r = ckpt_params(gx_lib, ShardRounds.shard_file(tmp_path, g, G))
        assert (p.n_shards, p.shard_id, r) == (G, g, sum(PREFIX))
    sh2 = LocalShards.load(gx_lib, tmp_path, "cuda:0")
    assert_sharded_equal(whole, sh2, f"{name} G={G} restored at round {whole.round}")
    for chunk in REST:
        for e in (whole, orc, sh, sh2):
            e.run_rounds(chunk)
        assert_sharded_equal(whole, sh2, f"{name} G={G} round {whole.round}")
        assert_sharded_equal(orc, sh2, f"{name} G={G} round {whole.round} vs oracle")
        assert_sharded_equal(whole, sh, f"{name} G={G} round {whole.round}, the cluster that saved")
    st = orc.stats()
    assert st["ae_deferred"] > 0 and st["ae_locked"] > 0  # (as the schedules' own test: not vacuous)
    # the pool's cross-shard counters are state: the restored cluster goes on counting where the saved one was
    assert sh2.ro_counts() == sh.ro_counts()


def test_gpu_shard_file_into_another_shard(gx_lib, tmp_path):
    sh = LocalShards(gx_lib, 2, device="cuda:0", **_kw("matching_p8"))
    sh.run_rounds(3)
    sh.save(tmp_path)
    f0 = ShardRounds.shard_file(tmp_path, 0, 2)
    for bad in (dict(shard_id=1), dict(n_shards=4), dict(n_shards=1)):
        with pytest.raises(GxError) as err:
            Engine.from_checkpoint(f0, lib=gx_lib, **bad)
        assert err.value.rc == GX_EINVAL, bad
    e = Engine.from_checkpoint(f0, lib=gx_lib)
    assert (e.G, e.lo, e.hi, e.round) == (2, 0, 16, 3)
