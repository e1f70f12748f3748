"""Coded checkpoints of sharded HIP engines (include/gx_ckpt.h gx_ckpt_save_coded through
sidecar_amd.dist ShardRounds.save(dirname, code)): the q8 schedule of tests/ckpt_coded_cases.py saved
at round 12, where the oracle holds every shape of FIFO window at once, on G = 3 (Hl = 11: the count
table needs its padding, the server-time table is [11][33]) and G = 2. The cluster restored from the
coded files continues bit for bit as the unsharded engine and the oracle."""
import numpy as np
import pytest

from sidecar_amd.abi import CK_FIFO, CK_SRVT, CKPT_CODE_FIFO, CKPT_CODE_SRVT, CKPT_FIFO, CKPT_VIEWS, Engine, default_params
from sidecar_amd.dist import LocalShards
from tests import ckpt_coded_cases as cc
from tests import ckpt_fifo_ref
from tests.test_shards_cpu import assert_sharded_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("G", [3, 2])
def test_gpu_shards_coded_save_load_continue(gx_lib, oracle_lib, tmp_path, G):
    kw = cc.CASES["q8"]
    whole = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    sh = LocalShards(gx_lib, G, device="cuda:0", **kw)
    for e in (whole, orc, sh):
        e.run_rounds(12)
    shapes = cc.fifo_shapes(orc)
    assert all(shapes[k] > 0 for k in cc.FIFO_SHAPES), shapes
    infos = sh.save(tmp_path, CKPT_CODE_SRVT | CKPT_CODE_FIFO)
    assert len(infos) == G
    for e, info in zip(sh.engines, infos):
        Hl = e.hi - e.lo
        assert (info["sections"][CK_SRVT]["coding"], info["sections"][CK_FIFO]["coding"]) == (CKPT_VIEWS, CKPT_FIFO)
        assert info["sections"][CK_SRVT]["raw_bytes"] == 16 * Hl * e.H
        queues = cc.queues(e)
        assert info["sections"][CK_FIFO]["stored_bytes"] == ckpt_fifo_ref.stored_bytes([len(q) for q in queues])
        assert queues == cc.queues(orc)[e.lo:e.hi]
    sh2 = LocalShards.load(gx_lib, tmp_path, "cuda:0")
    assert_sharded_equal(whole, sh2, f"G={G} restored at round 12")
    for a, b in zip(sh.engines, sh2.engines):
        assert np.array_equal(cc.srvt_table(a), cc.srvt_table(b)) and cc.queues(a) == cc.queues(b)
    for e in (whole, orc, sh, sh2):
        e.run_rounds(20)
    assert_sharded_equal(whole, sh2, f"G={G} round 32")
    assert_sharded_equal(orc, sh2, f"G={G} round 32 vs oracle")
    assert_sharded_equal(whole, sh, f"G={G} round 32, the cluster that saved")
    table = np.concatenate([cc.srvt_table(e) for e in sh2.engines])
    assert np.array_equal(table, cc.srvt_table(orc))
    assert sum((cc.queues(e) for e in sh2.engines), []) == cc.queues(orc)
