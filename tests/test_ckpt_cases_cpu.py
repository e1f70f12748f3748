"""The checkpoint continuity runs (tests/ckpt_cases.py) are not vacuous: by the oracle, the states they
save hold, between them, every kind of work that waits across rounds; and the checkpoint entry points
of sidecar_amd.abi answer GX_ENOSYS on the oracle library, which has none of gx_ckpt.h's symbols."""
import pytest

from sidecar_amd.abi import GX_ENOSYS, Engine, GxError, ckpt_params, default_params
from sidecar_amd.dist import LocalShards
from tests import ckpt_cases


def test_save_points_cover_every_waiting_state(oracle_lib):
    seen = {}
    for name, (_, _, n1, _, _) in ckpt_cases.RUNS.items():
        seen[name] = ckpt_cases.features(ckpt_cases.oracle_at(oracle_lib, name, n1))
    union = set().union(*seen.values())
    assert union == set(ckpt_cases.FEATURES), seen
    # the lock_readers runs saved past the storm hold a waiting merge and a non-empty lock buffer
    for name in ("matching", "initiate", "gm4", "odd_rows"):
        assert {"waiting_merge", "lock_buffer", "pending"} <= seen[f"{name}_r15"], (name, seen[f"{name}_r15"])
    assert "pending_expire" in seen["fd_r15"] and "sleepers" in seen["churn_depart_bytes_r40"]


def test_oracle_has_no_checkpoints(oracle_lib, tmp_path):
    e = Engine(default_params(oracle_lib, n_hosts=8, n_services=2), lib=oracle_lib)
    path = tmp_path / "x.gxck"
    (tmp_path / "shard_000_of_002.gxck").write_bytes(b"")  # LocalShards.load reads G from the name
    for call in (lambda: e.ckpt_save(path), lambda: Engine.from_checkpoint(path, lib=oracle_lib),
                 lambda: ckpt_params(oracle_lib, path), lambda: LocalShards.load(oracle_lib, tmp_path)):
        with pytest.raises(GxError) as err:
            call()
        assert err.value.rc == GX_ENOSYS
