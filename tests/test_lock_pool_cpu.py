"""The preconditions of tests/test_gpu_lock_pool.py, on the CPU oracle alone: on every schedule the
claimed pool (gx.h lock_readers = 2) is run with, fewer merges ever wait at once than the pool has
slots, and the direct-mapped pool of the same size still loses some."""
import pytest

from sidecar_amd.abi import LOCK_READERS_MAPPED, Engine, default_params
from tests.lock_pool_cases import CONTRAST, ROUNDS, SCHEDULES, lossless_oracle, schedule, waiting


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_lossless_peak_fits_the_pool(oracle_lib, name):
    """The peak at a round's end is the true peak: drains happen in the merge phase, claims in the
    later push-pull phase."""
    kw, slots = schedule(name)
    o = lossless_oracle(oracle_lib, kw)
    peak = 0
    for _ in range(ROUNDS):
        o.run_rounds(1)
        peak = max(peak, len(waiting(o)))
    st = o.stats()
    assert st["ae_deferred"] > 0 and st["ae_defer_lost"] == 0, st
    assert 0 < peak <= (slots or 64), peak
    if name == "matching":
        assert peak > 2  # the overflow test's pool of 2 must overflow


@pytest.mark.parametrize("name", CONTRAST)
def test_direct_mapped_pool_loses_merges(oracle_lib, name):
    kw, slots = schedule(name)
    o = Engine(default_params(oracle_lib, lock_readers=LOCK_READERS_MAPPED, lock_defer_slots=slots, **kw),
               lib=oracle_lib)
    o.run_rounds(ROUNDS)
    assert o.stats()["ae_defer_lost"] >= 1
