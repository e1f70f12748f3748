"""Quiet rounds on the CPU oracle (tests/quiet_cases.py): the bound that predicts them never covers a
round that is not quiet, on the schedules the GPU tests run. This pins the inputs of
tests/test_gpu_quiet_rounds.py; it does not test the HIP engine."""
import pytest

from tests import quiet_cases


@pytest.mark.parametrize("name", sorted(quiet_cases.SCHEDULES))
def test_predicted_rounds_are_quiet(name):
    t = quiet_cases.oracle_trace(name)
    assert t["predicted"] <= t["quiet"], sorted(t["predicted"] - t["quiet"])
    assert len(t["predicted"]) >= quiet_cases.MIN_PREDICTED[name], (len(t["predicted"]), len(t["quiet"]))
    assert t["unlocks"] >= 1  # the bound is tested against hosts that do unlock inside the run


def test_cold_start_has_no_quiet_round():
    t = quiet_cases.oracle_trace("cold")
    assert not t["quiet"] and not t["predicted"]
