"""The schedules of tests/quiet_send_cases.py on the CPU oracle: they have the predicted quiet rounds,
free of queue, list and sleep drops, and the first two cut the pending ring inside them. This pins
the inputs of tests/test_gpu_quiet_send.py; it does not test the HIP engine."""
import pytest

from tests import quiet_send_cases as cases


@pytest.mark.parametrize("name", sorted(cases.SCHEDULES))
def test_schedule(name):
    t = cases.oracle_trace(name)
    print(f"{name}: {len(t['quiet'])} quiet rounds, {len(t['predicted'])} predicted, "
          f"{t['pending_drops_predicted']} pending_drops inside predicted rounds")
    assert t["predicted"] <= t["quiet"], sorted(t["predicted"] - t["quiet"])
    assert len(t["predicted"]) >= cases.MIN_PREDICTED[name], (len(t["predicted"]), len(t["quiet"]))
    s = t["stats"]
    assert s["queue_drops"] == s["list_drops"] == s["sleep_drops"] == 0, s
    if name in cases.PENDING:
        assert t["pending_drops_predicted"] > 0
