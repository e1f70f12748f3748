"""Quiet rounds on the HIP engine: in a round the device has reported as quiet ahead of
time, gx_run_rounds launches no receive phase and no push-pull pairs. The results stay the oracle's
bit for bit however the rounds are cut into calls, the path is taken where it can be and nowhere
else, and an ABI call between rounds sends the next rounds down the generic path again.

The schedules and the oracle's side are tests/quiet_cases.py (checked on the CPU by
tests/test_quiet_rounds_cpu.py). The merge class (gx_timing.launches) counts one launch per round
on the generic path and none in a quiet round."""
import numpy as np
import pytest

from sidecar_amd.abi import ALIVE, Engine, default_params
from tests import quiet_cases
from tests.parity import _dict_diff, _first_diff, assert_same, snapshot

pytestmark = pytest.mark.gpu

ROUNDS = quiet_cases.ROUNDS


def assert_snap(g, want, what):
    got = snapshot(g)
    assert got["stats"] == want["stats"], f"{what}: stats differ\n{_dict_diff(got['stats'], want['stats'])}"
    assert np.array_equal(got["views"], want["views"]), f"{what}: views differ"
    assert got["hosts"] == want["hosts"], f"{what}: host states differ at {_first_diff(got['hosts'], want['hosts'])}"
    assert np.array_equal(got["digests"], want["digests"]), f"{what}: queue digests differ"
    assert np.array_equal(got["last_changed"], want["last_changed"]), f"{what}: state.LastChanged differs"
    assert np.array_equal(got["times"], want["times"]), f"{what}: server times differ"


def merge_launches(g):
    return g.timing()["merge"]["launches"]


def run_checked(g, chunk, snaps, what):
    """Runs to ROUNDS in calls of at most `chunk` rounds, cut at the rounds the oracle's snapshots were
    taken at, and compares there (reading state back invalidates nothing)."""
    for stop in quiet_cases.CHECK_ROUNDS:
        while g.round < stop:
            g.run_rounds(min(chunk, stop - g.round))
        assert_snap(g, snaps[stop], f"{what} round {stop}")


@pytest.mark.parametrize("chunk", [ROUNDS, 1, 7])
@pytest.mark.parametrize("name", sorted(quiet_cases.SCHEDULES))
def test_parity(gx_lib, name, chunk):
    """One run_rounds(150) (compared at round 150), calls of 1 round and calls of 7 rounds (compared
    at rounds 10, 50, 51, 100 and 150) all give the oracle's run."""
    t = quiet_cases.oracle_trace(name)
    g = Engine(default_params(gx_lib, **t["params"]), lib=gx_lib)
    if chunk == ROUNDS:
        g.run_rounds(ROUNDS)
        assert_snap(g, t["snaps"][ROUNDS], f"{name} one call")
    else:
        run_checked(g, chunk, t["snaps"], f"{name} calls of {chunk}")
    skipped = ROUNDS - merge_launches(g)
    print(f"{name} calls of {chunk}: {skipped} rounds took the quiet path, the oracle has {len(t['quiet'])} quiet")
    assert 0 <= skipped <= len(t["quiet"])
    if chunk == 1:  # every call ends with the device caught up: each bound is seen before the next round
        assert skipped >= quiet_cases.MIN_PREDICTED[name] // 2


@pytest.mark.parametrize("name", sorted(quiet_cases.SCHEDULES))
def test_path_taken(gx_lib, name):
    """One run_rounds(150): fewer receive phases than rounds, and never fewer than the rounds the
    oracle does not call quiet."""
    t = quiet_cases.oracle_trace(name)
    g = Engine(default_params(gx_lib, **t["params"]), lib=gx_lib)
    g.run_rounds(ROUNDS)
    n = merge_launches(g)
    print(f"{name}: {n} merge launches in {ROUNDS} rounds, the oracle has {len(t['quiet'])} quiet rounds")
    assert n < ROUNDS
    assert n >= ROUNDS - len(t["quiet"])


@pytest.mark.parametrize("case", ["cold", "lock_model_0", "lock_readers_1"])
def test_control_every_round_merges(gx_lib, case):
    """No quiet round on a cold start; none taken without the lock model or with read-locked
    exchanges, where the bound's argument was not made."""
    kw = dict(quiet_cases.COLD) if case == "cold" else dict(quiet_cases.SCHEDULES["h128"])
    if case == "lock_model_0":
        kw["lock_model"] = 0
    elif case == "lock_readers_1":
        kw["lock_readers"] = 1
    g = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    for _ in range(ROUNDS // 10):  # the device caught up between calls: a bound would be seen
        g.run_rounds(10)
    assert merge_launches(g) == ROUNDS


@pytest.mark.parametrize("name", sorted(quiet_cases.SCHEDULES))
def test_invalidation(gx_lib, oracle_lib, name):
    """Chunks of 10 rounds with gx_add_service_entries and gx_set_round (to the same round) between
    them, on both engines: parity holds, and the two rounds after the calls take the generic path
    whatever was known before (the first folds the first bound that counts again, the second asks for
    it). Every other chunk is one call of 10 rounds; the rest are cut after those two rounds, which
    shows by the launch counts that it is exactly they that merge."""
    kw = quiet_cases.SCHEDULES[name]
    g = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    o = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    skipped = 0
    for c in range(ROUNDS // 10):
        if c:
            rec = (3, c % 16, g.now(), ALIVE)
            for e in (g, o):
                e.add_service_entries([3], [rec])
                e.set_round(e.round)
        before = merge_launches(g)
        if c % 2:
            g.run_rounds(2)
            assert merge_launches(g) - before == 2, f"{name} round {g.round}: a round after the calls took the quiet path"
            g.run_rounds(8)
        else:
            g.run_rounds(10)
            assert merge_launches(g) - before >= 2, f"{name} round {g.round}: a round after the calls took the quiet path"
        skipped += 10 - (merge_launches(g) - before)
        o.run_rounds(10)
        assert_same(g, o, f"{name} invalidation round {g.round}")
    print(f"{name}: {skipped} rounds took the quiet path between the calls")
    assert skipped > 0  # the path is found again after the calls
