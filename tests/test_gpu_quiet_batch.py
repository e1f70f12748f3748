"""A stretch of quiet rounds in one k_send launch on the HIP engine, over the schedules
of tests/quiet_batch_cases.py: those of the quiet-round and lean-send tests (128-256 hosts, 150 rounds,
a ragged last block, packets that leave records pending and cut the ring, every owner-tick class and
the separate k_owner, fanout 5, push-pull every 10 rounds, a partition over [0, 50)).

The results stay the oracle's bit for bit however the rounds are cut into calls and whatever the cap on
a batch; a batched run leaves what a run of one launch per round leaves (GX_QUIET_BATCH=1 in a fresh
process), the send class's bytes and units included; batches are taken; none starts after a mutating
entry before a fresh bound has arrived; and none runs while a record watch or a listener is armed.

The send class (gx_timing.launches) counts one launch per round and one per batch, the merge class one
per round on the generic path and none in a quiet round."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from sidecar_amd.abi import WATCH_ANY
from tests import quiet_batch_cases as cases
from tests.parity import assert_same
from tests.test_gpu_quiet_rounds import assert_snap, merge_launches

pytestmark = pytest.mark.gpu

ROUNDS = cases.ROUNDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(cases.SCHEDULES)


def _default_cap():
    assert "GX_QUIET_BATCH" not in os.environ and os.environ.get("GX_QUIET_SEND", "1") != "0", \
        "this process must run batches at the default cap"


def _child(mode, name, batch):
    env = dict(os.environ, GX_QUIET_BATCH=str(batch))
    out = subprocess.run([sys.executable, "-m", "tests.quiet_batch_cases", mode, name], cwd=ROOT, env=env, check=True,
                         stdout=subprocess.PIPE, timeout=120).stdout
    return json.loads(out.decode().strip().splitlines()[-1])


@pytest.mark.parametrize("chunk", cases.CHUNKS)
@pytest.mark.parametrize("name", NAMES)
def test_parity(gx_lib, name, chunk):
    """One run_rounds(150), calls of 10 and calls of 7 at the default cap give the oracle's run."""
    _default_cap()
    n = cases.run_parity(gx_lib, name, chunk)
    print(f"{name} calls of {chunk}: {n['send_launches']} send launches, {ROUNDS - n['merge_launches']} quiet rounds taken")
    assert n["send_launches"] <= ROUNDS


@pytest.mark.parametrize("name", NAMES)
def test_parity_cap_3(name):
    """The same three runs in a fresh process with GX_QUIET_BATCH=3 (the child asserts the parity)."""
    n = _child("parity", name, 3)
    print(f"{name} cap 3: {n}")
    for c in cases.CHUNKS:
        assert n[str(c)]["send_launches"] <= ROUNDS


@pytest.mark.parametrize("name", NAMES)
def test_batched_equals_unbatched(gx_lib, name):
    """Calls of 10 here (batched) and in a fresh process with GX_QUIET_BATCH=1: identical state at round
    150 (stats, hosts, views, digests, LastChanged, server times), identical send bytes and units.
    Batching happens here: at least MIN_PREDICTED // 4 launches are saved (the quiet-round tests ask for
    half of the predicted rounds on the quiet path, and batches of two or more save at least half of
    those launches); the fresh process saves none."""
    _default_cap()
    batched = cases.run_calls(gx_lib, name)
    single = _child("calls", name, 1)
    saved = {k: ROUNDS - fp.pop("send_launches") for k, fp in (("batched", batched), ("single", single))}
    quiet = {k: ROUNDS - fp.pop("merge_launches") for k, fp in (("batched", batched), ("single", single))}
    print(f"{name}: launches saved {saved}, quiet rounds taken {quiet}, send bytes {batched['send_bytes']} / "
          f"{single['send_bytes']}, units {batched['send_units']} / {single['send_units']}")
    diff = {k: (batched[k], single[k]) for k in batched if batched[k] != single[k] and k != "hosts"}
    assert not diff, diff
    assert batched["hosts"] == single["hosts"]
    assert saved["single"] == 0
    assert saved["batched"] >= cases.MIN_PREDICTED[name] // 4


@pytest.mark.parametrize("name", ["h128", "h130_cap8_pend4"])
def test_invalidation(gx_lib, oracle_lib, name):
    """Calls of 10 with gx_set_round (to the same round) between them, on both engines: the two rounds
    after the call are generic and launched one by one (the first folds the first bound that counts
    again, the second asks for it), so no batch starts before a fresh bound has arrived; batches are
    found again after that, and parity holds."""
    _default_cap()
    g = cases.engine(gx_lib, name)
    o = cases.engine(oracle_lib, name)
    saved = 0
    for c in range(ROUNDS // 10):
        if c:
            for e in (g, o):
                e.set_round(e.round)
        merges, sends = merge_launches(g), cases.send_launches(g)
        g.run_rounds(2)
        assert merge_launches(g) - merges == 2, f"{name} round {g.round}: a round after the call took the quiet path"
        assert cases.send_launches(g) - sends == 2
        g.run_rounds(8)
        saved += 10 - (cases.send_launches(g) - sends)
        o.run_rounds(10)
        assert_same(g, o, f"{name} invalidation round {g.round}")
    print(f"{name}: {saved} launches saved between the calls")
    assert saved > 0


@pytest.mark.parametrize("armed", ["watch", "listener"])
def test_no_batch_when_observed(gx_lib, oracle_lib, armed):
    """A record watch counts per round and a listener's rounds are generic: every round has its own
    send launch, and the run is the oracle's."""
    _default_cap()
    name = "h128"
    g = cases.engine(gx_lib, name)
    if armed == "watch":
        g.watch_arm(2, ROUNDS)
        g.watch_set(0, [5, 3 * 16 + 1], [WATCH_ANY, WATCH_ANY])
        for _ in range(ROUNDS // 10):
            g.run_rounds(10)
        assert_snap(g, cases.oracle_trace(name)["snaps"][ROUNDS], f"{name} watch")
        counts, live, first, logged, missed = g.watch_read()
        assert (first, logged, missed) == (0, ROUNDS, 0)
        assert np.all(counts[-1, :, 0] > 0)  # every round was logged: the records are held at the end
        assert ROUNDS - merge_launches(g) > 0  # quiet rounds are still taken, one launch each
    else:
        o = cases.engine(oracle_lib, name)
        for e in (g, o):
            e.add_listener(3, 1, 16)
        for _ in range(ROUNDS // 10):
            g.run_rounds(10)
            o.run_rounds(10)
        assert_same(g, o, f"{name} listener")
    assert cases.send_launches(g) == ROUNDS
