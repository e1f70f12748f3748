"""k_send's lean instance for quiet rounds on the HIP engine, over the schedules of
tests/quiet_send_cases.py (checked on the CPU by tests/test_quiet_send_cpu.py): dropped packets that
leave batch records pending and cut the ring, a ragged last block, the peers sampled in k_send's
prologue and in each owner-tick class of the fused launch, more peers than team lanes.

The results stay the oracle's bit for bit, the quiet path is taken, and the lean instance leaves what
the generic one leaves (engine created with GX_QUIET_SEND=0, in a fresh process), the algorithmic
bytes and units of the send class included."""
import json
import os
import subprocess
import sys

import pytest

from sidecar_amd.abi import Engine, default_params
from tests import quiet_send_cases as cases
from tests.test_gpu_quiet_rounds import assert_snap, merge_launches, run_checked

pytestmark = pytest.mark.gpu

ROUNDS = cases.ROUNDS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("chunk", [ROUNDS, 1])
@pytest.mark.parametrize("name", sorted(cases.SCHEDULES))
def test_parity(gx_lib, name, chunk):
    """One run_rounds(150) (compared at round 150) and calls of 1 round (compared at rounds 10, 50, 51,
    100 and 150) give the oracle's run; with calls of 1 round, at least half of the oracle's
    predicted rounds launch no merge."""
    assert os.environ.get("GX_QUIET_SEND", "1") != "0", "this process must run the lean instance"
    t = cases.oracle_trace(name)
    g = Engine(default_params(gx_lib, **t["params"]), lib=gx_lib)
    if chunk == ROUNDS:
        g.run_rounds(ROUNDS)
        assert_snap(g, t["snaps"][ROUNDS], f"{name} one call")
    else:
        run_checked(g, chunk, t["snaps"], f"{name} calls of {chunk}")
    skipped = ROUNDS - merge_launches(g)
    print(f"{name} calls of {chunk}: {skipped} rounds took the quiet path, the oracle has {len(t['quiet'])} quiet")
    assert 0 <= skipped <= len(t["quiet"])
    if chunk == 1:
        assert skipped >= cases.MIN_PREDICTED[name] // 2


@pytest.mark.parametrize("name", sorted(cases.SCHEDULES))
def test_lean_equals_generic(name):
    """The same schedule in calls of 1 round here (lean) and in a fresh process whose engine keeps the
    generic instance in quiet rounds: identical state at round 150 (stats, hosts, views, digests,
    LastChanged, server times) and identical send bytes and units."""
    assert os.environ.get("GX_QUIET_SEND", "1") != "0", "this process must run the lean instance"
    lean = cases.run_product(name)
    env = dict(os.environ, GX_QUIET_SEND="0")
    out = subprocess.run([sys.executable, "-m", "tests.quiet_send_cases", name], cwd=ROOT, env=env, check=True,
                         stdout=subprocess.PIPE, timeout=120).stdout
    generic = json.loads(out.decode().strip().splitlines()[-1])
    print(f"{name}: lean {ROUNDS - lean['merge_launches']} quiet rounds taken, send bytes {lean['send_bytes']} "
          f"units {lean['send_units']}; generic {ROUNDS - generic['merge_launches']}, {generic['send_bytes']}, "
          f"{generic['send_units']}")
    for fp in (lean, generic):  # both took the quiet path (the host's side is the same), then it is not compared
        assert ROUNDS - fp.pop("merge_launches") >= cases.MIN_PREDICTED[name] // 2
    diff = {k: (lean[k], generic[k]) for k in lean if lean[k] != generic[k] and k != "hosts"}
    assert not diff, diff
    assert lean["hosts"] == generic["hosts"]
