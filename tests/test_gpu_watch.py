"""The record watch (include/gx_watch.h) on the HIP engine: the device log of per-round holds,
older and live equals, row by row, the counts taken from an unsharded oracle engine's views after
every round (tests/watch_ref.py; tests/test_watch_ref_cpu.py shows on the oracle alone that these
schedules exercise every count). The watch changes nothing the engine computes."""
import numpy as np
import pytest

from sidecar_amd.abi import WATCH_ANY, WATCH_MAX, WATCH_OFF, Engine, GxError, default_params
from sidecar_amd.spread import owner_versions, spread_rounds
from tests.parity import assert_same, snapshot
from tests.watch_ref import ARM, ROUNDS, SCHEDULES, OracleWatch, entries, owner_version, spread_direct

pytestmark = pytest.mark.gpu


def pair(gx_lib, oracle_lib, name):
    kw = SCHEDULES[name]
    g = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    o = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    g.run_rounds(ARM)
    o.run_rounds(ARM)
    return g, o


def armed(gx_lib, oracle_lib, name, log_rounds=None):
    """HIP engine and oracle after ARM rounds, the schedule's entries set on both."""
    g, o = pair(gx_lib, oracle_lib, name)
    keys, thr = entries(name, o)
    g.watch_arm(len(keys), ROUNDS[name] if log_rounds is None else log_rounds)
    g.watch_set(0, keys, thr)
    ref = OracleWatch(o, len(keys))
    ref.set(0, keys, thr)
    return g, ref, keys, thr


def assert_log(g, ref, what, rows=None):
    counts, live, first_round, n_logged, missed = g.watch_read()
    want_c, want_l = ref.log()
    rows = len(want_l) if rows is None else rows
    assert first_round == ref.first_round and n_logged == rows, what
    bad = np.argwhere(counts != want_c[:rows])
    assert not len(bad), f"{what}: {len(bad)} counts differ, first (row, entry, holds|older) {bad[:5].tolist()}"
    assert np.array_equal(live, want_l[:rows]), what
    return counts, live, missed


@pytest.fixture(scope="module")
def odd_rows(gx_lib, oracle_lib):
    """Case 1, run once: 33 x 3, 70 entries, 5 rounds, arm, the schedule's rounds in uneven calls."""
    g, ref, keys, thr = armed(gx_lib, oracle_lib, "odd_rows")
    left = ROUNDS["odd_rows"]
    for chunk in (1, 2, 7, 30, left - 40):  # one gx_run_rounds call logs every round it runs
        g.run_rounds(chunk)
    ref.run(left)
    yield g, ref, keys, thr
    g.close()


def test_log_equals_reference_odd_rows(odd_rows):
    g, ref, keys, thr = odd_rows
    assert len(keys) == 70 and g.H * g.S == 99
    _, _, missed = assert_log(g, ref, "odd_rows")
    assert missed == 0
    # a range of rows
    counts, live, *_ = g.watch_read(3, 4)
    assert np.array_equal(counts, ref.log()[0][3:7]) and np.array_equal(live, ref.log()[1][3:7])


@pytest.mark.parametrize("name", ["storm", "fd"])
def test_log_equals_reference(gx_lib, oracle_lib, name):
    """storm: BASE's ExpireServer storm in the first watched round (tombstones are present slots,
    views behind on older versions); fd: hosts depart inside the window, their views are left out
    and live matches."""
    g, ref, keys, thr = armed(gx_lib, oracle_lib, name)
    g.run_rounds(ROUNDS[name])
    ref.run(ROUNDS[name])
    counts, live, _ = assert_log(g, ref, name)
    if name == "fd":
        assert live[-1] < live[0] == g.H
    assert_same(g, ref.orc, name)


def test_watch_set_mid_run(gx_lib, oracle_lib):
    """Entries rewritten after round k count with the old thresholds through round k and with the
    new ones from k + 1; the log is not reset."""
    g, ref, keys, thr = armed(gx_lib, oracle_lib, "odd_rows", log_rounds=30)
    g.run_rounds(10)
    ref.run(10)
    new_keys = np.array([k if k != WATCH_OFF else 12 for k in keys[:10]], dtype=np.uint32)  # the off entry goes on
    new_thr = np.array([owner_version(ref.orc, k) for k in new_keys], dtype=np.int64)
    assert (new_thr != thr[:10]).any()
    assert np.array_equal(owner_versions(g, new_keys), np.where(new_thr == WATCH_ANY, -1, new_thr))
    g.watch_set(0, new_keys, new_thr)
    ref.set(0, new_keys, new_thr)
    g.run_rounds(20)
    ref.run(20)
    counts, _, _ = assert_log(g, ref, "watch_set mid-run")
    assert (counts[:10, 4] == 0).all() and (counts[10:, 4] != 0).any()


def test_log_bound_and_rearm(gx_lib, oracle_lib):
    g, ref, keys, thr = armed(gx_lib, oracle_lib, "odd_rows", log_rounds=8)
    g.run_rounds(20)
    ref.run(20)
    _, _, missed = assert_log(g, ref, "log bound", rows=8)
    assert missed == 12
    with pytest.raises(GxError, match="rc=-22"):
        g.watch_read(0, 9)  # past n_logged
    # re-arming resets: entries off, an empty log from this round on
    g.watch_arm(len(keys), 8)
    assert g.watch_info() == (g.round, 0, 0)
    g.run_rounds(2)
    counts, live, first_round, n_logged, missed = g.watch_read()
    assert (first_round, n_logged, missed) == (ARM + 20, 2, 0)
    assert not counts.any() and (live == g.H).all()
    ref2 = OracleWatch(ref.orc, len(keys))
    ref.run(2)
    ref2.set(0, keys, thr)
    g.watch_set(0, keys, thr)
    g.run_rounds(3)
    ref2.run(3)
    assert np.array_equal(g.watch_read(2)[0], ref2.log()[0])


def test_watch_changes_nothing(gx_lib, odd_rows):
    """The watched engine equals the oracle, and an engine that never armed a watch."""
    g, ref, _, _ = odd_rows
    assert_same(g, ref.orc, "watched HIP engine vs oracle")
    plain = Engine(default_params(gx_lib, **SCHEDULES["odd_rows"]), lib=gx_lib)
    plain.run_rounds(g.round)
    a, b = snapshot(g), snapshot(plain)
    assert a["stats"] == b["stats"] and a["hosts"] == b["hosts"]
    for k in ("views", "digests", "times", "last_changed"):
        assert np.array_equal(a[k], b[k]), k
    plain.close()


def test_refusals(gx_lib):
    kw = dict(SCHEDULES["odd_rows"])
    g = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    R = g.H * g.S

    def refused(f, *a):
        with pytest.raises(GxError, match="rc=-22"):
            f(*a)

    refused(g.watch_info)  # no watch: read and set
    refused(g.watch_set, 0, [1], [WATCH_ANY])
    g.watch_arm(0)
    g.watch_arm(0)  # disarming twice is fine
    refused(g.watch_info)
    refused(g.watch_arm, WATCH_MAX + 1, 1)
    refused(g.watch_arm, 4, 0)
    refused(g.watch_arm, 1023, (256 << 20) // (8 * 1024) + 1)  # a log past 256 MiB
    g.watch_arm(1023, (256 << 20) // (8 * 1024))  # exactly 256 MiB
    g.watch_arm(WATCH_MAX, 2)
    g.watch_arm(4, 16)
    refused(g.watch_set, 0, [R], [WATCH_ANY])  # key >= R
    refused(g.watch_set, 3, [1, 2], [WATCH_ANY, WATCH_ANY])  # past n
    refused(g.watch_set, 0, [1], [g.epoch - 1])  # before the window
    refused(g.watch_set, 0, [1], [g.epoch + (1 << 61)])  # after it
    g.watch_set(0, [1, R - 1], [g.epoch, g.epoch + (1 << 61) - 1])  # the window's ends
    g.watch_set(2, [WATCH_OFF, 0], [0, g.now()])  # an off entry's time is not looked at
    g.run_rounds(3)
    counts, live, first_round, n_logged, missed = g.watch_read()
    assert (first_round, n_logged, missed) == (0, 3, 0) and counts.shape == (3, 4, 2)
    assert (counts[:, 1, 0] == 0).all() and (counts[:, 2] == 0).all()
    g.close()  # destroying an engine with an armed watch is clean
    g2 = Engine(default_params(gx_lib, **kw), lib=gx_lib)  # and leaves the device usable
    g2.run_rounds(2)
    g2.close()


def test_spread_rounds_on_the_log(odd_rows):
    g, ref, keys, thr = odd_rows
    counts, live, first_round, *_ = g.watch_read()
    for born in (first_round, first_round + 4):
        assert spread_rounds(counts, live, first_round, born) == spread_direct(ref.views, keys, thr, first_round, born)
    full, _ = spread_rounds(counts, live, first_round, first_round)
    assert any(x for x in full) and None in full
