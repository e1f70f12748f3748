"""The GPU watch tests (tests/test_gpu_watch.py) are not vacuous: on the oracle alone, with their
schedules, seeds, rounds and entries (tests/watch_ref.py), the expected log shows a version
reaching every view inside the window, views behind on an older version, views without the record,
and, in the departure schedule, live views dropping. Also sidecar_amd.spread.spread_rounds against
latencies taken straight from the oracle's per-round views, and the sharded schedules' parameters
on oracle shards."""
import numpy as np
import pytest

from sidecar_amd.abi import Engine, default_params
from sidecar_amd.spread import spread_rounds
from tests.watch_ref import ARM, ROUNDS, SCHEDULES, OracleWatch, entries, spread_direct


def reference(oracle_lib, name, rounds=None):
    orc = Engine(default_params(oracle_lib, **SCHEDULES[name]), lib=oracle_lib)
    orc.run_rounds(ARM)
    keys, thr = entries(name, orc)
    ref = OracleWatch(orc, len(keys))
    ref.set(0, keys, thr)
    ref.run(ROUNDS[name] if rounds is None else rounds)
    return ref, keys, thr


@pytest.fixture(scope="module", params=sorted(SCHEDULES))
def case(request, oracle_lib):
    return (request.param,) + reference(oracle_lib, request.param)


def test_reference_is_not_vacuous(case):
    name, ref, keys, thr = case
    counts, live = ref.log()
    holds, older = counts[:, :, 0].astype(np.int64), counts[:, :, 1].astype(np.int64)
    lv = live.astype(np.int64)[:, None]
    full = holds == lv
    assert ((~full[:-1]) & full[1:]).any(), "no entry goes from holds < live to holds == live"
    assert (older > 0).any(), "no view is ever behind"
    assert (lv - holds - older > 0).any(), "no view is ever without a watched record"
    assert (lv - holds - older >= 0).all() and (live <= ref.orc.H).all()
    if name == "fd":
        assert live[0] == ref.orc.H and live[-1] < live[0], "no host departs inside the window"
    else:
        assert (live == ref.orc.H).all()
    if name == "storm":  # the storm's tombstones are present slots that hold its version
        got = [ref.orc.read_view(v) for v in range(ref.orc.H)]
        assert any((st[keys[::2]] == 1).any() for _, st in got)


def test_entry_kinds(oracle_lib):
    """What the odd_rows entries are meant to show, each on the reference."""
    ref, keys, thr = reference(oracle_lib, "odd_rows")
    counts, live = ref.log()
    assert len(keys) == 70
    assert (counts[:, 4] == 0).all()  # off
    assert (counts[:, 5, 1] == 0).all() and (counts[:, 5, 0] > 0).all()  # any version: present = holds
    assert (counts[:, 6, 0] == 0).all() and (counts[:, 6, 1] > 0).any()  # the future version: nobody holds it
    assert keys[3] == keys[0] and (counts[:, 3] != counts[:, 0]).any()  # duplicates count independently
    assert (counts[:, 0, 0] + counts[:, 0, 1] == counts[:, 3, 0] + counts[:, 3, 1]).all()  # of the same slots


def test_spread_rounds_matches_direct(case):
    name, ref, keys, thr = case
    counts, live = ref.log()
    for born in (ref.first_round, ref.first_round + 3):
        assert spread_rounds(counts, live, ref.first_round, born) == \
            spread_direct(ref.views, keys, thr, ref.first_round, born)
    full, clean = spread_rounds(counts, live, ref.first_round, ref.first_round)
    assert any(x is not None and x > 0 for x in full) and any(x is None for x in full)
    assert name == "fd" or any(x is not None and x > 0 for x in clean)  # (fd: behind at the start or never)


def test_spread_rounds_small():
    counts = np.array([[[1, 2], [0, 0]], [[3, 0], [0, 0]], [[3, 0], [0, 3]]], dtype=np.uint32)
    live = np.array([3, 3, 3], dtype=np.uint32)
    assert spread_rounds(counts, live, 10, 10) == ([1, None], [1, 0])
    assert spread_rounds(counts, live, 10, [11, 12]) == ([0, None], [0, None])
    assert spread_rounds(counts[:0], live[:0], 10, 10) == ([None, None], [None, None])
    live0 = np.array([0, 3, 3], dtype=np.uint32)  # a row of a round that was jumped over shows nothing
    assert spread_rounds(counts, live0, 10, 10)[1] == [1, 1]
