"""The record watch on sharded HIP engines (LocalShards on one GPU): each shard counts its own
views, also for keys whose owner lives on another shard, and the logs summed over the shards equal
the unsharded HIP engine's log and the counts taken from an unsharded oracle's views, round by
round: planned rounds, sized rounds (gossip_messages = 4), and push-pull rounds that the all-locked
census replaces (gx_ae_skip_locked)."""
import numpy as np
import pytest

from sidecar_amd.abi import WATCH_ANY, WATCH_OFF, Engine, default_params
from sidecar_amd.dist import LocalShards
from sidecar_amd.spread import owner_versions
from tests.test_shards_cpu import LOCKED, SCEN
from tests.watch_ref import ARM, SCHEDULES, OracleWatch, entries, owner_version

pytestmark = pytest.mark.gpu

ROUNDS = 40


def ragged_entries(orc):
    """70 x 11 (R = 770): 130 entries over every shard's owners, three waves' worth with a tail."""
    R = orc.H * orc.S
    keys = [(17 * i + 5) % R for i in range(130)]
    keys[9] = WATCH_OFF
    thr = [owner_version(orc, k) if k != WATCH_OFF else 0 for k in keys]
    thr[11] = WATCH_ANY
    return np.array(keys, dtype=np.uint32), np.array(thr, dtype=np.int64)


def locked_entries(orc):
    R = orc.H * orc.S
    keys = [(37 * i + 2) % R for i in range(64)]
    # INIT_WARM: every view starts with every record; the versions to come are the ones to watch
    thr = [owner_version(orc, k) + (1 if i % 2 else 0) for i, k in enumerate(keys)]
    return np.array(keys, dtype=np.uint32), np.array(thr, dtype=np.int64)


CASES = {
    # name: (schedule, G, entries)
    "odd_rows_g2": (SCHEDULES["odd_rows"], 2, lambda o: entries("odd_rows", o)),
    "odd_rows_g3": (SCHEDULES["odd_rows"], 3, lambda o: entries("odd_rows", o)),
    "odd_rows_g5": (SCHEDULES["odd_rows"], 5, lambda o: entries("odd_rows", o)),
    "odd_rows_gm4_g3": (dict(SCHEDULES["odd_rows"], gossip_messages=4), 3, lambda o: entries("odd_rows", o)),
    "ragged_g8": (SCEN["blocks_ragged"], 8, ragged_entries),
    "locked_g2": (LOCKED, 2, locked_entries),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_summed_logs_equal_whole_and_oracle(gx_lib, oracle_lib, name):
    kw, G, make = CASES[name]
    whole = Engine(default_params(gx_lib, **kw), lib=gx_lib)
    orc = Engine(default_params(oracle_lib, **kw), lib=oracle_lib)
    sh = LocalShards(gx_lib, G, device="cuda:0", **kw)
    for x in (whole, orc, sh):
        x.run_rounds(ARM)
    keys, thr = make(orc)
    on = keys != WATCH_OFF
    assert len({int(k) // orc.S * G // orc.H for k in keys[on]}) > 1  # owners on several shards
    # the helper reads each key from the shard that owns it
    assert np.array_equal(owner_versions(sh, keys[on]), owner_versions(orc, keys[on]))
    ref = OracleWatch(orc, len(keys))
    ref.set(0, keys, thr)
    for x in (whole, sh):
        x.watch_arm(len(keys), ROUNDS)
        x.watch_set(0, keys, thr)
    whole.run_rounds(ROUNDS)
    sh.run_rounds(ROUNDS)
    ref.run(ROUNDS)
    want_c, want_l = ref.log()
    counts, live, first_round, n_logged, missed = sh.watch_read()
    assert (first_round, n_logged, missed) == (ARM, ROUNDS, 0)
    wc, wl, *_ = whole.watch_read()
    assert np.array_equal(counts, wc) and np.array_equal(live, wl), f"{name}: shards vs the unsharded HIP engine"
    bad = np.argwhere(counts != want_c)
    assert not len(bad), f"{name}: {len(bad)} counts differ from the oracle's, first {bad[:5].tolist()}"
    assert np.array_equal(live, want_l)
    # every shard saw records of owners it does not hold
    for e in sh.engines:
        c = e.watch_read()[0].astype(np.int64)
        foreign = np.array([k != WATCH_OFF and not e.lo <= int(k) // e.S < e.hi for k in keys])
        assert c[:, foreign].sum() > 0
    gm = kw.get("gossip_messages", 1)
    assert sh.exchange_paths == ({"planned": 0, "sized": ARM + ROUNDS} if gm > 1 else {"planned": ARM + ROUNDS, "sized": 0})
    if name == "locked_g2":  # push-pull rounds with every host locked end through gx_ae_skip_locked
        assert sh.ae_skipped > 0
        assert (counts[:, :, 1] > 0).any()
    views = np.concatenate([e.read_views() for e in sh.engines])
    assert np.array_equal(views, orc.read_views())
    for e in sh.engines:
        e.close()
    whole.close()
