"""The rule quiet rounds rest on, entry by entry: an ABI call that changes the engine
between rounds sends the next rounds down the generic path, and a call that only reads does not.
Which is which is the argument each entry gives the engine's entry guard (enter() in gx_engine.hip).

Schedule quiet_cases.SCHEDULES["h128"] (128 hosts x 16 services, 150 rounds), the HIP engine beside
the oracle. The merge class (gx_timing.launches) counts one launch per round on the generic path
and none in a quiet round.

test_mutating_entry has one case per entry the guard marks mutating that an unsharded engine without
the failure detector accepts. It cannot reach the others: gx_fd_notify, gx_fd_probe, gx_fd_timers,
gx_fd_merge_state and gx_fd_get_broadcasts need the detector, gx_inbox_unpack and the rest of the
sharded phase calls a second shard, and quiet rounds are predicted with neither. gx_set_names is in
the table because it rewrites the static message bytes, as gx_set_static_bytes does; before the
guard it was missing from the hand-kept list of invalidating entries, so that one case fails its
launch count on a library older than the guard (its parity check passes there too)."""
import pytest

from sidecar_amd.abi import ALIVE, TOMBSTONE, Engine, default_params
from sidecar_amd.codec import synthetic_names
from tests import quiet_cases
from tests.parity import assert_same, snapshot
from tests.test_gpu_quiet_rounds import assert_snap, merge_launches

pytestmark = pytest.mark.gpu

NAME = "h128"
KW = quiet_cases.SCHEDULES[NAME]
ROUNDS = quiet_cases.ROUNDS
QUIET_BY = 100  # a case that has seen no quiet round by this round fails as vacuous
H, S = KW["n_hosts"], KW["n_services"]


def _phase_round(e):
    e.round_send()
    e.round_merge()
    if e.is_ae_round():
        e.ae_merge()
    e.round_end()


def _listener(e):
    e.add_listener(3, 1, 16)
    assert e.remove_listener(3, 1) == 0


def _json(e):
    rc, _ = e.merge_remote_state_json(5, e.local_state_json(70))
    assert rc == 0


# Each call, made on both engines with the same arguments at the same round (t = that round's time).
# Where a call changes state, parity to round 150 covers it.
CALLS = {
    "gx_set_round": lambda e, t: e.set_round(e.round),
    "gx_add_service_entries": lambda e, t: e.add_service_entries([3, 70], [(3, 5, t, ALIVE), (9, 1, t, TOMBSTONE)]),
    "gx_notify_msg": lambda e, t: e.notify_msg(4, [(7, 2, t, ALIVE)]),
    "gx_notify_msgs": lambda e, t: e.notify_msgs([4, 4, 9], [(7, 2, t, ALIVE), (8, 0, t, ALIVE), (100, 3, t, TOMBSTONE)]),
    "gx_merge_remote_state": lambda e, t: e.merge_remote_state(5, [(9, 1, t, ALIVE), (110, 0, t, TOMBSTONE)]),
    "gx_merge_remote_state_json": lambda e, t: _json(e),
    "gx_merge": lambda e, t: e.merge(6, 70),
    "gx_tombstone_others": lambda e, t: e.tombstone_others(3),
    "gx_tombstone_services": lambda e, t: e.tombstone_services(3, [0, 1, 2]),
    "gx_expire_server": lambda e, t: e.expire_server(3, 100),
    "gx_notify_leave": lambda e, t: e.notify_leave(4, 101),
    "gx_send_services": lambda e, t: e.send_services(3, [(3, 0, t, ALIVE)], 2),
    "gx_broadcast_services": lambda e, t: e.broadcast_services(3, [(3, 1, t, ALIVE)]),
    "gx_broadcast_tombstones": lambda e, t: e.broadcast_tombstones(3, [(3, 2, t, TOMBSTONE)]),
    "gx_get_broadcasts": lambda e, t: e.get_broadcasts(3),
    "gx_get_broadcasts_bytes": lambda e, t: e.get_broadcasts_bytes(3, 3, 1400),
    "gx_set_static_bytes": lambda e, t: e.set_static_bytes(0, 2, [100] * (2 * S)),
    "gx_set_names": lambda e, t: e.set_names(synthetic_names(H, S, seed=7)),
    "gx_write_views": lambda e, t: e.write_views(e.read_views(3, 5), lo=3),
    "gx_write_slot": lambda e, t: e.write_slot(3, (20, 1, t, ALIVE)),
    "gx_add_listener+gx_remove_listener": lambda e, t: _listener(e),
    "gx_set_stream": lambda e, t: e.set_stream(None, False),
    "phase_calls_round": lambda e, t: _phase_round(e),
}


def _pair(gx_lib, oracle_lib):
    return (Engine(default_params(gx_lib, **KW), lib=gx_lib), Engine(default_params(oracle_lib, **KW), lib=oracle_lib))


def _step(g):
    """One round in one call; whether it took the quiet path."""
    before = merge_launches(g)
    g.run_rounds(1)
    return merge_launches(g) == before


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_mutating_entry(gx_lib, oracle_lib, entry):
    g, o = _pair(gx_lib, oracle_lib)
    if entry == "gx_merge_remote_state_json":  # the codec's names, from the start on both
        for e in (g, o):
            e.set_names(synthetic_names(H, S, seed=5))
    while not _step(g):
        assert g.round < QUIET_BY, f"no quiet round by round {QUIET_BY}: the case shows nothing"
    found = g.round - 1
    o.run_rounds(g.round)
    t = g.now()
    for e in (g, o):
        CALLS[entry](e, t)
    assert g.round == o.round
    before = merge_launches(g)
    g.run_rounds(2)
    assert merge_launches(g) - before == 2, f"{entry}: a round after the call took the quiet path"
    again = 0
    while g.round < ROUNDS:
        again += _step(g)
    o.run_rounds(ROUNDS - o.round)
    print(f"{entry}: first quiet round {found}, {again} quiet rounds after the call")
    assert_same(g, o, f"{entry} round {ROUNDS}")
    assert again >= 1, f"{entry}: the quiet path is not found again after the call"


def test_readers_do_not_invalidate(gx_lib):
    """Every read-only entry after every round: as many quiet rounds as calls of one round alone
    must find (test_gpu_quiet_rounds.test_parity's bound), and the oracle's state at round 150."""
    want = quiet_cases.oracle_trace(NAME)["snaps"][ROUNDS]
    g = Engine(default_params(gx_lib, **KW), lib=gx_lib)
    g.set_service_names([f"svc-{r % S}" for r in range(H * S)])  # ByService's names: nothing a round reads
    rec = (3, 5, g.now(), ALIVE)
    quiet = 0
    while g.round < ROUNDS:
        quiet += _step(g)
        v = g.round % H
        snapshot(g)
        g.stats(), g.timing(), g.read_views(), g.hosts(), g.digests(), g.converged()
        g.queue(v), g.sleepers(v), g.pending(v), g.read_list(v, 0), g.local_state(v)
        g.each_service_sorted(v), g.each_service_sorted(v, 3), g.by_service(v)
        g.server_times(v), g.last_changed(), g.is_new_service(v, rec), g.owner_slots_in_use(v)
        g.message_bytes([rec, (9, 1, g.now(), TOMBSTONE)])
    print(f"{quiet} rounds took the quiet path with every reader called between the rounds")
    assert quiet >= quiet_cases.MIN_PREDICTED[NAME] // 2
    assert_snap(g, want, f"{NAME} readers round {ROUNDS}")
