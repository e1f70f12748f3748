"""Return codes of the single-host ABI calls (sidecar_amd/csrc/gx_api_host.hpp) for the arguments
every one of them checks before it touches the device: a null engine, and a view, host or owner id
outside the engine's range, are GX_EINVAL. The engine is the smallest gx_create accepts with two
services (8 hosts x 2); every other argument of a call is valid, so the id is what is refused."""
import ctypes as C

import pytest

from sidecar_amd.abi import GX_EINVAL, Engine, default_params

pytestmark = pytest.mark.gpu

H, S = 8, 2
BAD = H  # the first id past the engine's range (hosts, views and owners are 0 .. H - 1)

# gx.h entries of gx_api_host.hpp with their id arguments, by position after the engine. Each row is
# one call: the arguments named get the values given, every other integer is 0 (an empty list, a
# zero capacity) and every pointer a zeroed buffer.
BAD_IDS = [
    ("gx_notify_msg", {0: BAD}), ("gx_merge_remote_state", {0: BAD}), ("gx_merge", {0: BAD}), ("gx_merge", {1: BAD}),
    ("gx_tombstone_others", {0: BAD}), ("gx_tombstone_services", {0: BAD}), ("gx_expire_server", {0: BAD}),
    ("gx_expire_server", {1: BAD}), ("gx_notify_leave", {0: BAD}), ("gx_notify_leave", {1: BAD}),
    ("gx_send_services", {0: BAD, 3: 1}), ("gx_broadcast_services", {0: BAD}), ("gx_broadcast_tombstones", {0: BAD}),
    ("gx_owner_slots_in_use", {0: BAD}), ("gx_is_new_service", {0: BAD}), ("gx_get_broadcasts", {0: BAD}),
    ("gx_get_broadcasts_bytes", {0: BAD}), ("gx_set_static_bytes", {1: H + 1}), ("gx_local_state", {0: BAD}),
    ("gx_each_service_sorted", {0: BAD, 1: 0xFFFFFFFF}), ("gx_each_service_sorted", {1: BAD}), ("gx_by_service", {0: BAD}),
    ("gx_read_server_times", {0: BAD}), ("gx_read_server_times", {2: H + 1}), ("gx_read_last_changed", {0: BAD, 1: H + 1}),
    ("gx_add_listener", {0: BAD, 2: 1}), ("gx_read_views", {0: BAD, 1: H + 1}), ("gx_read_view", {0: BAD}),
    ("gx_write_views", {0: BAD, 1: H + 1}), ("gx_write_slot", {0: BAD}), ("gx_read_hosts", {0: BAD, 1: H + 1}),
    ("gx_read_queue", {0: BAD}), ("gx_read_sleepers", {0: BAD}), ("gx_read_pending", {0: BAD}), ("gx_read_list", {0: BAD}),
    ("gx_fd_read_members", {0: BAD}), ("gx_fd_read_hosts", {0: BAD, 1: H + 1}), ("gx_fd_read_queue", {0: BAD}),
    ("gx_fd_notify", {0: BAD}), ("gx_fd_get_broadcasts", {0: BAD}), ("gx_fd_probe", {0: BAD}), ("gx_fd_timers", {0: BAD}),
    ("gx_fd_merge_state", {0: BAD}),
]
# ... and the ones that take no id, or take it inside a list (below)
NO_ID = ["gx_add_service_entries", "gx_notify_msgs", "gx_message_bytes", "gx_set_service_names", "gx_epoch",
         "gx_remove_listener", "gx_listener_drain", "gx_host_digests", "gx_owner_words", "gx_view_minmax", "gx_stats_get",
         "gx_timing_get", "gx_fd_converged", "gx_converged"]
# diagnostics outside gx.h: (engine, a pointer or two)
UNDECLARED = {"gx_xplan_waits": 1, "gx_probe_cross": 1, "gx_kprof_read": 3}


def _args(fn, given, keep):
    out = []
    for i, t in enumerate(fn.argtypes[1:]):
        if i in given:
            out.append(given[i])
        elif issubclass(t, (C._Pointer, C.c_void_p, C.c_char_p)):
            buf = C.create_string_buffer(1 << 16)
            keep.append(buf)
            out.append(C.cast(buf, t))
        else:
            out.append(0)
    return out


@pytest.fixture(scope="module")
def engine(gx_lib):
    with Engine(default_params(gx_lib, n_hosts=H, n_services=S), lib=gx_lib) as e:
        yield e


def test_null_engine(gx_lib):
    keep = []
    for name in sorted({n for n, _ in BAD_IDS} | set(NO_ID)):
        fn = getattr(gx_lib, name)
        assert fn(None, *_args(fn, {}, keep)) == GX_EINVAL, name
    for name, nptr in UNDECLARED.items():
        bufs = [C.create_string_buffer(64) for _ in range(nptr)]
        args = [C.c_void_p(C.addressof(b)) for b in bufs]
        if name == "gx_kprof_read":
            args[1] = C.c_uint64(0)
        assert getattr(gx_lib, name)(C.c_void_p(None), *args) == GX_EINVAL, name


@pytest.mark.parametrize("name,given", BAD_IDS, ids=[f"{n}-{'_'.join(map(str, sorted(g)))}" for n, g in BAD_IDS])
def test_id_out_of_range(gx_lib, engine, name, given):
    keep = []
    fn = getattr(gx_lib, name)
    assert fn(engine.h, *_args(fn, given, keep)) == GX_EINVAL
    good = {i: (1 if v in (BAD, H + 1) else v) for i, v in given.items()}  # the same call with ids in range
    if not name.startswith("gx_fd_"):  # (the detector is off: those refuse every host)
        assert fn(engine.h, *_args(fn, good, keep)) != GX_EINVAL, f"{name}: the call is refused for another reason"


def test_id_in_a_list(gx_lib, engine):
    """gx_add_service_entries and gx_notify_msgs name their views per record."""
    views = (C.c_uint32 * 1)(BAD)
    recs = (gx_lib.gx_notify_msg.argtypes[2]._type_ * 1)()
    acc = C.c_uint32()
    assert gx_lib.gx_add_service_entries(engine.h, views, recs, 1, C.byref(acc)) == GX_EINVAL
    assert gx_lib.gx_notify_msgs(engine.h, views, recs, 1) == GX_EINVAL
    views[0] = 0
    assert gx_lib.gx_add_service_entries(engine.h, views, recs, 1, C.byref(acc)) == 0
    assert gx_lib.gx_notify_msgs(engine.h, views, recs, 1) == 0
