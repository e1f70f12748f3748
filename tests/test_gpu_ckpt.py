"""Engine checkpoints (include/gx_ckpt.h) on the HIP engine: an engine restored from a file continues
bit for bit as the saved one (and as the oracle's uninterrupted run); the device's view coder writes
and reads exactly what the numpy reference of the format does (tests/ckpt_ref.py); damaged files,
saves inside a round and overrides a fork may not make are refused by validation; a fork into a
schedule whose events have not begun equals the oracle's run of that schedule from round 0; saving
changes nothing, the quiet-round bounds included."""
import numpy as np
import pytest

from sidecar_amd.abi import (CK_SRVT, CK_VIEW, CKPT_VIEWS, GX_EINVAL, GX_EIO, INIT_OWN, INIT_WARM, Engine, GxError,
                             ckpt_params, default_params)
from tests import ckpt_cases, ckpt_ref, quiet_cases
from tests.fd_parity import assert_same_fd
from tests.parity import assert_same
from tests.test_gpu_quiet_rounds import assert_snap, merge_launches

pytestmark = pytest.mark.gpu


def _eng(lib, **kw):
    return Engine(default_params(lib, **kw), lib=lib)


# ----------------------------------------------------------------------------- continuity --
@pytest.mark.parametrize("name", sorted(ckpt_cases.RUNS))
def test_continuity(gx_lib, oracle_lib, tmp_path, name):
    """A runs n1, saves, runs n2; B and C, both restored from the file, run n2: A = B = C = the oracle
    after n1 + n2 (the save rounds: tests/ckpt_cases.py)."""
    kw, okw, n1, n2, fd = ckpt_cases.RUNS[name]
    path = tmp_path / "a.gxck"
    a, o = _eng(gx_lib, **kw), _eng(oracle_lib, **okw)
    a.run_rounds(n1)
    o.run_rounds(n1)
    info = a.ckpt_save(path)
    assert info["sections"][CK_VIEW]["coding"] == CKPT_VIEWS and info["file_bytes"] == path.stat().st_size
    p, r = ckpt_params(gx_lib, path)
    assert r == n1 and bytes(p) == bytes(a.params)
    b, c = Engine.from_checkpoint(path, lib=gx_lib), Engine.from_checkpoint(path, lib=gx_lib)
    assert b.round == c.round == n1 and (b.H, b.S, b.lo, b.hi) == (a.H, a.S, a.lo, a.hi)
    assert_same(b, c, f"{name}: two loads")
    assert_same(a, b, f"{name}: restored at round {n1}")
    for e in (a, b, c, o):
        e.run_rounds(n2)
    assert_same(a, b, f"{name}: saved at {n1}, round {a.round}")
    assert_same(b, c, f"{name}: two loads, round {a.round}")
    assert_same(b, o, f"{name}: restored vs oracle, round {a.round}")
    if fd:
        assert_same_fd(b, a, f"{name}: members")
        assert_same_fd(b, o, f"{name}: members vs oracle")


def test_continuity_quiet_stretch(gx_lib, tmp_path):
    """h128 saved at round 60, inside a stretch of rounds the device has predicted quiet (the oracle's
    trace), restored and run to 150 against the oracle's snapshots at rounds 100 and 150."""
    t = quiet_cases.oracle_trace("h128")
    assert {58, 59, 60} <= t["predicted"]  # rounds 52..60 are one predicted stretch
    a = _eng(gx_lib, **t["params"])
    a.run_rounds(60)
    a.ckpt_save(tmp_path / "q.gxck")
    b = Engine.from_checkpoint(tmp_path / "q.gxck", lib=gx_lib)
    for stop in (100, 150):
        for e in (a, b):
            while e.round < stop:
                e.run_rounds(1)  # the device caught up at every call: the bounds are seen
            assert_snap(e, t["snaps"][stop], f"h128 round {stop}")
    # the restored engine's bounds started from nothing: it skips the receive phase in no round the
    # oracle does not call quiet (its launch counts start at the load: 90 rounds)
    later_quiet = sum(1 for r in t["quiet"] if r >= 60)
    assert 90 - later_quiet <= merge_launches(b) <= 90


# ------------------------------------------------------------- coding against the reference --
def _mixed_views(e, seed):
    """Views for write_views that take every path of the coder: equal rows, rows differing in a few
    slots at block edges, one row that must go raw."""
    rng = np.random.default_rng(seed)
    Hl, R = e.hi - e.lo, e.H * e.S
    base = (rng.integers(1 << 20, 1 << 30, size=R, dtype=np.uint64) << np.uint64(3)) | np.uint64(1)
    v = np.tile(base, (Hl, 1))
    nblk = ckpt_ref.nblk_of(R)
    for i in range(0, Hl, 2):
        b = i % nblk
        v[i, b * 512] -= np.uint64(8)
        v[i, min(R, (b + 1) * 512) - 1] -= np.uint64(8)
        v[i, rng.integers(0, R, size=3)] -= np.uint64(16)
    v[1] -= np.uint64(8)
    return v


@pytest.mark.parametrize("H,S", [(4, 1), (33, 3), (64, 8), (19, 27), (70, 11), (96, 16)])
def test_coding_against_reference(gx_lib, tmp_path, H, S):
    """R = 4, 99, 512, 513, 770, 1536. The file's view section is byte for byte the reference
    writer's and decodes to read_views(), for a run's own state and for views that take every path of
    the coder; a file the reference wrote loads and reads back equal."""
    R = H * S
    e = _eng(gx_lib, n_hosts=H, n_services=S, init_mode=INIT_OWN, churn_ppm=50000, ae_period_rounds=5, queue_cap=4096)
    e.run_rounds(12)
    for what in ("run", "mixed"):
        if what == "mixed":
            e.write_views(_mixed_views(e, R))
        path = tmp_path / f"{what}.gxck"
        info = e.ckpt_save(path)
        views = e.read_views()
        f = ckpt_ref.CkptFile.read(path)  # verifies every checksum
        coding, raw, body = f.sections[CK_VIEW]
        assert (coding, raw) == (CKPT_VIEWS, 8 * H * R)
        assert np.array_equal(ckpt_ref.decode_views(body, H, R), views), what
        assert len(body) == ckpt_ref.view_section_bytes(views) == info["sections"][CK_VIEW]["stored_bytes"]
        assert body == ckpt_ref.encode_views(views), what
        if what == "mixed":
            assert info["views_raw"] >= 1
    # the other way: the reference writes the file, the engine's decoder reads it
    other = _mixed_views(e, R + 1)
    f.sections[CK_VIEW] = (CKPT_VIEWS, 8 * H * R, ckpt_ref.encode_views(other))
    f.write(tmp_path / "ref.gxck")
    g = Engine.from_checkpoint(tmp_path / "ref.gxck", lib=gx_lib)
    assert np.array_equal(g.read_views(), other)
    assert g.round == e.round and g.stats() == e.stats()


def test_warm_view_section_size(gx_lib, tmp_path):
    """A warm engine's views all equal base: 8 R + Hl * 8 * (1 + ceil(nblk / 64)) bytes."""
    e = _eng(gx_lib, n_hosts=70, n_services=11, init_mode=INIT_WARM)
    info = e.ckpt_save(tmp_path / "w.gxck")
    R = 770
    assert info["sections"][CK_VIEW]["stored_bytes"] == 8 * R + 70 * 8 * (1 + ckpt_ref.pw_of(R))
    assert info["views_raw"] == 0 and info["chunks"] >= 1


# -------------------------------------------------------------------------------- refusals --
def _rc(call):
    with pytest.raises(GxError) as err:
        call()
    return err.value.rc


def test_save_inside_a_round_is_refused(gx_lib, oracle_lib, tmp_path):
    kw = dict(n_hosts=32, n_services=4, init_mode=INIT_OWN, ae_period_rounds=3, queue_cap=4096)
    g, o = _eng(gx_lib, **kw), _eng(oracle_lib, **kw)
    g.run_rounds(4)
    o.run_rounds(5)
    g.round_send()
    assert _rc(lambda: g.ckpt_save(tmp_path / "x.gxck")) == GX_EINVAL
    assert not (tmp_path / "x.gxck").exists()
    g.round_merge()
    assert _rc(lambda: g.ckpt_save(tmp_path / "x.gxck")) == GX_EINVAL
    g.round_end()
    assert_same(g, o, "the round completed after the refused save")
    g.ckpt_save(tmp_path / "x.gxck")
    b = Engine.from_checkpoint(tmp_path / "x.gxck", lib=gx_lib)
    for e in (g, b, o):
        e.run_rounds(7)
    assert_same(b, o, "restored after the completed round")


def test_damaged_files_are_refused(gx_lib, tmp_path):
    """Every one is rejected by validation (no device fault: the process goes on to load the intact
    file and run it)."""
    kw = dict(n_hosts=33, n_services=3, init_mode=INIT_OWN, churn_ppm=50000, ae_period_rounds=5, queue_cap=4096)
    e = _eng(gx_lib, **kw)
    e.run_rounds(12)
    e.write_views(_mixed_views(e, 5))  # view 0 is coded, with literals
    good = tmp_path / "good.gxck"
    e.ckpt_save(good)
    data = good.read_bytes()
    bad = tmp_path / "bad.gxck"

    def load_rc(b, **override):
        bad.write_bytes(b)
        return _rc(lambda: Engine.from_checkpoint(bad, lib=gx_lib, **override))

    head = ckpt_ref.HEADER_BYTES + ckpt_ref.pad8(len(bytes(e.params)))
    assert load_rc(data[:len(data) // 2]) == GX_EIO  # truncated
    assert load_rc(data[:-8]) == GX_EIO
    assert load_rc(data[:20]) == GX_EIO
    for at in (0, 9, 26, ckpt_ref.HEADER_BYTES + 2, head + 9):  # magic, format, round, params, table
        b = bytearray(data)
        b[at] ^= 0x04
        assert load_rc(bytes(b)) == GX_EIO, at
        assert _rc(lambda: ckpt_params(gx_lib, bad)) == GX_EIO
    f = ckpt_ref.CkptFile.read(good)
    coding, raw, body = f.sections[CK_VIEW]
    # payload bytes, caught by the sections' checksums: base, the last view record, the server times
    for at in (f.offsets[CK_VIEW] + 3, f.offsets[CK_VIEW] + len(body) - 1, f.offsets[CK_SRVT] + 100):
        b = bytearray(data)
        b[at] ^= 0x40
        assert load_rc(bytes(b)) == GX_EIO, at
    # a view record whose n_lit disagrees with its masks, the checksum recomputed: the device's check
    w = np.frombuffer(body, dtype="<u8").copy()
    R, PW = 99, 1
    at = R  # view 0's record

    def u64(x):
        return np.array([x], dtype=np.uint64)

    nl, npres = int(w[at]), bin(int(w[at + 1])).count("1")
    end = at + 1 + PW + 8 * npres + nl
    assert 2 <= nl < 80 and npres == 1
    more = np.concatenate([w[:at], u64(nl + 1), w[at + 1:end], w[end - 1:end], w[end:]])  # a literal the masks do not have
    less = np.concatenate([w[:at], u64(nl - 1), w[at + 1:end - 1], w[end:]])               # a literal fewer than they say
    past = w.copy()
    past[at + 1 + PW + 1] |= np.uint64(1 << 40)  # slot 64 + 40 >= R = 99 (and a literal more, so n_lit matches)
    past = np.concatenate([past[:at], u64(nl + 1), past[at + 1:end], w[end - 1:end], past[end:]])
    stray = w.copy()
    stray[at + 1] |= np.uint64(1 << 5)  # a present bit past the last block
    for what, w2 in (("more", more), ("less", less), ("past", past), ("stray", stray)):
        f.sections[CK_VIEW] = (coding, raw, w2.astype("<u8").tobytes())
        f.write(bad)  # (every checksum recomputed)
        assert _rc(lambda: Engine.from_checkpoint(bad, lib=gx_lib)) == GX_EIO, what
    # params with another n_hosts: as an override, and in a file whose header says so
    assert _rc(lambda: Engine.from_checkpoint(good, lib=gx_lib, n_hosts=34)) == GX_EINVAL
    f = ckpt_ref.CkptFile.read(good)
    p = type(e.params).from_buffer_copy(f.params)
    p.n_hosts = 34
    f.params = bytes(p)
    f.write(bad)
    assert _rc(lambda: Engine.from_checkpoint(bad, lib=gx_lib)) == GX_EINVAL
    # the intact file still loads and continues as the saved engine
    b = Engine.from_checkpoint(good, lib=gx_lib)
    for x in (e, b):
        x.run_rounds(9)
    assert_same(e, b, "after the refusals")


def test_overrides_a_fork_may_not_make(gx_lib, tmp_path):
    kw = dict(n_hosts=32, n_services=4, init_mode=INIT_OWN, ae_period_rounds=5, queue_cap=4096, storm_round=5,
              partition_start=2, partition_end=30, depart_round=8, depart_ppm=100000)
    e = _eng(gx_lib, **kw)
    e.run_rounds(10)
    path = tmp_path / "f.gxck"
    e.ckpt_save(path)
    for bad in (dict(seed=7), dict(ae_period_rounds=7), dict(n_services=5), dict(lock_buffer=64),
                dict(storm_round=40), dict(storm_round=-1),          # the saved storm has begun
                dict(partition_end=60), dict(partition_start=20),   # the saved partition has begun
                dict(depart_ppm=50000), dict(depart_round=30)):      # the saved departures have begun
        assert _rc(lambda: Engine.from_checkpoint(path, lib=gx_lib, **bad)) == GX_EINVAL, bad
    e2 = _eng(gx_lib, n_hosts=32, n_services=4, init_mode=INIT_OWN, ae_period_rounds=5, queue_cap=4096)
    e2.run_rounds(10)
    e2.ckpt_save(path)
    for bad in (dict(storm_round=10), dict(storm_round=3), dict(depart_round=10, depart_ppm=1000),
                dict(partition_start=10, partition_end=20)):        # the new event would have begun
        assert _rc(lambda: Engine.from_checkpoint(path, lib=gx_lib, **bad)) == GX_EINVAL, bad
    Engine.from_checkpoint(path, lib=gx_lib, storm_round=11, device=0).close()


# ------------------------------------------------------------------------------------ fork --
FORK_BASE = dict(n_hosts=48, n_services=6, init_mode=INIT_OWN, churn_ppm=40000, ae_period_rounds=5, queue_cap=4096,
                 alive_interval_rounds=2, tombstone_interval_rounds=7)
FORKS = {"storm": dict(storm_round=30), "partition": dict(partition_start=30, partition_end=45),
         "depart": dict(depart_round=30, depart_ppm=100000)}


@pytest.fixture(scope="module")
def fork_file(gx_lib, tmp_path_factory):
    e = _eng(gx_lib, **FORK_BASE)
    e.run_rounds(20)
    path = tmp_path_factory.mktemp("fork") / "r20.gxck"
    e.ckpt_save(path)
    return path


@pytest.mark.parametrize("name", sorted(FORKS))
def test_fork(gx_lib, oracle_lib, fork_file, name):
    """One schedule without events saved at round 20, forked into an event that begins at round 30:
    the oracle's run of that schedule from round 0, at rounds 31, 46 and 80."""
    o = _eng(oracle_lib, **dict(FORK_BASE, **FORKS[name]))
    g = Engine.from_checkpoint(fork_file, lib=gx_lib, **FORKS[name])
    o.run_rounds(20)
    assert_same(g, o, f"fork {name} at the saved round")
    for stop in (31, 46, 80):
        for e in (g, o):
            e.run_rounds(stop - e.round)
        assert_same(g, o, f"fork {name} round {stop}")
    st = o.stats()
    assert {"storm": st["expire_server"] > 0, "partition": True, "depart": True}[name]


# ---------------------------------------------------------------------- save is read-only --
def test_save_is_read_only(gx_lib, tmp_path):
    """h128 to round 150 in calls of one round, one engine saving every 10 rounds: equal throughout,
    and both take the same number of quiet rounds (the merge class's launches, as
    tests/test_gpu_quiet_rounds.py counts them): a save keeps the quiet-round bounds."""
    t = quiet_cases.oracle_trace("h128")
    a, b = _eng(gx_lib, **t["params"]), _eng(gx_lib, **t["params"])
    for r in range(1, 151):
        a.run_rounds(1)
        b.run_rounds(1)
        if r % 10 == 0:
            a.ckpt_save(tmp_path / "s.gxck")
            assert_same(a, b, f"round {r}")
    assert_snap(a, t["snaps"][150], "the saving engine, round 150")
    na, nb = merge_launches(a), merge_launches(b)
    print(f"merge launches: saving {na}, not saving {nb}; the oracle has {len(t['quiet'])} quiet rounds")
    assert na == nb < 150
