"""Coded checkpoints (include/gx_ckpt.h gx_ckpt_save_coded) on the HIP engine: the server times in the
views' ROW CODING and the broadcast FIFOs as their stored windows. An engine restored from a coded
file continues bit for bit as the saving one, as one restored from the raw file of the same state and
as the oracle's uninterrupted run; the device's coders write and read exactly what the numpy
references of the format do (tests/ckpt_ref.py, tests/ckpt_fifo_ref.py); chunk seams change no byte;
damaged files are refused by validation. The schedules and what they cover: tests/ckpt_coded_cases.py."""
import os

import numpy as np
import pytest

from sidecar_amd.abi import (CK_FIFO, CK_HS, CK_SRVT, CK_VIEW, CKPT_CODE_FIFO, CKPT_CODE_SRVT, CKPT_FIFO, CKPT_RAW,
                             CKPT_VIEWS, GX_EINVAL, GX_EIO, GX_ENOMEM, Engine, GxError)
from tests import ckpt_coded_cases as cc
from tests import ckpt_fifo_ref, ckpt_ref, quiet_cases
from tests.parity import assert_same
from tests.test_gpu_ckpt import FORK_BASE, FORKS, _eng
from tests.test_gpu_quiet_rounds import assert_snap, merge_launches

pytestmark = pytest.mark.gpu

BOTH = CKPT_CODE_SRVT | CKPT_CODE_FIFO
MORE = 25  # rounds after the save: every ring of Q = 8 and Q = 16 goes round more than once


def _rc(call):
    with pytest.raises(GxError) as err:
        call()
    return err.value.rc


def _tables(e):
    return cc.srvt_table(e), cc.queues(e)


def _same_tables(a, b, what):
    (ta, qa), (tb, qb) = _tables(a), _tables(b)
    assert np.array_equal(ta, tb), f"{what}: server times"
    assert qa == qb, f"{what}: queues"


def _codings(info):
    return {k: info["sections"][k]["coding"] for k in (CK_VIEW, CK_FIFO, CK_SRVT)}


# ----------------------------------------------------------------------------- continuity --
@pytest.mark.parametrize("code", [CKPT_CODE_SRVT, CKPT_CODE_FIFO, BOTH])
@pytest.mark.parametrize("name,n1", cc.SAVES)
def test_continuity(gx_lib, oracle_lib, tmp_path, name, n1, code):
    """A runs n1, saves coded and raw, runs 25 more; B (from the coded file) and C (from the raw file)
    run 25: A = B = C = the oracle, server times of every view and queues of every host included."""
    a, o = cc.engine(gx_lib, name), cc.engine(oracle_lib, name)
    a.run_rounds(n1)
    o.run_rounds(n1)
    info = a.ckpt_save(tmp_path / "coded.gxck", code)
    a.ckpt_save(tmp_path / "raw.gxck")
    assert _codings(info) == {CK_VIEW: CKPT_VIEWS, CK_FIFO: CKPT_FIFO if code & CKPT_CODE_FIFO else CKPT_RAW,
                              CK_SRVT: CKPT_VIEWS if code & CKPT_CODE_SRVT else CKPT_RAW}
    assert info["file_bytes"] == (tmp_path / "coded.gxck").stat().st_size
    b = Engine.from_checkpoint(tmp_path / "coded.gxck", lib=gx_lib)
    c = Engine.from_checkpoint(tmp_path / "raw.gxck", lib=gx_lib)
    assert b.round == c.round == n1 and _codings(b.ckpt_info) == _codings(info)
    for x, what in ((b, "coded"), (c, "raw")):
        assert_same(a, x, f"{name}: restored from the {what} file at round {n1}")
        _same_tables(a, x, f"{name}: {what} file at round {n1}")
    _same_tables(a, o, f"{name}: the oracle at round {n1}")
    for e in (a, b, c, o):
        e.run_rounds(MORE)
    assert_same(a, b, f"{name}: saved at {n1}, round {a.round}")
    assert_same(b, c, f"{name}: coded vs raw file, round {a.round}")
    assert_same(b, o, f"{name}: restored vs oracle, round {a.round}")
    for x in (a, c, o):
        _same_tables(b, x, f"{name}: round {b.round}")


# ----------------------------------------------------------- bytes against the references --
@pytest.mark.parametrize("name,n1", cc.SAVES)
def test_bytes_against_references(gx_lib, tmp_path, name, n1):
    """The GX_CK_SRVT body is the row reference's encoding of the table read back from the engine, the
    GX_CK_FIFO body the FIFO reference's of its queues; sizes equal info; a file in which the
    references re-encoded both sections loads and reads back equal."""
    e = cc.engine(gx_lib, name)
    e.run_rounds(n1)
    path = tmp_path / "c.gxck"
    info = e.ckpt_save(path, BOTH)
    table, queues = cc.srvt_table(e, stored=True), cc.queues(e)  # (the times as the engine keeps them)
    Hl, W, Q = e.hi - e.lo, 2 * e.H, e.params.queue_cap
    f = ckpt_ref.CkptFile.read(path)  # verifies every checksum
    coding, raw, body = f.sections[CK_SRVT]
    want = ckpt_ref.encode_views(table)
    assert (coding, raw) == (CKPT_VIEWS, 8 * Hl * W)
    assert len(body) == len(want) == info["sections"][CK_SRVT]["stored_bytes"]
    assert body == want
    assert np.array_equal(ckpt_ref.decode_views(body, Hl, W), table)
    raw_rows = cc.srvt_rows(table)[0]
    assert info["coded"]["srvt_rows_raw"] == raw_rows and info["coded"]["srvt_chunks"] >= 1
    coding, raw, body = f.sections[CK_FIFO]
    want = ckpt_fifo_ref.encode(queues)
    assert (coding, raw) == (CKPT_FIFO, 16 * Hl * Q)
    assert len(body) == len(want) == info["sections"][CK_FIFO]["stored_bytes"]
    assert body == want
    assert ckpt_fifo_ref.decode(body, Hl, Q, ckpt_fifo_ref.windows_of(e.hosts())) == queues
    assert info["coded"]["fifo_jobs"] == sum(map(len, queues))
    # the other way: a raw file whose two sections the references coded
    e.ckpt_save(tmp_path / "r.gxck")
    g = ckpt_ref.CkptFile.read(tmp_path / "r.gxck")
    assert g.sections[CK_SRVT][0] == g.sections[CK_FIFO][0] == CKPT_RAW
    g.sections[CK_SRVT] = (CKPT_VIEWS, 8 * Hl * W, ckpt_ref.encode_views(table))
    g.sections[CK_FIFO] = (CKPT_FIFO, 16 * Hl * Q, ckpt_fifo_ref.encode(queues))
    g.write(tmp_path / "ref.gxck")
    assert (tmp_path / "ref.gxck").read_bytes() == path.read_bytes()
    b = Engine.from_checkpoint(tmp_path / "ref.gxck", lib=gx_lib)
    assert_same(e, b, f"{name}: the references' file")
    _same_tables(e, b, f"{name}: the references' file")


@pytest.mark.parametrize("name", ["warm257", "warm256"])
def test_warm_sizes(gx_lib, tmp_path, name):
    """A warm cluster as created: every server-time row equals base, every FIFO is empty."""
    e = cc.engine(gx_lib, name)
    info = e.ckpt_save(tmp_path / "w.gxck", BOTH)
    H = e.H
    nblk = (2 * H + 511) // 512
    assert info["sections"][CK_SRVT]["stored_bytes"] == 16 * H + H * 8 * (1 + (nblk + 63) // 64)
    assert info["sections"][CK_FIFO]["stored_bytes"] == ckpt_fifo_ref.pad8(4 * H)
    assert info["coded"]["srvt_rows_raw"] == 0 and info["coded"]["fifo_jobs"] == 0 and info["coded"]["fifo_chunks"] == 0
    b = Engine.from_checkpoint(tmp_path / "w.gxck", lib=gx_lib)
    assert_same(e, b, name)


@pytest.mark.parametrize("name,n1", [("q8", 12), ("warm257", 20)])
def test_code_zero_is_the_plain_save(gx_lib, tmp_path, name, n1):
    """gx_ckpt_save_coded with code 0 (and null info structs) writes gx_ckpt_save's file, byte for byte."""
    e = cc.engine(gx_lib, name)
    e.run_rounds(n1)
    e.ckpt_save(tmp_path / "plain.gxck")
    assert gx_lib.gx_ckpt_save_coded(e.h, os.fsencode(tmp_path / "zero.gxck"), 0, None, None) == 0
    assert (tmp_path / "plain.gxck").read_bytes() == (tmp_path / "zero.gxck").read_bytes()
    f = ckpt_ref.CkptFile.read(tmp_path / "zero.gxck")
    assert all(coding == (CKPT_VIEWS if sid == CK_VIEW else CKPT_RAW) for sid, (coding, _, _) in f.sections.items())


def test_block_per_host_rings(gx_lib, oracle_lib, tmp_path):
    """Rings above 1024 jobs take the FIFO kernels' block-per-host form (the schedules above take the
    wave-per-host one): the q8 schedule with rings of 1100 jobs, bytes against the reference and
    continuity against the oracle."""
    a, o = cc.engine(gx_lib, "q8", queue_cap=1100), cc.engine(oracle_lib, "q8", queue_cap=1100)
    a.run_rounds(12)
    o.run_rounds(12)
    info = a.ckpt_save(tmp_path / "c.gxck", BOTH)
    queues = cc.queues(a)
    assert queues == cc.queues(o) and max(map(len, queues)) > 8  # windows the rings of 8 could not hold
    assert ckpt_ref.CkptFile.read(tmp_path / "c.gxck").sections[CK_FIFO][2] == ckpt_fifo_ref.encode(queues)
    assert info["coded"]["fifo_jobs"] == sum(map(len, queues))
    b = Engine.from_checkpoint(tmp_path / "c.gxck", lib=gx_lib)
    assert_same(a, b, "restored at round 12")
    for e in (a, b, o):
        e.run_rounds(MORE)
    assert_same(a, b, "round 37")
    assert_same(b, o, "round 37 vs oracle")
    _same_tables(b, o, "round 37 vs oracle")


# ----------------------------------------------------------------------------- chunk seams --
def test_chunk_seams(gx_lib, tmp_path, monkeypatch):
    """warm257 at round 40 through a staging area of two worst-case server-time rows: at least 3
    chunks in every coded section, the same bytes as through the full area, and the same engine from
    a load under the override and under none."""
    e = cc.engine(gx_lib, "warm257")
    e.run_rounds(40)
    whole = tmp_path / "whole.gxck"
    info0 = e.ckpt_save(whole, BOTH)
    assert info0["chunks"] == info0["coded"]["srvt_chunks"] == info0["coded"]["fifo_chunks"] == 1
    stage = 2 * (8 + 8 * 514)
    monkeypatch.setenv("GX_CKPT_STAGE_BYTES", str(stage))
    small = tmp_path / "small.gxck"
    info = e.ckpt_save(small, BOTH)
    assert info["chunks"] >= 3 and info["coded"]["srvt_chunks"] >= 3 and info["coded"]["fifo_chunks"] >= 3
    assert info["coded"]["srvt_chunks"] == (257 + 1) // 2  # two rows a chunk
    assert 16 * info["coded"]["fifo_jobs"] > 2 * stage
    assert small.read_bytes() == whole.read_bytes()
    assert info["sections"] == info0["sections"]
    b = Engine.from_checkpoint(small, lib=gx_lib)
    assert b.ckpt_info["chunks"] >= 3
    monkeypatch.setenv("GX_CKPT_STAGE_BYTES", str(8 + 8 * 514 - 8))  # below one server-time record
    assert _rc(lambda: e.ckpt_save(tmp_path / "x.gxck", BOTH)) == GX_ENOMEM
    assert _rc(lambda: Engine.from_checkpoint(small, lib=gx_lib)) == GX_ENOMEM
    e.ckpt_save(tmp_path / "x.gxck", CKPT_CODE_FIFO)  # (a FIFO record is 16 Q = 512 bytes, a view's 2064)
    assert ckpt_ref.CkptFile.read(tmp_path / "x.gxck").sections[CK_FIFO][2] == ckpt_ref.CkptFile.read(whole).sections[CK_FIFO][2]
    monkeypatch.setenv("GX_CKPT_STAGE_BYTES", "8244")  # no multiple of 8
    assert _rc(lambda: e.ckpt_save(tmp_path / "y.gxck", BOTH)) == GX_EINVAL
    assert not (tmp_path / "y.gxck").exists()
    monkeypatch.delenv("GX_CKPT_STAGE_BYTES")
    c = Engine.from_checkpoint(small, lib=gx_lib)
    assert c.ckpt_info["chunks"] == 1
    for x in (b, c):
        assert_same(e, x, "restored across the seams")
        _same_tables(e, x, "restored across the seams")
    for x in (e, b, c):
        x.run_rounds(10)
    assert_same(e, b, "10 rounds on")
    assert_same(b, c, "10 rounds on")


# -------------------------------------------------------------------------------- refusals --
def _records(words, W, Hl):
    """(offset, n_lit, present word) of each row record of a W <= 4096 section (one present word)."""
    out, at = [], W
    for _ in range(Hl):
        nl = int(words[at])
        if nl == ckpt_ref.MAXU64:
            out.append((at, nl, 0))
            at += 1 + W
        else:
            pres = int(words[at + 1])
            out.append((at, nl, pres))
            at += 2 + 8 * bin(pres).count("1") + nl
    assert at == len(words)
    return out


def test_damaged_coded_files_are_refused(gx_lib, tmp_path):
    """Every one is rejected by validation (no device fault: the process goes on to load the intact
    file and run it)."""
    e = cc.engine(gx_lib, "warm257")
    e.run_rounds(40)  # (most rows differ from base in both blocks, the ragged one included)
    good, bad = tmp_path / "good.gxck", tmp_path / "bad.gxck"
    e.ckpt_save(good, BOTH)
    data = good.read_bytes()
    f = ckpt_ref.CkptFile.read(good)
    Hl, W, Q = 257, 514, 32

    def load_rc():
        return _rc(lambda: Engine.from_checkpoint(bad, lib=gx_lib))

    # a flipped payload byte in each coded section: the checksums
    for sid in (CK_SRVT, CK_FIFO):
        body = f.sections[sid][2]
        for at in (f.offsets[sid] + 5, f.offsets[sid] + len(body) - 3):
            b = bytearray(data)
            b[at] ^= 0x20
            bad.write_bytes(bytes(b))
            assert load_rc() == GX_EIO, (sid, at)

    def rewritten(sid, body):
        g = ckpt_ref.CkptFile.read(good)
        g.sections[sid] = (g.sections[sid][0], g.sections[sid][1], body)
        g.write(bad)  # every checksum recomputed
        return load_rc()

    # the FIFO count table
    fifo = f.sections[CK_FIFO][2]
    n = list(np.frombuffer(fifo[:4 * Hl], dtype="<u4"))
    v = next(i for i, k in enumerate(n) if 0 < k < Q)
    w = next(i for i, k in enumerate(n) if k > 0 and i != v)
    moved = list(n)  # the sum holds: only the host states tell
    moved[v] += 1
    moved[w] -= 1
    assert rewritten(CK_FIFO, ckpt_fifo_ref.with_counts(fifo, Hl, moved)) == GX_EIO
    above = list(n)  # a count above Q, jobs appended so that table and jobs fill the section
    above[v] = Q + 1
    assert rewritten(CK_FIFO, ckpt_fifo_ref.with_counts(fifo, Hl, above) + b"\0" * 16 * (Q + 1 - n[v])) == GX_EIO
    past = list(n)  # the table sums past the section
    past[v] += 1
    assert rewritten(CK_FIFO, ckpt_fifo_ref.with_counts(fifo, Hl, past)) == GX_EIO
    huge = list(n)
    huge[Hl - 1] = 0xFFFFFFFF
    assert rewritten(CK_FIFO, ckpt_fifo_ref.with_counts(fifo, Hl, huge)) == GX_EIO
    assert rewritten(CK_FIFO, fifo[:-16]) == GX_EIO
    assert rewritten(CK_FIFO, fifo[:4 * Hl - 4]) == GX_EIO  # shorter than its table

    # server-time records
    words = np.frombuffer(f.sections[CK_SRVT][2], dtype="<u8").copy()
    recs = _records(words, W, Hl)
    at, nl, pres = next(r for r in recs if r[2] == 3 and 2 <= r[1] <= 490)  # both blocks present; room for a literal
    end = at + 2 + 16 + nl

    def u64(x):
        return np.array([x], dtype=np.uint64)

    more = np.concatenate([words[:at], u64(nl + 1), words[at + 1:end], words[end - 1:end], words[end:]])
    less = np.concatenate([words[:at], u64(nl - 1), words[at + 1:end - 1], words[end:]])
    bit = words.copy()
    assert not (int(bit[at + 2 + 8]) >> 2) & 1
    bit[at + 2 + 8] |= np.uint64(1 << 2)  # block 1, slot 512 + 2 = W: a literal more, so n_lit matches
    bit = np.concatenate([bit[:at], u64(nl + 1), bit[at + 1:end], words[end - 1:end], bit[end:]])
    far = words.copy()
    far[at + 2 + 8 + 7] |= np.uint64(1 << 63)  # slot 1023
    far = np.concatenate([far[:at], u64(nl + 1), far[at + 1:end], words[end - 1:end], far[end:]])
    stray = words.copy()
    stray[at + 1] |= np.uint64(1 << 2)  # a present bit past the last block
    for what, w2 in (("more", more), ("less", less), ("bit", bit), ("far", far), ("stray", stray)):
        assert rewritten(CK_SRVT, w2.astype("<u8").tobytes()) == GX_EIO, what
    assert rewritten(CK_SRVT, words[:-1].astype("<u8").tobytes()) == GX_EIO
    assert rewritten(CK_SRVT, words[:W - 1].astype("<u8").tobytes()) == GX_EIO  # shorter than base

    # the host states' section removed: the FIFO counts have nothing to be checked against
    g = ckpt_ref.CkptFile.read(good)
    del g.sections[CK_HS]
    g.write(bad)
    assert load_rc() == GX_EIO
    # a coding the table does not admit for the section
    g = ckpt_ref.CkptFile.read(good)
    g.sections[CK_VIEW] = (CKPT_FIFO,) + g.sections[CK_VIEW][1:]
    g.write(bad)
    assert load_rc() == GX_EINVAL

    # the intact file still loads and continues as the saved engine
    b = Engine.from_checkpoint(good, lib=gx_lib)
    for x in (e, b):
        x.run_rounds(9)
    assert_same(e, b, "after the refusals")
    _same_tables(e, b, "after the refusals")


def test_refused_saves(gx_lib, oracle_lib, tmp_path):
    g, o = cc.engine(gx_lib, "q16"), cc.engine(oracle_lib, "q16")
    g.run_rounds(2)
    o.run_rounds(3)
    path = tmp_path / "x.gxck"
    for code in (4, 4 | BOTH, 16, 1 << 31):
        assert _rc(lambda: g.ckpt_save(path, code)) == GX_EINVAL, code
        assert not path.exists()
    g.round_send()
    assert _rc(lambda: g.ckpt_save(path, BOTH)) == GX_EINVAL
    assert not path.exists()
    g.round_merge()
    assert _rc(lambda: g.ckpt_save(path, BOTH)) == GX_EINVAL
    assert not path.exists()
    g.round_end()
    assert_same(g, o, "the round completed after the refused saves")
    g.ckpt_save(path, BOTH)
    b = Engine.from_checkpoint(path, lib=gx_lib)
    for e in (g, b, o):
        e.run_rounds(7)
    assert_same(b, o, "restored after the completed round")


# ------------------------------------------------------------------- fork and read-only --
def test_fork_from_a_coded_file(gx_lib, oracle_lib, tmp_path):
    """The storm fork of tests/test_gpu_ckpt.py, from a coded file saved at round 20."""
    e = _eng(gx_lib, **FORK_BASE)
    e.run_rounds(20)
    info = e.ckpt_save(tmp_path / "r20.gxck", BOTH)
    assert _codings(info) == {CK_VIEW: CKPT_VIEWS, CK_FIFO: CKPT_FIFO, CK_SRVT: CKPT_VIEWS}
    o = _eng(oracle_lib, **dict(FORK_BASE, **FORKS["storm"]))
    g = Engine.from_checkpoint(tmp_path / "r20.gxck", lib=gx_lib, **FORKS["storm"])
    o.run_rounds(20)
    assert_same(g, o, "fork at the saved round")
    for stop in (31, 46, 80):
        for x in (g, o):
            x.run_rounds(stop - x.round)
        assert_same(g, o, f"fork round {stop}")
    assert o.stats()["expire_server"] > 0


def test_coded_save_is_read_only(gx_lib, tmp_path):
    """As tests/test_gpu_ckpt.py test_save_is_read_only, the saves coded: equal throughout, the same
    number of quiet rounds."""
    t = quiet_cases.oracle_trace("h128")
    a, b = _eng(gx_lib, **t["params"]), _eng(gx_lib, **t["params"])
    for r in range(1, 151):
        a.run_rounds(1)
        b.run_rounds(1)
        if r % 10 == 0:
            a.ckpt_save(tmp_path / "s.gxck", BOTH)
            assert_same(a, b, f"round {r}")
    assert_snap(a, t["snaps"][150], "the saving engine, round 150")
    na, nb = merge_launches(a), merge_launches(b)
    assert na == nb < 150
