"""The coded-checkpoint schedules (tests/ckpt_coded_cases.py) are not vacuous: by the oracle, the states
they save hold every shape of FIFO window and every kind of server-time row; the numpy references
(tests/ckpt_ref.py for the ROW CODING, tests/ckpt_fifo_ref.py for the FIFO SECTION) round-trip the
oracle's own state; and the FIFO reference refuses what include/gx_ckpt.h says a load refuses."""
import numpy as np
import pytest

from tests import ckpt_coded_cases as cc
from tests import ckpt_fifo_ref, ckpt_ref


@pytest.fixture(scope="module")
def states(oracle_lib):
    """(case, round) -> (server-time table, host states, queues, FIFO shapes) by the oracle."""
    rounds = {"q8": (0, 6, 12), "q16": (6,), "warm257": (0, 6, 20, 40), "warm256": (0, 12), "h4": (6,)}
    out = {}
    for name, rs in rounds.items():
        e = cc.engine(oracle_lib, name)
        for r in rs:
            e.run_rounds(r - e.round)
            out[name, r] = (cc.srvt_table(e), e.hosts(), cc.queues(e), cc.fifo_shapes(e))
        e.close()
    return out


def test_every_saved_state_is_probed(states):
    assert set(cc.SAVES) <= set(states)


def test_fifo_shapes(states):
    for key in (("q8", 12), ("q16", 6)):  # every shape at once
        shapes = states[key][3]
        assert all(shapes[k] > 0 for k in cc.FIFO_SHAPES), (key, shapes)
    assert cc.CASES["q8"]["queue_cap"] < 12  # below k_send's head prefetch
    late = states["warm257", 40][3]
    assert late["wrapped"] > 0 and late["deferred"] > 0, late
    for key in (("warm257", 0), ("warm256", 0)):
        assert states[key][3]["empty"] == len(states[key][1])


def test_server_time_rows(states):
    rows = {k: cc.srvt_rows(v[0]) for k, v in states.items()}
    raw, coded, equal, _ = rows["q8", 0]
    assert (raw, coded, equal) == (33, 0, 0)  # a cold start: all raw
    for key in (("q8", 6), ("q16", 6)):
        raw, coded, equal, lits = rows[key]
        assert raw > 0 and coded > 0 and lits > 0, (key, rows[key])
    for key, n in ((("warm257", 0), 257), (("warm256", 0), 256)):
        assert rows[key][:3] == (0, 0, n)  # every row equals base
    for key, n in ((("warm257", 6), 257), (("warm257", 20), 257), (("warm257", 40), 257), (("warm256", 12), 256)):
        raw, coded, equal, lits = rows[key]
        assert (raw, coded, equal) == (0, n, 0) and lits > 0, (key, rows[key])  # all coded
    assert rows["warm257", 6][3] < rows["warm257", 20][3] < rows["warm257", 40][3]
    raw, coded, equal, _ = rows["h4", 6]  # W = 8: a row is raw, or equals base
    assert raw > 0 and coded + equal > 0
    assert {states[k, r][0].shape[1] for k, r in (("warm257", 0), ("warm256", 0), ("h4", 6))} == {514, 512, 8}


def test_row_reference_round_trips_the_server_times(states):
    for key, (table, _, _, _) in states.items():
        body = ckpt_ref.encode_views(table)
        Hl, W = table.shape
        assert len(body) == ckpt_ref.view_section_bytes(table), key
        assert np.array_equal(ckpt_ref.decode_views(body, Hl, W), table), key
    for key, H in ((("warm257", 0), 257), (("warm256", 0), 256)):  # the warm formula of gx_ckpt.h
        nblk = (2 * H + 511) // 512
        assert len(ckpt_ref.encode_views(states[key][0])) == 16 * H + H * 8 * (1 + (nblk + 63) // 64)


def test_fifo_reference_round_trips_the_queues(states):
    for (name, r), (_, hosts, queues, _) in states.items():
        Q = cc.CASES[name]["queue_cap"]
        body = ckpt_fifo_ref.encode(queues)
        win = ckpt_fifo_ref.windows_of(hosts)
        assert [len(q) for q in queues] == win, (name, r)  # gx_read_queue returns the stored window
        assert len(body) == ckpt_fifo_ref.stored_bytes(win)
        assert ckpt_fifo_ref.decode(body, len(hosts), Q, win) == queues, (name, r)
    assert len(ckpt_fifo_ref.encode(states["warm257", 0][2])) == ckpt_fifo_ref.pad8(4 * 257)  # an empty section


def test_fifo_reference_refusals(states):
    _, hosts, queues, _ = states["q8", 12]
    Hl, Q = len(hosts), 8
    body = ckpt_fifo_ref.encode(queues)
    n = [len(q) for q in queues]
    v = next(i for i, k in enumerate(n) if 0 < k < Q)

    def refused(data, windows=None):
        with pytest.raises(AssertionError):
            ckpt_fifo_ref.decode(data, Hl, Q, windows)

    more = list(n)
    more[v] += 1  # the counts overrun the section
    refused(ckpt_fifo_ref.with_counts(body, Hl, more))
    above = list(n)
    above[v] = Q + 1  # a count above Q, the section's length made to agree
    refused(ckpt_fifo_ref.with_counts(body, Hl, above) + b"\0" * 16 * (Q + 1 - n[v]))
    refused(body[:-16])
    refused(body[:4 * Hl - 1])
    moved = list(n)  # the sum holds, two counts disagree with the host states
    w = next(i for i, k in enumerate(n) if k > 0 and i != v)
    moved[v] += 1
    moved[w] -= 1
    ckpt_fifo_ref.decode(ckpt_fifo_ref.with_counts(body, Hl, moved), Hl, Q)
    refused(ckpt_fifo_ref.with_counts(body, Hl, moved), ckpt_fifo_ref.windows_of(hosts))
