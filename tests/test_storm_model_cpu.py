"""The storm contract on the oracle alone (tests/storm_cases.py): storm_model equals the oracle's
storm round on every case, and each case's inputs reach what the case claims (the vacuity guards), so
the GPU tests that import the same cases cannot quietly stop testing it."""
import numpy as np
import pytest

from tests import storm_cases as sc
from tests.oracle_lib import load_oracle


def storm_round_on(lib, name, ev):
    """An engine stepped through the case's storm round_send() on the case's views."""
    case = sc.CASES[name]
    words = sc.case_views(name)
    e = sc.make_engine(lib, name)
    e.run_rounds(case["storm_round"])
    e.write_views(words)
    if ev:
        sc.add_listeners(e)
    before = sc.before_state(e)
    e.round_send()
    return e, words, before, (sc.drain_all(e) if ev else None)


def live_matrix(fig, H, v0, v1):
    """[viewer of [v0, v1), owner of its other half] -> live, for the viewers whose storm ran."""
    lo, hi = sc.other_half(H, v0)
    m = np.zeros((v1 - v0, hi - lo), dtype=bool)
    for v in range(v0, v1):
        if fig["runs"][v]:
            m[v - v0, fig["live"][v] - lo] = True
    return m


@pytest.mark.parametrize("run", sc.RUNS, ids=sc.run_id)
def test_storm_model_and_guards(run):
    name, ev = run
    case = sc.CASES[name]
    H, S = case["H"], case["S"]
    e, words, before, events = storm_round_on(load_oracle(omp=True), name, ev)
    fig = sc.check_against_model(e, name, words, before, None, events)
    runs, jobs = fig["runs"], fig["jobs"]
    half = H // 2
    # (a) the stretch is longer than the seam the case names
    assert min(case["nw"]) > case["min_nw"]
    # (b) a dead owner directly before a live one at every seam position, on a viewer whose storm ran
    share = []
    for v0, v1 in ((0, half), (half, H)):
        lo, hi = sc.other_half(H, v0)
        live = live_matrix(fig, H, v0, v1)
        share.append(live[runs[v0:v1]].mean())
        for seam, pos in sc.seam_positions(S, (hi - lo) * S).items():
            assert len(pos), (name, seam)
            gap = live[:, pos // S] & ~live[:, pos // S - 1]
            assert gap.any(axis=0).all(), f"{name}: no gap in the job ranks at seam {seam}, words {pos[~gap.any(axis=0)]}"
    Q = e.params.queue_cap
    t0q = fig["tail0"] % Q
    wrapped = runs & (t0q != 0) & (t0q + jobs > Q) & (jobs > fig["room"]) & (fig["room"] > 0)
    if name == "s16_wrap":  # (c)
        assert wrapped.any() and (runs & (jobs > 0) & (jobs < fig["room"])).any()
        assert e.stats()["queue_deferred"] > before["stats"]["queue_deferred"]
    if ev:  # (d) a listener overflows; one receives events from more than two tiles
        caps = dict(sc.listener_views(H))
        assert any(len(x) == caps[v] for v, x in events.items())
        tile = 2048 if sc.is_p2(S) else 1024 // S * S
        assert any(len({((t[0] - sc.other_half(H, v)[0]) * S + t[1]) // tile for t in x}) > 2 for v, x in events.items())
        assert all(runs[v] for v in caps)
    if e.params.lock_model:  # (e)
        lk = before["locked"]
        assert lk[:half].any() and lk[half:].any() and runs[:half].any() and runs[half:].any()
    if e.params.depart_ppm:
        assert before["departed"][:half].any() and before["departed"][half:].any()
    print(f"STORM-CASE {sc.run_id(run)}: nw={case['nw']} seams={list(sc.seam_positions(S, case['nw'][0]))} "
          f"live share={np.mean(share):.3f} wrapped={int(wrapped.sum())} deferred-cut={int((runs & (jobs > fig['room'])).sum())} "
          f"locked={int(before['locked'].sum())} departed={int(before['departed'].sum())} viewers={H} "
          f"jobs={int(jobs.sum())} calls={fig['calls']}")


def test_storm_model_palette_counts():
    """The model on hand-written cells: one viewer, S = 4, every palette kind once."""
    S, H = 4, 20  # viewer 0 expires owners 10..19
    now, epoch = 5_000_000_000, 1_000_000_000
    tomb = ((now - epoch) << 3) | 1

    def w(ts, st):
        return (ts << 3) | st
    A = 7
    cells = [[A, A, A, A],                                  # absent
             [w(5, 1), w(6, 1), w(7, 1), w(8, 1)],          # all tombstones: not live
             [w(5, 0), w(6, 0), w(7, 0), w(8, 0)],          # all alive
             [A, w(6, 0), A, w(8, 1)],                      # sparse
             [w(5, 0), A, A, A],                            # slot 0 only
             [A, A, A, w(8, 0)],                            # slot S - 1 only
             [w(9, 0), w(2, 1), w(9, 2), w(3, 1)],          # live + older tombstones
             [A, A, w(7, 4), w(1, 1)],                      # DRAINING the only live record
             [w(5, 0), tomb, A, A],                         # beside a record that is the tombstone already
             [A, w(6, 1), A, A]]                            # a lone tombstone
    views = np.full((H, H * S), 7, dtype=np.uint64)
    views[0, 10 * S:] = np.array(cells, dtype=np.uint64).reshape(-1)
    m = sc.storm_model(views, H, S, 0, now, epoch)
    assert m["jobs"].tolist() == [[15, 12], [10, 13], [1, 14], [8, 15], [15, 16], [12, 17], [3, 18]]
    assert m["live"].tolist() == [12, 13, 14, 15, 16, 17, 18]
    assert m["calls"] == 4 + 2 + 1 + 1 + 4 + 2 + 2 and m["written"] == m["calls"] - 1
    after = m["cols"].reshape(10, S)
    assert (after[[0, 1, 9]] == np.array(cells, dtype=np.uint64)[[0, 1, 9]]).all()
    assert after[3].tolist() == [7, tomb, 7, tomb] and after[8].tolist() == [tomb, tomb, 7, 7]
    assert m["events"][:5].tolist() == [[12, 0, now, 1, 0], [12, 1, now, 1, 0], [12, 2, now, 1, 0], [12, 3, now, 1, 0],
                                        [13, 1, now, 1, 0]]
    assert m["events"][-4:].tolist() == [[17, 2, now, 1, 4], [17, 3, now, 1, 1], [18, 0, now, 1, 0], [18, 1, now, 1, 1]]
    assert len(m["events"]) == m["calls"]
