"""The call contract of the sharded push-pull chain (gx_ae_bytes .. gx_ae_merge, gx_ae_claim_*,
gx_ae_skip_locked) for tests/test_gpu_ae_chain_order.py: two LocalShards engines driven by hand
through the second push-pull round of a run, so the first one's plan, sizes and guards are stale.
`chain` is ShardRounds._ae_chain unrolled, stopping before each of its calls; a scenario makes its
wrong calls on shard 0 there, each refused with GX_EINVAL before any kernel is launched or any
buffer is read past the size the caller gave, and the chain carries on with the right call. A
scenario ends the round, runs a few more and compares with the unsharded engine: a refused call
leaves nothing behind. Every function takes the library, so the same table runs on any build."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from sidecar_amd.abi import INIT_OWN, PP_INITIATE, Engine, GxError, default_params
from sidecar_amd.dist import LocalShards, _ptr, planned_exchange
from tests.test_shards_cpu import assert_sharded_equal

# churn keeps the rows of the two shards apart, so the cross pairs ship blocks
KW = dict(n_hosts=32, n_services=4, init_mode=INIT_OWN, churn_ppm=100000, ae_period_rounds=4, queue_cap=4096)
AE_ROUND = 4     # the run's second push-pull round (ae_phase 0)
MORE_ROUNDS = 5  # run after the scenario's round: one more push-pull round among them


def refused(call, *a):
    with pytest.raises(GxError, match=r"rc=-22$"):
        call(*a)


def _gossip(sh) -> bool:
    """The gossip half of one round, as ShardRounds.run_rounds takes it; True in a push-pull round
    (otherwise the round has ended)."""
    if planned_exchange(sh.engines[0].params):
        return sh._gossip_planned()
    ae = sh._gossip_sized()
    if not ae:
        for e in sh.engines:
            e.round_end()
    return ae


def start(lib, rounds=AE_ROUND, **kw):
    """The shards after `rounds` rounds, and a scratch device buffer that every wrong call may be
    handed: larger than any message of these runs."""
    kw = dict(KW, **kw)
    sh = LocalShards(lib, 2, device="cuda:0", **kw)
    sh.run_rounds(rounds)
    return sh, kw, torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")


def finish(lib, sh, kw, what):
    for e in sh.engines:
        e.round_end()
    sh.run_rounds(MORE_ROUNDS)
    whole = Engine(default_params(lib, **kw), lib=lib)
    whole.run_rounds(sh.engines[0].round)
    assert_sharded_equal(whole, sh, what)


def chain(sh, claim_set_last=False):
    """One run of the chain, call by call. Yields (the name of the call that comes next, c) with
    what the calls so far returned in c: sizes, dig, delta, won, lead, rsz, ret (per shard).
    claim_set_last: shard 0 admits its claimants only just before its gx_ae_merge (the others at
    the usual place; nothing between reads what gx_ae_claim_set writes)."""
    es = sh.engines
    c = SimpleNamespace()
    yield "ae_bytes", c
    c.sizes = [e.ae_bytes() for e in es]
    yield "ae_pack", c
    _, c.dig = sh._exchange_sized(c.sizes, lambda i, p, n: es[i].ae_pack(p, n))
    yield "ae_merge_local", c
    for e in es:
        e.ae_merge_local()
    yield "ae_delta_bytes", c
    c.delta = [e.ae_delta_bytes(_ptr(x), x.numel()) for e, x in zip(es, c.dig)]
    if sh._arbitrate:
        yield "ae_claim_want", c
        want = torch.empty((len(es), es[0].params.lock_defer_slots or 64), dtype=torch.int64, device=sh.device)
        for e, w in zip(es, want):
            e.ae_claim_want(_ptr(w))
        c.won = sh._reduce(want, "min").contiguous()
        for e in es[1 if claim_set_last else 0:]:
            e.ae_claim_set(_ptr(c.won))
    yield "ae_delta_pack", c
    _, c.lead = sh._exchange_sized(c.delta, lambda i, p, n: es[i].ae_delta_pack(p, n))
    yield "ae_return_bytes", c
    c.rsz = [e.ae_return_bytes(_ptr(x), x.numel()) for e, x in zip(es, c.lead)]
    yield "ae_return_pack", c
    _, c.ret = sh._exchange_sized(
        c.rsz, lambda i, p, n: es[i].ae_return_pack(_ptr(c.lead[i]), c.lead[i].numel(), p, n))
    yield "ae_merge", c
    if sh._arbitrate and claim_set_last:
        es[0].ae_claim_set(_ptr(c.won))
    for e, x, y in zip(es, c.lead, c.ret):
        e.ae_merge(_ptr(x), x.numel(), _ptr(y), y.numel())


def assert_ships_blocks(sh, c):
    """Shard 0 has a cross pair, and a lead message that is more than its 16-byte header."""
    pairs = int(c.sizes[0][1]) // sh.wire.dig_msg
    assert c.sizes[0][1] > 0 and pairs > 0
    assert int(c.delta[0][1]) > 16 * pairs


def before_the_plan(lib):
    """Calls that need this round's gx_ae_bytes, made before it; the calls of the arbitration without
    lock_readers; the all-locked shortcut with free hosts; then gx_ae_bytes twice."""
    sh, kw, big = start(lib)
    e0 = sh.engines[0]
    assert _gossip(sh)
    for call, c in chain(sh):
        if call == "ae_bytes":
            refused(e0.ae_pack, _ptr(big), big.numel())
            refused(e0.ae_delta_bytes, _ptr(big), sh.wire.dig_msg)
            refused(e0.ae_delta_bytes, 0, 0)
            refused(e0.ae_merge_local)
            refused(e0.ae_merge)
            refused(e0.ae_claim_want, _ptr(big))
            refused(e0.ae_claim_set, _ptr(big))
            refused(e0.ae_ro_counts)
            assert e0.lock_census() > 0
            refused(e0.ae_skip_locked)
        elif call == "ae_pack":
            assert np.array_equal(e0.ae_bytes(), c.sizes[0])
            assert np.array_equal(e0.ae_bytes(), c.sizes[0])
        elif call == "ae_delta_pack":
            assert_ships_blocks(sh, c)
    finish(lib, sh, kw, "before the plan")


def wrong_sizes_and_order(lib):
    """Each later call before the one it needs, and with a size that is off by one unit."""
    sh, kw, big = start(lib)
    e0 = sh.engines[0]
    assert _gossip(sh)
    for call, c in chain(sh):
        if call == "ae_delta_bytes":
            dig = c.dig[0]
            refused(e0.ae_delta_pack, _ptr(big), big.numel())
            refused(e0.ae_return_bytes, _ptr(big), 0)
            refused(e0.ae_delta_bytes, _ptr(dig), dig.numel() - sh.wire.dig_msg)
            e0.ae_merge_local()  # a second time: nothing happens
            # planned again (once the local pairs, which read the plan, are through): they stay run
            torch.cuda.synchronize()
            assert np.array_equal(e0.ae_bytes(), c.sizes[0])
        elif call == "ae_delta_pack":
            assert_ships_blocks(sh, c)
            refused(e0.ae_delta_pack, _ptr(big), int(c.delta[0].sum()) - 1)
            refused(e0.ae_return_pack, _ptr(big), 0, _ptr(big), big.numel())
        elif call == "ae_return_bytes":
            lead = c.lead[0]
            assert lead.numel() > 0
            refused(e0.ae_return_pack, _ptr(lead), lead.numel(), _ptr(big), big.numel())
            refused(e0.ae_merge, _ptr(lead), lead.numel(), _ptr(big), 0)
            refused(e0.ae_return_bytes, _ptr(lead), lead.numel() + 8)
        elif call == "ae_merge":
            lead, ret = c.lead[0], c.ret[0]
            assert ret.numel() > 8
            refused(e0.ae_merge, _ptr(lead), lead.numel(), _ptr(ret), ret.numel() - 8)
    finish(lib, sh, kw, "wrong sizes and order")


def round_without_push_pull(lib):
    """Every call of the chain is empty in a round without push-pull, and refuses bytes."""
    sh, kw, big = start(lib, rounds=AE_ROUND + 1)
    e0 = sh.engines[0]
    assert not e0.is_ae_round()
    assert not e0.ae_bytes().any()
    e0.ae_pack(0, 0)
    assert not e0.ae_delta_bytes(0, 0).any()
    assert not e0.ae_return_bytes(0, 0).any()
    e0.ae_merge_local()
    e0.ae_merge()
    refused(e0.ae_delta_bytes, _ptr(big), 16)
    refused(e0.ae_return_bytes, _ptr(big), 16)
    assert not _gossip(sh)  # the round ends on its own
    sh.run_rounds(MORE_ROUNDS)
    whole = Engine(default_params(lib, **kw), lib=lib)
    whole.run_rounds(e0.round)
    assert_sharded_equal(whole, sh, "round without push-pull")


def claims(lib):
    """lock_readers = 1: the arbitration's place in the chain."""
    sh, kw, big = start(lib, lock_readers=1, lock_defer_slots=8)
    e0 = sh.engines[0]
    assert sh._arbitrate and _gossip(sh)
    for call, c in chain(sh, claim_set_last=True):
        if call == "ae_delta_bytes":
            assert c.sizes[0][1] > 0
            refused(e0.ae_claim_want, _ptr(big))  # the cross pairs' verdicts come with the digests
        elif call == "ae_claim_want":
            refused(e0.ae_claim_set, _ptr(big))  # the local pairs have not rejoined the stream
        elif call == "ae_delta_pack":
            assert_ships_blocks(sh, c)
        elif call == "ae_merge":
            lead, ret = c.lead[0], c.ret[0]
            refused(e0.ae_merge, _ptr(lead), lead.numel(), _ptr(ret), ret.numel())  # before gx_ae_claim_set
    finish(lib, sh, kw, "claims")


def past_the_last_batch(lib):
    """GX_PP_INITIATE: the chain runs once per batch; after the last one its calls are empty."""
    sh, kw, big = start(lib, push_pull_mode=PP_INITIATE)
    e0 = sh.engines[0]
    assert _gossip(sh)
    nb = e0.ae_batches()
    assert nb > 0
    cross = 0
    for _ in range(nb):
        for call, c in chain(sh):
            if call == "ae_pack":
                cross += int(c.sizes[0][1])
    assert cross > 0
    assert not e0.ae_bytes().any()
    e0.ae_merge()
    refused(e0.ae_merge, _ptr(big), 16)
    finish(lib, sh, kw, "past the last batch")


CASES = [before_the_plan, wrong_sizes_and_order, round_without_push_pull, claims, past_the_last_batch]
