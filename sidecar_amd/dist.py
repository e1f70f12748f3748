"""Host sharding across engines: one round = send phase, packet exchange, merge phase,
push-pull digest exchange, push-pull delta exchange, end.

Each engine owns the contiguous host block [g*H/G, (g+1)*H/G). The exchange moves the wire
formats of include/gx.h between shards. One driver, ``ShardRounds``, steps the shards this
process holds through the round's C-ABI calls, phase by phase; what carries the bytes between
shards is a transport of three operations (size matrix, move, reduce), and there are two:
  * ``DistShard`` — one shard per process and GPU, ``torch.distributed`` collectives (RCCL over
    xGMI for the HIP engine with backend "nccl"; gloo for the CPU oracle in tests);
  * ``LocalShards`` — every shard in this process (one GPU or the CPU); the exchange is a
    device-side concatenation. Checks the sharded kernels, and the driver, against the unsharded
    engine.
Exchange buffers are torch uint8 tensors on the engine's device: the HIP engine reads and
writes them as device memory.
"""
from __future__ import annotations

import os
from itertools import accumulate
from typing import List

import numpy as np
import torch

from .abi import PP_INITIATE, Engine, GxParams, default_params

# stats that hold the earliest round something happened (-1: never): the minimum over shards
FIRST_ROUND_STATS = ("first_drop_round", "first_locked_round")
_NEVER = 1 << 62  # -1 in a MIN reduction


def planned_exchange(p: GxParams) -> bool:
    """A gossip round exchanges fixed, seeded slot counts (gx_exchange_plan: no size collective, no
    host wait) iff the failure detector is off and GossipMessages is at most one message per target
    (0 and 1 both mean one). Past one message the plan reserves GossipMessages slots per sampled peer
    and ships mostly padding (GM 15: ~85 MB per rank per round at cfg 5, G = 8), so the exact sizes
    are gathered instead."""
    return not p.fd_enable and p.gossip_messages <= 1


def lock_shortcut(p: GxParams) -> bool:
    """A push-pull round may be replaced by gx_ae_skip_locked when every host holds the lock: the
    lock model on, no failure detector (its membership half runs regardless), no departures, no
    lock_readers (an exchange between read-locked hosts runs, gx.h)."""
    return bool(p.lock_model) and not p.fd_enable and not (p.depart_round >= 0 and p.depart_ppm) and \
        not p.lock_readers


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr() if t.numel() else 0


def _fold(t: torch.Tensor, op: str) -> torch.Tensor:
    """An int64 tensor of one row per shard reduced over the shards; op: "sum", "min", "max"."""
    return {"sum": t.sum, "min": t.amin, "max": t.amax}[op](0)


class WireBytes:
    """Bytes each exchange moved between shards (this process's shards, sent side)."""

    def __init__(self, e: Engine):
        p = e.params
        self.R = e.H * e.S
        # one digest message per cross-shard pair (gx.h "digest")
        self.dig_msg = 16 + 16 * ((self.R + 511) // 512) + (8 * e.H if p.fd_enable and p.fd_push_pull_state else 0)
        self.packets = self.ae_digest = self.ae_delta = self.ae_lead = self.ae_return = self.ae_full_rows = 0

    def add_ae(self, digest_sizes, lead_sizes, return_sizes):
        dig = int(np.asarray(digest_sizes).sum())
        n_msgs = dig // self.dig_msg
        self.ae_digest += dig
        lead, ret = int(np.asarray(lead_sizes).sum()), int(np.asarray(return_sizes).sum())
        self.ae_lead += lead
        self.ae_return += ret
        self.ae_delta += lead + ret
        self.ae_full_rows += n_msgs * (16 + 8 * self.R)  # the same pairs' full rows

    def as_dict(self):
        return {"packets": self.packets, "ae_digest": self.ae_digest, "ae_delta": self.ae_delta,
                "ae_lead": self.ae_lead, "ae_return": self.ae_return, "ae_full_rows_equivalent": self.ae_full_rows}


class _Shard:
    def __init__(self, params: GxParams, lib, device: torch.device, engine: Engine = None):
        self.e = engine if engine is not None else Engine(params, lib=lib)  # a ready engine: ShardRounds.load
        self.device = device
        if device.type == "cuda":
            # the engine queues its work on torch's stream, so packing, the collectives and
            # unpacking are ordered by the stream; only calls that return sizes wait
            self.e.set_stream(torch.cuda.current_stream(device).cuda_stream, True)

    def pack(self, sizes, packer) -> torch.Tensor:
        buf = torch.empty(int(sum(sizes)), dtype=torch.uint8, device=self.device)
        packer(_ptr(buf), buf.numel())
        return buf


class ShardRounds:
    """The round driver: shards `ids` (ascending) of a G-shard cluster, held by this process, stepped
    through a round's C-ABI calls phase by phase. Every shard packs before anything moves, so shards
    in one process can feed each other. A subclass adds the transport:
      _matrix(rows)  each held shard's per-destination sizes (host array, or a device tensor the
                     engine filled) -> the G x G size matrix m[src][dst] on the host (lists of int)
      _move(bufs, m, planned=False)  each held shard's send buffer (its m[src] segments, destinations
                     ascending) -> each held shard's inbox (sources ascending)
      _reduce(t, op) an int64 tensor of one row per held shard -> its _fold over all G shards
    Engine methods are looked up at each call (tests and profiling tools patch them)."""

    def __init__(self, lib, G: int, ids, device, kw, engines=None):
        """engines: the held shards' engines, ready made (restored from checkpoints, `_load_engines`),
        in the order of `ids`; else each is created from `kw`."""
        self.device = torch.device(device)
        self.G = G
        self.shards: List[_Shard] = []
        for i, g in enumerate(ids):
            if engines is not None:
                e = engines[i]
                assert max(1, e.params.n_shards) == G and (e.params.shard_id if G > 1 else 0) == g
                self.shards.append(_Shard(e.params, lib, self.device, engine=e))
                continue
            p = default_params(lib, **kw)
            p.n_shards = G
            p.shard_id = g
            if self.device.type == "cuda":
                p.device = self.device.index or 0
            self.shards.append(_Shard(p, lib, self.device))
        self._own = slice(ids[0], ids[-1] + 1)  # the held shards' rows of a size matrix
        self.wire = WireBytes(self.shards[0].e)
        self.exchange_paths = {"planned": 0, "sized": 0}  # gossip rounds per exchange path (planned_exchange)
        self.trace_ae = False  # keep each push-pull round's digest and delta inboxes (host copies)
        self.ae_trace = []
        self.ae_skipped = 0  # push-pull rounds with every host locked (gx_ae_skip_locked)
        self.skip_locked = True  # False: run the whole exchange even then (wire tests)
        self.ae_batches_run = 0  # GX_PP_INITIATE: runs of the push-pull chain, one per batch
        # lock_readers: the pool of waiting merges is cluster-wide, so every run of the chain
        # arbitrates its slots over all shards (_claim_slots)
        self._arbitrate = G > 1 and bool(self.shards[0].e.params.lock_readers)
        self._pb = None

    @property
    def engines(self) -> List[Engine]:
        return [s.e for s in self.shards]

    # checkpoints (include/gx_ckpt.h): one file per held shard, no collective. The driver's own state
    # (the planned exchange's buffers and matrix, diagnostics) is derived and starts fresh on a load.
    @staticmethod
    def shard_file(dirname, g: int, G: int) -> str:
        return os.path.join(os.fspath(dirname), f"shard_{g:03d}_of_{G:03d}.gxck")

    def save(self, dirname, code=0) -> List[dict]:
        """Every held shard's checkpoint into `dirname` (between rounds: run_rounds has returned);
        each file's gx_ckpt_info. code: Engine.ckpt_save's mask of coded sections."""
        os.makedirs(dirname, exist_ok=True)
        return [e.ckpt_save(self.shard_file(dirname, e.params.shard_id if self.G > 1 else 0, self.G), code)
                for e in self.engines]

    @classmethod
    def _load_engines(cls, lib, dirname, G: int, ids, device, override) -> List[Engine]:
        device = torch.device(device)
        if device.type == "cuda":
            override = dict(override, device=device.index or 0)
        return [Engine.from_checkpoint(cls.shard_file(dirname, g, G), lib=lib, **override) for g in ids]

    def _exchange_sized(self, rows, pack, after_pack=None):
        """One exchange whose sizes the shards report (`rows`); pack(i, ptr, cap) fills held shard
        i's send buffer. Returns the held shards' rows of the size matrix and their inboxes."""
        m = self._matrix(rows)
        own = m[self._own]
        bufs = [s.pack(sz, lambda p, n, i=i: pack(i, p, n)) for i, (s, sz) in enumerate(zip(self.shards, own))]
        if after_pack is not None:
            for e in self.engines:
                after_pack(e)
        return own, self._move(bufs, m)

    def _planned_bufs(self) -> List[torch.Tensor]:
        """Each held shard's send buffer of the planned exchange, allocated once at its bound (k_send
        writes the slots straight into it, before the round's counts reach the host: a shard sends at
        most fanout * GossipMessages packet slots per host, and with probe_piggyback the host's ping
        and ack, gx.h gx_exchange_plan); the plan matrix comes with them."""
        if self._pb is None:
            p = self.shards[0].e.params
            slot = 16 + 16 * p.packet_cap
            per_host = p.fanout * max(1, p.gossip_messages) + (2 if p.probe_piggyback else 0)
            self._pb = [torch.empty((e.hi - e.lo) * per_host * slot, dtype=torch.uint8, device=self.device)
                        for e in self.engines]
            self._plan = np.zeros((self.G, self.G), dtype=np.uint64)  # m[src][dst], as gx_exchange_plan fills it
        return self._pb

    def _gossip_planned(self) -> bool:
        """One planned gossip round in two engine calls around the move: no size matrix to gather, no
        host wait. True when it is a push-pull round; otherwise gx_round_gossip_end ended the round."""
        bufs = self._planned_bufs()
        for s, b in zip(self.shards, bufs):
            s.e.round_gossip_begin(self._plan, _ptr(b), b.numel())  # each writes the whole, seeded matrix
        m = self._plan.tolist()
        self.wire.packets += sum(map(sum, m[self._own]))
        ae = [s.e.round_gossip_end(_ptr(x), x.numel()) for s, x in zip(self.shards, self._move(bufs, m, planned=True))]
        assert all(a == ae[0] for a in ae)
        return ae[0]

    def _gossip_sized(self) -> bool:
        """One gossip round with gathered sizes: the engines write their outbox sizes into device
        tensors (no host wait), the size matrix is the exchange's one wait. True in a push-pull round."""
        for s in self.shards:
            s.e.round_send()
        rows = [torch.zeros(self.G, dtype=torch.int64, device=self.device) for _ in self.shards]
        for s, t in zip(self.shards, rows):
            s.e.outbox_sizes_async(_ptr(t))
        m, inb = self._exchange_sized(rows, lambda i, p, c: self.shards[i].e.outbox_pack(p, c))
        self.wire.packets += sum(map(sum, m))
        for s, x in zip(self.shards, inb):
            s.e.inbox_unpack(_ptr(x), x.numel())
        for s in self.shards:
            s.e.round_merge()
        return self.shards[0].e.is_ae_round()  # every shard agrees: the schedule is global

    def _claim_slots(self):
        """lock_readers: each held shard's holders and lowest claimants per pool slot, their minimum
        over all shards, and each shard admits its claimants named in it (gx.h lock_readers). One
        reduction in every run of the chain, whatever the device data say."""
        es = self.engines
        want = torch.empty((len(es), self.shards[0].e.params.lock_defer_slots or 64), dtype=torch.int64,
                           device=self.device)
        for e, w in zip(es, want):
            e.ae_claim_want(_ptr(w))
        won = self._reduce(want, "min").contiguous()
        for e in es:
            e.ae_claim_set(_ptr(won))  # (queued on the stream that frees `won`)

    def ro_counts(self) -> dict:
        """lock_readers: the read-locked exchanges between shards, over this process's shards since
        they were made: those that ran (counted by the shard of the pair's first host), their sides
        admitted to the pool, and the sides (of any pair) that lost their merge to a host of another
        shard, the slot's holder or a lower claimant. Kept on the device by the kernels that decide
        them; reading them waits for the device, the chain never does."""
        keys = ("cross_exchanges", "cross_admitted", "lost_to_other_shard")
        if not self._arbitrate:
            return dict.fromkeys(keys, 0)
        return dict(zip(keys, map(sum, zip(*(e.ae_ro_counts() for e in self.engines)))))

    def probe_cross(self):
        """probe_piggyback: (pings, acks) with records that this process's shards have sent to hosts
        of other shards since they were made (the HIP engine's gx_probe_cross; waits for the device)."""
        return tuple(map(sum, zip(*(e.probe_cross() for e in self.engines))))

    def _ae_chain(self):
        """One run of the push-pull chain over the pairs the engines plan (the round's matching, or
        one batch of GX_PP_INITIATE): digests, the blocks each side leads, the partners' return
        blocks (gx.h); shard-local pairs overlap the exchanges. With lock_readers the pool's slots are
        arbitrated once the digests have told each shard its cross pairs' verdicts."""
        es = self.engines
        dsz, dig = self._exchange_sized([e.ae_bytes() for e in es], lambda i, p, c: es[i].ae_pack(p, c),
                                        after_pack=lambda e: e.ae_merge_local())
        delta = [e.ae_delta_bytes(_ptr(x), x.numel()) for e, x in zip(es, dig)]
        if self._arbitrate:
            self._claim_slots()
        lsz, lead = self._exchange_sized(delta, lambda i, p, c: es[i].ae_delta_pack(p, c))
        rsz, ret = self._exchange_sized(
            [e.ae_return_bytes(_ptr(x), x.numel()) for e, x in zip(es, lead)],
            lambda i, p, c: es[i].ae_return_pack(_ptr(lead[i]), lead[i].numel(), p, c))
        for a, b, c in zip(dsz, lsz, rsz):
            self.wire.add_ae(a, b, c)
        if self.trace_ae and any(x.numel() for x in dig):
            self.ae_trace.append(tuple([x.cpu().numpy().tobytes() for x in inb] for inb in (dig, lead, ret)))
        for e, x, y in zip(es, lead, ret):
            e.ae_merge(_ptr(x), x.numel(), _ptr(y), y.numel())

    def _push_pull(self):
        """The push-pull steps of a round and its end. With every host of the cluster locked (one
        census reduction) every pair fails: the counts only. Otherwise the chain runs once over the
        round's matching, or in GX_PP_INITIATE once per batch of the round's exchanges, in batch
        order (a batch sees the rows as the one before left them; every shard derives the same
        batches, so every rank makes the same collectives)."""
        es = self.engines
        initiate = self.G > 1 and es[0].params.push_pull_mode == PP_INITIATE
        nb = es[0].ae_batches() if initiate else 1  # host-only; 0: nobody's timer fires this round
        if nb == 0:
            pass
        elif self.G > 1 and self.skip_locked and lock_shortcut(es[0].params) and \
                int(self._reduce(torch.tensor([[e.lock_census()] for e in es], dtype=torch.int64), "sum")) == 0:
            for e in es:
                e.ae_skip_locked()
            self.ae_skipped += 1
        elif initiate:
            for _ in range(nb):
                self._ae_chain()
                self.ae_batches_run += 1
        else:
            self._ae_chain()
        for e in es:
            e.round_end()

    def round_gossip(self) -> bool:
        """The gossip half of one round: send, exchange, merge. True in a push-pull round, whose
        views then stand as the push-pull steps will read them; round_finish() ends the round."""
        planned = planned_exchange(self.shards[0].e.params)  # sizes from the seeded plan: no host wait
        self.exchange_paths["planned" if planned else "sized"] += 1
        return self._gossip_planned() if planned else self._gossip_sized()

    def round_finish(self, ae: bool):
        """The rest of the round round_gossip() began (`ae`: what it returned): the push-pull steps
        and the round's end."""
        if ae:
            self._push_pull()
        elif not planned_exchange(self.shards[0].e.params):  # the planned gossip's end call ended the round
            for s in self.shards:
                s.e.round_end()

    def run_rounds(self, n: int):
        for _ in range(n):
            self.round_finish(self.round_gossip())

    def watch_arm(self, n: int, log_rounds: int = 0):
        """A record watch on every held shard (include/gx_watch.h): each counts its own views."""
        for e in self.engines:
            e.watch_arm(n, log_rounds)

    def watch_set(self, first: int, keys, min_updated_ns):
        for e in self.engines:
            e.watch_set(first, keys, min_updated_ns)

    def watch_read(self, row: int = 0, rows=None):
        """The cluster's log: the shards' logs summed over all G shards (one reduction, made here and
        in no round). Returns what Engine.watch_read returns; the shards end the same rounds, so
        first_round, n_logged and missed are any shard's."""
        got = [e.watch_read(row, rows) for e in self.engines]
        counts, live, first_round, n_logged, missed = got[0]
        t = torch.tensor(np.stack([np.concatenate([c.reshape(-1), l]).astype(np.int64) for c, l, *_ in got]))
        s = self._reduce(t, "sum").cpu().numpy().astype(np.uint32)
        return s[:counts.size].reshape(counts.shape), s[counts.size:], first_round, n_logged, missed

    def stats(self) -> dict:
        """The cluster's counters: summed over the shards, but the latest `round` and
        `last_change_round` and the earliest of each FIRST_ROUND_STATS (-1: in no shard)."""
        sts = [e.stats() for e in self.engines]
        keys = sorted(sts[0])
        t = torch.tensor([[st[k] for k in keys] for st in sts], dtype=torch.int64)
        first = torch.tensor([[st[k] if st[k] >= 0 else _NEVER for k in FIRST_ROUND_STATS] for st in sts],
                             dtype=torch.int64)
        out = dict(zip(keys, self._reduce(t, "sum").tolist()))
        mx = self._reduce(t, "max").tolist()
        for k in ("round", "last_change_round"):
            out[k] = mx[keys.index(k)]
        for k, x in zip(FIRST_ROUND_STATS, self._reduce(first, "min").tolist()):
            out[k] = x if x < _NEVER else -1
        return out

    def converged(self):
        """(agreed, n): n = catalog records on which the live views disagree (all shards); once they
        agree, with the failure detector, the sum over shards of the nodes some of the shard's live
        views misjudge (a node misjudged in several shards counts once per shard). Every rank takes
        the same branch: `bad` is reduced first."""
        es = self.engines
        R = es[0].H * es[0].S
        mn = torch.empty((len(es), R), dtype=torch.int64, device=self.device)
        mx = torch.empty((len(es), R), dtype=torch.int64, device=self.device)
        for i, e in enumerate(es):
            e.view_minmax(_ptr(mn[i]), _ptr(mx[i]))
        bad = int((self._reduce(mn, "min") != self._reduce(mx, "max")).sum().item())
        if bad == 0 and es[0].params.fd_enable:  # membership agrees with the truth on every shard too
            bad = int(self._reduce(torch.tensor([[e.fd_converged()[1]] for e in es], dtype=torch.int64), "sum"))
        return bad == 0, bad


class LocalShards(ShardRounds):
    """G shards of one cluster driven in one process; the transport is slicing and concatenation."""

    def __init__(self, lib, G: int, device="cpu", **kw):
        super().__init__(lib, G, range(G), device, kw)

    @classmethod
    def load(cls, lib, dirname, device="cpu", **override) -> "LocalShards":
        """The cluster `save` wrote into `dirname`: every shard file found there (shard 0's name tells
        G). override: as Engine.from_checkpoint, applied to every shard."""
        names = [n for n in sorted(os.listdir(dirname)) if n.startswith("shard_000_of_") and n.endswith(".gxck")]
        if len(names) != 1:
            raise FileNotFoundError(f"no single shard_000_of_*.gxck in {dirname}")
        G = int(names[0][len("shard_000_of_"):-len(".gxck")])
        self = cls.__new__(cls)
        ShardRounds.__init__(self, lib, G, range(G), device, None,
                             engines=cls._load_engines(lib, dirname, G, range(G), device, override))
        return self

    def _matrix(self, rows) -> List[List[int]]:
        if isinstance(rows[0], torch.Tensor):
            return torch.stack(rows).tolist()  # device rows: the one host wait of the exchange
        return [r.tolist() for r in rows]

    def _move(self, bufs, m, planned=False) -> List[torch.Tensor]:
        off = [[0, *accumulate(row)] for row in m]  # off[src][dst]: where dst's segment starts in src's buffer
        return [torch.cat([b[o[dst]:o[dst + 1]] for b, o in zip(bufs, off)]) for dst in range(self.G)]

    def _reduce(self, t: torch.Tensor, op: str) -> torch.Tensor:
        return _fold(t, op)


class DistShard(ShardRounds):
    """This process's shard; the others are peers in a torch.distributed group, and the transport is
    its collectives."""

    CHUNK = 256 << 20  # bytes per peer per all-to-all call

    def __init__(self, lib, rank: int, world: int, device, group=None, _engines=None, **kw):
        import torch.distributed as dist
        self.dist = dist
        self.group = group
        self.rank, self.world = rank, world
        super().__init__(lib, world, [rank], device, kw, engines=_engines)
        self.e = self.shards[0].e
        # gloo has no device all-to-all / all-gather: a gloo group over device shards (the one-GPU
        # rehearsal of the RCCL path in tests/test_gpu_dist.py) stages collectives through the host
        self.stage = self.device.type == "cuda" and dist.get_backend(group) == "gloo"
        self._precv = torch.empty(0, dtype=torch.uint8, device=self.device)  # the planned move's inbox

    @classmethod
    def load(cls, lib, dirname, rank: int, world: int, device, group=None, **override) -> "DistShard":
        """This rank's shard of the cluster `save` wrote into `dirname` (every rank wrote its own file
        there); no collective. override: as Engine.from_checkpoint."""
        return cls(lib, rank, world, device, group=group,
                   _engines=cls._load_engines(lib, dirname, world, [rank], device, override))

    def _host(self, t: torch.Tensor) -> torch.Tensor:
        return t.cpu() if self.stage else t

    def _a2a(self, recv, send, rs, ss):
        if not self.stage:
            self.dist.all_to_all_single(recv, send, output_split_sizes=rs, input_split_sizes=ss, group=self.group)
            return
        r = torch.empty(recv.numel(), dtype=recv.dtype)
        self.dist.all_to_all_single(r, send.cpu(), output_split_sizes=rs, input_split_sizes=ss, group=self.group)
        recv.copy_(r)

    def _all_reduce(self, t: torch.Tensor, op):
        h = self._host(t)
        self.dist.all_reduce(h, op=op, group=self.group)
        if h is not t:
            t.copy_(h)

    def _reduce(self, t: torch.Tensor, op: str) -> torch.Tensor:
        t = _fold(t, op).to(self.device)
        self._all_reduce(t, getattr(self.dist.ReduceOp, op.upper()))
        return t

    def _matrix(self, rows) -> List[List[int]]:
        """Every rank learns the whole size matrix in one all-gather: its receive sizes, and the
        number of chunked calls all ranks make. A device row travels in it without a host wait of
        its own."""
        mine = rows[0]
        if not isinstance(mine, torch.Tensor):
            mine = torch.tensor(mine.astype(np.int64), device=self.device)
        mine = self._host(mine)
        got = [torch.empty_like(mine) for _ in range(self.world)]
        self.dist.all_gather(got, mine, group=self.group)
        return torch.stack(got).tolist()  # the one host wait of the exchange

    def _move(self, bufs, m, planned=False) -> List[torch.Tensor]:
        """all-to-all of this shard's per-destination segments. The planned move sends from the
        persistent buffer and receives into one that grows to a round's size when a round needs more
        (with a quarter of headroom); its bound, every other shard's fanout slots per host, is only
        reached when every packet of the cluster comes here."""
        send = bufs[0]
        ss, rs = m[self.rank], [r[self.rank] for r in m]
        ns, nr = sum(ss), sum(rs)
        if planned:
            if ns > send.numel():
                raise RuntimeError("planned exchange larger than its bound")  # cannot happen (gx.h)
            if nr > self._precv.numel():
                self._precv = torch.empty(nr + nr // 4, dtype=torch.uint8, device=self.device)
            send, recv = send[:ns], self._precv[:nr]
        else:
            recv = torch.empty(nr, dtype=torch.uint8, device=self.device)
        self._a2a_chunked(recv, send, rs, ss, max(map(max, m)))
        return [recv]

    def _a2a_chunked(self, recv, send, rs, ss, largest):
        """all_to_all_single of per-peer segments, split into calls of at most CHUNK bytes per peer.
        `largest`: the largest segment between any two ranks (every rank knows the whole size
        matrix), so every rank makes the same number of calls, ceil(largest / CHUNK)."""
        calls = (int(largest) + self.CHUNK - 1) // self.CHUNK
        if calls <= 1:
            self._a2a(recv, send, rs, ss)
            return
        soff = np.concatenate([[0], np.cumsum(ss)])
        roff = np.concatenate([[0], np.cumsum(rs)])
        for c in range(calls):
            lo = c * self.CHUNK
            s_part = [max(0, min(self.CHUNK, n - lo)) for n in ss]
            r_part = [max(0, min(self.CHUNK, n - lo)) for n in rs]
            s_buf = torch.cat([send[int(soff[p]) + lo:int(soff[p]) + lo + s_part[p]] for p in range(self.world)])
            r_buf = torch.empty(sum(r_part), dtype=torch.uint8, device=self.device)
            self._a2a(r_buf, s_buf, r_part, s_part)
            o = 0
            for p in range(self.world):
                if r_part[p]:
                    recv[int(roff[p]) + lo:int(roff[p]) + lo + r_part[p]].copy_(r_buf[o:o + r_part[p]])
                o += r_part[p]

    def _exchange(self, sizes, packer) -> torch.Tensor:
        """One sized exchange of this shard's messages (`sizes`: host array or device tensor, as
        _matrix takes them; packer(ptr, cap) fills the send buffer); returns the inbox."""
        return self._exchange_sized([sizes], lambda i, p, c: packer(p, c))[1][0]

    def close(self):
        """Wait for the engine's work (its stream and the planned exchange's look-ahead stream) and
        free it, before the caller tears the process group down: RCCL's communicator teardown
        must not race the engine's kernels or buffers."""
        if getattr(self, "e", None) is None:
            return
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.e.close()
        self._pb = None
        self._precv = None
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
