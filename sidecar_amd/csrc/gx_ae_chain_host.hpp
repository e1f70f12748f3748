// gx_ae_chain_host.hpp — host side of a sharded engine's push-pull chain: the plan of
// a step's pairs, the digest, lead and return exchanges (gx_ae_bytes .. gx_ae_merge), the pool's
// arbitration under lock_readers (gx_ae_claim_*), the all-locked shortcut (gx_ae_skip_locked) and
// gx_ae_batches. The step's host state is gx_engine::AeChain; the kernels are in gx_kernels.hpp.
// Included by gx_engine.hip after the engine's host helpers.
#pragma once
#include <numeric>
#include <vector>

// ------------------------------------------------------------------------- the step's guard --
// A chain call is in order when the calls it builds on have completed for the step that is current
// now (ae_step). Every call asks ae_done before it launches or reads anything, and says ae_mark
// once it has succeeded.
static bool ae_done(const gx_engine *e, uint32_t calls) {
  return e->chain.step == ae_step(e) && (e->chain.done & calls) == calls;
}
static void ae_mark(gx_engine *e, uint32_t call) {
  gx_engine::AeChain &c = e->chain;
  if (c.step != ae_step(e)) {  // the first call of a new step: what an earlier step completed is void
    c.step = ae_step(e);
    c.done = 0;
  }
  c.done |= call;
}

static size_t dig_bytes(const gx_engine *e) { return dig_stride(e->d, e->nblk); }
// the lead and return kernels with the offsets up front, a wave per block (profiles/ab_shard_ae.sh),
// while a row's digest blocks fit their LDS tables
static bool ae_wave_blocks(const gx_engine *e) { return e->nblk <= XS_MAXB; }

// ---------------------------------------------------------------- one selection site per kernel --
// (as launch_send and launch_merge: every variant is named here and nowhere else)
// k_ae_mask: with the read-locked verdicts under gx.h lock_readers
static void launch_ae_mask(gx_engine *e, const void *digests) {
  const uint32_t np = e->chain.n_pack;
  with_flag(e->d.p.lock_readers != 0, [&](auto RO) {
    k_ae_mask<RO()><<<np, 256, 0, e->stream>>>(e->d, (const uint8_t *)digests, e->ae_dig, e->ae_pack_t, e->ae_pack_host,
                                               e->ae_pack_other, e->ae_pack_first, e->nblk, e->nmw, e->ae_mask,
                                               e->ae_fmask, e->ae_lt, e->ae_cnt, e->ae_nfol, e->ae_sz, e->ae_sz + np,
                                               e->ae_err, e->ae_skip, RO() ? e->ae_rov : nullptr,
                                               RO() ? e->ro_xc : nullptr);
  });
}
static void launch_ae_lead_pack(gx_engine *e, void *buf) {
  const uint32_t np = e->chain.n_pack;
  if (ae_wave_blocks(e))
    k_ae_lead_pack_w<<<np, 256, 0, e->stream>>>(e->d, e->ae_pack_host, e->ae_pack_t, e->ae_mask, e->ae_cnt, e->ae_off,
                                                e->nmw, (const ulonglong2 *)e->ae_dig, e->nblk, (uint8_t *)buf);
  else
    k_ae_lead_pack<<<np, 256, 0, e->stream>>>(e->d, e->ae_pack_host, e->ae_pack_t, e->ae_mask, e->ae_cnt, e->ae_off,
                                              e->nmw, (uint8_t *)buf);
}
// COUNT: the return messages' sizes only (gx_ae_return_bytes); else the messages into buf
template <bool COUNT>
static void launch_ae_ret(gx_engine *e, const void *lead, void *buf) {
  const uint32_t np = e->chain.n_pack;
  uint64_t *rsz = e->ae_sz + 2 * np;
  const uint64_t *roff = COUNT ? nullptr : e->ae_off + 2 * np, *rtab = COUNT ? nullptr : e->ae_off + 3 * np;
  if (ae_wave_blocks(e))
    k_ae_ret_w<COUNT><<<np, 256, 0, e->stream>>>(e->d, e->ae_pack_host, e->ae_pack_t, e->ae_fmask, e->ae_nfol, e->ae_lt,
                                                 (const uint8_t *)lead, e->ae_off + np, e->nblk, e->nmw, rsz, roff, rtab,
                                                 (uint8_t *)buf, e->ae_retL);
  else
    k_ae_ret<COUNT><<<np, 256, 0, e->stream>>>(e->d, e->ae_pack_host, e->ae_pack_t, e->ae_fmask, e->ae_nfol, e->ae_lt,
                                               (const uint8_t *)lead, e->ae_off + np, e->nblk, e->nmw, rsz, roff, rtab,
                                               (uint8_t *)buf);
}

// ------------------------------------------------------------------------------- the plan --
// The matching's pairs in global order t (k_ae_pairs, as k_ae draws them) on the host.
static int ae_pairs_host(gx_engine *e, const AeMatching &m, std::vector<uint32_t> &pa, std::vector<uint32_t> &pb) {
  pa.resize(m.np);
  pb.resize(m.np);
  if (!m.np) return GX_OK;
  k_ae_pairs<<<(m.np + 255) / 256, 256, 0, e->stream>>>(m.base[0], m.len[0], m.key0, m.base[1], m.len[1], m.key1, m.n0,
                                                         m.np, e->ae_pa, e->ae_pb);
  HIPCHK(hipMemcpyAsync(pa.data(), e->ae_pa, 4ull * m.np, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(pb.data(), e->ae_pb, 4ull * m.np, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

// Push-pull plan of this step (host side): global pairs t -> (a, b); local pairs, rows to send
// (grouped by destination shard, ascending t) and rows to receive (by source shard, ascending t).
static int ae_plan(gx_engine *e, uint64_t *bytes) {
  Dev &d = e->d;
  gx_engine::AeChain &c = e->chain;
  std::vector<uint32_t> pa, pb, pt;  // pt: each pair's index in the round's list (the messages' pair index)
  if (d.p.push_pull_mode == GX_PP_INITIATE) {
    // the batch at the cursor (ae_step_due): its exchanges, named by their place in initiator order
    pp_schedule(e);
    const size_t n = e->pp_idx.size(), lo = e->pp_off[e->pp_cursor], hi = e->pp_off[e->pp_cursor + 1];
    if (hi - lo > d.H / 2) return GX_EINVAL;  // hosts of a batch are disjoint: the pair buffers hold H / 2 + 1
    pa.assign(e->pp_host.begin() + lo, e->pp_host.begin() + hi);
    pb.assign(e->pp_host.begin() + n + lo, e->pp_host.begin() + n + hi);
    pt.assign(e->pp_idx.begin() + lo, e->pp_idx.begin() + hi);
    int rc = sync_check(e);  // the batch before (its launches read the plan rewritten below) is done
    if (rc) return rc;
  } else {
    // the pair schedule (Feistel permutations) on the device, read back once
    int rc = ae_pairs_host(e, ae_matching(d), pa, pb);
    if (rc) return rc;
    pt.resize(pa.size());
    std::iota(pt.begin(), pt.end(), 0u);
  }
  // one pass over the pairs: cross pairs bucketed by the partner's shard (messages go out and
  // come in grouped by shard, ascending t, so cross pair k has the same index both ways), then
  // the pairs with both hosts here
  std::vector<std::vector<uint32_t>> by_g(d.G);
  std::vector<uint32_t> local_t;
  for (size_t t = 0; t < pa.size(); t++) {
    // a pair with a crashed member does not run (both shards skip it alike; pair indices unchanged)
    if (d.departures && (departed_at(d.p, d.round, pa[t]) || departed_at(d.p, d.round, pb[t]))) continue;
    bool la = own(e, pa[t]), lb = own(e, pb[t]);
    if (la && lb) local_t.push_back((uint32_t)t);
    else if (la != lb) by_g[shard_of(d, la ? pb[t] : pa[t])].push_back((uint32_t)t);
  }
  // the rows to send, in pack order: this shard's host, the pair's index, the partner, who initiates
  std::vector<uint32_t> pack_host, pack_t, pack_other;
  std::vector<uint8_t> pack_first;
  c.gstart.assign(d.G + 1, 0);
  for (uint32_t g = 0; g < d.G; g++) {
    c.gstart[g] = (uint32_t)pack_host.size();
    for (uint32_t t : by_g[g]) {
      const bool la = own(e, pa[t]);
      pack_host.push_back(la ? pa[t] : pb[t]);
      pack_t.push_back(pt[t]);
      pack_other.push_back(la ? pb[t] : pa[t]);
      pack_first.push_back(la ? 1 : 0);
    }
    bytes[g] = by_g[g].size() * dig_bytes(e);
  }
  c.n_pack = c.gstart[d.G] = (uint32_t)pack_host.size();
  // the pairs to run: cross pair k (this shard's host first) with the row it receives, k, and
  // whether it counts the exchange; then the local pairs, no row
  std::vector<uint32_t> plan_a(pack_host), plan_b(pack_other);
  std::vector<uint8_t> plan_cnt(pack_first);
  for (uint32_t t : local_t) {
    plan_a.push_back(pa[t]);
    plan_b.push_back(pb[t]);
  }
  c.n_plan = (uint32_t)plan_a.size();
  std::vector<int32_t> plan_row(c.n_plan, -1);
  std::iota(plan_row.begin(), plan_row.begin() + c.n_pack, 0);
  plan_cnt.resize(c.n_plan, 0);
  if (c.n_plan) {
    HIPCHK(hipMemcpy(e->ae_pa, plan_a.data(), 4 * c.n_plan, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ae_pb, plan_b.data(), 4 * c.n_plan, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ae_prow, plan_row.data(), 4 * c.n_plan, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ae_pcount, plan_cnt.data(), c.n_plan, hipMemcpyHostToDevice));
  }
  if (c.n_pack) {
    HIPCHK(hipMemcpy(e->ae_pack_host, pack_host.data(), 4 * c.n_pack, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ae_pack_t, pack_t.data(), 4 * c.n_pack, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ae_pack_other, pack_other.data(), 4 * c.n_pack, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ae_pack_first, pack_first.data(), c.n_pack, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(e->ae_skip, 0, c.n_pack, e->stream));
  }
  if (pp_state(d)) k_fd_snap<<<2048, 256, 0, e->stream>>>(d);  // round-start member lists (pushPull)
  ae_mark(e, AE_PLANNED);
  return GX_OK;
}

// One exchange's messages as they lie in a send buffer: by destination shard (gstart), in pack
// order, each shard's part opening with `head` bytes per message (the return's size table, gx.h).
// off[k]: where message k starts; tab[k]: where its table entry does; part[g]: shard g's bytes
// (tab, part: or null). Returns the total.
static uint64_t ae_layout(const gx_engine::AeChain &c, uint64_t head, const uint64_t *size, uint64_t *off, uint64_t *tab,
                          uint64_t *part) {
  uint64_t o = 0;
  for (size_t g = 0; g + 1 < c.gstart.size(); g++) {
    const uint32_t k0 = c.gstart[g], k1 = c.gstart[g + 1];
    const uint64_t seg = o;
    o += head * (k1 - k0);
    for (uint32_t k = k0; k < k1; k++) {
      if (tab) tab[k] = seg + head * (k - k0);
      off[k] = o;
      o += size[k];
    }
    if (part) part[g] = o - seg;
  }
  return o;
}

// The cross pairs' inboxes and per-pair tables, as the kernels that rebuild a partner's row take them.
static AeIn ae_in(const gx_engine *e, const void *lead, const void *ret) {
  AeIn in;
  in.lead = (const uint8_t *)lead;
  in.ret = (const uint8_t *)ret;
  in.ioff = e->ae_off + e->chain.n_pack;
  in.rioff = e->ae_rioff;
  in.lmask = e->ae_mask;
  in.fmask = e->ae_fmask;
  in.lt = e->ae_lt;
  in.nlead = e->ae_cnt;
  in.bcnt = e->ae_bcnt;
  in.nmw = e->nmw;
  in.nblk = e->nblk;
  return in;
}
// Launch the planned pairs [lo, hi) (received-row pairs first, then shard-local pairs).
static void ae_plan_launch(gx_engine *e, uint32_t lo, uint32_t hi, const void *lead, const void *ret,
                           hipStream_t st = nullptr) {
  if (hi <= lo) return;
  if (!st) st = e->stream;
  LaunchTimer t(e, GX_K_AE, st);
  const AeIn in = ae_in(e, lead, ret);
  // fewer than 4 pairs per CU: per-block bandwidth decides (2 tiles in flight measured slower for
  // the cross pairs of a post-heal round: 8.2 -> 9.3 ms at G = 2, H = 16384)
  const bool small = hi - lo < 1024;
  launch_ae_plan(e, small, hi - lo, st, e->ae_pa + lo, e->ae_pb + lo, e->ae_prow + lo, e->ae_pcount + lo, in, e->ae_skip);
}

// gx.h lock_readers: the pool rows of the cross pairs' admitted read-locked sides (k_ae_xdefer)
static void ae_xdefer_launch(gx_engine *e, const void *lead) {
  if (!e->chain.n_pack) return;
  LaunchTimer t(e, GX_K_AE);
  const AeIn in = ae_in(e, lead, nullptr);
  with_flag(vec_of(e), [&](auto V) {
    k_ae_xdefer<V()><<<e->chain.n_pack, 256, 0, e->stream>>>(e->d, e->ae_pack_host, e->ae_pack_first, e->ae_rov, in,
                                                             e->ro_xc);
  });
}

static bool ae_claims_on(const gx_engine *e) { return e->d.G > 1 && e->d.p.lock_readers; }

// k_ae_locked_note's counts of the exchanges (pa[t], pb[t]): those whose first host lives here
// (each exchange is counted once, by that shard), and whether any host of them does.
static void ae_locked_note(gx_engine *e, const uint32_t *pa, const uint32_t *pb, size_t n) {
  uint32_t n_first = 0, any = 0;
  for (size_t t = 0; t < n; t++) {
    const bool la = own(e, pa[t]), lb = own(e, pb[t]);
    n_first += la ? 1u : 0u;
    any |= (la || lb) ? 1u : 0u;
  }
  k_ae_locked_note<<<1, 64, 0, e->stream>>>(e->d, n_first, any);
}

// ------------------------------------------------------------------------------ ABI ------
extern "C" {

int gx_ae_bytes(gx_engine *e, uint64_t *bytes) {
  if (!e || !bytes) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  gx_engine::AeChain &c = e->chain;
  for (uint32_t g = 0; g < e->d.G; g++) bytes[g] = 0;
  c.n_plan = c.n_pack = 0;
  c.done &= ~AE_PLANNED;  // planned again in one step, the local pairs stay run (AE_LOCAL)
  if (!ae_step_due(e)) return GX_OK;
  return ae_plan(e, bytes);
}

int gx_ae_pack(gx_engine *e, void *buf, uint64_t cap) {
  if (!e || (cap && !buf)) return GX_EINVAL;
  const uint32_t np = e->chain.n_pack;
  if (!np) return GX_OK;
  if (!ae_done(e, AE_PLANNED) || cap < np * dig_bytes(e)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  with_flags(vec_of(e), e->d.p.lock_readers != 0, [&](auto V, auto RO) {
    k_ae_digest<V(), RO()><<<np, 256, 0, e->stream>>>(e->d, e->ae_pack_host, e->ae_pack_t, e->ae_pack_other,
                                                      e->ae_pack_first, (uint8_t *)buf, e->ae_dig, e->nblk, e->ae_bcnt);
  });
  return phase_done(e);
}

// Received digests -> differing blocks and who leads each; lead message sizes per shard, and the
// offsets of this side's lead messages and of the partner's in the lead inbox.
int gx_ae_delta_bytes(gx_engine *e, const void *digests, uint64_t bytes, uint64_t *out) {
  if (!e || !out || (bytes && !digests)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  Dev &d = e->d;
  gx_engine::AeChain &c = e->chain;
  for (uint32_t g = 0; g < d.G; g++) out[g] = 0;
  c.done &= ~(AE_DELTA | AE_RET);
  c.lead_total = c.lead_in_total = 0;
  if (!ae_step_due(e)) return bytes ? GX_EINVAL : GX_OK;
  if (!ae_done(e, AE_PLANNED) || bytes != c.n_pack * dig_bytes(e)) return GX_EINVAL;
  const uint32_t np = c.n_pack;
  std::vector<uint64_t> sz(2 * (size_t)np);
  if (np) {
    HIPCHK(hipMemsetAsync(e->ae_err, 0, sizeof(uint32_t), e->stream));
    launch_ae_mask(e, digests);
    if (pp_state(d))  // the partners' member lists ride with their digests
      k_fd_rsnap<<<1024, 256, 0, e->stream>>>(d, (const uint8_t *)digests, dig_bytes(e), e->nblk, np, e->fd_rsnap);
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, e->ae_err, sizeof(uint32_t), hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(sz.data(), e->ae_sz, sizeof(uint64_t) * 2 * np, hipMemcpyDeviceToHost, e->stream));
    int rc = sync_main(e);
    if (rc) return rc;
    if (err) return GX_EINVAL;  // digests of another pair or another row size
  }
  c.lead_off.assign(2 * (size_t)np, 0);  // this side's lead messages, then the partners' in the lead inbox
  c.lead_total = ae_layout(c, 0, sz.data(), c.lead_off.data(), nullptr, out);
  c.lead_in_total = ae_layout(c, 0, sz.data() + np, c.lead_off.data() + np, nullptr, nullptr);
  if (np) HIPCHK(hipMemcpy(e->ae_off, c.lead_off.data(), sizeof(uint64_t) * 2 * np, hipMemcpyHostToDevice));
  ae_mark(e, AE_DELTA);
  return GX_OK;
}

int gx_ae_delta_pack(gx_engine *e, void *buf, uint64_t cap) {
  if (!e || (cap && !buf)) return GX_EINVAL;
  if (!e->chain.n_pack) return GX_OK;
  if (!ae_done(e, AE_DELTA) || cap < e->chain.lead_total) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  launch_ae_lead_pack(e, buf);
  return phase_done(e);
}

// Received lead blocks -> return message sizes: per destination shard a u64 size table, then the
// messages (gx.h "return").
int gx_ae_return_bytes(gx_engine *e, const void *lead, uint64_t lead_bytes, uint64_t *out) {
  if (!e || !out || (lead_bytes && !lead)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  gx_engine::AeChain &c = e->chain;
  for (uint32_t g = 0; g < e->d.G; g++) out[g] = 0;
  c.done &= ~AE_RET;
  c.ret_total = 0;
  const uint32_t np = c.n_pack;
  if (!ae_step_due(e) || !np) return lead_bytes ? GX_EINVAL : GX_OK;
  if (!ae_done(e, AE_DELTA) || lead_bytes != c.lead_in_total) return GX_EINVAL;
  launch_ae_ret<true>(e, lead, nullptr);
  std::vector<uint64_t> rsz(np);
  HIPCHK(hipMemcpyAsync(rsz.data(), e->ae_sz + 2 * np, sizeof(uint64_t) * np, hipMemcpyDeviceToHost, e->stream));
  int rc = sync_main(e);
  if (rc) return rc;
  std::vector<uint64_t> off(2 * (size_t)np);  // message offsets, size-table entry offsets
  c.ret_total = ae_layout(c, 8, rsz.data(), off.data(), off.data() + np, out);
  HIPCHK(hipMemcpy(e->ae_off + 2 * np, off.data(), sizeof(uint64_t) * 2 * np, hipMemcpyHostToDevice));
  ae_mark(e, AE_RET);
  return GX_OK;
}

int gx_ae_return_pack(gx_engine *e, const void *lead, uint64_t lead_bytes, void *buf, uint64_t cap) {
  if (!e || (cap && !buf) || (lead_bytes && !lead)) return GX_EINVAL;
  const gx_engine::AeChain &c = e->chain;
  if (!c.n_pack) return GX_OK;
  if (!ae_done(e, AE_RET) || cap < c.ret_total || lead_bytes != c.lead_in_total) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  launch_ae_ret<false>(e, lead, buf);
  return phase_done(e);
}

int gx_ae_merge_local(gx_engine *e) {
  if (!e) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  if (!ae_step_due(e) || ae_done(e, AE_LOCAL)) return GX_OK;
  if (!ae_done(e, AE_PLANNED)) return GX_EINVAL;
  // on the side stream, after the rows are packed: the exchange layer's collectives (ordered
  // behind `stream`) run while these merges do; gx_ae_merge joins them back
  HIPCHK(hipEventRecord(e->side_start, e->stream));
  HIPCHK(hipStreamWaitEvent(e->side_stream, e->side_start, 0));
  ae_plan_launch(e, e->chain.n_pack, e->chain.n_plan, nullptr, nullptr, e->side_stream);
  HIPCHK(hipEventRecord(e->side_done, e->side_stream));
  e->side_pending = true;
  HIPCHK(hipGetLastError());
  ae_mark(e, AE_LOCAL);
  return GX_OK;
}

int gx_ae_merge(gx_engine *e, const void *lead, uint64_t lead_bytes, const void *ret, uint64_t ret_bytes) {
  if (!e || (lead_bytes && !lead) || (ret_bytes && !ret)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  if (!ae_round(e)) return GX_OK;
  if (e->d.G < 2) {
    int rc = ae_whole_impl(e, false);
    return rc ? rc : sync_check(e);
  }
  if (!ae_step_due(e)) return (lead_bytes || ret_bytes) ? GX_EINVAL : GX_OK;  // past the round's last batch
  if (!ae_done(e, AE_PLANNED)) return GX_EINVAL;
  const gx_engine::AeChain &c = e->chain;
  const uint32_t np = c.n_pack;
  if (np) {
    if (!ae_done(e, AE_RET) || lead_bytes != c.lead_in_total) return GX_EINVAL;
    // the return inbox: per source shard a size table, then that shard's messages. The sizes are
    // on the device, so the walk (ae_layout's, from the receiving end) reads them shard by shard.
    std::vector<uint64_t> rio(np), tab;
    uint64_t o = 0;
    for (uint32_t g = 0; g < e->d.G; g++) {
      uint32_t k0 = c.gstart[g], k1 = c.gstart[g + 1];
      if (k1 == k0) continue;
      if (o + 8ull * (k1 - k0) > ret_bytes) return GX_EINVAL;
      tab.resize(k1 - k0);
      HIPCHK(hipMemcpyAsync(tab.data(), (const uint8_t *)ret + o, 8ull * (k1 - k0), hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      o += 8ull * (k1 - k0);
      for (uint32_t k = k0; k < k1; k++) {
        rio[k] = o;
        o += tab[k - k0];
      }
    }
    if (o != ret_bytes) return GX_EINVAL;
    HIPCHK(hipMemcpy(e->ae_rioff, rio.data(), sizeof(uint64_t) * np, hipMemcpyHostToDevice));
  }
  if (e->d.p.lock_readers) {  // the admitted read-locked sides of cross pairs keep their partners' rows
    if (!ae_done(e, AE_CLAIM)) return GX_EINVAL;  // gx_ae_claim_want, gx_ae_claim_set come first
    ae_xdefer_launch(e, lead);
  }
  ae_plan_launch(e, 0, ae_done(e, AE_LOCAL) ? c.n_pack : c.n_plan, lead, ret);
  if (pp_state(e->d) && c.n_plan) {  // pushPull's membership half, every planned pair
    LaunchTimer t(e, GX_K_FD);
    k_fd_pushpull_plan<<<2 * c.n_plan, 64, 0, e->stream>>>(e->d, e->ae_pa, e->ae_pb, e->ae_prow, e->ae_skip,
                                                           e->fd_rsnap);
  }
  int jr = join_side(e);  // the next batch, and the next round's phases, see the local pairs merged
  if (jr) return jr;
  if (e->d.p.push_pull_mode == GX_PP_INITIATE) e->pp_cursor++;  // the chain's next run takes the next batch
  return phase_done(e);
}

// gx.h lock_readers = 1 on a sharded engine (outside gx.h's declarations, described there with the
// sharded rounds): the cluster-wide pool's arbitration, between gx_ae_delta_bytes and gx_ae_merge in
// every run of the chain. gx_ae_claim_want writes lock_defer_slots int64 entries at `want` (device
// memory): -1 for a slot one of this shard's hosts holds, else this shard's lowest claimant of the
// slot in this run (the read-locked sides of its local and cross pairs), else 2^62. The caller takes
// the minimum over all shards and hands it to gx_ae_claim_set, which admits the claimants named in
// it, counts the others lost and runs the local read-locked exchanges (k_ae_rox). A run with nothing
// planned on this shard still answers (held slots, no claimants) and sets nothing.
int gx_ae_claim_want(gx_engine *e, int64_t *want) {
  if (!e || !want || !ae_claims_on(e)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  const gx_engine::AeChain &c = e->chain;
  const bool due = ae_step_due(e);
  if (due && !ae_done(e, c.n_pack ? AE_PLANNED | AE_DELTA : AE_PLANNED)) return GX_EINVAL;
  if (due && !ae_done(e, AE_LOCAL)) {  // the local pairs' launch flags their read-locked exchanges
    int rc = gx_ae_merge_local(e);
    if (rc) return rc;
  }
  int jr = join_side(e);  // ro_flag is written
  if (jr) return jr;
  const uint32_t np = due ? c.n_pack : 0, nl = due ? c.n_plan - np : 0;  // cross pairs, then local ones
  k_ae_want<<<1, 256, 0, e->stream>>>(e->d, e->ae_pa + np, e->ae_pb + np, nl, e->ae_pack_host, e->ae_rov, np,
                                      (long long *)want);
  return phase_done(e);
}
int gx_ae_claim_set(gx_engine *e, const int64_t *won) {
  if (!e || !won || !ae_claims_on(e)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  if (!ae_step_due(e)) return GX_OK;
  if (!ae_done(e, AE_PLANNED | AE_LOCAL) || e->side_pending) return GX_EINVAL;
  const uint32_t lo = e->chain.n_pack, nl = e->chain.n_plan - lo;  // the local pairs
  {
    LaunchTimer t(e, GX_K_AE);
    k_ae_claim_set<<<1, 256, 0, e->stream>>>(e->d, e->ae_pa + lo, e->ae_pb + lo, nl, e->ae_pack_host, e->ae_rov,
                                             e->chain.n_pack, (const long long *)won, e->ro_xc);
    if (nl)  // the local read-locked exchanges, slots decided
      with_flags(vec_of(e), ev_of(e), [&](auto V, auto E) {
        k_ae_rox<V(), E()><<<ae_grid(nl, 1), 256, 0, e->stream>>>(e->d, e->ae_pa + lo, e->ae_pb + lo, 0, 0);
      });
  }
  ae_mark(e, AE_CLAIM);
  return phase_done(e);
}
// The driver's counters of the sharded read-locked exchanges, summed since gx_create: out[0] cross-
// shard exchanges that ran with a read-locked side (counted by the shard of the pair's first host),
// out[1] read-locked sides of cross pairs admitted to the pool, out[2] sides of this shard that lost
// their merge to a host of another shard (the slot's holder, or a lower claimant). Waits for the device.
int gx_ae_ro_counts(gx_engine *e, uint64_t *out) {
  if (!e || !out || !ae_claims_on(e)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipMemcpyAsync(out, e->ro_xc, sizeof(uint64_t) * 3, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

int gx_lock_census(gx_engine *e, uint32_t *unlocked) {
  if (!e || !unlocked) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  uint32_t *dv;
  GXTRY(api_carve(e, region(dv, 1)));
  HIPCHK(hipMemsetAsync(dv, 0, sizeof(uint32_t), e->stream));
  if (e->d.Hl) k_lock_census<<<nblk(e->d.Hl, 256), 256, 0, e->stream>>>(e->d, dv);
  return read_back(e, dv, unlocked);
}

// A push-pull round in which every host of the cluster holds the lock (the caller's collective
// census): every pair fails, so the round is only its counts, as the full exchange would make them
// (gx_ae_bytes .. gx_ae_merge): ae_locked once per pair, by the shard of its first host.
int gx_ae_skip_locked(gx_engine *e) {
  if (!e) return GX_EINVAL;
  Dev &d = e->d;
  if (!ae_round(e)) return GX_OK;
  // sharded engines only (one engine runs its push-pull itself; the pair buffers exist when G > 1)
  // (nor with lock_readers: an exchange between read-locked hosts runs)
  if (d.G < 2 || !e->ae_pa || !d.p.lock_model || d.departures || d.p.fd_enable || d.p.lock_readers) return GX_EINVAL;
  uint32_t unlocked = 0;
  int rc = gx_lock_census(e, &unlocked);
  if (rc) return rc;
  if (unlocked) return GX_EINVAL;  // a host here is free: the pairs must run the exchange
  GXTRY(enter(e, ENTRY_PHASE));
  if (d.p.push_pull_mode == GX_PP_INITIATE) {  // once per exchange, by its initiator's shard (pp_schedule)
    e->pp_cursor = pp_schedule(e);  // no batch is left to run
    const size_t n = e->pp_idx.size();
    if (!n) return GX_OK;
    ae_locked_note(e, e->pp_host.data(), e->pp_host.data() + n, n);
    return phase_done(e);
  }
  std::vector<uint32_t> pa, pb;
  rc = ae_pairs_host(e, ae_matching(d), pa, pb);
  if (rc || pa.empty()) return rc;
  ae_locked_note(e, pa.data(), pb.data(), pa.size());
  return phase_done(e);
}

// Outside gx.h's declarations (described there with the sharded rounds): how many runs of the
// push-pull chain gx_ae_bytes .. gx_ae_merge this round takes on a sharded engine: 0 when it is not
// a push-pull round or nobody initiates, 1 for the matching, the batch count in GX_PP_INITIATE.
// From (seed, round) on the host: no device work, the same answer on every shard.
int gx_ae_batches(gx_engine *e, uint32_t *n) {
  if (!e || !n) return GX_EINVAL;
  *n = !ae_round(e) ? 0 : e->d.p.push_pull_mode == GX_PP_INITIATE ? pp_schedule(e) : 1;
  return GX_OK;
}

}  // extern "C"
