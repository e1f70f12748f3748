// gx_engine.hip — sidecar-gx gossip-convergence engine for MI355X (gfx950).
//
// Implements include/gx.h. One engine object owns one GPU's slice of the simulated cluster and
// advances it one gossip round at a time (gx_run_rounds). Round phases and the kernels that run
// them (DESIGN.md "Round model", "Kernels"):
//   0+1 k_owner      a team of S lanes per host: wake re-armed SendServices passes; discovery churn;
//                    BroadcastServices tick (services_state.go:525-574) + TrackNewServices; the
//                    BroadcastTombstones tick lists the views whose expiry scan can change anything
//   1   k_scan       TombstoneOthersServices full-view expiry scan (services_state.go:635-683) over
//                    that worklist: one 256-thread block streams one 4 MB view row, ordered compaction
//   1   k_bt_finish  TombstoneServices + SendServices(TOMBSTONE_COUNT) or nil (services_state.go:606-633);
//                    folded into k_send unless another phase queues jobs in between (storm, detector)
//   2   k_storm      NotifyLeave -> ExpireServer for every host of the other half (services_state.go:150-192)
//   3   k_send       peer sampling + GetBroadcasts/packPacket per peer (services_delegate.go:85-144,186-223);
//                    each packet is registered in its receiver's inbox with one atomic
//   4   k_merge      gather-then-merge: one wave per receiver sorts its inbox by sender key, takes its
//                    inbound records straight from the packets, folds duplicates of a key in arrival
//                    order with the AddServiceEntry rule (services_state.go:293-347), writes each
//                    touched slot once, and compacts accepted foreign records into the receiver's
//                    broadcast FIFO with a wave ballot
//   5   k_ae         anti-entropy push-pull: one 256-thread block per host pair streams both views
//                    and merges each into the other (services_delegate.go:153-167, Merge :367-373)
//   end k_watch      only while a record watch is armed (gx_watch.h): per watched record, the views
//                    that hold its version and those that hold an older one, into the round's log row
// No MFMA: the work is int64 compare/select over HBM-resident views (memory-bound).
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <deque>
#include <numeric>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>


#define HIPCHK(x)                                                                          \
  do {                                                                                     \
    hipError_t _e = (x);                                                                   \
    if (_e != hipSuccess) {                                                                \
      fprintf(stderr, "gx: HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); \
      return GX_EIO;                                                                       \
    }                                                                                      \
  } while (0)
// a step's GX_* result: anything but GX_OK is returned at once
#define GXTRY(x)         \
  do {                   \
    int rc_ = (x);       \
    if (rc_) return rc_; \
  } while (0)

static uint32_t pow2_at_least(uint32_t x) {
  uint32_t v = 1;
  while (v < x) v <<= 1;
  return v;
}

#include "../../include/gx_watch.h"
#include "../../include/gx_ckpt.h"
#include "gx_kernels.hpp"
#include "gx_fd.hpp"
#include "gx_codec.hpp"

// ================================================================================ host ==
struct TimedLaunch {
  int cls;
  hipEvent_t a, b;
};

// Device allocations that share one lifetime (an engine's, the codec's name tables, one call's
// temporaries): every take() is freed by release(), at the latest when the owner goes.
struct DevMem {
  // id: the buffer's checkpoint section (gx_ckpt.h GX_CK_*: class STATE, saved), 0 = class DERIVED
  // (not saved: some kernel rewrites it before anything reads it) or not an engine buffer at all
  struct Buf {
    void *p;
    size_t bytes;
    uint32_t id;
  };
  std::vector<Buf> bufs;
  DevMem() = default;
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  ~DevMem() { release(); }
  template <class T>
  int take(uint32_t id, T *&p, size_t bytes) {
    void *q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return GX_ENOMEM;
    }
    bufs.push_back({q, bytes, id});
    p = (T *)q;
    return GX_OK;
  }
  // ... with every byte set to `fill` on stream s, so before whatever s runs next (a hipMemset on the
  // null stream is ordered with neither the host nor a non-blocking stream)
  template <class T>
  int take(uint32_t id, T *&p, size_t bytes, int fill, hipStream_t s) {
    GXTRY(take(id, p, bytes));
    if (bytes) HIPCHK(hipMemsetAsync(p, fill, bytes, s));
    return GX_OK;
  }
  template <class T>
  int take(T *&p, size_t bytes) {
    return take(0u, p, bytes);
  }
  template <class T>
  int take(T *&p, size_t bytes, int fill, hipStream_t s) {
    return take(0u, p, bytes, fill, s);
  }
  // one buffer (or none: p == nullptr) ahead of the rest
  template <class T>
  void drop(T *&p) {
    bufs.erase(std::remove_if(bufs.begin(), bufs.end(), [&](const Buf &b) { return b.p == (void *)p; }), bufs.end());
    (void)hipFree(p);
    p = nullptr;
  }
  const Buf *find(uint32_t id) const {
    for (const Buf &b : bufs)
      if (b.id == id) return &b;
    return nullptr;
  }
  void release() {
    for (const Buf &b : bufs) (void)hipFree(b.p);
    bufs.clear();
  }
};

// grow-only device buffer (a power of two >= min_cap bytes)
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  ~DevBuf() { (void)hipFree(p); }
};
static int dbuf(DevBuf &b, size_t bytes, void **out, size_t min_cap = 1 << 16) {
  if (bytes > b.cap) {
    (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    size_t c = min_cap;
    while (c < bytes) c <<= 1;
    if (hipMalloc(&b.p, c) != hipSuccess) {
      (void)hipGetLastError();
      return GX_ENOMEM;
    }
    b.cap = c;
  }
  *out = b.p;
  return GX_OK;
}

// Quiet-round bounds asked for and not stored yet, one every second round: with all of them
// outstanding the host is 8 rounds ahead of the device and lets it catch up (quiet_probe). 8 rounds
// are 250 us of queued work at cfg 5; the shortest quiet stretches of the test schedules are 10.
#define GX_QUIET_SLOTS 4

// The calls of a sharded engine's push-pull chain that later calls of the same step build on
// (gx_engine::AeChain::done): gx_ae_bytes, gx_ae_merge_local, gx_ae_delta_bytes, gx_ae_return_bytes,
// gx_ae_claim_set.
enum AeCall : uint32_t { AE_PLANNED = 1, AE_LOCAL = 2, AE_DELTA = 4, AE_RET = 8, AE_CLAIM = 16 };

struct gx_engine {
  Dev d{};
  DevMem mem;  // every device buffer that lives as long as the engine
  hipStream_t stream;      // where all device work goes (own_stream, or the caller's: gx_set_stream)
  hipStream_t own_stream;
  // shard-local push-pull pairs run on side_stream, between side_start (recorded on `stream` after
  // the rows are packed) and side_done (joined back into `stream` before anything reads them)
  hipStream_t side_stream;
  hipEvent_t side_start, side_done;
  bool side_pending;
  // a round is open: gx_round_send / gx_round_gossip_begin ran and gx_round_end has not (gx_ckpt.h:
  // gx_ckpt_save is refused until it has)
  bool round_open;
  // Where a round's expiry scans run (round_send_impl): in k_send's prologue (one launch with the
  // owner ticks and the sends; a block streams its own listed views, fine while almost no view
  // needs a scan) or, while views do get scanned, in k_owner + k_scan + k_send, where k_scan
  // streams the listed rows with the whole chip. Decided from the device's count of scanned views
  // (work_cnt[GX_WC_SCANS]) read back without stalling the device: a snapshot is copied to pinned
  // memory every second round and consumed two snapshots later (scan_probe_begin). Both placements give
  // the same results; only the time differs.
  bool scan_heavy = true;  // k_scan placement until the first snapshots say no view gets scanned
  uint64_t *scan_snap;      // [2 + GX_QUIET_SLOTS] pinned host copies of (tag << 32 | a work_cnt word), written by
                            // k_send: [0..1] work_cnt[GX_WC_SCANS] tagged with the round, then quiet-round
                            // bounds (quiet_probe)
  uint64_t *scan_snap_dev;  // the same memory as the device addresses it
  uint32_t scan_tag[2] = {~0u, ~0u};  // the round each slot's snapshot was asked for
  uint32_t scan_k, scan_last;
  // Quiet rounds (quiet_round): every round from now until quiet_until is quiet, by the
  // bounds the device has reported through scan_snap[2..]. quiet_tag: the snapshot each slot was asked
  // for and has not shown yet (0 = none; tags are never reused, so a snapshot from before an
  // invalidation is ignored); quiet_from: no bound folded before this round counts
  // (quiet_invalidate); quiet_now: this round takes the quiet path.
  uint32_t quiet_tag[GX_QUIET_SLOTS], quiet_seq;
  bool quiet_nowait;  // a bound took too long in this gx_run_rounds call: no more polling in it
  int64_t quiet_until, quiet_from;
  bool quiet_now;
  bool quiet_send = true;  // quiet rounds launch k_send's lean instance (env GX_QUIET_SEND=0: the generic one, for A/B runs)
  uint32_t quiet_batch;    // quiet rounds one launch of it runs at the most (quiet_batch_len; env GX_QUIET_BATCH, 1: a launch per round)
  uint32_t *in_cnt_buf;     // [2][Hl] inbox counts by round parity (Dev::in_cnt, in_cnt_nx)
  int async_phases;         // sharded phase calls return without waiting (gx_set_stream)
  int device;
  int timing;
  std::vector<TimedLaunch> pending_ev;
  // GX_PP_INITIATE, the schedule of round pp_round (pp_schedule): the exchanges batch by batch
  // (pp_host: the n initiators, then the n partners), each one's index in initiator order, batch q =
  // [pp_off[q], pp_off[q + 1]); a sharded engine runs the batch at pp_cursor (gx_ae_bytes .. gx_ae_merge)
  std::vector<uint32_t> pp_host, pp_idx, pp_off;
  int64_t pp_round = -1;
  uint32_t pp_cursor;
  uint32_t *pp_dev;
  int32_t *pp_prow;               // all -1: every exchange is local
  uint32_t *name_rank;            // [R] ByService: rank of each record's Service.Name (gx_set_service_names)
  double ms[GX_K_COUNT];
  uint64_t launches[GX_K_COUNT];
  uint64_t host_bytes[GX_K_COUNT], host_units[GX_K_COUNT];  // codec classes (gx_codec_host.hpp)
  struct CodecState *codec;
  // sharded rounds: outbox entry list and push-pull plan (device), rebuilt per round
  uint32_t *ob_entries;
  uint32_t *ob_counts;  // [G] packets per destination shard, then [chunks][G] counts and offsets
  uint32_t n_ob;
  bool ob_async;        // the outbox slot count is on the device only (gx_outbox_sizes_async)
  uint32_t *ob_total;   // [1] that count
  uint32_t *ae_pa, *ae_pb, *ae_pack_host, *ae_pack_t, *ae_pack_other;
  uint8_t *ae_pack_first, *ae_skip;  // this side is the pair's initiator; the pair does not run
  uint64_t *fd_rsnap;                // [pairs][H] partner member lists received with the digests
  int32_t *ae_prow;
  uint8_t *ae_pcount;
  // push-pull digests / delta (per cross pair k, in pack order = receive order)
  uint32_t nblk, nmw;
  ulonglong2 *ae_dig;  // [Hl][nblk] own digests
  uint32_t *ae_mask;   // [Hl][nmw] differing blocks this side leads
  uint32_t *ae_fmask;  // [Hl][nmw] differing blocks the partner leads
  uint16_t *ae_lt;     // [Hl][nblk] the partner's literal counts (its digests)
  uint16_t *ae_retL;   // [Hl][nblk] literal counts of this side's return blocks (follow order)
  uint32_t *ae_bcnt;   // [Hl][nblk] own blocks: present | stale << 16 (digest pass)
  uint32_t *ae_cnt;    // [Hl] blocks this side leads
  uint32_t *ae_nfol;   // [Hl] blocks the partner leads
  uint64_t *ae_sz;     // [4][Hl] lead message size, partner's lead size, return size, scratch
  uint64_t *ae_off;    // [4][Hl] lead offsets, lead inbox offsets, return offsets, return table entries
  uint64_t *ae_rioff;  // [Hl] return inbox offsets
  uint32_t *ae_err;
  // gx.h lock_readers on a sharded engine: each cross pair's read-locked verdict (k_ae_mask<true>) and
  // the driver's counters (gx_ae_ro_counts)
  uint8_t *ae_rov;             // [pairs] 1: this side is read-locked | 2: the partner is; 0: another verdict
  unsigned long long *ro_xc;   // [3]
  // The push-pull chain's host state (gx_ae_chain_host.hpp), all of one step (ae_step: the round, in
  // GX_PP_INITIATE the batch too): what gx_ae_bytes planned, the sizes the later calls check their
  // buffers against, and which calls have completed for the step (AeCall bits; ae_done, ae_mark).
  struct AeChain {
    int64_t step = -1;
    uint32_t done;
    uint32_t n_plan, n_pack;  // planned pairs (ae_pa, ae_pb): the n_pack cross pairs in pack order, then the local ones
    std::vector<uint32_t> gstart;          // pack index range per destination shard
    std::vector<uint64_t> lead_off;        // [2][n_pack] lead message offsets, out and in the inbox (ae_off's first half)
    uint64_t lead_total, lead_in_total, ret_total;  // bytes of the lead messages out, of those in, of the return out
  } chain;
  // listeners: host-side channels fed from the per-view device event logs
  struct Listener {
    uint32_t view, id, cap;
    std::deque<gx_change_event> ring;
  };
  std::vector<Listener> listeners;
  std::vector<uint32_t> log_views;  // view of each device event log
  uint64_t listener_drops;
  // small device scratch for single-host ABI calls
  DevBuf api;
  unsigned long long *conv_bad;
  uint64_t *digest_buf;
  size_t kprof_n;  // diagnostics: u64 marks in d.kprof (env GX_KPROF)
  // planned gossip exchange (gx_exchange_plan): slot bounds of XPLAN_BATCH rounds computed ahead on
  // xplan_stream into pinned host memory, two batches (the current one and the next)
  hipStream_t xplan_stream;
  uint32_t *xplan_dev;           // [2][XPLAN_BATCH][G][G] (k_send of a packing round reads its row)
  uint32_t *xplan_host;          // [2][XPLAN_BATCH][G][G] pinned
  int64_t xplan_start[2] = {-1, -1};
  uint64_t xplan_waits[2];       // diagnostics: calls whose batch was not ready yet (a host wait) / all calls
  hipEvent_t xplan_ev[2];
  hipEvent_t xplan_join;         // a batch is rewritten after the rounds queued before it (xplan_launch)
  int64_t xbound_round = -1;     // the round xbound holds
  XBound xbound;                 // this shard's slots per destination this round
  const uint32_t *xbound_dev;    // the same row on the device
  uint32_t *ob_claim;            // Dev::ob_claim (gx_round_gossip_begin packing in k_send)
  // the worklist expiry scan's row split (k_scan_split / k_scan_join): chunks per row, chunk length,
  // each chunk's first L expirations and its result
  uint32_t scan_nch;
  grec *scan_tmp;
  ScanChunk *scan_chunk;
  // the record watch (gx_watch.h, gx_watch_host.hpp): armed while n != 0; its buffers are in `mem`
  struct Watch {
    uint32_t n, log_rounds;
    int64_t first_round;  // the round of log row 0
    uint64_t missed;      // rounds that ended past the log's last row
    uint32_t *keys;       // [n] record keys, GX_WATCH_OFF = entry off
    uint64_t *thr;        // [n] thresholds as packed words of status 0 (k_watch)
    uint32_t *log;        // [log_rounds][n + 1] {holds, older} per entry, then {live, 0}
    std::vector<uint32_t> keys_host;  // the entries as last set: gx_watch_set stages its copies from here
    std::vector<uint64_t> thr_host;
  } watch;
};

static void codec_free(gx_engine *e);  // gx_codec_host.hpp

static int ensure_api(gx_engine *e, size_t bytes) {
  void *p;
  return dbuf(e->api, bytes, &p, 1 << 20);
}

static bool own(const gx_engine *e, uint32_t v) { return v >= e->d.lo && v < e->d.lo + e->d.Hl; }
// The two runtime flags that kernel variants are built for, each read here only:
// VEC, an even row length (view rows stream as 16-B pairs of slots)
static bool vec_of(const gx_engine *e) { return e->d.R % 2 == 0; }
// EV, some view has a listener (the ChangeEvent variants)
static bool ev_of(const gx_engine *e) { return !e->log_views.empty(); }
// push-pull also merges memberlist state (mergeState)
static bool pp_state(const Dev &d) { return d.p.fd_enable && d.p.fd_push_pull_state; }
static int64_t now_of(const gx_engine *e) { return e->d.p.t0_ns + e->d.round * e->d.p.round_ns; }
// slot time -> absolute for server times and state.LastChanged: 0 = never set (time.Unix(0, 0),
// services_state.go:62-63,95)
static int64_t abs_tm(const gx_engine *e, int64_t t) { return t ? t + e->d.epoch : 0; }
static void set_round_fields(gx_engine *e) {
  Dev &d = e->d;
  const uint32_t par = (uint32_t)(d.round & 1);
  d.in_cnt = e->in_cnt_buf + (size_t)par * d.Hl;
  d.in_cnt_nx = e->in_cnt_buf + (size_t)(par ^ 1u) * d.Hl;
  d.wl_cnt = d.work_cnt + par;
  d.wl_cnt_nx = d.work_cnt + (par ^ 1u);
  d.ovf_cnt = d.work_cnt + 2 + par;
  d.ovf_cnt_nx = d.work_cnt + 2 + (par ^ 1u);
  e->d.now = now_of(e);
  e->d.partitioned = e->d.round >= e->d.p.partition_start && e->d.round < e->d.p.partition_end;
  e->d.pair_split = e->d.partitioned && !e->d.p.fd_enable;
}

struct LaunchTimer {
  gx_engine *e;
  int cls;
  hipEvent_t a, b;
  hipStream_t st;
  LaunchTimer(gx_engine *e_, int cls_, hipStream_t s_ = nullptr) : e(e_), cls(cls_), a(nullptr), b(nullptr), st(s_ ? s_ : e_->stream) {
    e->launches[cls]++;
    if (e->timing) {
      (void)hipEventCreate(&a);
      (void)hipEventCreate(&b);
      (void)hipEventRecord(a, st);
    }
  }
  ~LaunchTimer() {
    if (e->timing) {
      (void)hipEventRecord(b, st);
      e->pending_ev.push_back({cls, a, b});
    }
  }
};

static int drain_timing(gx_engine *e) {
  if (e->pending_ev.empty()) return GX_OK;
  HIPCHK(hipStreamSynchronize(e->stream));
  for (auto &t : e->pending_ev) {
    float ms = 0;
    (void)hipEventElapsedTime(&ms, t.a, t.b);
    e->ms[t.cls] += ms;
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  e->pending_ev.clear();
  return GX_OK;
}

// Deliver the device event logs into the listeners' channels (non-blocking sends: a full
// channel drops the event, services_state.go:230-236) and reset the logs. Channels are drained
// only between ABI calls, so each listener receives a prefix of its view's events.
static int deliver_events(gx_engine *e) {
  size_t nlog = e->log_views.size();
  if (!nlog) return GX_OK;
  std::vector<uint32_t> cnt(nlog);
  HIPCHK(hipMemcpy(cnt.data(), e->d.ev_cnt, sizeof(uint32_t) * nlog, hipMemcpyDeviceToHost));
  bool any = false;
  for (uint32_t c : cnt) any |= c != 0;
  if (!any) return GX_OK;
  for (size_t k = 0; k < nlog; k++) {
    if (!cnt[k]) continue;
    uint32_t n = cnt[k] < e->d.ev_cap ? cnt[k] : e->d.ev_cap;
    std::vector<gx_change_event> ev(n);
    HIPCHK(hipMemcpy(ev.data(), &e->d.ev_log[k * e->d.ev_cap], sizeof(gx_change_event) * n, hipMemcpyDeviceToHost));
    for (auto &x : ev) {
      x.service.updated_ns += e->d.epoch;
      x.time_ns = abs_tm(e, x.time_ns);
    }
    for (auto &l : e->listeners) {
      if (l.view != e->log_views[k]) continue;
      uint32_t room = l.cap - (uint32_t)l.ring.size();
      uint32_t take = cnt[k] < room ? cnt[k] : room;  // take <= n: ev_cap >= every capacity
      for (uint32_t i = 0; i < take; i++) l.ring.push_back(ev[i]);
      e->listener_drops += cnt[k] - take;
    }
  }
  HIPCHK(hipMemset(e->d.ev_cnt, 0, sizeof(uint32_t) * nlog));
  return GX_OK;
}

// A received packet slot that failed validation (k_inbox_unpack: the oracle's gx_inbox_unpack
// checks) was skipped on the device; the next call that waits reports it, once.
static int take_device_error(gx_engine *e) {
  if (e->d.G < 2) return GX_OK;
  uint32_t err = 0;
  HIPCHK(hipMemcpy(&err, &e->d.work_cnt[GX_WC_ERR], sizeof(err), hipMemcpyDeviceToHost));
  if (!err) return GX_OK;
  HIPCHK(hipMemset(&e->d.work_cnt[GX_WC_ERR], 0, sizeof(err)));
  return GX_EINVAL;
}

// The shard-local push-pull merges rejoin the engine's stream (gx_ae_merge_local).
static int join_side(gx_engine *e) {
  if (!e->side_pending) return GX_OK;
  HIPCHK(hipStreamWaitEvent(e->stream, e->side_done, 0));
  e->side_pending = false;
  return GX_OK;
}

// The push-pull exchange stages read sizes back without waiting for the shard-local merges on
// side_stream (they touch rows no exchange stage reads); gx_ae_merge / gx_round_end join them.
static int sync_main(gx_engine *e) {
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  return take_device_error(e);
}

static int sync_check(gx_engine *e) {
  int jr = join_side(e);
  if (jr) return jr;
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipGetLastError());
  int rc = take_device_error(e);
  if (rc) return rc;
  return ev_of(e) ? deliver_events(e) : GX_OK;
}

// One scalar result of an ABI call's kernel: copied back on the engine's stream, then sync_check.
template <class T>
static int read_back(gx_engine *e, const void *dev, T *host) {
  HIPCHK(hipMemcpyAsync(host, dev, sizeof(T), hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

// End of a sharded phase call: with async phases (and no listeners to feed) the caller's stream
// orders the next step, so only launch errors are checked here.
static int phase_done(gx_engine *e) {
  if (e->async_phases && !ev_of(e)) {
    HIPCHK(hipGetLastError());
    return GX_OK;
  }
  return sync_check(e);
}

static inline unsigned nblk(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// Runtime flags -> template arguments: f is a generic lambda that gets one std::integral_constant
// per flag and names its kernel with them, k_scan<V(), E()><<<...>>>(...). Every combination is
// instantiated, so these serve only where all of them are built anyway; a subset stays an if.
template <class F>
static void with_flag(bool a, F &&f) {
  if (a) f(std::true_type{});
  else f(std::false_type{});
}
template <class F>
static void with_flags(bool a, bool b, F &&f) {
  with_flag(a, [&](auto A) { with_flag(b, [&](auto B) { f(A, B); }); });
}
// k_send's OWN: services per lane of the 4-lane owner teams, 0 = the owner ticks are not in k_send
static int own_class(uint32_t S) { return S <= 4 ? 1 : S <= 8 ? 2 : 4; }
template <class F>
static void with_own(int own, F &&f) {
  if (own == 0) f(std::integral_constant<int, 0>{});
  else if (own == 1) f(std::integral_constant<int, 1>{});
  else if (own == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 4>{});
}

// d.in_round for the launches of a round phase: ExpireServer waits for a held lock (gx.h lock_model)
struct InRound {
  Dev &d;
  explicit InRound(Dev &d_) : d(d_) { d.in_round = 1; }
  ~InRound() { d.in_round = 0; }
};

// k_owner with a team of T >= S lanes per host (lane s = service s)
template <int T>
static void launch_owner(const Dev &d, hipStream_t s) {
  k_owner<T><<<nblk(d.Hl, 256 / T), 256, 0, s>>>(d);  // 64- and 128-thread blocks measured 13.6 / 12.6 vs 12.5 us
}
// teams of the smallest power of two >= S (16 -> 32 -> 64 lanes measured 12.3 / 17.4 / 29.2 us at cfg 5)
static void owner_launch(const Dev &d, hipStream_t s) {
  if (d.S <= 1) launch_owner<1>(d, s);
  else if (d.S <= 2) launch_owner<2>(d, s);
  else if (d.S <= 4) launch_owner<4>(d, s);
  else if (d.S <= 8) launch_owner<8>(d, s);
  else if (d.S <= 16) launch_owner<16>(d, s);
  else if (d.S <= 32) launch_owner<32>(d, s);
  else launch_owner<64>(d, s);
}
#define SCAN_GRID 2048  // worklist blocks: every listed row of a round streams at once, a quick exit when none do

// Every second round: takes the scanned-view count of the snapshot two probes back, if the device
// has written it by now (the slot carries the round it was asked for; nothing waits for it: with the
// device further behind, the last decision stands), and has this round's k_send store a new one
// (Dev::snap, one 8-B store to pinned host memory, no event in the stream). A view scanned between
// the two consumed snapshots selects the k_scan placement.
static int scan_probe_begin(gx_engine *e) {
  e->d.snap = nullptr;
  if (e->d.round % 2) return GX_OK;
  e->d.snap_tag = (uint32_t)e->d.round;
  e->d.snap_word = GX_WC_SCANS;
  const uint32_t i = e->scan_k & 1u;
  if (e->scan_k >= 2) {
    const uint64_t v = __atomic_load_n(&e->scan_snap[i], __ATOMIC_ACQUIRE);
    if ((uint32_t)(v >> 32) == e->scan_tag[i]) {
      e->scan_heavy = (uint32_t)v != e->scan_last;
      e->scan_last = (uint32_t)v;
    }
  }
  e->scan_tag[i] = (uint32_t)e->d.round;
  e->d.snap = &e->scan_snap_dev[i];
  return GX_OK;
}
static int scan_probe_end(gx_engine *e) {
  if (!e->d.snap) return GX_OK;
  if (e->d.snap < &e->scan_snap_dev[2]) e->scan_k++;  // (not quiet_probe's)
  e->d.snap = nullptr;
  return GX_OK;
}

// The parameters under which quiet rounds are predicted (quiet_term's argument): one engine, the lock
// modelled without read-locked exchanges, no detector, departures or shared handoff queue, one
// GetBroadcasts call per target and none outside k_send (probe_piggyback), planned sends (they count
// a full pipeline's drops at plan time and register nothing).
static bool quiet_params(const Dev &d) {
  return d.G == 1 && d.K && d.p.lock_model == 1 && !d.p.lock_readers && !d.p.fd_enable && !d.departures &&
         !d.p.fd_handoff_shared && d.NG == 1 && !d.p.probe_piggyback && !d.p.limit_bytes && d.p.retransmit_rounds > 0;
}
// The bounds the device has stored by now (scan_snap[2..], each tagged as asked); returns a free
// slot or -1.
static int quiet_take(gx_engine *e) {
  int free_slot = -1;
  for (int i = GX_QUIET_SLOTS - 1; i >= 0; i--) {
    if (e->quiet_tag[i]) {
      const uint64_t v = __atomic_load_n(&e->scan_snap[2 + i], __ATOMIC_ACQUIRE);
      if ((uint32_t)(v >> 32) != e->quiet_tag[i]) continue;
      e->quiet_tag[i] = 0;
      if ((int64_t)(uint32_t)v > e->quiet_until) e->quiet_until = (int64_t)(uint32_t)v;
    }
    free_slot = i;
  }
  return free_slot;
}
// The other rounds (after scan_probe_begin left Dev::snap free): takes the bounds asked for earlier
// that the device has stored by now, and asks this round's k_send for the bound the last round's
// k_send finished (the minimum of its waves' terms, Dev::quiet_w; valid from this round on).
// The host's lead is bounded here: a bound helps only while it reaches past the round the host is
// queueing, and left alone the host queues a whole gx_run_rounds call before the device has run its
// first rounds (measured: no round of a 150-round call took the quiet path). With every slot
// outstanding the host is 2 * GX_QUIET_SLOTS rounds ahead, and it polls the slots until the oldest
// bound arrives. gx_run_rounds returns only when the device is done, so the call takes no longer
// while those rounds keep the device's queue filled. A bound that takes more than GX_QUIET_WAIT_MS
// (a stuck device, a kernel of seconds) ends the polling for the rest of the call (quiet_nowait): a
// late or missing bound only means the generic path.
#define GX_QUIET_WAIT_MS 1000
static void quiet_probe(gx_engine *e) {
  Dev &d = e->d;
  int free_slot = quiet_take(e);
  if (d.snap || d.round <= e->quiet_from) return;
  if (free_slot < 0 && !e->quiet_nowait) {
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(GX_QUIET_WAIT_MS);
    while ((free_slot = quiet_take(e)) < 0) {
      if (std::chrono::steady_clock::now() > deadline) {
        e->quiet_nowait = true;
        break;
      }
      std::this_thread::yield();
    }
  }
  if (free_slot < 0) return;
  if (!++e->quiet_seq) ++e->quiet_seq;
  e->quiet_tag[free_slot] = e->quiet_seq;
  d.snap = &e->scan_snap_dev[2 + free_slot];
  d.snap_tag = e->quiet_seq;
  d.snap_word = GX_SNAP_QUIET;
}
// What the device reported, or still reports, about rounds before now no longer counts. Called by
// enter() alone, for every entry that states it changes the engine.
static void quiet_invalidate(gx_engine *e) {
  memset(e->quiet_tag, 0, sizeof(e->quiet_tag));
  e->quiet_until = 0;
  e->quiet_from = e->d.round;  // the round that runs next folds the first bound that counts
}

// What an ABI entry does to the engine, stated once, where the entry calls enter(). By what the
// entry does, not by whether quiet rounds can occur in the configurations that accept it:
// invalidating an engine that never predicts quiet rounds (quiet_params) changes nothing.
enum Entry {
  ENTRY_READ,    // leaves everything a round reads as it is (copies out, computes into scratch, sets
                 // ByService's name ranks): the quiet-round bounds stand
  ENTRY_MUTATE,  // changes catalog, queue, memberlist, listener or stream state between rounds, or
                 // the record watch's entries (gx_watch_arm, gx_watch_set)
  ENTRY_PHASE,   // one piece of a round the caller drives itself (gx_round_*, gx_outbox_*, gx_ae_*)
  ENTRY_ROUNDS,  // gx_run_rounds alone: the one entry that runs rounds and keeps the bounds, which
                 // describe exactly the rounds it runs
};
// The preamble of every ABI entry that touches the device, after the entry's own argument checks
// (a bad argument is GX_EINVAL before any HIP call): the engine's device is current, a mutating or
// phase entry has dropped the quiet-round bounds, and Dev's per-round fields are those of d.round
// for whatever the entry launches (an entry that moves d.round itself sets them again).
static int enter(gx_engine *e, Entry what) {
  HIPCHK(hipSetDevice(e->device));
  if (what == ENTRY_MUTATE || what == ENTRY_PHASE) quiet_invalidate(e);
  set_round_fields(e);
  return GX_OK;
}
// Whether round d.round skips its receive phase (run_one_round) and its push-pull pairs
// (ae_whole_impl): a bound reported by the device covers it. The storm's round and rounds with a
// listener stay on the generic path (no test covers them quiet; nothing to gain there).
static bool quiet_round(const gx_engine *e, bool storm) {
  return quiet_params(e->d) && !storm && e->log_views.empty() && e->d.round < e->quiet_until;
}

// k_send's variant. X: departures or the detector; SCAN: the round's expiry scans run in k_send's
// prologue; own: own_class(S) when the owner ticks run there too, else 0; PLAN: send_planned;
// quiet: the round is quiet (quiet_round, which implies plan, no x and no listener) and takes the
// lean instance (QUIET) unless the engine was created with GX_QUIET_SEND=0.
struct SendSel {
  bool x, scan, plan;
  int own;
  bool quiet;
};
// The whole table of k_send variants: (X, PLAN) without both at once; with SCAN, VEC x EV x OWN; without
// it one variant each; and QUIET beside every PLAN variant without EV: with SCAN, VEC x OWN, without
// it one (k_send's static_asserts state the same). Lean and generic instance give identical results.
// 4 lanes per host: measured best of 1/4/8/16/64 (profiles/send_team.sh);
// teams of 2 / 8 lanes measured 25.6 / 28.7 vs 21.1 us (profiles/r02/gossip/send_team_ab.log)
// nr: the quiet rounds the launch runs (a batch, run_quiet_batch); only the lean instance takes more than 1.
static void launch_send(gx_engine *e, SendSel sel, int do_bt, int nr) {
  const Dev &d = e->d;
  const unsigned g = nblk(d.Hl, 64);
  hipStream_t s = e->stream;
  if (sel.quiet && sel.plan && !ev_of(e)) {
    if (!sel.scan) {
      k_send<4, false, false, false, false, 0, true, true><<<g, 256, 0, s>>>(d, do_bt, nr);
      return;
    }
    with_flag(vec_of(e), [&](auto V) {
      with_own(sel.own, [&](auto O) { k_send<4, false, true, V(), false, O(), true, true><<<g, 256, 0, s>>>(d, do_bt, nr); });
    });
    return;
  }
  auto rest = [&](auto X, auto P) {
    if (!sel.scan) {
      k_send<4, X(), false, false, false, 0, P()><<<g, 256, 0, s>>>(d, do_bt, 1);
      return;
    }
    with_flags(vec_of(e), ev_of(e), [&](auto V, auto E) {
      with_own(sel.own, [&](auto O) { k_send<4, X(), true, V(), E(), O(), P()><<<g, 256, 0, s>>>(d, do_bt, 1); });
    });
  };
  if (sel.plan) rest(std::false_type{}, std::true_type{});
  else with_flag(sel.x, [&](auto X) { rest(X, std::false_type{}); });
}

// Phases 0-3 (wake, owners, expiry scan, storm, GetBroadcasts) for this engine's hosts.
// nr > 1: the quiet rounds [d.round, d.round + nr) in these launches (run_quiet_batch, which has checked
// them): the owner, scan and send launches of the first, whose k_send runs the others' ticks and
// sends itself. Such a launch carries no snapshot: no view is scanned in those rounds, and the bound
// it would report is read from the half of Dev::quiet_w that its own last round rewrites when nr is even.
static int round_send_impl(gx_engine *e, int nr = 1) {
  Dev &d = e->d;
  set_round_fields(e);
  InRound in_round_guard(d);
  if (nr > 1) {
    d.snap = nullptr;
    quiet_take(e);
  } else {
    int rc = scan_probe_begin(e);
    if (rc) return rc;
    if (quiet_params(d)) quiet_probe(e);
  }
  d.n_remote = 0;
  hipStream_t s = e->stream;
  if (d.p.probe_piggyback) {  // the probe ping and ack calls come before the owner phase (gx.h)
    LaunchTimer t(e, GX_K_SEND);
    // phase 0 first: inside a gx_run_rounds call the due sleepers re-enter the FIFOs in the owner
    // tick (the oracle's ph_wake opens the round), which runs after these calls
    k_wake<<<nblk(d.Hl, 64), 64, 0, s>>>(d);
    k_probe<4><<<nblk(d.Hl, 64), 256, 0, s>>>(d);
  }
  const bool vec = vec_of(e), ev = ev_of(e);
  const bool storm = d.p.storm_round >= 0 && d.round == d.p.storm_round && d.H >= 2;
  // BroadcastTombstones' SendServices is queued before the detector's and the storm's jobs
  const bool bt_apart = d.p.fd_enable || storm;
  // with the tick finished in k_send, the expiry scans run in k_send's prologue (no k_scan launch)
  const bool scan_in_send = !bt_apart && d.K && !e->scan_heavy;
  // a round without the detector or the storm: owner ticks, expiry scans and sends in one launch
  // (S <= 16: owner teams of the send's 4 lanes with up to 4 services each)
  const bool fused = scan_in_send && d.S <= 16;
  // planned GetBroadcasts (send_planned): record budget, no detector or departures, re-armed
  // passes sleep; teams of 4 lanes per host
  const bool plan = !d.p.limit_bytes && d.p.retransmit_rounds > 0 && !d.departures && !d.p.fd_enable;
  e->quiet_now = quiet_round(e, storm);
  const SendSel sel{d.p.fd_enable || d.departures, scan_in_send, plan, fused ? own_class(d.S) : 0,
                    e->quiet_now && e->quiet_send};
  if (!fused) {
    LaunchTimer t(e, GX_K_OWNER);
    owner_launch(d, s);
  }
  if (!scan_in_send) {
    LaunchTimer t(e, GX_K_SCAN);
    const unsigned grid = d.Hl < SCAN_GRID ? d.Hl : SCAN_GRID;
    if (vec && !ev && e->scan_nch > 1) {  // rows split over blocks, then joined per view
      k_scan_split<true><<<SCAN_GRID, 256, GX_SCAN_WAVE ? 4 * sizeof(grec) * d.L : 0, s>>>(d, e->scan_tmp, e->scan_chunk,
                                                                                         e->scan_nch);
      k_scan_join<<<grid, 256, 0, s>>>(d, e->scan_tmp, e->scan_chunk, e->scan_nch);
    } else {
      with_flags(vec, ev, [&](auto V, auto E) {
        k_scan<V(), E()><<<grid, 256, 0, s>>>(d, d.scan_list, d.L, d.L, d.scan_cnt, -1);
      });
    }
    if (bt_apart) k_bt_finish<<<nblk(d.Hl, 256), 256, 0, s>>>(d);
  }
  if (d.p.fd_enable) {  // suspicion timers -> deadNode -> NotifyLeave; probe ticks
    LaunchTimer t(e, GX_K_FD);
    k_fd_tick<<<d.Hl, 64, 0, s>>>(d);
  }
  if (storm) {
    LaunchTimer t(e, GX_K_STORM);
    // nontemporal row stream: 30.3 -> 27.9 ms at cfg 5 (profiles/ab/storm_nt_ab_r02.log)
    with_flag(ev, [&](auto E) {
      if (d.S >= 2 && 64 % d.S == 0) k_storm_p2<E(), true><<<d.Hl, 256, 0, s>>>(d);
      else k_storm<E()><<<d.Hl, 256, 0, s>>>(d);
    });
  }
  {
    LaunchTimer t(e, GX_K_SEND);
    if (d.p.fd_enable) k_fd_send<<<nblk(d.Hl, 64), 64, 0, s>>>(d);  // memberlist's targets + messages
    launch_send(e, sel, bt_apart ? 0 : 1, sel.quiet ? nr : 1);
  }
  HIPCHK(hipGetLastError());
  return scan_probe_end(e);
}

#ifndef GX_LOCK_APPEND
#define GX_LOCK_APPEND 1
#endif
// with k_lock_append taking the locked receivers, the merge's 64-receiver blocks are faster again:
// cfg 5 lock on, filling 80.7 -> 77.9 us, full 32.8 -> 30.6 us (profiles/r06/ab/merge_nr64_lapp_cfg5.jsonl)
#ifndef GX_MERGE_LAPP_NR64
#define GX_MERGE_LAPP_NR64 1
#endif
#ifndef GX_LOCK_APPEND_HL
#define GX_LOCK_APPEND_HL 32768
#endif
#ifndef GX_MERGE_SMALL_HL
#define GX_MERGE_SMALL_HL 16384  // 16 receivers per block below this many local hosts: merge 2.0 -> 1.1 ms (cfg 2)
                                 // and 2.4 -> 1.5 ms (cfg 4) over 60 rounds lock off (profiles/r05/ab/merge_nr16_*)
#endif
// k_merge_seg over every receiver: 16 receivers per block at MERGE_WPE_GM waves per SIMD (`small`) or
// the default 64; 32-bit sort keys while R < 2^26 (K32).
static void launch_merge(gx_engine *e, bool small) {
  const Dev &d = e->d;
  const unsigned g = nblk(d.Hl, small ? 16u : (unsigned)MERGE_NR);
  with_flags(d.R < (1u << 26), ev_of(e), [&](auto K32, auto E) {
    if (small) k_merge_seg<K32(), E(), 16, MERGE_WPE_GM><<<g, 64 * MERGE_WAVES, 0, e->stream>>>(d);
    else k_merge_seg<K32(), E()><<<g, 64 * MERGE_WAVES, 0, e->stream>>>(d);
  });
}

// Phase 4: gather-then-merge of every receiver's inbox (local and received packets).
static int round_merge_impl(gx_engine *e) {
  Dev &d = e->d;
  set_round_fields(e);
  InRound in_round_guard(d);
  hipStream_t s = e->stream;
  if (d.p.lock_readers) {  // waiting push-pull merges of hosts unlocked now, before their pipelines
    LaunchTimer t(e, GX_K_AE);
    with_flags(vec_of(e), ev_of(e), [&](auto V, auto E) { k_defer_drain<V(), E()><<<d.P, 256, 0, s>>>(d); });
  }
  if (d.KE) {  // (fanout 0 with probe_piggyback: the pings and acks are the only packets)
    LaunchTimer t(e, GX_K_MERGE);
    // receivers routed by their live records. GossipMessages > 1: inboxes of hundreds of live
    // records, each folded by a whole wave tile by tile, so more waves in flight (16 receivers per
    // block, 4 waves per SIMD: 10% faster than 3 in the GM 15 accepting stretch,
    // profiles/r03/ab/merge_wpe_gm15.jsonl); else 64 receivers per block (3% faster at cfg 5)
    // ... and when 64 receivers per block leave most CUs idle (a shard, a small cluster): a block's
    // waves fold their receivers one item after another, so fewer per block shortens the launch
    // ... and with the lock modelled (round 6): a locked receiver's pipeline append is a short
    // dependent chain, and 64 receivers per block run a wave's four of them one after another; 16 per
    // block spread them over more waves (cfg 5, locked gossip rounds 93.7 -> 87.7 us; lock off the
    // 64-receiver blocks stay 3-5% faster, profiles/r06/ab/merge_nr16_cfg5.jsonl)
    // locked receivers' pipeline appends first, at high occupancy (k_lock_append), where k_merge_seg's
    // item waves would take several passes over the receivers: cfg 5 (32768 receivers) lock-on gossip
    // rounds 88.1 -> 79.8 us, a round whose pipelines are all full 30.0 -> 32.3 us (the launch with
    // nothing to append); at 16384 receivers (cfg 3) the extra launch cost 7.7 us per round, and
    // with GossipMessages 15 most locked inboxes exceed a segment (+4%), so neither takes it
    // (profiles/r06/ab/lock_append_*.jsonl)
    const bool lapp = GX_LOCK_APPEND && d.p.lock_model && !d.p.fd_handoff_shared && d.NG == 1 && d.Hl >= GX_LOCK_APPEND_HL;
    if (lapp) k_lock_append<<<nblk(d.Hl, 16), 256, 0, s>>>(d);
    const bool small = d.NG > 1 || d.Hl < GX_MERGE_SMALL_HL || (d.p.lock_model && !(GX_MERGE_LAPP_NR64 && lapp));
    launch_merge(e, small);
  }
  if (d.p.fd_enable && d.K) {  // the packets' memberlist messages, after the catalog merge
    LaunchTimer t(e, GX_K_FD);
    k_fd_recv<<<nblk(d.Hl, 64), 64, 0, s>>>(d);
  }
  HIPCHK(hipGetLastError());
  return GX_OK;
}

// lock off, cfg 2's window (two push-pull rounds): 0.94 ms as built; two tiles in flight 1.01, plain
// row loads and stores 0.98, two tiles at 3 waves per SIMD 1.08 (profiles/r06/ab/ae_cfg2_variants.jsonl)
#ifndef GX_AE_PF_OFF
#define GX_AE_PF_OFF 1  // lock off: tiles in flight per pair
#endif
#ifndef GX_AE_NT_OFF
#define GX_AE_NT_OFF true  // lock off: nontemporal row loads and stores
#endif
#ifndef GX_AE_PF_LOCK
#define GX_AE_PF_LOCK 1  // 2 tiles in flight spill (92 B scratch): 0.98 vs 0.71 ms at cfg 5 lock on (profiles/r05/ab/ae_pf_lock.jsonl)
#endif
static bool ae_round(const gx_engine *e) {
  const Dev &d = e->d;
  if (d.p.ae_period_rounds && d.p.push_pull_stagger) return true;  // some host's staggered timer, every round
  return d.p.ae_period_rounds && (uint64_t)d.round % d.p.ae_period_rounds == d.p.ae_phase;
}
// gx.h push_pull_stagger: host i's push-pull timer fires in the rounds of its seeded phase
static bool pp_initiates(const Dev &d, uint32_t i) {
  if (!d.p.push_pull_stagger) return true;
  return (uint64_t)d.round % d.p.ae_period_rounds == rng4(d.p.seed, ST_PP_PHASE, i, 0, 0) % d.p.ae_period_rounds;
}
// The round's matching (GX_PP_MATCHING): the hosts [base[i], base[i] + len[i]) of each group (one, or
// the two sides of a pair split) are paired off by a Feistel permutation keyed key0 / key1, n0 pairs
// in group 0 and np in all, as k_ae and k_ae_pairs draw them.
struct AeMatching {
  uint32_t base[2], len[2];
  uint64_t key0, key1;
  uint32_t n0, np;
};
static AeMatching ae_matching(const Dev &d) {
  AeMatching m;
  m.base[0] = 0;
  m.base[1] = d.H / 2;
  m.len[0] = d.pair_split ? d.H / 2 : d.H;
  m.len[1] = d.pair_split ? d.H - d.H / 2 : 0;
  m.key0 = rng4(d.p.seed, ST_AE, (uint64_t)d.round, m.base[0], 0);
  m.key1 = m.len[1] ? rng4(d.p.seed, ST_AE, (uint64_t)d.round, m.base[1], 0) : 0;
  m.n0 = m.len[0] / 2;
  m.np = m.n0 + m.len[1] / 2;
  return m;
}

// GX_PP_INITIATE: every live host starts one exchange with a partner drawn at random on its side;
// the exchanges run in initiator order, in batches of exchanges with no host in common (an exchange
// goes into the batch after the last one holding either of its hosts). The oracle's pp_batches
// computes the same batches (pp_schedule). On an unsharded engine each batch is one k_ae_plan
// launch over its pair list (local pairs: both sides merge the other's pre-exchange row); on a
// sharded one each batch is one run of the push-pull chain over its pairs (ae_plan).
static bool ae_partner(const Dev &d, uint32_t i, uint32_t *out) {
  uint32_t base = 0, m = d.H;
  if (d.partitioned && !d.p.fd_enable) {
    const uint32_t half = d.H / 2;
    base = i < half ? 0 : half;
    m = i < half ? half : d.H - half;
  }
  if (m < 2) return false;
  const uint64_t x = rng4(d.p.seed, ST_AE, (uint64_t)d.round, i, 1);
  const uint32_t idx = unif(x, m - 1), self = i - base;
  *out = base + (idx >= self ? idx + 1 : idx);
  return true;
}
// gx.h lock_readers: the read-locked exchanges of the last push-pull launch: k_ae_claim gives their
// read-locked sides pool slots by the policy's rule, then k_ae_rox runs the pairs in parallel over
// at most as many blocks as the launch itself had
static void ae_ro_launch(gx_engine *e, const uint32_t *pa, const uint32_t *pb, uint64_t key0, uint64_t key1, uint32_t np) {
  const Dev &d = e->d;
  k_ae_claim<<<1, 256, 0, e->stream>>>(d, pa, pb, key0, key1, np);
  with_flags(vec_of(e), ev_of(e), [&](auto V, auto E) {
    k_ae_rox<V(), E()><<<ae_grid(np, 1), 256, 0, e->stream>>>(d, pa, pb, key0, key1);
  });
}
// The planned pairs' exchange: the ChangeEvent variant while some view has a listener, else two
// tiles in flight where the caller asks (pf2), else one.
static void launch_ae_plan(gx_engine *e, bool pf2, unsigned np, hipStream_t st, const uint32_t *pa, const uint32_t *pb,
                           const int32_t *prow, const uint8_t *pcount, const AeIn &in, const uint8_t *skip) {
  const bool ev = ev_of(e);
  with_flag(vec_of(e), [&](auto V) {
    (ev ? k_ae_plan_ev<V()> : pf2 ? k_ae_plan_pf2<V()> : k_ae_plan<V()>)<<<np, 256, 0, st>>>(e->d, pa, pb, prow, pcount, in, skip);
  });
}
// This round's exchanges and batches (the oracle's pp_batches), from (seed, round) alone: every
// shard computes the same schedule. Kept for the round (pp_round); returns the batch count.
static uint32_t pp_schedule(gx_engine *e) {
  Dev &d = e->d;
  if (e->pp_round == d.round) return (uint32_t)e->pp_off.size() - 1;
  set_round_fields(e);  // ae_partner draws inside a partition's side
  const bool dep = d.departures;
  std::vector<uint32_t> last(d.H, 0), bat, ia, ib;
  uint32_t nb = 0;
  for (uint32_t i = 0; i < d.H; i++) {
    uint32_t b;
    if (!pp_initiates(d, i) || (dep && departed_at(d.p, d.round, i)) || !ae_partner(d, i, &b) ||
        (dep && departed_at(d.p, d.round, b)))
      continue;
    const uint32_t k = 1 + std::max(last[i], last[b]);
    last[i] = last[b] = k;
    ia.push_back(i);
    ib.push_back(b);
    bat.push_back(k - 1);
    nb = std::max(nb, k);
  }
  const size_t n = ia.size();
  e->pp_off.assign(nb + 1, 0);
  for (uint32_t x : bat) e->pp_off[x + 1]++;
  for (uint32_t q = 0; q < nb; q++) e->pp_off[q + 1] += e->pp_off[q];
  std::vector<uint32_t> cur(e->pp_off.begin(), e->pp_off.end() - 1);
  e->pp_host.assign(2 * n, 0);
  e->pp_idx.assign(n, 0);
  for (size_t t = 0; t < n; t++) {  // stable: initiator order inside a batch
    const uint32_t at = cur[bat[t]]++;
    e->pp_host[at] = ia[t];
    e->pp_host[n + at] = ib[t];
    e->pp_idx[at] = (uint32_t)t;
  }
  e->pp_round = d.round;
  e->pp_cursor = 0;
  return nb;
}
// A sharded engine's push-pull chain (gx_ae_bytes .. gx_ae_merge) has a step to run: the round's
// matching, or in GX_PP_INITIATE the batch at the cursor (past the last one the calls do nothing,
// as on a round without push-pull) ...
static bool ae_step_due(gx_engine *e) {
  if (e->d.G < 2 || !ae_round(e)) return false;
  if (e->d.p.push_pull_mode != GX_PP_INITIATE) return true;
  const uint32_t nb = pp_schedule(e);
  return e->pp_cursor < nb;
}
// ... and its name for the chain's guards: the round and the batch (a batch count is at most H)
static int64_t ae_step(const gx_engine *e) {
  return e->d.round * (2 * (int64_t)GX_MAX_HOSTS) + (e->d.p.push_pull_mode == GX_PP_INITIATE ? e->pp_cursor : 0);
}
static int ae_initiate(gx_engine *e) {
  Dev &d = e->d;
  const uint32_t nb = pp_schedule(e);
  const size_t n = e->pp_idx.size();
  if (!n) return GX_OK;
  const std::vector<uint32_t> &off = e->pp_off;
  HIPCHK(hipMemcpyAsync(e->pp_dev, e->pp_host.data(), sizeof(uint32_t) * 2 * n, hipMemcpyHostToDevice, e->stream));
  AeIn none;
  memset(&none, 0, sizeof(none));
  LaunchTimer t(e, GX_K_AE);
  for (uint32_t q = 0; q < nb; q++) {
    const uint32_t *pa = e->pp_dev + off[q], *pb = e->pp_dev + n + off[q];
    const unsigned np = off[q + 1] - off[q];
    launch_ae_plan(e, false, np, e->stream, pa, pb, e->pp_prow, nullptr, none, nullptr);
    if (d.p.lock_readers) ae_ro_launch(e, pa, pb, 0, 0, np);  // the batch's read-locked exchanges
  }
  return GX_OK;
}

// Phase 5 on an unsharded engine: pairs derived on device.
static int ae_whole_impl(gx_engine *e, bool quiet) {
  Dev &d = e->d;
  set_round_fields(e);
  hipStream_t s = e->stream;
  if (ae_round(e) && d.p.push_pull_mode == GX_PP_INITIATE) {
    int rc = ae_initiate(e);
    if (rc) return rc;
  } else if (ae_round(e)) {
    const AeMatching m = ae_matching(d);
    const uint32_t np = m.np;
    const uint64_t key0 = m.key0, key1 = m.key1;
    if (np && quiet) {  // every host holds the lock: each pair fails on it, the round is only its counts
      LaunchTimer t(e, GX_K_AE);
      k_ae_locked_note<<<1, 64, 0, s>>>(d, np, 1u);
    } else if (np) {
      LaunchTimer t(e, GX_K_AE);
      // PF = 1: deeper prefetch measured within noise (profiles/ae_variants.sh)
      // the ChangeEvent variant only while some view has a listener
      const bool vec = vec_of(e), ev = ev_of(e);
      // nontemporal row loads and stores: -1% over the bench window (profiles/ab/ae_nt_ab_r02.log)
      // under the lock model chunks of pairs per block (ae_round_pairs): a round whose pairs a lock
      // skips costs one round trip per chunk, not a block per pair
      if (vec && !ev && d.p.lock_model)
        k_ae_chunk<true, GX_AE_PF_LOCK, true, true><<<ae_grid(np, 1), 256, 0, s>>>(d, key0, key1, np);
      else if (vec && !ev) k_ae<true, GX_AE_PF_OFF, GX_AE_NT_OFF, GX_AE_NT_OFF><<<np, 256, 0, s>>>(d, key0, key1);
      else if (vec) k_ae_ev<true><<<np, 256, 0, s>>>(d, key0, key1);
      else if (!ev) k_ae<false><<<np, 256, 0, s>>>(d, key0, key1);
      else k_ae_ev<false><<<np, 256, 0, s>>>(d, key0, key1);
    }
    if (np && pp_state(d)) {  // pushPull's membership half (mergeState), from round-start lists
      LaunchTimer t(e, GX_K_FD);
      k_fd_pushpull_pair<<<np, 128, 0, s>>>(d, key0, key1);  // both directions in lockstep: no snapshot
    }
    if (np && d.p.lock_readers) {  // the read-locked exchanges (after the membership half reads ro_flag)
      LaunchTimer t(e, GX_K_AE);
      ae_ro_launch(e, nullptr, nullptr, key0, key1, np);
    }
  }
  HIPCHK(hipGetLastError());
  return GX_OK;
}

// The one place a round ends (run_one_round, gx_round_end): every phase of round d.round is queued
// on the engine's stream. With a watch armed (gx_watch.h) the round's counts are taken here, from
// the views as those phases leave them, into the round's row of the log; past the last row the round
// is only counted. Without one nothing is launched. Then the round number moves.
#define WATCH_GRID 512  // blocks per entry group: 64 views each at cfg 5, 128 atomics per block
static int watch_round_end(gx_engine *e) {
  gx_engine::Watch &w = e->watch;
  Dev &d = e->d;
  if (w.n) {
    const int64_t k = d.round - w.first_round;
    if (k >= (int64_t)w.log_rounds) {
      w.missed++;
    } else if (d.Hl) {
      LaunchTimer t(e, GX_K_CONVERGE);
      const unsigned gx = std::min(nblk(d.Hl, WATCH_VIEWS), (unsigned)WATCH_GRID);
      k_watch<<<dim3(gx, nblk(w.n, 64)), 256, 0, e->stream>>>(d, w.keys, w.thr, w.n, w.log + 2 * ((size_t)w.n + 1) * (size_t)k);
      HIPCHK(hipGetLastError());
    }
  }
  d.round++;
  return GX_OK;
}

// A quiet round (quiet_round, decided in round_send_impl) has no receive phase: no inbox was written
// and every pipeline is full and stays (k_lock_append and k_merge_seg would find nothing).
static int run_one_round(gx_engine *e) {
  int rc = round_send_impl(e);
  const bool quiet = e->quiet_now;
  e->quiet_now = false;
  if (!rc && !quiet) rc = round_merge_impl(e);
  if (!rc) rc = ae_whole_impl(e, quiet);
  if (!rc) rc = watch_round_end(e);
  return rc;
}

// A batch of quiet rounds: how many rounds from d.round on, `left` at the most, one
// k_send launch may run. Each must be quiet by a bound already taken (quiet_until), none the storm's,
// with no listener and no record watch (its counts are per round); the lean instance must be in use,
// and a push-pull round of GX_PP_INITIATE mode ends the batch before it (its batches launch in quiet
// rounds too, ae_whole_impl). Fewer than 2: the round runs alone (run_one_round).
#ifndef GX_QUIET_BATCH
#define GX_QUIET_BATCH 32
#endif
static uint32_t quiet_batch_len(gx_engine *e, uint32_t left) {
  Dev &d = e->d;
  if (e->quiet_batch < 2 || left < 2 || !e->quiet_send || !quiet_params(d) || !e->log_views.empty() || e->watch.n) return 1;
  quiet_take(e);
  const int64_t r0 = d.round;
  if (r0 >= e->quiet_until) return 1;
  uint32_t n = (uint32_t)std::min<int64_t>({(int64_t)left, (int64_t)e->quiet_batch, e->quiet_until - r0});
  for (uint32_t j = 0; j < n; j++) {
    d.round = r0 + j;
    const bool storm = d.p.storm_round >= 0 && d.round == d.p.storm_round;
    if (storm || (d.p.push_pull_mode == GX_PP_INITIATE && ae_round(e))) n = j;
  }
  d.round = r0;
  return n < 2 ? 1 : n;
}
// Runs it: the first round's launches with the round count, then the push-pull rounds among them,
// which in a quiet round are only their counts (ae_whole_impl): one note with the pairs of all of
// them, at the round of the first (the first locked round it may set), then the round number moves.
static int run_quiet_batch(gx_engine *e, uint32_t n) {
  Dev &d = e->d;
  int rc = round_send_impl(e, (int)n);
  e->quiet_now = false;
  if (rc) return rc;
  const int64_t r0 = d.round;
  int64_t first = -1;
  uint32_t pairs = 0;
  for (uint32_t j = 0; j < n; j++) {
    d.round = r0 + j;
    if (!ae_round(e)) continue;
    set_round_fields(e);  // the matching draws inside a partition's side
    const uint32_t np = ae_matching(d).np;
    if (np && first < 0) first = d.round;
    pairs += np;
  }
  if (pairs) {
    d.round = first;
    set_round_fields(e);
    LaunchTimer t(e, GX_K_AE);
    k_ae_locked_note<<<1, 64, 0, e->stream>>>(d, pairs, 1u);
  }
  d.round = r0 + n;
  HIPCHK(hipGetLastError());
  return GX_OK;
}

static int wake_all(gx_engine *e) {
  set_round_fields(e);
  k_wake<<<nblk(e->d.Hl, 64), 64, 0, e->stream>>>(e->d);
  HIPCHK(hipGetLastError());
  return GX_OK;
}

// ------------------------------------------------------------------------------ ABI ------
extern "C" {

int gx_abi_version(void) { return GX_ABI_VERSION; }

int gx_set_stream(gx_engine *e, void *stream, int mode) {
  if (!e || (mode & ~(GX_STREAM_CALLER | GX_STREAM_ASYNC))) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  if (e->side_pending) HIPCHK(hipStreamSynchronize(e->side_stream));
  e->side_pending = false;
  HIPCHK(hipStreamSynchronize(e->stream));  // work queued so far completes first
  e->stream = (mode & GX_STREAM_CALLER) ? (hipStream_t)stream : e->own_stream;
  e->async_phases = (mode & GX_STREAM_ASYNC) ? 1 : 0;
  return GX_OK;
}
const char *gx_backend(void) { return "hip-gfx950"; }

void gx_params_default(gx_params *p) {
  memset(p, 0, sizeof(*p));
  p->n_hosts = 64;
  p->n_services = 8;
  p->fanout = 3;
  p->packet_cap = 32;
  p->pending_cap = 100;
  p->queue_cap = 1024;
  p->list_slots = 16;
  p->gossip_stop_on_empty = 1;
  p->alive_interval_rounds = 5;
  p->tombstone_interval_rounds = 10;
  p->retransmit_rounds = 5;
  p->alive_count = 5;
  p->tombstone_count = 10;
  p->init_mode = GX_INIT_EMPTY;
  p->t0_ns = 1700000000000000000ll;
  p->round_ns = 200000000ll;
  p->alive_lifespan_ns = 80000000000ll;
  p->draining_lifespan_ns = 600000000000ll;
  p->tombstone_lifespan_ns = 10800000000000ll;
  p->stale_fudge_ns = 60000000000ll;
  p->alive_broadcast_interval_ns = 60000000000ll;
  p->pass_increment_ns = 50;
  p->tombstone_bump_ns = 1000000000ll;
  p->seed = 0x5EEDull;
  p->aged_max_ns = 100000000000ll;
  p->storm_round = -1;
  p->overhead_bytes = 3;
  p->fd_probe_rounds = 5;
  p->fd_indirect_checks = 3;
  p->fd_msg_cap = 16;
  p->fd_msg_bytes = 64;
  p->fd_gossip_dead_rounds = 150;
  p->depart_round = -1;
  p->fd_push_pull_state = 1;
  p->lock_model = 1;
  p->lock_buffer = 1024 + 1 + 25 + 1 + 25 + 1;  // gx.h lock_model: handoff queue .. AddServiceEntry
  gx_fd_defaults(p);
}

// memberlist's size-derived parameters: util.go retransmitLimit / suspicionTimeout,
// suspicion.go remainingSuspicionTime (include/gx.h).
int gx_fd_defaults(gx_params *p) {
  if (!p || p->n_hosts < 1 || p->fd_probe_rounds < 1 || p->round_ns <= 0) return GX_EINVAL;
  const int suspicion_mult = 4, max_mult = 6, retransmit_mult = 4;
  const double n = (double)p->n_hosts;
  uint32_t limit = (uint32_t)(retransmit_mult * (int)ceil(log10(n + 1.0)));
  p->fd_retransmit_limit = limit > GX_FD_MAX_TX ? GX_FD_MAX_TX : limit;
  const double node_scale = fmax(1.0, log10(fmax(1.0, n)));
  const int64_t interval = (int64_t)p->fd_probe_rounds * p->round_ns;
  const int64_t tmin = (int64_t)suspicion_mult * (int64_t)(node_scale * 1000.0) * interval / 1000;
  const int64_t tmax = (int64_t)max_mult * tmin;
  int k = suspicion_mult - 2;
  if ((int)p->n_hosts - 2 < k) k = 0;
  p->fd_suspicion_k = (uint32_t)k;
  for (int c = 0; c < 8; c++) {
    int64_t t = tmin;
    if (c == 0) {
      t = k < 1 ? tmin : tmax;
    } else if (c <= k) {
      const double frac = log((double)c + 1.0) / log((double)k + 1.0);
      const double raw = (double)tmax / 1e9 - frac * ((double)tmax / 1e9 - (double)tmin / 1e9);
      t = (int64_t)floor(1000.0 * raw) * 1000000ll;
      if (t < tmin) t = tmin;
    }
    p->fd_suspicion_rounds[c] = (uint32_t)((t + p->round_ns - 1) / p->round_ns);
  }
  return GX_OK;
}

static int check_params(const gx_params *p) {
  if (!p || p->n_hosts < 1 || p->n_services < 1 || p->n_services > 64) return GX_EINVAL;
  if (p->fanout > 16 || p->packet_cap < 1 || p->packet_cap > 256 || p->pending_cap > 256) return GX_EINVAL;
  if (p->queue_cap < 1 || p->list_slots < 1 || p->list_slots > GX_MAX_LIST_SLOTS) return GX_EINVAL;
  if (p->n_hosts > GX_MAX_HOSTS) return GX_EINVAL;  // gx_job owner field
  if (p->alive_interval_rounds < 1 || p->tombstone_interval_rounds < 1) return GX_EINVAL;
  if (p->retransmit_rounds > 1000) return GX_EINVAL;
  if (p->alive_count < 1 || p->alive_count > GX_JOB_MAX_PASSES || p->tombstone_count < 1 ||
      p->tombstone_count > GX_JOB_MAX_PASSES)
    return GX_EINVAL;
  if (p->init_mode > GX_INIT_WARM) return GX_EINVAL;
  if (p->t0_ns < 0 || p->t0_ns > ((int64_t)1 << 62) || p->round_ns <= 0) return GX_EINVAL;
  {  // lifespans stay far inside the half window before t0 (gx.h GX_TS_SHIFT)
    const int64_t lim = (int64_t)1 << 58;
    for (int64_t x : {p->alive_lifespan_ns, p->draining_lifespan_ns, p->tombstone_lifespan_ns, p->stale_fudge_ns,
                      p->aged_max_ns})
      if (x < 0 || x > lim) return GX_EINVAL;
  }
  if ((uint64_t)p->n_hosts * p->n_services > 0xffffffffull) return GX_EINVAL;
  if (p->ae_period_rounds && p->ae_phase >= p->ae_period_rounds) return GX_EINVAL;
  if (p->limit_bytes > (1u << 24) || p->overhead_bytes > (1u << 16)) return GX_EINVAL;
  if (p->n_shards > 1 && (p->shard_id >= p->n_shards || p->n_shards > p->n_hosts || p->n_shards > 64)) return GX_EINVAL;
  if (p->depart_ppm > 1000000u) return GX_EINVAL;
  if (p->gossip_messages > 16) return GX_EINVAL;
  if (p->push_pull_mode > GX_PP_INITIATE || (p->push_pull_mode == GX_PP_INITIATE && p->fd_enable)) return GX_EINVAL;
  if (p->inbox_slots > GX_DI_MAX) return GX_EINVAL;
  if (p->lock_model > 1 || p->lock_buffer < 1 || p->lock_buffer > 65535) return GX_EINVAL;
  if (p->lock_model && (((uint64_t)p->n_hosts + (p->n_shards > 1 ? p->n_shards : 1) - 1) / (p->n_shards > 1 ? p->n_shards : 1)) *
                               p->lock_buffer * 16ull > GX_LOCK_BUF_MAX_BYTES)
    return GX_EINVAL; // the pipelines' records (gx.h lock_buffer)
  if (p->probe_piggyback > 1 || (p->probe_piggyback && (p->fd_enable || p->fd_probe_rounds < 1)))
    return GX_EINVAL;  // gx.h probe_piggyback: without the failure detector (sharded engines too)
  if (p->push_pull_stagger > 1 || (p->push_pull_stagger && (p->push_pull_mode != GX_PP_INITIATE || !p->ae_period_rounds)))
    return GX_EINVAL;
  if (p->lock_readers > GX_LOCK_READERS_CLAIMED || (p->lock_readers && !p->lock_model) || p->lock_defer_slots > GX_POOL_MAX)
    return GX_EINVAL;  // gx.h lock_readers (either pool policy): with the lock modelled
  if (p->lock_readers && p->n_shards > 1 && (p->lock_readers == GX_LOCK_READERS_CLAIMED || p->fd_enable))
    return GX_EINVAL;  // sharded engines: the direct-mapped pool, without the failure detector
  if (p->fd_handoff_shared > 1 || (p->fd_handoff_shared && (!p->fd_enable || !p->lock_model || p->n_shards > 1)))
    return GX_EINVAL;  // gx.h fd_handoff_shared
  if (p->fd_enable) {
    if (p->n_hosts > 65534 || p->fanout > 16) return GX_EINVAL;
    if (p->fd_probe_rounds < 1 || p->fd_indirect_checks > 16 || p->fd_msg_cap < 1 || p->fd_msg_cap > 64) return GX_EINVAL;
    if (p->fd_retransmit_limit < 1 || p->fd_retransmit_limit > GX_FD_MAX_TX || p->fd_suspicion_k > 2) return GX_EINVAL;
    for (uint32_t c = 0; c <= p->fd_suspicion_k; c++)
      if (p->fd_suspicion_rounds[c] > (1u << 30)) return GX_EINVAL;
  }
  return GX_OK;
}

int gx_destroy(gx_engine *e) {
  if (!e) return GX_EINVAL;
  (void)hipSetDevice(e->device);
  // every stream that may still run a kernel over the engine's buffers, before any is freed (the
  // planned exchange's look-ahead k_xplan batch on xplan_stream included: it was synchronized only
  // after the frees before round 6)
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  if (e->side_stream) (void)hipStreamSynchronize(e->side_stream);
  if (e->xplan_stream) (void)hipStreamSynchronize(e->xplan_stream);
  for (auto &t : e->pending_ev) {
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  e->mem.release();
  codec_free(e);
  // what is not hipMalloc memory
  if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
  if (e->side_stream) (void)hipStreamDestroy(e->side_stream);
  if (e->xplan_stream) (void)hipStreamDestroy(e->xplan_stream);
  for (hipEvent_t ev : {e->side_start, e->side_done, e->xplan_ev[0], e->xplan_ev[1], e->xplan_join})
    if (ev) (void)hipEventDestroy(ev);
  if (e->scan_snap) (void)hipHostFree(e->scan_snap);
  if (e->xplan_host) (void)hipHostFree(e->xplan_host);
  delete e;  // with the api scratch (DevBuf)
  return GX_OK;
}

// ------------------------------------------------------------------------------ gx_create --
// Its steps. A step that fails returns at once: gx_create destroys the engine with whatever the
// steps made so far.
static void create_dims(gx_engine *e, const gx_params *p) {
  Dev &d = e->d;
  d.p = *p;
  d.epoch = gx_epoch_of(p->t0_ns);
  d.p.t0_ns -= d.epoch;  // every device time is epoch-relative
  d.H = p->n_hosts;
  d.S = p->n_services;
  d.R = p->n_hosts * p->n_services;
  d.Q = p->queue_cap;
  d.A = p->list_slots;
  d.AW = (d.A + 31) / 32;
  d.L = p->packet_cap + p->pending_cap;
  d.K = p->fanout;
  d.NG = p->gossip_messages > 1 ? p->gossip_messages : 1;
  d.KG = d.K * d.NG;
  d.KE = d.KG + (p->probe_piggyback ? 2u : 0u);  // the probe ping and ack entries (gx.h probe_piggyback)
  d.divS = d.S > 1 ? ~0ull / d.S + 1 : 0;
  while ((1u << d.logS) < d.S) d.logS++;  // used where S divides 64 (a power of two)
  d.G = p->n_shards > 1 ? p->n_shards : 1;
  d.gid = d.G > 1 ? p->shard_id : 0;
  d.lo = (uint32_t)(((uint64_t)d.gid * d.H) / d.G);
  d.Hl = (uint32_t)(((uint64_t)(d.gid + 1) * d.H) / d.G) - d.lo;
  d.SQ = pow2_at_least(64 > d.KE * (p->retransmit_rounds + 1) ? 64 : d.KE * (p->retransmit_rounds + 1));
  d.DQ = pow2_at_least(d.L + p->pending_cap + 64);
  d.nblk_ae = (d.R + GX_DIGEST_SLOTS - 1) / GX_DIGEST_SLOTS;
  // default: 64 slots; with GossipMessages > 1 (up to NG packets per sender) GX_DI_MAX, so the
  // wave merge takes the wide inboxes instead of the serial overflow path
  d.DI = p->inbox_slots ? p->inbox_slots : (d.NG > 1 ? GX_DI_MAX : 64);
  d.DR = d.DI < 8 ? d.DI : 8;  // inline packets: 99.6% of Poisson(fanout 3) in-degrees fit 8 slots
  // senders read their local receivers' view slots and drop no-op records; packets from other
  // shards are filtered the same way on arrival (k_inbox_unpack)
  d.sfilt = 1u;
  d.QW = 4 * nblk(d.Hl ? d.Hl : 1, 64);  // k_send's waves (launch_send: 64 hosts per 256-thread block)
  d.departures = p->depart_round >= 0 && p->depart_ppm;
  if (p->lock_model) {  // gx.h lock_model, lock_readers, fd_handoff_shared
    d.C = p->lock_buffer;
    d.PW = (d.H + 31) / 32;
    if (p->lock_readers) d.P = p->lock_defer_slots ? p->lock_defer_slots : 64;
    // the handoff queue's places after the 53 the handler's chain holds
    if (p->fd_handoff_shared) d.HQ = d.C > GX_LOCK_HANDLER_AT ? d.C - GX_LOCK_HANDLER_AT : 0;
  }
  // worklist scans split rows of at least 64K slots into chunks of >= 32K (S | 128: owners never
  // straddle a chunk; the split path runs without listeners)
  e->scan_nch = 1;
  if (d.R >= 65536 && d.S >= 2 && 128 % d.S == 0)
    e->scan_nch = d.R / 32768 < 16 ? d.R / 32768 : 16;  // the most chunks a row takes (scan_chunks)
  if (getenv("GX_KPROF"))  // diagnostics: phase marks of every k_send wave (gx_kprof_read)
    e->kprof_n = (size_t)nblk(d.Hl, 64) * 4 * 8 + GX_KPROF_MERGE_N + 3ull * d.H;  // + merge counts + push-pull blocks + scans
  if (const char *qs = getenv("GX_QUIET_SEND")) e->quiet_send = strcmp(qs, "0") != 0;
  e->quiet_batch = GX_QUIET_BATCH;
  if (const char *qb = getenv("GX_QUIET_BATCH")) e->quiet_batch = (uint32_t)std::min(std::max(atol(qb), 1l), 1024l);
  if (d.G > 1) {
    e->nblk = d.nblk_ae;
    e->nmw = (e->nblk + 31) / 32;
  }
}

static int create_streams(gx_engine *e) {
  HIPCHK(hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking));
  e->stream = e->own_stream;
  HIPCHK(hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&e->side_start, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&e->side_done, hipEventDisableTiming));
  HIPCHK(hipHostMalloc((void **)&e->scan_snap, (2 + GX_QUIET_SLOTS) * sizeof(uint64_t), hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer((void **)&e->scan_snap_dev, e->scan_snap, 0));
  e->scan_snap[0] = e->scan_snap[1] = ~0ull;
  for (int i = 0; i < GX_QUIET_SLOTS; i++) e->scan_snap[2 + i] = 0;
  return GX_OK;
}

// TAKE(class, ptr, bytes[, fill byte, s]): one engine buffer, filled on the engine's stream. Its
// class is STATE, named by its checkpoint section (gx_ckpt.h GX_CK_*: gx_ckpt_save writes it,
// gx_ckpt_load restores it), or DERIVED with the reason nothing reads it before it is rewritten: after
// a load it is as this function leaves it. In doubt a buffer is STATE.
#define DERIVED 0u
#define TAKE(...) GXTRY(e->mem.take(__VA_ARGS__))

static int create_buffers(gx_engine *e) {
  Dev &d = e->d;
  const gx_params *p = &d.p;
  hipStream_t s = e->stream;
  // per-host arrays hold this shard's Hl hosts; the message table also takes the packets received
  // from other shards (at most (H - Hl) * K), so it is sized H * K.
  const size_t Hg = d.H, H = d.Hl, K = d.KE ? d.KE : 1;
  TAKE(GX_CK_VIEW, d.view, sizeof(uint64_t) * H * d.R);
  TAKE(GX_CK_OWN_STATUS, d.own_status, H * d.S);
  TAKE(GX_CK_HS, d.hs, sizeof(gx_host_state) * H);
  TAKE(GX_CK_FIFO, d.fifo, sizeof(gx_job) * H * d.Q);
  TAKE(GX_CK_SLEEP, d.sleep, sizeof(gx_sleeper) * H * d.SQ);
  TAKE(GX_CK_DQ, d.dq, sizeof(grec) * H * d.DQ);
  TAKE(GX_CK_ARENA, d.arena, sizeof(grec) * H * d.A * d.L);
  TAKE(GX_CK_ARENA_LEN, d.arena_len, sizeof(uint32_t) * H * d.A, 0, s);
  TAKE(GX_CK_ARENA_BITS, d.arena_bits, sizeof(uint32_t) * H * d.AW);
  TAKE(GX_CK_MSG, d.msg, sizeof(grec) * Hg * K * p->packet_cap);
  TAKE(GX_CK_MSG_W0, d.msg_w0, sizeof(uint64_t) * Hg * K * p->packet_cap);
  TAKE(GX_CK_MSG_LEN, d.msg_len, sizeof(uint32_t) * Hg * K, 0, s);
  TAKE(GX_CK_MSG_DST, d.msg_dst, sizeof(uint32_t) * Hg * K);
  TAKE(GX_CK_MSG_KEY, d.msg_key, sizeof(uint32_t) * Hg * K);
  TAKE(GX_CK_IN_CNT, e->in_cnt_buf, sizeof(uint32_t) * 2 * H, 0, s);
  TAKE(GX_CK_IN_HDR, d.in_hdr, sizeof(uint4) * H * d.DI);
  TAKE(GX_CK_IN_OVF, d.in_ovf, sizeof(uint4) * Hg * K);
  TAKE(GX_CK_IN_REC, d.in_rec, sizeof(grec) * H * d.DR * p->packet_cap);
  TAKE(GX_CK_WORK_CNT, d.work_cnt, sizeof(uint32_t) * GX_WC_N, 0, s);
  TAKE(DERIVED, d.quiet_w, sizeof(uint32_t) * 2 * d.QW, 0, s);  // (0: no round is quiet); DERIVED: tagged by the host's bound sequence, which restarts: k_send rewrites its wave's word before the host trusts any bound (quiet_from)
  TAKE(GX_CK_WORK, d.work, sizeof(uint32_t) * H);
  if (p->push_pull_mode == GX_PP_INITIATE && d.G < 2) {  // a sharded engine's batches go through ae_pa, ae_pb
    TAKE(DERIVED, e->pp_dev, sizeof(uint32_t) * 2 * Hg);  // DERIVED: ae_initiate copies the round's schedule in before its launches
    TAKE(DERIVED, e->pp_prow, sizeof(int32_t) * Hg, 0xff, s);  // DERIVED: constant: all -1 since gx_create
  }
  TAKE(GX_CK_MREC, d.mrec, sizeof(uint32_t) * H, 0, s);
  TAKE(GX_CK_MINEXP, d.minexp, sizeof(unsigned long long) * H);
  TAKE(GX_CK_SCAN_LIST, d.scan_list, sizeof(grec) * H * d.L);
  TAKE(GX_CK_SCAN_CNT, d.scan_cnt, sizeof(uint32_t) * H);
  if (e->scan_nch > 1) {
    TAKE(DERIVED, e->scan_tmp, sizeof(grec) * H * e->scan_nch * d.L);  // DERIVED: k_scan_split writes a row's chunks before k_scan_join reads them, in the same round
    TAKE(DERIVED, e->scan_chunk, sizeof(ScanChunk) * H * e->scan_nch);  // DERIVED: as scan_tmp
  }
  TAKE(GX_CK_TICK, d.tick, H, 0, s);
  TAKE(GX_CK_SBYTES, d.sbytes, sizeof(uint16_t) * d.R);
  TAKE(GX_CK_SRVT, d.srvt, sizeof(gx_server_times) * H * Hg);
  TAKE(GX_CK_VLC, d.vlc, sizeof(int64_t) * H);
  TAKE(DERIVED, d.ev_slot, sizeof(int32_t) * H, 0xff, s);  // -1: no listener; DERIVED: listeners are not part of a checkpoint: -1 as created
  TAKE(GX_CK_CTR, d.ctr, sizeof(DevCtr), 0, s);
  if (p->fd_enable) {  // member rows of this shard's hosts
    TAKE(GX_CK_MEM, d.mem, sizeof(gx_member) * H * Hg);
    TAKE(GX_CK_FD_DL, d.fd_dl, sizeof(int32_t) * H * Hg);
    TAKE(GX_CK_FDH, d.fdh, sizeof(gx_fd_host) * H);
    TAKE(GX_CK_FDM, d.fdm, sizeof(gx_fd_msg) * Hg * K * p->fd_msg_cap);
    TAKE(GX_CK_FD_LEN, d.fd_len, sizeof(uint32_t) * Hg * K, 0, s);
    TAKE(GX_CK_FD_PEERS, d.fd_peers, sizeof(uint32_t) * H * K);
    TAKE(GX_CK_FD_NP, d.fd_np, sizeof(uint32_t) * H);
    if (p->fd_push_pull_state) TAKE(GX_CK_FD_SNAP, d.fd_snap, sizeof(uint64_t) * H * Hg);
  }
  if (p->lock_model) {  // locked hosts' inbound pipelines and waiting ExpireServer calls (gx.h lock_model)
    TAKE(GX_CK_LKB, d.lkb, sizeof(grec) * H * d.C);
    if (p->storm_round >= 0 || p->fd_enable) TAKE(GX_CK_PEXP, d.pexp, sizeof(uint32_t) * H * d.PW, 0, s);
    if (p->lock_readers) {  // the waiting push-pull merges' pool (gx.h lock_readers)
      TAKE(GX_CK_DPOOL, d.dpool, sizeof(uint64_t) * d.P * d.R);
      TAKE(GX_CK_DPOOL_HOST, d.dpool_host, sizeof(uint32_t) * d.P, 0xff, s);
      TAKE(GX_CK_DPOOL_RES, d.dpool_res, sizeof(uint32_t) * d.P, 0, s);
      TAKE(DERIVED, d.ro_flag, H, 0, s);  // DERIVED: k_ae_claim clears every flag it lists: zero between rounds, as created
      TAKE(DERIVED, d.ro_list, sizeof(uint32_t) * H);  // DERIVED: k_ae_claim writes the list before k_ae_rox reads it
      TAKE(DERIVED, d.ro_n, sizeof(uint32_t), 0, s);  // DERIVED: k_ae_claim writes it before k_ae_rox reads it
      TAKE(GX_CK_DSLOT, d.dslot, sizeof(uint32_t) * Hg, 0xff, s);  // each host's slot, the claimants' bits
      TAKE(DERIVED, d.claim_bits, sizeof(uint32_t) * ((Hg + 31) / 32), 0, s);  // DERIVED: k_ae_claim sets and clears them in one launch: zero between rounds
    }
    if (p->fd_handoff_shared) TAKE(GX_CK_FDQ, d.fdq, sizeof(gx_fd_msg) * H * (d.HQ ? d.HQ : 1));
  }
  TAKE(DERIVED, e->conv_bad, sizeof(unsigned long long));  // DERIVED: gx_converged zeroes it before its kernel
  if (e->kprof_n) TAKE(DERIVED, d.kprof, sizeof(unsigned long long) * e->kprof_n, 0, s);  // DERIVED: diagnostics
  TAKE(DERIVED, e->digest_buf, sizeof(uint64_t) * H);  // DERIVED: k_digest writes it before gx_host_digests copies it out
  if (d.G > 1) {
    TAKE(DERIVED, e->ob_entries, sizeof(uint32_t) * H * K);  // DERIVED: outbox_plan rebuilds it every round before a pack reads it
    TAKE(GX_CK_IN_STAMP, d.in_stamp, sizeof(uint32_t) * Hg * K, 0, s);
    TAKE(DERIVED, e->ob_total, sizeof(uint32_t));  // DERIVED: k_ob_bytes writes it before k_outbox_pack reads it
    TAKE(DERIVED, e->ob_claim, sizeof(uint32_t) * (XPLAN_GMAX + 1), 0, s);  // DERIVED: the last block of a packing k_send resets it: zero between rounds
    if (p->probe_piggyback) TAKE(GX_CK_PROBE_X, d.probe_x, sizeof(unsigned long long) * 2, 0, s);
    TAKE(DERIVED, e->ob_counts, sizeof(uint32_t) * d.G * (1 + 2 * ((H * K + 255) / 256)));  // DERIVED: outbox_plan rebuilds it every round
    const size_t np = Hg / 2 + 1;
    TAKE(DERIVED, e->ae_pa, sizeof(uint32_t) * np);  // DERIVED: the push-pull chain (gx_ae_bytes) plans it anew every step
    TAKE(DERIVED, e->ae_pb, sizeof(uint32_t) * np);  // DERIVED: as ae_pa
    TAKE(DERIVED, e->ae_prow, sizeof(int32_t) * np);  // DERIVED: as ae_pa
    TAKE(DERIVED, e->ae_pcount, np);  // DERIVED: as ae_pa
    TAKE(DERIVED, e->ae_pack_host, sizeof(uint32_t) * np);  // DERIVED: as ae_pa
    TAKE(DERIVED, e->ae_pack_t, sizeof(uint32_t) * np);  // DERIVED: as ae_pa
    TAKE(DERIVED, e->ae_pack_other, sizeof(uint32_t) * np);  // DERIVED: as ae_pa
    TAKE(DERIVED, e->ae_pack_first, np);  // DERIVED: as ae_pa
    TAKE(DERIVED, e->ae_skip, np);  // DERIVED: as ae_pa
    if (pp_state(d)) TAKE(DERIVED, e->fd_rsnap, sizeof(uint64_t) * np * Hg);  // DERIVED: received with the step's digests before the merge reads it
    TAKE(DERIVED, e->ae_dig, sizeof(ulonglong2) * H * e->nblk);  // DERIVED: the step's digest pass writes it
    TAKE(DERIVED, e->ae_mask, sizeof(uint32_t) * H * e->nmw);  // DERIVED: the step's mask pass writes it
    TAKE(DERIVED, e->ae_fmask, sizeof(uint32_t) * H * e->nmw);  // DERIVED: as ae_mask
    TAKE(DERIVED, e->ae_lt, sizeof(uint16_t) * H * e->nblk);  // DERIVED: as ae_mask
    TAKE(DERIVED, e->ae_retL, sizeof(uint16_t) * H * e->nblk);  // DERIVED: the step's return pass writes it
    TAKE(DERIVED, e->ae_bcnt, sizeof(uint32_t) * H * e->nblk);  // DERIVED: as ae_dig
    TAKE(DERIVED, e->ae_cnt, sizeof(uint32_t) * H);  // DERIVED: as ae_mask
    TAKE(DERIVED, e->ae_nfol, sizeof(uint32_t) * H);  // DERIVED: as ae_mask
    TAKE(DERIVED, e->ae_sz, sizeof(uint64_t) * 4 * H);  // DERIVED: the step's size passes write it
    TAKE(DERIVED, e->ae_off, sizeof(uint64_t) * 4 * H);  // DERIVED: the step's scans write it
    TAKE(DERIVED, e->ae_rioff, sizeof(uint64_t) * H);  // DERIVED: as ae_off
    TAKE(DERIVED, e->ae_err, sizeof(uint32_t));  // DERIVED: each chain call zeroes it before its kernels
    if (p->lock_readers) {
      TAKE(DERIVED, e->ae_rov, np, 0, s);  // DERIVED: k_ae_mask writes each planned pair's verdict before the step reads it
      TAKE(GX_CK_RO_XC, e->ro_xc, sizeof(unsigned long long) * 3, 0, s);
    }
  }
  return GX_OK;
}
#undef TAKE
#undef DERIVED

static int create_init(gx_engine *e) {
  Dev &d = e->d;
  hipStream_t s = e->stream;
  DevMem tmp;  // freed on every return, after sync_check has waited for the kernels
  uint64_t *rec_word;
  GXTRY(tmp.take(rec_word, sizeof(uint64_t) * d.R));
  HIPCHK(hipMemsetAsync(d.ctr->first_drop, 0xff, sizeof(d.ctr->first_drop), s));  // min: none yet
  k_fill_u16<<<256, 256, 0, s>>>(d.sbytes, d.R, (uint16_t)GX_STATIC_BYTES_DEFAULT);
  set_round_fields(e);
  k_init_rec<<<nblk(d.R, 256), 256, 0, s>>>(d, rec_word);
  k_init_views<<<2048, 256, 0, s>>>(d, rec_word);
  k_init_times<<<2048, 256, 0, s>>>(d, rec_word);
  k_init_hosts<<<nblk(d.Hl, 256), 256, 0, s>>>(d);
  if (d.p.fd_enable) k_fd_init<<<2048, 256, 0, s>>>(d);
  k_minexp_recompute<<<d.Hl, 256, 0, s>>>(d, 0);
  return sync_check(e);
}

int gx_create(const gx_params *p, gx_engine **out) {
  if (!out) return GX_EINVAL;
  int rc = check_params(p);
  if (rc) return rc;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || p->device < 0 || p->device >= ndev) return GX_EIO;
  HIPCHK(hipSetDevice(p->device));
  gx_engine *e = new gx_engine();  // value-initialised: zero wherever the struct names no other value
  e->device = p->device;
  create_dims(e, p);
  if ((rc = create_streams(e)) || (rc = create_buffers(e)) || (rc = create_init(e))) {
    (void)hipGetLastError();
    gx_destroy(e);
    return rc;
  }
  *out = e;
  return GX_OK;
}

int gx_set_round(gx_engine *e, int64_t round) {
  if (!e || round < e->d.round || round >= GX_MAX_ROUND) return GX_EINVAL;
  const bool jump = round != e->d.round;
  e->d.round = round;
  e->pp_cursor = 0;
  GXTRY(enter(e, ENTRY_MUTATE));  // with the new round: no bound from before the jump counts in it
  if (jump) {  // this round's and the next round's counters start empty
    HIPCHK(hipMemsetAsync(e->in_cnt_buf, 0, sizeof(uint32_t) * 2 * e->d.Hl, e->stream));
    HIPCHK(hipMemsetAsync(e->d.work_cnt, 0, sizeof(uint32_t) * GX_WC_ERR, e->stream));
  }
  int rc = wake_all(e);
  return rc ? rc : sync_check(e);
}

int gx_get_round(gx_engine *e, int64_t *round) {
  if (!e || !round) return GX_EINVAL;
  *round = e->d.round;
  return GX_OK;
}

int gx_enable_timing(gx_engine *e, int on) {
  if (!e) return GX_EINVAL;
  e->timing = on ? 1 : 0;
  return GX_OK;
}

int gx_run_rounds(gx_engine *e, uint32_t n_rounds) {
  if (!e || e->d.G > 1 || e->d.round + n_rounds >= GX_MAX_ROUND) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_ROUNDS));
  e->quiet_nowait = false;
  for (uint32_t i = 0; i < n_rounds;) {
    const uint32_t nb = quiet_batch_len(e, n_rounds - i);
    int rc = nb > 1 ? run_quiet_batch(e, nb) : run_one_round(e);
    if (rc) return rc;
    i += nb;
    if (e->pending_ev.size() > 4096) {
      rc = drain_timing(e);
      if (rc) return rc;
    }
  }
  int rc = wake_all(e);
  if (rc) return rc;
  return sync_check(e);
}

// ------------------------------------------------------------------------- sharded rounds --
static uint32_t shard_of(const Dev &d, uint32_t v) {  // shard g owns [floor(g H / G), floor((g + 1) H / G))
  uint32_t g = (uint32_t)(((uint64_t)v * d.G) / d.H);
  while (g > 0 && (uint32_t)(((uint64_t)g * d.H) / d.G) > v) g--;
  while (g + 1 < d.G && (uint32_t)(((uint64_t)(g + 1) * d.H) / d.G) <= v) g++;
  return g;
}
// packet slot (gx.h wire format): header, packet_cap records, then fd_msg_cap memberlist messages
// when the failure detector is on
static size_t slot_bytes(const Dev &d) {
  return 16 + 16ull * d.p.packet_cap + (d.p.fd_enable ? 16ull * d.p.fd_msg_cap : 0);
}

int gx_round_send(gx_engine *e) {
  if (!e) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  e->round_open = true;
  int rc = round_send_impl(e);
  return rc ? rc : phase_done(e);
}

// This round's outbox plan: the entries of this shard's packets bound for other shards, grouped by
// destination shard in key order (ob_entries), and the packets per destination (ob_counts[0..G)).
static void outbox_plan(gx_engine *e) {
  const Dev &d = e->d;
  const size_t ne = (size_t)d.Hl * d.KE;
  const uint32_t nchunk = (uint32_t)((ne + 255) / 256);
  uint32_t *ccnt = e->ob_counts + d.G, *off = ccnt + (size_t)nchunk * d.G;
  const size_t lds = sizeof(uint32_t) * 4 * d.G;
  k_ob_count<<<nchunk, 256, lds, e->stream>>>(d, ccnt);
  k_ob_scan<<<1, 256, 0, e->stream>>>(d, ccnt, nchunk, off, e->ob_counts);
  k_ob_fill<<<nchunk, 256, lds, e->stream>>>(d, off, e->ob_entries);
}

// The outbox plan, read back: sizes in bytes per shard.
int gx_outbox_bytes(gx_engine *e, uint64_t *bytes) {
  if (!e || !bytes) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  Dev &d = e->d;
  for (uint32_t g = 0; g < d.G; g++) bytes[g] = 0;
  e->n_ob = 0;
  e->ob_async = false;
  if (d.G < 2 || !d.KE) return GX_OK;
  outbox_plan(e);
  std::vector<uint32_t> cnt(d.G);
  HIPCHK(hipMemcpyAsync(cnt.data(), e->ob_counts, sizeof(uint32_t) * d.G, hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  uint64_t n = 0;
  for (uint32_t g = 0; g < d.G; g++) {
    bytes[g] = cnt[g] * slot_bytes(d);
    n += cnt[g];
  }
  e->n_ob = (uint32_t)n;
  return GX_OK;
}

int gx_outbox_sizes_async(gx_engine *e, uint64_t *bytes) {
  if (!e || !bytes) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  Dev &d = e->d;
  e->n_ob = 0;
  e->ob_async = false;
  if (d.G < 2 || !d.KE) {
    HIPCHK(hipMemsetAsync(bytes, 0, sizeof(uint64_t) * d.G, e->stream));
    return phase_done(e);
  }
  outbox_plan(e);
  k_ob_bytes<<<1, 64, 0, e->stream>>>(d, e->ob_counts, (unsigned long long *)bytes, e->ob_total);
  e->ob_async = true;
  return phase_done(e);
}

int gx_outbox_pack(gx_engine *e, void *buf, uint64_t cap) {
  if (!e || (cap && !buf)) return GX_EINVAL;
  if (!e->ob_async && !e->n_ob) return GX_OK;
  if (!e->ob_async && cap < e->n_ob * slot_bytes(e->d)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  if (e->ob_async) {  // the slot count is on the device: a grid of the largest possible count
    e->ob_async = false;
    const uint32_t cap_slots = (uint32_t)(cap / slot_bytes(e->d));
    const uint32_t nmax = e->d.Hl * e->d.KE;
    if (nmax) k_outbox_pack<<<nmax, 64, 0, e->stream>>>(e->d, e->ob_entries, 0, (uint8_t *)buf, e->ob_total, cap_slots);
    return phase_done(e);
  }
  k_outbox_pack<<<e->n_ob, 64, 0, e->stream>>>(e->d, e->ob_entries, e->n_ob, (uint8_t *)buf);
  return phase_done(e);
}

static bool send_packs(const Dev &d);
// Batch `start` of slot bounds into host slot k (asynchronous, on xplan_stream).
static int xplan_launch(gx_engine *e, int k, int64_t start) {
  Dev &d = e->d;
  const size_t n = (size_t)XPLAN_BATCH * d.G * d.G;
  uint32_t *dev = e->xplan_dev + (size_t)k * n;
  // the rounds queued so far may read this half (a packing k_send, Dev::ob_cnt): the rewrite waits
  // for them; without packing sends only the host half is read, so the look-ahead runs at once
  if (send_packs(d)) {
    HIPCHK(hipEventRecord(e->xplan_join, e->stream));
    HIPCHK(hipStreamWaitEvent(e->xplan_stream, e->xplan_join, 0));
  }
  HIPCHK(hipMemsetAsync(dev, 0, sizeof(uint32_t) * n, e->xplan_stream));
  k_xplan<<<dim3(nblk(d.H, 256), XPLAN_BATCH), 256, 0, e->xplan_stream>>>(d, start, dev);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(e->xplan_host + (size_t)k * n, dev, sizeof(uint32_t) * n, hipMemcpyDeviceToHost,
                        e->xplan_stream));
  HIPCHK(hipEventRecord(e->xplan_ev[k], e->xplan_stream));
  e->xplan_start[k] = start;
  return GX_OK;
}
// The counts of the current round: its batch (computed XPLAN_BATCH rounds ahead, so the wait below
// finds it done except for the first batch) and the next batch queued behind it.
static int xplan_counts(gx_engine *e, const uint32_t **out) {
  Dev &d = e->d;
  if (!e->xplan_dev) {
    if (hipStreamCreateWithFlags(&e->xplan_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->xplan_ev[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->xplan_ev[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->xplan_join, hipEventDisableTiming) != hipSuccess ||
        hipHostMalloc((void **)&e->xplan_host, sizeof(uint32_t) * 2 * XPLAN_BATCH * d.G * d.G) != hipSuccess ||
        e->mem.take(e->xplan_dev, sizeof(uint32_t) * 2 * XPLAN_BATCH * d.G * d.G)) {
      (void)hipGetLastError();
      return GX_ENOMEM;
    }
  }
  const int64_t start = d.round - d.round % XPLAN_BATCH;
  const int k = (int)((start / XPLAN_BATCH) & 1);
  int rc = GX_OK;
  if (e->xplan_start[k] != start) rc = xplan_launch(e, k, start);
  if (!rc && e->xplan_start[k ^ 1] != start + XPLAN_BATCH) rc = xplan_launch(e, k ^ 1, start + XPLAN_BATCH);
  if (rc) return rc;
  e->xplan_waits[1]++;
  const hipError_t q = hipEventQuery(e->xplan_ev[k]);
  if (q == hipErrorNotReady) {
    e->xplan_waits[0]++;  // this call blocks the host
    HIPCHK(hipEventSynchronize(e->xplan_ev[k]));
  } else {
    HIPCHK(q);
  }
  const size_t row = ((size_t)k * XPLAN_BATCH + (size_t)(d.round - start)) * d.G * d.G;
  *out = e->xplan_host + row;
  e->xbound_dev = e->xplan_dev + row + (size_t)d.gid * d.G;
  return GX_OK;
}

int gx_exchange_plan(gx_engine *e, uint64_t *sizes) {
  if (!e || !sizes) return GX_EINVAL;
  Dev &d = e->d;
  if (d.p.fd_enable) return GX_ENOSYS;
  if (d.G > XPLAN_GMAX) return GX_EINVAL;
  for (uint32_t i = 0; i < d.G * d.G; i++) sizes[i] = 0;
  if (d.G < 2 || !d.KE) return GX_OK;
  GXTRY(enter(e, ENTRY_PHASE));
  const uint32_t *c = nullptr;
  int rc = xplan_counts(e, &c);
  if (rc) return rc;
  for (uint32_t i = 0; i < d.G * d.G; i++) sizes[i] = (uint64_t)c[i] * slot_bytes(d);
  for (uint32_t g = 0; g < XPLAN_GMAX; g++) e->xbound.n[g] = g < d.G ? c[d.gid * d.G + g] : 0u;
  e->xbound_round = d.round;
  return GX_OK;
}

int gx_outbox_pack_planned(gx_engine *e, void *buf, uint64_t cap) {
  if (!e || (cap && !buf)) return GX_EINVAL;
  Dev &d = e->d;
  if (d.p.fd_enable) return GX_ENOSYS;
  if (d.G < 2 || !d.KE) return GX_OK;
  if (e->xbound_round != d.round) {  // the plan of this round, if the caller did not ask for it
    std::vector<uint64_t> tmp((size_t)d.G * d.G);
    int rc = gx_exchange_plan(e, tmp.data());
    if (rc) return rc;
  }
  uint64_t slots = 0;
  for (uint32_t g = 0; g < d.G; g++) slots += e->xbound.n[g];
  if (cap < slots * slot_bytes(d)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  outbox_plan(e);
  // one block at least: block 0 checks every destination's packets against its plan bound
  k_outbox_pack_planned<<<(unsigned)(slots ? slots : 1), 64, 0, e->stream>>>(d, e->ob_entries, e->ob_counts, e->xbound, (uint8_t *)buf);
  e->n_ob = 0;
  e->ob_async = false;
  return phase_done(e);
}

int gx_inbox_unpack(gx_engine *e, const void *buf, uint64_t bytes) {
  if (!e || (bytes && !buf) || bytes % slot_bytes(e->d)) return GX_EINVAL;
  uint64_t n = bytes / slot_bytes(e->d);
  if (n > (uint64_t)(e->d.H - e->d.Hl) * e->d.KE) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  if (n) k_inbox_unpack<<<(unsigned)n, 64, 0, e->stream>>>(e->d, (const uint8_t *)buf, (uint32_t)n);
  e->d.n_remote = (uint32_t)n;
  return phase_done(e);
}

int gx_round_merge(gx_engine *e) {
  if (!e) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_PHASE));
  int rc = round_merge_impl(e);
  return rc ? rc : phase_done(e);
}

int gx_round_end(gx_engine *e) {
  if (!e || e->d.round + 1 >= GX_MAX_ROUND) return GX_EINVAL;  // rounds are 32-bit in jobs and sleepers
  GXTRY(enter(e, ENTRY_PHASE));
  int rc = join_side(e);
  if (rc) return rc;
  GXTRY(watch_round_end(e));
  e->round_open = false;
  e->pp_cursor = 0;
  rc = wake_all(e);
  return rc ? rc : phase_done(e);
}

// A round whose k_send packs the planned exchange itself (Dev::ob_buf): send_planned's rounds
// (round_send_impl's `plan`) with one message per target.
static bool send_packs(const Dev &d) {
  return d.G >= 2 && d.K && d.NG == 1 && !d.p.limit_bytes && d.p.retransmit_rounds > 0 && !d.departures &&
         !d.p.fd_enable;
}

int gx_round_gossip_begin(gx_engine *e, uint64_t *plan, void *buf, uint64_t cap) {
  if (!e || !plan || (cap && !buf)) return GX_EINVAL;
  Dev &d = e->d;
  e->round_open = true;
  if (!send_packs(d)) {
    int rc = gx_round_send(e);
    if (!rc) rc = gx_exchange_plan(e, plan);
    if (!rc) rc = gx_outbox_pack_planned(e, buf, cap);
    return rc;
  }
  // the plan first (its batch is on the device since the host saw it done), then one launch that
  // sends and writes every slot of the buffer
  int rc = gx_exchange_plan(e, plan);
  if (rc) return rc;
  uint64_t slots = 0;
  for (uint32_t g = 0; g < d.G; g++) slots += e->xbound.n[g];
  if (cap < slots * slot_bytes(d)) return GX_EINVAL;
  d.ob_buf = (uint8_t *)buf;
  d.ob_cnt = e->xbound_dev;
  d.ob_claim = e->ob_claim;
  rc = gx_round_send(e);
  d.ob_buf = nullptr;
  d.ob_cnt = nullptr;
  d.ob_claim = nullptr;
  e->n_ob = 0;
  e->ob_async = false;
  return rc;
}

int gx_round_gossip_end(gx_engine *e, const void *buf, uint64_t bytes, int *ae) {
  if (!e || !ae) return GX_EINVAL;
  int rc = gx_inbox_unpack(e, buf, bytes);
  if (!rc) rc = gx_round_merge(e);
  if (rc) return rc;
  *ae = ae_round(e) ? 1 : 0;
  return *ae ? GX_OK : gx_round_end(e);
}

}  // extern "C"

// the single-host calls: catalog, readers, listeners, memberlist, stats and diagnostics
#include "gx_api_host.hpp"

// the record watch of include/gx_watch.h: gx_watch_arm, gx_watch_set, gx_watch_read
#include "gx_watch_host.hpp"

// a sharded engine's push-pull chain: gx_ae_bytes .. gx_ae_merge, gx_ae_claim_*, gx_ae_skip_locked
#include "gx_ae_chain_host.hpp"

// engine checkpoints of include/gx_ckpt.h: gx_ckpt_save, gx_ckpt_save_coded, gx_ckpt_params, gx_ckpt_load
#include "gx_ckpt_host.hpp"

// full-state JSON codec: gx_set_names, gx_local_state_json, gx_decode_state_json,
// gx_merge_remote_state_json
#include "gx_codec_host.hpp"
