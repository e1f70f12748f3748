// gx_api_host.hpp — the single-host calls of include/gx.h: catalog calls, readers, listeners, the
// memberlist calls, stats and diagnostics. Included by gx_engine.hip, which keeps the engine proper
// (buffers, create / destroy, the round driver and the sharded phase calls) and the entry guard
// every call here opens with (enter).

// ---------------------------------------------------------------------- record helpers --
static int to_grec(const gx_engine *e, const gx_service *s, grec *g) {
  if (s->host >= e->d.H || s->svc >= e->d.S || s->status > 6) return GX_EINVAL;
  g->w = pack(gx_ts_in(s->updated_ns, e->d.epoch), s->status);
  g->r = s->host * e->d.S + s->svc;
  g->pad = 0;
  return GX_OK;
}
static void to_svc(const gx_engine *e, const grec *g, gx_service *s) {
  s->updated_ns = ts_of(g->w) + e->d.epoch;
  s->host = g->r / e->d.S;
  s->svc = (uint16_t)(g->r % e->d.S);
  s->status = (uint8_t)st_of(g->w);
  s->flags = 0;
}

// One call's layout of the api scratch: api_carve(e, region(p, n), ...) points each p at n elements
// of its type, the regions in order, after one ensure_api for all of them, so the size asked for and
// the pointers used come from the same description. Every region starts on its own 256 bytes: a
// count the device writes never shares them with the list behind it.
template <class T>
struct ApiRegion {
  T *&p;
  size_t n;
};
template <class T>
static ApiRegion<T> region(T *&p, size_t n) {
  return {p, n};
}
static size_t api_pad(size_t bytes) { return ((bytes ? bytes : 1) + 255) & ~(size_t)255; }
template <class... T>
static int api_carve(gx_engine *e, ApiRegion<T>... r) {
  GXTRY(ensure_api(e, (api_pad(sizeof(T) * r.n) + ... + 0)));
  char *at = (char *)e->api.p;
  ((r.p = (T *)at, at += api_pad(sizeof(T) * r.n)), ...);
  return GX_OK;
}

// Caller records -> grecs, checked (the host half of staging them) ...
static int to_grecs(const gx_engine *e, const gx_service *svcs, uint32_t n, std::vector<grec> &g) {
  g.resize(n);
  for (uint32_t i = 0; i < n; i++)
    if (to_grec(e, &svcs[i], &g[i])) return GX_EINVAL;
  return GX_OK;
}
// ... and into their region of the api scratch, on the engine's stream
static int stage_recs(gx_engine *e, const std::vector<grec> &g, grec *dev) {
  if (!g.empty()) HIPCHK(hipMemcpyAsync(dev, g.data(), sizeof(grec) * g.size(), hipMemcpyHostToDevice, e->stream));
  return GX_OK;
}

// `n` elements of a device ring of `ring` elements from `head` on, at most `cap` of them, to the host.
template <class J>
static int read_ring(const J *base, uint32_t ring, uint32_t head, uint32_t n, J *out, uint32_t cap) {
  const uint32_t m = n < cap ? n : cap;
  for (uint32_t i = 0; i < m;) {
    const uint32_t idx = (head + i) % ring;
    uint32_t run = ring - idx;
    if (run > m - i) run = m - i;
    HIPCHK(hipMemcpy(&out[i], &base[idx], sizeof(J) * run, hipMemcpyDeviceToHost));
    i += run;
  }
  return GX_OK;
}
// n records on the device (a list, or a ring from `head` on), up to `cap` of them back as
// gx_service. The device is done with them: the caller has waited (read_back, gx_read_hosts).
static int copy_out_recs(const gx_engine *e, const grec *dev, uint32_t n, gx_service *out, uint32_t cap,
                         uint32_t ring = ~0u, uint32_t head = 0) {
  const uint32_t m = n < cap ? n : cap;
  std::vector<grec> tmp(m);
  GXTRY(read_ring(dev, ring, head, m, tmp.data(), m));
  for (uint32_t i = 0; i < m; i++) to_svc(e, &tmp[i], &out[i]);
  return GX_OK;
}
// One record for a list the host builds itself: written while it fits, counted always.
static void put_rec(const gx_engine *e, uint64_t w, uint32_t r, gx_service *out, uint32_t cap, uint32_t &n) {
  if (n < cap) {
    grec g;
    g.w = w;
    g.r = r;
    to_svc(e, &g, &out[n]);
  }
  n++;
}

// TombstoneOthersServices over one view for an ABI call: one block, always the ChangeEvent variant.
static void scan_one_view(gx_engine *e, uint32_t view, grec *list, uint32_t cap, uint32_t *cnt) {
  with_flag(vec_of(e), [&](auto V) { k_scan<V(), true><<<1, 256, 0, e->stream>>>(e->d, list, 0, cap, cnt, (int)view); });
}

extern "C" {

static int api_add(gx_engine *e, const uint32_t *views, uint32_t fixed_view, const gx_service *svcs, uint32_t n,
                   int src, uint32_t *n_acc) {
  if (views)
    for (uint32_t i = 0; i < n; i++)
      if (!own(e, views[i])) return GX_EINVAL;
  std::vector<grec> g;
  GXTRY(to_grecs(e, svcs, n, g));
  GXTRY(enter(e, ENTRY_MUTATE));
  uint32_t *dviews, *dacc;
  grec *drec;
  GXTRY(api_carve(e, region(dviews, n), region(dacc, 1), region(drec, n)));
  GXTRY(stage_recs(e, g, drec));
  if (views && n) HIPCHK(hipMemcpyAsync(dviews, views, sizeof(uint32_t) * n, hipMemcpyHostToDevice, e->stream));
  k_api_add<<<1, 64, 0, e->stream>>>(e->d, views ? dviews : nullptr, fixed_view, drec, n, src, dacc);
  uint32_t acc = 0;
  int rc = read_back(e, dacc, &acc);
  if (!rc && n_acc) *n_acc = acc;
  return rc;
}

int gx_add_service_entries(gx_engine *e, const uint32_t *views, const gx_service *svcs, uint32_t n,
                           uint32_t *n_accepted) {
  if (!e || (n && (!views || !svcs))) return GX_EINVAL;
  return api_add(e, views, 0, svcs, n, SRC_LOCAL, n_accepted);
}

int gx_notify_msg(gx_engine *e, uint32_t host, const gx_service *recs, uint32_t n) {
  if (!e || !own(e, host) || (n && !recs)) return GX_EINVAL;
  return api_add(e, nullptr, host, recs, n, SRC_GOSSIP, nullptr);
}

int gx_merge_remote_state(gx_engine *e, uint32_t view, const gx_service *svcs, uint32_t n) {
  if (!e || !own(e, view) || (n && !svcs)) return GX_EINVAL;
  return api_add(e, nullptr, view, svcs, n, SRC_AE, nullptr);
}

int gx_merge(gx_engine *e, uint32_t dst, uint32_t src) {
  if (!e || !own(e, dst) || !own(e, src)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  with_flags(vec_of(e), ev_of(e),
             [&](auto V, auto E) { k_merge_views<V(), E()><<<1, 256, 0, e->stream>>>(e->d, dst, src); });
  return sync_check(e);
}

int gx_tombstone_others(gx_engine *e, uint32_t view, gx_service *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, view) || (cap && !out)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  uint32_t *dcnt;
  grec *dlist;
  GXTRY(api_carve(e, region(dcnt, 1), region(dlist, cap)));
  scan_one_view(e, view, dlist, cap, dcnt);
  uint32_t n = 0;
  GXTRY(read_back(e, dcnt, &n));
  GXTRY(copy_out_recs(e, dlist, n, out, cap));
  if (n_out) *n_out = n;
  return GX_OK;
}

int gx_tombstone_services(gx_engine *e, uint32_t host, const uint16_t *running, uint32_t n_running, gx_service *out,
                          uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, host) || (n_running && !running) || (cap && !out)) return GX_EINVAL;
  uint64_t mask = 0;
  for (uint32_t i = 0; i < n_running; i++) {
    if (running[i] >= e->d.S) return GX_EINVAL;
    mask |= 1ull << running[i];
  }
  GXTRY(enter(e, ENTRY_MUTATE));
  uint64_t *dm;
  GXTRY(api_carve(e, region(dm, 1)));
  k_api_tomb<<<1, 64, 0, e->stream>>>(e->d, host, mask, dm);
  uint64_t m = 0;
  GXTRY(read_back(e, dm, &m));
  uint32_t n = 0;
  const uint64_t w = pack(now_of(e), GX_TOMBSTONE);
  for (uint32_t s = 0; s < e->d.S; s++)
    if ((m >> s) & 1ull)
      for (int k = 0; k < 2; k++) put_rec(e, w, host * e->d.S + s, out, cap, n);
  if (n_out) *n_out = n;
  return GX_OK;
}

int gx_expire_server(gx_engine *e, uint32_t view, uint32_t owner, int *expired) {
  if (!e || !own(e, view) || owner >= e->d.H) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  uint32_t *dx;
  GXTRY(api_carve(e, region(dx, 1)));
  k_api_expire<<<1, 64, 0, e->stream>>>(e->d, view, owner, dx);
  uint32_t x = 0;
  int rc = read_back(e, dx, &x);
  if (!rc && expired) *expired = (int)x;
  return rc;
}

int gx_notify_leave(gx_engine *e, uint32_t view, uint32_t node) { return gx_expire_server(e, view, node, nullptr); }

int gx_send_services(gx_engine *e, uint32_t host, const gx_service *svcs, uint32_t n, uint32_t n_passes) {
  if (!e || !own(e, host) || (n && !svcs) || n_passes < 1 || n_passes > GX_JOB_MAX_PASSES) return GX_EINVAL;
  std::vector<grec> g;
  GXTRY(to_grecs(e, svcs, n, g));
  GXTRY(enter(e, ENTRY_MUTATE));
  grec *drec;
  GXTRY(api_carve(e, region(drec, n)));
  GXTRY(stage_recs(e, g, drec));
  k_api_send<<<1, 64, 0, e->stream>>>(e->d, host, drec, n, n_passes);
  return sync_check(e);
}

int gx_broadcast_services(gx_engine *e, uint32_t host, const gx_service *list, uint32_t n) {
  if (!e || !own(e, host) || (n && !list) || n > 64) return GX_EINVAL;
  for (uint32_t i = 0; i < n; i++)
    if (list[i].host != host) return GX_EINVAL;
  std::vector<grec> g;
  GXTRY(to_grecs(e, list, n, g));
  GXTRY(enter(e, ENTRY_MUTATE));
  grec *drec;
  GXTRY(api_carve(e, region(drec, n)));
  GXTRY(stage_recs(e, g, drec));
  k_api_bs<<<1, 64, 0, e->stream>>>(e->d, host, drec, n);
  return sync_check(e);
}

int gx_broadcast_tombstones(gx_engine *e, uint32_t host, const gx_service *list, uint32_t n) {
  if (!e || !own(e, host) || (n && !list)) return GX_EINVAL;
  uint64_t mask = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (list[i].host != host || list[i].svc >= e->d.S) return GX_EINVAL;
    mask |= 1ull << list[i].svc;
  }
  GXTRY(enter(e, ENTRY_MUTATE));
  uint32_t *dcnt;
  grec *dlist;
  GXTRY(api_carve(e, region(dcnt, 1), region(dlist, e->d.L)));
  scan_one_view(e, host, dlist, e->d.L, dcnt);
  k_api_bt<<<1, 64, 0, e->stream>>>(e->d, host, mask, dlist, dcnt);
  return sync_check(e);
}

int gx_owner_slots_in_use(gx_engine *e, uint32_t owner, uint64_t *mask) {
  if (!e || !mask || owner >= e->d.H) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  unsigned long long *dm;
  GXTRY(api_carve(e, region(dm, 1)));
  HIPCHK(hipMemsetAsync(dm, 0, sizeof(uint64_t), e->stream));
  k_slots_in_use<<<nblk(e->d.Hl, 256), 256, 0, e->stream>>>(e->d, owner, dm);
  HIPCHK(hipMemcpyAsync(mask, dm, sizeof(uint64_t), hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

int gx_is_new_service(gx_engine *e, uint32_t view, const gx_service *svc, int *out) {
  grec g;
  if (!e || !svc || !out || !own(e, view) || to_grec(e, svc, &g)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  uint32_t *dx;
  GXTRY(api_carve(e, region(dx, 1)));
  k_api_is_new<<<1, 64, 0, e->stream>>>(e->d, view, g.w, g.r, dx);
  uint32_t x = 0;
  int rc = read_back(e, dx, &x);
  if (!rc) *out = (int)x;
  return rc;
}

static int getb_impl(gx_engine *e, uint32_t host, uint32_t limit, uint32_t limit_bytes, uint32_t overhead,
                     gx_service *out, uint32_t *n_out) {
  GXTRY(enter(e, ENTRY_MUTATE));
  uint32_t *dn;
  grec *dpk;
  GXTRY(api_carve(e, region(dn, 1), region(dpk, limit)));
  k_api_getb<<<1, 64, 0, e->stream>>>(e->d, host, limit, dpk, dn, limit_bytes, overhead);
  uint32_t n = 0;
  GXTRY(read_back(e, dn, &n));
  GXTRY(copy_out_recs(e, dpk, n, out, limit));  // (the callers' cap >= limit >= n)
  *n_out = n;
  return GX_OK;
}

int gx_get_broadcasts(gx_engine *e, uint32_t host, uint32_t limit, gx_service *out, uint32_t cap, uint32_t *n_out) {
  if (limit == GX_LIMIT_DEFAULT) limit = e ? e->d.p.packet_cap : 0;
  if (!e || !own(e, host) || !n_out || limit > 256 || cap < limit || (limit && !out)) return GX_EINVAL;
  return getb_impl(e, host, limit, 0, 0, out, n_out);
}

int gx_get_broadcasts_bytes(gx_engine *e, uint32_t host, uint32_t overhead, uint32_t limit, gx_service *out,
                            uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, host) || !n_out || (cap && !out) || cap > (1u << 20)) return GX_EINVAL;
  if (limit == 0 || cap == 0) {  // nothing can fit: the batch still moves to pending
    return getb_impl(e, host, 0, 0, 0, out, n_out);
  }
  return getb_impl(e, host, cap, limit, overhead, out, n_out);
}

int gx_set_static_bytes(gx_engine *e, uint32_t owner_lo, uint32_t owner_hi, const uint16_t *bytes) {
  if (!e || owner_lo > owner_hi || owner_hi > e->d.H || (owner_hi > owner_lo && !bytes)) return GX_EINVAL;
  if (owner_hi == owner_lo) return GX_OK;
  GXTRY(enter(e, ENTRY_MUTATE));
  HIPCHK(hipStreamSynchronize(e->stream));
  size_t n = (size_t)(owner_hi - owner_lo) * e->d.S;
  HIPCHK(hipMemcpy(&e->d.sbytes[(size_t)owner_lo * e->d.S], bytes, sizeof(uint16_t) * n, hipMemcpyHostToDevice));
  return GX_OK;
}

int gx_message_bytes(gx_engine *e, const gx_service *recs, uint32_t n, uint32_t *out_bytes) {
  if (!e || (n && (!recs || !out_bytes))) return GX_EINVAL;
  if (!n) return GX_OK;
  std::vector<grec> g;
  GXTRY(to_grecs(e, recs, n, g));
  GXTRY(enter(e, ENTRY_READ));
  grec *dg;
  uint32_t *dout;
  GXTRY(api_carve(e, region(dg, n), region(dout, n)));
  GXTRY(stage_recs(e, g, dg));
  k_api_msg_bytes<<<nblk(n, 256), 256, 0, e->stream>>>(e->d, dg, n, dout);
  HIPCHK(hipMemcpyAsync(out_bytes, dout, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

int gx_local_state(gx_engine *e, uint32_t view, gx_service *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, view) || (cap && !out)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipStreamSynchronize(e->stream));
  std::vector<uint64_t> row(e->d.R);
  HIPCHK(hipMemcpy(row.data(), &e->d.view[(size_t)(view - e->d.lo) * e->d.R], sizeof(uint64_t) * e->d.R,
                   hipMemcpyDeviceToHost));
  uint32_t n = 0;
  for (uint32_t r = 0; r < e->d.R; r++) {
    if (st_of(row[r]) != GX_ABSENT) put_rec(e, row[r], r, out, cap, n);
  }
  if (n_out) *n_out = n;
  return GX_OK;
}

extern "C" int gx_sort_u64_pairs(void *tmp, size_t *tmp_bytes, uint64_t *keys_in, uint64_t *keys_out,
                                 uint32_t *vals_in, uint32_t *vals_out, uint32_t n, int end_bit, hipStream_t s);
extern "C" int gx_sort_u32_pairs(void *tmp, size_t *tmp_bytes, uint32_t *keys_in, uint32_t *keys_out,
                                 uint32_t *vals_in, uint32_t *vals_out, uint32_t n, int end_bit, hipStream_t s);

// EachServiceSorted / SortedServices / ByService on the device: the view's present records
// compacted in key order, stable radix sort by Updated (ties stay in key order), for ByService a
// second stable sort by the Name rank, then written out as gx_service.
static int sorted_view(gx_engine *e, uint32_t view, uint32_t owner, bool by_name, gx_service *out, uint32_t *group_out,
                       uint32_t cap, uint32_t *n_out) {
  Dev &d = e->d;
  GXTRY(enter(e, ENTRY_READ));
  hipStream_t s = e->stream;
  const uint32_t vi = view - d.lo, nb = (d.R + VC_CHUNK - 1) / VC_CHUNK;
  uint32_t *cnt = nullptr, *v0 = nullptr, *v1 = nullptr, *k32a = nullptr, *k32b = nullptr;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  gx_service *dout = nullptr;
  void *tmp = nullptr;
  uint32_t n = 0;
  DevMem mem;  // this call's temporaries, freed on every return
  GXTRY(mem.take(cnt, sizeof(uint32_t) * (nb + 1)));
  k_vc_count<<<nb, 256, 0, s>>>(d, vi, owner, cnt);
  k_vc_scan<<<1, 1024, 0, s>>>(cnt, nb);
  HIPCHK(hipMemcpyAsync(&n, &cnt[nb], sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (n) {
    GXTRY(mem.take(k0, sizeof(uint64_t) * n));
    GXTRY(mem.take(k1, sizeof(uint64_t) * n));
    GXTRY(mem.take(v0, sizeof(uint32_t) * n));
    GXTRY(mem.take(v1, sizeof(uint32_t) * n));
    GXTRY(mem.take(dout, sizeof(gx_service) * n));
    k_vc_write<<<nb, 256, 0, s>>>(d, vi, owner, cnt, k0, v0);
    size_t tb = 0, tb2 = 0;
    if (gx_sort_u64_pairs(nullptr, &tb, k0, k1, v0, v1, n, 64 - GX_TS_SHIFT, s)) return GX_EIO;
    if (by_name) {
      GXTRY(mem.take(k32a, sizeof(uint32_t) * n));
      GXTRY(mem.take(k32b, sizeof(uint32_t) * n));
      if (gx_sort_u32_pairs(nullptr, &tb2, k32a, k32b, v1, v0, n, 32, s)) return GX_EIO;
    }
    GXTRY(mem.take(tmp, std::max<size_t>(std::max(tb, tb2), 1)));
    if (gx_sort_u64_pairs(tmp, &tb, k0, k1, v0, v1, n, 64 - GX_TS_SHIFT, s)) return GX_EIO;
    uint32_t *order = v1;
    if (by_name) {
      k_vc_rank<<<nblk(n, 256), 256, 0, s>>>(e->name_rank, v1, k32a, n);
      if (gx_sort_u32_pairs(tmp, &tb2, k32a, k32b, v1, v0, n, 32, s)) return GX_EIO;
      order = v0;
    }
    k_vc_out<<<nblk(n, 256), 256, 0, s>>>(d, vi, order, n, dout);
    const uint32_t m = n < cap ? n : cap;
    if (m) {
      HIPCHK(hipMemcpyAsync(out, dout, sizeof(gx_service) * m, hipMemcpyDeviceToHost, s));
      if (by_name && group_out) HIPCHK(hipMemcpyAsync(group_out, k32b, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, s));
    }
    HIPCHK(hipStreamSynchronize(s));
    HIPCHK(hipGetLastError());
  }
  if (n_out) *n_out = n;
  return GX_OK;
}

int gx_each_service_sorted(gx_engine *e, uint32_t view, uint32_t owner, gx_service *out, uint32_t cap,
                           uint32_t *n_out) {
  if (!e || !own(e, view) || (owner != GX_ALL_OWNERS && owner >= e->d.H) || (cap && !out)) return GX_EINVAL;
  return sorted_view(e, view, owner, false, out, nullptr, cap, n_out);
}

int gx_set_service_names(gx_engine *e, const char *names, const uint64_t *off) {
  if (!e || !off) return GX_EINVAL;
  const uint32_t R = e->d.R;
  if (off[0] != 0) return GX_EINVAL;
  for (uint32_t r = 0; r < R; r++)
    if (off[r + 1] < off[r]) return GX_EINVAL;
  if (off[R] && !names) return GX_EINVAL;
  // rank = index of the record's Name among the distinct names in bytewise order
  std::vector<uint32_t> idx(R), rank(R);
  for (uint32_t r = 0; r < R; r++) idx[r] = r;
  auto name = [&](uint32_t r) { return std::string(names ? names + off[r] : "", (size_t)(off[r + 1] - off[r])); };
  std::vector<std::string> nm(R);
  for (uint32_t r = 0; r < R; r++) nm[r] = name(r);
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return nm[a] < nm[b]; });
  uint32_t g = 0;
  for (uint32_t k = 0; k < R; k++) {
    if (k && nm[idx[k]] != nm[idx[k - 1]]) g++;
    rank[idx[k]] = g;
  }
  GXTRY(enter(e, ENTRY_READ));
  if (!e->name_rank) GXTRY(e->mem.take(e->name_rank, sizeof(uint32_t) * R));
  HIPCHK(hipMemcpy(e->name_rank, rank.data(), sizeof(uint32_t) * R, hipMemcpyHostToDevice));
  return GX_OK;
}

int gx_by_service(gx_engine *e, uint32_t view, gx_service *out, uint32_t *group_out, uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, view) || (cap && !out)) return GX_EINVAL;
  if (!e->name_rank) return GX_ENOENT;
  return sorted_view(e, view, GX_ALL_OWNERS, true, out, group_out, cap, n_out);
}

int gx_epoch(gx_engine *e, int64_t *epoch_ns) {
  if (!e || !epoch_ns) return GX_EINVAL;
  *epoch_ns = e->d.epoch;
  return GX_OK;
}

int gx_read_server_times(gx_engine *e, uint32_t view, uint32_t lo, uint32_t hi, gx_server_times *out) {
  if (!e || !own(e, view) || lo > hi || hi > e->d.H || (hi > lo && !out)) return GX_EINVAL;
  if (hi == lo) return GX_OK;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, &e->d.srvt[(size_t)(view - e->d.lo) * e->d.H + lo], sizeof(gx_server_times) * (hi - lo),
                   hipMemcpyDeviceToHost));
  for (uint32_t o = 0; o < hi - lo; o++) {
    out[o].last_updated_ns = abs_tm(e, out[o].last_updated_ns);
    out[o].last_changed_ns = abs_tm(e, out[o].last_changed_ns);
  }
  return GX_OK;
}

int gx_read_last_changed(gx_engine *e, uint32_t lo, uint32_t hi, int64_t *out) {
  if (!e || lo > hi || (hi > lo && (!out || !own(e, lo) || !own(e, hi - 1)))) return GX_EINVAL;
  if (hi == lo) return GX_OK;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, &e->d.vlc[lo - e->d.lo], sizeof(int64_t) * (hi - lo), hipMemcpyDeviceToHost));
  for (uint32_t v = 0; v < hi - lo; v++) out[v] = abs_tm(e, out[v]);
  return GX_OK;
}

// Device event logs: one per listening view, sized for the largest channel capacity.
static int rebuild_logs(gx_engine *e) {
  Dev &d = e->d;
  std::vector<uint32_t> views;
  uint32_t cap = 0;
  for (auto &l : e->listeners) {
    bool seen = false;
    for (uint32_t v : views) seen |= v == l.view;
    if (!seen) views.push_back(l.view);
    cap = l.cap > cap ? l.cap : cap;
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  e->mem.drop(d.ev_log);
  e->mem.drop(d.ev_cnt);
  d.ev_cap = 0;
  HIPCHK(hipMemset(d.ev_slot, 0xff, sizeof(int32_t) * d.Hl));
  e->log_views = views;
  if (views.empty()) return GX_OK;
  int rc = e->mem.take(d.ev_log, sizeof(gx_change_event) * cap * views.size());
  if (!rc) rc = e->mem.take(d.ev_cnt, sizeof(uint32_t) * views.size(), 0, e->stream);
  if (rc) {
    e->listeners.clear();
    e->log_views.clear();
    return rc;
  }
  d.ev_cap = cap;
  for (size_t k = 0; k < views.size(); k++) {
    int32_t slot = (int32_t)k;
    HIPCHK(hipMemcpy(&d.ev_slot[views[k] - d.lo], &slot, sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return GX_OK;
}

int gx_add_listener(gx_engine *e, uint32_t view, uint32_t id, uint32_t capacity) {
  if (!e || !own(e, view) || capacity < 1 || capacity > GX_LISTENER_MAX_CAPACITY) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  bool found = false;
  for (auto &l : e->listeners)
    if (l.view == view && l.id == id) {
      l.cap = capacity;
      l.ring.clear();
      found = true;
    }
  if (!found) {
    if (e->listeners.size() >= GX_MAX_LISTENERS) return GX_ENOMEM;
    e->listeners.push_back({view, id, capacity, {}});
  }
  return rebuild_logs(e);
}

int gx_remove_listener(gx_engine *e, uint32_t view, uint32_t id) {
  if (!e) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  for (size_t i = 0; i < e->listeners.size(); i++)
    if (e->listeners[i].view == view && e->listeners[i].id == id) {
      e->listeners.erase(e->listeners.begin() + (long)i);
      return rebuild_logs(e);
    }
  return GX_ENOENT;
}

int gx_listener_drain(gx_engine *e, uint32_t view, uint32_t id, gx_change_event *out, uint32_t cap,
                      uint32_t *n_out) {
  if (!e || !n_out || (cap && !out)) return GX_EINVAL;
  for (auto &l : e->listeners)
    if (l.view == view && l.id == id) {
      uint32_t n = (uint32_t)l.ring.size() < cap ? (uint32_t)l.ring.size() : cap;
      for (uint32_t i = 0; i < n; i++) {
        out[i] = l.ring.front();
        l.ring.pop_front();
      }
      *n_out = n;
      return GX_OK;
    }
  return GX_ENOENT;
}

int gx_read_views(gx_engine *e, uint32_t lo, uint32_t hi, uint64_t *out) {
  if (!e || lo > hi || lo < e->d.lo || hi > e->d.lo + e->d.Hl || (hi > lo && !out)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (hi > lo)
    HIPCHK(hipMemcpy(out, &e->d.view[(size_t)(lo - e->d.lo) * e->d.R], sizeof(uint64_t) * (size_t)(hi - lo) * e->d.R,
                     hipMemcpyDeviceToHost));
  return GX_OK;
}

int gx_notify_msgs(gx_engine *e, const uint32_t *hosts, const gx_service *recs, uint32_t n) {
  if (!e || (n && (!hosts || !recs))) return GX_EINVAL;
  for (uint32_t i = 0; i < n;) {
    uint32_t j = i + 1;
    while (j < n && hosts[j] == hosts[i]) j++;
    int rc = gx_notify_msg(e, hosts[i], recs + i, j - i);
    if (rc) return rc;
    i = j;
  }
  return GX_OK;
}

int gx_read_view(gx_engine *e, uint32_t view, int64_t *ts_ns, uint8_t *status) {
  if (!e || !ts_ns || !status) return GX_EINVAL;
  size_t R = (size_t)e->d.R;
  uint64_t *w = (uint64_t *)malloc(8 * R);
  if (!w) return GX_ENOMEM;
  int rc = gx_read_views(e, view, view + 1, w);
  for (size_t r = 0; rc == GX_OK && r < R; r++) {
    status[r] = (uint8_t)(w[r] & 7u);
    ts_ns[r] = status[r] == GX_ABSENT ? INT64_MIN : (int64_t)(w[r] >> 3) + e->d.epoch;
  }
  free(w);
  return rc;
}

int gx_write_views(gx_engine *e, uint32_t lo, uint32_t hi, const uint64_t *in) {
  if (!e || lo > hi || lo < e->d.lo || hi > e->d.lo + e->d.Hl || (hi > lo && !in)) return GX_EINVAL;
  size_t n = (size_t)(hi - lo) * e->d.R;
  for (size_t i = 0; i < n; i++)
    if (st_of(in[i]) == 7 && in[i] != GX_SLOT_ABSENT) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (n) HIPCHK(hipMemcpy(&e->d.view[(size_t)(lo - e->d.lo) * e->d.R], in, sizeof(uint64_t) * n, hipMemcpyHostToDevice));
  k_api_mark<<<1, 64, 0, e->stream>>>(e->d);
  if (hi > lo) k_minexp_recompute<<<hi - lo, 256, 0, e->stream>>>(e->d, lo - e->d.lo);
  return sync_check(e);
}

int gx_write_slot(gx_engine *e, uint32_t view, const gx_service *svc) {
  if (!e || !svc || !own(e, view)) return GX_EINVAL;
  uint64_t w;
  uint32_t r;
  if (svc->status == GX_ABSENT) {
    if (svc->host >= e->d.H || svc->svc >= e->d.S) return GX_EINVAL;
    w = GX_SLOT_ABSENT;
    r = svc->host * e->d.S + svc->svc;
  } else {
    grec g;
    if (to_grec(e, svc, &g)) return GX_EINVAL;
    w = g.w;
    r = g.r;
  }
  GXTRY(enter(e, ENTRY_MUTATE));
  k_api_set_slot<<<1, 64, 0, e->stream>>>(e->d, view, r, w);
  return sync_check(e);
}

int gx_read_hosts(gx_engine *e, uint32_t lo, uint32_t hi, gx_host_state *out) {
  if (!e || lo > hi || lo < e->d.lo || hi > e->d.lo + e->d.Hl || (hi > lo && !out)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipStreamSynchronize(e->stream));
  if (hi > lo) HIPCHK(hipMemcpy(out, &e->d.hs[lo - e->d.lo], sizeof(gx_host_state) * (hi - lo), hipMemcpyDeviceToHost));
  return GX_OK;
}

int gx_read_queue(gx_engine *e, uint32_t host, gx_job *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, host) || (cap && !out)) return GX_EINVAL;
  gx_host_state h;
  int rc = gx_read_hosts(e, host, host + 1, &h);
  if (rc) return rc;
  uint32_t n = h.fifo_stored - h.fifo_head;  // the stored jobs (gx.h)
  rc = read_ring(&e->d.fifo[(size_t)(host - e->d.lo) * e->d.Q], e->d.Q, h.fifo_head % e->d.Q, n, out, cap);
  if (rc) return rc;
  if (n_out) *n_out = n;
  return GX_OK;
}

int gx_read_sleepers(gx_engine *e, uint32_t host, gx_sleeper *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, host) || (cap && !out)) return GX_EINVAL;
  gx_host_state h;
  int rc = gx_read_hosts(e, host, host + 1, &h);
  if (rc) return rc;
  uint32_t n = h.sleep_tail - h.sleep_head;
  rc = read_ring(&e->d.sleep[(size_t)(host - e->d.lo) * e->d.SQ], e->d.SQ, h.sleep_head % e->d.SQ, n, out, cap);
  if (rc) return rc;
  if (n_out) *n_out = n;
  return GX_OK;
}

int gx_read_pending(gx_engine *e, uint32_t host, gx_service *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, host) || (cap && !out)) return GX_EINVAL;
  gx_host_state h;
  int rc = gx_read_hosts(e, host, host + 1, &h);
  if (rc) return rc;
  GXTRY(copy_out_recs(e, &e->d.dq[(size_t)(host - e->d.lo) * e->d.DQ], h.dq_len, out, cap, e->d.DQ,
                      h.dq_head & (e->d.DQ - 1)));
  if (n_out) *n_out = h.dq_len;
  return GX_OK;
}

int gx_read_list(gx_engine *e, uint32_t host, uint32_t slot, gx_service *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !own(e, host) || slot >= e->d.A || (cap && !out)) return GX_EINVAL;
  gx_host_state h;
  int rc = gx_read_hosts(e, host, host + 1, &h);
  if (rc) return rc;
  uint32_t n = 0, bits = 0;
  HIPCHK(hipMemcpy(&bits, &e->d.arena_bits[(size_t)(host - e->d.lo) * e->d.AW + slot / 32], sizeof(uint32_t),
                   hipMemcpyDeviceToHost));
  if ((bits >> (slot % 32)) & 1u)
    HIPCHK(hipMemcpy(&n, &e->d.arena_len[(size_t)(host - e->d.lo) * e->d.A + slot], sizeof(uint32_t), hipMemcpyDeviceToHost));
  GXTRY(copy_out_recs(e, &e->d.arena[((size_t)(host - e->d.lo) * e->d.A + slot) * e->d.L], n, out, cap));
  if (n_out) *n_out = n;
  return GX_OK;
}

int gx_host_digests(gx_engine *e, uint64_t *out) {
  if (!e || !out) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  k_digest<<<nblk(e->d.Hl, 256), 256, 0, e->stream>>>(e->d, e->digest_buf);
  HIPCHK(hipMemcpyAsync(out, e->digest_buf, sizeof(uint64_t) * e->d.Hl, hipMemcpyDeviceToHost, e->stream));
  return sync_check(e);
}

int gx_owner_words(gx_engine *e, uint64_t *out) {
  if (!e || !out) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  k_owner_words<<<nblk(e->d.R, 256), 256, 0, e->stream>>>(e->d, out);
  return sync_check(e);
}

int gx_view_minmax(gx_engine *e, uint64_t *mn, uint64_t *mx) {
  if (!e || !mn || !mx) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  k_view_minmax<<<nblk(e->d.R, 256), 256, 0, e->stream>>>(e->d, mn, mx);
  return sync_check(e);
}

static int read_ctr(gx_engine *e, unsigned long long *c, unsigned long long *last_p1, unsigned long long *bytes,
                    unsigned long long *units, unsigned long long *first_drop = nullptr,
                    unsigned long long *first_locked = nullptr) {
  std::vector<DevCtr> tmp(1);
  HIPCHK(hipMemcpyAsync(tmp.data(), e->d.ctr, sizeof(DevCtr), hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  const DevCtr &x = tmp[0];
  for (int i = 0; i < GX_NCTR_SLOTS; i++) c[i] = 0;
  for (int i = 0; i < 16; i++) bytes[i] = units[i] = 0;
  *last_p1 = 0;
  if (first_drop) *first_drop = ~0ull;
  if (first_locked) *first_locked = ~0ull;
  for (int s = 0; s < GX_SHARDS; s++) {
    if (first_drop && x.first_drop[s][0] < *first_drop) *first_drop = x.first_drop[s][0];
    if (first_locked && x.first_drop[s][1] < *first_locked) *first_locked = x.first_drop[s][1];
    for (int i = 0; i < GX_NCTR_SLOTS; i++) c[i] += x.c[s][i];
    for (int i = 0; i < 16; i++) {
      bytes[i] += x.bytes[s][i];
      units[i] += x.units[s][i];
    }
    if (x.last_change_p1[s][0] > *last_p1) *last_p1 = x.last_change_p1[s][0];
  }
  return GX_OK;
}

int gx_stats_get(gx_engine *e, gx_stats *out) {
  if (!e || !out) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  unsigned long long c[GX_NCTR_SLOTS], lp1, bytes[16], units[16], fdr, flr;
  int rc = read_ctr(e, c, &lp1, bytes, units, &fdr, &flr);
  if (rc) return rc;
  memset(out, 0, sizeof(*out));
  out->queue_deferred = c[C_QDEFER];
  out->locked_merges = c[C_LOCKED_MERGES];
  out->first_locked_round = flr == ~0ull ? -1 : (int64_t)flr;
  out->lock_buffered = c[C_LOCK_BUF];
  out->lock_drops = c[C_LOCK_DROP];
  out->lock_drained = c[C_LOCK_DRAIN];
  out->ae_locked = c[C_AE_LOCKED];
  out->expire_deferred = c[C_EXP_DEFER];
  out->ae_deferred = c[C_AE_DEFER];
  out->ae_defer_lost = c[C_AE_DEFER_LOST];
  out->fd_handoff_queued = c[C_FD_HQ];
  out->fd_handoff_drops = c[C_FD_HQ_DROP];
  out->false_expiries = c[C_FEXP];
  out->first_drop_round = fdr == ~0ull ? -1 : (int64_t)fdr;
  out->lost_packets = c[C_LOST];
  out->fd_probes = c[C_FD_PROBES];
  out->fd_probe_failures = c[C_FD_PROBE_FAIL];
  out->fd_suspicions = c[C_FD_SUSPECT];
  out->fd_confirmations = c[C_FD_CONFIRM];
  out->fd_deaths = c[C_FD_DEATH];
  out->fd_refutes = c[C_FD_REFUTE];
  out->fd_alive_updates = c[C_FD_ALIVE];
  out->fd_msgs_sent = c[C_FD_SENT];
  out->fd_msgs_received = c[C_FD_RECV];
  out->fd_state_merges = c[C_FD_STATE_MERGE];
  out->round = e->d.round;
  out->gossip_merges = c[C_GOSSIP_MERGES];
  out->ae_merges = c[C_AE_MERGES];
  out->local_merges = c[C_LOCAL_MERGES];
  out->gossip_accepts = c[C_GOSSIP_ACC];
  out->ae_accepts = c[C_AE_ACC];
  out->local_accepts = c[C_LOCAL_ACC];
  out->stale_drops = c[C_STALE];
  out->retransmits = c[C_RETX];
  out->queue_drops = c[C_QDROP];
  out->list_drops = c[C_LDROP];
  out->sleep_drops = c[C_SDROP];
  out->pending_drops = c[C_PDROP];
  out->dequeues = c[C_DEQ];
  out->nil_batches = c[C_NIL];
  out->packets = c[C_PACKETS];
  out->records_sent = c[C_RECSENT];
  out->expired = c[C_EXPIRED];
  out->gc = c[C_GC];
  out->own_tombstones = c[C_OWNTOMB];
  out->expire_server = c[C_EXPSRV];
  out->send_jobs = c[C_SENDJOBS];
  out->ae_exchanges = c[C_AEX];
  out->churn_events = c[C_CHURN];
  out->change_events = c[C_CHG];
  out->listener_drops = e->listener_drops;
  out->bytes_sent = c[C_BYTESENT];
  out->cap_cuts = c[C_CAPCUT];
  out->scan_slots = c[C_SCANSLOTS];
  out->ae_slots = c[C_AESLOTS];
  out->last_change_round = (int64_t)lp1 - 1;
  return GX_OK;
}

int gx_timing_get(gx_engine *e, gx_timing *out) {
  if (!e || !out) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  int rc = drain_timing(e);
  if (rc) return rc;
  unsigned long long c[GX_NCTR_SLOTS], lp1, bytes[16], units[16];
  rc = read_ctr(e, c, &lp1, bytes, units);
  if (rc) return rc;
  memset(out, 0, sizeof(*out));
  for (int i = 0; i < GX_K_COUNT; i++) {
    out->ms[i] = e->ms[i];
    out->launches[i] = e->launches[i];
    const bool host = i == GX_K_ENCODE || i == GX_K_DECODE;  // codec classes: accounted on the host
    out->bytes[i] = host ? e->host_bytes[i] : bytes[i];
    out->units[i] = host ? e->host_units[i] : units[i];
  }
  return GX_OK;
}

// ------------------------------------------------------- memberlist failure detection ----
static bool fd_ok(const gx_engine *e, uint32_t host) { return e && e->d.p.fd_enable && own(e, host); }

int gx_fd_read_members(gx_engine *e, uint32_t host, uint32_t lo, uint32_t hi, gx_member *out) {
  if (!fd_ok(e, host) || lo > hi || hi > e->d.H || (!out && hi > lo)) return GX_EINVAL;
  if (hi == lo) return GX_OK;
  GXTRY(enter(e, ENTRY_READ));
  const Dev &d = e->d;
  std::vector<int32_t> dl(hi - lo);
  HIPCHK(hipMemcpyAsync(out, &d.mem[(size_t)(host - d.lo) * d.H + lo], sizeof(gx_member) * (hi - lo),
                        hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(dl.data(), &d.fd_dl[(size_t)(host - d.lo) * d.H + lo], sizeof(int32_t) * (hi - lo),
                        hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  for (uint32_t i = 0; i < hi - lo; i++) out[i].deadline = dl[i];
  return GX_OK;
}

int gx_fd_read_hosts(gx_engine *e, uint32_t lo, uint32_t hi, gx_fd_host *out) {
  if (!e || !e->d.p.fd_enable || lo > hi || (hi > lo && (!own(e, lo) || !own(e, hi - 1))) || (!out && hi > lo))
    return GX_EINVAL;
  if (hi == lo) return GX_OK;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipMemcpyAsync(out, &e->d.fdh[lo - e->d.lo], sizeof(gx_fd_host) * (hi - lo), hipMemcpyDeviceToHost,
                        e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  for (uint32_t v = lo; v < hi; v++) out[v - lo].departed = departed_at(e->d.p, e->d.round, v) ? 1u : 0u;
  return GX_OK;
}

int gx_fd_read_queue(gx_engine *e, uint32_t host, gx_fd_msg *out, uint8_t *transmits, uint32_t cap,
                     uint32_t *n_out) {
  if (!fd_ok(e, host) || !n_out) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  const Dev &d = e->d;
  std::vector<gx_member> row(d.H);
  gx_fd_host h;
  HIPCHK(hipMemcpyAsync(row.data(), &d.mem[(size_t)(host - d.lo) * d.H], sizeof(gx_member) * d.H,
                        hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(&h, &d.fdh[host - d.lo], sizeof(gx_fd_host), hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  uint32_t n = 0;
  for (uint32_t b = 0; b < d.p.fd_retransmit_limit; b++)
    for (uint32_t m = h.q_head[b]; m != GX_FD_NONE && n <= d.H; m = row[m].q_next) {
      if (n < cap) {
        if (out) {
          gx_fd_msg g = {};
          g.incarnation = row[m].msg_incarnation;
          g.node = (uint16_t)m;
          g.from = row[m].msg_from;
          g.kind = row[m].msg_kind;
          out[n] = g;
        }
        if (transmits) transmits[n] = (uint8_t)b;
      }
      n++;
    }
  *n_out = n;
  return GX_OK;
}

int gx_fd_notify(gx_engine *e, uint32_t host, const gx_fd_msg *msgs, uint32_t n) {
  if (!fd_ok(e, host) || (!msgs && n)) return GX_EINVAL;
  for (uint32_t i = 0; i < n; i++)
    if (msgs[i].node >= e->d.H || msgs[i].kind > GX_M_DEAD) return GX_EINVAL;
  if (!n) return GX_OK;
  GXTRY(enter(e, ENTRY_MUTATE));
  gx_fd_msg *dm;
  GXTRY(api_carve(e, region(dm, n)));
  HIPCHK(hipMemcpyAsync(dm, msgs, sizeof(gx_fd_msg) * n, hipMemcpyHostToDevice, e->stream));
  k_fd_api_notify<<<1, 64, 0, e->stream>>>(e->d, host, dm, n);
  return sync_check(e);
}

int gx_fd_get_broadcasts(gx_engine *e, uint32_t host, uint32_t limit, gx_fd_msg *out, uint32_t *n_out) {
  if (!fd_ok(e, host) || !n_out || limit > 64 || (!out && limit)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  uint32_t *dn;
  gx_fd_msg *dm;
  GXTRY(api_carve(e, region(dn, 1), region(dm, 64)));
  k_fd_api_getb<<<1, 64, 0, e->stream>>>(e->d, host, limit, dm, dn);
  uint32_t n = 0;
  GXTRY(read_back(e, dn, &n));
  if (n) {
    HIPCHK(hipMemcpyAsync(out, dm, sizeof(gx_fd_msg) * n, hipMemcpyDeviceToHost, e->stream));
    GXTRY(sync_check(e));
  }
  *n_out = n;
  return GX_OK;
}

int gx_fd_probe(gx_engine *e, uint32_t host, uint32_t *target, int *acked) {
  if (!fd_ok(e, host)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  uint32_t *dx;
  GXTRY(api_carve(e, region(dx, 2)));
  k_fd_api_probe<<<1, 64, 0, e->stream>>>(e->d, host, dx);
  uint32_t x[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(x, dx, sizeof(x), hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  if (target) *target = x[0];
  if (acked) *acked = (int)x[1];
  return GX_OK;
}

int gx_fd_timers(gx_engine *e, uint32_t host) {
  if (!fd_ok(e, host)) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  k_fd_api_timers<<<1, 64, 0, e->stream>>>(e->d, host);
  return sync_check(e);
}

int gx_fd_merge_state(gx_engine *e, uint32_t host, const uint64_t *remote) {
  if (!fd_ok(e, host) || !remote) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  uint64_t *dr;
  GXTRY(api_carve(e, region(dr, e->d.H)));
  HIPCHK(hipMemcpyAsync(dr, remote, sizeof(uint64_t) * e->d.H, hipMemcpyHostToDevice, e->stream));
  k_fd_api_merge_state<<<1, 64, 0, e->stream>>>(e->d, host, dr);
  return sync_check(e);
}

int gx_fd_converged(gx_engine *e, int *converged, uint64_t *n_disagree) {
  if (!e || !e->d.p.fd_enable) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipMemsetAsync(e->conv_bad, 0, sizeof(unsigned long long), e->stream));
  k_fd_converged<<<nblk(e->d.H, 256), 256, 0, e->stream>>>(e->d, e->conv_bad);
  unsigned long long bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, e->conv_bad, sizeof(bad), hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  if (converged) *converged = bad == 0;
  if (n_disagree) *n_disagree = bad;
  return GX_OK;
}

// Diagnostics outside gx.h: out[0] = gx_exchange_plan calls that found their batch of slot bounds
// not computed yet and waited on the host, out[1] = all calls.
int gx_xplan_waits(gx_engine *e, uint64_t *out) {
  if (!e || !out) return GX_EINVAL;
  out[0] = e->xplan_waits[0];
  out[1] = e->xplan_waits[1];
  return GX_OK;
}

// Diagnostics outside gx.h: the non-empty probe ping packets (out[0]) and ack packets (out[1]) this
// engine has sent to hosts of other shards since create (gx.h probe_piggyback; k_probe counts them).
// Zeros on an unsharded engine and with probe_piggyback = 0. Waits for the device.
int gx_probe_cross(gx_engine *e, uint64_t *out) {
  if (!e || !out) return GX_EINVAL;
  out[0] = out[1] = 0;
  if (!e->d.probe_x) return GX_OK;
  GXTRY(enter(e, ENTRY_READ));
  unsigned long long c[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(c, e->d.probe_x, sizeof(c), hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  out[0] = c[0];
  out[1] = c[1];
  return GX_OK;
}

// Diagnostics outside gx.h (env GX_KPROF at gx_create): the wall-clock phase marks (100 MHz) of the
// last k_send launch, 8 per wave: start, ticks done, block barrier, sends begin, send_host begin,
// first chunk planned, first chunk's records stored, sends done (0 = not reached).
int gx_kprof_read(gx_engine *e, uint64_t *out, uint64_t cap, uint64_t *n_out) {
  if (!e || !n_out) return GX_EINVAL;
  *n_out = e->kprof_n;
  if (!e->kprof_n || !out) return GX_OK;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipStreamSynchronize(e->stream));
  HIPCHK(hipMemcpy(out, e->d.kprof, sizeof(uint64_t) * (cap < e->kprof_n ? cap : e->kprof_n), hipMemcpyDeviceToHost));
  return GX_OK;
}

int gx_converged(gx_engine *e, int *converged, uint64_t *n_disagree) {
  if (!e || e->d.G > 1) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  HIPCHK(hipMemsetAsync(e->conv_bad, 0, sizeof(unsigned long long), e->stream));
  {
    LaunchTimer t(e, GX_K_CONVERGE);
    k_converged<<<nblk(e->d.R, 256), 256, 0, e->stream>>>(e->d, e->conv_bad);
  }
  unsigned long long bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, e->conv_bad, sizeof(bad), hipMemcpyDeviceToHost, e->stream));
  int rc = sync_check(e);
  if (rc) return rc;
  if (converged) *converged = bad == 0;
  if (n_disagree) *n_disagree = bad;
  return GX_OK;
}

}  // extern "C"
