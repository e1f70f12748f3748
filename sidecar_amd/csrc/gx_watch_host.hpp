// gx_watch_host.hpp — the record watch of include/gx_watch.h: gx_watch_arm, gx_watch_set,
// gx_watch_read. Included by gx_engine.hip, which keeps the watch's state (gx_engine::Watch) and the
// round-end hook that launches k_watch (watch_round_end).

static void watch_free(gx_engine *e) {
  gx_engine::Watch &w = e->watch;
  e->mem.drop(w.keys);
  e->mem.drop(w.thr);
  e->mem.drop(w.log);
  w = gx_engine::Watch{};
}

extern "C" {

int gx_watch_arm(gx_engine *e, uint32_t n, uint32_t log_rounds) {
  if (!e || n > GX_WATCH_MAX || (n && !log_rounds)) return GX_EINVAL;
  const uint64_t row_bytes = 8ull * (n + 1);
  if (n && log_rounds > GX_WATCH_LOG_MAX_BYTES / row_bytes) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_MUTATE));
  // a launch queued for the old watch still reads its buffers
  GXTRY(sync_check(e));
  watch_free(e);
  if (!n) return GX_OK;
  gx_engine::Watch &w = e->watch;
  hipStream_t s = e->stream;
  int rc = e->mem.take(w.keys, sizeof(uint32_t) * n, 0xff, s);  // GX_WATCH_OFF
  if (!rc) rc = e->mem.take(w.thr, sizeof(uint64_t) * n, 0, s);
  if (!rc) rc = e->mem.take(w.log, row_bytes * log_rounds, 0, s);
  if (rc) {
    watch_free(e);
    return rc;
  }
  w.keys_host.assign(n, GX_WATCH_OFF);
  w.thr_host.assign(n, 0);
  w.n = n;
  w.log_rounds = log_rounds;
  w.first_round = e->d.round;
  return GX_OK;
}

int gx_watch_set(gx_engine *e, uint32_t first, const uint32_t *keys, const int64_t *min_updated_ns, uint32_t count) {
  if (!e || !e->watch.n || first > e->watch.n || count > e->watch.n - first) return GX_EINVAL;
  if (count && (!keys || !min_updated_ns)) return GX_EINVAL;
  const Dev &d = e->d;
  gx_engine::Watch &w = e->watch;
  std::vector<uint64_t> thr(count);
  for (uint32_t i = 0; i < count; i++) {
    if (keys[i] == GX_WATCH_OFF) continue;  // (its time is not looked at)
    if (keys[i] >= d.R) return GX_EINVAL;
    const int64_t t = min_updated_ns[i];
    if (t == INT64_MIN) continue;  // the window's start: every present slot holds
    if (t < d.epoch || t - d.epoch >= GX_TS_LIMIT) return GX_EINVAL;
    thr[i] = pack(t - d.epoch, 0);
  }
  GXTRY(enter(e, ENTRY_MUTATE));
  if (!count) return GX_OK;
  // staged from the watch's own copy of the entries, which outlives the call
  std::copy(keys, keys + count, w.keys_host.begin() + first);
  std::copy(thr.begin(), thr.end(), w.thr_host.begin() + first);
  HIPCHK(hipMemcpyAsync(w.keys + first, &w.keys_host[first], sizeof(uint32_t) * count, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(w.thr + first, &w.thr_host[first], sizeof(uint64_t) * count, hipMemcpyHostToDevice, e->stream));
  return GX_OK;
}

int gx_watch_read(gx_engine *e, uint32_t row, uint32_t rows, gx_watch_count *counts, uint32_t *live, int64_t *info) {
  if (!e || !e->watch.n || !info || (rows && (!counts || !live))) return GX_EINVAL;
  const gx_engine::Watch &w = e->watch;
  const int64_t ended = e->d.round - w.first_round;
  const uint32_t n_logged = ended < (int64_t)w.log_rounds ? (uint32_t)ended : w.log_rounds;
  if (row > n_logged || rows > n_logged - row) return GX_EINVAL;
  GXTRY(enter(e, ENTRY_READ));
  const size_t rw = 2 * ((size_t)w.n + 1);  // words per log row
  std::vector<uint32_t> tmp(rw * rows);
  if (rows)
    HIPCHK(hipMemcpyAsync(tmp.data(), w.log + rw * row, sizeof(uint32_t) * rw * rows, hipMemcpyDeviceToHost, e->stream));
  GXTRY(sync_check(e));
  for (uint32_t k = 0; k < rows; k++) {
    memcpy(counts + (size_t)k * w.n, &tmp[rw * k], sizeof(gx_watch_count) * w.n);
    live[k] = tmp[rw * k + 2 * w.n];
  }
  info[0] = w.first_round;
  info[1] = n_logged;
  info[2] = (int64_t)w.missed;
  return GX_OK;
}

}  // extern "C"
