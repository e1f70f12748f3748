/* gx_watch.h — record watch: per-round spread counts for chosen records, kept on the device.
 *
 * Symbols of the HIP engine beside include/gx.h (the CPU oracle has none of them, like
 * gx_ae_batches and gx_probe_cross; GX_ABI_VERSION counts gx.h alone). A caller names up to
 * GX_WATCH_MAX records, each with a version (a threshold on Updated). While the watch is armed every
 * round ends with one more kernel, which counts for each entry, over this engine's views, how many
 * hold the version and how many hold an older one, into a per-round log in device memory. The
 * watch is read-only: it changes nothing a round computes, and with no watch armed nothing is
 * launched for it.
 *
 * Entry i is (key, min_updated_ns). key = host * S + svc < R names the record; key == GX_WATCH_OFF
 * disables the entry (it logs zeros; its time is not looked at). Entries with the same key are
 * independent. min_updated_ns is an absolute time like gx_service.updated_ns and must lie in the
 * engine's time window (gx.h GX_TS_SHIFT; GX_EINVAL otherwise); INT64_MIN stands for "any
 * version": every present slot holds.
 *
 * Counts of round n: the views as the round's last phase left them, taken before the round number
 * becomes n + 1, over the views of this engine's hosts that have not departed by round n (the rule
 * of gx_view_minmax):
 *   holds  views whose slot of the record is present (status != GX_ABSENT; a tombstone is present)
 *          with Updated >= min_updated_ns
 *   older  views whose slot is present with Updated < min_updated_ns
 *   live   the views counted, once per round; live - holds - older views hold no record
 * Every way a round ends logs once: gx_run_rounds' rounds (quiet ones too), gx_round_end, and
 * gx_round_gossip_end when it ends the round. gx_set_round logs nothing: the rows of rounds jumped
 * over stay zero (live = 0).
 * A sharded engine counts its own views; a key's owner need not be one of its hosts. The
 * cluster's counts are the sums over the shards' logs. No round gains a collective. */
#ifndef GX_WATCH_H
#define GX_WATCH_H

#include "gx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GX_WATCH_MAX 1024u
#define GX_WATCH_OFF 0xffffffffu
#define GX_WATCH_LOG_MAX_BYTES ((uint64_t)256 << 20)

typedef struct gx_watch_count {
  uint32_t holds, older;
} gx_watch_count;

/* Allocates a watch of n entries (all off) with a zeroed log of log_rounds rows and starts it: row
 * k is round first_round + k, first_round = the round that ends next. A watch armed before is
 * dropped with its log. n = 0 disarms and frees (fine without a watch). GX_EINVAL for n >
 * GX_WATCH_MAX, log_rounds = 0 with n > 0, or a log, log_rounds * (n + 1) * 8 bytes, past
 * GX_WATCH_LOG_MAX_BYTES. Rounds that end past the log's last row are not written; they are
 * counted (missed). gx_destroy frees an armed watch. */
int gx_watch_arm(gx_engine *e, uint32_t n, uint32_t log_rounds);
/* Rewrites entries [first, first + count) from keys[count] and min_updated_ns[count] (host memory).
 * The log is left as it is; the new entries count from the next round end on. GX_EINVAL without a
 * watch, for a range past n, a key that is neither < R nor GX_WATCH_OFF, or a time outside the
 * window (nothing is rewritten then). */
int gx_watch_set(gx_engine *e, uint32_t first, const uint32_t *keys, const int64_t *min_updated_ns, uint32_t count);
/* Waits for the device and copies log rows [row, row + rows) out (host memory): counts[rows][n] and
 * live[rows]; both may be null when rows = 0. Always fills info[3] = {first_round, n_logged, missed}:
 * n_logged = rows whose round has ended, min(round - first_round, log_rounds). GX_EINVAL without a
 * watch or for rows past n_logged. */
int gx_watch_read(gx_engine *e, uint32_t row, uint32_t rows, gx_watch_count *counts, uint32_t *live, int64_t *info);

#ifdef __cplusplus
}
#endif
#endif
