/* gx_ckpt.h — engine checkpoints: save an engine between two rounds, restore it, fork it.
 *
 * Symbols of the HIP engine beside include/gx.h (the CPU oracle has none of them, like gx_watch.h;
 * GX_ABI_VERSION counts gx.h alone). A checkpoint is the state between two rounds that determines
 * every later round and every read-back: the round, gx_params and every engine buffer that carries
 * state across rounds (class STATE; the table is in DESIGN.md "Checkpoints"). Buffers that some
 * kernel rewrites before anything reads them (class DERIVED) are not saved: after a load they are
 * exactly as gx_create left them. An engine restored from a file continues bit for bit as the saved
 * one would have.
 *
 * Not part of a checkpoint; the caller sets these again after a load: the stream mode
 * (gx_set_stream), listeners and their device logs, the record watch (gx_watch.h), the codec's name
 * tables (gx_set_names, gx_set_service_names). Static record sizes (gx_set_static_bytes) are state
 * and are saved. Saving with listeners or a watch registered is allowed and ignores them. The
 * host side of a loaded engine is a fresh engine's with the round set: no quiet-round bound, the
 * default scan placement, no planned-exchange batch, no push-pull schedule or chain step, timing off
 * and zeroed.
 *
 * When: only between rounds. gx_round_send and gx_round_gossip_begin open a round; gx_round_end, and
 * a gx_round_gossip_end that ends the round, close it. gx_ckpt_save answers GX_EINVAL while a round
 * is open or shard-local push-pull merges are still pending. Save reads only: it changes nothing a
 * round computes and keeps the quiet-round bounds, so a run that saves equals one that does not. A
 * sharded engine saves its own shard to its own file; no call here is a collective.
 *
 * FILE (little-endian, everything 8-byte aligned)
 *   header, GX_CKPT_HEADER_BYTES + pad8(sizeof(gx_params)) bytes:
 *     u64 magic GX_CKPT_MAGIC     u32 format GX_CKPT_FORMAT     u32 GX_ABI_VERSION
 *     u32 sizeof(gx_params)       u32 n_sections                i64 round
 *     u64 checksum of the header with this field 0, followed by the section table
 *     gx_params as the engine was created with (absolute t0_ns), zero-padded to 8 bytes
 *   section table, n_sections entries of 32 bytes, ascending id:
 *     u32 id (GX_CK_*)   u32 coding (GX_CKPT_RAW, GX_CKPT_VIEWS)   u64 raw bytes   u64 stored bytes
 *     u64 checksum of the stored bytes
 *   the sections' stored bytes in table order, each zero-padded to 8 bytes (the padding is not
 *   counted in stored bytes and not checksummed)
 * Checksum of n bytes: the bytes as u64 words w[0..ceil(n / 8)) (the last zero-padded); with
 *   m(i) = w[i] ^ ((i + 1) * 0x9E3779B97F4A7C15),  m ^= m >> 32,  m *= 0xD6E8FEB86659FD93,  m ^= m >> 32
 * the checksum is (sum of m(i) mod 2^64) ^ n. Every single changed word changes it.
 * Every section is stored raw (the buffer's bytes) except the views.
 *
 * VIEW SECTION (coding GX_CKPT_VIEWS; raw bytes = 8 * Hl * R). R = n_hosts * n_services slots per
 * view, Hl views (this engine's hosts, departed ones included), nblk = ceil(R / 512) blocks of
 * GX_DIGEST_SLOTS slots. First base[R] (u64): base[r] = the unsigned maximum of word r over the Hl
 * views. Then one record per view in ascending view order:
 *     u64 n_lit                      literals of this view; UINT64_MAX = stored raw: R words follow, nothing else
 *     u64 present[ceil(nblk / 64)]   bit b: block b has a slot that differs from base
 *     u64 mask[8] per present block  bit i: slot 512 b + i < R and word != base[slot]; bits past R are 0
 *     u64 literal per mask bit       the view's words, ascending slot order
 * A view is stored raw exactly when its coded record, 8 * (1 + ceil(nblk / 64) + 8 * present blocks
 * + n_lit) bytes, would not be smaller than 8 * R bytes. A warm cluster's views all equal base: the
 * section is 8 R + Hl * 8 * (1 + ceil(nblk / 64)) bytes.
 *
 * MEMORY. Save and load stream through one staging area on the device (a chunk of view records)
 * and two halves in pinned host memory (one is written to the file or read from it while the other
 * is copied), each the largest piece the engine has and GX_CKPT_STAGE_BYTES at most: 256 MiB on the
 * device and 512 MiB pinned at the most, under the 1 GiB this design was given. A chunk is as many
 * views as fit the area at their worst case, 8 + 8 R bytes each; an engine whose single view record
 * exceeds the area (R > 2^25) is GX_ENOMEM. Beyond that both directions allocate the base row (8 R
 * bytes) and 12 bytes per (view, block) of a chunk on the device, and load the new engine. Nothing
 * proportional to the views is allocated on either side.
 *
 * FORK. gx_ckpt_load's `override` may differ from the saved params only in device, partition_start /
 * partition_end, storm_round, depart_round / depart_ppm, and an event (the partition, the storm, the
 * departures) may differ only while neither its saved nor its new form has begun at the saved
 * round: it begins at partition_start, storm_round or depart_round, so it has begun when that round
 * is at or before the saved one (the round that runs next); -1 never begins, nor do departures with
 * depart_ppm = 0 or a partition whose window is empty. No field of these is refused outright: none
 * shapes state before its event begins (an engine with departures scheduled takes k_send's generic
 * instead of its planned instance; both compute the oracle's rounds, tests/test_gpu_send_variants.py,
 * and the fork tests cross from one to the other).
 * Before its start an event changes nothing, so the fork equals a
 * run of the new schedule from round 0. The engine is created from the new params; a section the file
 * lacks (pexp when a storm is added) keeps its gx_create state, a section the new engine lacks is
 * skipped (it can only hold its initial state). Any other difference is GX_EINVAL. */
#ifndef GX_CKPT_H
#define GX_CKPT_H

#include "gx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GX_CKPT_MAGIC 0x31304b4358474b43ull /* "CKGXCK01" */
#define GX_CKPT_FORMAT 1u
#define GX_CKPT_HEADER_BYTES 40u
#define GX_CKPT_RAW 0u
#define GX_CKPT_VIEWS 1u
#define GX_CKPT_STAGE_BYTES ((uint64_t)256 << 20) /* the device staging area, and each of the two pinned halves */
#define GX_CKPT_MAX_SECTIONS 64u

/* Section ids: one per STATE buffer of the engine. Ids are never reused. */
enum {
  GX_CK_VIEW = 1, GX_CK_OWN_STATUS, GX_CK_HS, GX_CK_FIFO, GX_CK_SLEEP, GX_CK_DQ, GX_CK_ARENA, GX_CK_ARENA_LEN,
  GX_CK_ARENA_BITS, GX_CK_MSG, GX_CK_MSG_W0, GX_CK_MSG_LEN, GX_CK_MSG_DST, GX_CK_MSG_KEY, GX_CK_IN_CNT,
  GX_CK_IN_HDR, GX_CK_IN_OVF, GX_CK_IN_REC, GX_CK_WORK_CNT, GX_CK_WORK, GX_CK_MREC, GX_CK_MINEXP, GX_CK_SCAN_LIST,
  GX_CK_SCAN_CNT, GX_CK_TICK, GX_CK_SBYTES, GX_CK_SRVT, GX_CK_VLC, GX_CK_CTR, GX_CK_MEM, GX_CK_FD_DL, GX_CK_FDH,
  GX_CK_FDM, GX_CK_FD_LEN, GX_CK_FD_PEERS, GX_CK_FD_NP, GX_CK_FD_SNAP, GX_CK_LKB, GX_CK_PEXP, GX_CK_DPOOL,
  GX_CK_DPOOL_HOST, GX_CK_DPOOL_RES, GX_CK_DSLOT, GX_CK_FDQ, GX_CK_IN_STAMP, GX_CK_PROBE_X, GX_CK_RO_XC,
  GX_CK_ID_END
};

typedef struct gx_ckpt_section {
  uint32_t id, coding;
  uint64_t raw_bytes, stored_bytes;
} gx_ckpt_section;

typedef struct gx_ckpt_info {
  uint32_t n_sections, pad;
  uint64_t raw_bytes, stored_bytes; /* totals over the sections */
  uint64_t file_bytes;
  /* device time of the view coder (HIP events around its kernels, summed over the chunks): save:
   * base reduction, count + scan, emit; load: validate + scan, expand */
  float coder_ms, base_ms, count_ms, emit_ms;
  uint32_t views_raw, chunks; /* views stored raw; chunks the view section went through */
  gx_ckpt_section sections[GX_CKPT_MAX_SECTIONS];
} gx_ckpt_info;

/* Writes the engine's checkpoint to `path` (created or replaced; removed again on failure). GX_EINVAL
 * inside a round or for a null argument, GX_EIO when the file cannot be written, GX_ENOMEM. */
int gx_ckpt_save(gx_engine *e, const char *path, gx_ckpt_info *info /* may be null */);
/* The header alone, no device: the saved params and round. GX_EIO for a file that cannot be read, is
 * short, is no checkpoint or whose header checksum fails; GX_EINVAL for another format version, ABI
 * version or sizeof(gx_params). */
int gx_ckpt_params(const char *path, gx_params *out, int64_t *round);
/* Creates an engine from the file (override = null: as saved, on the saved device). An override
 * starts from the copy gx_ckpt_params returns, with the fields of the FORK rule changed: the rest is
 * compared byte for byte with the saved struct, padding included. The header is
 * checked as by gx_ckpt_params, the override by the FORK rule, then each section's size against
 * what gx_create allocated for the params (GX_EINVAL for a file that does not fit) and each
 * section's checksum before its bytes are handed to a kernel (GX_EIO for a short or damaged file).
 * The view decoder checks on the device, bounded by the section's stored size whatever the records
 * say, that every record's shape holds (present bits below nblk, mask bits below R, popcount of the
 * masks = n_lit, the records fill the section exactly); a section that fails is GX_EIO. No engine
 * is left behind on failure (*out = null). info may be null. */
int gx_ckpt_load(const char *path, const gx_params *override, gx_engine **out, gx_ckpt_info *info);

#ifdef __cplusplus
}
#endif
#endif
