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
 *     u32 id (GX_CK_*)   u32 coding (GX_CKPT_RAW, _VIEWS, _FIFO)   u64 raw bytes   u64 stored bytes
 *     u64 checksum of the stored bytes
 *   the sections' stored bytes in table order, each zero-padded to 8 bytes (the padding is not
 *   counted in stored bytes and not checksummed)
 * Checksum of n bytes: the bytes as u64 words w[0..ceil(n / 8)) (the last zero-padded); with
 *   m(i) = w[i] ^ ((i + 1) * 0x9E3779B97F4A7C15),  m ^= m >> 32,  m *= 0xD6E8FEB86659FD93,  m ^= m >> 32
 * the checksum is (sum of m(i) mod 2^64) ^ n. Every single changed word changes it.
 * gx_ckpt_save stores every section raw (the buffer's bytes) except the views; gx_ckpt_save_coded
 * may also code the server times (GX_CKPT_CODE_SRVT) and the broadcast FIFOs (GX_CKPT_CODE_FIFO).
 * The table admits exactly these (id, coding) pairs: GX_CKPT_RAW with any id, GX_CKPT_VIEWS with
 * GX_CK_VIEW or GX_CK_SRVT, GX_CKPT_FIFO with GX_CK_FIFO.
 *
 * ROW CODING (coding GX_CKPT_VIEWS; raw bytes = 8 * rows * W): a table of `rows` rows of W u64 words,
 * nblk = ceil(W / 512) blocks of GX_DIGEST_SLOTS slots per row. Two sections instantiate it:
 *     GX_CK_VIEW  the VIEW SECTION: W = R = n_hosts * n_services slots, rows = Hl views (this engine's
 *                 hosts, departed ones included)
 *     GX_CK_SRVT  the SERVER TIMES, gx_server_times [Hl][n_hosts] read as u64 words: W = 2 * n_hosts
 *                 (always even), rows = Hl; the times as the engine keeps them, relative to gx_epoch
 *                 (0 stays 0), as in the raw section
 * First base[W] (u64): base[r] = the unsigned maximum of word r over the rows. Then one record per
 * row in ascending row order:
 *     u64 n_lit                      literals of this row; UINT64_MAX = stored raw: W words follow, nothing else
 *     u64 present[ceil(nblk / 64)]   bit b: block b has a slot that differs from base
 *     u64 mask[8] per present block  bit i: slot 512 b + i < W and word != base[slot]; bits past W are 0
 *     u64 literal per mask bit       the row's words, ascending slot order
 * A row is stored raw exactly when its coded record, 8 * (1 + ceil(nblk / 64) + 8 * present blocks
 * + n_lit) bytes, would not be smaller than 8 * W bytes. A warm cluster's rows all equal base: the
 * section is 8 W + rows * 8 * (1 + ceil(nblk / 64)) bytes (the server times: 16 n_hosts + Hl * 8 *
 * (1 + ceil(ceil(2 n_hosts / 512) / 64))).
 *
 * FIFO SECTION (coding GX_CKPT_FIFO; raw bytes = 16 * Hl * Q, Q = queue_cap): only each ring's stored
 * window, the jobs gx_read_queue returns. u32 n[Hl], zero-padded to 8 bytes, then for each host in
 * ascending order its n[v] jobs of 16 bytes in queue order: ring positions p % Q for p = fifo_head ..
 * fifo_stored - 1 of the host's gx_host_state. Stored bytes = pad8(4 Hl) + 16 * sum of n. The
 * positions [fifo_stored, fifo_tail) are counted, not stored, in the ring as in the file. A load
 * restores the ring slots outside the window as zero: nothing reads a slot outside [fifo_head,
 * fifo_stored) before a push has written it (the readers are listed in DESIGN.md "Checkpoints").
 * The file must hold the GX_CK_HS section (the lower id: it is restored first); every n[v] <= Q; n[v]
 * = fifo_stored - fifo_head (mod 2^32) of the restored hs[v]; table and jobs fill the section
 * exactly. Anything else is GX_EIO.
 *
 * MEMORY. Save and load stream through one staging area on the device (a chunk of records) and two
 * halves in pinned host memory (one is written to the file or read from it while the other is
 * copied), each the largest piece the engine has and GX_CKPT_STAGE_BYTES at most: 256 MiB on the
 * device and 512 MiB pinned at the most, under the 1 GiB this design was given. The three coders
 * share them, one section at a time:
 *     views         a chunk is as many views as fit the area at their worst case, 8 + 8 R bytes each
 *     server times  as many rows as fit at 8 + 8 W bytes each
 *     FIFOs         as many consecutive hosts as fit with the jobs their counts state; a host's
 *                   worst case is 16 Q bytes
 * An engine whose single worst-case record of a coded section exceeds the area (R > 2^25) is
 * GX_ENOMEM. Beyond that both directions allocate, per row-coded section, the base row (8 W bytes)
 * and 12 bytes per (row, block) of a chunk on the device; for the FIFOs 12 bytes per host on the
 * device and 4 per host on the host (the count table and its scan); and load the new engine. Nothing
 * proportional to the views, the server-time table or the rings is allocated on either side.
 * The environment variable GX_CKPT_STAGE_BYTES, read at each call, lowers the area and the halves
 * (it cannot raise them): a multiple of 8, else GX_EINVAL; GX_ENOMEM when it is smaller than one
 * worst-case record of a section this call codes or decodes. It exists so that tests reach the chunk
 * seams at small sizes; unset, nothing changes.
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
#define GX_CKPT_FIFO 2u
/* gx_ckpt_save_coded's mask: the sections coded beside the views */
#define GX_CKPT_CODE_SRVT 1u /* GX_CK_SRVT in the ROW CODING */
#define GX_CKPT_CODE_FIFO 2u /* GX_CK_FIFO as a FIFO SECTION */
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

/* The figures of gx_ckpt_save_coded's coders (gx_ckpt_info's times and counts stay the view
 * section's). Device times are HIP events around the kernels, summed over the chunks. */
typedef struct gx_ckpt_coded_info {
  float srvt_ms, srvt_base_ms, srvt_count_ms, srvt_emit_ms; /* server times: total; base, count + scans, emit */
  float fifo_ms;                                            /* FIFOs: counts, scan and pack */
  uint32_t srvt_rows_raw;                                   /* server-time rows stored raw */
  uint32_t srvt_chunks, fifo_chunks;                        /* chunks each coder went through */
  uint64_t fifo_jobs;                                     /* jobs written: the sum of the count table */
} gx_ckpt_coded_info;

/* Writes the engine's checkpoint to `path` (created or replaced; removed again on failure). GX_EINVAL
 * inside a round or for a null argument, GX_EIO when the file cannot be written, GX_ENOMEM. */
int gx_ckpt_save(gx_engine *e, const char *path, gx_ckpt_info *info /* may be null */);
/* gx_ckpt_save with the sections of `code` (a mask of GX_CKPT_CODE_*; any other bit is GX_EINVAL)
 * coded on the device. code = 0 is gx_ckpt_save: the same file, byte for byte. A bit whose buffer
 * the engine lacks is ignored. gx_ckpt_load reads either kind of file: the table says how each
 * section is coded. info and coded may be null. */
int gx_ckpt_save_coded(gx_engine *e, const char *path, uint32_t code, gx_ckpt_info *info, gx_ckpt_coded_info *coded);
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
 * The row decoder checks on the device, bounded by the section's stored size whatever the records
 * say, that every record's shape holds (present bits below nblk, mask bits below W, popcount of the
 * masks = n_lit, the records fill the section exactly), the FIFO decoder the rules of FIFO SECTION,
 * every read bounded by the section's end whatever the table says; a section that fails is GX_EIO. No engine
 * is left behind on failure (*out = null). info may be null. */
int gx_ckpt_load(const char *path, const gx_params *override, gx_engine **out, gx_ckpt_info *info);

#ifdef __cplusplus
}
#endif
#endif
