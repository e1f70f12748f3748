// gx_ckpt_file.hpp — the checkpoint file of include/gx_ckpt.h as the host sees it: checksum, header
// and section table (write, read, check), the fork rule, the walk over a row-coded section's records
// and the FIFO section's count table. Plain C++ with no device call, so it also builds into
// stand-alone host programs (tests/cpp/test_ckpt_file.cpp, tests/cpp/test_ckpt_coded_file.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/gx_ckpt.h"

// The checksum of gx_ckpt.h, fed piece by piece: every piece but the last a multiple of 8 bytes.
struct CkSum {
  uint64_t sum = 0, words = 0, bytes = 0;
  void add(const void *p, size_t n) {
    const uint8_t *b = (const uint8_t *)p;
    const size_t nw = n / 8;
    uint64_t s = sum, i = words;
    for (size_t k = 0; k < nw; k++) {
      uint64_t w;
      memcpy(&w, b + 8 * k, 8);
      s += mix(w, ++i);
    }
    if (n % 8) {
      uint64_t w = 0;
      memcpy(&w, b + 8 * nw, n % 8);
      s += mix(w, ++i);
    }
    sum = s;
    words = i;
    bytes += n;
  }
  uint64_t get() const { return sum ^ bytes; }
  static uint64_t mix(uint64_t w, uint64_t i1) {
    uint64_t m = w ^ (i1 * 0x9E3779B97F4A7C15ull);
    m ^= m >> 32;
    m *= 0xD6E8FEB86659FD93ull;
    return m ^ (m >> 32);
  }
};

struct CkSection {
  uint32_t id, coding;
  uint64_t raw, stored, sum;
  uint64_t at;  // file offset of the stored bytes (not in the file: from the order)
};
struct CkHeader {
  gx_params p;
  int64_t round;
  std::vector<CkSection> sec;
};

static inline uint64_t ck_pad8(uint64_t n) { return (n + 7) & ~7ull; }
static inline uint64_t ck_head_bytes(size_t nsec) {
  return GX_CKPT_HEADER_BYTES + ck_pad8(sizeof(gx_params)) + 32ull * nsec;
}

// header + table as the file holds them, the checksum field filled
static inline std::vector<uint8_t> ck_head_encode(const CkHeader &h) {
  std::vector<uint8_t> b(ck_head_bytes(h.sec.size()), 0);
  const uint64_t magic = GX_CKPT_MAGIC;
  const uint32_t w[4] = {GX_CKPT_FORMAT, (uint32_t)GX_ABI_VERSION, (uint32_t)sizeof(gx_params), (uint32_t)h.sec.size()};
  memcpy(&b[0], &magic, 8);
  memcpy(&b[8], w, 16);
  memcpy(&b[24], &h.round, 8);
  memcpy(&b[GX_CKPT_HEADER_BYTES], &h.p, sizeof(gx_params));
  size_t o = GX_CKPT_HEADER_BYTES + ck_pad8(sizeof(gx_params));
  for (const CkSection &s : h.sec) {
    memcpy(&b[o], &s.id, 4);
    memcpy(&b[o + 4], &s.coding, 4);
    memcpy(&b[o + 8], &s.raw, 8);
    memcpy(&b[o + 16], &s.stored, 8);
    memcpy(&b[o + 24], &s.sum, 8);
    o += 32;
  }
  CkSum c;
  c.add(b.data(), b.size());
  const uint64_t sum = c.get();
  memcpy(&b[32], &sum, 8);
  return b;
}

// The (id, coding) pairs the section table admits (gx_ckpt.h FILE).
static inline bool ck_coding_admitted(uint32_t id, uint32_t coding) {
  if (coding == GX_CKPT_RAW) return true;
  if (coding == GX_CKPT_VIEWS) return id == GX_CK_VIEW || id == GX_CK_SRVT;
  if (coding == GX_CKPT_FIFO) return id == GX_CK_FIFO;
  return false;
}

// Reads and checks header and table (gx_ckpt.h gx_ckpt_params); file_bytes = the file's length: the
// sections must fill it exactly.
static inline int ck_head_read(FILE *f, uint64_t file_bytes, CkHeader *h) {
  uint8_t fix[GX_CKPT_HEADER_BYTES];
  if (file_bytes < sizeof(fix) || fseek(f, 0, SEEK_SET) || fread(fix, 1, sizeof(fix), f) != sizeof(fix)) return GX_EIO;
  uint64_t magic, sum;
  uint32_t w[4];
  memcpy(&magic, &fix[0], 8);
  memcpy(w, &fix[8], 16);
  memcpy(&h->round, &fix[24], 8);
  memcpy(&sum, &fix[32], 8);
  if (magic != GX_CKPT_MAGIC) return GX_EIO;
  // the checksum covers the table, whose length the header states: bounded before it is believed
  const uint32_t psz = w[2], nsec = w[3];
  if (nsec > GX_CKPT_MAX_SECTIONS || psz > 4096) return GX_EIO;
  const uint64_t hb = GX_CKPT_HEADER_BYTES + ck_pad8(psz) + 32ull * nsec;
  if (file_bytes < hb) return GX_EIO;
  std::vector<uint8_t> b(hb);
  memcpy(b.data(), fix, sizeof(fix));
  if (fread(b.data() + sizeof(fix), 1, hb - sizeof(fix), f) != hb - sizeof(fix)) return GX_EIO;
  memset(&b[32], 0, 8);
  CkSum c;
  c.add(b.data(), b.size());
  if (c.get() != sum) return GX_EIO;
  if (w[0] != GX_CKPT_FORMAT || w[1] != (uint32_t)GX_ABI_VERSION || psz != sizeof(gx_params)) return GX_EINVAL;
  if (h->round < 0 || h->round >= GX_MAX_ROUND) return GX_EINVAL;
  memcpy(&h->p, &b[GX_CKPT_HEADER_BYTES], sizeof(gx_params));
  h->sec.resize(nsec);
  size_t o = GX_CKPT_HEADER_BYTES + ck_pad8(psz);
  uint64_t at = hb;
  for (uint32_t i = 0; i < nsec; i++, o += 32) {
    CkSection &s = h->sec[i];
    memcpy(&s.id, &b[o], 4);
    memcpy(&s.coding, &b[o + 4], 4);
    memcpy(&s.raw, &b[o + 8], 8);
    memcpy(&s.stored, &b[o + 16], 8);
    memcpy(&s.sum, &b[o + 24], 8);
    if (!s.id || s.id >= GX_CK_ID_END || (i && s.id <= h->sec[i - 1].id)) return GX_EINVAL;
    if (!ck_coding_admitted(s.id, s.coding)) return GX_EINVAL;
    if (s.coding == GX_CKPT_RAW && s.stored != s.raw) return GX_EINVAL;
    // gx_ckpt.h FIFO SECTION: the counts are checked against the host states of the same file
    // (ascending ids: GX_CK_HS, if there, is the entry before)
    if (s.coding == GX_CKPT_FIFO && !(i && h->sec[i - 1].id == GX_CK_HS)) return GX_EIO;
    if (s.stored > file_bytes - at) return GX_EIO;  // a short file (at <= file_bytes throughout)
    s.at = at;
    at += ck_pad8(s.stored);
    if (at > file_bytes) at = file_bytes;  // only the last section's padding can be cut: told apart below
  }
  uint64_t want = hb;
  for (const CkSection &s : h->sec) want += ck_pad8(s.stored);
  if (want != file_bytes) return GX_EIO;
  return GX_OK;
}

// gx_ckpt.h FORK: what `o` may change against the saved params at the saved round.
static inline int ck_fork_check(const gx_params &saved, const gx_params &o, int64_t round) {
  gx_params a = saved, b = o;
  a.device = b.device = 0;
  a.partition_start = b.partition_start = a.partition_end = b.partition_end = 0;
  a.storm_round = b.storm_round = 0;
  a.depart_round = b.depart_round = 0;
  a.depart_ppm = b.depart_ppm = 0;
  if (memcmp(&a, &b, sizeof(gx_params))) return GX_EINVAL;
  auto begun = [&](int64_t start) { return start >= 0 && start <= round; };
  // the partition begins at partition_start (an empty window [s, e), e <= s, never holds a round)
  auto part_begun = [&](const gx_params &p) { return p.partition_end > p.partition_start && begun(p.partition_start); };
  if ((saved.partition_start != o.partition_start || saved.partition_end != o.partition_end) &&
      (part_begun(saved) || part_begun(o)))
    return GX_EINVAL;
  if (saved.storm_round != o.storm_round && (begun(saved.storm_round) || begun(o.storm_round))) return GX_EINVAL;
  auto dep_begun = [&](const gx_params &p) { return p.depart_ppm && begun(p.depart_round); };
  if ((saved.depart_round != o.depart_round || saved.depart_ppm != o.depart_ppm) && (dep_begun(saved) || dep_begun(o)))
    return GX_EINVAL;
  return GX_OK;
}

// gx_ckpt.h FIFO SECTION: the count table at `table` (table_bytes of it are there) of a section of
// `stored` bytes for Hl hosts with rings of Q jobs. The jobs the section holds, or -1 if it can be
// none: a short table, a count above Q, padding that is not zero, table and jobs that do not fill
// the section exactly. (That a count equals the host's window is the device's to check.)
static inline int64_t ck_fifo_table_jobs(const void *table, uint64_t table_bytes, uint64_t Hl, uint64_t Q, uint64_t stored) {
  const uint64_t tb = ck_pad8(4 * Hl);
  if (stored < tb || table_bytes < tb || (stored - tb) % 16) return -1;
  uint64_t jobs = 0;
  for (uint64_t v = 0; v < tb / 4; v++) {
    uint32_t n;
    memcpy(&n, (const uint8_t *)table + 4 * v, 4);
    if (v >= Hl ? n != 0 : n > Q) return -1;
    jobs += n;
  }
  return jobs == (stored - tb) / 16 ? (int64_t)jobs : -1;
}
// The hosts from v0 on whose jobs fit `bytes` of staging together (16 bytes a job); 0 when the
// first one's alone do not. *jobs = what they hold.
static inline uint32_t ck_fifo_chunk_hosts(const uint32_t *n, uint32_t v0, uint32_t Hl, uint64_t bytes, uint64_t *jobs) {
  uint64_t sum = 0;
  uint32_t v = v0;
  for (; v < Hl && 16 * (sum + n[v]) <= bytes; v++) sum += n[v];
  *jobs = sum;
  return v - v0;
}

// A row record (gx_ckpt.h ROW CODING; a view's, or a server-time row's with R = W) at
// words[0 .. have): its length in words if it is complete and well-formed so far as
// the host can tell (n_lit and the present words; the masks are the device's to check), 0 if more
// words are needed, -1 if it can never be one. R slots, nblk blocks, PW present words.
static inline int64_t ck_view_record_words(const uint64_t *words, uint64_t have, uint64_t R, uint64_t nblk, uint64_t PW) {
  if (have < 1) return 0;
  const uint64_t nl = words[0];
  if (nl == ~0ull) return have >= 1 + R ? (int64_t)(1 + R) : 0;
  if (nl > R) return -1;
  if (have < 1 + PW) return 0;
  uint64_t np = 0;
  for (uint64_t j = 0; j < PW; j++) np += (uint64_t)__builtin_popcountll(words[1 + j]);
  if (np > nblk || (np == 0) != (nl == 0) || nl < np) return -1;
  const uint64_t len = 1 + PW + 8 * np + nl;
  if (len >= R) return -1;  // such a view is stored raw
  return have >= len ? (int64_t)len : 0;
}
