// gx_ckpt_host.hpp — engine checkpoints (include/gx_ckpt.h): gx_ckpt_save, gx_ckpt_save_coded,
// gx_ckpt_params, gx_ckpt_load and the coders' kernels. Included by gx_engine.hip after the ABI.
//
// The row coder (gx_ckpt.h ROW CODING) serves the views (rows of R words) and the server times (rows
// of W = 2 H words) through the same kernels: CkRows names the table, and in the kernels "view" and
// "R" stand for a row and its length. It works a chunk of rows at a time: as many as fit the device
// staging area at their worst case (8 + 8 R bytes each). One wave owns one (view, block) unit, a
// block being the 512 slots of GX_DIGEST_SLOTS: lane i of the wave reads slot 64 q + i of the block
// for q = 0..7, so the ballot of "differs from base" is mask word q as the file holds it, with no
// LDS and no atomics.
//   save   k_ck_base     base[r] = max over the views (one stream over the views)
//          k_ck_count    literals per unit (second stream)
//          k_ck_vscan    per view, an ordered scan over its blocks: each block's literal offset and
//                        rank among the present blocks; the record's length, or raw
//          k_ck_offsets  ordered scan over the chunk's record lengths
//          k_ck_emit     n_lit, present words, masks, literals (ballot + popcount rank); a raw view's
//                        row. Third stream, of the present blocks only.
//   load   k_ck_dcount   per unit: the block's rank among the present ones, its masks' popcount; checks
//                        the record's shape, every read bounded by the record's end
//          k_ck_vscan    literal offsets; sum of the popcounts = n_lit, length = what the host walked
//          k_ck_expand   rows from base and literals, 16-B loads and stores on even R
//
// The FIFO coder (gx_ckpt.h FIFO SECTION) keeps each ring's stored window [fifo_head, fifo_stored):
//   save   k_ck_fcount   n[v] from hs
//          k_ck_foffsets ordered exclusive scan of n (one block)
//          k_ck_fpack    a chunk of consecutive hosts, a team per host (a wave; a block when Q >
//                        CK_FIFO_WAVE_Q): lane i copies job i, i + T, ... of the window with one 16-B
//                        load and one 16-B store. The window wraps at most once, so a host reads two
//                        contiguous runs of its ring and writes one run of the staging area.
//   load   k_ck_foffsets the same scan, of the file's table
//          k_ck_funpack  every ring slot written once: its job of the window, or zero outside it;
//                        checks n[v] <= Q, n[v] = the restored window's length and that the jobs lie
//                        inside the chunk, else the error word (no read past the chunk's jobs
//                        whatever the table says)
#include <stdlib.h>
#include <sys/stat.h>

#include "gx_ckpt_file.hpp"

#define CK_BS GX_DIGEST_SLOTS
#define CK_MAX_CHUNK_VIEWS 65536u  // rows of a chunk at the most, of either row-coded table
#define CK_ERR_SHAPE 1u
#define CK_FIFO_WAVE_Q 1024u  // rings up to this size take a wave per host, larger ones a block

// A table the row coder codes: `rows` rows of W words; t0: the first of its three timing classes
// (CkStage::time_begin); vec: k_ck_expand's 16-B variant (W even, so every row is 16-B aligned).
struct CkRows {
  uint64_t *p;
  uint32_t W, rows;
  int t0;
  bool vec;
};
struct CkRowStats {
  uint32_t chunks = 0, raw = 0;
};
static uint32_t ck_nblk(uint32_t W) { return (W + CK_BS - 1) / CK_BS; }
#define CK_T_VIEW 0
#define CK_T_SRVT 3
#define CK_T_FIFO 6
#define CK_T_N 7

struct CkChunk {
  uint64_t *view;        // the chunk's first row
  const uint64_t *base;  // [R]
  uint32_t R, nblk, PW, nv;  // R: the row's length (the views' R, the server times' W)
  uint32_t *cnt, *loff, *prank;  // [nv][nblk] literals of the unit, literals / present blocks before it in the view
  uint64_t *vnl;                 // [nv] n_lit as the record states it
  uint32_t *vnp;                 // [nv] present blocks
  uint64_t *vwords;              // [nv] record length in words
  uint64_t *voff;                // [nv + 1] record offsets in the staging area, in words
  uint64_t *buf;                 // the staging area
};

// grid (ceil(R / 256), VG): slice y takes the views y, y + VG, ...; base is zeroed before
__global__ __launch_bounds__(256) void k_ck_base(const uint64_t *view, uint32_t R, uint32_t Hl, unsigned long long *base) {
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  uint64_t m = 0;
  uint32_t v = blockIdx.y;
  for (; v + 3 * gridDim.y < Hl; v += 4 * gridDim.y) {  // four rows in flight
    const uint64_t a = gld(&view[(size_t)v * R + r]), b = gld(&view[(size_t)(v + gridDim.y) * R + r]);
    const uint64_t c = gld(&view[(size_t)(v + 2 * gridDim.y) * R + r]), d = gld(&view[(size_t)(v + 3 * gridDim.y) * R + r]);
    const uint64_t ab = a > b ? a : b, cd = c > d ? c : d;
    m = m > ab ? m : ab;
    m = m > cd ? m : cd;
  }
  for (; v < Hl; v += gridDim.y) {
    const uint64_t a = gld(&view[(size_t)v * R + r]);
    m = m > a ? m : a;
  }
  if (gridDim.y == 1) base[r] = m;
  else if (m) atomicMax(&base[r], (unsigned long long)m);
}

// the unit of this wave, or false past the last one (wave-uniform)
GXD bool ck_unit(const CkChunk &c, uint32_t *u, uint32_t *v, uint32_t *b) {
  *u = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (*u >= c.nv * c.nblk) return false;
  *v = *u / c.nblk;
  *b = *u % c.nblk;
  return true;
}

__global__ __launch_bounds__(256) void k_ck_count(CkChunk c) {
  uint32_t u, v, b;
  if (!ck_unit(c, &u, &v, &b)) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *row = c.view + (size_t)v * c.R;
  const uint64_t r0 = (uint64_t)b * CK_BS + lane;
  uint32_t n = 0;
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) {
    const uint64_t r = r0 + 64 * q;
    const bool ne = r < c.R && gld(&row[r]) != gld(&c.base[r]);
    n += (uint32_t)__popcll(__ballot(ne));
  }
  if (lane == 0) c.cnt[u] = n;
}

// Exclusive scan of x over the block's 256 threads (s_w: 4 words of LDS); *total = the block's sum.
GXD uint64_t ck_block_scan(uint64_t x, uint64_t *s_w, uint64_t *total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t inc = x;
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t y = __shfl_up((unsigned long long)inc, o, 64);
    if (lane >= (uint32_t)o) inc += y;
  }
  __syncthreads();  // the last call's reads of s_w
  if (lane == 63) s_w[w] = inc;
  __syncthreads();
  uint64_t pre = 0, tot = 0;
  for (uint32_t q = 0; q < 4; q++) {
    if (q < w) pre += s_w[q];
    tot += s_w[q];
  }
  *total = tot;
  return pre + inc - x;
}

// One block per view: loff (and, encoding, prank) from cnt, in block order. Encoding: the record's
// n_lit, present blocks and length, raw when the coded record would reach 8 R bytes. Decoding:
// checks the record against its masks and against the length the host walked.
template <bool ENC>
__global__ __launch_bounds__(256) void k_ck_vscan(CkChunk c, uint32_t *err) {
  __shared__ uint64_t s_w[4];
  const uint32_t v = blockIdx.x, t = threadIdx.x;
  if (!ENC && c.buf[c.voff[v]] == ~0ull) return;  // a raw view (block-uniform); its length was the host's to check
  uint64_t carry = 0;  // present blocks << 32 | literals (at most R < 2^32)
  for (uint32_t b0 = 0; b0 < c.nblk; b0 += 256) {
    const uint32_t b = b0 + t;  // (nblk < 2^23)
    const uint32_t n = b < c.nblk ? c.cnt[(size_t)v * c.nblk + b] : 0u;
    uint64_t tot;
    const uint64_t pre = carry + ck_block_scan((uint64_t)n | ((uint64_t)(n != 0) << 32), s_w, &tot);
    if (b < c.nblk) {
      c.loff[(size_t)v * c.nblk + b] = (uint32_t)pre;
      if (ENC) c.prank[(size_t)v * c.nblk + b] = (uint32_t)(pre >> 32);
    }
    carry += tot;
  }
  if (t) return;
  const uint64_t nl = (uint32_t)carry, np = carry >> 32, words = 1 + c.PW + 8 * np + nl;
  c.vnp[v] = (uint32_t)np;
  if (ENC) {
    const bool raw = words >= c.R;
    c.vnl[v] = raw ? ~0ull : nl;
    c.vwords[v] = raw ? 1 + (uint64_t)c.R : words;
  } else if (c.buf[c.voff[v]] != nl || words != c.voff[v + 1] - c.voff[v]) {
    atomicOr(err, CK_ERR_SHAPE);
  }
}

// voff = exclusive scan of vwords, voff[nv] = the chunk's length (one block)
__global__ __launch_bounds__(256) void k_ck_offsets(CkChunk c) {
  __shared__ uint64_t s_w[4];
  uint64_t carry = 0;
  for (uint32_t v0 = 0; v0 < c.nv; v0 += 256) {
    const uint32_t v = v0 + threadIdx.x;
    uint64_t tot;
    const uint64_t pre = carry + ck_block_scan(v < c.nv ? c.vwords[v] : 0ull, s_w, &tot);
    if (v < c.nv) c.voff[v] = pre;
    carry += tot;
  }
  if (threadIdx.x == 0) c.voff[c.nv] = carry;
}

// Every offset comes from counts of the same words (the engine is idle between the passes), and a
// record is never longer than 1 + R words: the chunk stays inside nv * (1 + R) words of buf.
__global__ __launch_bounds__(256) void k_ck_emit(CkChunk c) {
  uint32_t u, v, b;
  if (!ck_unit(c, &u, &v, &b)) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *row = c.view + (size_t)v * c.R;
  uint64_t *o = c.buf + c.voff[v];
  const uint64_t nl = c.vnl[v], r0 = (uint64_t)b * CK_BS + lane;
  if (b == 0 && lane == 0) o[0] = nl;
  if (nl == ~0ull) {  // raw: the row
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
      const uint64_t r = r0 + 64 * q;
      if (r < c.R) o[1 + r] = gld(&row[r]);
    }
    return;
  }
  if (b % 64 == 0) {  // this unit also writes the present word of blocks [b, b + 64)
    const bool p = b + lane < c.nblk && c.cnt[u + lane] != 0;
    const uint64_t m = __ballot(p);
    if (lane == 0) o[1 + b / 64] = m;
  }
  if (!c.cnt[u]) return;
  uint64_t *mo = o + 1 + c.PW + 8ull * c.prank[u];
  uint64_t *lo = o + 1 + c.PW + 8ull * c.vnp[v] + c.loff[u];
  uint32_t run = 0;
#pragma unroll
  for (uint32_t q = 0; q < 8; q++) {
    const uint64_t r = r0 + 64 * q;
    const uint64_t w = r < c.R ? gld(&row[r]) : 0ull;
    const bool ne = r < c.R && w != gld(&c.base[r]);
    const uint64_t m = __ballot(ne);
    if (lane == 0) mo[q] = m;
    if (ne) lo[run + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = w;
    run += (uint32_t)__popcll(m);
  }
}

// Decoding. voff comes from the host's walk over the records (ck_view_record_words): a coded record
// holds at least 1 + PW words and ends inside the bytes copied in.
__global__ __launch_bounds__(256) void k_ck_dcount(CkChunk c, uint32_t *err) {
  uint32_t u, v, b;
  if (!ck_unit(c, &u, &v, &b)) return;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t *rec = c.buf + c.voff[v];
  const uint64_t len = c.voff[v + 1] - c.voff[v];
  uint32_t n = 0, pr = 0;
  bool bad = false;
  if (rec[0] != ~0ull) {
    const uint32_t wi = b >> 6;
    for (uint32_t j = lane; j <= wi; j += 64) {  // present blocks before b
      uint64_t pw = rec[1 + j];
      if (j == wi) pw &= (1ull << (b & 63u)) - 1ull;
      pr += (uint32_t)__popcll(pw);
    }
    pr = (uint32_t)wave_sum(pr);
    // present bits past the last block
    if (b == c.nblk - 1 && (b & 63u) != 63u && (rec[1 + wi] >> ((b & 63u) + 1))) bad = true;
    if ((rec[1 + wi] >> (b & 63u)) & 1ull) {
      const uint64_t moff = 1 + c.PW + 8ull * pr;
      if (moff + 8 > len) {
        bad = true;
      } else {
        const uint64_t mw = lane < 8 ? rec[moff + lane] : 0ull;
        n = (uint32_t)wave_sum((unsigned long long)__popcll(mw));
        const uint64_t s0 = (uint64_t)b * CK_BS + 64ull * lane;  // mask bits at or past R
        const uint64_t past = s0 >= c.R ? ~0ull : c.R - s0 >= 64 ? 0ull : ~0ull << (c.R - s0);
        if (__ballot(lane < 8 && (mw & past)) || !n) bad = true;
      }
    }
  }
  if (lane == 0) {
    c.cnt[u] = bad ? 0u : n;
    c.prank[u] = pr;
    if (bad) atomicOr(err, CK_ERR_SHAPE);
  }
}

// Rows from base and literals. A literal's index is bounded by the record's length whatever the
// masks say (k_ck_vscan has checked them; this holds regardless). VEC (even R): a lane takes the slot
// pair 128 q + 2 lane of its block with 16-B loads of base and 16-B nontemporal stores of the row.
template <bool VEC>
__global__ __launch_bounds__(256) void k_ck_expand(CkChunk c) {
  uint32_t u, v, b;
  if (!ck_unit(c, &u, &v, &b)) return;
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t *row = c.view + (size_t)v * c.R;
  const uint64_t *rec = c.buf + c.voff[v];
  const uint64_t len = c.voff[v + 1] - c.voff[v];
  const uint64_t rb = (uint64_t)b * CK_BS;
  if (rec[0] == ~0ull) {  // raw (len = 1 + R: the host's walk)
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
      const uint64_t r = rb + 64 * q + lane;
      if (r < c.R) row[r] = rec[1 + r];
    }
    return;
  }
  const uint32_t n = c.cnt[u];
  uint64_t mw = 0;
  if (n && lane < 8) mw = rec[1 + c.PW + 8ull * c.prank[u] + lane];  // (inside the record: k_ck_dcount)
  const uint64_t lit0 = 1 + c.PW + 8ull * c.vnp[v] + c.loff[u];
  uint32_t run = 0;
  if (VEC) {
    typedef unsigned long long v2u64s __attribute__((ext_vector_type(2)));
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) {
      const uint64_t ma = __shfl((unsigned long long)mw, 2 * q, 64), mb = __shfl((unsigned long long)mw, 2 * q + 1, 64);
      const uint32_t ca = (uint32_t)__popcll(ma);
      const bool hi = lane >= 32;
      const uint64_t m = hi ? mb : ma;
      const uint32_t bit = (2 * lane) & 63u;
      const uint32_t rank = run + (hi ? ca : 0u) + (uint32_t)__popcll(m & ((1ull << bit) - 1ull));
      const bool l0 = (m >> bit) & 1ull, l1 = (m >> (bit + 1)) & 1ull;
      const uint64_t r = rb + 128 * q + 2 * lane;
      if (r < c.R) {  // R even: the pair is inside the row, 16-B aligned
        const gx_u32x4 bw = gld4(&c.base[r]);
        uint64_t w0 = (uint64_t)bw.x | ((uint64_t)bw.y << 32), w1 = (uint64_t)bw.z | ((uint64_t)bw.w << 32);
        const uint64_t i0 = lit0 + rank, i1 = lit0 + rank + (l0 ? 1u : 0u);
        if (l0 && i0 < len) w0 = rec[i0];
        if (l1 && i1 < len) w1 = rec[i1];
        __builtin_nontemporal_store((v2u64s){w0, w1}, reinterpret_cast<v2u64s *>(&row[r]));
      }
      run += ca + (uint32_t)__popcll(mb);
    }
  } else {
#pragma unroll
    for (uint32_t q = 0; q < 8; q++) {
      const uint64_t m = __shfl((unsigned long long)mw, q, 64);
      const uint64_t r = rb + 64 * q + lane;
      if (r < c.R) {
        uint64_t w = gld(&c.base[r]);
        const uint64_t i = lit0 + run + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (((m >> lane) & 1ull) && i < len) w = rec[i];
        row[r] = w;
      }
      run += (uint32_t)__popcll(m);
    }
  }
}

// ------------------------------------------------------------------------------- FIFO coder --
struct CkFifo {
  const gx_host_state *hs;  // the chunk's first host
  gx_job *ring;             // and its ring
  const uint32_t *n;        // [nv] the chunk's entries of the count table
  const uint64_t *off;      // [nv + 1] the table's exclusive scan, from the chunk's first host on
  uint32_t Q, nv;
  uint64_t jobs;            // the chunk's jobs as the host summed them: what buf holds
  gx_job *buf;              // the staging area
};

__global__ __launch_bounds__(256) void k_ck_fcount(const gx_host_state *hs, uint32_t Hl, uint32_t *n) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v < Hl) n[v] = gld(&hs[v].fifo_stored) - gld(&hs[v].fifo_head);
}

// off = exclusive scan of n, off[Hl] = the jobs of all hosts (one block)
__global__ __launch_bounds__(256) void k_ck_foffsets(const uint32_t *n, uint32_t Hl, uint64_t *off) {
  __shared__ uint64_t s_w[4];
  uint64_t carry = 0;
  for (uint32_t v0 = 0; v0 < Hl; v0 += 256) {
    const uint32_t v = v0 + threadIdx.x;
    uint64_t tot;
    const uint64_t pre = carry + ck_block_scan(v < Hl ? (uint64_t)n[v] : 0ull, s_w, &tot);
    if (v < Hl) off[v] = pre;
    carry += tot;
  }
  if (threadIdx.x == 0) off[Hl] = carry;
}

// Teams of T lanes, one per host. Job i of the window is ring position (head + i) % Q: no read
// leaves the ring (the count is clamped to Q) and no store leaves the chunk's c.jobs jobs of buf.
template <int T>
__global__ __launch_bounds__(256) void k_ck_fpack(CkFifo c) {
  const uint32_t v = blockIdx.x * (256 / T) + threadIdx.x / T, t = threadIdx.x % T;
  if (v >= c.nv) return;
  const uint32_t n = min(c.n[v], c.Q), h0 = gld(&c.hs[v].fifo_head) % c.Q;
  const uint64_t o = c.off[v] - c.off[0];
  const gx_job *ring = c.ring + (size_t)v * c.Q;
  for (uint32_t i = t; i < n && o + i < c.jobs; i += T) {
    uint32_t p = h0 + i;  // (h0 < Q, i < Q)
    if (p >= c.Q) p -= c.Q;
    gst4(&c.buf[o + i], gld4(&ring[p]));
  }
}

// The reverse, over every slot of the ring: slot p holds job (p - head) mod Q of the window, or zero.
// A host whose count fails a check of gx_ckpt.h FIFO SECTION gets an empty ring and sets *err.
template <int T>
__global__ __launch_bounds__(256) void k_ck_funpack(CkFifo c, uint32_t *err) {
  const uint32_t v = blockIdx.x * (256 / T) + threadIdx.x / T, t = threadIdx.x % T;
  if (v >= c.nv) return;
  const uint32_t n = c.n[v], head = gld(&c.hs[v].fifo_head), stored = gld(&c.hs[v].fifo_stored);
  const uint64_t o = c.off[v] - c.off[0];
  const bool ok = n <= c.Q && n == stored - head && o <= c.jobs && n <= c.jobs - o;
  if (!ok && t == 0) atomicOr(err, CK_ERR_SHAPE);
  const uint32_t h0 = head % c.Q, nn = ok ? n : 0u;
  gx_job *ring = c.ring + (size_t)v * c.Q;
  for (uint32_t p = t; p < c.Q; p += T) {
    const uint32_t i = p >= h0 ? p - h0 : p + c.Q - h0;
    gx_u32x4 j = {0u, 0u, 0u, 0u};
    if (i < nn) j = gld4(&c.buf[o + i]);  // o + i < o + n <= c.jobs
    gst4(&ring[p], j);
  }
}

// ------------------------------------------------------------------------------------ host --
// The staging both directions stream through: one area on the device (the coder's chunk) and two
// pinned halves the file is written from and read into, `half` bytes each (<= GX_CKPT_STAGE_BYTES).
struct CkStage {
  uint8_t *dev = nullptr, *pin[2] = {nullptr, nullptr};
  uint64_t *voff_pin = nullptr;  // load: [CK_MAX_CHUNK_VIEWS + 1] record offsets of a chunk
  hipEvent_t ev[2] = {nullptr, nullptr};
  size_t half = 0, n[2] = {0, 0};
  bool busy[2] = {false, false};
  int k = 0;
  hipStream_t s = nullptr;
  FILE *f = nullptr;
  CkSum sum;
  std::vector<hipEvent_t> timed;  // (a, b, class) triples flattened: a, b per launch group
  std::vector<int> timed_cls;
  ~CkStage() {
    if (s) (void)hipStreamSynchronize(s);
    (void)hipFree(dev);
    for (int i = 0; i < 2; i++) {
      if (pin[i]) (void)hipHostFree(pin[i]);
      if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
    if (voff_pin) (void)hipHostFree(voff_pin);
    for (hipEvent_t x : timed) (void)hipEventDestroy(x);
    if (f) fclose(f);
  }
  int init(hipStream_t s_, size_t half_, bool with_dev, bool with_voff) {
    s = s_;
    half = half_ < 4096 ? 4096 : (half_ + 7) & ~(size_t)7;
    for (int i = 0; i < 2; i++) {
      if (hipHostMalloc((void **)&pin[i], half) != hipSuccess || hipEventCreateWithFlags(&ev[i], hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        return GX_ENOMEM;
      }
    }
    if (with_dev && hipMalloc((void **)&dev, half) != hipSuccess) {
      (void)hipGetLastError();
      return GX_ENOMEM;
    }
    if (with_voff && hipHostMalloc((void **)&voff_pin, sizeof(uint64_t) * (CK_MAX_CHUNK_VIEWS + 1)) != hipSuccess) {
      (void)hipGetLastError();
      return GX_ENOMEM;
    }
    return GX_OK;
  }
  // save: the half's bytes have arrived; checksum them and append them to the file
  int flush(int i) {
    if (!busy[i]) return GX_OK;
    HIPCHK(hipEventSynchronize(ev[i]));
    busy[i] = false;
    sum.add(pin[i], n[i]);
    return fwrite(pin[i], 1, n[i], f) == n[i] ? GX_OK : GX_EIO;
  }
  // save: `bytes` (<= half) of device memory go to the file next; the piece before it is written
  // while this one is copied
  int push(const void *src, size_t bytes) {
    GXTRY(flush(k));
    HIPCHK(hipMemcpyAsync(pin[k], src, bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(ev[k], s));
    n[k] = bytes;
    busy[k] = true;
    k ^= 1;
    return flush(k);
  }
  int drain() {
    GXTRY(flush(k));
    return flush(k ^ 1);
  }
  void time_begin(int cls) {
    hipEvent_t a = nullptr, b = nullptr;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    timed.push_back(a);
    timed.push_back(b);
    timed_cls.push_back(cls);
    (void)hipEventRecord(a, s);
  }
  void time_end() { (void)hipEventRecord(timed.back(), s); }
  // after the stream is idle
  void time_collect(float *ms /* [CK_T_N] */) {
    for (size_t i = 0; i < timed_cls.size(); i++) {
      float x = 0;
      if (hipEventElapsedTime(&x, timed[2 * i], timed[2 * i + 1]) == hipSuccess) ms[timed_cls[i]] += x;
    }
    (void)hipGetLastError();
  }
};

// rows of table t per chunk: what fits the staging half at 8 + 8 W bytes each
static uint32_t ck_chunk_rows(const CkRows &t, size_t half) {
  const uint64_t rec = 8ull * (1 + (uint64_t)t.W);
  uint64_t n = half / rec;
  if (n > t.rows) n = t.rows;
  if (n > CK_MAX_CHUNK_VIEWS) n = CK_MAX_CHUNK_VIEWS;
  // the units of a chunk are counted in 32 bits
  while (n > 1 && n * (uint64_t)ck_nblk(t.W) > 0x7fffffffull) n /= 2;
  return (uint32_t)n;
}
// the per-chunk arrays of CkChunk for chunks of cv rows of table t
static int ck_chunk_alloc(DevMem &tmp, const CkRows &t, uint32_t cv, CkChunk *c, uint32_t **err, hipStream_t s) {
  const size_t nu = (size_t)cv * ck_nblk(t.W);
  c->R = t.W;
  c->nblk = ck_nblk(t.W);
  c->PW = (c->nblk + 63) / 64;
  GXTRY(tmp.take(c->cnt, sizeof(uint32_t) * nu));
  GXTRY(tmp.take(c->loff, sizeof(uint32_t) * nu));
  GXTRY(tmp.take(c->prank, sizeof(uint32_t) * nu));
  GXTRY(tmp.take(c->vnl, sizeof(uint64_t) * cv));
  GXTRY(tmp.take(c->vnp, sizeof(uint32_t) * cv));
  GXTRY(tmp.take(c->vwords, sizeof(uint64_t) * cv));
  GXTRY(tmp.take(c->voff, sizeof(uint64_t) * ((size_t)cv + 1)));
  return tmp.take(*err, sizeof(uint32_t), 0, s);
}

// The tables of an engine the row coder may code.
static CkRows ck_rows_views(const gx_engine *e) { return {e->d.view, e->d.R, e->d.Hl, CK_T_VIEW, vec_of(e)}; }
// gx_server_times [Hl][H] as words: W = 2 H is even whatever R is
static CkRows ck_rows_srvt(const gx_engine *e) { return {(uint64_t *)e->d.srvt, 2 * e->d.H, e->d.Hl, CK_T_SRVT, true}; }

// gx_ckpt.h MEMORY: GX_CKPT_STAGE_BYTES, or the smaller value the environment gives at this call.
static int ck_stage_cap(uint64_t *cap) {
  *cap = GX_CKPT_STAGE_BYTES;
  const char *s = getenv("GX_CKPT_STAGE_BYTES");
  if (!s || !*s) return GX_OK;
  char *end = nullptr;
  const unsigned long long v = strtoull(s, &end, 10);
  if (*end || !v || v % 8) return GX_EINVAL;
  if (v < *cap) *cap = v;
  return GX_OK;
}

// The staging half an engine's checkpoint streams through: the largest piece, the cap at most. srvt,
// fifo: this call codes or decodes that section.
static int ck_half_bytes(const gx_engine *e, bool srvt, bool fifo, size_t *half) {
  const Dev &d = e->d;
  uint64_t cap;
  GXTRY(ck_stage_cap(&cap));
  const uint64_t rows = std::min<uint64_t>(d.Hl ? d.Hl : 1, CK_MAX_CHUNK_VIEWS);
  const uint64_t rec = 8ull * (1 + (uint64_t)d.R), rec_t = 8ull * (1 + 2ull * d.H), rec_f = sizeof(gx_job) * (uint64_t)d.Q;
  // gx_ckpt.h MEMORY: one worst-case record of every coded section fits
  if (rec > cap || (srvt && rec_t > cap) || (fifo && rec_f > cap)) return GX_ENOMEM;
  uint64_t want = rec * rows;
  if (srvt) want = std::max(want, rec_t * rows);
  for (const DevMem::Buf &b : e->mem.bufs)
    if (b.id && b.id != GX_CK_VIEW) want = std::max<uint64_t>(want, b.bytes);
  *half = (size_t)std::min<uint64_t>(want, cap);
  return GX_OK;
}

// One row-coded section of table t, to the file.
static int ck_save_rows(gx_engine *e, CkStage &st, const CkRows &t, CkRowStats *stats) {
  hipStream_t s = e->stream;
  DevMem tmp;  // freed on return; the hipStreamSynchronize below runs first, so no kernel still reads it
  const uint32_t cv = ck_chunk_rows(t, st.half);
  if (!cv) return t.rows ? GX_ENOMEM : GX_OK;
  CkChunk c{};
  uint32_t *err;
  unsigned long long *base;
  GXTRY(tmp.take(base, sizeof(uint64_t) * t.W, 0, s));
  GXTRY(ck_chunk_alloc(tmp, t, cv, &c, &err, s));
  c.base = (const uint64_t *)base;
  c.buf = (uint64_t *)st.dev;
  int rc = GX_OK;
  auto body = [&]() -> int {
    st.time_begin(t.t0);
    const unsigned gx = nblk(t.W, 256);
    const unsigned vg = std::max(1u, std::min(t.rows, 4096u / std::min(gx, 4096u)));
    k_ck_base<<<dim3(gx, vg), 256, 0, s>>>(t.p, t.W, t.rows, base);
    st.time_end();
    HIPCHK(hipGetLastError());
    for (uint64_t o = 0; o < 8ull * t.W; o += st.half)
      GXTRY(st.push((const uint8_t *)base + o, (size_t)std::min<uint64_t>(st.half, 8ull * t.W - o)));
    std::vector<uint64_t> vnl(cv);
    for (uint32_t v0 = 0; v0 < t.rows; v0 += cv) {
      c.nv = std::min(cv, t.rows - v0);
      c.view = t.p + (size_t)v0 * t.W;
      const unsigned gu = nblk((size_t)c.nv * c.nblk, 4);
      st.time_begin(t.t0 + 1);
      k_ck_count<<<gu, 256, 0, s>>>(c);
      k_ck_vscan<true><<<c.nv, 256, 0, s>>>(c, err);
      k_ck_offsets<<<1, 256, 0, s>>>(c);
      st.time_end();
      HIPCHK(hipGetLastError());
      uint64_t words = 0;
      HIPCHK(hipMemcpyAsync(&words, &c.voff[c.nv], sizeof(words), hipMemcpyDeviceToHost, s));
      HIPCHK(hipMemcpyAsync(vnl.data(), c.vnl, sizeof(uint64_t) * c.nv, hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (8 * words > st.half) return GX_EIO;  // (cannot happen: a record is at most 8 + 8 R bytes)
      st.time_begin(t.t0 + 2);
      k_ck_emit<<<gu, 256, 0, s>>>(c);
      st.time_end();
      HIPCHK(hipGetLastError());
      GXTRY(st.push(st.dev, (size_t)(8 * words)));
      stats->chunks++;
      for (uint32_t i = 0; i < c.nv; i++) stats->raw += vnl[i] == ~0ull;
    }
    return st.drain();
  };
  rc = body();
  (void)hipStreamSynchronize(s);  // before tmp goes
  return rc;
}

// The device side of a FIFO section: the count table (padded to 8 bytes, the padding zero) and its scan.
struct CkFifoTab {
  DevMem mem;
  uint32_t *n = nullptr;
  uint64_t *off = nullptr;
  int init(uint32_t Hl, hipStream_t s) {
    GXTRY(mem.take(n, (size_t)ck_pad8(4ull * Hl), 0, s));
    return mem.take(off, sizeof(uint64_t) * ((size_t)Hl + 1));
  }
};
template <class F>
static void ck_fifo_team(uint32_t Q, F &&f) {
  if (Q > CK_FIFO_WAVE_Q) f(std::integral_constant<int, 256>{});
  else f(std::integral_constant<int, 64>{});
}

// The FIFO section, to the file: the count table, then chunks of consecutive hosts' windows.
static int ck_save_fifo(gx_engine *e, CkStage &st, uint32_t *chunks, uint64_t *jobs_out) {
  const Dev &d = e->d;
  hipStream_t s = e->stream;
  if (!d.Hl) return GX_OK;
  CkFifoTab tab;  // freed on return, after the hipStreamSynchronize below
  GXTRY(tab.init(d.Hl, s));
  auto body = [&]() -> int {
    st.time_begin(CK_T_FIFO);
    k_ck_fcount<<<nblk(d.Hl, 256), 256, 0, s>>>(d.hs, d.Hl, tab.n);
    k_ck_foffsets<<<1, 256, 0, s>>>(tab.n, d.Hl, tab.off);
    st.time_end();
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> n(d.Hl);
    HIPCHK(hipMemcpyAsync(n.data(), tab.n, sizeof(uint32_t) * d.Hl, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (uint32_t v = 0; v < d.Hl; v++)
      if (n[v] > d.Q) return GX_EIO;  // (cannot happen: the stored window never exceeds the ring)
    const uint64_t tb = ck_pad8(4ull * d.Hl);
    for (uint64_t o = 0; o < tb; o += st.half)
      GXTRY(st.push((const uint8_t *)tab.n + o, (size_t)std::min<uint64_t>(st.half, tb - o)));
    for (uint32_t v0 = 0; v0 < d.Hl;) {
      uint64_t jobs;
      const uint32_t nv = ck_fifo_chunk_hosts(n.data(), v0, d.Hl, st.half, &jobs);
      if (!nv) return GX_ENOMEM;  // (cannot happen: ck_half_bytes, n <= Q)
      if (jobs) {
        const CkFifo c{d.hs + v0, d.fifo + (size_t)v0 * d.Q, tab.n + v0, tab.off + v0, d.Q, nv, jobs, (gx_job *)st.dev};
        st.time_begin(CK_T_FIFO);
        ck_fifo_team(d.Q, [&](auto T) { k_ck_fpack<T()><<<nblk(nv, 256 / T()), 256, 0, s>>>(c); });
        st.time_end();
        HIPCHK(hipGetLastError());
        GXTRY(st.push(st.dev, (size_t)(sizeof(gx_job) * jobs)));
        ++*chunks;
        *jobs_out += jobs;
      }
      v0 += nv;
    }
    return st.drain();
  };
  const int rc = body();
  (void)hipStreamSynchronize(s);  // before tab goes
  return rc;
}

static void ck_info_begin(gx_ckpt_info *info) {
  if (info) memset(info, 0, sizeof(*info));
}
static void ck_info_section(gx_ckpt_info *info, const CkSection &x) {
  if (!info) return;
  if (info->n_sections < GX_CKPT_MAX_SECTIONS) info->sections[info->n_sections] = {x.id, x.coding, x.raw, x.stored};
  info->n_sections++;
  info->raw_bytes += x.raw;
  info->stored_bytes += x.stored;
}
static void ck_info_times(gx_ckpt_info *info, gx_ckpt_coded_info *coded, CkStage &st) {
  if (!info && !coded) return;
  float ms[CK_T_N] = {0};
  st.time_collect(ms);
  if (info) {
    info->base_ms = ms[CK_T_VIEW];
    info->count_ms = ms[CK_T_VIEW + 1];
    info->emit_ms = ms[CK_T_VIEW + 2];
    info->coder_ms = info->base_ms + info->count_ms + info->emit_ms;
  }
  if (coded) {
    coded->srvt_base_ms = ms[CK_T_SRVT];
    coded->srvt_count_ms = ms[CK_T_SRVT + 1];
    coded->srvt_emit_ms = ms[CK_T_SRVT + 2];
    coded->srvt_ms = coded->srvt_base_ms + coded->srvt_count_ms + coded->srvt_emit_ms;
    coded->fifo_ms = ms[CK_T_FIFO];
  }
}

static int ck_save(gx_engine *e, const char *path, uint32_t code, gx_ckpt_info *info, gx_ckpt_coded_info *coded, bool *opened) {
  Dev &d = e->d;
  HIPCHK(hipStreamSynchronize(e->stream));
  const bool srvt = (code & GX_CKPT_CODE_SRVT) && e->mem.find(GX_CK_SRVT);
  const bool fifo = (code & GX_CKPT_CODE_FIFO) && e->mem.find(GX_CK_FIFO);
  size_t half;
  GXTRY(ck_half_bytes(e, srvt, fifo, &half));
  CkStage st;
  GXTRY(st.init(e->stream, half, true, false));
  st.f = fopen(path, "wb");
  if (!st.f) return GX_EIO;
  *opened = true;
  CkHeader h;
  h.p = d.p;
  h.p.t0_ns += d.epoch;  // as gx_create was given it
  h.round = d.round;
  std::vector<const DevMem::Buf *> bufs;
  for (uint32_t id = 1; id < GX_CK_ID_END; id++)
    if (const DevMem::Buf *b = e->mem.find(id)) bufs.push_back(b);
  if (bufs.size() > GX_CKPT_MAX_SECTIONS) return GX_EINVAL;
  const std::vector<uint8_t> blank(ck_head_bytes(bufs.size()), 0);
  if (fwrite(blank.data(), 1, blank.size(), st.f) != blank.size()) return GX_EIO;
  const uint8_t zero[8] = {0};
  for (const DevMem::Buf *b : bufs) {
    CkSection x{b->id, GX_CKPT_RAW, b->bytes, 0, 0, 0};
    st.sum = CkSum();
    if (b->id == GX_CK_VIEW) {
      x.coding = GX_CKPT_VIEWS;
      CkRowStats rs;
      GXTRY(ck_save_rows(e, st, ck_rows_views(e), &rs));
      if (info) {
        info->chunks = rs.chunks;
        info->views_raw = rs.raw;
      }
    } else if (b->id == GX_CK_SRVT && srvt) {
      x.coding = GX_CKPT_VIEWS;
      CkRowStats rs;
      GXTRY(ck_save_rows(e, st, ck_rows_srvt(e), &rs));
      if (coded) {
        coded->srvt_chunks = rs.chunks;
        coded->srvt_rows_raw = rs.raw;
      }
    } else if (b->id == GX_CK_FIFO && fifo) {
      x.coding = GX_CKPT_FIFO;
      uint32_t chunks = 0;
      uint64_t jobs = 0;
      GXTRY(ck_save_fifo(e, st, &chunks, &jobs));
      if (coded) {
        coded->fifo_chunks = chunks;
        coded->fifo_jobs = jobs;
      }
    } else {
      for (size_t o = 0; o < b->bytes; o += st.half)
        GXTRY(st.push((const uint8_t *)b->p + o, std::min(st.half, b->bytes - o)));
      GXTRY(st.drain());
    }
    x.stored = st.sum.bytes;
    x.sum = st.sum.get();
    const size_t pad = (size_t)(ck_pad8(x.stored) - x.stored);
    if (pad && fwrite(zero, 1, pad, st.f) != pad) return GX_EIO;
    h.sec.push_back(x);
    ck_info_section(info, x);
  }
  const std::vector<uint8_t> head = ck_head_encode(h);
  if (info) info->file_bytes = (uint64_t)ftell(st.f);
  if (fseek(st.f, 0, SEEK_SET) || fwrite(head.data(), 1, head.size(), st.f) != head.size()) return GX_EIO;
  const int bad = fclose(st.f);
  st.f = nullptr;
  if (bad) return GX_EIO;
  HIPCHK(hipStreamSynchronize(e->stream));
  ck_info_times(info, coded, st);
  return GX_OK;
}

static int ck_open(const char *path, FILE **f, CkHeader *h) {
  *f = fopen(path, "rb");
  if (!*f) return GX_EIO;
  uint64_t size = 0;
  if (fseek(*f, 0, SEEK_END) == 0) {
    const long at = ftell(*f);
    if (at > 0) size = (uint64_t)at;
  }
  return ck_head_read(*f, size, h);
}

// every section's checksum, through buf (cap bytes, a multiple of 8)
static int ck_verify(FILE *f, const CkHeader &h, uint8_t *buf, size_t cap) {
  for (const CkSection &x : h.sec) {
    if (fseek(f, (long)x.at, SEEK_SET)) return GX_EIO;
    CkSum sum;
    for (uint64_t o = 0; o < x.stored;) {
      const size_t n = (size_t)std::min<uint64_t>(cap, x.stored - o);
      if (fread(buf, 1, n, f) != n) return GX_EIO;
      sum.add(buf, n);
      o += n;
    }
    if (sum.get() != x.sum) return GX_EIO;
  }
  return GX_OK;
}

// load: a half is free again once the copy queued from it has run
static int ck_half_free(CkStage &st, int i) {
  if (!st.busy[i]) return GX_OK;
  HIPCHK(hipEventSynchronize(st.ev[i]));
  st.busy[i] = false;
  return GX_OK;
}
static int ck_load_raw(CkStage &st, FILE *f, void *dst, uint64_t bytes) {
  for (uint64_t o = 0; o < bytes;) {
    const size_t n = (size_t)std::min<uint64_t>(st.half, bytes - o);
    GXTRY(ck_half_free(st, st.k));
    if (fread(st.pin[st.k], 1, n, f) != n) return GX_EIO;
    HIPCHK(hipMemcpyAsync((uint8_t *)dst + o, st.pin[st.k], n, hipMemcpyHostToDevice, st.s));
    HIPCHK(hipEventRecord(st.ev[st.k], st.s));
    st.busy[st.k] = true;
    st.k ^= 1;
    o += n;
  }
  return GX_OK;
}

// One row-coded section of the file into table t.
static int ck_load_rows(gx_engine *e, CkStage &st, FILE *f, const CkSection &x, const CkRows &t, CkRowStats *stats) {
  hipStream_t s = e->stream;
  if (x.stored % 8 || x.stored < 8ull * t.W) return GX_EIO;
  DevMem tmp;
  const uint32_t cv = ck_chunk_rows(t, st.half);
  if (!cv) return t.rows ? GX_ENOMEM : GX_OK;
  CkChunk c{};
  uint32_t *err;
  uint64_t *base;
  GXTRY(tmp.take(base, sizeof(uint64_t) * t.W));
  GXTRY(ck_chunk_alloc(tmp, t, cv, &c, &err, s));
  c.base = base;
  c.buf = (uint64_t *)st.dev;
  auto body = [&]() -> int {
    GXTRY(ck_load_raw(st, f, base, 8ull * t.W));
    GXTRY(ck_half_free(st, 0));
    GXTRY(ck_half_free(st, 1));
    uint64_t left = x.stored - 8ull * t.W;  // of the section, not read yet
    size_t have = 0, pos = 0;  // pin[k] holds `have` bytes of the section; the records before `pos` are decoded
    int k = 0;
    uint32_t v0 = 0;
    while (v0 < t.rows) {
      // the complete records at the cursor
      const uint64_t *w = (const uint64_t *)(st.pin[k] + pos);
      uint64_t at = 0;
      uint32_t nv = 0;
      while (nv < cv && v0 + nv < t.rows) {
        const int64_t len = ck_view_record_words(w + at, (have - pos) / 8 - at, t.W, c.nblk, c.PW);
        if (len < 0) return GX_EIO;
        if (!len) break;
        st.voff_pin[nv++] = at;
        at += (uint64_t)len;
      }
      if (!nv) {
        // No whole record is left in this half: its rest moves to the front of the other one (the
        // copies out of both have run: the stream is idle after every chunk) and that one is filled
        // from the file. A record fits a half, so a rest that cannot grow is a record that does not
        // end inside the section.
        if (!left || (pos == 0 && have == st.half)) return GX_EIO;
        memcpy(st.pin[k ^ 1], st.pin[k] + pos, have - pos);
        have -= pos;
        pos = 0;
        k ^= 1;
        const size_t more = (size_t)std::min<uint64_t>(st.half - have, left);
        if (fread(st.pin[k] + have, 1, more, f) != more) return GX_EIO;
        have += more;
        left -= more;
        continue;
      }
      st.voff_pin[nv] = at;
      c.nv = nv;
      c.view = t.p + (size_t)v0 * t.W;
      HIPCHK(hipMemcpyAsync(st.dev, w, (size_t)(8 * at), hipMemcpyHostToDevice, s));
      HIPCHK(hipMemcpyAsync(c.voff, st.voff_pin, sizeof(uint64_t) * (nv + 1), hipMemcpyHostToDevice, s));
      const unsigned gu = nblk((size_t)nv * c.nblk, 4);
      st.time_begin(t.t0 + 1);
      k_ck_dcount<<<gu, 256, 0, s>>>(c, err);
      k_ck_vscan<false><<<nv, 256, 0, s>>>(c, err);
      st.time_end();
      HIPCHK(hipGetLastError());
      uint32_t bad = 0;
      HIPCHK(hipMemcpyAsync(&bad, err, sizeof(bad), hipMemcpyDeviceToHost, s));
      HIPCHK(hipStreamSynchronize(s));
      if (bad) return GX_EIO;
      st.time_begin(t.t0 + 2);
      with_flag(t.vec, [&](auto V) { k_ck_expand<V()><<<gu, 256, 0, s>>>(c); });
      st.time_end();
      HIPCHK(hipGetLastError());
      stats->chunks++;
      for (uint32_t i = 0; i < nv; i++) stats->raw += w[st.voff_pin[i]] == ~0ull;
      pos += (size_t)(8 * at);
      v0 += nv;
    }
    return have != pos || left ? GX_EIO : GX_OK;  // the records fill the section exactly
  };
  const int rc = body();
  (void)hipStreamSynchronize(s);  // before tmp goes
  return rc;
}

// The FIFO section of the file into the rings. The host states are restored already, on the same
// stream (ck_head_read: their section is in the file, ahead of this one). The host walks the count
// table (ck_fifo_table_jobs) before a kernel sees it; k_ck_funpack compares it with the host states.
static int ck_load_fifo(gx_engine *e, CkStage &st, FILE *f, const CkSection &x) {
  const Dev &d = e->d;
  hipStream_t s = e->stream;
  if (!d.Hl) return x.stored ? GX_EIO : GX_OK;
  const uint64_t tb = ck_pad8(4ull * d.Hl);
  if (x.stored < tb) return GX_EIO;
  std::vector<uint32_t> n((size_t)(tb / 4));
  if (fread(n.data(), 1, (size_t)tb, f) != tb) return GX_EIO;
  if (ck_fifo_table_jobs(n.data(), tb, d.Hl, d.Q, x.stored) < 0) return GX_EIO;
  CkFifoTab tab;
  uint32_t *err;
  GXTRY(tab.init(d.Hl, s));
  GXTRY(tab.mem.take(err, sizeof(uint32_t), 0, s));
  auto body = [&]() -> int {
    HIPCHK(hipMemcpyAsync(tab.n, n.data(), (size_t)tb, hipMemcpyHostToDevice, s));
    st.time_begin(CK_T_FIFO);
    k_ck_foffsets<<<1, 256, 0, s>>>(tab.n, d.Hl, tab.off);
    st.time_end();
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(s));  // n is pageable: the copy has left it
    for (uint32_t v0 = 0; v0 < d.Hl;) {
      uint64_t jobs;
      const uint32_t nv = ck_fifo_chunk_hosts(n.data(), v0, d.Hl, st.half, &jobs);
      if (!nv) return GX_ENOMEM;  // (cannot happen: ck_half_bytes, n <= Q)
      const size_t bytes = (size_t)(sizeof(gx_job) * jobs);
      const int k = st.k;
      GXTRY(ck_half_free(st, k));
      if (bytes && fread(st.pin[k], 1, bytes, f) != bytes) return GX_EIO;
      // (the copy into the one staging area waits, in stream order, for the kernel before it)
      if (bytes) HIPCHK(hipMemcpyAsync(st.dev, st.pin[k], bytes, hipMemcpyHostToDevice, s));
      const CkFifo c{d.hs + v0, d.fifo + (size_t)v0 * d.Q, tab.n + v0, tab.off + v0, d.Q, nv, jobs, (gx_job *)st.dev};
      st.time_begin(CK_T_FIFO);
      ck_fifo_team(d.Q, [&](auto T) { k_ck_funpack<T()><<<nblk(nv, 256 / T()), 256, 0, s>>>(c, err); });
      st.time_end();
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(st.ev[k], s));
      st.busy[k] = true;
      st.k ^= 1;
      v0 += nv;
    }
    uint32_t bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, err, sizeof(bad), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return bad ? GX_EIO : GX_OK;
  };
  const int rc = body();
  (void)hipStreamSynchronize(s);  // before tab goes
  return rc;
}

static int ck_load_into(gx_engine *e, FILE *f, const CkHeader &h, gx_ckpt_info *info) {
  Dev &d = e->d;
  // each section against the buffer gx_create allocated for these params
  bool srvt = false, fifo = false;
  for (const CkSection &x : h.sec) {
    const DevMem::Buf *b = e->mem.find(x.id);
    if (b && b->bytes != x.raw) return GX_EINVAL;
    if (b && x.id == GX_CK_SRVT && x.coding == GX_CKPT_VIEWS) srvt = true;
    if (b && x.coding == GX_CKPT_FIFO) fifo = true;
  }
  size_t half;
  GXTRY(ck_half_bytes(e, srvt, fifo, &half));
  CkStage st;
  GXTRY(st.init(e->stream, half, true, true));
  GXTRY(ck_verify(f, h, st.pin[0], st.half));
  for (const CkSection &x : h.sec) {
    const DevMem::Buf *b = e->mem.find(x.id);
    if (!b) continue;  // gx_ckpt.h FORK: a section the new engine lacks holds its initial state
    if (fseek(f, (long)x.at, SEEK_SET)) return GX_EIO;
    if (x.coding == GX_CKPT_VIEWS) {  // (ck_head_read: GX_CK_VIEW or GX_CK_SRVT)
      CkRowStats rs;
      GXTRY(ck_load_rows(e, st, f, x, x.id == GX_CK_VIEW ? ck_rows_views(e) : ck_rows_srvt(e), &rs));
      if (info && x.id == GX_CK_VIEW) {
        info->chunks = rs.chunks;
        info->views_raw = rs.raw;
      }
    } else if (x.coding == GX_CKPT_FIFO) {
      GXTRY(ck_load_fifo(e, st, f, x));
    } else {
      GXTRY(ck_load_raw(st, f, b->p, x.stored));
    }
    ck_info_section(info, x);
  }
  HIPCHK(hipStreamSynchronize(e->stream));
  ck_info_times(info, nullptr, st);
  d.round = h.round;
  set_round_fields(e);
  quiet_invalidate(e);
  return sync_check(e);
}

extern "C" {

int gx_ckpt_save(gx_engine *e, const char *path, gx_ckpt_info *info) { return gx_ckpt_save_coded(e, path, 0, info, nullptr); }

int gx_ckpt_save_coded(gx_engine *e, const char *path, uint32_t code, gx_ckpt_info *info, gx_ckpt_coded_info *coded) {
  if (!e || !path || (code & ~(GX_CKPT_CODE_SRVT | GX_CKPT_CODE_FIFO))) return GX_EINVAL;
  if (e->round_open || e->side_pending) return GX_EINVAL;  // gx_ckpt.h: only between rounds
  GXTRY(enter(e, ENTRY_READ));
  ck_info_begin(info);
  if (coded) memset(coded, 0, sizeof(*coded));
  bool opened = false;
  const int rc = ck_save(e, path, code, info, coded, &opened);
  if (rc) {
    (void)hipGetLastError();
    struct stat sb;  // no half-written file stays (a device node or pipe given as the path does)
    if (opened && stat(path, &sb) == 0 && S_ISREG(sb.st_mode)) (void)remove(path);
  }
  return rc;
}

int gx_ckpt_params(const char *path, gx_params *out, int64_t *round) {
  if (!path || !out || !round) return GX_EINVAL;
  FILE *f;
  CkHeader h;
  const int rc = ck_open(path, &f, &h);
  if (f) fclose(f);
  if (rc) return rc;
  *out = h.p;
  *round = h.round;
  return GX_OK;
}

int gx_ckpt_load(const char *path, const gx_params *override, gx_engine **out, gx_ckpt_info *info) {
  if (!path || !out) return GX_EINVAL;
  *out = nullptr;
  ck_info_begin(info);
  FILE *f;
  CkHeader h;
  int rc = ck_open(path, &f, &h);
  gx_engine *e = nullptr;
  if (!rc && override) rc = ck_fork_check(h.p, *override, h.round);
  if (!rc) rc = gx_create(override ? override : &h.p, &e);
  if (!rc) rc = ck_load_into(e, f, h, info);
  if (f) fclose(f);
  if (rc) {
    (void)hipGetLastError();
    if (e) gx_destroy(e);
    return rc;
  }
  if (info) {
    info->file_bytes = ck_head_bytes(h.sec.size());
    for (const CkSection &x : h.sec) info->file_bytes += ck_pad8(x.stored);
  }
  *out = e;
  return GX_OK;
}

}  // extern "C"
