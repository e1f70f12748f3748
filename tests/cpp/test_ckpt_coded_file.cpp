// The host-side walks of the coded checkpoint sections (sidecar_amd/csrc/gx_ckpt_file.hpp) as a
// stand-alone program: the (id, coding) pairs the section table admits, the FIFO SECTION's count
// table and its refusals, the chunks of hosts the FIFO coder forms, and the walk over server-time
// row records at W = 514. No device; built with -fsanitize=address,undefined by
// tests/test_ckpt_coded_file_cpp.py. Usage: test_ckpt_coded_file <scratch file>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../sidecar_amd/csrc/gx_ckpt_file.hpp"

static int failures = 0;
#define CHECK(x)                                          \
  do {                                                    \
    if (!(x)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x); \
      failures++;                                         \
    }                                                     \
  } while (0)

// a file of sections whose bodies are `stored` zero bytes each (ck_head_read checks no body)
static int head_rc(const char *path, const std::vector<CkSection> &sec) {
  CkHeader h;
  memset(&h.p, 0, sizeof(h.p));
  h.p.n_hosts = 33;
  h.p.n_services = 3;
  h.round = 12;
  h.sec = sec;
  std::vector<uint8_t> file = ck_head_encode(h);
  for (const CkSection &s : sec) file.resize(file.size() + ck_pad8(s.stored), 0);
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(file.data(), 1, file.size(), f) != file.size()) {
    printf("cannot write %s\n", path);
    exit(2);
  }
  fclose(f);
  f = fopen(path, "rb");
  CkHeader g;
  const int rc = ck_head_read(f, file.size(), &g);
  fclose(f);
  if (rc == GX_OK) CHECK(g.sec.size() == sec.size());
  return rc;
}

// the exact-size table of n (heap: the sanitizer sees a read past it)
static std::vector<uint32_t> table_of(const std::vector<uint32_t> &n) {
  std::vector<uint32_t> t(n);
  if (t.size() % 2) t.push_back(0);
  return t;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const char *path = argv[1];

  // the admitted (id, coding) pairs
  CHECK(ck_coding_admitted(GX_CK_VIEW, GX_CKPT_VIEWS) && ck_coding_admitted(GX_CK_SRVT, GX_CKPT_VIEWS));
  CHECK(ck_coding_admitted(GX_CK_FIFO, GX_CKPT_FIFO));
  for (uint32_t id = 1; id < GX_CK_ID_END; id++) {
    CHECK(ck_coding_admitted(id, GX_CKPT_RAW));
    CHECK(ck_coding_admitted(id, GX_CKPT_VIEWS) == (id == GX_CK_VIEW || id == GX_CK_SRVT));
    CHECK(ck_coding_admitted(id, GX_CKPT_FIFO) == (id == GX_CK_FIFO));
    CHECK(!ck_coding_admitted(id, 3u));
  }
  // ... as ck_head_read applies them: Hl = 33, Q = 8, H = 33 (W = 66)
  const uint64_t Hl = 33, Q = 8, W = 66;
  const CkSection view{GX_CK_VIEW, GX_CKPT_VIEWS, 8 * Hl * 99, 8 * 99 + 16 * Hl, 0, 0};
  const CkSection hs{GX_CK_HS, GX_CKPT_RAW, 80 * Hl, 80 * Hl, 0, 0};
  const CkSection fifo{GX_CK_FIFO, GX_CKPT_FIFO, 16 * Hl * Q, ck_pad8(4 * Hl) + 16 * 5, 0, 0};
  const CkSection srvt{GX_CK_SRVT, GX_CKPT_VIEWS, 8 * Hl * W, 8 * W + 16 * Hl, 0, 0};
  CHECK(head_rc(path, {view, hs, fifo, srvt}) == GX_OK);
  CHECK(head_rc(path, {view, fifo, srvt}) == GX_EIO);  // a FIFO section without the host states
  CHECK(head_rc(path, {fifo}) == GX_EIO);
  {
    CkSection x = view;
    x.coding = GX_CKPT_FIFO;  // GX_CKPT_FIFO on GX_CK_VIEW
    CHECK(head_rc(path, {x, hs, fifo}) == GX_EINVAL);
    x = hs;
    x.coding = GX_CKPT_VIEWS;
    CHECK(head_rc(path, {view, x}) == GX_EINVAL);
    x = srvt;
    x.coding = GX_CKPT_FIFO;
    CHECK(head_rc(path, {view, hs, x}) == GX_EINVAL);
    x = fifo;
    x.coding = GX_CKPT_VIEWS;
    CHECK(head_rc(path, {view, hs, x}) == GX_EINVAL);
    x = fifo;
    x.coding = 3u;
    CHECK(head_rc(path, {view, hs, x}) == GX_EINVAL);
    x = fifo;
    x.coding = GX_CKPT_RAW;  // raw: stored = raw
    CHECK(head_rc(path, {view, hs, x}) == GX_EINVAL);
    x.stored = x.raw;
    CHECK(head_rc(path, {view, x}) == GX_OK);  // a raw FIFO section needs no host states beside it
  }

  // the FIFO count table
  {
    std::vector<uint32_t> n(Hl, 0);
    n[0] = 8;
    n[7] = 3;
    n[32] = 1;
    const uint64_t tb = ck_pad8(4 * Hl), full = tb + 16 * 12;
    std::vector<uint32_t> t = table_of(n);
    CHECK(tb == 136 && t.size() * 4 == tb);
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, full) == 12);
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, full - 16) == -1);  // sum of n != the section's jobs
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, full + 16) == -1);
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, full + 8) == -1);   // no whole job
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, tb - 8) == -1);     // a section shorter than its table
    CHECK(ck_fifo_table_jobs(t.data(), 0, Hl, Q, 0) == -1);
    {
      std::vector<uint32_t> part(t.begin(), t.begin() + 16);  // the table cut short: never read past
      CHECK(ck_fifo_table_jobs(part.data(), 64, Hl, Q, full) == -1);
    }
    t[7] = 9;  // n > Q
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, tb + 16 * 18) == -1);
    t[7] = 0xffffffffu;
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, full) == -1);
    t[7] = 3;
    t[33] = 1;  // padding that is not zero
    CHECK(ck_fifo_table_jobs(t.data(), tb, Hl, Q, full + 16) == -1);
    t[33] = 0;
    std::vector<uint32_t> none = table_of(std::vector<uint32_t>(Hl, 0));
    CHECK(ck_fifo_table_jobs(none.data(), tb, Hl, Q, tb) == 0);  // an empty section: pad8(4 Hl)
    std::vector<uint32_t> all = table_of(std::vector<uint32_t>(32, 8));  // an even Hl, every ring full
    CHECK(ck_fifo_table_jobs(all.data(), 128, 32, Q, 128 + 16 * 256) == 256);

    // chunks of hosts for a staging half of 16 jobs
    uint64_t jobs = 0;
    CHECK(ck_fifo_chunk_hosts(n.data(), 0, Hl, 16 * 16, &jobs) == 33 && jobs == 12);
    CHECK(ck_fifo_chunk_hosts(n.data(), 0, Hl, 16 * 10, &jobs) == 7 && jobs == 8);   // host 7's three do not fit
    CHECK(ck_fifo_chunk_hosts(n.data(), 7, Hl, 16 * 10, &jobs) == 26 && jobs == 4);
    CHECK(ck_fifo_chunk_hosts(n.data(), 0, Hl, 16 * 7, &jobs) == 0 && jobs == 0);     // the first one's alone do not
    CHECK(ck_fifo_chunk_hosts(n.data(), 1, Hl, 8, &jobs) == 6 && jobs == 0);           // empty hosts take no room
    CHECK(ck_fifo_chunk_hosts(n.data(), 33, Hl, 64, &jobs) == 0);
    uint32_t v = 0, chunks = 0;
    uint64_t total = 0;
    while (v < Hl) {  // the coder's loop: every host lands in one chunk
      const uint32_t nv = ck_fifo_chunk_hosts(n.data(), v, Hl, 16 * 8, &jobs);
      CHECK(nv > 0 && 16 * jobs <= 16 * 8);
      if (!nv) break;
      v += nv;
      total += jobs;
      chunks++;
    }
    CHECK(v == Hl && total == 12 && chunks == 2);  // hosts [0, 7) with 8 jobs, [7, 33) with 4
  }

  // the row walk at W = 514 (the server times of 257 hosts): 2 blocks, the last with 2 slots
  {
    const uint64_t Wt = 514, nb = 2, PW = 1;
    std::vector<uint64_t> w(Wt + 1, 0);
    CHECK(ck_view_record_words(w.data(), 0, Wt, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), 1, Wt, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), 2, Wt, nb, PW) == 2);  // a row that equals base
    w[0] = 2;
    w[1] = 2;  // the ragged block alone: 1 + 1 + 8 + 2
    CHECK(ck_view_record_words(w.data(), 11, Wt, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), 12, Wt, nb, PW) == 12);
    w[1] = 7;  // three present blocks of two
    CHECK(ck_view_record_words(w.data(), Wt + 1, Wt, nb, PW) == -1);
    w[1] = 3;
    w[0] = 495;  // 1 + 1 + 16 + 495 = 513 < W: the longest coded record
    CHECK(ck_view_record_words(w.data(), 512, Wt, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), 513, Wt, nb, PW) == 513);
    w[0] = 496;  // 514 words: such a row is stored raw
    CHECK(ck_view_record_words(w.data(), Wt + 1, Wt, nb, PW) == -1);
    w[0] = 515;  // more literals than slots
    CHECK(ck_view_record_words(w.data(), Wt + 1, Wt, nb, PW) == -1);
    w[0] = ~0ull;
    CHECK(ck_view_record_words(w.data(), Wt, Wt, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), Wt + 1, Wt, nb, PW) == (int64_t)(Wt + 1));
    // a chunk of records back to back, as ck_load_rows walks them
    std::vector<uint64_t> two = {0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 77};
    CHECK(ck_view_record_words(two.data(), two.size(), Wt, nb, PW) == 2);
    CHECK(ck_view_record_words(two.data() + 2, two.size() - 2, Wt, nb, PW) == 11);
    CHECK(ck_view_record_words(two.data() + 2, two.size() - 3, Wt, nb, PW) == 0);
  }
  remove(path);
  printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
