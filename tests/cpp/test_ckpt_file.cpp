// The checkpoint file's host side (sidecar_amd/csrc/gx_ckpt_file.hpp) as a stand-alone program:
// checksum, header and section table round trip, the refusals of ck_head_read, the fork rule and the
// walk over view records. No device; built with -fsanitize=address,undefined by
// tests/test_ckpt_file_cpp.py. Usage: test_ckpt_file <scratch file> [<checksum file>]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../sidecar_amd/csrc/gx_ckpt_file.hpp"

static int failures = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);     \
      failures++;                                             \
    }                                                         \
  } while (0)

static std::vector<uint8_t> bytes_of(size_t n, uint64_t seed) {
  std::vector<uint8_t> b(n);
  for (size_t i = 0; i < n; i++) b[i] = (uint8_t)(CkSum::mix(i, seed) >> 24);
  return b;
}

static void put(const char *path, const std::vector<uint8_t> &b) {
  FILE *f = fopen(path, "wb");
  if (!f || (!b.empty() && fwrite(b.data(), 1, b.size(), f) != b.size())) {
    printf("cannot write %s\n", path);
    exit(2);
  }
  fclose(f);
}

static int read_head(const char *path, CkHeader *h) {
  FILE *f = fopen(path, "rb");
  if (!f) return GX_EIO;
  fseek(f, 0, SEEK_END);
  const uint64_t size = (uint64_t)ftell(f);
  const int rc = ck_head_read(f, size, h);
  fclose(f);
  return rc;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const char *path = argv[1];

  // checksum: pieces give what the whole gives; a changed byte, a changed length change it
  for (size_t n : {(size_t)0, (size_t)1, (size_t)7, (size_t)8, (size_t)9, (size_t)4096, (size_t)4099}) {
    const std::vector<uint8_t> b = bytes_of(n, 7);
    CkSum whole, parts;
    whole.add(b.data(), n);
    const size_t cut = n / 16 * 8;
    parts.add(b.data(), cut);
    parts.add(b.data() + cut, n - cut);
    CHECK(whole.get() == parts.get());
    if (n) {
      std::vector<uint8_t> c = b;
      c[n / 2] ^= 1;
      CkSum x;
      x.add(c.data(), n);
      CHECK(x.get() != whole.get());
      CkSum y;
      y.add(b.data(), n - 1);
      CHECK(y.get() != whole.get());
    }
  }
  if (argc > 2) {  // the sums of a few byte strings, for the numpy reference to compare
    FILE *f = fopen(argv[2], "w");
    for (size_t n : {(size_t)0, (size_t)5, (size_t)64, (size_t)1001}) {
      const std::vector<uint8_t> b = bytes_of(n, 3);
      CkSum x;
      x.add(b.data(), n);
      fprintf(f, "%zu %llu\n", n, (unsigned long long)x.get());
    }
    fclose(f);
  }

  // header + table + sections: round trip
  CkHeader h;
  memset(&h.p, 0, sizeof(h.p));
  h.p.n_hosts = 33;
  h.p.n_services = 3;
  h.p.storm_round = -1;
  h.p.depart_round = -1;
  h.round = 20;
  const std::vector<uint8_t> s1 = bytes_of(99 * 8, 1), s2 = bytes_of(13, 2);
  CkSum c1, c2;
  c1.add(s1.data(), s1.size());
  c2.add(s2.data(), s2.size());
  h.sec.push_back({GX_CK_VIEW, GX_CKPT_VIEWS, 33 * 99 * 8, s1.size(), c1.get(), 0});
  h.sec.push_back({GX_CK_TICK, GX_CKPT_RAW, s2.size(), s2.size(), c2.get(), 0});
  std::vector<uint8_t> file = ck_head_encode(h);
  CHECK(file.size() == ck_head_bytes(2));
  file.insert(file.end(), s1.begin(), s1.end());
  file.insert(file.end(), s2.begin(), s2.end());
  file.resize(file.size() + 3, 0);  // 13 -> 16
  put(path, file);
  CkHeader g;
  CHECK(read_head(path, &g) == GX_OK);
  CHECK(g.round == 20 && g.sec.size() == 2 && !memcmp(&g.p, &h.p, sizeof(gx_params)));
  CHECK(g.sec[0].at == ck_head_bytes(2) && g.sec[1].at == ck_head_bytes(2) + s1.size());
  CHECK(g.sec[1].stored == 13 && g.sec[1].sum == c2.get());

  // refusals: every truncation, every flipped header or table byte
  for (size_t n = 0; n < file.size(); n += (n < ck_head_bytes(2) + 16 ? 1 : 97)) {
    put(path, std::vector<uint8_t>(file.begin(), file.begin() + n));
    CkHeader x;
    CHECK(read_head(path, &x) == GX_EIO);
  }
  for (size_t i = 0; i < ck_head_bytes(2); i++) {
    std::vector<uint8_t> b = file;
    b[i] ^= 0x10;
    put(path, b);
    CkHeader x;
    CHECK(read_head(path, &x) == GX_EIO);
  }
  {  // a well-formed header of another format or ABI version: GX_EINVAL
    for (size_t at : {(size_t)8, (size_t)12}) {
      std::vector<uint8_t> b = file;
      b[at] ^= 1;
      memset(&b[32], 0, 8);
      CkSum c;
      c.add(b.data(), ck_head_bytes(2));
      const uint64_t sum = c.get();
      memcpy(&b[32], &sum, 8);
      put(path, b);
      CkHeader x;
      CHECK(read_head(path, &x) == GX_EINVAL);
    }
  }
  {  // trailing bytes
    std::vector<uint8_t> b = file;
    b.resize(b.size() + 8, 0);
    put(path, b);
    CkHeader x;
    CHECK(read_head(path, &x) == GX_EIO);
  }

  // the fork rule
  gx_params a = h.p, o = a;
  CHECK(ck_fork_check(a, o, 20) == GX_OK);
  o.device = 3;
  CHECK(ck_fork_check(a, o, 20) == GX_OK);
  o.storm_round = 30;
  CHECK(ck_fork_check(a, o, 20) == GX_OK);
  o.storm_round = 21;
  CHECK(ck_fork_check(a, o, 20) == GX_OK);
  o.storm_round = 20;  // begins at the saved round: begun
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);
  o.storm_round = 5;
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);
  o = a;
  a.storm_round = 5;  // the saved storm has begun
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);
  a.storm_round = 30;  // a saved one that has not may go or move
  CHECK(ck_fork_check(a, o, 20) == GX_OK);
  a = o = h.p;
  o.partition_start = 30;
  o.partition_end = 45;
  CHECK(ck_fork_check(a, o, 20) == GX_OK);
  o.partition_start = 10;
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);
  o = a;
  o.depart_round = 30;
  o.depart_ppm = 100000;
  CHECK(ck_fork_check(a, o, 20) == GX_OK);
  o.depart_round = 3;
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);
  o = a;
  o.seed ^= 1;
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);
  o = a;
  o.ae_period_rounds = 7;
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);
  o = a;
  o.n_hosts = 34;
  CHECK(ck_fork_check(a, o, 20) == GX_EINVAL);

  // the walk over view records: R = 770 (2 blocks, 1 present word)
  {
    const uint64_t R = 770, nb = 2, PW = 1;
    std::vector<uint64_t> w(2000, 0);
    CHECK(ck_view_record_words(w.data(), 0, R, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), 1, R, nb, PW) == 0);   // needs the present word
    CHECK(ck_view_record_words(w.data(), 2, R, nb, PW) == 2);   // n_lit 0, nothing present
    w[0] = 3;
    CHECK(ck_view_record_words(w.data(), 2, R, nb, PW) == -1);  // literals without a present block
    w[1] = 2;  // block 1
    CHECK(ck_view_record_words(w.data(), 12, R, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), 13, R, nb, PW) == 13);
    w[1] = 7;  // three blocks of two
    CHECK(ck_view_record_words(w.data(), 100, R, nb, PW) == -1);
    w[1] = 3;
    w[0] = 1;  // fewer literals than present blocks
    CHECK(ck_view_record_words(w.data(), 100, R, nb, PW) == -1);
    w[0] = 771;
    CHECK(ck_view_record_words(w.data(), 2000, R, nb, PW) == -1);
    w[0] = 760;  // 1 + 1 + 16 + 760 >= R: such a view is stored raw
    CHECK(ck_view_record_words(w.data(), 2000, R, nb, PW) == -1);
    w[0] = ~0ull;
    CHECK(ck_view_record_words(w.data(), 770, R, nb, PW) == 0);
    CHECK(ck_view_record_words(w.data(), 771, R, nb, PW) == 771);
  }
  remove(path);
  printf("failures=%d\n", failures);
  return failures ? 1 : 0;
}
