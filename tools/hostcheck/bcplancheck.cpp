// The echo store's host planner (hbbft_amd/csrc/bcplan.hpp) for the CPU: a C interface for
// tests/test_bcplan.py (a shared object driven through ctypes), and, with -DBCPLAN_MAIN, a
// stand-alone program that plans the sets it reads from standard input, which the test builds with
// -fsanitize=address,undefined.
//   g++ -O1 -std=c++17 -shared -fPIC -o libbcplancheck.so tools/hostcheck/bcplancheck.cpp
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DBCPLAN_MAIN -o bcplancheck tools/hostcheck/bcplancheck.cpp
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../hbbft_amd/csrc/bcplan.hpp"

extern "C" {

int bp_check_items(const uint32_t* inst, const uint32_t* sender, uint32_t count, uint32_t n, uint32_t insts) {
  return hbx_bcplan::check_items(inst, sender, count, n, insts);
}

int bp_check_offsets(const uint64_t* val_off, uint32_t count, uint64_t values_bytes) {
  return hbx_bcplan::check_offsets(val_off, count, values_bytes);
}

int bp_check_offsets_bad(const uint64_t* val_off, uint32_t count, uint64_t values_bytes, uint32_t* bad) {
  return hbx_bcplan::check_offsets(val_off, count, values_bytes, bad);
}

int bp_check_rows(uint64_t buf_bytes, const uint64_t* off, const uint32_t* len, const uint32_t* pitch, uint32_t inst,
                  uint32_t n, uint32_t* max_len, uint32_t* bad) {
  return hbx_bcplan::check_rows(buf_bytes, off, len, pitch, inst, n, max_len, bad);
}

// Hash blocks of the long values: blk_len[cap], blk_idx[cap][lanes]; returns the block count (only
// `cap` blocks are written).
int bp_group_long(const uint64_t* val_off, uint32_t count, uint32_t lanes, uint64_t max_value, uint32_t* blk_len,
                  uint32_t* blk_idx, uint32_t cap) {
  std::vector<uint32_t> bl, bi;
  hbx_bcplan::group_long(val_off, count, lanes, max_value, bl, bi);
  for (size_t b = 0; b < bl.size() && b < cap; b++) {
    blk_len[b] = bl[b];
    for (uint32_t q = 0; q < lanes; q++) blk_idx[b * lanes + q] = bi[b * lanes + q];
  }
  return (int)bl.size();
}

int bp_check_attempts(const uint32_t* insts, const uint8_t* roots, const uint32_t* len, const uint8_t* use, uint32_t na,
                      uint32_t n, uint32_t store_insts, uint32_t max_shard_len) {
  return hbx_bcplan::check_attempts(insts, roots, len, use, na, n, store_insts, max_shard_len);
}

uint64_t bp_work_layout(const uint32_t* len, uint32_t na, uint32_t n, uint64_t* off, uint32_t* pitch) {
  std::vector<uint64_t> o;
  std::vector<uint32_t> p;
  const uint64_t total = hbx_bcplan::work_layout(len, na, n, o, p);
  for (uint32_t a = 0; a < na; a++) off[a] = o[a], pitch[a] = p[a];
  return total;
}

int bp_check_out(const uint32_t* len, const uint64_t* out_off, uint32_t na, uint32_t k, uint64_t out_bytes) {
  return hbx_bcplan::check_out(len, out_off, na, k, out_bytes);
}

int bp_check_out_bad(const uint32_t* len, const uint64_t* out_off, uint32_t na, uint32_t k, uint64_t out_bytes,
                     uint32_t* bad) {
  return hbx_bcplan::check_out(len, out_off, na, k, out_bytes, bad);
}
}

#ifdef BCPLAN_MAIN
// Input, one set per line:
//   add n insts max_value lanes values_bytes count  inst0 sender0 ..  off0 .. off_count
//   dec n insts max_shard_len k out_bytes na  inst0 rootbyte0 len0 usebits0 out_off0 ..
//   row n buf_bytes inst  off0 len0 pitch0 ..
// (a root is its byte repeated 32 times; usebits: bit i = sender i allowed, n <= 32).
// Output: "rc R" on a rejection ("rc R bad0 bad1" for row); else for add "blocks B" and per block
// "len L idx ..", for dec "total T" and per attempt "off O pitch P", for row "max M".
static std::vector<unsigned long long> take(size_t count) {
  std::vector<unsigned long long> v(count);
  for (auto& x : v)
    if (scanf("%llu", &x) != 1) exit(2);
  return v;
}

int main() {
  char kind[8];
  while (scanf("%7s", kind) == 1) {
    const auto h = take(kind[0] == 'r' ? 3 : 6);
    const uint32_t n = (uint32_t)h[0];
    if (kind[0] == 'a') {
      const uint32_t count = (uint32_t)h[5];
      const auto items = take(2 * (size_t)count), offs = take((size_t)count + 1);
      std::vector<uint32_t> in(count), sn(count);
      for (size_t j = 0; j < count; j++) in[j] = (uint32_t)items[2 * j], sn[j] = (uint32_t)items[2 * j + 1];
      std::vector<uint64_t> off(offs.begin(), offs.end());
      int rc = hbx_bcplan::check_items(in.data(), sn.data(), count, n, (uint32_t)h[1]);
      if (!rc) rc = hbx_bcplan::check_offsets(off.data(), count, h[4]);
      if (rc) printf("rc %d\n", rc);
      if (rc) continue;
      std::vector<uint32_t> bl, bi;
      hbx_bcplan::group_long(off.data(), count, (uint32_t)h[3], h[2], bl, bi);
      printf("blocks %zu\n", bl.size());
      for (size_t b = 0; b < bl.size(); b++) {
        printf("len %u idx", bl[b]);
        for (size_t q = 0; q < h[3]; q++) printf(" %u", bi[b * h[3] + q]);
        printf("\n");
      }
    } else if (kind[0] == 'd') {
      const uint32_t na = (uint32_t)h[5];
      const auto rows = take(5 * (size_t)na);
      std::vector<uint32_t> in(na), len(na);
      std::vector<uint8_t> roots((size_t)na * 32), use((size_t)na * n);
      std::vector<uint64_t> out_off(na);
      for (size_t a = 0; a < na; a++) {
        in[a] = (uint32_t)rows[5 * a], len[a] = (uint32_t)rows[5 * a + 2], out_off[a] = rows[5 * a + 4];
        for (int b = 0; b < 32; b++) roots[a * 32 + b] = (uint8_t)rows[5 * a + 1];
        for (size_t i = 0; i < n; i++) use[a * n + i] = (uint8_t)((rows[5 * a + 3] >> i) & 1);
      }
      int rc = hbx_bcplan::check_attempts(in.data(), roots.data(), len.data(), use.data(), na, n, h[1], h[2]);
      if (!rc) rc = hbx_bcplan::check_out(len.data(), out_off.data(), na, (uint32_t)h[3], h[4]);
      if (rc) printf("rc %d\n", rc);
      if (rc) continue;
      std::vector<uint64_t> off;
      std::vector<uint32_t> pitch;
      printf("total %llu\n", (unsigned long long)hbx_bcplan::work_layout(len.data(), na, n, off, pitch));
      for (size_t a = 0; a < na; a++) printf("off %llu pitch %u\n", (unsigned long long)off[a], pitch[a]);
    } else {
      const uint32_t inst = (uint32_t)h[2];
      const auto rows = take(3 * (size_t)inst);
      std::vector<uint64_t> off(inst);
      std::vector<uint32_t> len(inst), pitch(inst);
      for (size_t q = 0; q < inst; q++)
        off[q] = rows[3 * q], len[q] = (uint32_t)rows[3 * q + 1], pitch[q] = (uint32_t)rows[3 * q + 2];
      uint32_t max_len = 0, bad[2] = {0, 0};
      const int rc = hbx_bcplan::check_rows(h[1], off.data(), len.data(), pitch.data(), inst, n, &max_len, bad);
      if (rc) printf("rc %d %u %u\n", rc, bad[0], bad[1]);
      else printf("max %u\n", max_len);
    }
  }
  return 0;
}
#endif

