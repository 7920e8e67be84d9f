// The echo store's host planner (hbbft_amd/csrc/bcplan.hpp) for the CPU: a C interface for
// tests/test_bcplan.py (a shared object driven through ctypes), and, with -DBCPLAN_MAIN, a
// stand-alone program that plans the sets it reads from standard input, which the test builds with
// -fsanitize=address,undefined.
//
//   g++ -O1 -std=c++17 -shared -fPIC -o libbcplancheck.so tools/hostcheck/bcplancheck.cpp
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DBCPLAN_MAIN -o bcplancheck tools/hostcheck/bcplancheck.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../hbbft_amd/csrc/bcplan.hpp"

extern "C" {

int bp_check_items(const uint32_t* inst, const uint32_t* sender, uint32_t count, uint32_t n, uint32_t insts) {
  return hbx_bcplan::check_items(inst, sender, count, n, insts);
}

int bp_check_offsets(const uint64_t* val_off, uint32_t count, uint64_t values_bytes) {
  return hbx_bcplan::check_offsets(val_off, count, values_bytes);
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
}

#ifdef BCPLAN_MAIN
// Input, one set per line:
//   add n insts max_value lanes values_bytes count  inst0 sender0 ..  off0 .. off_count
//   dec n insts max_shard_len k out_bytes na  inst0 rootbyte0 len0 usebits0 out_off0 ..
// (a root is its byte repeated 32 times; usebits: bit i = sender i allowed, n <= 32).
// Output: "rc R" on a rejection; else for add "blocks B" and per block "len L idx ..", for dec
// "total T" and per attempt "off O pitch P".
int main() {
  char kind[8];
  while (scanf("%7s", kind) == 1) {
    if (kind[0] == 'a') {
      unsigned long long n, insts, max_value, lanes, vb, count;
      if (scanf("%llu %llu %llu %llu %llu %llu", &n, &insts, &max_value, &lanes, &vb, &count) != 6) return 2;
      std::vector<uint32_t> in(count), sn(count);
      std::vector<uint64_t> off(count + 1);
      for (size_t j = 0; j < count; j++) {
        unsigned long long a, b;
        if (scanf("%llu %llu", &a, &b) != 2) return 2;
        in[j] = (uint32_t)a, sn[j] = (uint32_t)b;
      }
      for (size_t j = 0; j <= count; j++) {
        unsigned long long a;
        if (scanf("%llu", &a) != 1) return 2;
        off[j] = a;
      }
      int rc = hbx_bcplan::check_items(in.data(), sn.data(), (uint32_t)count, (uint32_t)n, (uint32_t)insts);
      if (!rc) rc = hbx_bcplan::check_offsets(off.data(), (uint32_t)count, vb);
      if (rc) {
        printf("rc %d\n", rc);
        continue;
      }
      std::vector<uint32_t> bl, bi;
      hbx_bcplan::group_long(off.data(), (uint32_t)count, (uint32_t)lanes, max_value, bl, bi);
      printf("blocks %zu\n", bl.size());
      for (size_t b = 0; b < bl.size(); b++) {
        printf("len %u idx", bl[b]);
        for (size_t q = 0; q < lanes; q++) printf(" %u", bi[b * lanes + q]);
        printf("\n");
      }
    } else {
      unsigned long long n, insts, max_len, k, ob, na;
      if (scanf("%llu %llu %llu %llu %llu %llu", &n, &insts, &max_len, &k, &ob, &na) != 6) return 2;
      std::vector<uint32_t> in(na), len(na);
      std::vector<uint8_t> roots(na * 32), use(na * n);
      std::vector<uint64_t> out_off(na);
      for (size_t a = 0; a < na; a++) {
        unsigned long long q, r, l, u, o;
        if (scanf("%llu %llu %llu %llu %llu", &q, &r, &l, &u, &o) != 5) return 2;
        in[a] = (uint32_t)q, len[a] = (uint32_t)l, out_off[a] = o;
        for (int b = 0; b < 32; b++) roots[a * 32 + b] = (uint8_t)r;
        for (size_t i = 0; i < n; i++) use[a * n + i] = (uint8_t)((u >> i) & 1);
      }
      int rc = hbx_bcplan::check_attempts(in.data(), roots.data(), len.data(), use.data(), (uint32_t)na, (uint32_t)n,
                                          (uint32_t)insts, (uint32_t)max_len);
      if (!rc) rc = hbx_bcplan::check_out(len.data(), out_off.data(), (uint32_t)na, (uint32_t)k, ob);
      if (rc) {
        printf("rc %d\n", rc);
        continue;
      }
      std::vector<uint64_t> off;
      std::vector<uint32_t> pitch;
      printf("total %llu\n", (unsigned long long)hbx_bcplan::work_layout(len.data(), (uint32_t)na, (uint32_t)n, off, pitch));
      for (size_t a = 0; a < na; a++) printf("off %llu pitch %u\n", (unsigned long long)off[a], pitch[a]);
    }
  }
  return 0;
}
#endif
