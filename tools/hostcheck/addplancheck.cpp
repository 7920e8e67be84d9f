// The add's launch planner (hbbft_amd/csrc/addplan.hpp) for the CPU: a C interface for
// tests/test_addplan.py (a shared object driven through ctypes), and, with -DADDPLAN_MAIN, a
// stand-alone program that plans the item sets it reads from standard input, which the test builds
// with -fsanitize=address,undefined.
//
//   g++ -O1 -std=c++17 -shared -fPIC -o libaddplancheck.so tools/hostcheck/addplancheck.cpp
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DADDPLAN_MAIN -o addplancheck tools/hostcheck/addplancheck.cpp
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../hbbft_amd/csrc/addplan.hpp"

extern "C" {

// Tiles of shape `shape` (0..3: 1, 2, 3, 6 lanes per check) that the items touch, as (x, j) pairs
// into out_tiles[2 * cap].  Returns the tile count (which may exceed cap: then only cap are
// written), or -PLAN_* on a rejection.  live: the items with sender < n.
int ap_plan(const uint32_t* proposer, const uint32_t* sender, uint32_t count, uint32_t n, uint32_t p, uint32_t me,
            int shape, uint32_t* out_tiles, uint32_t cap, uint32_t* live) {
  hbx_addplan::plan pl;
  const int rc = hbx_addplan::build(proposer, sender, count, n, p, me, pl);
  if (rc != hbx_addplan::PLAN_OK) return -rc;
  if (shape < 0 || shape >= hbx_addplan::SHAPES) return -100;
  const std::vector<hbx_addplan::tile>& v = pl.tiles[shape];
  for (size_t k = 0; k < v.size() && k < cap; k++) {
    out_tiles[2 * k] = v[k].x;
    out_tiles[2 * k + 1] = v[k].j;
  }
  if (live) *live = pl.live;
  return (int)v.size();
}

// Lanes per check of the items' launch (the ladder over the touched-tile counts), or -PLAN_*.
int ap_lanes_of(const uint32_t* proposer, const uint32_t* sender, uint32_t count, uint32_t n, uint32_t p, uint32_t me) {
  hbx_addplan::plan pl;
  const int rc = hbx_addplan::build(proposer, sender, count, n, p, me, pl);
  return rc != hbx_addplan::PLAN_OK ? -rc : hbx_addplan::lanes_of(pl);
}

int ap_choose_lanes(uint64_t t1, uint64_t t6, uint64_t t3, uint64_t t2) {
  return hbx_addplan::choose_lanes((size_t)t1, (size_t)t6, (size_t)t3, (size_t)t2);
}

int ap_shape_of_lanes(int lanes) { return hbx_addplan::shape_of_lanes(lanes); }
uint32_t ap_shape_senders(int shape) { return hbx_addplan::SHAPE_SENDERS[shape]; }
}

#ifdef ADDPLAN_MAIN
// Input, one item set per line:  n p me count  j0 i0 j1 i1 ...   (me = 4294967295: not own-share mode)
// Output per set: "rc R" on a rejection, else "lanes L live V" and, per shape, "shape S T x j x j ...".
int main() {
  unsigned long long n, p, me, count;
  while (scanf("%llu %llu %llu %llu", &n, &p, &me, &count) == 4) {
    std::vector<uint32_t> prop(count), snd(count);
    for (size_t k = 0; k < count; k++) {
      unsigned long long j, i;
      if (scanf("%llu %llu", &j, &i) != 2) return 2;
      prop[k] = (uint32_t)j;
      snd[k] = (uint32_t)i;
    }
    hbx_addplan::plan pl;
    const int rc = hbx_addplan::build(prop.data(), snd.data(), (uint32_t)count, (uint32_t)n, (uint32_t)p, (uint32_t)me, pl);
    if (rc != hbx_addplan::PLAN_OK) {
      printf("rc %d\n", rc);
      continue;
    }
    printf("lanes %d live %u\n", hbx_addplan::lanes_of(pl), pl.live);
    for (int s = 0; s < hbx_addplan::SHAPES; s++) {
      printf("shape %d %zu", s, pl.tiles[s].size());
      for (const hbx_addplan::tile& t : pl.tiles[s]) printf(" %u %u", t.x, t.j);
      printf("\n");
    }
  }
  return 0;
}
#endif
