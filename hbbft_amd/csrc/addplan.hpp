// Launch planning of hbx_add_dec_shares_d (include/hbx.h): which tiles of the p x n share matrix a
// set of (proposer, sender) items touches, for each lanes-per-check shape of the share-check
// kernels, and how many lanes per check such a launch gets.  Host-only and free of HIP, so
// tools/hostcheck/addplancheck.cpp builds it with a plain C++ compiler (tests/test_addplan.py).
//
// A tile is one 64-thread block of a check kernel: sender chunk x of proposer j, where a chunk is
// 64 senders with one lane per check, 32 with two, 21 with three (G3_PER_WAVE) and 10 with six
// (G6_PER_WAVE).  A matrix verification launches every tile, (chunks, p); an add launches the
// touched ones only, in (j, x) order, and the kernels read their coordinates from the list.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace hbx_addplan {

constexpr int SHAPES = 4;
constexpr uint32_t SHAPE_LANES[SHAPES] = {1, 2, 3, 6};
constexpr uint32_t SHAPE_SENDERS[SHAPES] = {64, 32, 21, 10};  // senders per tile
constexpr size_t FILL_WAVES = 1024;                           // one wave per SIMD (MI355X: 256 CUs x 4)

enum { PLAN_OK = 0, PLAN_BAD_PROPOSER = 1, PLAN_DUPLICATE = 2, PLAN_OWN_SENDER = 3 };

struct tile {
  uint32_t x, j;  // sender chunk, proposer: the layout the kernels read as uint2
};

struct plan {
  std::vector<tile> tiles[SHAPES];  // per shape, sorted by (j, x), no repeats
  uint32_t live = 0;                // items with sender < n (the others touch no position)
};

inline int shape_of_lanes(int lanes) {  // 7 = the one-lane check as one kernel: the one-lane tiles
  return lanes == 2 ? 1 : lanes == 3 ? 2 : lanes == 6 ? 3 : 0;
}

// The ladder of a matrix verification (verify_impl), over the touched-tile counts: one lane per
// check when the launch fills the chip, else the most lanes per check that still leave at most one
// wave per SIMD.
inline int choose_lanes(size_t t1, size_t t6, size_t t3, size_t t2) {
  return t1 >= FILL_WAVES ? 1 : t6 <= FILL_WAVES ? 6 : t3 <= FILL_WAVES ? 3 : t2 <= FILL_WAVES ? 2 : 3;
}

// Groups the items by proposer and lists the touched tiles of every shape.  `me` is this node's
// index in own-share mode (its entry is never received), else UINT32_MAX.  On a rejection `out` is
// unspecified.
inline int build(const uint32_t* proposer, const uint32_t* sender, uint32_t count, uint32_t n, uint32_t p, uint32_t me,
                 plan& out) {
  std::vector<uint64_t> keys(count);
  for (uint32_t k = 0; k < count; k++) {
    if (proposer[k] >= p) return PLAN_BAD_PROPOSER;
    if (me != UINT32_MAX && sender[k] == me) return PLAN_OWN_SENDER;
    keys[k] = ((uint64_t)proposer[k] << 32) | sender[k];
  }
  std::sort(keys.begin(), keys.end());
  if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) return PLAN_DUPLICATE;
  out.live = 0;
  for (int s = 0; s < SHAPES; s++) out.tiles[s].clear();
  for (uint64_t key : keys) {
    const uint32_t j = (uint32_t)(key >> 32), i = (uint32_t)key;
    if (i >= n) continue;
    out.live++;
    for (int s = 0; s < SHAPES; s++) {
      const uint32_t x = i / SHAPE_SENDERS[s];
      std::vector<tile>& v = out.tiles[s];
      if (v.empty() || v.back().j != j || v.back().x != x) v.push_back(tile{x, j});  // sorted keys: repeats are adjacent
    }
  }
  return PLAN_OK;
}

inline int lanes_of(const plan& pl) {
  return choose_lanes(pl.tiles[0].size(), pl.tiles[3].size(), pl.tiles[2].size(), pl.tiles[1].size());
}

}  // namespace hbx_addplan
