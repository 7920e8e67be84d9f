// Host planning of the Broadcast calls that take host lists (include/hbx.h: the *_ragged_d forms,
// hbx_add_echoes_d, hbx_broadcast_decode_insts_d): the argument checks that come before any launch,
// the grouping of long values by length into hash blocks, and the work-buffer layout of a decode list.
// Host-only and free of HIP, so tools/hostcheck/bcplancheck.cpp builds it with a plain C++ compiler
// (tests/test_bcplan.py).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace hbx_bcplan {

constexpr uint32_t VAL_NONE = 0xFFFFFFFFu;  // unused lane of a hash block (broadcast.hpp)
constexpr uint32_t IN_LANE_MAX = 256;       // values up to this many bytes are hashed by the validating lane
constexpr uint32_t WORK_ALIGN = 16;         // work-buffer rows and instances start this aligned

enum {
  PLAN_OK = 0,
  PLAN_BAD_INST = 1,     // an instance at or beyond the store's count
  PLAN_BAD_SENDER = 2,   // sender >= n
  PLAN_DUPLICATE = 3,    // the same (inst, sender) / the same (inst, root, use row) twice
  PLAN_BAD_OFFSETS = 4,  // val_off decreasing, a value of 4 GiB or more, or ending past the blob
  PLAN_BAD_LEN = 5,      // len[a] == 0 or > max_shard_len
  PLAN_NO_ROOM = 6,      // no room for k len - 4 output bytes, or output ranges overlap
};

// An add's (inst, sender) items: bounds, then each pair once.
inline int check_items(const uint32_t* inst, const uint32_t* sender, uint32_t count, uint32_t n, uint32_t insts) {
  std::vector<uint64_t> keys(count);
  for (uint32_t k = 0; k < count; k++) {
    if (inst[k] >= insts) return PLAN_BAD_INST;
    if (sender[k] >= n) return PLAN_BAD_SENDER;
    keys[k] = ((uint64_t)inst[k] << 32) | sender[k];
  }
  std::sort(keys.begin(), keys.end());
  return std::adjacent_find(keys.begin(), keys.end()) != keys.end() ? PLAN_DUPLICATE : PLAN_OK;
}

// *bad (optional) = the first j whose val_off[j..j + 1] is no value; `count`: the list ends past the blob.
inline int check_offsets(const uint64_t* val_off, uint32_t count, uint64_t values_bytes, uint32_t* bad = nullptr) {
  uint32_t j = 0;
  while (j < count && val_off[j + 1] >= val_off[j] && val_off[j + 1] - val_off[j] <= 0xFFFFFFFFull) j++;
  if (bad) *bad = j;
  return j < count || val_off[count] > values_bytes ? PLAN_BAD_OFFSETS : PLAN_OK;
}

// The values longer than IN_LANE_MAX bytes (and, with max_value != 0, no longer than it: an
// oversize value is never hashed), sorted by (length, index) and cut into blocks of `lanes`
// values of one length: blk_len[b], blk_idx[b][lanes] (filled from lane 0, VAL_NONE after).
inline void group_long(const uint64_t* val_off, uint32_t count, uint32_t lanes, uint64_t max_value,
                       std::vector<uint32_t>& blk_len, std::vector<uint32_t>& blk_idx) {
  std::vector<uint64_t> lng;
  for (uint32_t j = 0; j < count; j++) {
    const uint64_t v = val_off[j + 1] - val_off[j];
    if (v > IN_LANE_MAX && (max_value == 0 || v <= max_value)) lng.push_back((v << 32) | j);
  }
  if (!std::is_sorted(lng.begin(), lng.end())) std::sort(lng.begin(), lng.end());
  blk_len.clear();
  blk_idx.clear();
  blk_idx.reserve(lng.size() + lanes);
  for (size_t i = 0; i < lng.size();) {
    size_t e = i;
    while (e < lng.size() && e - i < lanes && (lng[e] >> 32) == (lng[i] >> 32)) e++;
    blk_len.push_back((uint32_t)(lng[i] >> 32));
    for (size_t q = 0; q < lanes; q++) blk_idx.push_back(i + q < e ? (uint32_t)lng[i + q] : VAL_NONE);
    i = e;
  }
}

// A decode list's attempts: instance bounds, shard lengths, and each (instance, root, use row)
// once.  use == nullptr: every sender allowed.
inline int check_attempts(const uint32_t* insts, const uint8_t* roots, const uint32_t* len, const uint8_t* use,
                          uint32_t na, uint32_t n, uint32_t store_insts, uint32_t max_shard_len) {
  for (uint32_t a = 0; a < na; a++) {
    if (insts[a] >= store_insts) return PLAN_BAD_INST;
    if (len[a] == 0 || len[a] > max_shard_len) return PLAN_BAD_LEN;
  }
  std::vector<uint32_t> order(na);
  for (uint32_t a = 0; a < na; a++) order[a] = a;
  auto cmp = [&](uint32_t x, uint32_t y) {
    if (insts[x] != insts[y]) return insts[x] < insts[y] ? -1 : 1;
    if (int c = memcmp(roots + (size_t)x * 32, roots + (size_t)y * 32, 32)) return c;
    if (!use) return 0;
    for (uint32_t i = 0; i < n; i++) {  // a use byte allows its sender iff it is non-zero
      const int a = use[(size_t)x * n + i] != 0, b = use[(size_t)y * n + i] != 0;
      if (a != b) return a - b;
    }
    return 0;
  };
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return cmp(x, y) < 0; });
  for (uint32_t r = 1; r < na; r++)
    if (cmp(order[r - 1], order[r]) == 0) return PLAN_DUPLICATE;
  return PLAN_OK;
}

// The work buffer of a decode list: attempt a's n rows at off[a], pitch[a] = len[a] rounded up to
// WORK_ALIGN, attempts back to back.  Returns the buffer's size.
inline uint64_t work_layout(const uint32_t* len, uint32_t na, uint32_t n, std::vector<uint64_t>& off,
                            std::vector<uint32_t>& pitch) {
  off.resize(na);
  pitch.resize(na);
  uint64_t at = 0;
  for (uint32_t a = 0; a < na; a++) {
    pitch[a] = (uint32_t)(((uint64_t)len[a] + WORK_ALIGN - 1) / WORK_ALIGN * WORK_ALIGN);
    off[a] = at;
    at += (uint64_t)n * pitch[a];
  }
  return at;
}

// Output room as in the ragged decode: attempt a may write k len[a] - 4 bytes at out_off[a], apart
// from the others' ranges.  *bad (optional) = the first attempt without room; `na`: ranges overlap.
inline int check_out(const uint32_t* len, const uint64_t* out_off, uint32_t na, uint32_t k, uint64_t out_bytes,
                     uint32_t* bad = nullptr) {
  std::vector<std::pair<uint64_t, uint64_t>> rng;
  for (uint32_t a = 0; a < na; a++) {
    const uint64_t need = (uint64_t)k * len[a] >= 4 ? (uint64_t)k * len[a] - 4 : 0;
    if (bad) *bad = a;
    if (out_off[a] > out_bytes || need > out_bytes - out_off[a]) return PLAN_NO_ROOM;
    if (need) rng.emplace_back(out_off[a], out_off[a] + need);
  }
  if (bad) *bad = na;
  std::sort(rng.begin(), rng.end());
  for (size_t r = 1; r < rng.size(); r++)
    if (rng[r].first < rng[r - 1].second) return PLAN_NO_ROOM;
  return PLAN_OK;
}

enum { ROWS_OK = 0, ROWS_UNALIGNED = 1, ROWS_BAD_LEN = 2, ROWS_PAST_END = 3, ROWS_OVERLAP = 4 };

// The row descriptors of a ragged call (include/hbx.h; instance q's n rows of len[q] bytes start at
// off[q], pitch[q] apart), per instance in turn, then no two instances' rows overlap.  bad[0] (and
// bad[1] of an overlapping pair, in offset order) = the offending instance; *max_len = the longest shard.
inline int check_rows(uint64_t buf_bytes, const uint64_t* off, const uint32_t* len, const uint32_t* pitch, uint32_t inst,
                      uint32_t n, uint32_t* max_len, uint32_t bad[2]) {
  uint32_t mx = 0;
  for (uint32_t q = 0; q < inst; q++) {
    bad[0] = q;
    if (off[q] % 4 || pitch[q] % 4) return ROWS_UNALIGNED;
    if (len[q] == 0 || pitch[q] < len[q]) return ROWS_BAD_LEN;
    if (off[q] > buf_bytes || (uint64_t)n * pitch[q] > buf_bytes - off[q]) return ROWS_PAST_END;
    if (len[q] > mx) mx = len[q];
  }
  std::vector<uint32_t> order(inst);
  for (uint32_t q = 0; q < inst; q++) order[q] = q;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return off[a] < off[b]; });
  for (uint32_t r = 1; r < inst; r++) {
    bad[0] = order[r - 1], bad[1] = order[r];
    if (off[bad[1]] < off[bad[0]] + (uint64_t)n * pitch[bad[0]]) return ROWS_OVERLAP;
  }
  *max_len = mx;
  return ROWS_OK;
}

}  // namespace hbx_bcplan
