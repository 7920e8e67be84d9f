// Host build (g++, like hostcheck.cpp) of the batched share verification's arithmetic
// (hbbft_amd/csrc/batchd.hpp): the coefficient derivation, one lane's term r_i S_ji and the block's
// complete-addition reduction.  tests/test_batch_host.py compares them with the oracle.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../hbbft_amd/csrc/batchd.hpp"
using namespace hbx;
extern "C" {
// r4: four little-endian words of r_i
void bc_coeff(const uint8_t* seed32, uint64_t call_index, uint32_t i, uint32_t* r4) {
  batch_coeff(seed32, call_index, i, r4);
}
// out48 = compress(r * P) through the lane's routine; returns the decode status of p48
int bc_term(const uint8_t* p48, const uint32_t* r4, uint8_t* out48) {
  g1a P;
  const int32_t st = g1_decompress(p48, P);
  if (st != HBX_PT_OK) return st;
  g1_compress(g1_to_affine(batch_term(P, r4)), out48);
  return 0;
}
// out48 = compress(sum of `count` points) through the block reduction's shape; the identity
// encoding is an operand like any other.  Returns -1 if a point does not decode.
int bc_reduce(const uint8_t* pts48, uint32_t count, uint8_t* out48) {
  std::vector<g1j> terms(count);
  for (uint32_t i = 0; i < count; i++) {
    g1a P;
    const int32_t st = g1_decompress(pts48 + (size_t)i * 48, P);
    if (st != HBX_PT_OK && st != HBX_PT_INFINITY) return -1;
    terms[i] = st == HBX_PT_INFINITY ? g1_identity() : g1_from_affine(P);
  }
  g1_compress(g1_to_affine(batch_reduce_model(terms.data(), count)), out48);
  return 0;
}
// A_j of one column: out48 = compress(sum_{include[i]} r_i S_i), r_i from (seed32, call_index, i)
int bc_column(const uint8_t* shares48, const uint8_t* include, uint32_t n, const uint8_t* seed32, uint64_t call_index,
              uint8_t* out48) {
  std::vector<g1j> terms(n);
  for (uint32_t i = 0; i < n; i++) {
    terms[i] = g1_identity();
    if (!include[i]) continue;
    g1a P;
    if (g1_decompress(shares48 + (size_t)i * 48, P) != HBX_PT_OK) return -1;
    uint32_t r4[4];
    batch_coeff(seed32, call_index, i, r4);
    terms[i] = batch_term(P, r4);
  }
  g1_compress(g1_to_affine(batch_reduce_model(terms.data(), n)), out48);
  return 0;
}
}
