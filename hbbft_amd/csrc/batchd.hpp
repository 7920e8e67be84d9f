// Batched decryption-share verification by random linear combination (DESIGN.md "Batched share
// verification"): the pieces shared by the kernels (hbx_kernels.hip k_batch_*) and the CPU check
// (tools/hostcheck/batchcheck.cpp).  All n shares of proposer j's ciphertext verify against the
// same G2 points H_j and W_j, so one equation per column decides them,
//   e(sum_i r_i S_ji, H_j) e(-sum_i r_i pk_i, W_j) == 1,
// with secret 128-bit coefficients r_i.  Each lane multiplies its share by r_i (g1d.hpp's 4-bit
// window routine: a share that decoded is a point of G1) and the block sums the products with the
// COMPLETE addition g1_add: senders choose the shares, so equal, opposite and identity operands
// do meet in the sum.
#pragma once
#include "g1d.hpp"
#include "hash.hpp"

namespace hbx {

constexpr uint32_t BATCH_CT_INDEX = 0xFFFFFFFFu;  // the coefficient of the folded Ciphertext::verify
constexpr int BATCH_THREADS = 256;                // k_batch_msm: one block per column, four waves

// r_i = the little-endian integer of the first 16 bytes of SHA-256(seed32 || LE64(call) || LE32(i)),
// four little-endian words.  Always SHA-256, whatever DIGEST the context hashes points with.
HBX_HD void batch_coeff(const uint8_t* seed32, uint64_t call_index, uint32_t i, uint32_t* r4) {
  uint8_t m[12], d[32];
  for (int q = 0; q < 8; q++) m[q] = (uint8_t)(call_index >> (8 * q));
  for (int q = 0; q < 4; q++) m[8 + q] = (uint8_t)(i >> (8 * q));
  sha256_2(seed32, 32, m, 12, d);
  for (int k = 0; k < 4; k++)
    r4[k] = (uint32_t)d[4 * k] | ((uint32_t)d[4 * k + 1] << 8) | ((uint32_t)d[4 * k + 2] << 16) |
            ((uint32_t)d[4 * k + 3] << 24);
}

// One lane's term r_i S_ji: S in G1 (prime order), any 128-bit r including 0.
HBX_HD g1j batch_term(const g1a& S, const uint32_t* r4) { return g1d_mul_u128_w4(S, r4); }

// The block reduction's shape on one thread (the CPU check): lane l of BATCH_THREADS sums the terms
// l, l + 256, ..., each wave folds its 64 lanes by halves (offsets 32 .. 1), and the four wave sums
// are added in order -- k_batch_msm with the shuffles and the LDS exchange written as loops.
HBX_HD g1j batch_reduce_model(const g1j* terms, uint32_t count) {
  g1j total = g1_identity();
  for (int wv = 0; wv < BATCH_THREADS / 64; wv++) {
    g1j lane[64];
    for (int l = 0; l < 64; l++) {
      lane[l] = g1_identity();
      for (uint32_t i = (uint32_t)(wv * 64 + l); i < count; i += BATCH_THREADS) lane[l] = g1_add(lane[l], terms[i]);
    }
    for (int off = 32; off > 0; off >>= 1)
      for (int l = 0; l < off; l++) lane[l] = g1_add(lane[l], lane[l + off]);
    total = g1_add(total, lane[0]);
  }
  return total;
}

}  // namespace hbx
