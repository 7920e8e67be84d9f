// SyncKeyGen (reference src/sync_key_gen.rs) per-lane arithmetic: Fr polynomials of the dealer's
// BivarPoly, Lagrange interpolation at 0 in Fr (generate(), :396-409), the public key shares of a
// commitment (messaging.rs:251-254) and the non-threshold SecretKey::decrypt keystream (:326, :444).
// __host__ __device__ throughout: the kernels of hbx_kernels.hip are thin wrappers, and
// tools/hostcheck builds the same functions for the CPU (tests/test_hostcheck_keygen.py).
//
// Scalars cross the ABI as canonical 32-byte big-endian Fr.  Inside, a value is either PLAIN
// (8 little-endian limbs, < r) or MONTGOMERY (times 2^256); fr_mul(plain, mont) is the plain
// product, so a Horner chain keeps its accumulator and coefficients plain and only the evaluation
// point in Montgomery form: one fr_mul per step, no conversion of the coefficients.
#pragma once
#include "curve.hpp"
#include "hash.hpp"

namespace hbx {

// 32-byte big-endian -> 8 LE limbs; false if the value is >= r (not a canonical Fr).
HBX_HD bool kg_fr_load_be(const uint8_t* b, fr& out) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint8_t* q = b + 28 - 4 * i;
    out.l[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
  }
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) (void)subb32(out.l[i], FR_R[i], borrow);
  return borrow != 0;
}
HBX_HD void kg_fr_store_be(const fr& a, uint8_t* b) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint8_t* q = b + 28 - 4 * i;
    q[0] = (uint8_t)(a.l[i] >> 24);
    q[1] = (uint8_t)(a.l[i] >> 16);
    q[2] = (uint8_t)(a.l[i] >> 8);
    q[3] = (uint8_t)a.l[i];
  }
}
HBX_HD fr kg_fr_zero() {
  fr z;
#pragma unroll
  for (int i = 0; i < 8; i++) z.l[i] = 0;
  return z;
}
// u64 -> Montgomery form (any u64 is < r)
HBX_HD fr kg_fr_mont_u64(uint64_t x) {
  fr a = kg_fr_zero();
  a.l[0] = (uint32_t)x;
  a.l[1] = (uint32_t)(x >> 32);
  return fr_to_mont(a);
}

// threshold_crypto's storage of a symmetric bivariate polynomial: a_ij = a_ji once, at
// coeff_pos(i, j) = j (j + 1) / 2 + i for i <= j.
HBX_HD uint32_t kg_coeff_pos(uint32_t i, uint32_t j) { return i <= j ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j; }

// Poly::evaluate(x) (sync_key_gen.rs:341 `row.evaluate(idx + 1)`): sum_j c_j x^j by Horner over
// deg + 1 canonical big-endian coefficients; plain result.
HBX_HD fr kg_poly_eval(const uint8_t* coeff32, uint32_t deg, uint64_t x) {
  const fr xm = kg_fr_mont_u64(x);
  fr acc = kg_fr_zero();
  for (int j = (int)deg; j >= 0; j--) {
    fr c;
    (void)kg_fr_load_be(coeff32 + (size_t)j * 32, c);
    acc = fr_add(fr_mul(acc, xm), c);
  }
  return acc;
}

// BivarPoly::row(x) (sync_key_gen.rs:293), coefficient j: sum_i a_ij x^i by Horner in x over the
// coeff_pos storage ((t + 1)(t + 2)/2 canonical big-endian scalars); plain result.
HBX_HD fr kg_bivar_row_coeff(const uint8_t* coeff32, uint32_t t, uint64_t x, uint32_t j) {
  const fr xm = kg_fr_mont_u64(x);
  fr acc = kg_fr_zero();
  for (int i = (int)t; i >= 0; i--) {
    fr c;
    (void)kg_fr_load_be(coeff32 + (size_t)kg_coeff_pos((uint32_t)i, j) * 32, c);
    acc = fr_add(fr_mul(acc, xm), c);
  }
  return acc;
}

// Poly::interpolate(points).evaluate(0) (sync_key_gen.rs:404-407): sum_k lambda_k(0) v_k with
// lambda_k(0) = prod_{m != k} y_m / (y_m - y_k) over cnt points (y_k, v_k), y as u64 and v as
// canonical big-endian Fr.  The terms are summed as one fraction N / D, so a lane inverts once.
// cnt = 0 gives 0.  dup is set (and 0 returned) when two y are equal: the reference's BTreeMap cannot
// hold such points.
HBX_HD fr kg_lagrange0_sum(const uint64_t* y, const uint8_t* vals32, uint32_t cnt, bool& dup) {
  dup = false;
  for (uint32_t k = 0; k < cnt; k++)
    for (uint32_t m = k + 1; m < cnt; m++)
      if (y[m] == y[k]) dup = true;
  if (dup || cnt == 0) return kg_fr_zero();
  fr N = kg_fr_zero();               // plain
  fr D = fr_from_const(FR_ONE);      // Montgomery
  for (uint32_t k = 0; k < cnt; k++) {
    const fr yk = kg_fr_mont_u64(y[k]);
    fr num = fr_from_const(FR_ONE), den = fr_from_const(FR_ONE);  // Montgomery
    for (uint32_t m = 0; m < cnt; m++) {
      if (m == k) continue;
      const fr ym = kg_fr_mont_u64(y[m]);
      num = fr_mul(num, ym);
      den = fr_mul(den, fr_sub(ym, yk));
    }
    fr v;
    (void)kg_fr_load_be(vals32 + (size_t)k * 32, v);
    // N / D + v num / den = (N den + v num D) / (D den)
    N = fr_add(fr_mul(N, den), fr_mul(fr_mul(v, num), D));
    D = fr_mul(D, den);
  }
  return fr_mul(N, fr_inv(D));
}

// PublicKeySet::public_key_share(i) = commit.evaluate(i + 1) (messaging.rs:251-254):
// sum_j P_j x^j by Horner in G1 over the t + 1 decoded commitment points.
HBX_HD g1j kg_commit_eval(const g1a* P, uint32_t t, uint64_t x) {
  g1j acc = g1_identity();
  for (int j = (int)t; j >= 0; j--) acc = g1_add_mixed_i(g1j_mul_u64(acc, x), P[j]);
  return acc;
}

// SecretKey::decrypt after Ciphertext::verify (sync_key_gen.rs:326, :444): out = V xor
// hash_bytes(sk U, |V|), the keystream of PublicKey::encrypt (k_encrypt).  sk8: plain limbs.
HBX_HD void kg_sk_decrypt(const g1a& U, const uint32_t* sk8, const uint8_t* v, uint64_t len, uint8_t* out, int digest) {
  const g1a g = g1_to_affine(g1_mul_scalar(g1_from_affine(U), sk8));
  uint8_t gc[48], d[32];
  g1_compress(g, gc);
  digest2(digest, gc, 48, nullptr, 0, d);
  chacha_rng rng;
  chacha_rng_from_digest(rng, d);
  for (uint64_t q = 0; q < len; q++) out[q] = v[q] ^ (uint8_t)chacha_next_u32(rng);
}

}  // namespace hbx
