// Developer tool: the one-lane Miller kernel's line form "divided by the constant term" -- the
// second normalised table (pairing.hpp g2_normalise_line_z2), the product fq12d_mul_by_1ab
// (fieldd.hpp) and the loop miller_loop2_unit_d (pairingd.hpp) -- compiled for the host with
// -DHBX_DCHECK and compared with field.hpp's generic tower and with the loop over lines divided by
// y_P (tests/test_line_unit_form.py).  NOT part of the product.
#include <cstring>
#include "../../hbbft_amd/csrc/pairing.hpp"
#include "../../hbbft_amd/csrc/pairingd.hpp"
using namespace hbx;

static fqd digits(const int32_t* d) {
  fqd r;
  for (int i = 0; i < 14; i++) r.d[i] = d[i];
  return r;
}
static fq2d digits2(const int32_t* d) { return fq2d{digits(d), digits(d + 14)}; }
static fq12d digits12(const int32_t* d) {
  return fq12d{fq6d{digits2(d), digits2(d + 28), digits2(d + 56)}, fq6d{digits2(d + 84), digits2(d + 112), digits2(d + 140)}};
}
static void put(const fq& a, uint8_t* out) { fq_to_be(fq_from_mont(fq_canon(a)), out); }
static void put12(const fq12& a, uint8_t* out) {
  const fq* c = &a.c0.c0.c0;
  for (int q = 0; q < 12; q++) put(c[q], out + 48 * q);
}
static fq2 fq2_be(const uint8_t* b) { return fq2{fq_to_mont(fq_from_be(b)), fq_to_mont(fq_from_be(b + 48))}; }
static bool fq12_same(const fq12& a, const fq12& b) {
  const fq *x = &a.c0.c0.c0, *y = &b.c0.c0.c0;
  bool same = true;
  for (int i = 0; i < 12; i++) same &= fq_eq(x[i], y[i]);
  return same;
}

extern "C" {
// n dependent products f <- f (1 + beta v + alpha v w) on raw digits (f: 12 x 14, digits 0..12
// within [-2^28, 2^28]; alpha, beta: 2 x 14 each, normalised), no canonicalisation in between,
// against field.hpp's generic fq12_mul by the same element.  576 canonical bytes each.
void lc_mul_by_1ab(const int32_t* f_, const int32_t* alpha_, const int32_t* beta_, int n, uint8_t* got, uint8_t* want) {
  fq12d f = digits12(f_);
  const fq2d alpha = digits2(alpha_), beta = digits2(beta_);
  fq12 F = fq12d_to_fq12(f);
  fq12 L;
  L.c0 = fq6{fq2_one(), fq2d_to_fq2(beta), fq2_zero()};
  L.c1 = fq6{fq2_zero(), fq2d_to_fq2(alpha), fq2_zero()};
  for (int k = 0; k < n; k++) {
    f = fq12d_mul_by_1ab(f, alpha, beta);
    F = fq12_mul(F, L);
  }
  put12(fq12d_to_fq12(f), got);
  put12(F, want);
}

// Both normalised tables of QA and QB off g2_normalise_line_z2 (QA's raw lines made from the
// Jacobian representative (x z^2, y z^3, z) when jac is set, as k_prepare_lines makes H''s), then
// the loop over the second table (miller_loop2_unit_d) against the loop over the first
// (miller_loop2_parked_d, k_verify_shares' loop) at (PA, PB).  Returns a bit set, or a negative decode error:
//   1  both loops give the same element after the final exponentiation
//   2  that element is 1 (the check holds)
//   4  the first table equals g2_normalise_line's of the affine points
//   8  every (a, b) of the second table times the raw c0 gives the raw line's (c2, c1) (Z-corrected)
//  16  no line was reported degenerate
int lc_unit_loop_cmp(const uint8_t* pa, const uint8_t* qa, const uint8_t* pb, const uint8_t* qb, int jac,
                     const uint8_t* z96) {
  g1a PA, PB; g2a QA, QB;
  if (g1_decompress(pa, PA) != HBX_PT_OK) return -1;
  if (g1_decompress(pb, PB) != HBX_PT_OK) return -2;
  if (g2_decompress(qa, QA) != HBX_PT_OK) return -3;
  if (g2_decompress(qb, QB) != HBX_PT_OK) return -4;
  static line_pre ref[2][MILLER_LINES], raw[2][MILLER_LINES], old[2][MILLER_LINES], unit[2][MILLER_LINES];
  static fq2 cref[MILLER_LINES], c2[2][MILLER_LINES];
  static line_pre_d D[2][MILLER_LINES], U[2][MILLER_LINES];
  int res = 4 | 8 | 16;
  for (int s = 0; s < 2; s++) {
    const g2a Q = s ? QB : QA;
    g2_raw_lines(Q, ref[s], cref);
    fq2 z = fq2_one();
    g2a Qz = Q;
    if (jac && s == 0) {
      z = fq2_be(z96);
      const fq2 zz = fq2_sqr(z);
      Qz.x = fq2_mul(Q.x, zz);
      Qz.y = fq2_mul(Q.y, fq2_mul(zz, z));
    }
    g2_raw_lines(Qz, raw[s], c2[s]);
    const fq2 z2 = fq2_sqr(z), z3 = fq2_mul(z2, z);
    for (int i = 0; i < MILLER_LINES; i++) {
      g2_normalise_line(ref[s][i], cref[i]);
      old[s][i] = raw[s][i];
      if (g2_normalise_line_z2(old[s][i], c2[s][i], z, unit[s][i])) res &= ~16;
      if (!fq2_eq(old[s][i].c0, ref[s][i].c0) || !fq2_eq(old[s][i].c1, ref[s][i].c1)) res &= ~4;
      if (!fq2_eq(fq2_mul(unit[s][i].c0, raw[s][i].c0), fq2_mul(c2[s][i], z3)) ||
          !fq2_eq(fq2_mul(unit[s][i].c1, raw[s][i].c0), fq2_mul(raw[s][i].c1, z2)))
        res &= ~8;
      D[s][i] = line_to_d(old[s][i]);
      U[s][i] = line_to_d(unit[s][i]);
    }
  }
  static uint32_t park[LDS_FQ12D_DWORDS];
  park_put_fqd(park, 0, fqd_from_fq(PA.x));
  park_put_fqd(park, 1, fqd_from_fq(PA.y));
  park_put_fqd(park, 2, fqd_from_fq(PB.x));
  park_put_fqd(park, 3, fqd_neg(fqd_from_fq(fq_neg(PB.y))));  // a negated digit vector, as the kernel parks -y_pk
  const fq12 e_old = final_exponentiation(fq12d_to_fq12(miller_loop2_parked_d(D[0], true, D[1], true, park)));
  const fq12 e_new = final_exponentiation(fq12d_to_fq12(miller_loop2_unit_d(U[0], true, U[1], true, park)));
  if (fq12_same(e_old, e_new)) res |= 1;
  if (fq12_is_one(e_new)) res |= 2;
  return res;
}

// A raw line (c0, c1), c2 and z as canonical bytes (Fq2: c0 then c1, 48 bytes each) through
// g2_normalise_line_z2.  Returns 1 if the line was reported degenerate, + 2 if the first-form line
// equals g2_normalise_line_z's of the same input, + 4 if the second-form line is (0, 0).
int lc_normalise_flags(const uint8_t* c0_96, const uint8_t* c1_96, const uint8_t* c2_96, const uint8_t* z96) {
  const fq2 c2 = fq2_be(c2_96), z = fq2_be(z96);
  line_pre a{fq2_be(c0_96), fq2_be(c1_96)}, b = a, u;
  const bool degenerate = g2_normalise_line_z2(a, c2, z, u);
  g2_normalise_line_z(b, c2, z);
  int res = degenerate ? 1 : 0;
  if (fq2_eq(a.c0, b.c0) && fq2_eq(a.c1, b.c1)) res |= 2;
  if (fq2_is_zero(u.c0) && fq2_is_zero(u.c1)) res |= 4;
  return res;
}
}
