// Developer tool: the digit tower's products (hbbft_amd/csrc/fieldd.hpp, pairingd.hpp, fe1d.hpp)
// compiled for the host with -DHBX_DCHECK and compared with field.hpp's 12-limb tower on operands
// given as RAW DIGITS, so a test can drive every digit to the operand bounds
// (tests/test_tower_forms.py).  NOT part of the product.
//
// Every function returns the digit tower's result (`got`) and field.hpp's (`want`) as canonical
// big-endian 48-byte values, c0 first.  A raw-digit operand reaches field.hpp through fqd_to_fq
// (one fqd_mul by a constant: any digits below 2^31).
#include <cstring>
#include "../../hbbft_amd/csrc/pairing.hpp"
#include "../../hbbft_amd/csrc/pairingd.hpp"
#include "../../hbbft_amd/csrc/fe1d.hpp"
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
static void put2(const fq2& a, uint8_t* out) {
  put(a.c0, out);
  put(a.c1, out + 48);
}
static void put12(const fq12& a, uint8_t* out) {
  const fq2* c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
  for (int q = 0; q < 6; q++) put2(*c[q], out + 96 * q);
}

extern "C" {
// a, b: 2 x 14 digits each (|digit| <= 2^29)
void tw_fq2d_mul(const int32_t* a, const int32_t* b, uint8_t* got, uint8_t* want) {
  const fq2d x = digits2(a), y = digits2(b);
  put2(fq2d_to_fq2(fq2d_mul(x, y)), got);
  put2(fq2_mul(fq2d_to_fq2(x), fq2d_to_fq2(y)), want);
}
// ab: (a, b) as 4 x 14 digits (|digit| <= 2^28); c0 = a^2 + xi b^2, c1 = 2 a b: 4 x 48 bytes
void tw_fq4d_sqr_lazy(const int32_t* ab, uint8_t* got, uint8_t* want) {
  const fq2d a = digits2(ab), b = digits2(ab + 28);
  fq2d c0, c1;
  fq4d_sqr_lazy(a, b, c0, c1);
  put2(fq2d_to_fq2(c0), got);
  put2(fq2d_to_fq2(c1), got + 96);
  const fq2 x = fq2d_to_fq2(a), y = fq2d_to_fq2(b);
  put2(fq2_add(fq2_sqr(x), fq2_mul_xi(fq2_sqr(y))), want);
  put2(fq2_dbl(fq2_mul(x, y)), want + 96);
}
// A chain of n dependent Fq12 operations on f (12 x 14 digits, digits 0..12 within [-2^28, 2^28]) with
// no canonicalisation in between; operation k is ops[k % nops]:
//   0 fq12d_sqr   1 fq12d_sqr_parked   2 fq12d_mul_by_01v(f, c0, c1)   3 fq12d_mul(f, g)
//   4 fq12d_mul_slot(f, g)   5 fq12d_mul_by_014(f, c0, c1, c4)   6 fq12d_conj
// line: c0, c1 (2 x 14 digits each) and c4 (14 digits), normalised; g: 12 x 14 digits, normalised.
// field.hpp runs the same chain on the same starting values.  576 bytes each.
void tw_fq12_chain(const int32_t* f_, const int32_t* line, const int32_t* g_, const int* ops, int nops, int n,
                   uint8_t* got, uint8_t* want) {
  fq12d f = digits12(f_);
  const fq12d g = digits12(g_);
  const fq2d c0 = digits2(line), c1 = digits2(line + 28);
  const fqd c4 = digits(line + 56);
  fq12 F = fq12d_to_fq12(f);
  const fq12 G = fq12d_to_fq12(g);
  const fq2 C0 = fq2d_to_fq2(c0), C1 = fq2d_to_fq2(c1);
  const fq C4 = fqd_to_fq(c4);
  static uint32_t park[LDS_FQ12D_DWORDS], slot[FE1_WORDS];
  s1_put_fq12d<1>(slot, g);
  for (int k = 0; k < n; k++) {
    switch (ops[k % nops]) {
      case 0: f = fq12d_sqr(f); F = fq12_sqr(F); break;
      case 1: f = fq12d_sqr_parked(f, park); F = fq12_sqr(F); break;
      case 2: f = fq12d_mul_by_01v(f, c0, c1); F = fq12_mul_by_014(F, C0, C1, fq_one()); break;
      case 3: f = fq12d_mul(f, g); F = fq12_mul(F, G); break;
      case 4: f = fq12d_mul_slot<1>(f, slot); F = fq12_mul(F, G); break;
      case 5: f = fq12d_mul_by_014(f, c0, c1, c4); F = fq12_mul_by_014(F, C0, C1, C4); break;
      default: f = fq12d_conj(f); F = fq12_conj(F); break;
    }
  }
  put12(fq12d_to_fq12(f), got);
  put12(F, want);
}
}
