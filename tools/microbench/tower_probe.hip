// Instruction-mix probe of the digit tower (fieldd.hpp): one kernel per tower function, each called
// once on per-lane operands read from global memory, result written back.  Compiled device-only for
// gfx950 and read by tools/tower_mix.py, which counts each kernel's instructions by class (64-bit
// multiply-adds, accumulator-register moves, scratch accesses, wait states, other VALU): the share
// check is issue-bound, so a tower function's cost is its instruction count.  Not meant to be run.
//   python tools/tower_mix.py            (compiles this file with each share-check unit's flags)
#include <hip/hip_runtime.h>
#include "../../hbbft_amd/csrc/pairing.hpp"
#include "../../hbbft_amd/csrc/pairingd.hpp"
#include "../../hbbft_amd/csrc/fe1d.hpp"

using namespace hbx;

// operand word w of this lane: [word][64 lanes]
__device__ __forceinline__ fqd ld_fqd(const int32_t* in, int w) {
  fqd r;
#pragma unroll
  for (int i = 0; i < 14; i++) r.d[i] = in[(size_t)(14 * w + i) * 64 + threadIdx.x];
  return r;
}
__device__ __forceinline__ void st_fqd(int32_t* out, int w, const fqd& a) {
#pragma unroll
  for (int i = 0; i < 14; i++) out[(size_t)(14 * w + i) * 64 + threadIdx.x] = a.d[i];
}
__device__ __forceinline__ fq2d ld_fq2d(const int32_t* in, int w) { return fq2d{ld_fqd(in, w), ld_fqd(in, w + 1)}; }
__device__ __forceinline__ fq6d ld_fq6d(const int32_t* in, int w) {
  return fq6d{ld_fq2d(in, w), ld_fq2d(in, w + 2), ld_fq2d(in, w + 4)};
}
__device__ __forceinline__ fq12d ld_fq12d(const int32_t* in, int w) { return fq12d{ld_fq6d(in, w), ld_fq6d(in, w + 6)}; }
__device__ __forceinline__ void st_fq2d(int32_t* out, int w, const fq2d& a) {
  st_fqd(out, w, a.c0);
  st_fqd(out, w + 1, a.c1);
}
__device__ __forceinline__ void st_fq6d(int32_t* out, int w, const fq6d& a) {
  st_fq2d(out, w, a.c0);
  st_fq2d(out, w + 2, a.c1);
  st_fq2d(out, w + 4, a.c2);
}
__device__ __forceinline__ void st_fq12d(int32_t* out, int w, const fq12d& a) {
  st_fq6d(out, w, a.c0);
  st_fq6d(out, w + 6, a.c1);
}

// -DPROBE_SELECT -DPROBE_SEL_<function>=1 ...: only those kernels (tools/tower_mix.py --only)
#if defined(PROBE_SELECT)
#define PROBE_ON(fn) PROBE_SEL_##fn
#else
#define PROBE_ON(fn) 1
#endif
#define PROBE_KERNEL(name) __global__ void __launch_bounds__(64) name(const int32_t* __restrict__ in, int32_t* __restrict__ out)

#if PROBE_ON(fqd_norm)
PROBE_KERNEL(p_fqd_norm) { st_fqd(out, 0, fqd_norm(ld_fqd(in, 0))); }
#endif
#if PROBE_ON(fqd_reduce)
PROBE_KERNEL(p_fqd_reduce) { st_fqd(out, 0, fqd_reduce(ld_fqd(in, 0))); }
#endif
#if PROBE_ON(fqd_relax)
PROBE_KERNEL(p_fqd_relax) { st_fqd(out, 0, fqd_relax(ld_fqd(in, 0))); }
#endif
#if PROBE_ON(fq2d_mul)
PROBE_KERNEL(p_fq2d_mul) { st_fq2d(out, 0, fq2d_mul(ld_fq2d(in, 0), ld_fq2d(in, 2))); }
#endif
#if PROBE_ON(fq2d_sqr)
PROBE_KERNEL(p_fq2d_sqr) { st_fq2d(out, 0, fq2d_sqr(ld_fq2d(in, 0))); }
#endif
#if PROBE_ON(fq2d_mul_fq)
PROBE_KERNEL(p_fq2d_mul_fq) { st_fq2d(out, 0, fq2d_mul_fq(ld_fq2d(in, 0), ld_fqd(in, 2))); }
#endif
#if PROBE_ON(fq4d_sqr_lazy)
PROBE_KERNEL(p_fq4d_sqr_lazy) {
  fq2d c0, c1;
  fq4d_sqr_lazy(ld_fq2d(in, 0), ld_fq2d(in, 2), c0, c1);
  st_fq2d(out, 0, c0);
  st_fq2d(out, 2, c1);
}
#endif
#if PROBE_ON(fq6d_mul)
PROBE_KERNEL(p_fq6d_mul) { st_fq6d(out, 0, fq6d_mul(ld_fq6d(in, 0), ld_fq6d(in, 6))); }
#endif
#if PROBE_ON(fq6d_mul_by_01)
PROBE_KERNEL(p_fq6d_mul_by_01) { st_fq6d(out, 0, fq6d_mul_by_01(ld_fq6d(in, 0), ld_fq2d(in, 6), ld_fq2d(in, 8))); }
#endif
#if PROBE_ON(fq12d_mul)
PROBE_KERNEL(p_fq12d_mul) { st_fq12d(out, 0, fq12d_mul(ld_fq12d(in, 0), ld_fq12d(in, 12))); }
#endif
#if PROBE_ON(fq12d_sqr)
PROBE_KERNEL(p_fq12d_sqr) { st_fq12d(out, 0, fq12d_sqr(ld_fq12d(in, 0))); }
#endif
#if PROBE_ON(fq12d_mul_by_01v)
PROBE_KERNEL(p_fq12d_mul_by_01v) { st_fq12d(out, 0, fq12d_mul_by_01v(ld_fq12d(in, 0), ld_fq2d(in, 12), ld_fq2d(in, 14))); }
#endif
#if PROBE_ON(fq12d_mul_by_1ab)
// the product by a line divided by its constant term (the one-lane Miller kernel's, pairingd.hpp)
PROBE_KERNEL(p_fq12d_mul_by_1ab) { st_fq12d(out, 0, fq12d_mul_by_1ab(ld_fq12d(in, 0), ld_fq2d(in, 12), ld_fq2d(in, 14))); }
#endif
#if PROBE_ON(fq12d_cyclotomic_sqr)
PROBE_KERNEL(p_fq12d_cyclotomic_sqr) { st_fq12d(out, 0, fq12d_cyclotomic_sqr(ld_fq12d(in, 0))); }
#endif
#if PROBE_ON(fq12d_sqr_parked)
// the Miller loop's squaring as the one-lane share check runs it (pairingd.hpp: one operand of the
// second Fq6 product streamed from the lane's LDS slot)
PROBE_KERNEL(p_fq12d_sqr_parked) {
  __shared__ uint32_t park[LDS_FQ12D_DWORDS * LDS_FQ12_STRIDE];
  st_fq12d(out, 0, fq12d_sqr_parked(ld_fq12d(in, 0), (lds_u32*)(park + threadIdx.x)));
}
#endif
// the final-exponentiation steps' own forms (fe1d.hpp): the fenced Granger-Scott squaring, one
// compressed (Karabina) squaring, and the product by a value streamed from the lane's LDS slot
#if PROBE_ON(fq12d_cyclotomic_sqr_seq)
PROBE_KERNEL(p_fq12d_cyclotomic_sqr_seq) { st_fq12d(out, 0, fq12d_cyclotomic_sqr_seq(ld_fq12d(in, 0))); }
#endif
#if PROBE_ON(karabina_sqr)
PROBE_KERNEL(p_karabina_sqr) {
  fq12c c{ld_fq2d(in, 0), ld_fq2d(in, 2), ld_fq2d(in, 4), ld_fq2d(in, 6)};
  karabina_sqr(c);
  st_fq2d(out, 0, c.g1);
  st_fq2d(out, 2, c.g2);
  st_fq2d(out, 4, c.g3);
  st_fq2d(out, 6, c.g5);
}
#endif
#if PROBE_ON(fq12d_mul_slot)
PROBE_KERNEL(p_fq12d_mul_slot) {
  __shared__ uint32_t slots[FE1_WORDS * 64];
  lds_u32* a = (lds_u32*)(slots + threadIdx.x);
  s1_copy<64, 64>(a, (const uint32_t*)in + 12 * 14 * 64 + threadIdx.x);
  HBX_SEQ();
  st_fq12d(out, 0, fq12d_mul_slot<64>(ld_fq12d(in, 0), a));
}
#endif
