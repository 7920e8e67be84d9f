// C-ABI implementation (include/hbx.h): context, device buffers, kernel launches.
// Host code only orchestrates -- every verification, combine and hash runs in the HIP kernels of
// hbx_kernels.hip.  There is no CPU fallback: without a usable HIP device every call fails with
// HBX_E_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/hbx.h"
#include "hbx_kernels.hip"
#include "broadcast.hpp"
#include "addplan.hpp"
#include "bcplan.hpp"
#if defined(HBX_TU) && HBX_TU == 0
#include "_kdecl.hpp"  // the kernels live in translation units 1..6 (tools/build.py)
#endif

#if !defined(HBX_TU) || HBX_TU == 0
using namespace hbx;

namespace {

// one wave per SIMD: a one-lane-per-check launch with fewer waves leaves SIMDs idle (addplan.hpp)
constexpr size_t FILL_WAVES = hbx_addplan::FILL_WAVES;
// the combine's precomputed tables: what k_prepare_lines' table lanes build (prepare_impl)
constexpr uint32_t COMB_FORM = 1;

// Ownership rule: every device allocation is a dbuf, every pinned one a pinbuf, every event a
// dev_event or the timing pool's, and each frees what it holds in its destructor: a context's by
// `delete`, a per-call temporary's at the end of its scope.  No list names a buffer to free it.
// live_buffers: the device and pinned allocations this process holds (hbx_debug_live_buffers).
std::atomic<uint64_t> live_buffers{0};

struct dbuf {
  void* p = nullptr;
  size_t cap = 0;
  dbuf() = default;
  dbuf(const dbuf&) = delete;
  dbuf& operator=(const dbuf&) = delete;
  ~dbuf() { release(); }
  bool ensure(size_t bytes) {
    if (bytes <= cap && p) return true;
    release();
    if (bytes == 0) bytes = 16;
    if (hipMalloc(&p, bytes) != hipSuccess) return false;
    live_buffers++;
    cap = bytes;
    return true;
  }
  void release() {
    if (p && hipFree(p) == hipSuccess) live_buffers--;
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// Pinned host memory; grows with half as much again, so a run of slightly longer calls reallocates once.
struct pinbuf {
  void* p = nullptr;
  size_t cap = 0;
  pinbuf() = default;
  pinbuf(const pinbuf&) = delete;
  pinbuf& operator=(const pinbuf&) = delete;
  ~pinbuf() { release(); }
  bool ensure(size_t bytes) {
    if (bytes <= cap) return true;
    release();
    const size_t want = bytes + bytes / 2 + 4096;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return false;
    live_buffers++;
    cap = want;
    return true;
  }
  void release() {
    if (p && hipHostFree(p) == hipSuccess) live_buffers--;
    p = nullptr;
    cap = 0;
  }
};

// An ordering event (no timing), created on first use; `recorded`: there is something to wait for.
struct dev_event {
  hipEvent_t e = nullptr;
  bool recorded = false;
  dev_event() = default;
  dev_event(const dev_event&) = delete;
  dev_event& operator=(const dev_event&) = delete;
  ~dev_event() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t create() { return e ? hipSuccess : hipEventCreateWithFlags(&e, hipEventDisableTiming); }
};

// opt-in kernel timing: event pairs per timed kernel (hbx_set_timing / hbx_kernel_time)
struct timing_state {
  bool on = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> tev[HBX_K_COUNT];
  std::vector<hipEvent_t> pool;
  timing_state() = default;
  timing_state(const timing_state&) = delete;
  timing_state& operator=(const timing_state&) = delete;
  ~timing_state() {
    reset();
    for (hipEvent_t e : pool) (void)hipEventDestroy(e);
  }
  hipEvent_t get() {
    if (!pool.empty()) {
      hipEvent_t e = pool.back();
      pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
  }
  void reset() {
    for (auto& v : tev) {
      for (auto& pr : v) {
        pool.push_back(pr.first);
        pool.push_back(pr.second);
      }
      v.clear();
    }
  }
};

// The state of an incremental add, one per share kind (hbx_add_dec_shares_d: rows = proposers, g1a;
// hbx_add_sig_shares_d: rows = instances, g2a).  The candidates of an add are decoded and checked
// apart from the held matrix, in the same [rows][n] layout (only the add's tiles are ever written or
// read): their points, decode statuses and verdicts.  `mask` holds the add's positions as the tile
// launch's present mask, all 0 between calls; mask_m = the bytes of it known to be 0.  item_st: the
// statuses of the items that touch no position (the coin's decode alone writes them).  in / out:
// the host form's staging of the items' bytes and of their statuses.
struct add_state {
  dbuf pts, pt_st, verdict, mask, item_st, in, out;
  size_t mask_m = 0;
  bool ensure(size_t m, size_t pt_bytes) {
    return pts.ensure(m * pt_bytes) && pt_st.ensure(m * 4) && verdict.ensure(m) && mask.ensure(m);
  }
  // Before the add's launches: zeroes the mask if it is a new buffer or an interrupted call left
  // it marked; from here to end() it counts as marked.
  hipError_t begin(size_t m, hipStream_t s) {
    const hipError_t e = mask_m < m ? hipMemsetAsync(mask.p, 0, mask.cap, s) : hipSuccess;
    mask_m = 0;
    return e;
  }
  // After the merge is enqueued: it clears every byte the decode set.
  void end() { mask_m = mask.cap; }
};

}  // namespace

struct hbx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool coin_h_ready = false;  // coin_H (the true hash_g2 of the prepared nonces) computed
  dev_event coin_ready_ev;  // end of hbx_prepare_nonces' work: later coin calls on any stream wait on it
  std::string err = "ok";
  int digest = DIGEST_SHA256;         // hbx_set_digest: threshold_crypto's DIGEST
  int merkle = 0;                     // hbx_set_merkle_digest: HBX_MERKLE_*
  int verify_lanes = 0;               // hbx_set_verify_lanes: 0 auto, 1, 2, 3 or 6 lanes per share check
  int combine_lanes = 0;              // hbx_set_combine_lanes: 0 auto, 1 or 4 lanes per Lagrange term
  int coin_lanes_used = 0;            // lanes per check of the last signature-share launch
  int lanes_used = 0;                 // lanes per check of the last share-check launch
  int ct_check = HBX_CT_CHECK_WIDE;   // hbx_set_ct_check: Ciphertext::verify of hbx_sk_decrypt
  int ct_check_used = -1;             // the mode the last hbx_sk_decrypt ran (-1: none yet)
  // era state
  uint32_t n_keys = 0;
  dbuf comb_partial, comb_done;  // k_combine_q: per-block partial sums, per-proposer block counters
  dbuf pk, pk_m, pk64, pk_status, pk_comp;  // pk_m = [3(x^2-1)] pk, pk64 = [2^64] pk (k_scale_keys)
  dbuf g1tab;  // fixed-base tables of the key shares, [n][64][15] affine (k_g1_tables; coin master identity)
  // epoch state
  uint32_t p_ct = 0;
  dbuf U, G2pts, Hj, lines, lines_d, scratch, ct_ok, ct_valid, dec_st;
  // the one-lane Miller kernel's lines, divided by their constant term (k_normalise_lines), and
  // the per-proposer flag of a line that has no such form
  dbuf lines_u, line_degen;
  // own-share mode (hbx_set_own_share): this node's index and secret share (8 LE limbs), and its
  // own decryption shares of the prepared ciphertexts
  uint32_t own_me = UINT32_MAX;
  dbuf own_sk, own_S, own_part;
  bool own_ready = false;  // own_S computed by the last prepare
  bool ct_known = false;  // ct_valid computed (else deferred into the next share verification)
  const uint8_t* d_v_blob = nullptr;  // device V blob used by the combine (caller-owned for _d)
  const uint64_t* d_v_off = nullptr;
  uint64_t max_v_len = 0;
  dbuf v_blob_own, v_off_own, u_comp_own, w_comp_own;
  // verification state: n_shares / verified_p of the last verify after the latest prepare
  // (0 = none: a prepare invalidates S / valid for the combine)
  uint32_t n_shares = 0, verified_p = 0;
  dbuf S, S_status, fallback, valid, shares_own, present_own, gslot;
  dbuf fe1slot;  // one-lane checks: the final exponentiation's global slots F, T, G (fe1d.hpp)
  uint32_t verify_tiles = 0;  // check blocks of the last share-check launch (hbx_get_verify_tiles_used)
  // hbx_add_dec_shares_d: the add's state, and the all-absent shares and present mask that
  // establish the epoch's matrix
  add_state dec_add;
  dbuf add_zero;
  uint32_t force_fallback = 0;  // hbx_debug_force_fallback (tests only)
  uint32_t force_degen = 0;  // hbx_debug_force_degenerate (tests only)
  // the combine's window tables (g1d.hpp; built by k_prepare_lines in the fused epoch call only):
  // cap + 1 slots of G1D_TABS entries per proposer and their presence flags.  They belong to the
  // shares decoded by the last fused prepare (tab_ready; dropped wherever n_shares is reset and
  // when a verification decodes other shares into S).
  int32_t comb_margin = HBX_COMBINE_MARGIN_AUTO;  // hbx_debug_set_combine_margin
  dbuf comb_tab, comb_tab_ok, comb_slow;
  bool tab_ready = false;
  uint32_t comb_slow_p = 0;  // proposers of the last combine launch (entries of comb_slow)
  uint32_t tab_cap = 0, tab_me = UINT32_MAX, tab_n = 0, tab_p = 0, tab_form = 0;
  // batched share verification (hbx_set_batch_verify): the seed, the index of the next batched
  // verification under it, and the p of the last verification if that one was batched (else 0);
  // key terms T[n + 1], ciphertext terms C[p], the sums Asum (affine) / AJ (Jacobian) / A / B [p],
  // per-column classes, verdicts, the per-share launch's ciphertext gate and the three counters
  bool batch_on = false;
  uint64_t batch_call = 0;
  uint32_t batch_last_p = 0;
  dbuf b_seed, b_AJ, b_T, b_C, b_Asum, b_A, b_B, b_cls0, b_cand, b_pass, b_zero, b_cls, b_ctok, b_stats;
  // u32 counters of the checks the fallback path decided: one for the one-lane decryption-share
  // checks, one for the two-lane coin checks, one for the pair-lane ciphertext checks of
  // hbx_sk_decrypt, summed over the call's chunks (launches of different kinds on different streams
  // must not mix their counts), one for the pair-lane signature checks of hbx_verify_sigs_keyed, summed
  // likewise; fb_last names the counter of the last launch of any kind, or none
  // when that launch used a lane count without a fallback path
  dbuf fb_lanes, fb_coin, fb_ct, fb_sigs;
  dbuf* fb_last = nullptr;
  dbuf hs[6];                   // staging of the host-pointer broadcast calls
  // combine state
  dbuf keys, status, out_own;
  // broadcast state: GF(2^8) tables, encoding matrix of (rs_k, rs_m), reconstruct jobs, Merkle
  dbuf gf_log, gf_exp;
  uint32_t rs_k = 0, rs_m = 0;
  dbuf rs_enc, rs_enc_job, rs_enc_coef, rs_enc_ptab, rs_ptab_d, rs_ptab_p, rs_jobs_d, rs_jobs_p, rs_coef_d, rs_coef_p, leaf_hash, leaf_slots, val_digest, roots;
  // ragged broadcast calls: the call's host descriptors are copied into pinned staging (rg_pin)
  // and uploaded to rg_dev in one async copy; rg_ev marks the end of that copy, the only thing a
  // later call waits for on the host (before it rewrites the staging)
  dbuf rg_dev;
  pinbuf rg_pin;
  dev_event rg_ev;
  // the echo store (hbx_prepare_broadcast): bc_live = the slots belong to (bc_inst, bc_k, bc_m,
  // bc_max) and the current Merkle digest (hbx_set_merkle_digest clears it).  Per slot inst * n +
  // sender: a state byte, the shard length, the shard row (bc_pitch = bc_max rounded up to 4; one
  // canary row follows the last slot's), the proof's root and its leaf digest.  bc_item_st: an add's
  // item statuses when the caller takes none.  A listed decode's work: the gathered rows, their
  // presence and leaf digests, the attempts' shard-size flags.
  bool bc_live = false;
  uint32_t bc_inst = 0, bc_k = 0, bc_m = 0, bc_max = 0, bc_pitch = 0;
  dbuf bc_state, bc_len, bc_shard, bc_root, bc_leaf, bc_item_st;
  dbuf bc_work, bc_present, bc_leaf_w, bc_size_bad;
  // common coin state: nonces' hash_g2 points and lines, signature shares, combined signatures
  uint32_t coin_I = 0, coin_n = 0;
  dbuf coin_blob, coin_off, coin_H, coin_Hp, coin_lines, coin_scratch, coin_sk, coin_sig96, coin_sig, coin_sig_st, coin_present,
      coin_valid, coin_comb, coin_comb_st, coin_mpk_comp, coin_mpk, coin_mpk_st, coin_ok, coin_par, coin_out96;
  // PublicKey::verify batches (hbx_verify_sigs)
  dbuf vs_pk, vs_blob, vs_off, vs_H, vs_lines, vs_lines_d, vs_scratch, vs_sig96, vs_sig, vs_sig_st, vs_status;
  // the keyed form (hbx_verify_sigs_keyed / hbx_sign_msgs): the key table's bytes, points and HBX_PT_*,
  // the items' key indices, the pairs' global slots of one pass, the signing key
  dbuf vk_pk48, vk_pk, vk_pkst, vk_idx, vk_gslot, vk_sk;
  dbuf coin_lines_d;  // the nonces' lines in the coin check's digit form
  bool coin_lines_ready = false;  // coin_lines_d computed for the prepared nonces (one-lane checks only)
  uint8_t coin_mpk48[48] = {0};   // the master key coin_mpk was decoded from
  bool coin_mpk_known = false;
  dbuf coin_use;      // hbx_combine_signatures_d: the verified shares masked by the caller's subset
  // hbx_add_sig_shares_d: coin_live = the [coin_I][coin_n] matrix belongs to the prepared nonces and
  // the current keys (read by the add alone: a matrix verification or an add sets it;
  // hbx_prepare_nonces, hbx_set_digest and hbx_set_pk_shares clear it); sig_add = the add's state.
  bool coin_live = false;
  uint32_t coin_tiles = 0;  // check blocks of the last signature-share launch (hbx_get_coin_tiles_used)
  add_state sig_add;
  dbuf coin_use_in;  // hbx_combine_signatures_insts: the host form's staging of `use`
  // SyncKeyGen commitment checks (hbx_bivar_rows / hbx_bivar_check_acks)
  dbuf bv_commit48, bv_C, bv_cst, bv_rows, bv_rows48, bv_pst, bv_ackp, bv_acky, bv_vals, bv_out;
  // SyncKeyGen SecretKey::decrypt (hbx_sk_decrypt): the key's limbs, plaintexts, HBX_CT_* per ciphertext
  dbuf kg_sk, kg_out, kg_st;
  timing_state timing;
  // ordering of this context's work across streams: every entry point waits on `ev_last` before
  // enqueuing on its stream and records it after (stream_scope), so a host call on `stream`
  // after a _d call on the caller's stream (or on NULL, which does not order against the
  // non-blocking `stream`) sees that call's results; readouts wait on this event only, not on
  // the whole device (other contexts' epochs in flight keep running)
  dev_event ev_last;
  // a new set of prepared ciphertexts (or none): S / valid of an earlier verify belong to other
  // ciphertexts, the combine's tables to other shares
  void invalidate_epoch() {
    ct_known = false;
    n_shares = 0;
    verified_p = 0;
    tab_ready = false;
  }
};

// Records a start event before and a stop event after one kernel launch on stream s.
struct timed {
  hbx_ctx* c;
  int id;
  hipStream_t s;
  hipEvent_t e0 = nullptr;
  timed(hbx_ctx* c_, int id_, hipStream_t s_) : c(c_), id(id_), s(s_) {
    if (c->timing.on && (e0 = c->timing.get())) (void)hipEventRecord(e0, s);
  }
  ~timed() {
    if (!e0) return;
    hipEvent_t e1 = c->timing.get();
    if (!e1) return;
    (void)hipEventRecord(e1, s);
    c->timing.tev[id].emplace_back(e0, e1);
  }
};

static int fail(hbx_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(ctx, expr)                                                                      \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess) return fail(ctx, HBX_E_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)
#define HBX_DEVICE(c) HIPCHK(c, hipSetDevice(c->device))

// _d API: the caller's stream; NULL is the HIP null stream (a framework's default stream), so the
// enqueued work is ordered with the caller's own work on it.  The stream first waits for this
// context's previous work on any stream (ev_last).
static hipStream_t pick(hbx_ctx* c, void* s) {
  hipStream_t st = static_cast<hipStream_t>(s);
  if (c && c->ev_last.recorded) (void)hipStreamWaitEvent(st, c->ev_last.e, 0);
  return st;
}
// Records ev_last on the entry point's stream when it returns (on every return path).
struct stream_scope {
  hbx_ctx* c;
  hipStream_t s;
  ~stream_scope() {
    if (c && c->ev_last.e && hipEventRecord(c->ev_last.e, s) == hipSuccess) c->ev_last.recorded = true;
  }
};
// The prologue of an entry point, after its argument checks: this context's device, `s` = the
// call's stream ordered after the context's earlier work, ev_last recorded on it at every return.
#define HBX_ENTER(c, on_stream)                          \
  HBX_DEVICE(c);                                         \
  [[maybe_unused]] hipStream_t s = pick(c, on_stream);   \
  stream_scope ss_ { c, s }
// Host-side wait for everything this context has enqueued (its own stream and callers' streams).
static hipError_t quiesce(hbx_ctx* c) {
  if (c->ev_last.recorded) {
    const hipError_t e = hipEventSynchronize(c->ev_last.e);
    if (e != hipSuccess) return e;
  }
  return hipStreamSynchronize(c->stream);
}

// bit k = (bytes[k] == 1): status bytes (HBX_SHARE_VALID, HBX_CT_VALID) and 0/1 flags alike
static void pack_bits(const uint8_t* bytes, size_t n, uint8_t* bits) {
  memset(bits, 0, (n + 7) / 8);
  for (size_t k = 0; k < n; k++)
    if (bytes[k] == 1) bits[k >> 3] |= (uint8_t)(1u << (k & 7));
}

static bool scalars_canonical(const uint8_t* s32, size_t count);

// Pairing checks of jobs [q_first, q_last] of every proposer (q < n: shares, q == n: ciphertext).
// `ct_ok`: the proposers to examine (c->ct_ok, or the batched verification's gate of it).
static int launch_pair_checks(hbx_ctx* c, hipStream_t s, uint32_t n, uint32_t p, uint32_t q_first, uint32_t q_last,
                              const uint8_t* d_present, const uint8_t* ct_ok) {
  if (!c->fallback.ensure((size_t)p * (n + 1)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "out of device memory (fallback flags)");
  HIPCHK(c, hipMemsetAsync(c->fallback.p, 0, (size_t)p * (n + 1), s));
  const uint32_t jobs = q_last - q_first + 1;
  {
    timed t_(c, HBX_K_CT_CHECKS, s);
    hipLaunchKernelGGL(k_verify_wide, dim3((jobs + WG_GROUPS - 1) / WG_GROUPS, p), dim3(WG_THREADS), 0, s,
                       c->S.as<g1a>(), c->S_status.as<int32_t>(), d_present, c->pk_m.as<g1a>(), c->n_keys,
                       c->U.as<g1a>(), c->G2pts.as<g2a>(), c->lines.as<line_block>(), ct_ok, n,
                       q_first, q_last, c->valid.as<uint8_t>(), c->ct_valid.as<uint8_t>(), c->fallback.as<uint8_t>());
  }
  HIPCHK(c, hipGetLastError());
  const size_t all = (size_t)p * (n + 1);
  hipLaunchKernelGGL(k_pair_fallback, dim3((unsigned)((all + 63) / 64)), dim3(64), 0, s, c->fallback.as<uint8_t>(),
                     c->S.as<g1a>(), c->pk_m.as<g1a>(), c->U.as<g1a>(), c->G2pts.as<g2a>(), c->lines.as<line_block>(),
                     n, p, c->valid.as<uint8_t>(), c->ct_valid.as<uint8_t>());
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// Batched verification, up to the per-share launch: one block per column for the share sums beside
// the key terms, then A_j and B_j, the p column equations on the six-lane check (the lowest latency per check:
// about half the 16-lane wide executor's for 256 columns, DESIGN.md "Batched share verification"), then
// per column its class, the counters and the ciphertext
// gate b_ctok under which the per-share kernels skip the columns the equation decided.
static int launch_batch_columns(hbx_ctx* c, hipStream_t s, const uint8_t* d_present, uint32_t n, uint32_t p, bool own,
                                bool fold) {
  if (!c->b_AJ.ensure((size_t)p * sizeof(g1j)) || !c->b_T.ensure((size_t)(n + 1) * sizeof(g1j)) ||
      !c->b_C.ensure((size_t)p * sizeof(g1j)) || !c->b_Asum.ensure((size_t)p * sizeof(g1a)) ||
      !c->b_A.ensure((size_t)p * sizeof(g1a)) || !c->b_B.ensure((size_t)p * sizeof(g1a)) || !c->b_cls0.ensure(p) ||
      !c->b_cand.ensure(p) || !c->b_pass.ensure(p) || !c->b_zero.ensure((size_t)p * 4) ||
      !c->b_cls.ensure(p) || !c->b_ctok.ensure(p) || !c->b_stats.ensure(12))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_dec_shares_d: out of device memory (batch)");
  HIPCHK(c, hipMemsetAsync(c->b_zero.p, 0, (size_t)p * 4, s));
  HIPCHK(c, hipMemsetAsync(c->b_pass.p, 0, p, s));
  HIPCHK(c, hipMemsetAsync(c->b_stats.p, 0, 12, s));
  {
    timed t_(c, HBX_K_BATCH_MSM, s);
    // the key-side lanes (n + 1, and p ciphertext terms with `fold`) as extra blocks of the same launch
    const uint32_t key_blocks = (n + 1 + (fold ? p : 0) + BATCH_THREADS - 1) / BATCH_THREADS;
    hipLaunchKernelGGL(k_batch_msm, dim3(p + key_blocks), dim3(BATCH_THREADS), 0, s, c->S.as<g1a>(),
                       c->S_status.as<int32_t>(), d_present, n, c->n_keys, own ? c->own_me : UINT32_MAX,
                       c->b_seed.as<uint8_t>(), c->batch_call, p, c->pk_m.as<g1a>(), fold ? 1u : 0u, c->b_T.as<g1j>(),
                       c->b_C.as<g1j>(), c->ct_ok.as<uint8_t>(), c->ct_known ? c->ct_valid.as<uint8_t>() : nullptr,
                       c->U.as<g1a>(), c->G2pts.as<g2a>(), c->b_Asum.as<g1a>(), c->b_AJ.as<g1j>(),
                       c->b_cls0.as<uint8_t>(), c->b_cand.as<uint8_t>());
    hipLaunchKernelGGL(k_batch_fin, dim3(p), dim3(BATCH_THREADS), 0, s, c->S_status.as<int32_t>(), d_present, n,
                       c->n_keys, own ? c->own_me : UINT32_MAX, c->b_T.as<g1j>(), c->b_C.as<g1j>(), fold ? 1u : 0u,
                       c->b_cand.as<uint8_t>(), c->b_Asum.as<g1a>(), c->b_AJ.as<g1j>(), c->b_A.as<g1a>(),
                       c->b_B.as<g1a>());
  }
  HIPCHK(c, hipGetLastError());
  {
    timed t_(c, HBX_K_BATCH_CHECK, s);
    // "one share per proposer": S = A, every status decodable, the key of column j = B_j, the
    // verdict byte in b_pass (1 = the equation holds); the identity cases are check2_g6d's
    hipLaunchKernelGGL(k_verify_shares6, dim3(1, p), dim3(64), 0, s, c->b_A.as<g1a>(), c->b_zero.as<int32_t>(), nullptr,
                       c->b_B.as<g1a>(), 1u, c->G2pts.as<g2a>(), c->lines_d.as<line_block_d>(), c->b_cand.as<uint8_t>(),
                       1u, c->b_pass.as<uint8_t>(), UINT32_MAX, nullptr, 1u, nullptr);
    hipLaunchKernelGGL(k_batch_mask, dim3((p + 63) / 64), dim3(64), 0, s, c->b_cls0.as<uint8_t>(), c->b_pass.as<uint8_t>(),
                       c->ct_ok.as<uint8_t>(), p, c->b_cls.as<uint8_t>(), c->b_ctok.as<uint8_t>(),
                       c->b_stats.as<uint32_t>());
  }
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// ---- broadcast: host-side set-up (ReedSolomon::new; tables and matrices only, no shard data) ----
struct gf_host {
  uint16_t lg[256];
  uint8_t ex[768];
  uint8_t mul(uint8_t a, uint8_t b) const { return (a == 0 || b == 0) ? 0 : ex[lg[a] + lg[b]]; }
  uint8_t inv(uint8_t a) const { return ex[255 - lg[a]]; }
  uint8_t pow(uint8_t a, uint32_t n) const {  // galois_8::exp, 0^0 = 1
    if (n == 0) return 1;
    if (a == 0) return 0;
    return ex[(lg[a] * n) % 255];
  }
};

static const gf_host& gf() {
  static gf_host g = [] {
    gf_host t{};
    uint32_t x = 1;
    for (int i = 0; i < 768; i++) t.ex[i] = 0;
    for (int i = 0; i < 255; i++) {
      t.ex[i] = (uint8_t)x;
      t.ex[i + 255] = (uint8_t)x;
      t.lg[x] = (uint16_t)i;
      x <<= 1;
      if (x & 0x100) x ^= 0x11D;
    }
    t.lg[0] = GF_LOG_ZERO;
    return t;
  }();
  return g;
}

// Byte-permute tables of one coefficient (layout in broadcast.hpp, gf_ptab).
static gf_ptab gf_perm_table(uint8_t c) {
  const gf_host& g = gf();
  uint8_t b[20];
  for (int i = 0; i < 8; i++) {
    b[i] = g.mul(c, (uint8_t)i);
    b[8 + i] = g.mul(c, (uint8_t)(i << 3));
  }
  for (int i = 0; i < 4; i++) b[16 + i] = g.mul(c, (uint8_t)(i << 6));
  gf_ptab t{};
  for (int w = 0; w < 5; w++)
    t.w[w] = (uint32_t)b[4 * w] | ((uint32_t)b[4 * w + 1] << 8) | ((uint32_t)b[4 * w + 2] << 16) |
             ((uint32_t)b[4 * w + 3] << 24);
  return t;
}

// The compiled triple tiles (output rows per pass, two dwords per lane), in the order of preference.
static const int rs_ch3[] = {21, 14, 12, 28, 42};
static_assert(rs_perm3_lds_bytes(RS_MAX_K, 12) <= 65536, "the 12-row tile's tables fit the LDS for every k");

// The tile whose row count wastes the fewest computed rows on `no` outputs per instance (each
// pass over the k input rows yields CH outputs; a short last pass still reads all k rows), among
// those whose tables fit the LDS at this k; ties to the earlier entry: the 21-row tile runs 88
// VGPRs (5 waves per SIMD) against 105 for 28 rows and 130 for 42 (r06t21: encode 0.405 ->
// 0.387-0.398 ms, the decode with spread erasures 1.33 -> 1.22 ms)
static int rs_tile3(uint32_t k, uint32_t no) {
  int ch = 12, best_rows = 1 << 30;
  for (int t : rs_ch3) {
    if (rs_perm3_lds_bytes(k, t) > 65536) continue;
    const int rows = (int)((no + t - 1) / t) * t;
    if (rows < best_rows) ch = t, best_rows = rows;
  }
  return ch;
}

// Calls f with tile `ch` of rs_ch3 as a compile-time constant (std::integral_constant<int, CH>).
template <class F>
static void rs_with_tile(int ch, F&& f) {
  switch (ch) {
    case 42: return f(std::integral_constant<int, 42>{});
    case 28: return f(std::integral_constant<int, 28>{});
    case 14: return f(std::integral_constant<int, 14>{});
    case 12: return f(std::integral_constant<int, 12>{});
    default: return f(std::integral_constant<int, 21>{});
  }
}

// One coding pass: the triple byte-permute kernel (4.0 VALU ops per coefficient-dword) when rows
// are whole dwords, else the LDS log/exp one.
// `no` is the outputs one instance's pass is expected to write: m on encode; on a reconstruct pass
// the f = m / 2 erasures of hbbft's fault bound (the bench's pattern; up to m still runs, in more passes).
static void rs_code(hbx_ctx* c, uint8_t* d_shards, size_t stride, uint32_t L, uint32_t k, uint32_t inst,
                    const rs_job* jobs, const uint16_t* coef, const gf_ptab* ptab, uint32_t job_stride, uint32_t no,
                    hipStream_t s) {
  timed t_(c, HBX_K_RS_CODE, s);
  if (no == 0) no = 1;  // grid.z >= 1; the kernels read the true count from the job
  if (L % 4 != 0) {
    hipLaunchKernelGGL(k_rs_code, dim3((L + 1023) / 1024, inst), dim3(256), 0, s, d_shards, stride, L, k, jobs, coef,
                       job_stride, c->gf_log.as<uint16_t>(), c->gf_exp.as<uint8_t>());
    return;
  }
  const uint32_t Ld = L / 4;
  int ch = rs_tile3(k, no);
  // tuning: HBX_RS_CH3 = 200 + CH pins a compiled tile (read once per process); any other value,
  // or a tile whose tables do not fit the LDS at this k, is ignored
  static const int pin = [] {
    const char* e = getenv("HBX_RS_CH3");
    const int v = e ? atoi(e) - 200 : 0;
    for (int t : rs_ch3)
      if (v == t) return v;
    return 0;
  }();
  if (pin && rs_perm3_lds_bytes(k, pin) <= 65536) ch = pin;
  rs_with_tile(ch, [&](auto tile) {
    constexpr int c3 = decltype(tile)::value;
    hipLaunchKernelGGL((k_rs_code_perm3<c3, 2>), dim3((Ld + 511) / 512, inst, (no + c3 - 1) / c3), dim3(256),
                       rs_perm3_lds_bytes(k, c3), s, d_shards, stride, L, k, jobs, ptab, job_stride);
  });
}

// Encoding matrix V * inverse(V[0..k]) with V[r][c] = r^c ((k + m) x k, reed-solomon-erasure 3.1.0).
static bool rs_matrix(uint32_t k, uint32_t m, std::vector<uint8_t>& out) {
  const gf_host& g = gf();
  const uint32_t n = k + m;
  std::vector<uint8_t> V(n * k), A(k * 2 * k);
  for (uint32_t r = 0; r < n; r++)
    for (uint32_t c = 0; c < k; c++) V[r * k + c] = g.pow((uint8_t)r, c);
  for (uint32_t r = 0; r < k; r++)
    for (uint32_t c = 0; c < 2 * k; c++) A[r * 2 * k + c] = c < k ? V[r * k + c] : (c - k == r ? 1 : 0);
  for (uint32_t r = 0; r < k; r++) {
    if (A[r * 2 * k + r] == 0) {
      uint32_t b = r + 1;
      while (b < k && A[b * 2 * k + r] == 0) b++;
      if (b == k) return false;
      for (uint32_t c = 0; c < 2 * k; c++) std::swap(A[r * 2 * k + c], A[b * 2 * k + c]);
    }
    const uint8_t inv = g.inv(A[r * 2 * k + r]);
    for (uint32_t c = 0; c < 2 * k; c++) A[r * 2 * k + c] = g.mul(A[r * 2 * k + c], inv);
    for (uint32_t i = 0; i < k; i++) {
      const uint8_t f = A[i * 2 * k + r];
      if (i == r || !f) continue;
      for (uint32_t c = 0; c < 2 * k; c++) A[i * 2 * k + c] ^= g.mul(f, A[r * 2 * k + c]);
    }
  }
  out.assign(n * k, 0);
  for (uint32_t r = 0; r < n; r++)
    for (uint32_t c = 0; c < k; c++) {
      uint8_t acc = 0;
      for (uint32_t q = 0; q < k; q++) acc ^= g.mul(V[r * k + q], A[q * 2 * k + k + c]);
      out[r * k + c] = acc;
    }
  return true;
}

static int rs_bounds(hbx_ctx* c, uint32_t k, uint32_t m) {
  if (k == 0 || k > (uint32_t)RS_MAX_K || k + m > (uint32_t)RS_MAX_N)
    return fail(c, HBX_E_INVALID_ARG, "rs: need 1 <= k <= %d and k + m <= %d (k=%u m=%u)", RS_MAX_K, RS_MAX_N, k, m);
  return HBX_OK;
}

static int rs_setup(hbx_ctx* c, uint32_t k, uint32_t m, hipStream_t s) {
  if (int rc = rs_bounds(c, k, m)) return rc;
  if (!c->gf_log.p) {
    if (!c->gf_log.ensure(512) || !c->gf_exp.ensure(768)) return fail(c, HBX_E_OUT_OF_MEMORY, "rs: tables");
    HIPCHK(c, hipMemcpyAsync(c->gf_log.p, gf().lg, 512, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(c->gf_exp.p, gf().ex, 768, hipMemcpyHostToDevice, s));
  }
  if (c->rs_k == k && c->rs_m == m) return HBX_OK;
  std::vector<uint8_t> M;
  if (m > 0 && !rs_matrix(k, m, M)) return fail(c, HBX_E_INVALID_ARG, "rs: singular Vandermonde block");
  if (m == 0) M.assign((size_t)k * k, 0);
  rs_job job{};
  job.n_out = (int32_t)m;
  for (uint32_t q = 0; q < k; q++) job.in_idx[q] = (int32_t)q;
  for (uint32_t o = 0; o < m; o++) job.out_idx[o] = (int32_t)(k + o);
  std::vector<uint16_t> coef((size_t)RS_MAX_N * k, GF_COEF_ZERO);
  for (uint32_t o = 0; o < m; o++)
    for (uint32_t q = 0; q < k; q++) {
      const uint8_t v = M[(size_t)(k + o) * k + q];
      coef[(size_t)o * k + q] = v ? gf().lg[v] : GF_COEF_ZERO;
    }
  std::vector<gf_ptab> ptab((size_t)m * k);
  for (uint32_t o = 0; o < m; o++)
    for (uint32_t q = 0; q < k; q++) ptab[(size_t)o * k + q] = gf_perm_table(M[(size_t)(k + o) * k + q]);
  if (!c->rs_enc.ensure(M.size()) || !c->rs_enc_job.ensure(sizeof(rs_job)) || !c->rs_enc_coef.ensure(coef.size() * 2) ||
      !c->rs_enc_ptab.ensure(ptab.size() * sizeof(gf_ptab) + sizeof(gf_ptab)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "rs: matrix");
  HIPCHK(c, hipMemcpyAsync(c->rs_enc_ptab.p, ptab.data(), ptab.size() * sizeof(gf_ptab), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->rs_enc.p, M.data(), M.size(), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->rs_enc_job.p, &job, sizeof(rs_job), hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->rs_enc_coef.p, coef.data(), coef.size() * 2, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipStreamSynchronize(s));  // host staging buffers die at return
  c->rs_k = k;
  c->rs_m = m;
  return HBX_OK;
}

// A reconstruct's set-up: per instance the status and the jobs and coefficients of its two coding
// passes (data, then parity); with `want_perm` their byte-permute tables, which the dword kernels read.
static int rs_reconstruct_tables(hbx_ctx* c, const uint8_t* d_present, uint32_t inst, uint32_t k, uint32_t m,
                                 int32_t* d_status, bool want_perm, hipStream_t s) {
  const size_t tab = (size_t)inst * RS_MAX_N * k;
  if (!c->rs_jobs_d.ensure((size_t)inst * sizeof(rs_job)) || !c->rs_jobs_p.ensure((size_t)inst * sizeof(rs_job)) ||
      !c->rs_coef_d.ensure(tab * 2) || !c->rs_coef_p.ensure(tab * 2) ||
      (want_perm && (!c->rs_ptab_d.ensure(tab * sizeof(gf_ptab)) || !c->rs_ptab_p.ensure(tab * sizeof(gf_ptab)))))
    return fail(c, HBX_E_OUT_OF_MEMORY, "rs_reconstruct: out of device memory");
  hipLaunchKernelGGL(k_rs_setup_reconstruct, dim3(inst), dim3(256), 0, s, d_present, k, m, c->rs_enc.as<uint8_t>(),
                     c->gf_log.as<uint16_t>(), c->gf_exp.as<uint8_t>(), c->rs_jobs_d.as<rs_job>(),
                     c->rs_coef_d.as<uint16_t>(), c->rs_jobs_p.as<rs_job>(), c->rs_coef_p.as<uint16_t>(), d_status);
  if (want_perm) {
    const dim3 tg((RS_MAX_N * k + 255) / 256, inst);
    hipLaunchKernelGGL(k_rs_perm_tables, tg, dim3(256), 0, s, c->rs_jobs_d.as<rs_job>(), c->rs_coef_d.as<uint16_t>(), k,
                       c->gf_log.as<uint16_t>(), c->gf_exp.as<uint8_t>(), c->rs_ptab_d.as<gf_ptab>());
    hipLaunchKernelGGL(k_rs_perm_tables, tg, dim3(256), 0, s, c->rs_jobs_p.as<rs_job>(), c->rs_coef_p.as<uint16_t>(), k,
                       c->gf_log.as<uint16_t>(), c->gf_exp.as<uint8_t>(), c->rs_ptab_p.as<gf_ptab>());
  }
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

static int rs_reconstruct(hbx_ctx* c, uint8_t* d_shards, const uint8_t* d_present, uint32_t inst, uint32_t k,
                          uint32_t m, uint32_t L, int32_t* d_status, hipStream_t s) {
  const size_t stride = (size_t)(k + m) * L;
  if (int rc = rs_reconstruct_tables(c, d_present, inst, k, m, d_status, L % 4 == 0, s)) return rc;
  rs_code(c, d_shards, stride, L, k, inst, c->rs_jobs_d.as<rs_job>(), c->rs_coef_d.as<uint16_t>(),
          c->rs_ptab_d.as<gf_ptab>(), 1u, (m + 1) / 2, s);
  HIPCHK(c, hipGetLastError());
  rs_code(c, d_shards, stride, L, k, inst, c->rs_jobs_p.as<rs_job>(), c->rs_coef_p.as<uint16_t>(),
          c->rs_ptab_p.as<gf_ptab>(), 1u, (m + 1) / 2, s);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// The leaf digests of every family (uniform or ragged leaves, ragged or echo values; a family's two
// kernels share a signature): a SHA-256 block hashes 64 items with 128 threads, a SHA3 block 32 with
// 64.  leaf_blocks: `blocks` of items grouped beforehand; leaf_digests: `items` in a row, `gy` times.
static uint32_t leaf_lanes(const hbx_ctx* c) { return c->merkle == HBX_MERKLE_SHA256 ? 64 : 32; }

template <class K, class... A>
static void leaf_blocks(hbx_ctx* c, hipStream_t s, K sha256, K sha3, dim3 blocks, A... args) {
  timed t_(c, HBX_K_MERKLE_LEAVES, s);
  if (c->merkle == HBX_MERKLE_SHA256) hipLaunchKernelGGL(sha256, blocks, dim3(128), 0, s, args...);
  else hipLaunchKernelGGL(sha3, blocks, dim3(64), 0, s, args...);
}

template <class K, class... A>
static void leaf_digests(hbx_ctx* c, hipStream_t s, K sha256, K sha3, uint32_t items, uint32_t gy, A... args) {
  leaf_blocks(c, s, sha256, sha3, dim3((items + leaf_lanes(c) - 1) / leaf_lanes(c), gy), args...);
}

// Uniform rows' leaf digests into c->leaf_hash: all n leaves, or the `nslots` listed per instance.
static void leaves_uniform(hbx_ctx* c, hipStream_t s, const uint8_t* d_shards, uint32_t inst, uint32_t n, uint32_t L,
                           const uint16_t* slots, uint32_t nslots) {
  leaf_digests(c, s, k_merkle_leaves_sha256, k_merkle_leaves_sha3, slots ? nslots : n, inst, d_shards, (size_t)n * L, n,
               L, c->leaf_hash.as<uint32_t>(), slots, nslots, 0u);
}

static int merkle_roots(hbx_ctx* c, const uint8_t* d_shards, uint32_t inst, uint32_t n, uint32_t L, uint8_t* d_roots,
                        hipStream_t s, uint8_t* d_nodes = nullptr) {
  if (n == 0 || n > (uint32_t)RS_MAX_N) return fail(c, HBX_E_INVALID_ARG, "merkle: need 1 <= n <= 256");
  if (!c->leaf_hash.ensure((size_t)inst * n * 32)) return fail(c, HBX_E_OUT_OF_MEMORY, "merkle: leaf hashes");
  leaves_uniform(c, s, d_shards, inst, n, L, nullptr, 0);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_merkle_tree, dim3(inst), dim3(128), 0, s, c->leaf_hash.as<uint32_t>(), n, d_roots, d_nodes,
                     c->merkle);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// A decode after its reconstruct: the rows' trees, the roots against the expected ones into the
// status, the glue.  With d_leaf_hash the present shards' leaf digests are taken from it (validated
// Echo proofs) and only the reconstructed shards are hashed.  The row layout's two launches are the
// caller's: leaves(slots, nslots) = all leaves' digests (slots == nullptr) or the listed ones', glue().
template <class Leaves, class Glue>
static int decode_tail(hbx_ctx* c, const uint8_t* d_present, const uint8_t* d_leaf_hash, const uint8_t* d_root_expect,
                       uint32_t inst, uint32_t n, uint32_t m, int32_t* d_status, hipStream_t s, Leaves leaves,
                       Glue glue) {
  if (!c->roots.ensure((size_t)inst * 32)) return fail(c, HBX_E_OUT_OF_MEMORY, "decode: roots");
  if (!c->leaf_hash.ensure((size_t)inst * n * 32) ||
      (d_leaf_hash && !c->leaf_slots.ensure((size_t)inst * (m ? m : 1) * 2)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "decode: leaf hashes");
  if (d_leaf_hash) {
    const uint32_t words = inst * n * 8;
    hipLaunchKernelGGL(k_import_leaf_hashes, dim3((words + 255) / 256), dim3(256), 0, s, d_leaf_hash, d_present,
                       inst * n, c->leaf_hash.as<uint32_t>());
    if (m) {  // Coding::Trivial reconstructs nothing: every shard is present or the status is an error
      hipLaunchKernelGGL(k_missing_slots, dim3(inst), dim3(64), 0, s, d_present, n, d_status, m,
                         c->leaf_slots.as<uint16_t>());
      leaves(c->leaf_slots.as<uint16_t>(), m);
    }
  }
  if (!d_leaf_hash) leaves(nullptr, 0u);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_merkle_tree, dim3(inst), dim3(128), 0, s, c->leaf_hash.as<uint32_t>(), n, c->roots.as<uint8_t>(),
                     (uint8_t*)nullptr, c->merkle);
  hipLaunchKernelGGL(k_root_check, dim3((inst + 63) / 64), dim3(64), 0, s, c->roots.as<uint8_t>(), d_root_expect, inst,
                     d_status);
  glue();
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// The host descriptors of a call (rg_desc per instance, and the call's other host arrays) are
// laid out in the context's pinned staging buffer and uploaded with one asynchronous copy on the
// call's stream, so the caller's arrays are consumed at return and nothing waits for the device
// -- except a later staged call, which waits for the previous upload (not the previous kernels)
// before it rewrites the staging, and rs_setup's one-off synchronisation per (k, m).  The same
// staging carries an add's items and tile list and the column combine's list.
// One call's staging as sub-ranges of `sizes` bytes, each starting 8 bytes aligned: fill host<T>(i),
// upload(s), hand dev<T>(i) to the kernels; both go by the one offset of range i.
struct staging {
  hbx_ctx* c;
  size_t off[5], bytes = 0;
  uint8_t* pin = nullptr;  // nullptr: out of memory
  staging(hbx_ctx* c_, std::initializer_list<size_t> sizes) : c(c_) {
    size_t* o = off;
    for (size_t b : sizes) bytes = (*o++ = (bytes + 7) & ~(size_t)7) + b;
    if (c->rg_ev.recorded && hipEventSynchronize(c->rg_ev.e) != hipSuccess) return;
    c->rg_ev.recorded = false;
    if (c->rg_pin.ensure(bytes) && c->rg_ev.create() == hipSuccess && c->rg_dev.ensure(bytes))
      pin = static_cast<uint8_t*>(c->rg_pin.p);
  }
  template <class T>
  T* host(int i) const {
    return reinterpret_cast<T*>(pin + off[i]);
  }
  int upload(hipStream_t s) const {
    HIPCHK(c, hipMemcpyAsync(c->rg_dev.p, c->rg_pin.p, bytes, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->rg_ev.e, s));
    c->rg_ev.recorded = true;
    return HBX_OK;
  }
  template <class T>
  const T* dev(int i) const {
    return reinterpret_cast<const T*>(c->rg_dev.as<uint8_t>() + off[i]);
  }
};

// The long values of a proof list (more than 256 bytes: Echo proofs of real shards) get their leaf
// digests from the leaf kernels, in blocks of one length each (bcplan.hpp group_long).  The digests
// land at the proof's own index, so neither the proofs' order nor the grouping shows in the results.
// Ranges 0 to 2 of the call's staging: val_off u64[count + 1] | blk_len | blk_idx; 3, 4: the caller's.
struct long_values {
  uint32_t lanes;
  std::vector<uint32_t> blk_len, blk_idx;
  long_values(const hbx_ctx* c, const uint64_t* val_off, uint32_t count, uint64_t max_value) : lanes(leaf_lanes(c)) {
    hbx_bcplan::group_long(val_off, count, lanes, max_value, blk_len, blk_idx);
  }
  size_t blocks() const { return blk_len.size(); }
  staging stage(hbx_ctx* c, const uint64_t* val_off, uint32_t count, size_t more3 = 0, size_t more4 = 0) const {
    const size_t b0 = (size_t)(count + 1) * 8, b1 = blocks() * 4, b2 = blocks() * lanes * 4;
    const staging st = more3 || more4 ? staging(c, {b0, b1, b2, more3, more4}) : staging(c, {b0, b1, b2});
    if (st.pin) memcpy(st.host<uint64_t>(0), val_off, b0);
    if (st.pin && b1) memcpy(st.host<uint32_t>(1), blk_len.data(), b1);
    if (st.pin && b1) memcpy(st.host<uint32_t>(2), blk_idx.data(), b2);
    return st;
  }
  // one block of the family's kernel per hash block; `tail` = the kernels' arguments after blk_idx
  template <class K, class... A>
  void hash(hbx_ctx* c, hipStream_t s, const staging& st, K sha256, K sha3, const uint8_t* d_values, A... tail) const {
    if (blocks())
      leaf_blocks(c, s, sha256, sha3, dim3((unsigned)blocks()), d_values, st.dev<uint64_t>(0), st.dev<uint32_t>(1),
                  st.dev<uint32_t>(2), tail...);
  }
};

extern "C" {

const char* hbx_version(void) { return "hbx 0.1.0 gfx950"; }
#ifndef HBX_SOURCE_HASH
#define HBX_SOURCE_HASH "unknown"
#endif
const char* hbx_build_id(void) { return HBX_SOURCE_HASH; }

const char* hbx_last_error(const hbx_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int hbx_ctx_create(int device, hbx_ctx** out) {
  if (!out) return HBX_E_INVALID_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return HBX_E_DEVICE;
  if (device < 0 || device >= count) return HBX_E_INVALID_ARG;
  if (hipSetDevice(device) != hipSuccess) return HBX_E_DEVICE;
  hbx_ctx* c = new hbx_ctx();
  c->device = device;
  if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    delete c;
    return HBX_E_DEVICE;
  }
  if (c->ev_last.create() != hipSuccess) {
    (void)hipStreamDestroy(c->stream);
    delete c;
    return HBX_E_DEVICE;
  }
  *out = c;
  return HBX_OK;
}

int hbx_ctx_destroy(hbx_ctx* c) {
  if (!c) return HBX_E_INVALID_ARG;
  (void)hipSetDevice(c->device);
  (void)quiesce(c);
  const hipStream_t stream = c->stream;
  delete c;  // every buffer and event the context holds frees itself
  (void)hipStreamDestroy(stream);
  return HBX_OK;
}

int hbx_set_digest(hbx_ctx* c, int variant) {
  if (!c || (variant != HBX_DIGEST_SHA256 && variant != HBX_DIGEST_SHA3_256))
    return fail(c, HBX_E_INVALID_ARG, "hbx_set_digest: unknown variant %d", variant);
  c->digest = variant == HBX_DIGEST_SHA3_256 ? DIGEST_SHA3_256 : DIGEST_SHA256;
  c->p_ct = 0;  // hashes prepared under the other digest are void
  c->invalidate_epoch();
  c->coin_I = 0;
  c->coin_n = 0;
  c->coin_live = false;
  return HBX_OK;
}

int hbx_set_verify_lanes(hbx_ctx* c, int lanes) {
  if (!c || lanes < 0 || lanes > 7 || lanes == 4 || lanes == 5)
    return fail(c, HBX_E_INVALID_ARG, "hbx_set_verify_lanes: 0 (auto), 1, 2, 3, 6 or 7, not %d", lanes);
  c->verify_lanes = lanes;
  return HBX_OK;
}

int hbx_get_verify_lanes_used(const hbx_ctx* c) { return c ? c->lanes_used : 0; }

int hbx_set_ct_check(hbx_ctx* c, int mode) {
  if (!c || (mode != HBX_CT_CHECK_WIDE && mode != HBX_CT_CHECK_PAIR))
    return fail(c, HBX_E_INVALID_ARG, "hbx_set_ct_check: 0 (wide) or 1 (pair), not %d", mode);
  c->ct_check = mode;
  return HBX_OK;
}

int hbx_get_ct_check_used(const hbx_ctx* c) { return c ? c->ct_check_used : -1; }

int hbx_debug_force_fallback(hbx_ctx* c, uint32_t every) {
  if (!c) return HBX_E_INVALID_ARG;
  c->force_fallback = every;
  return HBX_OK;
}

int hbx_debug_force_degenerate(hbx_ctx* c, uint32_t every) {
  if (!c) return HBX_E_INVALID_ARG;
  c->force_degen = every;
  return HBX_OK;
}

int64_t hbx_get_fallback_lanes(hbx_ctx* c) {
  if (!c) return HBX_E_INVALID_ARG;
  if (!c->fb_last) return 0;
  HBX_DEVICE(c);
  HIPCHK(c, quiesce(c));
  uint32_t v = 0;
  HIPCHK(c, hipMemcpy(&v, c->fb_last->p, 4, hipMemcpyDeviceToHost));
  return v;
}

int hbx_debug_set_combine_margin(hbx_ctx* c, int32_t margin) {
  if (!c || margin < HBX_COMBINE_TABLES_OFF)
    return fail(c, HBX_E_INVALID_ARG, "hbx_debug_set_combine_margin: margin >= 0, AUTO or TABLES_OFF, not %d", margin);
  c->comb_margin = margin;
  return HBX_OK;
}

int64_t hbx_get_combine_slow_terms(hbx_ctx* c) {
  if (!c) return HBX_E_INVALID_ARG;
  if (!c->comb_slow.p || c->comb_slow_p == 0) return 0;
  HBX_DEVICE(c);
  HIPCHK(c, quiesce(c));
  std::vector<uint32_t> v(c->comb_slow_p);
  HIPCHK(c, hipMemcpy(v.data(), c->comb_slow.p, v.size() * 4, hipMemcpyDeviceToHost));
  int64_t sum = 0;
  for (uint32_t x : v) sum += x;
  return sum;
}

// The combine's launch shape: a quad of lanes per GLV term over one-wave blocks (k_combine_q) when
// that still leaves at most one wave per SIMD (an epoch shard), else one lane per term in one block
// per proposer (k_combine, the only one that reads the window tables).
static bool combine_quads(const hbx_ctx* c, uint32_t t, uint32_t p) {
  const uint32_t nb = (2 * t + COMBQ_TERMS - 1) / COMBQ_TERMS;
  return c->combine_lanes == 4 ? nb <= 16
         : c->combine_lanes == 1 ? false
                                 : nb <= 16 && (size_t)nb * p <= FILL_WAVES;
}

// Senders per proposer whose window tables the fused epoch call precomputes (0: none): the first
// t valid senders lie below t + margin unless more than `margin` of them are invalid.  The default
// margin rounds t + 32 up to a whole wave of lanes.
static uint32_t combine_tab_cap(const hbx_ctx* c, uint32_t n, uint32_t t, uint32_t p) {
  if (c->comb_margin == HBX_COMBINE_TABLES_OFF || combine_quads(c, t, p)) return 0;
  const uint64_t want = c->comb_margin >= 0 ? (uint64_t)t + (uint32_t)c->comb_margin : ((uint64_t)t + 32 + 63) / 64 * 64;
  return (uint32_t)std::min<uint64_t>(n, want);
}

int hbx_set_batch_verify(hbx_ctx* c, const uint8_t* seed32) {
  if (!c) return HBX_E_INVALID_ARG;
  HBX_DEVICE(c);
  HIPCHK(c, quiesce(c));  // a verification enqueued earlier may still read the old seed
  c->batch_call = 0;
  c->batch_on = false;
  if (!seed32) return HBX_OK;
  if (!c->b_seed.ensure(32)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_set_batch_verify: out of device memory");
  HIPCHK(c, hipMemcpy(c->b_seed.p, seed32, 32, hipMemcpyHostToDevice));
  c->batch_on = true;
  return HBX_OK;
}

int hbx_get_batch_stats(hbx_ctx* c, uint32_t* cols_batched, uint32_t* cols_fallback, uint32_t* cols_skipped) {
  if (!c) return HBX_E_INVALID_ARG;
  uint32_t v[3] = {0, 0, 0};
  if (c->batch_last_p) {
    HBX_DEVICE(c);
    HIPCHK(c, quiesce(c));
    HIPCHK(c, hipMemcpy(v, c->b_stats.p, 12, hipMemcpyDeviceToHost));
  }
  if (cols_batched) *cols_batched = v[0];
  if (cols_fallback) *cols_fallback = v[1];
  if (cols_skipped) *cols_skipped = v[2];
  return HBX_OK;
}

int hbx_get_batch_sums(hbx_ctx* c, uint8_t* a48, size_t count) {
  if (!c || !a48) return fail(c, HBX_E_INVALID_ARG, "hbx_get_batch_sums: bad args");
  if (c->batch_last_p == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "hbx_get_batch_sums: the last verification was not batched");
  if (count != c->batch_last_p)
    return fail(c, HBX_E_INVALID_ARG, "hbx_get_batch_sums: count %zu, expected %u", count, c->batch_last_p);
  HBX_DEVICE(c);
  HIPCHK(c, quiesce(c));
  dbuf out;
  if (!out.ensure(count * 48)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_get_batch_sums: out of device memory");
  hipLaunchKernelGGL(k_batch_compress, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, c->stream, c->b_Asum.as<g1a>(),
                     (uint32_t)count, out.as<uint8_t>());
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(a48, out.p, count * 48, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, HBX_E_DEVICE, "hbx_get_batch_sums: %s", hipGetErrorString(e));
  return HBX_OK;
}

int hbx_set_combine_lanes(hbx_ctx* c, int lanes) {
  if (!c || (lanes != 0 && lanes != 1 && lanes != 4))
    return fail(c, HBX_E_INVALID_ARG, "hbx_set_combine_lanes: 0 (auto), 1 or 4, not %d", lanes);
  c->combine_lanes = lanes;
  return HBX_OK;
}

int hbx_set_merkle_digest(hbx_ctx* c, int variant) {
  if (!c || (variant != HBX_MERKLE_SHA256 && variant != HBX_MERKLE_SHA3))
    return fail(c, HBX_E_INVALID_ARG, "hbx_set_merkle_digest: unknown variant %d", variant);
  c->merkle = variant;
  c->bc_live = false;  // the held Echo values were validated under the previous digest
  return HBX_OK;
}

int hbx_set_pk_shares(hbx_ctx* c, const uint8_t* pk_comp, uint32_t n, int32_t* status) {
  if (!c || (!pk_comp && n)) return fail(c, HBX_E_INVALID_ARG, "hbx_set_pk_shares: bad args");
  HBX_DEVICE(c);
  // era change: nothing enqueued earlier (on any stream) may still read the old keys, and every
  // state derived from them is void -- the own share (its pk_me check was against the old keys)
  // and the current epoch's prepared ciphertexts / verified shares
  HIPCHK(c, quiesce(c));
  stream_scope ss_{c, pick(c, c->stream)};
  c->own_me = UINT32_MAX;
  c->own_ready = false;
  c->p_ct = 0;
  c->invalidate_epoch();
  c->coin_n = 0;
  c->coin_live = false;
  if (!c->pk.ensure((size_t)n * sizeof(g1a)) || !c->pk_m.ensure((size_t)n * sizeof(g1a)) ||
      !c->pk64.ensure((size_t)n * sizeof(g1a)) || !c->pk_status.ensure((size_t)n * 4) || !c->pk_comp.ensure((size_t)n * 48))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_set_pk_shares: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->pk_comp.p, pk_comp, (size_t)n * 48, hipMemcpyHostToDevice, c->stream));
  if (n) {
    hipLaunchKernelGGL(k_decompress_g1, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->pk_comp.as<uint8_t>(),
                       n, c->pk.as<g1a>(), c->pk_status.as<int32_t>());
    HIPCHK(c, hipGetLastError());
    // [3(x^2-1)] pk_i: the decryption-share checks' G1 side against H' = h_eff P (k_prepare_ct)
    hipLaunchKernelGGL(k_scale_keys, dim3((n + 63) / 64), dim3(64), 0, c->stream, c->pk.as<g1a>(), n,
                       c->pk_m.as<g1a>(), c->pk64.as<g1a>());
    HIPCHK(c, hipGetLastError());
    // [d 16^w] pk_i for the coin combine's master identity (k_combine_sigs): era set-up, not per round
    if (!c->g1tab.ensure((size_t)n * G1TAB_W * G1TAB_D * sizeof(g1a)))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_set_pk_shares: out of device memory (key tables)");
    hipLaunchKernelGGL(k_g1_tables, dim3((n * G1TAB_W + 63) / 64), dim3(64), 0, c->stream, c->pk.as<g1a>(), n,
                       c->g1tab.as<g1a>());
    HIPCHK(c, hipGetLastError());
  } else {
    c->g1tab.release();  // no tables of an older key set
  }
  std::vector<int32_t> st(n);
  HIPCHK(c, hipMemcpyAsync(st.data(), c->pk_status.p, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (status) memcpy(status, st.data(), (size_t)n * 4);
  c->n_keys = n;
  return HBX_OK;
}

int hbx_set_own_share(hbx_ctx* c, uint32_t me, const uint8_t* sk32) {
  if (!c) return HBX_E_INVALID_ARG;
  if (!sk32) {  // clear: back to separate Ciphertext::verify checks
    c->own_me = UINT32_MAX;
    c->own_ready = false;
    return HBX_OK;
  }
  if (c->n_keys == 0 || me >= c->n_keys) return fail(c, HBX_E_NO_KEYS, "hbx_set_own_share: me=%u, n=%u", me, c->n_keys);
  static const uint8_t ZERO[32] = {0};
  if (!scalars_canonical(sk32, 1) || memcmp(sk32, ZERO, 32) == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_set_own_share: scalar must be in [1, r)");
  // the secret share must match pk_me: the fused ciphertext check relies on pk_me = sk_me g1
  uint8_t pk48[48], want[48];
  int rc = hbx_public_keys(c, sk32, 1, pk48);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy(want, static_cast<uint8_t*>(c->pk_comp.p) + (size_t)me * 48, 48, hipMemcpyDeviceToHost));
  if (memcmp(pk48, want, 48) != 0) return fail(c, HBX_E_INVALID_ARG, "hbx_set_own_share: sk does not match pk[%u]", me);
  uint32_t limbs[8];
  for (int q = 0; q < 8; q++)
    limbs[q] = ((uint32_t)sk32[31 - 4 * q - 3] << 24) | ((uint32_t)sk32[31 - 4 * q - 2] << 16) |
               ((uint32_t)sk32[31 - 4 * q - 1] << 8) | sk32[31 - 4 * q];
  if (!c->own_sk.ensure(32)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_set_own_share: out of device memory");
  // a prepare enqueued earlier on any stream may still read own_sk
  HIPCHK(c, quiesce(c));
  HIPCHK(c, hipMemcpy(c->own_sk.p, limbs, 32, hipMemcpyHostToDevice));
  c->own_me = me;
  c->own_ready = false;
  return HBX_OK;
}

// The k_prepare_ct launch: the hash groups (H'_j, Jacobian, into Hj), the decode of U_j and W_j
// (U, G2pts, dec_st) and, in own-share mode, the halves of sk_me U_j; with `early_shares` the epoch's
// received shares are decoded beside them.  The caller has sized U, G2pts, Hj and dec_st for p
// ciphertexts (and S / S_status for the early shares).  Shared by prepare_impl and the pair-lane
// Ciphertext::verify of hbx_sk_decrypt, which needs none of prepare_impl's line tables.
static int launch_prepare_ct(hbx_ctx* c, hipStream_t s, const uint8_t* d_u_comp, const uint8_t* d_v_blob,
                             const uint64_t* d_v_off, const uint8_t* d_w_comp, uint32_t p, const uint8_t* early_shares,
                             size_t m_early, uint32_t early_n, uint32_t me_early) {
  const dim3 b64(64);
  const bool own = c->own_me != UINT32_MAX;
  {
    timed t_(c, HBX_K_PREPARE_CT, s);
    const uint32_t hash_blocks = (uint32_t)(((size_t)p * HASH_K + 63) / 64);
    const uint32_t dec_blocks = (own ? 4 : 2) * ((p + 63) / 64);  // wave-aligned parts (k_prepare_ct)
    const uint32_t share_blocks = (uint32_t)((m_early + 63) / 64);
    if (own && (!c->own_S.ensure((size_t)p * sizeof(g1a)) || !c->own_part.ensure((size_t)2 * p * sizeof(g1j))))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_prepare_ciphertexts_d: out of device memory");
    // HBX_SPLIT_PREP=1 (profiling): the hash part and the decode parts as two launches, so a
    // kernel trace times each chain on its own
    static const bool split = getenv("HBX_SPLIT_PREP") != nullptr;
    const uint32_t parts = split ? 2 : 1;
    for (uint32_t q = 0; q < parts; q++) {
      const uint32_t b0 = split && q == 1 ? hash_blocks : 0;
      const uint32_t nb = split ? (q == 0 ? hash_blocks : dec_blocks + share_blocks)
                                : hash_blocks + dec_blocks + share_blocks;
      hipLaunchKernelGGL(k_prepare_ct, dim3(nb), b64, 0, s, d_u_comp, d_v_blob, d_v_off, d_w_comp, p, hash_blocks,
                         c->U.as<g1a>(), c->G2pts.as<g2a>(), c->dec_st.as<int32_t>(),
                         own ? c->own_sk.as<uint32_t>() : nullptr, own ? c->own_part.as<g1j>() : nullptr, c->Hj.as<g2j>(), c->digest,
                         b0, dec_blocks, early_shares, m_early, early_n ? early_n : 1u, me_early, c->S.as<g1a>(),
                         c->S_status.as<int32_t>());
    }
    c->own_ready = own;
  }
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// Ciphertext preparation; with `early_shares` (the fused epoch call) the received shares of the
// epoch are decoded in the same launch, in waves beside the hash chains.
static int prepare_impl(hbx_ctx* c, const uint8_t* d_u_comp, const uint8_t* d_v_blob, const uint64_t* d_v_off,
                        const uint8_t* d_w_comp, uint32_t p, uint64_t max_v_len, uint8_t* d_ct_valid,
                        void* stream, const uint8_t* early_shares, uint32_t early_n, uint32_t tab_cap = 0) {
  if (!c || p == 0 || !d_u_comp || !d_v_off || !d_w_comp)
    return fail(c, HBX_E_INVALID_ARG, "hbx_prepare_ciphertexts_d: bad args");
  HBX_ENTER(c, stream);
  if (!c->U.ensure((size_t)p * sizeof(g1a)) || !c->G2pts.ensure((size_t)2 * p * sizeof(g2a)) || !c->Hj.ensure((size_t)p * sizeof(g2j)) ||
      !c->lines.ensure((size_t)p * sizeof(line_block)) || !c->lines_d.ensure((size_t)p * sizeof(line_block_d)) ||
      !c->lines_u.ensure((size_t)p * sizeof(line_block_d)) || !c->line_degen.ensure(p) ||
      !c->scratch.ensure((size_t)2 * p * MILLER_LINES * sizeof(fq2d)) || !c->ct_ok.ensure(p) ||
      !c->ct_valid.ensure(p) || !c->dec_st.ensure((size_t)2 * p * 4))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_prepare_ciphertexts_d: out of device memory");
  const size_t m_early = early_shares ? (size_t)early_n * p : 0;
  if (m_early && (!c->S.ensure(m_early * sizeof(g1a)) || !c->S_status.ensure(m_early * 4)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_prepare_ciphertexts_d: out of device memory");
  // What the table lanes precompute (g1d.hpp g1d_tab_stride): HBX_COMB_FORM=0..3 (profiling)
  // overrides the default; DESIGN.md section 5 records what each form measured.
  static const char* form_env = getenv("HBX_COMB_FORM");
  const uint32_t form = form_env && form_env[0] >= '0' && form_env[0] <= '3' ? (uint32_t)(form_env[0] - '0') : COMB_FORM;
  c->tab_ready = false;
  if (!m_early) tab_cap = 0;
  if (tab_cap && (!c->comb_tab.ensure((size_t)p * (tab_cap + 1) * g1d_tab_stride(form) * sizeof(g1jd)) ||
                  !c->comb_tab_ok.ensure((size_t)p * (tab_cap + 1))))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_decrypt_epoch_d: out of device memory for the combine's tables");
  const dim3 b64(64);
  const bool own = c->own_me != UINT32_MAX;
  // own entry of the early-decoded matrix (written by k_prepare_lines), as hbx_verify_dec_shares_d
  const uint32_t me_early = (own && c->own_me < early_n) ? c->own_me : UINT32_MAX;
  if (int rc = launch_prepare_ct(c, s, d_u_comp, d_v_blob, d_v_off, d_w_comp, p, early_shares, m_early, early_n, me_early))
    return rc;
  {
    timed t_(c, HBX_K_PREPARE_LINES, s);
    const uint32_t line_blocks = (2 * p * LINE_K + 63) / 64, own_blocks = own ? (p + 63) / 64 : 0;
    const bool own_entry = m_early && me_early != UINT32_MAX;
    // the combine's window tables in further blocks of this launch (k_prepare_lines): with the
    // default cap at N = 256, 512 waves beside the 128 line waves and the own-share waves, still
    // at most one wave per SIMD
    const uint32_t tab_blocks =
        tab_cap ? (form == 2 ? 2 : 1) * ((own_entry ? own_blocks : 0) + (uint32_t)(((size_t)p * tab_cap + 63) / 64)) : 0;
    // grouped addition steps (g2_raw_lines_group<true>) at every size: since the group rounds pick
    // their operands by blocks (groupd.hpp gd_round) the grouped kernel is the faster one at N=256
    // too (lines 1.00 -> 0.85 ms, epoch 23.43 -> 23.27 ms averaged over two runs each), and two
    // epochs in flight stay within the runs' spread (22.7-23.4 ms per epoch either way).  Round 3
    // had kept it to launches below a full chip: its register footprint then slowed two epochs in
    // flight 28.2 -> 32.5 ms per epoch (profiles/r03n_bisect_*).
    auto kpl = k_prepare_lines<true>;
    hipLaunchKernelGGL(kpl, dim3(line_blocks + own_blocks + tab_blocks), b64, 0, s, c->G2pts.as<g2a>(), 2 * p,
                       c->lines_d.as<line_pre_d>(), c->scratch.as<fq2d>(), c->dec_st.as<int32_t>(), p,
                       c->ct_ok.as<uint8_t>(), own ? c->own_part.as<g1j>() : nullptr,
                       own ? c->own_S.as<g1a>() : nullptr, early_n, me_early,
                       own_entry ? c->S.as<g1a>() : nullptr, own_entry ? c->S_status.as<int32_t>() : nullptr,
                       c->Hj.as<g2j>(), c->S.as<g1a>(), c->S_status.as<int32_t>(),
                       tab_cap ? c->comb_tab.as<g1jd>() : nullptr, c->comb_tab_ok.as<uint8_t>(), tab_cap, form);
    HIPCHK(c, hipGetLastError());
    const uint32_t nl = 2 * p * MILLER_LINES;
    HIPCHK(c, hipMemsetAsync(c->line_degen.p, 0, p, s));
    hipLaunchKernelGGL(k_normalise_lines, dim3((nl + 63) / 64), b64, 0, s, c->lines.as<line_pre>(),
                       c->scratch.as<fq2d>(), nl, c->lines_d.as<line_pre_d>(), c->G2pts.as<g2a>(),
                       c->Hj.as<g2j>(), c->lines_u.as<line_pre_d>(), c->line_degen.as<uint8_t>());
  }
  HIPCHK(c, hipGetLastError());
  c->p_ct = p;
  c->invalidate_epoch();
  c->tab_ready = tab_cap != 0;  // this call's tables, if it made any
  c->tab_cap = tab_cap;
  c->tab_me = me_early;
  c->tab_n = early_n;
  c->tab_p = p;
  c->tab_form = form;
  if (d_ct_valid) {
    // Ciphertext::verify now: one check per proposer (n = 0 share jobs, job 0 = the ciphertext)
    if (!c->S.ensure(sizeof(g1a)) || !c->S_status.ensure(4) || !c->valid.ensure(16))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_prepare_ciphertexts_d: out of device memory");
    int rc = launch_pair_checks(c, s, 0, p, 0, 0, nullptr, c->ct_ok.as<uint8_t>());
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(d_ct_valid, c->ct_valid.p, p, hipMemcpyDeviceToDevice, s));
    c->ct_known = true;
  }
  c->d_v_blob = d_v_blob;
  c->d_v_off = d_v_off;
  c->max_v_len = max_v_len;
  return HBX_OK;
}

int hbx_prepare_ciphertexts_d(hbx_ctx* c, const uint8_t* d_u_comp, const uint8_t* d_v_blob,
                              const uint64_t* d_v_off, const uint8_t* d_w_comp, uint32_t p,
                              uint64_t max_v_len, uint8_t* d_ct_valid, void* stream) {
  return prepare_impl(c, d_u_comp, d_v_blob, d_v_off, d_w_comp, p, max_v_len, d_ct_valid, stream, nullptr, 0);
}

int hbx_prepare_ciphertexts(hbx_ctx* c, const uint8_t* u_comp, const uint8_t* v_blob, const uint64_t* v_off,
                            const uint8_t* w_comp, uint32_t p, uint8_t* ct_valid_bits) {
  if (!c || p == 0 || !u_comp || !v_off || !w_comp)
    return fail(c, HBX_E_INVALID_ARG, "hbx_prepare_ciphertexts: bad args");
  HBX_ENTER(c, c->stream);
  const uint64_t vbytes = v_off[p];
  uint64_t maxv = 0;
  for (uint32_t j = 0; j < p; j++) {
    if (v_off[j + 1] < v_off[j]) return fail(c, HBX_E_INVALID_ARG, "v_off not monotone");
    maxv = std::max<uint64_t>(maxv, v_off[j + 1] - v_off[j]);
  }
  if (!c->u_comp_own.ensure((size_t)p * 48) || !c->w_comp_own.ensure((size_t)p * 96) ||
      !c->v_off_own.ensure((size_t)(p + 1) * 8) || !c->v_blob_own.ensure(vbytes ? vbytes : 16))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_prepare_ciphertexts: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->u_comp_own.p, u_comp, (size_t)p * 48, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->w_comp_own.p, w_comp, (size_t)p * 96, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->v_off_own.p, v_off, (size_t)(p + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (vbytes) HIPCHK(c, hipMemcpyAsync(c->v_blob_own.p, v_blob, vbytes, hipMemcpyHostToDevice, c->stream));
  if (!c->ct_valid.ensure(p)) return fail(c, HBX_E_OUT_OF_MEMORY, "out of device memory");
  int rc = hbx_prepare_ciphertexts_d(c, c->u_comp_own.as<uint8_t>(), c->v_blob_own.as<uint8_t>(),
                                     c->v_off_own.as<uint64_t>(), c->w_comp_own.as<uint8_t>(), p, maxv,
                                     c->ct_valid.as<uint8_t>(), c->stream);
  if (rc) return rc;
  std::vector<uint8_t> ok(p);
  HIPCHK(c, hipMemcpyAsync(ok.data(), c->ct_valid.p, p, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (ct_valid_bits) pack_bits(ok.data(), p, ct_valid_bits);
  return HBX_OK;
}

// The share-check launch at `lanes` lanes per check (7: the one-lane check as one kernel) over
// `grid` blocks: the tiles (chunks, p) of a matrix verification (tiles = nullptr), or the listed
// tiles of an add, grid (T, 1) (addplan.hpp).  `me` / `ctv`: own-share mode's lane and where its
// verdict goes as Ciphertext::verify.
static int launch_share_checks(hbx_ctx* c, hipStream_t s, int lanes, dim3 grid, const uint2* tiles, const g1a* S,
                               const int32_t* S_status, const uint8_t* d_present, uint8_t* vd, const uint8_t* ctok,
                               uint32_t n, uint32_t me, uint8_t* ctv) {
  const size_t blocks = (size_t)grid.x * grid.y;
  c->fb_last = nullptr;  // set again below by the one-lane path, the only one with a fallback
  if (lanes == 2) {
    // global slots of the final exponentiation: 2 x 78 dwords per lane of the launch
    if (!c->gslot.ensure(blocks * 64 * 2 * LDS_FQ6D_PACKED * 4))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_dec_shares_d: out of device memory (slots)");
    hipLaunchKernelGGL(k_verify_shares2, grid, dim3(64), 0, s, S, S_status, d_present, c->pk_m.as<g1a>(), c->n_keys,
                       c->G2pts.as<g2a>(), c->lines_d.as<line_block_d>(), ctok, n, vd, me, ctv, c->gslot.as<uint32_t>(),
                       tiles);
  } else if (lanes == 6)
    hipLaunchKernelGGL(k_verify_shares6, grid, dim3(64), 0, s, S, S_status, d_present, c->pk_m.as<g1a>(), c->n_keys,
                       c->G2pts.as<g2a>(), c->lines_d.as<line_block_d>(), ctok, n, vd, me, ctv, 0u, tiles);
  else if (lanes == 3)
    hipLaunchKernelGGL(k_verify_shares3, grid, dim3(64), 0, s, S, S_status, d_present, c->pk_m.as<g1a>(), c->n_keys,
                       c->G2pts.as<g2a>(), c->lines_d.as<line_block_d>(), ctok, n, vd, me, ctv, tiles);
  else if (lanes == 7)  // the one-lane check as one kernel (final exponentiation through call frames)
    hipLaunchKernelGGL(k_verify_shares, grid, dim3(64), 0, s, S, S_status, d_present, c->pk_m.as<g1a>(), c->n_keys,
                       c->G2pts.as<g2a>(), c->lines_d.as<line_block_d>(), ctok, n, vd, me, ctv, 0u, nullptr, tiles);
  else {
    // one lane per check: the Miller loops, then the final exponentiation's seven steps as four
    // kernels over per-lane slots (fe1d.hpp: no Fq12 ever crosses a call frame)
    if (!c->fe1slot.ensure(blocks * 64 * 3 * FE1_WORDS * 4))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_dec_shares_d: out of device memory (slots)");
    uint32_t* gs = c->fe1slot.as<uint32_t>();
    if (!c->fb_lanes.ensure(4)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_dec_shares_d: out of device memory");
    HIPCHK(c, hipMemsetAsync(c->fb_lanes.p, 0, 4, s));
    c->fb_last = &c->fb_lanes;
    hipLaunchKernelGGL(k_verify_shares_ml, grid, dim3(64), 0, s, S, S_status, d_present, c->pk_m.as<g1a>(), c->n_keys,
                       c->G2pts.as<g2a>(), c->lines_d.as<line_block_d>(), ctok, n, vd, me, gs,
                       c->lines_u.as<line_block_d>(), c->line_degen.as<uint8_t>(), c->force_degen, tiles);
    hipLaunchKernelGGL(k_fe1<0>, grid, dim3(64), 0, s, gs, n, vd, ctok, me, ctv, c->force_fallback, tiles);
    hipLaunchKernelGGL(k_fe1<1>, grid, dim3(64), 0, s, gs, n, vd, ctok, me, ctv, c->force_fallback, tiles);  // F1 + F2
    hipLaunchKernelGGL(k_fe1<3>, grid, dim3(64), 0, s, gs, n, vd, ctok, me, ctv, c->force_fallback, tiles);  // F3 + F4
    hipLaunchKernelGGL(k_fe1<5>, grid, dim3(64), 0, s, gs, n, vd, ctok, me, ctv, c->force_fallback, tiles);  // F5 + F6
    // lanes whose compressed squarings met g3 = 0, and the lanes of a proposer with a line whose
    // constant term is 0 (neither ever expected): the single-kernel check
    hipLaunchKernelGGL(k_verify_shares, grid, dim3(64), 0, s, S, S_status, d_present, c->pk_m.as<g1a>(), c->n_keys,
                       c->G2pts.as<g2a>(), c->lines_d.as<line_block_d>(), ctok, n, vd, me, ctv, 1u,
                       c->fb_lanes.as<uint32_t>(), tiles);
  }
  return HBX_OK;
}

// Share checks of the prepared ciphertexts.  `predecoded`: the fused epoch call (hbx_decrypt_epoch_d)
// had prepare_impl decode exactly these shares into S / S_status already.
static int verify_impl(hbx_ctx* c, const uint8_t* d_shares, const uint8_t* d_present, uint32_t n, uint32_t p,
                       uint8_t* d_valid, void* stream, bool predecoded) {
  if (!c || !d_shares || n == 0 || p == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_verify_dec_shares_d: bad args");
  if (c->n_keys == 0) return fail(c, HBX_E_NO_KEYS, "hbx_set_pk_shares has not been called");
  if (p != c->p_ct) return fail(c, HBX_E_NO_CIPHERTEXTS, "p=%u but %u ciphertexts prepared", p, c->p_ct);
  HBX_ENTER(c, stream);
  const size_t m = (size_t)n * p;
  if (!c->S.ensure(m * sizeof(g1a)) || !c->S_status.ensure(m * 4) || !c->valid.ensure(m))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_dec_shares_d: out of device memory");
  // own-share mode: this node's share is the one computed in prepare, and its check IS
  // Ciphertext::verify (k_verify_shares); otherwise the ciphertext checks run separately
  const bool own = c->own_ready && c->own_me < n;
  if (!predecoded) {
    c->tab_ready = false;  // S is about to hold other shares than the tables were made from
    hipLaunchKernelGGL(k_decompress_shares, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, d_shares, m,
                       c->S.as<g1a>(), c->S_status.as<int32_t>(), n, own ? c->own_me : UINT32_MAX,
                       own ? c->own_S.as<g1a>() : nullptr);
    HIPCHK(c, hipGetLastError());
  }
  // batched mode: the column equations first; the launches below then see only the columns that
  // failed theirs (ctok), and k_batch_merge writes the others' statuses
  const bool batch = c->batch_on;
  const uint8_t* ctok = c->ct_ok.as<uint8_t>();
  if (batch) {
    int rc = launch_batch_columns(c, s, d_present, n, p, own, !c->ct_known && !own);
    if (rc) return rc;
    ctok = c->b_ctok.as<uint8_t>();
  }
  // ciphertext checks (if prepare deferred them): latency-bound, p checks -> 16-lane groups
  if (!c->ct_known && !own) {
    int rc = launch_pair_checks(c, s, n, p, n, n, d_present, ctok);
    if (rc) return rc;
    c->ct_known = true;
  }
  // share checks: one lane per check when the launch fills the chip (throughput), else six lanes
  // per check when that still leaves at most one wave per SIMD, else three (latency: an epoch
  // shard on one of several GPUs; pairing3.hpp / pairing3d.hpp).  The two-lane
  // check (no scratch) measured slower than the one-lane check at N=256 (26.6 vs 24.0 ms,
  // profiles/r03a_bench.json), so it is only used when asked for.
  {
    timed t_(c, HBX_K_VERIFY_SHARES, s);
    // below a full chip: the most lanes per check that still fit one wave per SIMD -- six, three,
    // then two (an N=256 epoch over 2 GPUs: 1,024 two-lane waves, 11.0 ms against 17.4 for the
    // three-lane check in two rounds of waves, profiles/r04w_lanes.txt)
    // (the ladder itself: addplan.hpp choose_lanes, over the whole matrix's tiles of each shape)
    namespace ap = hbx_addplan;
    auto tiles_of = [&](int shape) { return (size_t)((n + ap::SHAPE_SENDERS[shape] - 1) / ap::SHAPE_SENDERS[shape]) * p; };
    const int lanes =
        c->verify_lanes ? c->verify_lanes : ap::choose_lanes(tiles_of(0), tiles_of(3), tiles_of(2), tiles_of(1));
    c->lanes_used = lanes;
    const uint32_t per = ap::SHAPE_SENDERS[ap::shape_of_lanes(lanes)];
    c->verify_tiles = (uint32_t)((n + per - 1) / per) * p;
    if (int rc = launch_share_checks(c, s, lanes, dim3((n + per - 1) / per, p), nullptr, c->S.as<g1a>(),
                                     c->S_status.as<int32_t>(), d_present, c->valid.as<uint8_t>(), ctok, n,
                                     own ? c->own_me : UINT32_MAX,
                                     (own && !c->ct_known) ? c->ct_valid.as<uint8_t>() : nullptr))
      return rc;
  }
  HIPCHK(c, hipGetLastError());
  c->ct_known = true;
  if (batch) {
    hipLaunchKernelGGL(k_batch_merge, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, c->b_cls.as<uint8_t>(),
                       c->S_status.as<int32_t>(), d_present, n, p, c->n_keys, own ? c->own_me : UINT32_MAX,
                       c->valid.as<uint8_t>(), c->ct_valid.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    c->batch_call++;
  }
  c->batch_last_p = batch ? p : 0;
  hipLaunchKernelGGL(k_gate_by_ct, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, c->valid.as<uint8_t>(),
                     c->ct_valid.as<uint8_t>(), n, p);
  HIPCHK(c, hipGetLastError());
  if (d_valid) HIPCHK(c, hipMemcpyAsync(d_valid, c->valid.p, m, hipMemcpyDeviceToDevice, s));
  c->n_shares = n;
  c->verified_p = p;
  return HBX_OK;
}

int hbx_verify_dec_shares_d(hbx_ctx* c, const uint8_t* d_shares, const uint8_t* d_present, uint32_t n,
                            uint32_t p, uint8_t* d_valid, void* stream) {
  return verify_impl(c, d_shares, d_present, n, p, d_valid, stream, false);
}

int hbx_verify_dec_shares(hbx_ctx* c, const uint8_t* shares, const uint8_t* present_bits, uint32_t n,
                          uint32_t p, uint8_t* valid_bits) {
  if (!c || !shares || n == 0 || p == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_verify_dec_shares: bad args");
  HBX_ENTER(c, c->stream);
  const size_t m = (size_t)n * p;
  if (!c->shares_own.ensure(m * 48) || (present_bits && !c->present_own.ensure(m)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_dec_shares: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->shares_own.p, shares, m * 48, hipMemcpyHostToDevice, c->stream));
  std::vector<uint8_t> pres;
  if (present_bits) {
    pres.resize(m);
    for (size_t k = 0; k < m; k++) pres[k] = (present_bits[k >> 3] >> (k & 7)) & 1;
    HIPCHK(c, hipMemcpyAsync(c->present_own.p, pres.data(), m, hipMemcpyHostToDevice, c->stream));
  }
  int rc = hbx_verify_dec_shares_d(c, c->shares_own.as<uint8_t>(),
                                   present_bits ? c->present_own.as<uint8_t>() : nullptr, n, p, nullptr,
                                   c->stream);
  if (rc) return rc;
  std::vector<uint8_t> v(m);
  HIPCHK(c, hipMemcpyAsync(v.data(), c->valid.p, m, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (valid_bits) pack_bits(v.data(), m, valid_bits);
  return HBX_OK;
}

int hbx_rs_encode_d(hbx_ctx* c, uint8_t* d_shards, uint32_t inst, uint32_t k, uint32_t m, uint32_t L, void* stream) {
  if (!c || !d_shards || inst == 0 || L == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_rs_encode_d: bad args");
  HBX_ENTER(c, stream);
  if (m == 0) return HBX_OK;  // Coding::Trivial
  int rc = rs_setup(c, k, m, s);
  if (rc) return rc;
  rs_code(c, d_shards, (size_t)(k + m) * L, L, k, inst, c->rs_enc_job.as<rs_job>(), c->rs_enc_coef.as<uint16_t>(),
          c->rs_enc_ptab.as<gf_ptab>(), 0u, m, s);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

int hbx_rs_reconstruct_d(hbx_ctx* c, uint8_t* d_shards, const uint8_t* d_present, uint32_t inst, uint32_t k,
                         uint32_t m, uint32_t L, int32_t* d_status, void* stream) {
  if (!c || !d_shards || !d_present || !d_status || inst == 0 || L == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_rs_reconstruct_d: bad args");
  HBX_ENTER(c, stream);
  int rc = rs_setup(c, k, m, s);
  if (rc) return rc;
  return rs_reconstruct(c, d_shards, d_present, inst, k, m, L, d_status, s);
}

int hbx_merkle_roots_d(hbx_ctx* c, const uint8_t* d_shards, uint32_t inst, uint32_t n, uint32_t L, uint8_t* d_roots,
                       void* stream) {
  if (!c || !d_shards || !d_roots || inst == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_roots_d: bad args");
  HBX_ENTER(c, stream);
  return merkle_roots(c, d_shards, inst, n, L, d_roots, s);
}

int hbx_merkle_validate_d(hbx_ctx* c, const uint8_t* d_values, uint32_t vlen, const uint8_t* d_node_hash,
                          const uint8_t* d_sib_hash, const uint32_t* d_sides, const uint32_t* d_depth,
                          const uint8_t* d_root, const uint32_t* d_sender, uint32_t count, uint32_t nproofs,
                          uint8_t* d_valid, void* stream) {
  if (!c || !d_values || !d_node_hash || !d_sib_hash || !d_sides || !d_depth || !d_root || !d_sender || !d_valid ||
      nproofs == 0 || vlen == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_validate_d: bad args");
  HBX_ENTER(c, stream);
  // long values (Echo proofs of real shards): their leaf digests first, by the leaf kernels (the
  // producer/consumer SHA-256 or the two-lane SHA3 schedule) instead of one lane per value inside
  // the path check
  const uint32_t* vdigest = nullptr;
  if (vlen > 256) {
    if (!c->val_digest.ensure((size_t)nproofs * 32))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_merkle_validate_d: out of device memory");
    leaf_digests(c, s, k_merkle_leaves_sha256, k_merkle_leaves_sha3, nproofs, 1u, d_values + 1, (size_t)0, nproofs,
                 vlen - 1, c->val_digest.as<uint32_t>(), (const uint16_t*)nullptr, 0u, vlen);
    HIPCHK(c, hipGetLastError());
    vdigest = c->val_digest.as<uint32_t>();
  }
  hipLaunchKernelGGL(k_merkle_validate, dim3((nproofs + 63) / 64), dim3(64), 0, s, d_values, vlen,
                     d_node_hash, d_sib_hash, d_sides, d_depth, d_root, d_sender, count, nproofs, d_valid, c->merkle,
                     vdigest);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

uint32_t hbx_merkle_node_count(uint32_t n) { return n ? merkle_node_count(n) : 0; }

int hbx_merkle_build_d(hbx_ctx* c, const uint8_t* d_shards, uint32_t inst, uint32_t n, uint32_t L, uint8_t* d_nodes,
                       uint8_t* d_roots, void* stream) {
  if (!c || !d_shards || !d_nodes || inst == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_build_d: bad args");
  HBX_ENTER(c, stream);
  uint8_t* roots = d_roots;
  if (!roots) {
    if (!c->roots.ensure((size_t)inst * 32)) return fail(c, HBX_E_OUT_OF_MEMORY, "merkle: roots");
    roots = c->roots.as<uint8_t>();
  }
  return merkle_roots(c, d_shards, inst, n, L, roots, s, d_nodes);
}

int hbx_merkle_proofs_d(hbx_ctx* c, const uint8_t* d_nodes, uint32_t n, const uint32_t* d_req, uint32_t count,
                        uint8_t* d_node_hash, uint8_t* d_sib_hash, uint32_t* d_sides, uint32_t* d_depth,
                        uint8_t* d_root, void* stream) {
  if (!c || !d_nodes || !d_req || !d_node_hash || !d_sib_hash || !d_sides || !d_depth || !d_root || count == 0 ||
      n == 0 || n > (uint32_t)RS_MAX_N)
    return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_proofs_d: bad args");
  HBX_ENTER(c, stream);
  hipLaunchKernelGGL(k_merkle_proofs, dim3((count + 63) / 64), dim3(64), 0, s, d_nodes, n, d_req, count,
                     d_node_hash, d_sib_hash, d_sides, d_depth, d_root);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// decode_from_shards + glue for `inst` instances of uniform rows.
static int broadcast_decode(hbx_ctx* c, uint8_t* d_shards, const uint8_t* d_present, const uint8_t* d_leaf_hash,
                            const uint8_t* d_root_expect, uint32_t inst, uint32_t k, uint32_t m, uint32_t L,
                            uint8_t* d_out, uint64_t out_stride, uint64_t* d_out_len, int32_t* d_status, void* stream) {
  if (!c || !d_shards || !d_present || !d_root_expect || !d_out || !d_out_len || !d_status || inst == 0 || L == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_broadcast_decode_d: bad args");
  // the payload length comes from the (untrusted) big-endian header: k L - 4 bytes is the most
  // glue_shards can take, so every output row must hold that many
  if ((uint64_t)k * L >= 4 && out_stride < (uint64_t)k * L - 4)
    return fail(c, HBX_E_INVALID_ARG, "hbx_broadcast_decode_d: out_stride %llu < k L - 4 = %llu",
                (unsigned long long)out_stride, (unsigned long long)((uint64_t)k * L - 4));
  HBX_ENTER(c, stream);
  int rc = rs_setup(c, k, m, s);
  if (rc) return rc;
  rc = rs_reconstruct(c, d_shards, d_present, inst, k, m, L, d_status, s);
  if (rc) return rc;
  const uint32_t n = k + m;
  const dim3 glue_grid((unsigned)(((uint64_t)k * L + 4095) / 4096), inst);
  return decode_tail(
      c, d_present, d_leaf_hash, d_root_expect, inst, n, m, d_status, s,
      [&](const uint16_t* slots, uint32_t nslots) { leaves_uniform(c, s, d_shards, inst, n, L, slots, nslots); },
      [&] { hipLaunchKernelGGL(k_glue, glue_grid, dim3(256), 0, s, d_shards, (size_t)n * L, k, L, d_out,
                               (size_t)out_stride, d_out_len, d_status); });
}

int hbx_broadcast_decode_d(hbx_ctx* c, uint8_t* d_shards, const uint8_t* d_present, const uint8_t* d_root_expect,
                           uint32_t inst, uint32_t k, uint32_t m, uint32_t L, uint8_t* d_out, uint64_t out_stride,
                           uint64_t* d_out_len, int32_t* d_status, void* stream) {
  return broadcast_decode(c, d_shards, d_present, nullptr, d_root_expect, inst, k, m, L, d_out, out_stride, d_out_len,
                          d_status, stream);
}

int hbx_broadcast_decode_leaves_d(hbx_ctx* c, uint8_t* d_shards, const uint8_t* d_present, const uint8_t* d_leaf_hash,
                                  const uint8_t* d_root_expect, uint32_t inst, uint32_t k, uint32_t m, uint32_t L,
                                  uint8_t* d_out, uint64_t out_stride, uint64_t* d_out_len, int32_t* d_status,
                                  void* stream) {
  if (!d_leaf_hash) return fail(c, HBX_E_INVALID_ARG, "hbx_broadcast_decode_leaves_d: d_leaf_hash is NULL");
  return broadcast_decode(c, d_shards, d_present, d_leaf_hash, d_root_expect, inst, k, m, L, d_out, out_stride,
                          d_out_len, d_status, stream);
}

// Every listed index is below `bound` and listed once (before anything is launched); `name` is the
// caller's array, `noun` what an entry of it names.
static int list_check(hbx_ctx* c, const char* fn, const char* name, const uint32_t* idx, uint32_t count, uint32_t bound,
                      const char* noun) {
  std::vector<uint8_t> seen(bound, 0);
  for (uint32_t k = 0; k < count; k++) {
    if (idx[k] >= bound || seen[idx[k]])
      return fail(c, HBX_E_INVALID_ARG, "%s: %s[%u] = %u is %s%s", fn, name, k, idx[k],
                  idx[k] >= bound ? "not a prepared " : "listed twice", idx[k] >= bound ? noun : "");
    seen[idx[k]] = 1;
  }
  return HBX_OK;
}

// ---- the incremental adds' common host steps (hbx_add_dec_shares_d, hbx_add_sig_shares_d) -------
// What addplan's build() refused, as entry point `fn`'s error; `row` = what an item's first index
// names, `row_bound` = the text for one that is not below `rows` (one %u).
static int add_plan_rejected(hbx_ctx* c, int plan_rc, const char* fn, const char* row, const char* row_bound,
                             uint32_t rows, uint32_t me) {
  char text[96];
  switch (plan_rc) {
    case hbx_addplan::PLAN_BAD_PROPOSER:
      snprintf(text, sizeof text, row_bound, rows);
      return fail(c, HBX_E_INVALID_ARG, "%s: %s", fn, text);
    case hbx_addplan::PLAN_DUPLICATE:
      return fail(c, HBX_E_INVALID_ARG, "%s: the same (%s, sender) twice in one call", fn, row);
    case hbx_addplan::PLAN_OWN_SENDER:
      return fail(c, HBX_E_INVALID_ARG, "%s: sender %u is this node (own-share mode)", fn, me);
    default:
      return HBX_OK;
  }
}

// An add's items as (row, sender) pairs and the tile list of the chosen shape, into the pinned
// staging and up in one copy on `s`: the caller's arrays are consumed before the call returns.
static int add_stage(hbx_ctx* c, const char* fn, const uint32_t* row, const uint32_t* sender, uint32_t count,
                     const std::vector<hbx_addplan::tile>& tiles, hipStream_t s, const uint2** d_items,
                     const uint2** d_tiles) {
  const size_t tiles_bytes = tiles.size() * sizeof(uint2);
  staging st(c, {(size_t)count * sizeof(uint2), tiles_bytes});
  if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "%s: out of memory (staging)", fn);
  uint2* it = st.host<uint2>(0);
  for (uint32_t k = 0; k < count; k++) it[k] = make_uint2(row[k], sender[k]);
  if (tiles_bytes) memcpy(st.host<uint2>(1), tiles.data(), tiles_bytes);
  if (int rc = st.upload(s)) return rc;
  *d_items = st.dev<uint2>(0);
  *d_tiles = st.dev<uint2>(1);
  return HBX_OK;
}

// The host form of an add, on the context's stream: the items' bytes (`width` each) up into the
// add state's `in`, the _d form `add_d` with its statuses into `out`, those read back; synchronised
// at return.
static int add_host(hbx_ctx* c, const char* fn, add_state hbx_ctx::*state, size_t width,
                    decltype(&hbx_add_dec_shares_d) add_d, const uint8_t* bytes, const uint32_t* row,
                    const uint32_t* sender, uint32_t count, uint32_t n, uint8_t* status) {
  if (!c || n == 0 || (count && (!bytes || !row || !sender))) return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  HBX_ENTER(c, c->stream);
  add_state& a = c->*state;
  if (!a.in.ensure((size_t)count * width) || !a.out.ensure(count))
    return fail(c, HBX_E_OUT_OF_MEMORY, "%s: out of device memory", fn);
  if (count) HIPCHK(c, hipMemcpyAsync(a.in.p, bytes, (size_t)count * width, hipMemcpyHostToDevice, c->stream));
  if (int rc = add_d(c, a.in.as<uint8_t>(), row, sender, count, n, a.out.as<uint8_t>(), c->stream)) return rc;
  std::vector<uint8_t> st(count);
  if (count) HIPCHK(c, hipMemcpyAsync(st.data(), a.out.p, count, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (status && count) memcpy(status, st.data(), count);
  return HBX_OK;
}

// ---- Broadcast, ragged forms (include/hbx.h): per-instance shard lengths in one call -----------
// The descriptor rules (bcplan.hpp check_rows) as entry point `fn`'s error; max_len = the longest shard.
static int rg_check(hbx_ctx* c, const char* fn, uint64_t buf_bytes, const uint64_t* off, const uint32_t* len,
                    const uint32_t* pitch, uint32_t inst, uint32_t n, uint32_t* max_len) {
  if (!off || !len || !pitch || inst == 0 || n == 0) return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  uint32_t bad[2] = {0, 0};
  const uint32_t& q = bad[0];
  switch (hbx_bcplan::check_rows(buf_bytes, off, len, pitch, inst, n, max_len, bad)) {
    case hbx_bcplan::ROWS_UNALIGNED:
      return fail(c, HBX_E_INVALID_ARG, "%s: instance %u: off %llu and pitch %u must be multiples of 4", fn, q,
                  (unsigned long long)off[q], pitch[q]);
    case hbx_bcplan::ROWS_BAD_LEN:
      return fail(c, HBX_E_INVALID_ARG, "%s: instance %u: need pitch %u >= len %u >= 1", fn, q, pitch[q], len[q]);
    case hbx_bcplan::ROWS_PAST_END:
      return fail(c, HBX_E_INVALID_ARG, "%s: instance %u: rows [%llu, +%u x %u) end past the buffer (%llu bytes)", fn, q,
                  (unsigned long long)off[q], n, pitch[q], (unsigned long long)buf_bytes);
    case hbx_bcplan::ROWS_OVERLAP:
      return fail(c, HBX_E_INVALID_ARG, "%s: instances %u and %u overlap", fn, bad[0], bad[1]);
    default:
      return HBX_OK;
  }
}

static int bc_plan_rejected(hbx_ctx* c, int rc, const char* fn) {
  switch (rc) {
    case hbx_bcplan::PLAN_BAD_INST:
      return fail(c, HBX_E_INVALID_ARG, "%s: an instance is not below the store's %u", fn, c->bc_inst);
    case hbx_bcplan::PLAN_BAD_SENDER:
      return fail(c, HBX_E_INVALID_ARG, "%s: a sender is not below n = %u", fn, c->bc_k + c->bc_m);
    case hbx_bcplan::PLAN_DUPLICATE:
      return fail(c, HBX_E_INVALID_ARG, "%s: the same entry twice in one call", fn);
    case hbx_bcplan::PLAN_BAD_OFFSETS:
      return fail(c, HBX_E_INVALID_ARG, "%s: val_off is not a non-decreasing offset list within the values", fn);
    case hbx_bcplan::PLAN_BAD_LEN:
      return fail(c, HBX_E_INVALID_ARG, "%s: need 1 <= len <= max_shard_len = %u", fn, c->bc_max);
    case hbx_bcplan::PLAN_NO_ROOM:
      return fail(c, HBX_E_INVALID_ARG, "%s: an attempt has no room of its own for k len - 4 output bytes", fn);
    default:
      return HBX_OK;
  }
}

// The descriptors into range 0 of the call's staging, and the staging up.
static int rg_upload(const staging& st, const uint64_t* off, const uint32_t* len, const uint32_t* pitch, uint32_t inst,
                     hipStream_t s) {
  rg_desc* d = st.host<rg_desc>(0);
  for (uint32_t q = 0; q < inst; q++) d[q] = rg_desc{off[q], len[q], pitch[q]};
  return st.upload(s);
}

// One ragged coding pass: the triple byte-permute kernel, tiled by output count as rs_code tiles it
// (rows are dword rows by construction, so the LDS log/exp byte kernel has no part here).
static void rs_code_rg(hbx_ctx* c, uint8_t* d_buf, const rg_desc* d_desc, uint32_t max_len, uint32_t k, uint32_t inst,
                       const rs_job* jobs, const gf_ptab* ptab, uint32_t job_stride, uint32_t no, hipStream_t s) {
  timed t_(c, HBX_K_RS_CODE, s);
  if (no == 0) no = 1;
  const uint32_t Ld = (max_len + 3) / 4;
  rs_with_tile(rs_tile3(k, no), [&](auto tile) {
    constexpr int c3 = decltype(tile)::value;
    hipLaunchKernelGGL((k_rs_code_perm3_rg<c3, 2>), dim3((Ld + 511) / 512, inst, (no + c3 - 1) / c3), dim3(256),
                       rs_perm3_lds_bytes(k, c3), s, d_buf, d_desc, k, jobs, ptab, job_stride);
  });
}

static int rs_reconstruct_rg(hbx_ctx* c, uint8_t* d_buf, const rg_desc* d_desc, uint32_t max_len,
                             const uint8_t* d_present, uint32_t inst, uint32_t k, uint32_t m, int32_t* d_status,
                             hipStream_t s) {
  if (int rc = rs_reconstruct_tables(c, d_present, inst, k, m, d_status, true, s)) return rc;
  rs_code_rg(c, d_buf, d_desc, max_len, k, inst, c->rs_jobs_d.as<rs_job>(), c->rs_ptab_d.as<gf_ptab>(), 1u, (m + 1) / 2, s);
  rs_code_rg(c, d_buf, d_desc, max_len, k, inst, c->rs_jobs_p.as<rs_job>(), c->rs_ptab_p.as<gf_ptab>(), 1u, (m + 1) / 2, s);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

// Ragged rows' leaf digests into c->leaf_hash: all n leaves, or the `nslots` listed per instance.
static void leaves_rg(hbx_ctx* c, hipStream_t s, const uint8_t* d_buf, const rg_desc* d_desc, uint32_t inst, uint32_t n,
                      const uint16_t* slots, uint32_t nslots) {
  leaf_digests(c, s, k_merkle_leaves_sha256_rg, k_merkle_leaves_sha3_rg, slots ? nslots : n, inst, d_buf, d_desc, n,
               c->leaf_hash.as<uint32_t>(), slots, nslots);
}

// decode_tail on rg_desc rows; d_out_off = the payloads' offsets in d_out.
static int decode_tail_rg(hbx_ctx* c, uint8_t* d_buf, const rg_desc* d_desc, uint32_t max_len, const uint8_t* d_present,
                          const uint8_t* d_leaf_hash, const uint8_t* d_root_expect, uint32_t inst, uint32_t k, uint32_t m,
                          uint8_t* d_out, const uint64_t* d_out_off, uint64_t* d_out_len, int32_t* d_status,
                          hipStream_t s) {
  const dim3 glue_grid((unsigned)(((uint64_t)k * max_len + 4095) / 4096), inst);
  return decode_tail(
      c, d_present, d_leaf_hash, d_root_expect, inst, k + m, m, d_status, s,
      [&](const uint16_t* slots, uint32_t nslots) { leaves_rg(c, s, d_buf, d_desc, inst, k + m, slots, nslots); },
      [&] { hipLaunchKernelGGL(k_glue_rg, glue_grid, dim3(256), 0, s, d_buf, d_desc, k, d_out, d_out_off, d_out_len,
                               d_status); });
}

int hbx_rs_encode_ragged_d(hbx_ctx* c, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off, const uint32_t* len,
                           const uint32_t* pitch, uint32_t inst, uint32_t k, uint32_t m, void* stream) {
  if (!c || !d_buf) return fail(c, HBX_E_INVALID_ARG, "hbx_rs_encode_ragged_d: bad args");
  uint32_t max_len = 0;
  int rc = rs_bounds(c, k, m);
  if (!rc) rc = rg_check(c, "hbx_rs_encode_ragged_d", buf_bytes, off, len, pitch, inst, k + m, &max_len);
  if (rc) return rc;
  HBX_ENTER(c, stream);
  if (m == 0) return HBX_OK;  // Coding::Trivial
  rc = rs_setup(c, k, m, s);
  if (rc) return rc;
  staging st(c, {(size_t)inst * sizeof(rg_desc)});
  if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_rs_encode_ragged_d: descriptor staging");
  rc = rg_upload(st, off, len, pitch, inst, s);
  if (rc) return rc;
  rs_code_rg(c, d_buf, st.dev<rg_desc>(0), max_len, k, inst, c->rs_enc_job.as<rs_job>(),
             c->rs_enc_ptab.as<gf_ptab>(), 0u, m, s);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

int hbx_rs_reconstruct_ragged_d(hbx_ctx* c, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off,
                                const uint32_t* len, const uint32_t* pitch, const uint8_t* d_present, uint32_t inst,
                                uint32_t k, uint32_t m, int32_t* d_status, void* stream) {
  if (!c || !d_buf || !d_present || !d_status) return fail(c, HBX_E_INVALID_ARG, "hbx_rs_reconstruct_ragged_d: bad args");
  uint32_t max_len = 0;
  int rc = rs_bounds(c, k, m);
  if (!rc) rc = rg_check(c, "hbx_rs_reconstruct_ragged_d", buf_bytes, off, len, pitch, inst, k + m, &max_len);
  if (rc) return rc;
  HBX_ENTER(c, stream);
  rc = rs_setup(c, k, m, s);
  if (rc) return rc;
  staging st(c, {(size_t)inst * sizeof(rg_desc)});
  if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_rs_reconstruct_ragged_d: descriptor staging");
  rc = rg_upload(st, off, len, pitch, inst, s);
  if (rc) return rc;
  return rs_reconstruct_rg(c, d_buf, st.dev<rg_desc>(0), max_len, d_present, inst, k, m, d_status, s);
}

int hbx_merkle_build_ragged_d(hbx_ctx* c, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off,
                              const uint32_t* len, const uint32_t* pitch, uint32_t inst, uint32_t n, uint8_t* d_nodes,
                              uint8_t* d_roots, void* stream) {
  if (!c || !d_buf || (!d_nodes && !d_roots)) return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_build_ragged_d: bad args");
  if (n == 0 || n > (uint32_t)RS_MAX_N) return fail(c, HBX_E_INVALID_ARG, "merkle: need 1 <= n <= 256");
  uint32_t max_len = 0;
  int rc = rg_check(c, "hbx_merkle_build_ragged_d", buf_bytes, off, len, pitch, inst, n, &max_len);
  if (rc) return rc;
  HBX_ENTER(c, stream);
  if (!c->leaf_hash.ensure((size_t)inst * n * 32) || (!d_roots && !c->roots.ensure((size_t)inst * 32)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "merkle: leaf hashes");
  staging st(c, {(size_t)inst * sizeof(rg_desc)});
  if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_merkle_build_ragged_d: descriptor staging");
  rc = rg_upload(st, off, len, pitch, inst, s);
  if (rc) return rc;
  leaves_rg(c, s, d_buf, st.dev<rg_desc>(0), inst, n, nullptr, 0);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_merkle_tree, dim3(inst), dim3(128), 0, s, c->leaf_hash.as<uint32_t>(), n,
                     d_roots ? d_roots : c->roots.as<uint8_t>(), d_nodes, c->merkle);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

int hbx_merkle_validate_ragged_d(hbx_ctx* c, const uint8_t* d_values, uint64_t values_bytes, const uint64_t* val_off,
                                 const uint8_t* d_node_hash, const uint8_t* d_sib_hash, const uint32_t* d_sides,
                                 const uint32_t* d_depth, const uint8_t* d_root, const uint32_t* d_sender,
                                 uint32_t count, uint32_t nproofs, uint8_t* d_valid, void* stream) {
  if (!c || !d_values || !val_off || !d_node_hash || !d_sib_hash || !d_sides || !d_depth || !d_root || !d_sender ||
      !d_valid || nproofs == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_validate_ragged_d: bad args");
  uint32_t bad = 0;
  if (hbx_bcplan::check_offsets(val_off, nproofs, values_bytes, &bad)) {
    if (bad < nproofs)
      return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_validate_ragged_d: val_off[%u..] is not a non-decreasing offset list", bad);
    return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_validate_ragged_d: val_off ends at %llu, past the %llu value bytes",
                (unsigned long long)val_off[nproofs], (unsigned long long)values_bytes);
  }
  HBX_ENTER(c, stream);
  const long_values lv(c, val_off, nproofs, 0);
  const staging st = lv.stage(c, val_off, nproofs);
  if (!st.pin || (lv.blocks() && !c->val_digest.ensure((size_t)nproofs * 32)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_merkle_validate_ragged_d: out of memory");
  if (int rc = st.upload(s)) return rc;
  lv.hash(c, s, st, k_merkle_values_sha256_rg, k_merkle_values_sha3_rg, d_values, c->val_digest.as<uint32_t>());
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_merkle_validate_rg, dim3((nproofs + 63) / 64), dim3(64), 0, s, d_values, st.dev<uint64_t>(0),
                     d_node_hash, d_sib_hash, d_sides, d_depth, d_root, d_sender, count, nproofs, d_valid, c->merkle,
                     c->val_digest.as<uint32_t>());
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

int hbx_broadcast_decode_ragged_d(hbx_ctx* c, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off,
                                  const uint32_t* len, const uint32_t* pitch, const uint8_t* d_present,
                                  const uint8_t* d_leaf_hash, const uint8_t* d_root_expect, uint32_t inst, uint32_t k,
                                  uint32_t m, uint8_t* d_out, uint64_t out_bytes, const uint64_t* out_off,
                                  uint64_t* d_out_len, int32_t* d_status, void* stream) {
  const char* fn = "hbx_broadcast_decode_ragged_d";
  if (!c || !d_buf || !d_present || !d_root_expect || !d_out || !out_off || !d_out_len || !d_status)
    return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  uint32_t max_len = 0;
  int rc = rs_bounds(c, k, m);
  if (!rc) rc = rg_check(c, fn, buf_bytes, off, len, pitch, inst, k + m, &max_len);
  if (rc) return rc;
  // the payload length comes from the (untrusted) header: k len - 4 bytes is the most glue_shards
  // can take, so every instance's output range must hold that many, apart from the others'
  uint32_t q = 0;
  if (hbx_bcplan::check_out(len, out_off, inst, k, out_bytes, &q)) {
    if (q == inst) return fail(c, HBX_E_INVALID_ARG, "%s: output ranges overlap", fn);
    const uint64_t need = (uint64_t)k * len[q] >= 4 ? (uint64_t)k * len[q] - 4 : 0;
    return fail(c, HBX_E_INVALID_ARG, "%s: instance %u: no room for k len - 4 = %llu bytes at out_off %llu of %llu", fn,
                q, (unsigned long long)need, (unsigned long long)out_off[q], (unsigned long long)out_bytes);
  }
  HBX_ENTER(c, stream);
  rc = rs_setup(c, k, m, s);
  if (rc) return rc;
  staging st(c, {(size_t)inst * sizeof(rg_desc), (size_t)inst * 8});  // rg_desc[inst] | out_off u64[inst]
  if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "%s: descriptor staging", fn);
  memcpy(st.host<uint64_t>(1), out_off, (size_t)inst * 8);
  rc = rg_upload(st, off, len, pitch, inst, s);
  if (rc) return rc;
  rc = rs_reconstruct_rg(c, d_buf, st.dev<rg_desc>(0), max_len, d_present, inst, k, m, d_status, s);
  if (rc) return rc;
  return decode_tail_rg(c, d_buf, st.dev<rg_desc>(0), max_len, d_present, d_leaf_hash, d_root_expect, inst, k, m, d_out,
                        st.dev<uint64_t>(1), d_out_len, d_status, s);
}

// ---- Broadcast, host-pointer forms (include/hbx.h): the _d calls above on context-owned staging
// buffers (c->hs[]), on the context's own stream, blocking until the outputs are on the host -- the
// shape a thin Rust FFI drives from Vec<u8> / &[u8] ------------
static uint8_t* stage(hbx_ctx* c, int slot, size_t bytes) {
  return c->hs[slot].ensure(bytes ? bytes : 1) ? c->hs[slot].as<uint8_t>() : nullptr;
}
#define HBX_STAGE(ptr, slot, bytes, what)                                                      \
  uint8_t* ptr = stage(c, slot, bytes);                                                      \
  if (!ptr) return fail(c, HBX_E_OUT_OF_MEMORY, "%s: out of device memory (staging)", what)
#define HBX_H2D(dst, src, bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream))
#define HBX_D2H(dst, src, bytes) HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream))

// P proofs up into hs[1..4]: node hashes, sibling hashes, u = sides | depth (| `more` u32 columns), roots.
struct proof_dev { uint8_t *nodes, *sibs, *root; uint32_t* u; };
static int stage_proofs(hbx_ctx* c, const char* fn, size_t P, const uint8_t* node_hash, const uint8_t* sib_hash,
                        const uint32_t* sides, const uint32_t* depth, const uint8_t* root, size_t more, proof_dev* pd) {
  HBX_STAGE(dh, 1, P * 17 * 32, fn);
  HBX_STAGE(dsib, 2, P * 16 * 32, fn);
  HBX_STAGE(du, 3, P * 4 * (2 + more), fn);
  HBX_STAGE(dr, 4, P * 32, fn);
  HBX_H2D(dh, node_hash, P * 17 * 32);
  HBX_H2D(dsib, sib_hash, P * 16 * 32);
  HBX_H2D(du, sides, P * 4);
  HBX_H2D(du + P * 4, depth, P * 4);
  HBX_H2D(dr, root, P * 32);
  *pd = proof_dev{dh, dsib, dr, (uint32_t*)du};
  return HBX_OK;
}

// A decode's payload bytes and dlen = out_len u64[count] | status i32[count] back; synchronised at return.
static int decode_readback(hbx_ctx* c, uint8_t* out, const uint8_t* dout, size_t out_bytes, uint64_t* out_len,
                           int32_t* status, const uint8_t* dlen, size_t count) {
  if (out_bytes) HBX_D2H(out, dout, out_bytes);
  HBX_D2H(out_len, dlen, count * 8);
  HBX_D2H(status, dlen + count * 8, count * 4);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_rs_encode(hbx_ctx* c, uint8_t* shards, uint32_t inst, uint32_t k, uint32_t m, uint32_t L) {
  if (!c || !shards || inst == 0 || L == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_rs_encode: bad args");
  if (m == 0) return HBX_OK;  // Coding::Trivial
  HBX_ENTER(c, c->stream);
  const size_t row = (size_t)(k + m) * L;
  HBX_STAGE(d, 0, row * inst, "hbx_rs_encode");
  // the k data shards of every instance in, the m parity shards out (one strided copy each way)
  HIPCHK(c, hipMemcpy2DAsync(d, row, shards, row, (size_t)k * L, inst, hipMemcpyHostToDevice, c->stream));
  int rc = hbx_rs_encode_d(c, d, inst, k, m, L, c->stream);
  if (rc) return rc;
  HIPCHK(c, hipMemcpy2DAsync(shards + (size_t)k * L, row, d + (size_t)k * L, row, (size_t)m * L, inst,
                             hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_rs_reconstruct(hbx_ctx* c, uint8_t* shards, const uint8_t* present, uint32_t inst, uint32_t k, uint32_t m,
                       uint32_t L, int32_t* status) {
  if (!c || !shards || !present || !status || inst == 0 || L == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_rs_reconstruct: bad args");
  HBX_ENTER(c, c->stream);
  const size_t n = (size_t)k + m, all = n * L * inst;
  HBX_STAGE(d, 0, all, "hbx_rs_reconstruct");
  HBX_STAGE(dp, 1, n * inst, "hbx_rs_reconstruct");
  HBX_STAGE(ds, 2, (size_t)inst * 4, "hbx_rs_reconstruct");
  HBX_H2D(d, shards, all);
  HBX_H2D(dp, present, n * inst);
  int rc = hbx_rs_reconstruct_d(c, d, dp, inst, k, m, L, (int32_t*)ds, c->stream);
  if (rc) return rc;
  HBX_D2H(shards, d, all);
  HBX_D2H(status, ds, (size_t)inst * 4);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_merkle_roots(hbx_ctx* c, const uint8_t* shards, uint32_t inst, uint32_t n, uint32_t L, uint8_t* roots) {
  if (!c || !shards || !roots || inst == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_roots: bad args");
  HBX_ENTER(c, c->stream);
  const size_t all = (size_t)n * L * inst;
  HBX_STAGE(d, 0, all, "hbx_merkle_roots");
  HBX_STAGE(dr, 1, (size_t)inst * 32, "hbx_merkle_roots");
  HBX_H2D(d, shards, all);
  int rc = hbx_merkle_roots_d(c, d, inst, n, L, dr, c->stream);
  if (rc) return rc;
  HBX_D2H(roots, dr, (size_t)inst * 32);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_merkle_build(hbx_ctx* c, const uint8_t* shards, uint32_t inst, uint32_t n, uint32_t L, uint8_t* nodes,
                     uint8_t* roots) {
  if (!c || !shards || !nodes || inst == 0 || n == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_build: bad args");
  HBX_ENTER(c, c->stream);
  const size_t all = (size_t)n * L * inst, nb = (size_t)inst * merkle_node_count(n) * 32;
  HBX_STAGE(d, 0, all, "hbx_merkle_build");
  HBX_STAGE(dn, 1, nb, "hbx_merkle_build");
  HBX_STAGE(dr, 2, (size_t)inst * 32, "hbx_merkle_build");
  HBX_H2D(d, shards, all);
  int rc = hbx_merkle_build_d(c, d, inst, n, L, dn, dr, c->stream);
  if (rc) return rc;
  HBX_D2H(nodes, dn, nb);
  if (roots) HBX_D2H(roots, dr, (size_t)inst * 32);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_merkle_proofs(hbx_ctx* c, const uint8_t* nodes, uint32_t inst, uint32_t n, const uint32_t* req, uint32_t count,
                      uint8_t* node_hash, uint8_t* sib_hash, uint32_t* sides, uint32_t* depth, uint8_t* root) {
  if (!c || !nodes || !req || !node_hash || !sib_hash || !sides || !depth || !root || inst == 0 || count == 0 ||
      n == 0 || n > (uint32_t)RS_MAX_N)
    return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_proofs: bad args");
  for (uint32_t q = 0; q < count; q++)
    if (req[2 * q] >= inst || req[2 * q + 1] >= n)
      return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_proofs: request %u names leaf %u of instance %u (inst %u, n %u)",
                  q, req[2 * q + 1], req[2 * q], inst, n);
  HBX_ENTER(c, c->stream);
  const size_t nb = (size_t)inst * merkle_node_count(n) * 32;
  HBX_STAGE(dn, 0, nb, "hbx_merkle_proofs");
  HBX_STAGE(dq, 1, (size_t)count * 8, "hbx_merkle_proofs");
  HBX_STAGE(dh, 2, (size_t)count * 17 * 32, "hbx_merkle_proofs");
  HBX_STAGE(dsib, 3, (size_t)count * 16 * 32, "hbx_merkle_proofs");
  HBX_STAGE(dsd, 4, (size_t)count * 8, "hbx_merkle_proofs");
  HBX_STAGE(dr, 5, (size_t)count * 32, "hbx_merkle_proofs");
  HBX_H2D(dn, nodes, nb);
  HBX_H2D(dq, req, (size_t)count * 8);
  // levels below a proof's depth are not written: zeros, as in a freshly allocated output
  HIPCHK(c, hipMemsetAsync(dh, 0, (size_t)count * 17 * 32, c->stream));
  HIPCHK(c, hipMemsetAsync(dsib, 0, (size_t)count * 16 * 32, c->stream));
  int rc = hbx_merkle_proofs_d(c, dn, n, (const uint32_t*)dq, count, dh, dsib, (uint32_t*)dsd,
                               (uint32_t*)dsd + count, dr, c->stream);
  if (rc) return rc;
  HBX_D2H(node_hash, dh, (size_t)count * 17 * 32);
  HBX_D2H(sib_hash, dsib, (size_t)count * 16 * 32);
  HBX_D2H(sides, dsd, (size_t)count * 4);
  HBX_D2H(depth, dsd + (size_t)count * 4, (size_t)count * 4);
  HBX_D2H(root, dr, (size_t)count * 32);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_merkle_validate(hbx_ctx* c, const uint8_t* values, uint32_t vlen, const uint8_t* node_hash,
                        const uint8_t* sib_hash, const uint32_t* sides, const uint32_t* depth, const uint8_t* root,
                        const uint32_t* sender, uint32_t count, uint32_t nproofs, uint8_t* valid) {
  if (!c || !values || !node_hash || !sib_hash || !sides || !depth || !root || !sender || !valid || nproofs == 0 ||
      vlen == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_merkle_validate: bad args");
  HBX_ENTER(c, c->stream);
  const size_t P = nproofs;
  HBX_STAGE(dv, 0, P * vlen, "hbx_merkle_validate");
  HBX_STAGE(dok, 5, P, "hbx_merkle_validate");
  proof_dev pd;
  if (int rc = stage_proofs(c, "hbx_merkle_validate", P, node_hash, sib_hash, sides, depth, root, 1, &pd)) return rc;
  HBX_H2D(dv, values, P * vlen);
  HBX_H2D(pd.u + 2 * P, sender, P * 4);  // the one more column of pd.u
  if (int rc = hbx_merkle_validate_d(c, dv, vlen, pd.nodes, pd.sibs, pd.u, pd.u + P, pd.root, pd.u + 2 * P, count,
                                     nproofs, dok, c->stream))
    return rc;
  HBX_D2H(valid, dok, P);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

static int broadcast_decode_host(hbx_ctx* c, uint8_t* shards, const uint8_t* present, const uint8_t* leaf_hash,
                                 const uint8_t* root_expect, uint32_t inst, uint32_t k, uint32_t m, uint32_t L,
                                 uint8_t* out, uint64_t out_stride, uint64_t* out_len, int32_t* status,
                                 const char* what) {
  if (!c || !shards || !present || !root_expect || !out || !out_len || !status || inst == 0 || L == 0)
    return fail(c, HBX_E_INVALID_ARG, "%s: bad args", what);
  HBX_ENTER(c, c->stream);
  const size_t n = (size_t)k + m, all = n * L * inst;
  HBX_STAGE(d, 0, all, what);
  HBX_STAGE(dp, 1, n * inst, what);
  HBX_STAGE(dre, 2, (size_t)inst * 32, what);
  HBX_STAGE(dout, 3, (size_t)inst * out_stride, what);
  HBX_STAGE(dlen, 4, (size_t)inst * 12, what);  // out_len (u64) | status (i32)
  uint8_t* dl = nullptr;
  if (leaf_hash) {
    dl = stage(c, 5, n * inst * 32);
    if (!dl) return fail(c, HBX_E_OUT_OF_MEMORY, "%s: out of device memory (staging)", what);
    HBX_H2D(dl, leaf_hash, n * inst * 32);
  }
  HBX_H2D(d, shards, all);
  HBX_H2D(dp, present, n * inst);
  HBX_H2D(dre, root_expect, (size_t)inst * 32);
  HIPCHK(c, hipMemsetAsync(dout, 0, (size_t)inst * out_stride, c->stream));  // bytes past a payload: 0
  int rc = broadcast_decode(c, d, dp, dl, dre, inst, k, m, L, dout, out_stride, (uint64_t*)dlen,
                            (int32_t*)(dlen + (size_t)inst * 8), c->stream);
  if (rc) return rc;
  HBX_D2H(shards, d, all);
  return decode_readback(c, out, dout, (size_t)inst * out_stride, out_len, status, dlen, inst);
}

int hbx_broadcast_decode(hbx_ctx* c, uint8_t* shards, const uint8_t* present, const uint8_t* root_expect, uint32_t inst,
                         uint32_t k, uint32_t m, uint32_t L, uint8_t* out, uint64_t out_stride, uint64_t* out_len,
                         int32_t* status) {
  return broadcast_decode_host(c, shards, present, nullptr, root_expect, inst, k, m, L, out, out_stride, out_len,
                               status, "hbx_broadcast_decode");
}

int hbx_broadcast_decode_leaves(hbx_ctx* c, uint8_t* shards, const uint8_t* present, const uint8_t* leaf_hash,
                                const uint8_t* root_expect, uint32_t inst, uint32_t k, uint32_t m, uint32_t L,
                                uint8_t* out, uint64_t out_stride, uint64_t* out_len, int32_t* status) {
  if (!leaf_hash) return fail(c, HBX_E_INVALID_ARG, "hbx_broadcast_decode_leaves: leaf_hash is NULL");
  return broadcast_decode_host(c, shards, present, leaf_hash, root_expect, inst, k, m, L, out, out_stride, out_len,
                               status, "hbx_broadcast_decode_leaves");
}
// ---- Broadcast, message by message (include/hbx.h): the echo store, adds and listed decodes -----
int hbx_prepare_broadcast(hbx_ctx* c, uint32_t inst, uint32_t k, uint32_t m, uint32_t max_shard_len) {
  const char* fn = "hbx_prepare_broadcast";
  if (!c || inst == 0 || max_shard_len == 0 || max_shard_len > 0xFFFFFFF0u)
    return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  if (int rc = rs_bounds(c, k, m)) return rc;
  HBX_ENTER(c, c->stream);
  const size_t slots = (size_t)inst * (k + m);
  const uint32_t pitch = (max_shard_len + 3) & ~3u;
  const bool same = c->bc_state.p && c->bc_inst == inst && c->bc_k == k && c->bc_m == m && c->bc_max == max_shard_len;
  c->bc_live = false;
  if (!same) {
    if (!c->bc_state.ensure(slots) || !c->bc_len.ensure(slots * 4) || !c->bc_shard.ensure((slots + 1) * pitch) ||
        !c->bc_root.ensure(slots * 32) || !c->bc_leaf.ensure(slots * 32))
      return fail(c, HBX_E_OUT_OF_MEMORY, "%s: out of device memory (%zu slots of %u bytes)", fn, slots, pitch);
    c->bc_inst = inst, c->bc_k = k, c->bc_m = m, c->bc_max = max_shard_len, c->bc_pitch = pitch;
    HIPCHK(c, hipMemsetAsync(c->bc_len.p, 0, slots * 4, s));
    HIPCHK(c, hipMemsetAsync(c->bc_root.p, 0, slots * 32, s));
    HIPCHK(c, hipMemsetAsync(c->bc_shard.as<uint8_t>() + slots * pitch, 0xA5, pitch, s));  // the canary row
  }
  HIPCHK(c, hipMemsetAsync(c->bc_state.p, 0, slots, s));
  c->bc_live = true;
  return HBX_OK;
}

static int bc_enter(hbx_ctx* c, const char* fn) {
  if (!c) return HBX_E_INVALID_ARG;
  if (!c->bc_live) return fail(c, HBX_E_NO_BROADCAST, "%s: no echo store (hbx_prepare_broadcast)", fn);
  return HBX_OK;
}

int hbx_add_echoes_d(hbx_ctx* c, const uint8_t* d_values, uint64_t values_bytes, const uint64_t* val_off,
                     const uint8_t* d_node_hash, const uint8_t* d_sib_hash, const uint32_t* d_sides,
                     const uint32_t* d_depth, const uint8_t* d_root, const uint32_t* inst, const uint32_t* sender,
                     uint32_t count, uint8_t* d_status, void* stream) {
  const char* fn = "hbx_add_echoes_d";
  if (int rc = bc_enter(c, fn)) return rc;
  if (count == 0) return HBX_OK;
  if (!d_values || !val_off || !d_node_hash || !d_sib_hash || !d_sides || !d_depth || !d_root || !inst || !sender)
    return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  const uint32_t n = c->bc_k + c->bc_m;
  if (int rc = hbx_bcplan::check_items(inst, sender, count, n, c->bc_inst)) return bc_plan_rejected(c, rc, fn);
  if (int rc = hbx_bcplan::check_offsets(val_off, count, values_bytes)) return bc_plan_rejected(c, rc, fn);
  HBX_ENTER(c, stream);
  const long_values lv(c, val_off, count, (uint64_t)c->bc_max + 1);
  // staging after the long values' ranges: items uint2[count] | sender u32[count]
  const staging stg = lv.stage(c, val_off, count, (size_t)count * 8, (size_t)count * 4);
  if (!stg.pin || (lv.blocks() && !c->val_digest.ensure((size_t)count * 32)) ||
      (!d_status && !c->bc_item_st.ensure(count)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "%s: out of memory", fn);
  uint2* it = stg.host<uint2>(3);
  for (uint32_t j = 0; j < count; j++) it[j] = make_uint2(inst[j], sender[j]);
  memcpy(stg.host<uint32_t>(4), sender, (size_t)count * 4);
  if (int rc = stg.upload(s)) return rc;
  const uint64_t* d_off = stg.dev<uint64_t>(0);
  const uint2* d_items = stg.dev<uint2>(3);
  uint8_t* st = d_status ? d_status : c->bc_item_st.as<uint8_t>();
  hipLaunchKernelGGL(k_echo_precheck, dim3((count + 63) / 64), dim3(64), 0, s, d_items, d_off, count, n, c->bc_max,
                     c->bc_state.as<uint8_t>(), st);
  lv.hash(c, s, stg, k_echo_values_sha256, k_echo_values_sha3, d_values, st, c->val_digest.as<uint32_t>());
  hipLaunchKernelGGL(k_echo_validate, dim3((count + 63) / 64), dim3(64), 0, s, d_values, d_off, d_node_hash, d_sib_hash,
                     d_sides, d_depth, d_root, stg.dev<uint32_t>(4), n, count, st, c->merkle,
                     c->val_digest.as<uint32_t>());
  // the longest value that can be stored bounds the copy grid; shorter items' spare blocks return at once
  uint64_t longest = 0;
  for (uint32_t j = 0; j < count; j++) {
    const uint64_t v = val_off[j + 1] - val_off[j];
    if (v <= (uint64_t)c->bc_max + 1 && v > longest) longest = v;
  }
  const uint32_t per_block = 256 * ECHO_COPY;
  const uint32_t xb = longest > 1 ? (uint32_t)((longest - 1 + per_block - 1) / per_block) : 1;
  for (uint32_t j0 = 0; j0 < count; j0 += 65535) {  // grid.y limit
    const uint32_t cnt = count - j0 < 65535 ? count - j0 : 65535;
    hipLaunchKernelGGL(k_echo_store, dim3(xb, cnt), dim3(256), 0, s, d_values, d_off + j0, d_items + j0,
                       d_node_hash + (size_t)j0 * 17 * 32, d_depth + j0, d_root + (size_t)j0 * 32, st + j0, n, c->bc_pitch,
                       c->bc_shard.as<uint8_t>(), c->bc_len.as<uint32_t>(), c->bc_root.as<uint8_t>(),
                       c->bc_leaf.as<uint8_t>(), c->bc_state.as<uint8_t>());
  }
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

int hbx_add_echoes(hbx_ctx* c, const uint8_t* values, uint64_t values_bytes, const uint64_t* val_off,
                   const uint8_t* node_hash, const uint8_t* sib_hash, const uint32_t* sides, const uint32_t* depth,
                   const uint8_t* root, const uint32_t* inst, const uint32_t* sender, uint32_t count, uint8_t* status) {
  const char* fn = "hbx_add_echoes";
  if (int rc = bc_enter(c, fn)) return rc;
  if (count == 0) return HBX_OK;
  if (!values || !val_off || !node_hash || !sib_hash || !sides || !depth || !root || !inst || !sender)
    return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  if (int rc = hbx_bcplan::check_offsets(val_off, count, values_bytes)) return bc_plan_rejected(c, rc, fn);
  HBX_ENTER(c, c->stream);
  const size_t P = count;
  HBX_STAGE(dv, 0, values_bytes, fn);
  HBX_STAGE(dst, 5, P, fn);
  proof_dev pd;
  if (int rc = stage_proofs(c, fn, P, node_hash, sib_hash, sides, depth, root, 0, &pd)) return rc;
  if (values_bytes) HBX_H2D(dv, values, values_bytes);
  if (int rc = hbx_add_echoes_d(c, dv, values_bytes, val_off, pd.nodes, pd.sibs, pd.u, pd.u + P, pd.root, inst, sender,
                                count, dst, c->stream))
    return rc;
  std::vector<uint8_t> got(P);
  HBX_D2H(got.data(), dst, P);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (status) memcpy(status, got.data(), P);
  return HBX_OK;
}

int hbx_broadcast_decode_insts_d(hbx_ctx* c, const uint32_t* insts, const uint8_t* roots, const uint32_t* len,
                                 const uint8_t* use, uint32_t na, uint8_t* d_out, uint64_t out_bytes,
                                 const uint64_t* out_off, uint64_t* d_out_len, int32_t* d_status, void* stream) {
  const char* fn = "hbx_broadcast_decode_insts_d";
  if (int rc = bc_enter(c, fn)) return rc;
  if (na == 0) return HBX_OK;
  if (!insts || !roots || !len || (!d_out && out_bytes) || !out_off || !d_out_len || !d_status)
    return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  const uint32_t k = c->bc_k, m = c->bc_m, n = k + m;
  if (na > 65535) return fail(c, HBX_E_INVALID_ARG, "%s: at most 65535 attempts per call", fn);
  if (int rc = hbx_bcplan::check_attempts(insts, roots, len, use, na, n, c->bc_inst, c->bc_max))
    return bc_plan_rejected(c, rc, fn);
  if (int rc = hbx_bcplan::check_out(len, out_off, na, k, out_bytes)) return bc_plan_rejected(c, rc, fn);
  std::vector<uint64_t> off;
  std::vector<uint32_t> pitch;
  const uint64_t work_bytes = hbx_bcplan::work_layout(len, na, n, off, pitch);
  uint32_t max_len = 0;
  for (uint32_t a = 0; a < na; a++) max_len = std::max(max_len, len[a]);
  HBX_ENTER(c, stream);
  int rc = rs_setup(c, k, m, s);
  if (rc) return rc;
  const size_t cells = (size_t)na * n;
  if (!c->bc_work.ensure(work_bytes) || !c->bc_present.ensure(cells) || !c->bc_leaf_w.ensure(cells * 32) ||
      !c->bc_size_bad.ensure((size_t)na * 4))
    return fail(c, HBX_E_OUT_OF_MEMORY, "%s: out of device memory", fn);
  // staging: rg_desc[na] | out_off u64[na] | insts u32[na] | roots [na][32] | use [na][n]
  staging st(c, {(size_t)na * sizeof(rg_desc), (size_t)na * 8, (size_t)na * 4, (size_t)na * 32, cells});
  if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "%s: descriptor staging", fn);
  memcpy(st.host<uint64_t>(1), out_off, (size_t)na * 8);
  memcpy(st.host<uint32_t>(2), insts, (size_t)na * 4);
  memcpy(st.host<uint8_t>(3), roots, (size_t)na * 32);
  if (use) memcpy(st.host<uint8_t>(4), use, cells);
  else memset(st.host<uint8_t>(4), 1, cells);
  rc = rg_upload(st, off.data(), len, pitch.data(), na, s);
  if (rc) return rc;
  const rg_desc* d_desc = st.dev<rg_desc>(0);
  const uint8_t* d_roots = st.dev<uint8_t>(3);
  uint8_t* work = c->bc_work.as<uint8_t>();
  const uint8_t* d_present = c->bc_present.as<uint8_t>();
  HIPCHK(c, hipMemsetAsync(c->bc_size_bad.p, 0, (size_t)na * 4, s));
  const uint32_t per_block = 256 * ECHO_COPY;
  hipLaunchKernelGGL(k_echo_gather, dim3((max_len + per_block - 1) / per_block, n, na), dim3(256), 0, s,
                     st.dev<uint32_t>(2), d_roots, st.dev<uint8_t>(4), d_desc, n, c->bc_pitch,
                     c->bc_shard.as<uint8_t>(), c->bc_len.as<uint32_t>(), c->bc_root.as<uint8_t>(),
                     c->bc_leaf.as<uint8_t>(), c->bc_state.as<uint8_t>(), work, c->bc_present.as<uint8_t>(),
                     c->bc_leaf_w.as<uint8_t>(), c->bc_size_bad.as<uint32_t>());
  HIPCHK(c, hipGetLastError());
  // from here on: the ragged decode's own pipeline, on the work buffer
  rc = rs_reconstruct_rg(c, work, d_desc, max_len, d_present, na, k, m, d_status, s);
  if (rc) return rc;
  hipLaunchKernelGGL(k_echo_size_status, dim3((na + 63) / 64), dim3(64), 0, s, c->bc_size_bad.as<uint32_t>(), na,
                     (int32_t)HBX_E_SHARD_SIZE, d_status);
  return decode_tail_rg(c, work, d_desc, max_len, d_present, c->bc_leaf_w.as<uint8_t>(), d_roots, na, k, m, d_out,
                        st.dev<uint64_t>(1), d_out_len, d_status, s);
}

int hbx_broadcast_decode_insts(hbx_ctx* c, const uint32_t* insts, const uint8_t* roots, const uint32_t* len,
                               const uint8_t* use, uint32_t na, uint8_t* out, uint64_t out_bytes, const uint64_t* out_off,
                               uint64_t* out_len, int32_t* status) {
  const char* fn = "hbx_broadcast_decode_insts";
  if (int rc = bc_enter(c, fn)) return rc;
  if (na == 0) return HBX_OK;
  if ((!out && out_bytes) || !out_len || !status) return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  HBX_ENTER(c, c->stream);
  HBX_STAGE(dout, 0, out_bytes, fn);
  HBX_STAGE(dlen, 1, (size_t)na * 12, fn);  // out_len (u64) | status (i32)
  HIPCHK(c, hipMemsetAsync(dout, 0, out_bytes ? out_bytes : 1, c->stream));  // bytes past a payload: 0
  if (int rc = hbx_broadcast_decode_insts_d(c, insts, roots, len, use, na, dout, out_bytes, out_off, (uint64_t*)dlen,
                                            (int32_t*)(dlen + (size_t)na * 8), c->stream))
    return rc;
  return decode_readback(c, out, dout, out_bytes, out_len, status, dlen, na);
}

int hbx_get_echo_slots(hbx_ctx* c, uint8_t* state, uint32_t* len, uint8_t* root) {
  if (int rc = bc_enter(c, "hbx_get_echo_slots")) return rc;
  HBX_ENTER(c, c->stream);
  const size_t slots = (size_t)c->bc_inst * (c->bc_k + c->bc_m);
  if (state) HBX_D2H(state, c->bc_state.p, slots);
  if (len) HBX_D2H(len, c->bc_len.p, slots * 4);
  if (root) HBX_D2H(root, c->bc_root.p, slots * 32);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_debug_get_echo_rows(hbx_ctx* c, uint8_t* rows, uint64_t bytes) {
  const char* fn = "hbx_debug_get_echo_rows";
  if (!c || !rows) return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  if (!c->bc_live) return fail(c, HBX_E_NO_BROADCAST, "%s: no echo store (hbx_prepare_broadcast)", fn);
  const uint64_t have = ((uint64_t)c->bc_inst * (c->bc_k + c->bc_m) + 1) * c->bc_pitch;
  if (bytes > have) return fail(c, HBX_E_INVALID_ARG, "%s: the store's rows are %llu bytes", fn, (unsigned long long)have);
  HBX_ENTER(c, c->stream);
  if (bytes) HBX_D2H(rows, c->bc_shard.p, bytes);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}
#undef HBX_STAGE
#undef HBX_H2D
#undef HBX_D2H

// ---- Common Coin ----------------------------------------------------------------------------
// The true H = hash_g2(nonce) of the prepared nonces from H' = [m] H (k_h2_from_heff), once, on s.
static int coin_true_h(hbx_ctx* c, hipStream_t s) {
  if (c->coin_h_ready) return HBX_OK;
  hipLaunchKernelGGL(k_h2_from_heff, dim3((c->coin_I + 63) / 64), dim3(64), 0, s, c->coin_Hp.as<g2a>(), c->coin_I,
                     c->coin_H.as<g2a>());
  HIPCHK(c, hipGetLastError());
  c->coin_h_ready = true;
  return HBX_OK;
}

int hbx_prepare_nonces(hbx_ctx* c, const uint8_t* nonce_blob, const uint64_t* nonce_off, uint32_t count,
                       uint8_t* h96) {
  if (!c || !nonce_off || count == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_prepare_nonces: bad args");
  for (uint32_t j = 0; j < count; j++)
    if (nonce_off[j + 1] < nonce_off[j]) return fail(c, HBX_E_INVALID_ARG, "nonce_off not monotone");
  const uint64_t total = nonce_off[count];
  if (total && !nonce_blob) return fail(c, HBX_E_INVALID_ARG, "hbx_prepare_nonces: null blob");
  HBX_ENTER(c, c->stream);
  if (!c->coin_blob.ensure(total ? total : 16) || !c->coin_off.ensure((size_t)(count + 1) * 8) ||
      !c->coin_H.ensure((size_t)count * sizeof(g2a)) || !c->coin_Hp.ensure((size_t)count * sizeof(g2a)) ||
      !c->coin_lines.ensure((size_t)count * MILLER_LINES * sizeof(line_pre)) ||
      !c->coin_lines_d.ensure((size_t)count * MILLER_LINES * sizeof(line_pre_d)) ||
      !c->coin_scratch.ensure((size_t)count * MILLER_LINES * sizeof(fq2d)) || !c->coin_out96.ensure((size_t)count * 96))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_prepare_nonces: out of device memory");
  if (total) HIPCHK(c, hipMemcpyAsync(c->coin_blob.p, nonce_blob, total, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->coin_off.p, nonce_off, (size_t)(count + 1) * 8, hipMemcpyHostToDevice, s));
  // the caller's host buffers are free once the uploads are done; the hashing itself is enqueued
  // and the call returns without waiting for it (unless h96 asks for the hashes)
  HIPCHK(c, hipStreamSynchronize(s));
  {
    timed t_(c, HBX_K_HASH_NONCES, s);
    hipLaunchKernelGGL(k_hash_nonces, dim3((unsigned)(((size_t)count * HASH_K + 63) / 64)), dim3(64), 0, s, c->coin_blob.as<uint8_t>(),
                       c->coin_off.as<uint64_t>(), count, c->coin_Hp.as<g2a>(), c->digest, 0);
  }
  HIPCHK(c, hipGetLastError());
  // the Miller lines of H' are prepared on demand by the one-lane share checks (the two-lane
  // kernel, the default for a coin round, generates both pairs' lines itself); the true H only for
  // hbx_sign and h96 (coin_true_h): the share checks and the combine work on H' = [m] H
  c->coin_lines_ready = false;
  c->coin_h_ready = false;
  c->coin_live = false;  // the matrix of an earlier round is not of these nonces (hbx_add_sig_shares_d)
  c->coin_I = count;
  if (h96) {
    if (int rc = coin_true_h(c, s)) return rc;
    hipLaunchKernelGGL(k_compress_g2, dim3((count + 63) / 64), dim3(64), 0, s, c->coin_H.as<g2a>(), count, 1u,
                       c->coin_out96.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h96, c->coin_out96.p, (size_t)count * 96, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
  }
  HIPCHK(c, c->coin_ready_ev.create());
  HIPCHK(c, hipEventRecord(c->coin_ready_ev.e, s));
  c->coin_I = count;
  return HBX_OK;
}

int hbx_sign(hbx_ctx* c, const uint8_t* sk32, uint32_t n, uint8_t* sig96) {
  if (!c || !sk32 || !sig96 || n == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_sign: bad args");
  if (c->coin_I == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "hbx_prepare_nonces has not been called");
  if (!scalars_canonical(sk32, n)) return fail(c, HBX_E_INVALID_ARG, "hbx_sign: scalar >= r");
  HBX_ENTER(c, c->stream);
  const size_t m = (size_t)n * c->coin_I;
  if (!c->coin_sk.ensure((size_t)n * 32) || !c->coin_sig96.ensure(m * 96))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_sign: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->coin_sk.p, sk32, (size_t)n * 32, hipMemcpyHostToDevice, s));
  if (int rc = coin_true_h(c, s)) return rc;
  hipLaunchKernelGGL(k_sign, dim3((n + 63) / 64, c->coin_I), dim3(64), 0, s, c->coin_sk.as<uint8_t>(), n,
                     c->coin_H.as<g2a>(), c->coin_sig96.as<uint8_t>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(sig96, c->coin_sig96.p, m * 96, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

// H''s prepared lines (wave-uniform loads) of the prepared nonces, once per hbx_prepare_nonces: the
// one-lane kernel's mixed loop, and since round 6 the two-lane kernel's H' pair (its lanes then
// generate only sigma's lines, together).
static int coin_prepare_lines(hbx_ctx* c, hipStream_t s) {
  if (c->coin_lines_ready) return HBX_OK;
  const uint32_t count = c->coin_I;
  timed t_(c, HBX_K_PREPARE_LINES, s);
  hipLaunchKernelGGL(k_prepare_lines<true>, dim3((count * LINE_K + 63) / 64), dim3(64), 0, s, c->coin_Hp.as<g2a>(), count,
                     c->coin_lines_d.as<line_pre_d>(), c->coin_scratch.as<fq2d>(), nullptr, 0u, nullptr, nullptr, nullptr, 1u,
                     UINT32_MAX, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, 0u);
  HIPCHK(c, hipGetLastError());
  const uint32_t nl = count * MILLER_LINES;
  hipLaunchKernelGGL(k_normalise_lines, dim3((nl + 63) / 64), dim3(64), 0, s, c->coin_lines.as<line_pre>(),
                     c->coin_scratch.as<fq2d>(), nl, c->coin_lines_d.as<line_pre_d>(), nullptr, nullptr, nullptr, nullptr);
  HIPCHK(c, hipGetLastError());
  c->coin_lines_ready = true;
  // the lines are built on this call's stream: move the prepare event past them, so a later
  // one-lane check on another stream (which waits on coin_ready_ev) is ordered after the build
  HIPCHK(c, c->coin_ready_ev.create());
  HIPCHK(c, hipEventRecord(c->coin_ready_ev.e, s));
  return HBX_OK;
}

// The signature-share check launch at `lanes` (1 or 2) lanes per check over `grid` blocks: the
// tiles (chunks, instances) of a matrix verification (tiles = nullptr), or the listed tiles of an
// add, grid (T, 1) (addplan.hpp).  Shares, decode statuses, present mask and verdicts are [I][n].
static int launch_sig_checks(hbx_ctx* c, hipStream_t s, int lanes, dim3 grid, const uint2* tiles, const g2a* sig,
                             const int32_t* sig_st, const uint8_t* d_present, uint32_t n, uint8_t* vd) {
  timed t_(c, HBX_K_VERIFY_SIG, s);
  c->coin_lanes_used = lanes;
  c->coin_tiles = grid.x * grid.y;
  if (lanes == 2) {
    const size_t glanes = (size_t)grid.x * grid.y * 64;
    if (!c->gslot.ensure(glanes * 2 * LDS_FQ6D_PACKED * 4))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_sig_shares: out of device memory (slots)");
    if (!c->fb_coin.ensure(4)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_sig_shares: out of device memory");
    HIPCHK(c, hipMemsetAsync(c->fb_coin.p, 0, 4, s));
    c->fb_last = &c->fb_coin;
    // Miller loops; the final exponentiation with compressed runs; then the pairs whose
    // decompression met g3 = 0 (SHARE_FALLBACK) once more, Miller and Granger-Scott squarings
    // only (both launches return at once per pair when there are none)
    for (uint32_t retry = 0; retry < 2; retry++) {
      hipLaunchKernelGGL(k_verify_sig_shares2, grid, dim3(64), 0, s, c->coin_Hp.as<g2a>(), c->pk.as<g1a>(), c->n_keys, sig,
                         sig_st, d_present, n, vd, c->gslot.as<uint32_t>(), retry, c->coin_lines_d.as<line_pre_d>(), tiles);
      HIPCHK(c, hipGetLastError());
      if (retry == 0)
        hipLaunchKernelGGL(k_verify_sig_shares2_fe<true>, grid, dim3(64), 0, s, n, vd, c->gslot.as<uint32_t>(),
                           c->force_fallback, c->fb_coin.as<uint32_t>(), tiles);
      else
        hipLaunchKernelGGL(k_verify_sig_shares2_fe<false>, grid, dim3(64), 0, s, n, vd, c->gslot.as<uint32_t>(), 0u,
                           c->fb_coin.as<uint32_t>(), tiles);
      HIPCHK(c, hipGetLastError());
    }
  } else {
    c->fb_last = nullptr;  // the one-lane coin check has no fallback path
    hipLaunchKernelGGL(k_verify_sig_shares, grid, dim3(64), 0, s, c->coin_lines_d.as<line_pre_d>(), c->coin_Hp.as<g2a>(),
                       c->pk.as<g1a>(), c->n_keys, sig, sig_st, d_present, n, vd, tiles);
    HIPCHK(c, hipGetLastError());
  }
  return HBX_OK;
}

// Signature-share checks of the prepared nonces on device buffers: d_sig96 [count][n][96],
// d_present [count][n] bytes (NULL = all present); statuses in c->coin_valid.
static int verify_sig_impl(hbx_ctx* c, const uint8_t* d_sig96, const uint8_t* d_present, uint32_t n, uint32_t count,
                           hipStream_t s) {
  const size_t m = (size_t)n * count;
  if (!c->coin_sig.ensure(m * sizeof(g2a)) || !c->coin_sig_st.ensure(m * 4) || !c->coin_valid.ensure(m))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_sig_shares: out of device memory");
  if (c->coin_ready_ev.e) HIPCHK(c, hipStreamWaitEvent(s, c->coin_ready_ev.e, 0));  // the nonces' hashes are in
  {
    timed t_(c, HBX_K_DECODE_SIGS, s);
    // curve membership only: the share checks test G2 membership on their Miller loop's [|x|] sigma
    hipLaunchKernelGGL(k_decompress_g2, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, d_sig96, m, c->coin_sig.as<g2a>(),
                       c->coin_sig_st.as<int32_t>(), 0u);
  }
  HIPCHK(c, hipGetLastError());
  // two lanes per check when one lane per check would leave SIMDs idle (a coin round of 256
  // instances at N = 128 is 512 one-lane waves on 1,024 SIMDs), or when asked for
  // (hbx_set_verify_lanes 2); one lane otherwise
  const size_t waves1 = (size_t)((n + 63) / 64) * count;
  const int lanes = c->verify_lanes == 1 || c->verify_lanes == 2 ? c->verify_lanes
                    : waves1 < FILL_WAVES ? 2 : 1;
  if (int rc = coin_prepare_lines(c, s)) return rc;
  const uint32_t per = lanes == 2 ? 32 : 64;
  if (int rc = launch_sig_checks(c, s, lanes, dim3((n + per - 1) / per, count), nullptr, c->coin_sig.as<g2a>(),
                                 c->coin_sig_st.as<int32_t>(), d_present, n, c->coin_valid.as<uint8_t>()))
    return rc;
  c->coin_n = n;
  c->coin_live = true;
  return HBX_OK;
}

static int verify_sig_check(hbx_ctx* c, uint32_t n, uint32_t count) {
  if (c->n_keys == 0) return fail(c, HBX_E_NO_KEYS, "hbx_set_pk_shares has not been called");
  if (count != c->coin_I) return fail(c, HBX_E_NO_CIPHERTEXTS, "%u instances but %u nonces prepared", count, c->coin_I);
  return HBX_OK;
}

int hbx_verify_sig_shares(hbx_ctx* c, const uint8_t* sig96, const uint8_t* present_bits, uint32_t n, uint32_t count,
                          uint8_t* valid_bits) {
  if (!c || !sig96 || n == 0 || count == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_verify_sig_shares: bad args");
  if (int rc = verify_sig_check(c, n, count)) return rc;
  HBX_ENTER(c, c->stream);
  const size_t m = (size_t)n * count;
  if (!c->coin_sig96.ensure(m * 96) || (present_bits && !c->coin_present.ensure(m)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_sig_shares: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->coin_sig96.p, sig96, m * 96, hipMemcpyHostToDevice, s));
  std::vector<uint8_t> pres;
  if (present_bits) {
    pres.resize(m);
    for (size_t k = 0; k < m; k++) pres[k] = (present_bits[k >> 3] >> (k & 7)) & 1;
    HIPCHK(c, hipMemcpyAsync(c->coin_present.p, pres.data(), m, hipMemcpyHostToDevice, s));
  }
  if (int rc = verify_sig_impl(c, c->coin_sig96.as<uint8_t>(), present_bits ? c->coin_present.as<uint8_t>() : nullptr,
                               n, count, s))
    return rc;
  std::vector<uint8_t> v(m);
  HIPCHK(c, hipMemcpyAsync(v.data(), c->coin_valid.p, m, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (valid_bits) pack_bits(v.data(), m, valid_bits);
  return HBX_OK;
}

int hbx_verify_sig_shares_d(hbx_ctx* c, const uint8_t* d_sig96, const uint8_t* d_present, uint32_t n, uint32_t count,
                            uint8_t* d_status, void* stream) {
  if (!c || !d_sig96 || n == 0 || count == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_verify_sig_shares_d: bad args");
  if (int rc = verify_sig_check(c, n, count)) return rc;
  HBX_ENTER(c, stream);
  if (int rc = verify_sig_impl(c, d_sig96, d_present, n, count, s)) return rc;
  if (d_status) HIPCHK(c, hipMemcpyAsync(d_status, c->coin_valid.p, (size_t)n * count, hipMemcpyDeviceToDevice, s));
  return HBX_OK;
}

int hbx_get_coin_lanes_used(const hbx_ctx* c) { return c ? c->coin_lanes_used : 0; }

int hbx_verify_sigs(hbx_ctx* c, const uint8_t* pk48, const uint8_t* msg_blob, const uint64_t* msg_off,
                    const uint8_t* sig96, uint32_t count, uint8_t* status) {
  if (!c || !pk48 || !msg_off || !sig96 || !status || count == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_verify_sigs: bad args");
  for (uint32_t i = 0; i < count; i++)
    if (msg_off[i + 1] < msg_off[i]) return fail(c, HBX_E_INVALID_ARG, "hbx_verify_sigs: msg_off not monotone");
  const uint64_t total = msg_off[count];
  if (total && !msg_blob) return fail(c, HBX_E_INVALID_ARG, "hbx_verify_sigs: null blob");
  HBX_ENTER(c, c->stream);
  if (!c->vs_pk.ensure((size_t)count * 48) || !c->vs_blob.ensure(total ? total : 16) ||
      !c->vs_off.ensure((size_t)(count + 1) * 8) || !c->vs_H.ensure((size_t)count * sizeof(g2a)) ||
      !c->vs_lines.ensure((size_t)count * MILLER_LINES * sizeof(line_pre)) ||
      !c->vs_lines_d.ensure((size_t)count * MILLER_LINES * sizeof(line_pre_d)) ||
      !c->vs_scratch.ensure((size_t)count * MILLER_LINES * sizeof(fq2d)) || !c->vs_sig96.ensure((size_t)count * 96) ||
      !c->vs_sig.ensure((size_t)count * sizeof(g2a)) || !c->vs_sig_st.ensure((size_t)count * 4) ||
      !c->vs_status.ensure(count))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_sigs: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->vs_pk.p, pk48, (size_t)count * 48, hipMemcpyHostToDevice, s));
  if (total) HIPCHK(c, hipMemcpyAsync(c->vs_blob.p, msg_blob, total, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->vs_off.p, msg_off, (size_t)(count + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->vs_sig96.p, sig96, (size_t)count * 96, hipMemcpyHostToDevice, s));
  // H_i = hash_g2(msg_i) on lane groups, its Miller lines, the signatures' decode
  hipLaunchKernelGGL(k_hash_nonces, dim3((unsigned)(((size_t)count * HASH_K + 63) / 64)), dim3(64), 0, s,
                     c->vs_blob.as<uint8_t>(), c->vs_off.as<uint64_t>(), count, c->vs_H.as<g2a>(), c->digest, 1);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_decompress_g2, dim3((count + 63) / 64), dim3(64), 0, s, c->vs_sig96.as<uint8_t>(), (size_t)count,
                     c->vs_sig.as<g2a>(), c->vs_sig_st.as<int32_t>(), 1u);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_prepare_lines<true>, dim3((count * LINE_K + 63) / 64), dim3(64), 0, s, c->vs_H.as<g2a>(), count,
                     c->vs_lines_d.as<line_pre_d>(), c->vs_scratch.as<fq2d>(), nullptr, 0u, nullptr, nullptr, nullptr, 1u,
                     UINT32_MAX, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, 0u);
  HIPCHK(c, hipGetLastError());
  const uint32_t nl = count * MILLER_LINES;
  hipLaunchKernelGGL(k_normalise_lines, dim3((nl + 63) / 64), dim3(64), 0, s, c->vs_lines.as<line_pre>(),
                     c->vs_scratch.as<fq2d>(), nl, c->vs_lines_d.as<line_pre_d>(), nullptr, nullptr, nullptr, nullptr);
  HIPCHK(c, hipGetLastError());
  {
    timed t_(c, HBX_K_VERIFY_SIG, s);
    hipLaunchKernelGGL(k_verify_sigs, dim3((count + 63) / 64), dim3(64), 0, s, c->vs_pk.as<uint8_t>(),
                       c->vs_lines_d.as<line_pre_d>(), c->vs_H.as<g2a>(), c->vs_sig.as<g2a>(), c->vs_sig_st.as<int32_t>(),
                       count, c->vs_status.as<uint8_t>());
  }
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(status, c->vs_status.p, count, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

namespace {
// Items per pass of hbx_verify_sigs_keyed and hbx_sign_msgs (hbbft_amd/hbx.py VERIFY_SIGS_CHUNK is the
// same number).  The state is about 2 KiB per item (H' and sigma decoded, the pair's 1.25 KiB slot
// for the halves of f, the compressed signature): 16,384 items are about 30 MB, 512 pair-check waves
// and 4,096 hash waves, as in hbx_sk_decrypt's pair mode.
constexpr uint32_t VERIFY_SIGS_CHUNK = 16384;

// shared argument check of the two message calls; the total blob length in *total
int msgs_check(hbx_ctx* c, const char* fn, const uint8_t* msg_blob, const uint64_t* msg_off, uint32_t count,
               uint64_t* total) {
  if (!msg_off || count == 0) return fail(c, HBX_E_INVALID_ARG, "%s: bad args", fn);
  for (uint32_t i = 0; i < count; i++)
    if (msg_off[i + 1] < msg_off[i]) return fail(c, HBX_E_INVALID_ARG, "%s: msg_off not monotone", fn);
  *total = msg_off[count] - msg_off[0];
  if (*total && !msg_blob) return fail(c, HBX_E_INVALID_ARG, "%s: null blob", fn);
  return HBX_OK;
}
}  // namespace

int hbx_verify_sigs_keyed(hbx_ctx* c, const uint8_t* pk48, uint32_t nkeys, const uint32_t* key_idx,
                          const uint8_t* msg_blob, const uint64_t* msg_off, const uint8_t* sig96, uint32_t count,
                          uint8_t* status, int32_t* key_status) {
  if (!c || !pk48 || nkeys == 0 || !key_idx || !sig96 || !status)
    return fail(c, HBX_E_INVALID_ARG, "hbx_verify_sigs_keyed: bad args");
  uint64_t total = 0;
  if (int rc = msgs_check(c, "hbx_verify_sigs_keyed", msg_blob, msg_off, count, &total)) return rc;
  HBX_ENTER(c, c->stream);
  // every buffer is sized here, before the first pass: the per-item state for one chunk only
  const size_t cap = std::min(VERIFY_SIGS_CHUNK, count);
  const uint64_t base = msg_off[0], end = msg_off[count];
  if (!c->vk_pk48.ensure((size_t)nkeys * 48) || !c->vk_pk.ensure((size_t)nkeys * sizeof(g1a)) ||
      !c->vk_pkst.ensure((size_t)nkeys * 4) || !c->vk_idx.ensure((size_t)count * 4) ||
      !c->vs_blob.ensure(end ? end : 16) || !c->vs_off.ensure((size_t)(count + 1) * 8) ||
      !c->vs_sig96.ensure((size_t)count * 96) || !c->vs_status.ensure(count) || !c->vs_H.ensure(cap * sizeof(g2a)) ||
      !c->vs_sig.ensure(cap * sizeof(g2a)) || !c->vs_sig_st.ensure(cap * 4) ||
      !c->vk_gslot.ensure((cap + 31) / 32 * 64 * 2 * LDS_FQ6D_PACKED * 4) || !c->fb_sigs.ensure(4))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_verify_sigs_keyed: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->vk_pk48.p, pk48, (size_t)nkeys * 48, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->vk_idx.p, key_idx, (size_t)count * 4, hipMemcpyHostToDevice, s));
  if (total)
    HIPCHK(c, hipMemcpyAsync(c->vs_blob.as<uint8_t>() + base, msg_blob + base, total, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->vs_off.p, msg_off, (size_t)(count + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->vs_sig96.p, sig96, (size_t)count * 96, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(c->fb_sigs.p, 0, 4, s));
  c->fb_last = &c->fb_sigs;
  // the key table once, one lane per key: decode = into_affine (curve + G1 membership), identity allowed
  hipLaunchKernelGGL(k_decompress_shares, dim3((nkeys + 255) / 256), dim3(256), 0, s, c->vk_pk48.as<uint8_t>(),
                     (size_t)nkeys, c->vk_pk.as<g1a>(), c->vk_pkst.as<int32_t>(), 1u, UINT32_MAX, nullptr);
  HIPCHK(c, hipGetLastError());
  if (key_status) HIPCHK(c, hipMemcpyAsync(key_status, c->vk_pkst.p, (size_t)nkeys * 4, hipMemcpyDeviceToHost, s));
  for (uint32_t j0 = 0; j0 < count; j0 += VERIFY_SIGS_CHUNK) {
    const uint32_t m = std::min(VERIFY_SIGS_CHUNK, count - j0);
    uint8_t* st = c->vs_status.as<uint8_t>() + j0;
    {
      // H'_i = [m] hash_g2(msg_i), affine, against -[m] g1 (the coin checks' form)
      timed t_(c, HBX_K_HASH_NONCES, s);
      hipLaunchKernelGGL(k_hash_nonces, dim3((unsigned)(((size_t)m * HASH_K + 63) / 64)), dim3(64), 0, s,
                         c->vs_blob.as<uint8_t>(), c->vs_off.as<uint64_t>() + j0, m, c->vs_H.as<g2a>(), c->digest, 0);
    }
    HIPCHK(c, hipGetLastError());
    {
      // curve membership only: the checks take G2 membership from their Miller loop's [|x|] sigma
      timed t_(c, HBX_K_DECODE_SIGS, s);
      hipLaunchKernelGGL(k_decompress_g2, dim3((m + 63) / 64), dim3(64), 0, s, c->vs_sig96.as<uint8_t>() + (size_t)j0 * 96,
                         (size_t)m, c->vs_sig.as<g2a>(), c->vs_sig_st.as<int32_t>(), 0u);
    }
    HIPCHK(c, hipGetLastError());
    {
      timed t_(c, HBX_K_VERIFY_SIG, s);
      const dim3 grid((m + 31) / 32);
      // Miller loops; the final exponentiation with compressed runs; then the pairs it sent back
      // (SHARE_FALLBACK) once more with Granger-Scott squarings only (hbx_sk_decrypt's pair mode)
      for (uint32_t retry = 0; retry < 2; retry++) {
        hipLaunchKernelGGL(k_verify_sigs2, grid, dim3(64), 0, s, c->vs_H.as<g2a>(), c->vk_pk.as<g1a>(),
                           c->vk_pkst.as<int32_t>(), nkeys, c->vk_idx.as<uint32_t>() + j0, c->vs_sig.as<g2a>(),
                           c->vs_sig_st.as<int32_t>(), m, st, c->vk_gslot.as<uint32_t>(), retry);
        if (retry == 0)
          hipLaunchKernelGGL(k_verify_sig_shares2_fe<true>, grid, dim3(64), 0, s, m, st, c->vk_gslot.as<uint32_t>(),
                             c->force_fallback, c->fb_sigs.as<uint32_t>(), nullptr);
        else
          hipLaunchKernelGGL(k_verify_sig_shares2_fe<false>, grid, dim3(64), 0, s, m, st, c->vk_gslot.as<uint32_t>(), 0u,
                             c->fb_sigs.as<uint32_t>(), nullptr);
      }
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(status + j0, st, m, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_sign_msgs(hbx_ctx* c, const uint8_t* sk32, const uint8_t* msg_blob, const uint64_t* msg_off, uint32_t count,
                  uint8_t* sig96) {
  if (!c || !sk32 || !sig96) return fail(c, HBX_E_INVALID_ARG, "hbx_sign_msgs: bad args");
  uint64_t total = 0;
  if (int rc = msgs_check(c, "hbx_sign_msgs", msg_blob, msg_off, count, &total)) return rc;
  static const uint8_t zero32[32] = {0};
  if (!scalars_canonical(sk32, 1) || memcmp(sk32, zero32, 32) == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_sign_msgs: secret key not in [1, r)");
  HBX_ENTER(c, c->stream);
  const size_t cap = std::min(VERIFY_SIGS_CHUNK, count);
  const uint64_t base = msg_off[0], end = msg_off[count];
  if (!c->vk_sk.ensure(32) || !c->vs_blob.ensure(end ? end : 16) || !c->vs_off.ensure((size_t)(count + 1) * 8) ||
      !c->vs_sig96.ensure((size_t)count * 96) || !c->vs_H.ensure(cap * sizeof(g2a)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_sign_msgs: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->vk_sk.p, sk32, 32, hipMemcpyHostToDevice, s));
  if (total)
    HIPCHK(c, hipMemcpyAsync(c->vs_blob.as<uint8_t>() + base, msg_blob + base, total, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->vs_off.p, msg_off, (size_t)(count + 1) * 8, hipMemcpyHostToDevice, s));
  for (uint32_t j0 = 0; j0 < count; j0 += VERIFY_SIGS_CHUNK) {
    const uint32_t m = std::min(VERIFY_SIGS_CHUNK, count - j0);
    {
      timed t_(c, HBX_K_HASH_NONCES, s);
      hipLaunchKernelGGL(k_hash_nonces, dim3((unsigned)(((size_t)m * HASH_K + 63) / 64)), dim3(64), 0, s,
                         c->vs_blob.as<uint8_t>(), c->vs_off.as<uint64_t>() + j0, m, c->vs_H.as<g2a>(), c->digest, 1);
    }
    HIPCHK(c, hipGetLastError());
    // SecretKey::sign: sk * H_i, one key (n = 1), one message per grid row
    hipLaunchKernelGGL(k_sign, dim3(1, m), dim3(64), 0, s, c->vk_sk.as<uint8_t>(), 1u, c->vs_H.as<g2a>(),
                       c->vs_sig96.as<uint8_t>() + (size_t)j0 * 96);
    HIPCHK(c, hipGetLastError());
  }
  HIPCHK(c, hipMemcpyAsync(sig96, c->vs_sig96.p, (size_t)count * 96, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

// Decode p commitments of degree t and compute their rows at x (device state for the checks).
static int bivar_rows_impl(hbx_ctx* c, const uint8_t* commit48, uint32_t p, uint32_t t, uint64_t x, bool want48) {
  if (!c || !commit48 || p == 0 || t > 4095) return fail(c, HBX_E_INVALID_ARG, "hbx_bivar: bad args");
  HBX_ENTER(c, c->stream);
  const size_t M = (size_t)(t + 1) * (t + 2) / 2, nr = (size_t)p * (t + 1);
  if (!c->bv_commit48.ensure(p * M * 48) || !c->bv_C.ensure(p * M * sizeof(g1a)) || !c->bv_cst.ensure(p * M * 4) ||
      !c->bv_rows.ensure(nr * sizeof(g1j)) || !c->bv_rows48.ensure(nr * 48) || !c->bv_pst.ensure(p))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_bivar: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->bv_commit48.p, commit48, p * M * 48, hipMemcpyHostToDevice, s));
  // decode = into_affine (curve + G1 membership), as a Part's commitment deserialises
  hipLaunchKernelGGL(k_decompress_shares, dim3((unsigned)((p * M + 255) / 256)), dim3(256), 0, s,
                     c->bv_commit48.as<uint8_t>(), p * M, c->bv_C.as<g1a>(), c->bv_cst.as<int32_t>(), 1u, UINT32_MAX,
                     nullptr);
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_bivar_rows, dim3((unsigned)((nr + 63) / 64)), dim3(64), 0, s, c->bv_C.as<g1a>(),
                     c->bv_cst.as<int32_t>(), p, t, x, c->bv_rows.as<g1j>(), want48 ? c->bv_rows48.as<uint8_t>() : nullptr,
                     c->bv_pst.as<uint8_t>());
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

int hbx_bivar_rows(hbx_ctx* c, const uint8_t* commit48, uint32_t p, uint32_t t, uint64_t x, uint8_t* rows48,
                   uint8_t* status) {
  if (!rows48 || !status) return fail(c, HBX_E_INVALID_ARG, "hbx_bivar_rows: null output");
  int rc = bivar_rows_impl(c, commit48, p, t, x, true);
  if (rc) return rc;
  hipStream_t s = pick(c, c->stream);
  stream_scope ss_{c, s};
  HIPCHK(c, hipMemcpyAsync(rows48, c->bv_rows48.p, (size_t)p * (t + 1) * 48, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(status, c->bv_pst.p, p, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_bivar_check_acks(hbx_ctx* c, const uint8_t* commit48, uint32_t p, uint32_t t, uint64_t x,
                         const uint32_t* ack_proposer, const uint64_t* ack_y, const uint8_t* vals32, uint32_t count,
                         uint8_t* status) {
  if (!ack_proposer || !ack_y || !vals32 || !status || count == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_bivar_check_acks: bad args");
  for (uint32_t k = 0; k < count; k++)
    if (ack_proposer[k] >= p) return fail(c, HBX_E_INVALID_ARG, "hbx_bivar_check_acks: proposer %u >= p", ack_proposer[k]);
  int rc = bivar_rows_impl(c, commit48, p, t, x, false);
  if (rc) return rc;
  hipStream_t s = pick(c, c->stream);
  stream_scope ss_{c, s};
  if (!c->bv_ackp.ensure((size_t)count * 4) || !c->bv_acky.ensure((size_t)count * 8) ||
      !c->bv_vals.ensure((size_t)count * 32) || !c->bv_out.ensure(count))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_bivar_check_acks: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->bv_ackp.p, ack_proposer, (size_t)count * 4, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->bv_acky.p, ack_y, (size_t)count * 8, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->bv_vals.p, vals32, (size_t)count * 32, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_bivar_check, dim3((count + 63) / 64), dim3(64), 0, s, c->bv_rows.as<g1j>(),
                     c->bv_pst.as<uint8_t>(), t, c->bv_ackp.as<uint32_t>(), c->bv_acky.as<uint64_t>(),
                     c->bv_vals.as<uint8_t>(), count, c->bv_out.as<uint8_t>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(status, c->bv_out.p, count, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

// combine_signatures + master check + parity of every prepared nonce over the valid shares of
// the last signature-share verification (masked by d_use [I][n] when given): results in
// coin_out96 / coin_comb_st / coin_ok / coin_par.  d_insts (device, `rows` entries): the listed
// instances only, block b = instance d_insts[b]; no other entry of the four results is written.
static int combine_sigs_impl(hbx_ctx* c, const uint8_t* master_pk48, uint32_t t, const uint8_t* d_use, hipStream_t s,
                             const uint32_t* d_insts = nullptr, uint32_t rows = 0) {
  if (!master_pk48 || t == 0 || t > (uint32_t)COMBINE_MAX_T) return fail(c, HBX_E_INVALID_ARG, "hbx_combine_signatures: bad args");
  if (c->coin_n == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "no verified signature shares");
  const uint32_t I = c->coin_I;
  if (!d_insts) rows = I;
  const size_t m = (size_t)I * c->coin_n;
  if (!c->coin_comb.ensure((size_t)I * sizeof(g2a)) || !c->coin_comb_st.ensure((size_t)I * 4) ||
      !c->coin_mpk_comp.ensure(48) || !c->coin_mpk.ensure(sizeof(g1a)) || !c->coin_mpk_st.ensure(4) ||
      !c->coin_ok.ensure(I) || !c->coin_par.ensure(I) || !c->coin_out96.ensure((size_t)I * 96) ||
      (d_use && !c->coin_use.ensure(m)))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_combine_signatures: out of device memory");
  if (c->coin_ready_ev.e) HIPCHK(c, hipStreamWaitEvent(s, c->coin_ready_ev.e, 0));
  // the master key: decoded once per distinct value (era state; checked on the host)
  if (!c->coin_mpk_known || memcmp(c->coin_mpk48, master_pk48, 48) != 0) {
    HIPCHK(c, hipMemcpyAsync(c->coin_mpk_comp.p, master_pk48, 48, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_decompress_g1, dim3(1), dim3(64), 0, s, c->coin_mpk_comp.as<uint8_t>(), 1u, c->coin_mpk.as<g1a>(),
                       c->coin_mpk_st.as<int32_t>());
    HIPCHK(c, hipGetLastError());
    int32_t mst = 0;
    HIPCHK(c, hipMemcpyAsync(&mst, c->coin_mpk_st.p, 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (mst != HBX_PT_OK) return fail(c, HBX_E_INVALID_ARG, "master public key does not decode (status %d)", mst);
    memcpy(c->coin_mpk48, master_pk48, 48);
    c->coin_mpk_known = true;
  }
  const uint8_t* valid = c->coin_valid.as<uint8_t>();
  if (d_use) {
    const size_t mr = (size_t)rows * c->coin_n;
    hipLaunchKernelGGL(k_coin_use, dim3((unsigned)((mr + 255) / 256)), dim3(256), 0, s, valid, d_use, c->coin_n, mr, d_insts,
                       c->coin_use.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    valid = c->coin_use.as<uint8_t>();
  }
  {
    // the G2 combine (waves 0..2) and the master-key identity (wave 3), one block per instance
    timed t_(c, HBX_K_COMBINE_SIGS, s);
    hipLaunchKernelGGL(k_combine_sigs, dim3(rows), dim3(SIGCOMB_THREADS), 0, s, valid, c->coin_sig.as<g2a>(), c->coin_n, t,
                       c->pk.as<g1a>(), c->pk64.as<g1a>(), c->coin_mpk.as<g1a>(), c->coin_comb.as<g2a>(),
                       c->coin_comb_st.as<int32_t>(), c->coin_ok.as<uint8_t>(),
                       c->g1tab.p ? c->g1tab.as<g1a>() : nullptr, d_insts);
  }
  HIPCHK(c, hipGetLastError());
  hipLaunchKernelGGL(k_sig_parity, dim3((rows + 63) / 64), dim3(64), 0, s, c->coin_comb.as<g2a>(),
                     c->coin_comb_st.as<int32_t>(), rows, c->coin_par.as<uint8_t>(), c->coin_out96.as<uint8_t>(), d_insts);
  HIPCHK(c, hipGetLastError());
  return HBX_OK;
}

int hbx_combine_signatures(hbx_ctx* c, const uint8_t* master_pk48, uint32_t t, uint8_t* sig96, int32_t* status,
                           uint8_t* master_ok_bits, uint8_t* parity_bits) {
  if (!c) return HBX_E_INVALID_ARG;
  HBX_ENTER(c, c->stream);
  if (int rc = combine_sigs_impl(c, master_pk48, t, nullptr, s)) return rc;
  const uint32_t I = c->coin_I;
  std::vector<uint8_t> ok(I), par(I);
  std::vector<int32_t> st(I);
  if (sig96) HIPCHK(c, hipMemcpyAsync(sig96, c->coin_out96.p, (size_t)I * 96, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(ok.data(), c->coin_ok.p, I, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(par.data(), c->coin_par.p, I, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(st.data(), c->coin_comb_st.p, (size_t)I * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  if (status) memcpy(status, st.data(), (size_t)I * 4);
  if (master_ok_bits) pack_bits(ok.data(), I, master_ok_bits);
  if (parity_bits) pack_bits(par.data(), I, parity_bits);
  return HBX_OK;
}

int hbx_combine_signatures_d(hbx_ctx* c, const uint8_t* master_pk48, uint32_t t, const uint8_t* d_use, uint8_t* d_sig96,
                             int32_t* d_status, uint8_t* d_master_ok, uint8_t* d_parity, void* stream) {
  if (!c) return HBX_E_INVALID_ARG;
  HBX_ENTER(c, stream);
  if (int rc = combine_sigs_impl(c, master_pk48, t, d_use, s)) return rc;
  const uint32_t I = c->coin_I;
  if (d_sig96) HIPCHK(c, hipMemcpyAsync(d_sig96, c->coin_out96.p, (size_t)I * 96, hipMemcpyDeviceToDevice, s));
  if (d_status) HIPCHK(c, hipMemcpyAsync(d_status, c->coin_comb_st.p, (size_t)I * 4, hipMemcpyDeviceToDevice, s));
  if (d_master_ok) HIPCHK(c, hipMemcpyAsync(d_master_ok, c->coin_ok.p, I, hipMemcpyDeviceToDevice, s));
  if (d_parity) HIPCHK(c, hipMemcpyAsync(d_parity, c->coin_par.p, I, hipMemcpyDeviceToDevice, s));
  return HBX_OK;
}

// ---- Common Coin, incremental (include/hbx.h) -------------------------------------------------
static_assert(hbx_addplan::SHAPE_SENDERS[0] == 64 && hbx_addplan::SHAPE_SENDERS[1] == 32,
              "addplan.hpp and the coin check kernels disagree on a tile's shape");

int hbx_add_sig_shares_d(hbx_ctx* c, const uint8_t* d_sig96, const uint32_t* inst, const uint32_t* sender, uint32_t count,
                         uint32_t n, uint8_t* d_status, void* stream) {
  if (!c || n == 0 || (count && (!d_sig96 || !inst || !sender)))
    return fail(c, HBX_E_INVALID_ARG, "hbx_add_sig_shares_d: bad args");
  if (c->n_keys == 0) return fail(c, HBX_E_NO_KEYS, "hbx_set_pk_shares has not been called");
  if (c->coin_I == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "hbx_add_sig_shares_d: hbx_prepare_nonces has not been called");
  const uint32_t I = c->coin_I;
  if (c->coin_live && n != c->coin_n)
    return fail(c, HBX_E_INVALID_ARG, "hbx_add_sig_shares_d: n=%u but the round's matrix has n=%u", n, c->coin_n);
  hbx_addplan::plan pl;
  if (int rc = add_plan_rejected(c, hbx_addplan::build(inst, sender, count, n, I, UINT32_MAX, pl), "hbx_add_sig_shares_d",
                                 "instance", "an instance index >= %u prepared nonces", I, UINT32_MAX))
    return rc;
  // one stream for the whole call: establishing the matrix is two memsets on it
  HBX_ENTER(c, stream);
  const size_t m = (size_t)n * I;
  if (!c->coin_sig.ensure(m * sizeof(g2a)) || !c->coin_sig_st.ensure(m * 4) || !c->coin_valid.ensure(m))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_add_sig_shares_d: out of device memory");
  if (c->coin_ready_ev.e) HIPCHK(c, hipStreamWaitEvent(s, c->coin_ready_ev.e, 0));  // the nonces' hashes are in
  if (!c->coin_live) {
    // no share has arrived: every entry absent, none decoded (no pairing work)
    HIPCHK(c, hipMemsetAsync(c->coin_valid.p, HBX_SHARE_ABSENT, m, s));
    HIPCHK(c, hipMemsetAsync(c->coin_sig_st.p, 0xFF, m * 4, s));
    c->coin_n = n;
    c->coin_live = true;
  }
  if (count == 0) return HBX_OK;
  add_state& a = c->sig_add;
  if (!a.ensure(m, sizeof(g2a)) || !a.item_st.ensure(count))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_add_sig_shares_d: out of device memory");
  HIPCHK(c, a.begin(m, s));
  // lanes per check from what is live: the matrix call's rule over the touched one-lane tiles
  const int lanes = c->verify_lanes == 1 || c->verify_lanes == 2 ? c->verify_lanes
                    : pl.tiles[0].size() < FILL_WAVES ? 2 : 1;
  const std::vector<hbx_addplan::tile>& tiles = pl.tiles[hbx_addplan::shape_of_lanes(lanes)];
  const uint2 *d_items, *d_tiles;
  if (int rc = add_stage(c, "hbx_add_sig_shares_d", inst, sender, count, tiles, s, &d_items, &d_tiles)) return rc;
  {
    timed t_(c, HBX_K_DECODE_SIGS, s);
    hipLaunchKernelGGL(k_coin_add_decode, dim3((count + 63) / 64), dim3(64), 0, s, d_sig96, d_items, count, n,
                       a.pts.as<g2a>(), a.pt_st.as<int32_t>(), a.mask.as<uint8_t>(), a.item_st.as<uint8_t>());
  }
  HIPCHK(c, hipGetLastError());
  if (pl.live) {
    if (int rc = coin_prepare_lines(c, s)) return rc;
    if (int rc = launch_sig_checks(c, s, lanes, dim3((unsigned)tiles.size(), 1), d_tiles, a.pts.as<g2a>(),
                                   a.pt_st.as<int32_t>(), a.mask.as<uint8_t>(), n, a.verdict.as<uint8_t>()))
      return rc;
  } else {
    c->coin_tiles = 0;
    c->fb_last = nullptr;
  }
  hipLaunchKernelGGL(k_coin_add_merge, dim3((count + 255) / 256), dim3(256), 0, s, d_items, count, n, a.pts.as<g2a>(),
                     a.pt_st.as<int32_t>(), a.verdict.as<uint8_t>(), a.mask.as<uint8_t>(), a.item_st.as<uint8_t>(),
                     c->coin_sig.as<g2a>(), c->coin_sig_st.as<int32_t>(), c->coin_valid.as<uint8_t>(), d_status);
  HIPCHK(c, hipGetLastError());
  a.end();
  return HBX_OK;
}

int hbx_add_sig_shares(hbx_ctx* c, const uint8_t* sig96, const uint32_t* inst, const uint32_t* sender, uint32_t count,
                       uint32_t n, uint8_t* status) {
  return add_host(c, "hbx_add_sig_shares", &hbx_ctx::sig_add, 96, hbx_add_sig_shares_d, sig96, inst, sender, count, n,
                  status);
}

uint32_t hbx_get_coin_tiles_used(const hbx_ctx* c) { return c ? c->coin_tiles : 0; }

int hbx_combine_signatures_insts_d(hbx_ctx* c, const uint8_t* master_pk48, uint32_t t, const uint32_t* insts,
                                   uint32_t ninsts, const uint8_t* d_use, uint8_t* d_sig96, int32_t* d_status,
                                   uint8_t* d_master_ok, uint8_t* d_parity, void* stream) {
  if (!c || (!insts && ninsts)) return fail(c, HBX_E_INVALID_ARG, "hbx_combine_signatures_insts_d: bad args");
  if (int rc = list_check(c, "hbx_combine_signatures_insts_d", "insts", insts, ninsts, c->coin_I, "instance")) return rc;
  if (ninsts == 0) return HBX_OK;
  HBX_ENTER(c, stream);
  // the listed instances, consumed before the call returns (pinned staging, as an add's items)
  const staging st(c, {(size_t)ninsts * 4});
  if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_combine_signatures_insts_d: out of memory (staging)");
  memcpy(st.pin, insts, (size_t)ninsts * 4);
  if (int rc = st.upload(s)) return rc;
  const uint32_t* d_insts = st.dev<uint32_t>(0);
  if (int rc = combine_sigs_impl(c, master_pk48, t, d_use, s, d_insts, ninsts)) return rc;
  if (d_sig96 || d_status || d_master_ok || d_parity) {
    hipLaunchKernelGGL(k_coin_scatter, dim3((ninsts * 96 + 255) / 256), dim3(256), 0, s, d_insts, ninsts,
                       c->coin_out96.as<uint8_t>(), c->coin_comb_st.as<int32_t>(), c->coin_ok.as<uint8_t>(),
                       c->coin_par.as<uint8_t>(), d_sig96, d_status, d_master_ok, d_parity);
    HIPCHK(c, hipGetLastError());
  }
  return HBX_OK;
}

int hbx_combine_signatures_insts(hbx_ctx* c, const uint8_t* master_pk48, uint32_t t, const uint32_t* insts, uint32_t ninsts,
                                 const uint8_t* use, uint8_t* sig96, int32_t* status, uint8_t* master_ok, uint8_t* parity) {
  if (!c || (!insts && ninsts)) return fail(c, HBX_E_INVALID_ARG, "hbx_combine_signatures_insts: bad args");
  if (int rc = list_check(c, "hbx_combine_signatures_insts", "insts", insts, ninsts, c->coin_I, "instance")) return rc;
  if (ninsts == 0) return HBX_OK;
  HBX_ENTER(c, c->stream);
  const uint32_t I = c->coin_I;
  const size_t m = (size_t)I * c->coin_n;
  if (use && m) {
    if (!c->coin_use_in.ensure(m)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_combine_signatures_insts: out of device memory");
    HIPCHK(c, hipMemcpyAsync(c->coin_use_in.p, use, m, hipMemcpyHostToDevice, s));
  }
  if (int rc = hbx_combine_signatures_insts_d(c, master_pk48, t, insts, ninsts, use && m ? c->coin_use_in.as<uint8_t>() : nullptr,
                                              nullptr, nullptr, nullptr, nullptr, s))
    return rc;
  std::vector<uint8_t> out(sig96 ? (size_t)I * 96 : 0), ok(I), par(I);
  std::vector<int32_t> st(I);
  if (sig96) HIPCHK(c, hipMemcpyAsync(out.data(), c->coin_out96.p, (size_t)I * 96, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(ok.data(), c->coin_ok.p, I, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(par.data(), c->coin_par.p, I, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(st.data(), c->coin_comb_st.p, (size_t)I * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  // the listed instances' entries only: nothing else of the caller's arrays is written
  for (uint32_t k = 0; k < ninsts; k++) {
    const uint32_t j = insts[k];
    if (sig96) memcpy(sig96 + (size_t)j * 96, out.data() + (size_t)j * 96, 96);
    if (status) status[j] = st[j];
    if (master_ok) master_ok[j] = ok[j];
    if (parity) parity[j] = par[j];
  }
  return HBX_OK;
}

int hbx_get_ct_valid_d(hbx_ctx* c, uint8_t* d_ct_valid, void* stream) {
  if (!c || !d_ct_valid) return fail(c, HBX_E_INVALID_ARG, "hbx_get_ct_valid_d: bad args");
  if (c->p_ct == 0 || !c->ct_known) return fail(c, HBX_E_NO_CIPHERTEXTS, "ciphertext validity not computed yet");
  HBX_ENTER(c, stream);
  HIPCHK(c, hipMemcpyAsync(d_ct_valid, c->ct_valid.p, c->p_ct, hipMemcpyDeviceToDevice, s));
  return HBX_OK;
}

// The combine of every proposer (cols = nullptr), or of the `ncols` listed ones: the blocks of
// proposer cols[b] only, so no other status entry or plaintext range is written.
static int combine_impl(hbx_ctx* c, uint32_t t, uint8_t* d_out_blob, int32_t* d_status, void* stream,
                        const uint32_t* cols, uint32_t ncols) {
  if (!c || t == 0 || t > (uint32_t)COMBINE_MAX_T || !d_out_blob || (ncols && !cols))
    return fail(c, HBX_E_INVALID_ARG, "hbx_combine_decrypt_d: bad args");
  if (c->n_shares == 0 || c->p_ct == 0 || !c->ct_known || c->verified_p != c->p_ct)
    return fail(c, HBX_E_NO_CIPHERTEXTS, "no verified shares for the prepared ciphertexts");
  const uint32_t p = c->p_ct;
  if (cols) {
    if (int rc = list_check(c, "hbx_combine_decrypt_cols_d", "cols", cols, ncols, p, "proposer")) return rc;
    if (ncols == 0) return HBX_OK;
  }
  HBX_ENTER(c, stream);
  // the listed columns, consumed before the call returns (pinned staging, as the ragged descriptors)
  const uint32_t* d_cols = nullptr;
  const uint32_t pl = cols ? ncols : p;  // proposers of this launch
  if (cols) {
    const staging st(c, {(size_t)ncols * 4});
    if (!st.pin) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_combine_decrypt_cols_d: out of memory (staging)");
    memcpy(st.pin, cols, (size_t)ncols * 4);
    if (int rc = st.upload(s)) return rc;
    d_cols = st.dev<uint32_t>(0);
  }
  if (!c->keys.ensure((size_t)p * 32) || !c->status.ensure((size_t)p * 4))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_combine_decrypt_d: out of device memory");
  {
    timed t_(c, HBX_K_COMBINE, s);
    // a quad of lanes per GLV term over one-wave blocks when that still leaves at most one wave per
    // SIMD (an epoch shard; k_combine_q), else one lane per term in one block per proposer
    const uint32_t nb = (2 * t + COMBQ_TERMS - 1) / COMBQ_TERMS;
    const bool quads = combine_quads(c, t, pl);
    // terms without tables, counted per proposer (every block writes its entry)
    if (!c->comb_slow.ensure((size_t)p * 4)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_combine_decrypt_d: out of device memory");
    c->comb_slow_p = p;
    if (cols) HIPCHK(c, hipMemsetAsync(c->comb_slow.p, 0, (size_t)p * 4, s));  // only the listed entries are written
    // window tables of the last fused prepare, if they are of these shares
    const bool tabs = c->tab_ready && c->tab_n == c->n_shares && c->tab_p == p;
    if (quads) {
      if (!c->comb_partial.ensure((size_t)p * nb * sizeof(g1j)) || !c->comb_done.ensure((size_t)p * 4))
        return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_combine_decrypt_d: out of device memory");
      HIPCHK(c, hipMemsetAsync(c->comb_done.p, 0, (size_t)p * 4, s));
      hipLaunchKernelGGL(k_combine_q, dim3(nb, pl), dim3(64), 0, s, c->valid.as<uint8_t>(), c->S.as<g1a>(),
                         c->n_shares, t, c->ct_valid.as<uint8_t>(), c->keys.as<uint32_t>(), c->status.as<int32_t>(),
                         c->digest, c->comb_partial.as<g1j>(), c->comb_done.as<uint32_t>(), c->comb_slow.as<uint32_t>(),
                         d_cols);
    } else
    hipLaunchKernelGGL(k_combine, dim3(pl), dim3(COMBINE_THREADS), 0, s, c->valid.as<uint8_t>(), c->S.as<g1a>(),
                       c->n_shares, t, c->ct_valid.as<uint8_t>(), c->keys.as<uint32_t>(), c->status.as<int32_t>(),
                       c->digest, tabs ? c->comb_tab.as<g1jd>() : nullptr, c->comb_tab_ok.as<uint8_t>(),
                       tabs ? c->tab_cap : 0u, c->tab_me, c->tab_form, c->comb_slow.as<uint32_t>(), d_cols);
  }
  HIPCHK(c, hipGetLastError());
  const uint64_t blocks = (c->max_v_len + 15) / 16;
  if (blocks) {
    hipLaunchKernelGGL(k_keystream_xor, dim3((unsigned)((blocks + 63) / 64), pl), dim3(64), 0, s,
                       c->keys.as<uint32_t>(), c->status.as<int32_t>(), c->d_v_blob, c->d_v_off, d_out_blob, d_cols);
    HIPCHK(c, hipGetLastError());
  }
  if (d_status && !cols) HIPCHK(c, hipMemcpyAsync(d_status, c->status.p, (size_t)p * 4, hipMemcpyDeviceToDevice, s));
  if (d_status && cols) {
    hipLaunchKernelGGL(k_scatter_cols, dim3((ncols + 63) / 64), dim3(64), 0, s, c->status.as<int32_t>(), d_cols, ncols,
                       d_status);
    HIPCHK(c, hipGetLastError());
  }
  return HBX_OK;
}

int hbx_combine_decrypt_d(hbx_ctx* c, uint32_t t, uint8_t* d_out_blob, int32_t* d_status, void* stream) {
  return combine_impl(c, t, d_out_blob, d_status, stream, nullptr, 0);
}

int hbx_combine_decrypt_cols_d(hbx_ctx* c, uint32_t t, const uint32_t* cols, uint32_t ncols, uint8_t* d_out_blob,
                               int32_t* d_status, void* stream) {
  if (!c || (!cols && ncols)) return fail(c, HBX_E_INVALID_ARG, "hbx_combine_decrypt_cols_d: bad args");
  if (ncols == 0) return HBX_OK;
  static const uint32_t none = 0;
  return combine_impl(c, t, d_out_blob, d_status, stream, cols ? cols : &none, ncols);
}

int hbx_decrypt_epoch_d(hbx_ctx* c, const uint8_t* d_u_comp, const uint8_t* d_v_blob, const uint64_t* d_v_off,
                        const uint8_t* d_w_comp, uint32_t p, uint64_t max_v_len, const uint8_t* d_shares,
                        const uint8_t* d_present, uint32_t n, uint32_t t, uint8_t* d_valid, uint8_t* d_ct_valid,
                        uint8_t* d_out_blob, int32_t* d_status, void* stream) {
  if (!c || !d_shares || n == 0 || p == 0 || t == 0 || t > (uint32_t)COMBINE_MAX_T || !d_out_blob)
    return fail(c, HBX_E_INVALID_ARG, "hbx_decrypt_epoch_d: bad args");
  if (c->n_keys == 0) return fail(c, HBX_E_NO_KEYS, "hbx_set_pk_shares has not been called");
  // Stages in stream order.  (Running Ciphertext::verify on the aux stream beside a speculative
  // combine was measured on MI355X and gained nothing: the combine's 4 waves per proposer already
  // occupy every SIMD, and two single-wave-per-SIMD kernels only time-share the VALU.)
  // The combine's window tables are made beside the line preparation, whose chains leave most of
  // the chip idle (k_prepare_lines); the combine falls back per term where a table is missing.
  int rc = prepare_impl(c, d_u_comp, d_v_blob, d_v_off, d_w_comp, p, max_v_len, nullptr, stream, d_shares, n,
                        combine_tab_cap(c, n, t, p));
  if (rc) return rc;
  rc = verify_impl(c, d_shares, d_present, n, p, d_valid, stream, true);
  if (rc) return rc;
  if (d_ct_valid) {
    rc = hbx_get_ct_valid_d(c, d_ct_valid, stream);
    if (rc) return rc;
  }
  return hbx_combine_decrypt_d(c, t, d_out_blob, d_status, stream);
}

// The host forms of the combine, on the context's stream: the offsets read back into `off`, out_own
// sized, the _d call over `cols` (nullptr: every proposer, into a zeroed out_own and on to out_blob),
// the statuses read back into `st`; synchronised at return.
static int combine_host(hbx_ctx* c, uint32_t t, const uint32_t* cols, uint32_t ncols, uint8_t* out_blob,
                        std::vector<uint64_t>& off, std::vector<int32_t>& st) {
  const uint32_t p = c->p_ct;
  if (p == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "no ciphertexts prepared");
  off.resize(p + 1);
  HIPCHK(c, hipMemcpyAsync(off.data(), c->d_v_off, off.size() * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const uint64_t total = off[p];
  if (!c->out_own.ensure(total ? total : 16)) return fail(c, HBX_E_OUT_OF_MEMORY, "out of device memory");
  if (!cols) HIPCHK(c, hipMemsetAsync(c->out_own.p, 0, total ? total : 16, c->stream));
  int rc = cols ? hbx_combine_decrypt_cols_d(c, t, cols, ncols, c->out_own.as<uint8_t>(), nullptr, c->stream)
                : hbx_combine_decrypt_d(c, t, c->out_own.as<uint8_t>(), nullptr, c->stream);
  if (rc) return rc;
  if (!cols && total) HIPCHK(c, hipMemcpyAsync(out_blob, c->out_own.p, total, hipMemcpyDeviceToHost, c->stream));
  st.resize(p);
  HIPCHK(c, hipMemcpyAsync(st.data(), c->status.p, (size_t)p * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

int hbx_combine_decrypt(hbx_ctx* c, uint32_t t, uint8_t* out_blob, int32_t* status) {
  if (!c || !out_blob) return fail(c, HBX_E_INVALID_ARG, "hbx_combine_decrypt: bad args");
  HBX_ENTER(c, c->stream);
  std::vector<uint64_t> off;
  std::vector<int32_t> st;
  if (int rc = combine_host(c, t, nullptr, 0, out_blob, off, st)) return rc;
  if (status) memcpy(status, st.data(), st.size() * 4);
  return HBX_OK;
}

int hbx_combine_decrypt_cols(hbx_ctx* c, uint32_t t, const uint32_t* cols, uint32_t ncols, uint8_t* out_blob,
                             int32_t* status) {
  if (!c || !out_blob || (!cols && ncols)) return fail(c, HBX_E_INVALID_ARG, "hbx_combine_decrypt_cols: bad args");
  if (ncols == 0) return HBX_OK;
  HBX_ENTER(c, c->stream);
  std::vector<uint64_t> off;
  std::vector<int32_t> st;
  if (int rc = combine_host(c, t, cols, ncols, out_blob, off, st)) return rc;
  // the listed proposers' entries and ranges only: nothing else of the caller's buffers is written
  // (a proposer that did not decrypt has no plaintext: its range stays as the caller had it)
  for (uint32_t k = 0; k < ncols; k++) {
    const uint64_t a = off[cols[k]], b = off[cols[k] + 1];
    if (status) status[cols[k]] = st[cols[k]];
    if (st[cols[k]] == 0 && b > a)
      HIPCHK(c, hipMemcpyAsync(out_blob + a, c->out_own.as<uint8_t>() + a, b - a, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

// ---- incremental share verification (include/hbx.h) ---------------------------------------------
// addplan.hpp states the check kernels' tile shapes for the host: the two must agree
static_assert(hbx_addplan::SHAPE_SENDERS[2] == (uint32_t)G3_PER_WAVE && hbx_addplan::SHAPE_SENDERS[3] == (uint32_t)G6_PER_WAVE &&
                  sizeof(hbx_addplan::tile) == sizeof(uint2),
              "addplan.hpp and the check kernels disagree on a tile's shape");

int hbx_add_dec_shares_d(hbx_ctx* c, const uint8_t* d_shares48, const uint32_t* proposer, const uint32_t* sender,
                         uint32_t count, uint32_t n, uint8_t* d_status, void* stream) {
  if (!c || n == 0 || (count && (!d_shares48 || !proposer || !sender)))
    return fail(c, HBX_E_INVALID_ARG, "hbx_add_dec_shares_d: bad args");
  if (c->n_keys == 0) return fail(c, HBX_E_NO_KEYS, "hbx_set_pk_shares has not been called");
  if (c->p_ct == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "hbx_add_dec_shares_d: no ciphertexts prepared");
  const uint32_t p = c->p_ct;
  const bool established = c->n_shares != 0 && c->verified_p == p;
  if (established && n != c->n_shares)
    return fail(c, HBX_E_INVALID_ARG, "hbx_add_dec_shares_d: n=%u but the epoch's matrix has n=%u", n, c->n_shares);
  const uint32_t me = (c->own_ready && c->own_me < n) ? c->own_me : UINT32_MAX;
  hbx_addplan::plan pl;
  if (int rc = add_plan_rejected(c, hbx_addplan::build(proposer, sender, count, n, p, me, pl), "hbx_add_dec_shares_d",
                                 "proposer", "a proposer index >= p=%u", p, me))
    return rc;
  // the device only: establishing the matrix is an entry of its own on the caller's stream
  // (verify_impl), so this call picks the stream before it and again after it
  HBX_DEVICE(c);
  const size_t m = (size_t)n * p;
  if (!established) {
    // the matrix call with every share absent: own-share mode's entries and checks, a deferred
    // Ciphertext::verify, the batched mode's call index -- whatever that call does on this context
    if (!c->add_zero.ensure(m * 49)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_add_dec_shares_d: out of device memory");
    hipStream_t s0 = pick(c, stream);
    {
      stream_scope ss0_{c, s0};
      HIPCHK(c, hipMemsetAsync(c->add_zero.p, 0, m * 49, s0));
    }
    int rc = verify_impl(c, c->add_zero.as<uint8_t>(), c->add_zero.as<uint8_t>() + m * 48, n, p, nullptr, stream, false);
    if (rc) return rc;
  }
  if (count == 0) return HBX_OK;
  hipStream_t s = pick(c, stream);
  stream_scope ss_{c, s};
  add_state& a = c->dec_add;
  if (!a.ensure(m, sizeof(g1a))) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_add_dec_shares_d: out of device memory");
  HIPCHK(c, a.begin(m, s));
  // lanes per check from what is live: the matrix call's ladder over the touched-tile counts
  const int lanes = c->verify_lanes ? c->verify_lanes : hbx_addplan::lanes_of(pl);
  const std::vector<hbx_addplan::tile>& tiles = pl.tiles[hbx_addplan::shape_of_lanes(lanes)];
  const uint2 *d_items, *d_tiles;
  if (int rc = add_stage(c, "hbx_add_dec_shares_d", proposer, sender, count, tiles, s, &d_items, &d_tiles)) return rc;
  c->tab_ready = false;  // S is about to hold other shares than the tables were made from
  const unsigned item_blocks = (count + 255) / 256;
  {
    timed t_(c, HBX_K_VERIFY_SHARES, s);
    c->verify_tiles = (uint32_t)tiles.size();
    if (pl.live) {
      hipLaunchKernelGGL(k_add_decode, dim3(item_blocks), dim3(256), 0, s, d_shares48, d_items, count, n, a.pts.as<g1a>(),
                         a.pt_st.as<int32_t>(), a.mask.as<uint8_t>());
      HIPCHK(c, hipGetLastError());
      c->lanes_used = lanes;
      // the add's own items always run the per-share checks (ct_ok, not a batched call's gate); the
      // own lane and the ciphertexts were decided when the matrix was established
      if (int rc = launch_share_checks(c, s, lanes, dim3((unsigned)tiles.size(), 1), d_tiles, a.pts.as<g1a>(),
                                       a.pt_st.as<int32_t>(), a.mask.as<uint8_t>(), a.verdict.as<uint8_t>(),
                                       c->ct_ok.as<uint8_t>(), n, UINT32_MAX, nullptr))
        return rc;
      HIPCHK(c, hipGetLastError());
    } else {
      c->fb_last = nullptr;
    }
    hipLaunchKernelGGL(k_add_merge, dim3(item_blocks), dim3(256), 0, s, d_items, count, n, a.pts.as<g1a>(),
                       a.pt_st.as<int32_t>(), a.verdict.as<uint8_t>(), a.mask.as<uint8_t>(), c->ct_valid.as<uint8_t>(),
                       c->S.as<g1a>(), c->S_status.as<int32_t>(), c->valid.as<uint8_t>(), d_status);
  }
  HIPCHK(c, hipGetLastError());
  a.end();
  return HBX_OK;
}

int hbx_add_dec_shares(hbx_ctx* c, const uint8_t* shares48, const uint32_t* proposer, const uint32_t* sender,
                       uint32_t count, uint32_t n, uint8_t* status) {
  return add_host(c, "hbx_add_dec_shares", &hbx_ctx::dec_add, 48, hbx_add_dec_shares_d, shares48, proposer, sender, count,
                  n, status);
}

uint32_t hbx_get_verify_tiles_used(const hbx_ctx* c) { return c ? c->verify_tiles : 0; }

// ---- status readout ---------------------------------------------------------------------------
static int copy_status(hbx_ctx* c, const dbuf& b, size_t have, uint8_t* out, size_t count, const char* what) {
  if (!out) return fail(c, HBX_E_INVALID_ARG, "%s: null output", what);
  if (have == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "%s: nothing computed yet", what);
  if (count != have) return fail(c, HBX_E_INVALID_ARG, "%s: count %zu, expected %zu", what, count, have);
  HBX_DEVICE(c);
  HIPCHK(c, quiesce(c));  // the last results may have been enqueued on a caller's stream
  HIPCHK(c, hipMemcpy(out, b.p, have, hipMemcpyDeviceToHost));
  return HBX_OK;
}

int hbx_get_share_status(hbx_ctx* c, uint8_t* status, size_t count) {
  if (!c) return HBX_E_INVALID_ARG;
  return copy_status(c, c->valid, (size_t)c->n_shares * c->verified_p, status, count, "hbx_get_share_status");
}

int hbx_get_ct_status(hbx_ctx* c, uint8_t* status, size_t count) {
  if (!c) return HBX_E_INVALID_ARG;
  return copy_status(c, c->ct_valid, c->ct_known ? c->p_ct : 0, status, count, "hbx_get_ct_status");
}

int hbx_get_ct_hashes(hbx_ctx* c, uint8_t* h96, size_t count) {
  if (!c || !h96) return fail(c, HBX_E_INVALID_ARG, "hbx_get_ct_hashes: bad args");
  if (c->p_ct == 0) return fail(c, HBX_E_NO_CIPHERTEXTS, "hbx_get_ct_hashes: no ciphertexts prepared");
  if (count != c->p_ct) return fail(c, HBX_E_INVALID_ARG, "hbx_get_ct_hashes: count %zu, expected %u", count, c->p_ct);
  HBX_DEVICE(c);
  HIPCHK(c, quiesce(c));
  dbuf out;
  if (!out.ensure(count * 96)) return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_get_ct_hashes: out of device memory");
  // Hj holds H' = h_eff P = [3(x^2-1)] H (k_prepare_ct); the reference's H = h2 P from it
  hipLaunchKernelGGL(k_true_hashes, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, c->stream, c->G2pts.as<g2a>(),
                     c->Hj.as<g2j>(), (uint32_t)count, out.as<uint8_t>());
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e == hipSuccess) e = hipMemcpy(h96, out.p, count * 96, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(c, HBX_E_DEVICE, "hbx_get_ct_hashes: %s", hipGetErrorString(e));
  return HBX_OK;
}

int hbx_get_sig_share_status(hbx_ctx* c, uint8_t* status, size_t count) {
  if (!c) return HBX_E_INVALID_ARG;
  return copy_status(c, c->coin_valid, (size_t)c->coin_n * c->coin_I, status, count, "hbx_get_sig_share_status");
}

// ---- producer side --------------------------------------------------------------------------
static bool scalars_canonical(const uint8_t* s32, size_t count) {
  static const uint8_t R_BE[32] = {0x73, 0xed, 0xa7, 0x53, 0x29, 0x9d, 0x7d, 0x48, 0x33, 0x39, 0xd8,
                                   0x08, 0x09, 0xa1, 0xd8, 0x05, 0x53, 0xbd, 0xa4, 0x02, 0xff, 0xfe,
                                   0x5b, 0xfe, 0xff, 0xff, 0xff, 0xff, 0x00, 0x00, 0x00, 0x01};
  for (size_t k = 0; k < count; k++)
    if (memcmp(s32 + 32 * k, R_BE, 32) >= 0) return false;
  return true;
}

int hbx_public_keys(hbx_ctx* c, const uint8_t* sk32, uint32_t n, uint8_t* pk48) {
  if (!c || !sk32 || !pk48 || n == 0) return fail(c, HBX_E_INVALID_ARG, "hbx_public_keys: bad args");
  if (!scalars_canonical(sk32, n)) return fail(c, HBX_E_INVALID_ARG, "hbx_public_keys: scalar >= r");
  HBX_ENTER(c, c->stream);
  dbuf dsk, dpk;
  if (!dsk.ensure((size_t)n * 32) || !dpk.ensure((size_t)n * 48))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_public_keys: out of device memory");
  int rc = HBX_OK;
  if (hipMemcpyAsync(dsk.p, sk32, (size_t)n * 32, hipMemcpyHostToDevice, c->stream) != hipSuccess) rc = HBX_E_DEVICE;
  if (rc == HBX_OK) {
    hipLaunchKernelGGL(k_public_keys, dim3((n + 63) / 64), dim3(64), 0, c->stream, dsk.as<uint8_t>(), n,
                       dpk.as<uint8_t>());
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(pk48, dpk.p, (size_t)n * 48, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
      rc = HBX_E_DEVICE;
  }
  return rc ? fail(c, rc, "hbx_public_keys: device error") : HBX_OK;
}

int hbx_encrypt(hbx_ctx* c, const uint8_t* pk48, const uint8_t* msg_blob, const uint64_t* msg_off, uint32_t p,
                const uint8_t* r32, uint8_t* u48, uint8_t* v_blob, uint8_t* w96) {
  if (!c || !pk48 || !msg_off || !r32 || !u48 || !w96 || p == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt: bad args");
  if (!scalars_canonical(r32, p)) return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt: scalar >= r");
  for (uint32_t j = 0; j < p; j++)
    if (msg_off[j + 1] < msg_off[j]) return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt: msg_off not monotone");
  const uint64_t total = msg_off[p];
  if (total && (!msg_blob || !v_blob)) return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt: bad args");
  HBX_ENTER(c, c->stream);
  dbuf dpkc, dpk, dst, dr, dm, doff, du, dv, dw;
  if (!dpkc.ensure(48) || !dpk.ensure(sizeof(g1a)) || !dst.ensure(4) || !dr.ensure((size_t)p * 32) ||
      !dm.ensure(total) || !doff.ensure((size_t)(p + 1) * 8) || !du.ensure((size_t)p * 48) || !dv.ensure(total) ||
      !dw.ensure((size_t)p * 96))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_encrypt: out of device memory");
  int rc = HBX_OK;
  int32_t st = 0;
  bool ok = hipMemcpyAsync(dpkc.p, pk48, 48, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
            hipMemcpyAsync(dr.p, r32, (size_t)p * 32, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
            hipMemcpyAsync(doff.p, msg_off, (size_t)(p + 1) * 8, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
            (total == 0 || hipMemcpyAsync(dm.p, msg_blob, total, hipMemcpyHostToDevice, c->stream) == hipSuccess);
  if (ok) {
    hipLaunchKernelGGL(k_decompress_g1, dim3(1), dim3(64), 0, c->stream, dpkc.as<uint8_t>(), 1u, dpk.as<g1a>(),
                       dst.as<int32_t>());
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(&st, dst.p, 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
         hipStreamSynchronize(c->stream) == hipSuccess;
  }
  if (ok && st != HBX_PT_OK)
    return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt: public key does not decode (status %d)", st);
  if (ok) {
    hipLaunchKernelGGL(k_encrypt, dim3((p + 63) / 64), dim3(64), 0, c->stream, dpk.as<g1a>(), dr.as<uint8_t>(),
                       dm.as<uint8_t>(), doff.as<uint64_t>(), p, du.as<uint8_t>(), dv.as<uint8_t>(), dw.as<uint8_t>(),
                       c->digest);
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(u48, du.p, (size_t)p * 48, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
         hipMemcpyAsync(w96, dw.p, (size_t)p * 96, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
         (total == 0 || hipMemcpyAsync(v_blob, dv.p, total, hipMemcpyDeviceToHost, c->stream) == hipSuccess) &&
         hipStreamSynchronize(c->stream) == hipSuccess;
  }
  if (!ok) rc = HBX_E_DEVICE;
  return rc ? fail(c, rc, "hbx_encrypt: device error") : HBX_OK;
}

int hbx_decrypt_shares(hbx_ctx* c, const uint8_t* sk32, uint32_t n, const uint8_t* u48, uint32_t p,
                       uint8_t* shares48) {
  if (!c || !sk32 || !u48 || !shares48 || n == 0 || p == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_decrypt_shares: bad args");
  if (!scalars_canonical(sk32, n)) return fail(c, HBX_E_INVALID_ARG, "hbx_decrypt_shares: scalar >= r");
  HBX_ENTER(c, c->stream);
  const size_t m = (size_t)n * p;
  dbuf dsk, duc, du, dst, dout;
  if (!dsk.ensure((size_t)n * 32) || !duc.ensure((size_t)p * 48) || !du.ensure((size_t)p * sizeof(g1a)) ||
      !dst.ensure((size_t)p * 4) || !dout.ensure(m * 48))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_decrypt_shares: out of device memory");
  std::vector<int32_t> st(p);
  bool ok = hipMemcpyAsync(dsk.p, sk32, (size_t)n * 32, hipMemcpyHostToDevice, c->stream) == hipSuccess &&
            hipMemcpyAsync(duc.p, u48, (size_t)p * 48, hipMemcpyHostToDevice, c->stream) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(k_decompress_g1, dim3((p + 63) / 64), dim3(64), 0, c->stream, duc.as<uint8_t>(), p,
                       du.as<g1a>(), dst.as<int32_t>());
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(st.data(), dst.p, (size_t)p * 4, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
         hipStreamSynchronize(c->stream) == hipSuccess;
  }
  for (uint32_t j = 0; ok && j < p; j++)
    if (st[j] != HBX_PT_OK && st[j] != HBX_PT_INFINITY)
      return fail(c, HBX_E_INVALID_ARG, "hbx_decrypt_shares: U_%u does not decode (status %d)", j, st[j]);
  if (ok) {
    hipLaunchKernelGGL(k_decrypt_shares, dim3((n + 63) / 64, p), dim3(64), 0, c->stream, dsk.as<uint8_t>(), n,
                       du.as<g1a>(), dout.as<uint8_t>());
    ok = hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(shares48, dout.p, m * 48, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
         hipStreamSynchronize(c->stream) == hipSuccess;
  }
  return ok ? HBX_OK : fail(c, HBX_E_DEVICE, "hbx_decrypt_shares: device error");
}

// ---- SyncKeyGen (src/sync_key_gen.rs) beyond the commitment checks -----------------------------
namespace {
// Ciphertexts per Ciphertext::verify pass of hbx_sk_decrypt.  The prepared-ciphertext state is about
// 100 KiB per ciphertext (two sets of 2 x 68 Miller lines and their scratch), so 1024 bound it near
// 100 MiB however many ciphertexts a call brings (N^2 = 65,536 at N = 256).  A larger chunk would not
// run faster: the wide check gives a ciphertext-only job a whole 128-thread block (one 16-lane group
// of its eight busy) and 45 KiB of LDS, so about 768 blocks are resident at a time.
constexpr uint32_t SK_DECRYPT_CHUNK = 1024;
// Ciphertexts per pass in HBX_CT_CHECK_PAIR mode (hbbft_amd/hbx.py SK_DECRYPT_PAIR_CHUNK is the same
// number).  The state is about 2 KiB per ciphertext (U, W and H' decoded, the Jacobian H', and the
// pair's 1.25 KiB slot for the halves of f): 16,384 ciphertexts are about 35 MB, 512 pair-check
// waves (one wave per SIMD resident: two full-chip rounds) and 4,096 hash waves.
constexpr uint32_t SK_DECRYPT_PAIR_CHUNK = 16384;

void be32_to_limbs(const uint8_t* b, uint32_t* k8) {
  for (int q = 0; q < 8; q++)
    k8[q] = ((uint32_t)b[28 - 4 * q] << 24) | ((uint32_t)b[29 - 4 * q] << 16) | ((uint32_t)b[30 - 4 * q] << 8) | b[31 - 4 * q];
}
}  // namespace

int hbx_encrypt_to(hbx_ctx* c, const uint8_t* pk48, const uint8_t* msg_blob, const uint64_t* msg_off, uint32_t count,
                   const uint8_t* r32, uint8_t* u48, uint8_t* v_blob, uint8_t* w96) {
  if (!c || !pk48 || !msg_off || !r32 || !u48 || !w96 || count == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt_to: bad args");
  if (!scalars_canonical(r32, count)) return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt_to: scalar >= r");
  for (uint32_t j = 0; j < count; j++)
    if (msg_off[j + 1] < msg_off[j]) return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt_to: msg_off not monotone");
  const uint64_t total = msg_off[count];
  if (total && (!msg_blob || !v_blob)) return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt_to: bad args");
  HBX_ENTER(c, c->stream);
  dbuf dpkc, dpk, dst, dr, dm, doff, du, dv, dw;
  if (!dpkc.ensure((size_t)count * 48) || !dpk.ensure((size_t)count * sizeof(g1a)) || !dst.ensure((size_t)count * 4) ||
      !dr.ensure((size_t)count * 32) || !dm.ensure(total) || !doff.ensure((size_t)(count + 1) * 8) ||
      !du.ensure((size_t)count * 48) || !dv.ensure(total) || !dw.ensure((size_t)count * 96))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_encrypt_to: out of device memory");
  HIPCHK(c, hipMemcpyAsync(dpkc.p, pk48, (size_t)count * 48, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(dr.p, r32, (size_t)count * 32, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(doff.p, msg_off, (size_t)(count + 1) * 8, hipMemcpyHostToDevice, s));
  if (total) HIPCHK(c, hipMemcpyAsync(dm.p, msg_blob, total, hipMemcpyHostToDevice, s));
  // decode = into_affine (curve + G1 membership), as a PublicKey deserialises
  hipLaunchKernelGGL(k_decompress_shares, dim3((count + 255) / 256), dim3(256), 0, s, dpkc.as<uint8_t>(), (size_t)count,
                     dpk.as<g1a>(), dst.as<int32_t>(), 1u, UINT32_MAX, nullptr);
  HIPCHK(c, hipGetLastError());
  std::vector<int32_t> st(count);
  HIPCHK(c, hipMemcpyAsync(st.data(), dst.p, (size_t)count * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (uint32_t j = 0; j < count; j++)
    if (st[j] != HBX_PT_OK)
      return fail(c, HBX_E_INVALID_ARG, "hbx_encrypt_to: public key %u does not decode (status %d)", j, st[j]);
  hipLaunchKernelGGL(k_encrypt_to, dim3((count + 63) / 64), dim3(64), 0, s, dpk.as<g1a>(), dr.as<uint8_t>(),
                     dm.as<uint8_t>(), doff.as<uint64_t>(), count, du.as<uint8_t>(), dv.as<uint8_t>(), dw.as<uint8_t>(),
                     c->digest);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(u48, du.p, (size_t)count * 48, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipMemcpyAsync(w96, dw.p, (size_t)count * 96, hipMemcpyDeviceToHost, s));
  if (total) HIPCHK(c, hipMemcpyAsync(v_blob, dv.p, total, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_sk_decrypt(hbx_ctx* c, const uint8_t* sk32, const uint8_t* u48, const uint8_t* v_blob, const uint64_t* v_off,
                   const uint8_t* w96, uint32_t count, uint8_t* out_blob, uint8_t* status) {
  if (!c || !sk32 || !u48 || !v_off || !w96 || !status || count == 0)
    return fail(c, HBX_E_INVALID_ARG, "hbx_sk_decrypt: bad args");
  if (!scalars_canonical(sk32, 1)) return fail(c, HBX_E_INVALID_ARG, "hbx_sk_decrypt: scalar >= r");
  uint64_t maxv = 0;
  for (uint32_t j = 0; j < count; j++) {
    if (v_off[j + 1] < v_off[j]) return fail(c, HBX_E_INVALID_ARG, "hbx_sk_decrypt: v_off not monotone");
    maxv = std::max<uint64_t>(maxv, v_off[j + 1] - v_off[j]);
  }
  const uint64_t total = v_off[count];
  if (total && (!v_blob || !out_blob)) return fail(c, HBX_E_INVALID_ARG, "hbx_sk_decrypt: bad args");
  HBX_ENTER(c, c->stream);
  if (!c->u_comp_own.ensure((size_t)count * 48) || !c->w_comp_own.ensure((size_t)count * 96) ||
      !c->v_off_own.ensure((size_t)(count + 1) * 8) || !c->v_blob_own.ensure(total ? total : 16) ||
      !c->kg_out.ensure(total ? total : 16) || !c->kg_st.ensure(count) || !c->kg_sk.ensure(32))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_sk_decrypt: out of device memory");
  uint32_t limbs[8];
  be32_to_limbs(sk32, limbs);
  // an earlier call's kernels may still read kg_sk
  HIPCHK(c, quiesce(c));
  HIPCHK(c, hipMemcpy(c->kg_sk.p, limbs, 32, hipMemcpyHostToDevice));
  HIPCHK(c, hipMemcpyAsync(c->u_comp_own.p, u48, (size_t)count * 48, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->w_comp_own.p, w96, (size_t)count * 96, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(c->v_off_own.p, v_off, (size_t)(count + 1) * 8, hipMemcpyHostToDevice, s));
  if (total) HIPCHK(c, hipMemcpyAsync(c->v_blob_own.p, v_blob, total, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemsetAsync(c->kg_out.p, 0, total ? total : 16, s));
  // Ciphertext::verify, a chunk at a time: through the prepared-ciphertext path with its immediate
  // checks (the wide executor), or, in HBX_CT_CHECK_PAIR mode, k_prepare_ct alone and one lane pair per
  // ciphertext, without the line tables.  `sk32` is the node's individual key, not its threshold share:
  // own-share mode is off for these prepares and restored below; the epoch's prepared ciphertexts
  // are void afterwards.
  const bool pair = c->ct_check == HBX_CT_CHECK_PAIR;
  c->ct_check_used = c->ct_check;
  const uint32_t chunk = pair ? SK_DECRYPT_PAIR_CHUNK : SK_DECRYPT_CHUNK;
  if (pair) {
    const size_t cap = std::min(chunk, count);
    if (!c->U.ensure(cap * sizeof(g1a)) || !c->G2pts.ensure(2 * cap * sizeof(g2a)) || !c->Hj.ensure(cap * sizeof(g2j)) ||
        !c->dec_st.ensure(2 * cap * 4) || !c->gslot.ensure((cap + 31) / 32 * 64 * 2 * LDS_FQ6D_PACKED * 4) ||
        !c->fb_ct.ensure(4))
      return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_sk_decrypt: out of device memory");
    HIPCHK(c, hipMemsetAsync(c->fb_ct.p, 0, 4, s));
    c->fb_last = &c->fb_ct;
  }
  const uint32_t saved_me = c->own_me;
  c->own_me = UINT32_MAX;
  int rc = HBX_OK;
  for (uint32_t j0 = 0; j0 < count && rc == HBX_OK; j0 += chunk) {
    const uint32_t m = std::min(chunk, count - j0);
    uint8_t* st = c->kg_st.as<uint8_t>() + j0;  // the chunk's HBX_CT_* land in kg_st
    if (pair) {
      rc = launch_prepare_ct(c, s, c->u_comp_own.as<uint8_t>() + (size_t)j0 * 48, c->v_blob_own.as<uint8_t>(),
                             c->v_off_own.as<uint64_t>() + j0, c->w_comp_own.as<uint8_t>() + (size_t)j0 * 96, m, nullptr, 0,
                             0, UINT32_MAX);
      if (rc) break;
      timed t_(c, HBX_K_CT_CHECKS, s);
      const dim3 grid((m + 31) / 32);
      // Miller loops; the final exponentiation with compressed runs; then the pairs whose
      // decompression met g3 = 0 (SHARE_FALLBACK) once more with Granger-Scott squarings only
      // (verify_sig_impl's protocol; both retry launches return at once per pair when there are none)
      for (uint32_t retry = 0; retry < 2; retry++) {
        hipLaunchKernelGGL(k_verify_ct2, grid, dim3(64), 0, s, c->U.as<g1a>(), c->G2pts.as<g2a>(), c->Hj.as<g2j>(),
                           c->dec_st.as<int32_t>(), m, st, c->gslot.as<uint32_t>(), retry);
        if (retry == 0)
          hipLaunchKernelGGL(k_verify_sig_shares2_fe<true>, grid, dim3(64), 0, s, m, st, c->gslot.as<uint32_t>(),
                             c->force_fallback, c->fb_ct.as<uint32_t>(), nullptr);
        else
          hipLaunchKernelGGL(k_verify_sig_shares2_fe<false>, grid, dim3(64), 0, s, m, st, c->gslot.as<uint32_t>(), 0u,
                             c->fb_ct.as<uint32_t>(), nullptr);
      }
    } else {
      rc = prepare_impl(c, c->u_comp_own.as<uint8_t>() + (size_t)j0 * 48, c->v_blob_own.as<uint8_t>(),
                        c->v_off_own.as<uint64_t>() + j0, c->w_comp_own.as<uint8_t>() + (size_t)j0 * 96, m, maxv, st, s,
                        nullptr, 0);
    }
    if (rc) break;
    if (hipGetLastError() != hipSuccess) {
      rc = fail(c, HBX_E_DEVICE, "hbx_sk_decrypt: device error");
      break;
    }
    {
      timed t_(c, HBX_K_SK_DECRYPT, s);
      hipLaunchKernelGGL(k_sk_decrypt, dim3((m + 63) / 64), dim3(64), 0, s, c->U.as<g1a>(),
                         st, c->kg_sk.as<uint32_t>(), c->v_blob_own.as<uint8_t>(),
                         c->v_off_own.as<uint64_t>() + j0, m, c->kg_out.as<uint8_t>(), c->digest);
    }
    if (hipGetLastError() != hipSuccess) rc = fail(c, HBX_E_DEVICE, "hbx_sk_decrypt: device error");
  }
  c->own_me = saved_me;
  c->own_ready = false;
  c->p_ct = 0;
  c->invalidate_epoch();
  if (rc) return rc;
  HIPCHK(c, hipMemcpyAsync(status, c->kg_st.p, count, hipMemcpyDeviceToHost, s));
  if (total) HIPCHK(c, hipMemcpyAsync(out_blob, c->kg_out.p, total, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_bivar_poly_rows(hbx_ctx* c, const uint8_t* coeff32, uint32_t t, uint32_t n, uint8_t* rows32) {
  if (!c || !coeff32 || !rows32 || n == 0 || t > 4095) return fail(c, HBX_E_INVALID_ARG, "hbx_bivar_poly_rows: bad args");
  const size_t M = (size_t)(t + 1) * (t + 2) / 2, lanes = (size_t)n * (t + 1);
  if (lanes > (size_t)1 << 30) return fail(c, HBX_E_INVALID_ARG, "hbx_bivar_poly_rows: n (t + 1) too large");
  if (!scalars_canonical(coeff32, M)) return fail(c, HBX_E_INVALID_ARG, "hbx_bivar_poly_rows: scalar >= r");
  HBX_ENTER(c, c->stream);
  dbuf dc, dout;
  if (!dc.ensure(M * 32) || !dout.ensure(lanes * 32))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_bivar_poly_rows: out of device memory");
  HIPCHK(c, hipMemcpyAsync(dc.p, coeff32, M * 32, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_bivar_poly_rows, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, dc.as<uint8_t>(), t, n,
                     dout.as<uint8_t>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(rows32, dout.p, lanes * 32, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_fr_poly_eval(hbx_ctx* c, const uint8_t* coeff32, uint32_t p, uint32_t t, uint32_t n, uint8_t* out32) {
  if (!c || !coeff32 || !out32 || p == 0 || n == 0 || t > 4095)
    return fail(c, HBX_E_INVALID_ARG, "hbx_fr_poly_eval: bad args");
  const size_t nc = (size_t)p * (t + 1), lanes = (size_t)p * n;
  if (lanes > (size_t)1 << 30 || nc > (size_t)1 << 30) return fail(c, HBX_E_INVALID_ARG, "hbx_fr_poly_eval: too large");
  if (!scalars_canonical(coeff32, nc)) return fail(c, HBX_E_INVALID_ARG, "hbx_fr_poly_eval: scalar >= r");
  HBX_ENTER(c, c->stream);
  dbuf dc, dout;
  if (!dc.ensure(nc * 32) || !dout.ensure(lanes * 32))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_fr_poly_eval: out of device memory");
  HIPCHK(c, hipMemcpyAsync(dc.p, coeff32, nc * 32, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_fr_poly_eval, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, s, dc.as<uint8_t>(), p, t, n,
                     dout.as<uint8_t>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out32, dout.p, lanes * 32, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_keygen_generate(hbx_ctx* c, const uint8_t* commit48, uint32_t p, uint32_t t, const uint8_t* complete,
                        const uint32_t* val_cnt, const uint64_t* val_y, const uint8_t* vals32, uint8_t* pk_commit48,
                        uint8_t* sk32_out, uint8_t* status) {
  if (!c || !commit48 || !complete || !pk_commit48 || !status || p == 0 || t > 4095)
    return fail(c, HBX_E_INVALID_ARG, "hbx_keygen_generate: bad args");
  if (sk32_out && (!val_cnt || !val_y || !vals32)) return fail(c, HBX_E_INVALID_ARG, "hbx_keygen_generate: null values");
  const size_t M = (size_t)(t + 1) * (t + 2) / 2, nv = (size_t)p * (t + 1);
  if (sk32_out) {
    for (uint32_t q = 0; q < p; q++) {
      if (!complete[q]) continue;
      if (val_cnt[q] > t + 1) return fail(c, HBX_E_INVALID_ARG, "hbx_keygen_generate: part %u has %u > t + 1 values", q, val_cnt[q]);
      const uint64_t* y = val_y + (size_t)q * (t + 1);
      if (!scalars_canonical(vals32 + (size_t)q * (t + 1) * 32, val_cnt[q]))
        return fail(c, HBX_E_INVALID_ARG, "hbx_keygen_generate: value >= r in part %u", q);
      for (uint32_t a = 0; a < val_cnt[q]; a++)
        for (uint32_t b = a + 1; b < val_cnt[q]; b++)
          if (y[a] == y[b]) return fail(c, HBX_E_DUPLICATE_ENTRY, "hbx_keygen_generate: part %u repeats y = %llu", q, (unsigned long long)y[a]);
    }
  }
  HBX_ENTER(c, c->stream);
  dbuf dcomp, dcnt, dy, dv, dpkc, dpart, dsk;
  if (!c->bv_commit48.ensure(p * M * 48) || !c->bv_C.ensure(p * M * sizeof(g1a)) || !c->bv_cst.ensure(p * M * 4) ||
      !dcomp.ensure(p) || !dpkc.ensure((size_t)(t + 1) * 48) ||
      (sk32_out && (!dcnt.ensure((size_t)p * 4) || !dy.ensure(nv * 8) || !dv.ensure(nv * 32) ||
                    !dpart.ensure((size_t)p * sizeof(fr)) || !dsk.ensure(32))))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_keygen_generate: out of device memory");
  HIPCHK(c, hipMemcpyAsync(c->bv_commit48.p, commit48, p * M * 48, hipMemcpyHostToDevice, s));
  HIPCHK(c, hipMemcpyAsync(dcomp.p, complete, p, hipMemcpyHostToDevice, s));
  if (sk32_out) {
    HIPCHK(c, hipMemcpyAsync(dcnt.p, val_cnt, (size_t)p * 4, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dy.p, val_y, nv * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipMemcpyAsync(dv.p, vals32, nv * 32, hipMemcpyHostToDevice, s));
  }
  // decode = into_affine (curve + G1 membership), as a Part's commitment deserialises
  hipLaunchKernelGGL(k_decompress_shares, dim3((unsigned)((p * M + 255) / 256)), dim3(256), 0, s,
                     c->bv_commit48.as<uint8_t>(), p * M, c->bv_C.as<g1a>(), c->bv_cst.as<int32_t>(), 1u, UINT32_MAX, nullptr);
  HIPCHK(c, hipGetLastError());
  std::vector<int32_t> cst(p * M);
  HIPCHK(c, hipMemcpyAsync(cst.data(), c->bv_cst.p, p * M * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  bool bad = false;
  for (uint32_t q = 0; q < p; q++) {
    status[q] = complete[q] ? HBX_SHARE_VALID : HBX_SHARE_ABSENT;
    for (size_t m = 0; complete[q] && m < M; m++) {
      const int32_t st = cst[q * M + m];
      if (st != HBX_PT_OK && st != HBX_PT_INFINITY) status[q] = HBX_SHARE_UNDECODABLE;
    }
    bad = bad || status[q] == HBX_SHARE_UNDECODABLE;
  }
  if (bad) return fail(c, HBX_E_INVALID_ARG, "hbx_keygen_generate: a complete part's commitment does not decode");
  const uint32_t lanes = t + 1 + (sk32_out ? p : 0);
  hipLaunchKernelGGL(k_keygen_generate, dim3((lanes + 63) / 64), dim3(64), 0, s, c->bv_C.as<g1a>(), p, t,
                     dcomp.as<uint8_t>(), dcnt.as<uint32_t>(), dy.as<uint64_t>(), dv.as<uint8_t>(), dpkc.as<uint8_t>(),
                     sk32_out ? dpart.as<fr>() : nullptr);
  HIPCHK(c, hipGetLastError());
  if (sk32_out) {
    hipLaunchKernelGGL(k_keygen_sum, dim3(1), dim3(64), 0, s, dpart.as<fr>(), p, dsk.as<uint8_t>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(sk32_out, dsk.p, 32, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(c, hipMemcpyAsync(pk_commit48, dpkc.p, (size_t)(t + 1) * 48, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_pk_shares_from_commit(hbx_ctx* c, const uint8_t* pk_commit48, uint32_t t, uint32_t n, uint8_t* pk48) {
  if (!c || !pk_commit48 || !pk48 || n == 0 || t > 4095)
    return fail(c, HBX_E_INVALID_ARG, "hbx_pk_shares_from_commit: bad args");
  HBX_ENTER(c, c->stream);
  dbuf dcc, dP, dst, dout;
  if (!dcc.ensure((size_t)(t + 1) * 48) || !dP.ensure((size_t)(t + 1) * sizeof(g1a)) || !dst.ensure((size_t)(t + 1) * 4) ||
      !dout.ensure((size_t)n * 48))
    return fail(c, HBX_E_OUT_OF_MEMORY, "hbx_pk_shares_from_commit: out of device memory");
  HIPCHK(c, hipMemcpyAsync(dcc.p, pk_commit48, (size_t)(t + 1) * 48, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(k_decompress_shares, dim3((t + 1 + 255) / 256), dim3(256), 0, s, dcc.as<uint8_t>(), (size_t)(t + 1),
                     dP.as<g1a>(), dst.as<int32_t>(), 1u, UINT32_MAX, nullptr);
  HIPCHK(c, hipGetLastError());
  std::vector<int32_t> st(t + 1);
  HIPCHK(c, hipMemcpyAsync(st.data(), dst.p, (size_t)(t + 1) * 4, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  for (uint32_t j = 0; j <= t; j++)
    if (st[j] != HBX_PT_OK && st[j] != HBX_PT_INFINITY)
      return fail(c, HBX_E_INVALID_ARG, "hbx_pk_shares_from_commit: point %u does not decode (status %d)", j, st[j]);
  hipLaunchKernelGGL(k_pk_shares_from_commit, dim3((n + 63) / 64), dim3(64), 0, s, dP.as<g1a>(), t, n, dout.as<uint8_t>());
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(pk48, dout.p, (size_t)n * 48, hipMemcpyDeviceToHost, s));
  HIPCHK(c, hipStreamSynchronize(s));
  return HBX_OK;
}

}  // extern "C"

int hbx_set_timing(hbx_ctx* c, int on) {
  if (!c) return HBX_E_INVALID_ARG;
  HBX_DEVICE(c);
  c->timing.reset();
  c->timing.on = on != 0;
  return HBX_OK;
}

int hbx_kernel_time(hbx_ctx* c, int kernel, double* total_ms, uint32_t* launches) {
  if (!c || kernel < 0 || kernel >= HBX_K_COUNT || !total_ms) return fail(c, HBX_E_INVALID_ARG, "hbx_kernel_time: bad argument");
  HBX_DEVICE(c);
  double tot = 0;
  for (auto& pr : c->timing.tev[kernel]) {
    HIPCHK(c, hipEventSynchronize(pr.second));
    float ms = 0;
    HIPCHK(c, hipEventElapsedTime(&ms, pr.first, pr.second));
    tot += ms;
  }
  *total_ms = tot;
  if (launches) *launches = (uint32_t)c->timing.tev[kernel].size();
  return HBX_OK;
}

uint64_t hbx_debug_live_buffers(void) { return live_buffers.load(); }
#endif  // host translation unit
