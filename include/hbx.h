/* hbx.h -- C ABI of the MI355X batch engine for hbbft's threshold-crypto hot path.
 *
 * Drop-in boundary.  The reference calls threshold_crypto / pairing 0.14 one
 * share at a time on the caller's thread; this ABI takes a whole epoch's worth in one call.  Each
 * entry point names the reference interface it replaces (file:line in jonnydubowsky/hbbft @ v0).
 *
 * Conventions
 *  - Plain pointers + sizes, caller-owned buffers, no torch types.
 *  - Functions without the `_d` suffix take HOST pointers, stage through device buffers owned
 *    by the context and block until results are back on the host.
 *  - Functions with the `_d` suffix take DEVICE pointers (hipMalloc'd on the context's device)
 *    and a hipStream_t passed as `void*` (NULL = the HIP null stream, i.e. what a framework's
 *    default stream hands over); they enqueue work on that stream, in stream order with the
 *    caller's own work on it, and return without synchronising.
 *  - Return value: HBX_OK (0) or a negative HBX_E_* code.  A failed verification is NOT an error:
 *    it is a 0 in the corresponding validity output, exactly as the reference returns `false`.
 *  - Validity outputs are byte-per-item (1 = valid) in the `_d` API and little-endian bitmaps
 *    (bit k of byte k/8) in the host API.
 *  - Point encodings are the zcash/pairing 0.14 formats: G1 compressed 48 B, G2 compressed
 *    96 B, G2 uncompressed 192 B (x.c1 || x.c0 || y.c1 || y.c0).
 *  - Share matrices are proposer-major: share[j][i] = the decryption share node i sent for
 *    proposer j's ciphertext, at offset (j * n + i) * 48.
 *  - One context per device.  Calls on one context must be serialised by the caller.
 */
#ifndef HBX_H
#define HBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBX_OK 0
#define HBX_E_INVALID_ARG (-1)
#define HBX_E_DEVICE (-2)
#define HBX_E_NOT_ENOUGH_SHARES (-3) /* threshold_crypto Error::NotEnoughShares */
#define HBX_E_DUPLICATE_ENTRY (-4)   /* threshold_crypto Error::DuplicateEntry */
#define HBX_E_NO_KEYS (-5)           /* hbx_set_pk_shares not called / wrong n */
#define HBX_E_NO_CIPHERTEXTS (-6)    /* hbx_prepare_ciphertexts not called / wrong p */
#define HBX_E_INVALID_CIPHERTEXT (-7)/* Ciphertext::verify failed or undecodable (honey_badger.rs:366-373) */
#define HBX_E_OUT_OF_MEMORY (-8)
#define HBX_E_TOO_FEW_SHARDS (-9)    /* reed_solomon_erasure Error::TooFewShardsPresent */
#define HBX_E_ROOT_MISMATCH (-10)    /* decode_from_shards: rebuilt Merkle root != hash (broadcast.rs:686) */
#define HBX_E_NO_PAYLOAD (-11)       /* glue_shards: fewer than 4 bytes (broadcast.rs:702) */
#define HBX_E_NO_BROADCAST (-12)     /* hbx_prepare_broadcast not called, or its store voided */
#define HBX_E_SHARD_SIZE (-13)       /* reed_solomon_erasure Error::IncorrectShardSize */

/* per-point decode status (hbx_set_pk_shares / hbx_prepare_ciphertexts) */
#define HBX_PT_OK 0
#define HBX_PT_BAD_FLAGS 1
#define HBX_PT_NOT_IN_FIELD 2
#define HBX_PT_NOT_ON_CURVE 3
#define HBX_PT_INFINITY 4
#define HBX_PT_NOT_IN_SUBGROUP 5 /* on the curve but not in G1 / G2 (pairing's into_affine rejects it) */

/* Per-share status (one byte per share: the d_valid arrays of the _d API, hbx_get_share_status,
 * hbx_get_sig_share_status).  1 = valid and 0 = verified false, so "byte == 1" is "valid";
 * the other codes tell the caller which reference fault, if any, the share maps to:
 *   HBX_SHARE_INVALID        verify returned false: FaultKind::UnverifiedDecryptionShareSender
 *                            (honey_badger.rs:199, :437) / UnverifiedSignatureShareSender
 *                            (common_coin.rs:153); the share is dropped.
 *   HBX_SHARE_VALID          verified true.
 *   HBX_SHARE_ABSENT         present bit 0: no message, nothing to report.
 *   HBX_SHARE_UNDECODABLE    the 48/96 bytes are not a subgroup point: the reference never sees
 *                            such a share (serde/bincode rejects the message before
 *                            HoneyBadger/CommonCoin), so no fault kind of the algorithm applies.
 *   HBX_SHARE_SKIPPED_CT     not verified because the proposer's ciphertext failed to decode or
 *                            Ciphertext::verify: the reference skips that proposer
 *                            (honey_badger.rs:359-376) and never verifies its shares.
 *   HBX_SHARE_UNKNOWN_SENDER sender index >= n of hbx_set_pk_shares: the reference rejects the
 *                            message with Error UnknownSender (honey_badger.rs:64-66,
 *                            common_coin.rs:158).  (own-share mode: `me` is always checked.) */
#define HBX_SHARE_INVALID 0
#define HBX_SHARE_VALID 1
#define HBX_SHARE_ABSENT 2
#define HBX_SHARE_UNDECODABLE 3
#define HBX_SHARE_SKIPPED_CT 4
#define HBX_SHARE_UNKNOWN_SENDER 5

/* Per-ciphertext status (d_ct_valid of the _d API, hbx_get_ct_status):
 *   HBX_CT_INVALID      Ciphertext::verify returned false: FaultKind::ShareDecryptionFailed
 *                       (honey_badger.rs:371-375).
 *   HBX_CT_VALID        verified.
 *   HBX_CT_UNDECODABLE  U or W does not decode to a subgroup point: bincode::deserialize of the
 *                       ciphertext fails, FaultKind::InvalidCiphertext (honey_badger.rs:359-368). */
#define HBX_CT_INVALID 0
#define HBX_CT_VALID 1
#define HBX_CT_UNDECODABLE 3

/* Digest variants (hbx_set_digest, hbx_set_merkle_digest). */
#define HBX_DIGEST_SHA256 0   /* default: ring SHA-256 (reference Cargo.toml:32) */
#define HBX_DIGEST_SHA3_256 1 /* tiny-keccak SHA3-256 */
#define HBX_MERKLE_SHA256 0   /* default: merkle (afck fork) + ring SHA-256, leaf H(0x00||v),
                                 node H(0x01||l||r), odd node promoted (broadcast.rs:161, :381) */
#define HBX_MERKLE_SHA3 1     /* later hbbft's own tree (src/broadcast/merkle.rs, tiny-keccak):
                                 leaf SHA3(v), node SHA3(l||r), odd node promoted */

typedef struct hbx_ctx hbx_ctx;

/* Create / destroy a context bound to HIP device `device`. */
int hbx_ctx_create(int device, hbx_ctx** out);
int hbx_ctx_destroy(hbx_ctx* ctx);
/* Human-readable description of the last error on this context (never NULL). */
const char* hbx_last_error(const hbx_ctx* ctx);
/* Library version string, e.g. "hbx 0.1.0 gfx950". */
const char* hbx_version(void);
/* SHA-256 (hex) of the sources this library was built from (hbbft_amd/buildinfo.py source_hash,
 * set by tools/build.py); "unknown" for a build outside it.  Provenance only: no reference
 * counterpart. */
const char* hbx_build_id(void);

/* Kernel timing (instrumentation; no reference counterpart).  With timing on, the library
 * brackets each launch of the kernels below with HIP events recorded on the stream the kernel
 * runs on; hbx_kernel_time synchronizes those events and reports the summed duration and the
 * number of launches since the last hbx_set_timing call. */
#define HBX_K_PREPARE_CT 0      /* hash_g1_g2 + decode of U/W per proposer */
#define HBX_K_PREPARE_LINES 1   /* prepared Miller lines of H_j, W_j (and coin H) */
#define HBX_K_CT_CHECKS 2       /* Ciphertext::verify pairing checks (wide executor; hbx_sk_decrypt in pair mode: k_verify_ct2 + final exponentiation) */
#define HBX_K_VERIFY_SHARES 3   /* decryption-share pairing checks */
#define HBX_K_COMBINE 4         /* Lagrange combine + key derivation per proposer */
#define HBX_K_VERIFY_SIG 5      /* coin signature-share checks */
#define HBX_K_COMBINE_SIGS 6    /* coin G2 Lagrange combine + master-key check */
#define HBX_K_RS_CODE 7         /* Reed-Solomon encode / reconstruct passes */
#define HBX_K_MERKLE_LEAVES 8   /* SHA-256 leaf hashes */
#define HBX_K_HASH_NONCES 9     /* coin nonce hash_g2 */
#define HBX_K_DECODE_SIGS 10    /* coin signature-share decode (G2 decompression; the checks test G2 membership) */
#define HBX_K_SK_DECRYPT 11   /* SecretKey::decrypt keystream after the chunked Ciphertext::verify (hbx_sk_decrypt) */
#define HBX_K_BATCH_MSM 12    /* batched verification: coefficients, key terms and the per-column sums A_j, B_j */
#define HBX_K_BATCH_CHECK 13  /* batched verification: the p column equations and the column classes */
#define HBX_K_COUNT 14
int hbx_set_timing(hbx_ctx* ctx, int on);
int hbx_kernel_time(hbx_ctx* ctx, int kernel, double* total_ms, uint32_t* launches);

/* ---------------------------------------------------------------------------------------------
 * DIGEST of threshold_crypto's hash_g2 / hash_g1_g2 / hash_bytes.  The
 * reference's threshold_crypto dependency is an unpinned git revision (Cargo.toml:35): revisions
 * hash with SHA-256 or with tiny-keccak's SHA3-256.  Per context, default HBX_DIGEST_SHA256;
 * switching voids the prepared ciphertexts / nonces.  Affects every H_j, W, plaintext keystream,
 * nonce hash and signature of this context.
 * hbx_set_merkle_digest -- the Merkle tree of the broadcast calls (HBX_MERKLE_*).
 * ------------------------------------------------------------------------------------------- */
int hbx_set_digest(hbx_ctx* ctx, int variant);
/* Lanes per decryption-share check (no reference counterpart; results identical): 1 = one lane
 * per check (the throughput path when a launch fills the chip: a Miller-loop kernel and the final
 * exponentiation as four step kernels over per-lane slots), 7 = one lane per check in a single
 * kernel (the final exponentiation through call frames; kept for comparison), 2 = a lane pair per
 * check (the
 * Fq12 state split in halves, no scratch), 3 = three cooperating lanes per check, 6 = six lanes per
 * check (the two Miller loops on two lane triplets side by side; lowest latency per check), 0 =
 * choose by launch size (default: 1 when one-lane checks fill >= 1024 waves, else 6 when six-lane
 * checks fit in 1024 waves, else 3). */
int hbx_set_verify_lanes(hbx_ctx* ctx, int lanes);
/* Lanes per check the last decryption-share launch used (1, 2, 3, 6 or 7; 0 before any launch). */
int hbx_get_verify_lanes_used(const hbx_ctx* ctx);
/* Tests only: in one-lane decryption-share checks, two-lane coin checks and pair-lane ciphertext
 * checks (hbx_set_ct_check), treat the check of every `every`-th sender, or every `every`-th
 * ciphertext of a chunk (0 = none, the default), as if its compressed squarings had met a zero
 * denominator, so the fallback path decides it (the single-kernel one-lane check; for the coin, the
 * pair's Miller loop again and a final exponentiation without compressed runs).  Results are
 * unchanged.  (Real inputs reach that path only through an element with a zero Fq2 coefficient at
 * the end of a compressed run, ~2^-760 for values nobody chose; the one degenerate start a proposer
 * can choose -- a ciphertext with r = 3(x^2 - 1), for which every honest share's check is 1 after
 * the easy part -- is decided by the first step without a fallback.) */
int hbx_debug_force_fallback(hbx_ctx* ctx, uint32_t every);
/* Tests only: in one-lane decryption-share checks, treat every `every`-th proposer (0 = none, the
 * default) as if one of the lines of its H' or W had a zero constant term, which the one-lane Miller
 * kernel's line form (divided by that term) cannot hold: every checkable share of such a proposer,
 * and in own-share mode its ciphertext check, is decided by the fallback path (the single-kernel
 * one-lane check over the lines divided by their y coefficient) and counted by
 * hbx_get_fallback_lanes.  Results are unchanged.  (A real line has a zero constant term with
 * probability ~2^-760 per line for a hash output; a proposer who chooses W to hit one only moves
 * its own column to the slower path.) */
int hbx_debug_force_degenerate(hbx_ctx* ctx, uint32_t every);
/* Checks of the last share-check launch (decryption-share, coin, the pair-lane ciphertext checks
 * of hbx_sk_decrypt or the pair-lane signature checks of hbx_verify_sigs_keyed, the latter two
 * summed over that call's chunks -- whichever came last) that the fallback path
 * decided: 0 unless hbx_debug_force_fallback or hbx_debug_force_degenerate is on, and 0 when that launch used a lane
 * count without a fallback path (decryption shares at lanes 2/3/6/7, coin at one lane).  The four
 * kinds count separately; "last" is host call order, so the value is meaningful when the caller
 * reads it after the launch it asks about (waits for the context's streams).  Diagnostics: no
 * reference counterpart. */
int64_t hbx_get_fallback_lanes(hbx_ctx* ctx);
/* Lanes per Lagrange term of hbx_combine_decrypt_d (no reference counterpart; results identical):
 * 1 = one lane per GLV term, one block per proposer (k_combine), 4 = a quad of lanes per term over
 * one-wave blocks (k_combine_q, t <= 128), 0 = by launch size (default: 4 when the quad blocks fit
 * in 1024 waves, else 1). */
int hbx_set_combine_lanes(hbx_ctx* ctx, int lanes);
/* The combine's precomputed window tables (no reference counterpart; results identical).
 * hbx_decrypt_epoch_d, when its combine runs one lane per term, has the line-preparation launch
 * also compute, for every proposer and every sender i < cap = min(n, t + margin) whose share
 * decoded (and for this node's own share), D = [2^64] S and the 4-bit tables of S and D; the
 * combine's lanes then run one interleaved loop from those tables instead of a 128-bit window
 * multiplication from the point.  A term without tables -- a sender at or beyond cap, the
 * three-call API, the quad combine -- multiplies from the point as before.  The table buffer is
 * allocated by the fused call only: p x (cap + 1) x 5,040 bytes.
 * hbx_debug_set_combine_margin (tests only): margin >= 0, HBX_COMBINE_MARGIN_AUTO (default: cap
 * = t + 32 rounded up to a multiple of 64) or HBX_COMBINE_TABLES_OFF (no tables at all).
 * hbx_get_combine_slow_terms: GLV half-terms of the last combine launch that multiplied from the
 * point (every term of a quad combine; 0 for an honest epoch at the default margin).  Read it
 * after the launch it asks about, as hbx_get_fallback_lanes. */
#define HBX_COMBINE_MARGIN_AUTO (-1)
#define HBX_COMBINE_TABLES_OFF (-2)
int hbx_debug_set_combine_margin(hbx_ctx* ctx, int32_t margin);
int64_t hbx_get_combine_slow_terms(hbx_ctx* ctx);
/* Device and pinned allocations the library currently holds in this process, over all contexts
 * (tests: a destroyed context, and a call that failed, leave none behind). */
uint64_t hbx_debug_live_buffers(void);
/* Batched decryption-share verification by random linear combination (no reference counterpart;
 * statuses identical except with probability <= 2^-128 per column, DESIGN.md "Batched share
 * verification").  seed32 != NULL: hbx_verify_dec_shares[_d] and hbx_decrypt_epoch_d decide each
 * proposer's column by one equation
 *   e( sum_i r_i S_ji , H_j ) e( -sum_i r_i pk_i , W_j ) == 1
 * over the included senders (present, known, share decoded) and run the per-share checks only for
 * columns whose equation fails, which name the culprits as before.  seed32 == NULL: per-share
 * checks (default).  Setting a seed resets the call index to 0.  Statuses written are those of the
 * per-share path (HBX_SHARE_*, HBX_CT_*); a deferred Ciphertext::verify is folded into the equation.
 * r_i = the little-endian integer of the first 16 bytes of SHA-256(seed32 || LE64(call_index) ||
 * LE32(i)), i the sender index (0xFFFFFFFF: the ciphertext term), call_index the number of batched
 * verifications since the seed was set; SHA-256 whatever hbx_set_digest says.  The seed MUST be
 * unpredictable to every sender: with a known seed a sender can forge a column. */
int hbx_set_batch_verify(hbx_ctx* ctx, const uint8_t* seed32);
/* Columns of the last share verification: decided by the equation / sent to the per-share path
 * (equation failed, or U_j, W_j or H_j is the identity) / not examined (ciphertext undecodable or
 * already known invalid).  All 0 after a per-share verification.  Blocking. */
int hbx_get_batch_stats(hbx_ctx* ctx, uint32_t* cols_batched, uint32_t* cols_fallback, uint32_t* cols_skipped);
/* Test hook: A_j = sum_{i included} r_i S_ji of the last batched verification, compressed, p x 48
 * (the identity encoding for an empty column and for one the equation was not evaluated for:
 * skipped, or a ciphertext point is the identity).  count must equal p.  Blocking. */
int hbx_get_batch_sums(hbx_ctx* ctx, uint8_t* a48, size_t count);
int hbx_set_merkle_digest(hbx_ctx* ctx, int variant);

/* ---------------------------------------------------------------------------------------------
 * Key material (once per era).
 * Replaces: NetworkInfo::new's public_key_share derivation (src/messaging.rs:251-254) and the
 * per-call lookup NetworkInfo::public_key_share (src/messaging.rs:312) used by
 * HoneyBadger::verify_decryption_share (src/honey_badger/honey_badger.rs:228-232).
 * pk_comp: n x 48 B compressed pk_i (node index order = BTreeMap order, messaging.rs:246-250).
 * status (optional, n entries): HBX_PT_* per key.
 * A new key set clears this node's own share (hbx_set_own_share must be called again for the
 * new era) and every epoch result computed under the old keys.
 * ------------------------------------------------------------------------------------------- */
int hbx_set_pk_shares(hbx_ctx* ctx, const uint8_t* pk_comp, uint32_t n, int32_t* status);

/* ---------------------------------------------------------------------------------------------
 * This node's own secret key share (once per era; optional).
 * Replaces: the node's own share path -- SecretKeyShare::decrypt_share_no_verify in
 * send_decryption_share (src/honey_badger/honey_badger.rs:394-418), whose result the node feeds
 * back to itself as sender `me`.  With it set, hbx_prepare_ciphertexts* computes S_j,me = sk_me U_j
 * for every ciphertext, hbx_verify_dec_shares* uses it for sender `me` (that row of the share
 * input is ignored), and the check of that share doubles as Ciphertext::verify (:371): U_j, W_j are
 * decoded with subgroup checks and H_j is in G2, so e(sk U, H) e(-sk g1, W) = 1 exactly when
 * e(U, H) = e(g1, W) (sk != 0 mod r).  This removes the separate latency-bound ciphertext checks.
 * sk32: canonical big-endian scalar in [1, r) matching pk[me] of hbx_set_pk_shares
 * (HBX_E_INVALID_ARG otherwise); NULL clears the mode.
 * ------------------------------------------------------------------------------------------- */
int hbx_set_own_share(hbx_ctx* ctx, uint32_t me, const uint8_t* sk32);

/* ---------------------------------------------------------------------------------------------
 * Ciphertexts of one epoch (one per accepted proposer).
 * Replaces: threshold_crypto Ciphertext::verify (src/honey_badger/honey_badger.rs:371) and
 * hoists hash_g1_g2(U_j, V_j) -- recomputed by the reference inside every
 * verify_decryption_share call -- to once per ciphertext.
 * u_comp: p x 48 B; w_comp: p x 96 B; v_blob + v_off[p + 1]: the V byte strings.
 * ct_valid_bits: ceil(p/8) B out; bit j = Ciphertext::verify(ct_j) (0 also for undecodable
 * points, i.e. the reference's InvalidCiphertext / ShareDecryptionFailed faults).
 * ------------------------------------------------------------------------------------------- */
int hbx_prepare_ciphertexts(hbx_ctx* ctx, const uint8_t* u_comp, const uint8_t* v_blob,
                            const uint64_t* v_off, const uint8_t* w_comp, uint32_t p,
                            uint8_t* ct_valid_bits);

/* ---------------------------------------------------------------------------------------------
 * Decryption-share verification, whole epoch.
 * Replaces: PublicKeyShare::verify_decryption_share (src/honey_badger/honey_badger.rs:229) as
 * called from verify_pending_decryption_shares (:422-444) and handle_decryption_share_message
 * (:198).  valid[j][i] = e(S_ji, H_j) == e(pk_i, W_j).  Absent shares (present bit 0), unknown
 * senders (i >= n of hbx_set_pk_shares), undecodable encodings and shares of a ciphertext that
 * failed hbx_prepare_ciphertexts give 0; hbx_get_share_status tells these apart (HBX_SHARE_*),
 * so a caller raises UnverifiedDecryptionShareSender exactly for HBX_SHARE_INVALID.
 * shares: p x n x 48 B; present_bits: ceil(p*n/8) B (NULL = all present);
 * valid_bits: ceil(p*n/8) B out (bit j*n + i).
 * ------------------------------------------------------------------------------------------- */
int hbx_verify_dec_shares(hbx_ctx* ctx, const uint8_t* shares, const uint8_t* present_bits,
                          uint32_t n, uint32_t p, uint8_t* valid_bits);

/* Status bytes of the last share verification (p x n, HBX_SHARE_*) and of the last prepared
 * ciphertexts (p, HBX_CT_*), copied to the host (blocking).  count must equal p*n (resp. p). */
int hbx_get_share_status(hbx_ctx* ctx, uint8_t* status, size_t count);
int hbx_get_ct_status(hbx_ctx* ctx, uint8_t* status, size_t count);
/* The hoisted H_j = hash_g1_g2(U_j, V_j) of the last prepared ciphertexts (threshold_crypto,
 * recomputed by the reference inside every verify_decryption_share, honey_badger.rs:229),
 * compressed, p x 96 B; the identity for a ciphertext that does not decode. */
int hbx_get_ct_hashes(hbx_ctx* ctx, uint8_t* h96, size_t count);

/* ---------------------------------------------------------------------------------------------
 * Threshold decryption of every proposer's contribution.
 * Replaces: PublicKeySet::decrypt (src/honey_badger/honey_badger.rs:340) inside
 * try_decrypt_proposer_contribution (:315-349): for each proposer j takes the FIRST t valid
 * shares in node-index order, Lagrange-interpolates at 0 (x = index + 1) and XORs V_j with
 * hash_bytes(g, |V_j|).  Uses the shares and validity of the last hbx_verify_dec_shares call.
 * out_blob: sum |V_j| bytes at the v_off offsets of hbx_prepare_ciphertexts.
 * status: p entries, HBX_OK / HBX_E_NOT_ENOUGH_SHARES / HBX_E_INVALID_CIPHERTEXT.
 * ------------------------------------------------------------------------------------------- */
int hbx_combine_decrypt(hbx_ctx* ctx, uint32_t t, uint8_t* out_blob, int32_t* status);

/* ---------------------------------------------------------------------------------------------
 * Device-pointer / stream variants (inputs resident in HBM; nothing is copied to the host).
 *   d_present is a byte-per-share array (nonzero = present); d_valid receives one HBX_SHARE_*
 *   status byte per share and d_ct_valid one HBX_CT_* byte per ciphertext (1 = valid in both).
 *   A prepare invalidates the previous verification: combine needs a verify of the same p after
 *   the latest prepare (HBX_E_NO_CIPHERTEXTS otherwise).
 * hbx_prepare_ciphertexts_d with d_ct_valid == NULL DEFERS Ciphertext::verify: the checks then run
 * fused into the next hbx_verify_dec_shares_d launch (one more pairing check per proposer next
 * to its n share checks), and hbx_get_ct_valid_d copies the result out afterwards.
 * ------------------------------------------------------------------------------------------- */
int hbx_prepare_ciphertexts_d(hbx_ctx* ctx, const uint8_t* d_u_comp, const uint8_t* d_v_blob,
                              const uint64_t* d_v_off, const uint8_t* d_w_comp, uint32_t p,
                              uint64_t max_v_len, uint8_t* d_ct_valid, void* stream);
int hbx_verify_dec_shares_d(hbx_ctx* ctx, const uint8_t* d_shares, const uint8_t* d_present,
                            uint32_t n, uint32_t p, uint8_t* d_valid, void* stream);
int hbx_combine_decrypt_d(hbx_ctx* ctx, uint32_t t, uint8_t* d_out_blob, int32_t* d_status,
                          void* stream);
int hbx_get_ct_valid_d(hbx_ctx* ctx, uint8_t* d_ct_valid, void* stream);

/* One node-epoch of threshold decryption in ONE call: what honey_badger.rs does per epoch through
 * Ciphertext::verify (:371), verify_decryption_share (:229, :422-444) and PublicKeySet::decrypt
 * (:340), batched ("route whole epochs' worth of shares through one batched call").
 * Results and stream semantics are those of hbx_prepare_ciphertexts_d (Ciphertext::verify
 * deferred) + hbx_verify_dec_shares_d + hbx_get_ct_valid_d + hbx_combine_decrypt_d.
 * All outputs are device arrays, complete when `stream` reaches the end of the call's work. */
int hbx_decrypt_epoch_d(hbx_ctx* ctx, const uint8_t* d_u_comp, const uint8_t* d_v_blob, const uint64_t* d_v_off,
                        const uint8_t* d_w_comp, uint32_t p, uint64_t max_v_len, const uint8_t* d_shares,
                        const uint8_t* d_present, uint32_t n, uint32_t t, uint8_t* d_valid, uint8_t* d_ct_valid,
                        uint8_t* d_out_blob, int32_t* d_status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Incremental share verification: the shares that arrive after the epoch's ciphertexts are
 * prepared, verified on arrival and merged into the epoch's p x n matrix.
 * Replaces: HoneyBadger::handle_decryption_share_message (src/honey_badger/honey_badger.rs:186-217,
 * the check at :198) for a node that is running the epoch, where hbx_verify_dec_shares[_d] decides
 * a finished one.  Item k is the 48 bytes shares48[k] for position (proposer[k] = column j < p,
 * sender[k] = node index i); the launch covers the tiles of the check kernels that the items touch,
 * not n * p, and the lanes per check follow the touched-tile count (hbx_set_verify_lanes overrides;
 * hbx_get_verify_lanes_used, hbx_debug_force_fallback, hbx_debug_force_degenerate and
 * hbx_get_fallback_lanes mean for an add what they mean for a matrix verification).
 *
 * The matrix: after hbx_verify_dec_shares[_d] or hbx_decrypt_epoch_d the add continues from that
 * call's matrix (n must be its n).  On a context whose latest prepare has not been followed by a
 * share verification of the same p, the add first behaves exactly as hbx_verify_dec_shares_d with
 * every present byte 0 and this n (own-share mode enters and checks this node's shares, a deferred
 * Ciphertext::verify is decided, the batched mode runs if a seed is set); count == 0 is allowed
 * (pointers may then be NULL) and only does that.  A prepare voids the matrix.
 *
 * status[k] is the HBX_SHARE_* byte hbx_verify_dec_shares_d writes for the same bytes at (j, i) of
 * the same epoch; sender[k] >= n gives HBX_SHARE_UNKNOWN_SENDER and touches no position.  The items
 * always run the per-share checks: a batch seed is neither used nor advanced by them.
 * Merge: an entry that is HBX_SHARE_VALID keeps its point and status when the item is not VALID
 * (the reference returns the fault before `insert`, :198-201); in every other case the entry takes
 * the item's status, and its point where it decoded (`insert` replaces, :205-210).  No other entry
 * changes, so delivering every share of an epoch once, in any partition into calls, leaves the
 * matrix, hbx_get_share_status, hbx_get_ct_status and the combine as one matrix call does.  The
 * precomputed combine tables of a fused call are void after an add.
 *
 * HBX_E_INVALID_ARG before anything is launched: proposer[k] >= p; the same (proposer, sender)
 * twice in one call (the second message of a pair goes into a later call); n different from the
 * matrix's; in own-share mode, sender[k] == me.  HBX_E_NO_KEYS / HBX_E_NO_CIPHERTEXTS as for the
 * matrix call.  The host index arrays are consumed before the call returns.  The _d form is
 * stream-ordered and does not synchronise (d_status may be NULL); the host form blocks.
 * ------------------------------------------------------------------------------------------- */
int hbx_add_dec_shares_d(hbx_ctx* ctx, const uint8_t* d_shares48 /* [count][48] */,
                         const uint32_t* proposer /* HOST [count]: column j < p */,
                         const uint32_t* sender /* HOST [count]: node index */, uint32_t count, uint32_t n,
                         uint8_t* d_status /* [count], may be NULL */, void* stream);
int hbx_add_dec_shares(hbx_ctx* ctx, const uint8_t* shares48, const uint32_t* proposer, const uint32_t* sender,
                       uint32_t count, uint32_t n, uint8_t* status);
/* Threshold decryption of the listed proposers only: try_decrypt_proposer_contribution
 * (src/honey_badger/honey_badger.rs:315-349) for the proposers that crossed the threshold.  Reads
 * what hbx_combine_decrypt_d reads (the first t VALID entries in index order at call time) and
 * writes only status[cols[k]] and the v_off ranges of the listed proposers that decrypted: no other
 * byte of either output changes.  cols (HOST, consumed before the call returns): cols[k] >= p or a
 * repeated column is HBX_E_INVALID_ARG; ncols == 0 is a no-op that returns HBX_OK.  The lanes per
 * Lagrange term are chosen as by hbx_set_combine_lanes with ncols in the place of p. */
int hbx_combine_decrypt_cols_d(hbx_ctx* ctx, uint32_t t, const uint32_t* cols /* HOST [ncols] */, uint32_t ncols,
                               uint8_t* d_out_blob, int32_t* d_status /* [p] */, void* stream);
int hbx_combine_decrypt_cols(hbx_ctx* ctx, uint32_t t, const uint32_t* cols, uint32_t ncols, uint8_t* out_blob,
                             int32_t* status);
/* Check blocks (64-thread tiles) of the last share-check launch: grid.x * grid.y for a matrix
 * verification, the tile-list length for an add; 0 before any.  Diagnostics: no reference
 * counterpart. */
uint32_t hbx_get_verify_tiles_used(const hbx_ctx* ctx);

/* ---------------------------------------------------------------------------------------------
 * Producer side.  Scalars are canonical Fr values as
 * 32-byte big-endian strings (< r; anything else is HBX_E_INVALID_ARG).
 *
 * hbx_public_keys -- threshold_crypto SecretKey::public_key, pk_i = g1 * sk_i, as used by the
 *   test key generation NetworkInfo::generate_map (src/messaging.rs:359-401).
 * hbx_encrypt -- PublicKey::encrypt (src/honey_badger/honey_badger.rs:116) with the randomness
 *   r_j passed in (threshold_crypto draws it from thread_rng):  U = g1 r, V = M xor
 *   hash_bytes(pk r, |M|), W = hash_g1_g2(U, V) r.  v_blob uses the msg_off offsets.
 * hbx_decrypt_shares -- SecretKeyShare::decrypt_share_no_verify
 *   (src/honey_badger/honey_badger.rs:403): shares[j][i] = sk_i * U_j, proposer-major p x n x 48.
 * ------------------------------------------------------------------------------------------- */
int hbx_public_keys(hbx_ctx* ctx, const uint8_t* sk32, uint32_t n, uint8_t* pk48);
int hbx_encrypt(hbx_ctx* ctx, const uint8_t* pk48, const uint8_t* msg_blob, const uint64_t* msg_off,
                uint32_t p, const uint8_t* r32, uint8_t* u48, uint8_t* v_blob, uint8_t* w96);
int hbx_decrypt_shares(hbx_ctx* ctx, const uint8_t* sk32, uint32_t n, const uint8_t* u48, uint32_t p,
                       uint8_t* shares48);

/* ---------------------------------------------------------------------------------------------
 * Common Coin, batched over `count` coin instances (concurrent
 * Agreement instances; the nonce of each is Nonce::new, src/agreement/mod.rs:155-165).
 * hbx_prepare_nonces -- hash_g2(nonce_i) once per instance (threshold_crypto, hoisted out of
 *   every share verification); h96 (optional) = the compressed points.  The call returns once the
 *   nonces are uploaded (with h96, once the hashes are in h96); later coin calls on any stream are
 *   ordered after the hashing, and only hbx_sign waits for the true H (the checks and the combine
 *   work on [m] H).
 * hbx_sign -- SecretKeyShare::sign (src/common_coin.rs:142): sig96[inst][i] = sk_i * hash_g2(nonce).
 * hbx_verify_sig_shares -- PublicKeyShare::verify (src/common_coin.rs:151) for a [count][n] matrix
 *   of compressed signature shares (present_bits NULL = all present); uses hbx_set_pk_shares keys.
 *   Bit inst*n+i = e(pk_i, H) == e(g1, sig_i); absent / undecodable / unknown sender -> 0.
 * hbx_combine_signatures -- PublicKeySet::combine_signatures over the first t valid shares in
 *   node-index order (src/common_coin.rs:190) + PublicKey::verify with the master key (:196) +
 *   Signature::parity (:173).  status[inst]: HBX_OK / HBX_E_NOT_ENOUGH_SHARES.
 * Device variants (torch-style HBM buffers, `stream` as in the threshold _d calls):
 * hbx_verify_sig_shares_d -- d_sig96 [count][n][96], d_present [count][n] bytes (NULL = all),
 *   d_status [count][n] = HBX_SHARE_* (NULL: keep them in the context only).
 * hbx_combine_signatures_d -- as hbx_combine_signatures over the last verification's valid shares,
 *   restricted to d_use[inst][i] != 0 when d_use is given (the shares a node held when try_output
 *   ran, common_coin.rs:163-190); outputs d_sig96 [I][96], d_status [I] int32, d_master_ok [I] and
 *   d_parity [I] bytes (each may be NULL).  The master key is a host pointer (48 bytes; decoded
 *   once per distinct value).
 * ------------------------------------------------------------------------------------------- */
int hbx_prepare_nonces(hbx_ctx* ctx, const uint8_t* nonce_blob, const uint64_t* nonce_off, uint32_t count,
                       uint8_t* h96);
int hbx_sign(hbx_ctx* ctx, const uint8_t* sk32, uint32_t n, uint8_t* sig96);
int hbx_verify_sig_shares(hbx_ctx* ctx, const uint8_t* sig96, const uint8_t* present_bits, uint32_t n,
                          uint32_t count, uint8_t* valid_bits);
/* HBX_SHARE_* status of every share of the last hbx_verify_sig_shares (count x n bytes). */
int hbx_get_sig_share_status(hbx_ctx* ctx, uint8_t* status, size_t count);
int hbx_combine_signatures(hbx_ctx* ctx, const uint8_t* master_pk48, uint32_t t, uint8_t* sig96,
                           int32_t* status, uint8_t* master_ok_bits, uint8_t* parity_bits);
int hbx_verify_sig_shares_d(hbx_ctx* ctx, const uint8_t* d_sig96, const uint8_t* d_present, uint32_t n,
                            uint32_t count, uint8_t* d_status, void* stream);
int hbx_combine_signatures_d(hbx_ctx* ctx, const uint8_t* master_pk48, uint32_t t, const uint8_t* d_use,
                             uint8_t* d_sig96, int32_t* d_status, uint8_t* d_master_ok, uint8_t* d_parity,
                             void* stream);
/* Lanes per check the last signature-share verification used (1 or 2; 0 before any): the coin
 * honours hbx_set_verify_lanes 1 and 2; 0, 3, 6 and 7 choose automatically (2 when one-lane checks
 * would fill fewer than 1024 waves, else 1). */
int hbx_get_coin_lanes_used(const hbx_ctx* ctx);

/* ---------------------------------------------------------------------------------------------
 * Common Coin, incremental: the signature shares that arrive while a node runs its coin instances,
 * verified on arrival and merged into the round's [I][n] matrix, and the combine of the instances
 * that crossed the threshold.  Where hbx_verify_sig_shares[_d] and hbx_combine_signatures[_d]
 * decide a finished round, these serve a node that is running one.
 *
 * hbx_add_sig_shares[_d] -- CommonCoin::handle_share (src/common_coin.rs:149-161).  Item k is the
 * 96 bytes sig96[k] for position (inst[k] < I prepared nonces, sender[k] = node index); the launch
 * covers the tiles of the check kernels that the items touch, not I * n.  Lanes per check: the
 * matrix call's rule over the touched one-lane tiles (2 when fewer than 1024, else 1;
 * hbx_set_verify_lanes 1 / 2 override); hbx_get_coin_lanes_used, hbx_debug_force_fallback and
 * hbx_get_fallback_lanes mean for an add what they mean for a matrix verification.
 *
 * The matrix: after a hbx_verify_sig_shares[_d] since the latest hbx_prepare_nonces the add
 * continues from that call's matrix (n must be its n).  Otherwise the first add establishes a matrix
 * of width n with every entry HBX_SHARE_ABSENT, without any pairing work; count == 0 is allowed
 * (pointers may then be NULL) and only does that.  hbx_prepare_nonces, hbx_set_digest and
 * hbx_set_pk_shares void the matrix.
 *
 * status[k] for sender[k] < n is the HBX_SHARE_* byte hbx_verify_sig_shares_d writes for the same
 * bytes at (inst[k], sender[k]): HBX_SHARE_UNKNOWN_SENDER for n_keys <= sender < n, and
 * HBX_SHARE_UNDECODABLE for a point on the curve but outside G2.  sender[k] >= n touches no
 * position: HBX_SHARE_UNDECODABLE when the bytes do not decode to a point of G2 (the reference never
 * sees a message serde rejects), else HBX_SHARE_UNKNOWN_SENDER (Err(UnknownSender), :158).
 * Merge: an entry that is HBX_SHARE_VALID keeps its point and status when the item is not VALID
 * (the fault is returned before `insert`, :151-155); in every other case the entry takes the item's
 * status, and its point where it decoded (`insert`, :156).  No other entry changes, so delivering
 * every share of a round once, in any partition into calls, leaves hbx_get_sig_share_status and
 * every combine as one matrix call does.
 *
 * HBX_E_INVALID_ARG before anything is launched, nothing changed: inst[k] >= I; the same
 * (inst, sender) twice in one call (the second message of a pair goes into a later call); n
 * different from the matrix's; n == 0.  HBX_E_NO_KEYS / HBX_E_NO_CIPHERTEXTS as for the matrix call.
 * The host index arrays are consumed before the call returns.  The _d form is stream-ordered and
 * does not synchronise (d_status may be NULL); the host form blocks.
 *
 * hbx_combine_signatures_insts[_d] -- try_output and combine_and_verify_sig (src/common_coin.rs:163-207)
 * for the listed instances only: what hbx_combine_signatures_d does (the first t VALID entries in
 * index order at call time, restricted by d_use [I][n] when given), writing only the listed
 * instances' entries of the four outputs ([I][96], [I] int32, [I], [I] bytes; each may be NULL): no
 * other byte changes.  insts (HOST, consumed before the call returns): an instance >= I or one
 * listed twice is HBX_E_INVALID_ARG; ninsts == 0 returns HBX_OK and does nothing.  The host form
 * takes use as bytes [I][n] (or NULL) and writes master_ok / parity as bytes [I], not bits.
 * ------------------------------------------------------------------------------------------- */
int hbx_add_sig_shares_d(hbx_ctx* ctx, const uint8_t* d_sig96 /* [count][96] */,
                         const uint32_t* inst /* HOST [count] */, const uint32_t* sender /* HOST [count] */,
                         uint32_t count, uint32_t n, uint8_t* d_status /* [count], may be NULL */, void* stream);
int hbx_add_sig_shares(hbx_ctx* ctx, const uint8_t* sig96, const uint32_t* inst, const uint32_t* sender,
                       uint32_t count, uint32_t n, uint8_t* status);
int hbx_combine_signatures_insts_d(hbx_ctx* ctx, const uint8_t* master_pk48, uint32_t t,
                                   const uint32_t* insts /* HOST [ninsts] */, uint32_t ninsts,
                                   const uint8_t* d_use /* [I][n] or NULL */, uint8_t* d_sig96 /* [I][96] */,
                                   int32_t* d_status /* [I] */, uint8_t* d_master_ok, uint8_t* d_parity, void* stream);
int hbx_combine_signatures_insts(hbx_ctx* ctx, const uint8_t* master_pk48, uint32_t t, const uint32_t* insts,
                                 uint32_t ninsts, const uint8_t* use /* bytes [I][n] or NULL */, uint8_t* sig96,
                                 int32_t* status, uint8_t* master_ok /* bytes [I] */, uint8_t* parity /* bytes [I] */);
/* Check blocks (64-thread tiles) of the last signature-share check launch: grid.x * grid.y for a
 * matrix verification, the tile-list length for an add (0 when no item had sender < n); 0 before
 * any.  Diagnostics: no reference counterpart. */
uint32_t hbx_get_coin_tiles_used(const hbx_ctx* ctx);

/* ---------------------------------------------------------------------------------------------
 * Dynamic HoneyBadger / key-generation signatures: threshold_crypto
 * PublicKey::verify(sig, msg) = e(pk, hash_g2(msg)) == e(g1, sig) for `count` independent items,
 * each with its own key, message and signature -- the signed votes of
 * src/dynamic_honey_badger/votes.rs:151-156 (msg = bincode(vote)) and the key-generation messages
 * of src/dynamic_honey_badger/dynamic_honey_badger.rs:395-410 (msg = bincode(kg_msg)).
 *   pk48[count][48], sig96[count][96] compressed; msg_off[count + 1] byte offsets into msg_blob.
 *   status[count] = HBX_SHARE_VALID (true), HBX_SHARE_INVALID (false), HBX_SHARE_UNDECODABLE (the
 *   key or the signature is not a subgroup point: the reference cannot deserialise it).
 *   hash_g2 uses the context's digest (hbx_set_digest).  Independent of the coin state.
 * ------------------------------------------------------------------------------------------- */
int hbx_verify_sigs(hbx_ctx* ctx, const uint8_t* pk48, const uint8_t* msg_blob, const uint64_t* msg_off,
                    const uint8_t* sig96, uint32_t count, uint8_t* status);
/* hbx_verify_sigs_keyed -- the same check at the scale of a key-generation era, over a key table:
 * item i is verified under pk48[key_idx[i]].  Dynamic HoneyBadger checks every committed
 * SignedKeyGenMsg this way before handle_part / handle_ack sees it
 * (src/dynamic_honey_badger/dynamic_honey_badger.rs:254-272 process_output, and :395-410
 * verify_signature on arrival); a batch of signed votes (votes.rs:151-156) is a small call of the
 * same kind.  An era at N validators is N Parts + N^2 Acks under N distinct keys.
 *   pk48[nkeys][48]: decoded once per call (curve + G1 membership, the identity allowed);
 *   key_status (optional, nkeys entries) receives HBX_PT_* per key.
 *   key_idx[count], msg_off[count + 1] into msg_blob, sig96[count][96].
 *   status[i], decided in this order:
 *     HBX_SHARE_UNKNOWN_SENDER  key_idx[i] >= nkeys (0xFFFFFFFF is the "no key" value: the
 *                               reference's pk_opt is None); nothing else of the item is examined;
 *     HBX_SHARE_UNDECODABLE     the key's status is neither HBX_PT_OK nor HBX_PT_INFINITY, or the
 *                               signature bytes are not a point of G2;
 *     HBX_SHARE_VALID / HBX_SHARE_INVALID otherwise, with hbx_verify_sigs' identity rules (identity
 *                               key and identity signature: valid; exactly one identity: invalid).
 *   With nkeys == count and key_idx[i] = i the status bytes equal hbx_verify_sigs'.
 *   The items run in passes of 16,384 on lane pairs, without prepared line tables (about 2 KiB of
 *   device state per item of a pass).  hash_g2 uses the context's digest (hbx_set_digest).  The call
 *   blocks, and leaves the prepared ciphertexts and the coin state as they were.
 *   count == 0, nkeys == 0, a NULL required pointer or non-monotone offsets: HBX_E_INVALID_ARG before
 *   anything is launched.  hbx_debug_force_fallback applies per pass; hbx_get_fallback_lanes counts
 *   these checks as a kind of their own, summed over the call's passes.
 * hbx_sign_msgs -- threshold_crypto SecretKey::sign, which send_transaction
 * (dynamic_honey_badger.rs:363) runs on every Part and Ack a node sends and votes.rs:151-156 on every
 * vote: sig96[i] = compress(sk * hash_g2(msg_i)) under the context's digest.  sk32 is canonical
 * big-endian in [1, r) (HBX_E_INVALID_ARG otherwise).  Passes as above; no coin state is touched. */
int hbx_verify_sigs_keyed(hbx_ctx* ctx, const uint8_t* pk48, uint32_t nkeys, const uint32_t* key_idx,
                          const uint8_t* msg_blob, const uint64_t* msg_off, const uint8_t* sig96,
                          uint32_t count, uint8_t* status, int32_t* key_status /* optional, nkeys */);
int hbx_sign_msgs(hbx_ctx* ctx, const uint8_t* sk32, const uint8_t* msg_blob, const uint64_t* msg_off,
                  uint32_t count, uint8_t* sig96);
/* SyncKeyGen (src/sync_key_gen.rs) commitment checks over p Parts' BivarCommitments of degree t:
 *   commit48[p][(t+1)(t+2)/2][48], compressed, in threshold_crypto's coefficient order
 *   coeff_pos(i, j) = j (j + 1)/2 + i for i <= j (the symmetric matrix stored once).
 * hbx_bivar_rows -- BivarCommitment::row(x) (sync_key_gen.rs:313 `commit.row(idx + 1)`, :401):
 *   rows48[p][t + 1][48] = sum_i C_ij x^i; status[p] = HBX_SHARE_VALID, or HBX_SHARE_UNDECODABLE
 *   when a point of the commitment is not in G1 (the Part does not deserialise).
 * hbx_bivar_check_acks -- handle_ack's value check (sync_key_gen.rs:449):
 *   commit[ack_proposer[k]].evaluate(x, ack_y[k]) == g1 * val_k with val_k = vals32[k] (32-byte
 *   big-endian Fr; x = our_idx + 1, y = sender_idx + 1).  status[k] = HBX_SHARE_VALID (equal),
 *   HBX_SHARE_INVALID ("wrong value"), HBX_SHARE_UNDECODABLE (val >= r or the commitment does
 *   not decode). */
int hbx_bivar_rows(hbx_ctx* ctx, const uint8_t* commit48, uint32_t p, uint32_t t, uint64_t x, uint8_t* rows48,
                   uint8_t* status);
int hbx_bivar_check_acks(hbx_ctx* ctx, const uint8_t* commit48, uint32_t p, uint32_t t, uint64_t x,
                         const uint32_t* ack_proposer, const uint64_t* ack_y, const uint8_t* vals32, uint32_t count,
                         uint8_t* status);

/* ---------------------------------------------------------------------------------------------
 * SyncKeyGen end to end (src/sync_key_gen.rs): what surrounds the two
 * commitment checks above.  Host-pointer forms; scalars are canonical 32-byte big-endian Fr
 * (HBX_E_INVALID_ARG otherwise).  Plaintext framing is the caller's: the engine sees byte strings
 * and raw scalars (DESIGN.md "Key generation": threshold_crypto's serde framing is parity-unpinned).
 * Commitments (`our_part.commitment()` :291, `row.commitment()` :334) are hbx_public_keys applied
 * to the coefficients: g1 * 0 is the identity encoding (0xC0, 47 zero bytes).
 *
 * hbx_encrypt_to -- PublicKey::encrypt to a DIFFERENT key per message: the encrypted rows of a Part
 *   (sync_key_gen.rs:295, `pk.encrypt(&bytes)` per node) and the encrypted values of an Ack (:345).
 *   As hbx_encrypt with pk48[count][48]; a key that does not decode to a G1 point other than the
 *   identity is HBX_E_INVALID_ARG.
 * hbx_sk_decrypt -- SecretKey::decrypt of our row of a Part (:326) and of our value of an Ack
 *   (:444): Ciphertext::verify, then V xor hash_bytes(sk U, |V|), under the node's individual secret
 *   key sk32 (not its threshold share).  status[count] = HBX_CT_*; out_blob (at the v_off offsets)
 *   holds the plaintext where the status is HBX_CT_VALID and zeros elsewhere (the reference returns
 *   None there).  Ciphertext::verify runs through the prepared-ciphertext path in chunks, or, after
 *   hbx_set_ct_check(HBX_CT_CHECK_PAIR), on one lane pair per ciphertext without prepared line tables
 *   (larger chunks, about 2 KiB of device state per ciphertext instead of about 100 KiB; the same
 *   status bytes and plaintexts).  In either mode own-share mode stays as it was, but the epoch's
 *   prepared ciphertexts are void afterwards, as after hbx_set_digest (a share verification then
 *   returns HBX_E_NO_CIPHERTEXTS until the next prepare).
 * hbx_set_ct_check -- how hbx_sk_decrypt runs Ciphertext::verify: HBX_CT_CHECK_WIDE (default) or
 *   HBX_CT_CHECK_PAIR; any other value is HBX_E_INVALID_ARG.  No reference counterpart; it governs
 *   hbx_sk_decrypt only (the epoch's prepares keep the wide executor or the own-share fusion).
 * hbx_get_ct_check_used -- the mode the last hbx_sk_decrypt ran; -1 before any call.
 * hbx_bivar_poly_rows -- BivarPoly::row(x) for x = 1..n (:293 `our_part.row(i + 1)`) of the dealer's
 *   polynomial coeff32[(t+1)(t+2)/2][32] in coeff_pos order: rows32[n][t + 1][32].
 * hbx_fr_poly_eval -- Poly::evaluate (:341 `row.evaluate(idx + 1)`) of p polynomials
 *   coeff32[p][t + 1][32] at x = 1..n: out32[p][n][32].
 * hbx_keygen_generate -- SyncKeyGen::generate (:396-409) over p Parts' commitments
 *   commit48[p][(t+1)(t+2)/2][48]: pk_commit48[t + 1][48] = sum over the parts with complete[q] != 0 of
 *   commit_q.row(0) (:401), and sk32_out = sum over those parts of
 *   Poly::interpolate(values_q).evaluate(0) (:404-407) over the part's val_cnt[q] <= t + 1 points
 *   (val_y[q][k], vals32[q][k]) (y = sender index + 1; a part with no point adds 0, fewer than t + 1
 *   points interpolate through what there is).  sk32_out NULL (an observer): val_* are not read.
 *   status[p]: HBX_SHARE_VALID, HBX_SHARE_ABSENT for a part that is not complete (not examined),
 *   HBX_SHARE_UNDECODABLE for a complete part whose commitment holds a non-G1 point -- the call then
 *   returns HBX_E_INVALID_ARG without writing the other outputs (the reference cannot hold such a
 *   Part).  A repeated y within a complete part is HBX_E_DUPLICATE_ENTRY.
 * hbx_pk_shares_from_commit -- PublicKeySet::public_key_share(i) = commit.evaluate(i + 1)
 *   (src/messaging.rs:251-254) for i < n: pk48[n][48], the input of hbx_set_pk_shares.
 * ------------------------------------------------------------------------------------------- */
int hbx_encrypt_to(hbx_ctx* ctx, const uint8_t* pk48, const uint8_t* msg_blob, const uint64_t* msg_off,
                   uint32_t count, const uint8_t* r32, uint8_t* u48, uint8_t* v_blob, uint8_t* w96);
int hbx_sk_decrypt(hbx_ctx* ctx, const uint8_t* sk32, const uint8_t* u48, const uint8_t* v_blob,
                   const uint64_t* v_off, const uint8_t* w96, uint32_t count, uint8_t* out_blob, uint8_t* status);
#define HBX_CT_CHECK_WIDE 0
#define HBX_CT_CHECK_PAIR 1
int hbx_set_ct_check(hbx_ctx* ctx, int mode);
int hbx_get_ct_check_used(const hbx_ctx* ctx);
int hbx_bivar_poly_rows(hbx_ctx* ctx, const uint8_t* coeff32, uint32_t t, uint32_t n, uint8_t* rows32);
int hbx_fr_poly_eval(hbx_ctx* ctx, const uint8_t* coeff32, uint32_t p, uint32_t t, uint32_t n, uint8_t* out32);
int hbx_keygen_generate(hbx_ctx* ctx, const uint8_t* commit48, uint32_t p, uint32_t t, const uint8_t* complete,
                        const uint32_t* val_cnt, const uint64_t* val_y, const uint8_t* vals32, uint8_t* pk_commit48,
                        uint8_t* sk32_out, uint8_t* status);
int hbx_pk_shares_from_commit(hbx_ctx* ctx, const uint8_t* pk_commit48, uint32_t t, uint32_t n, uint8_t* pk48);

/* ---------------------------------------------------------------------------------------------
 * Broadcast: Reed-Solomon erasure coding and the Merkle tree over shards (SURVEY.md §8 rows
 * C1-C5d), batched over `inst` broadcast instances.  Device pointers, stream-ordered.
 * Shards of one instance are contiguous: d_shards[inst][k + m][L]; leaf i of an instance is the
 * index byte i followed by shard i (src/broadcast.rs:373-377).  Requires k + m <= 256, k <= 128.
 *
 * hbx_rs_encode_d -- ReedSolomon::encode (reed-solomon-erasure 3.1.0) via Coding::encode
 *   (src/broadcast.rs:632-640, called at :365): fills the m parity shards of every instance.
 * hbx_rs_reconstruct_d -- ReedSolomon::reconstruct_shards via Coding::reconstruct_shards
 *   (src/broadcast.rs:643-657, called at :667): rebuilds every shard whose d_present byte is 0
 *   from the first k present shards.  d_status[inst]: HBX_OK or HBX_E_TOO_FEW_SHARDS.
 * hbx_merkle_roots_d -- MerkleTree::from_vec(&SHA256, leaves).root_hash() (src/broadcast.rs:381,
 *   :683-686) over the index-prefixed shards: d_roots[inst][32].
 * hbx_merkle_validate_d -- Broadcast::validate_proof (src/broadcast.rs:555-575):
 *   Proof::validate(&root_hash) && node_index(sender) == value[0] && Proof::index(count) == value[0],
 *   for nproofs flattened proofs: d_values[j][vlen] (the leaf: index byte + shard),
 *   d_node_hash[j][17][32] (lemma node hashes from the root down to the leaf hash),
 *   d_sib_hash[j][16][32], d_sides[j] (bit l: the level-l sibling is Positioned::Left),
 *   d_depth[j], d_root[j][32] (the proof's root_hash), d_sender[j]; d_valid[j] out.
 * hbx_broadcast_decode_d -- decode_from_shards + glue_shards (src/broadcast.rs:660-707):
 *   reconstruct, rebuild the tree, compare with d_root_expect[inst][32], glue the first k shards.
 *   d_out[inst][out_stride], d_out_len[inst], d_status[inst]: HBX_OK / HBX_E_TOO_FEW_SHARDS /
 *   HBX_E_ROOT_MISMATCH / HBX_E_NO_PAYLOAD.  With m == 0 (Coding::Trivial) any absent shard
 *   is HBX_E_TOO_FEW_SHARDS.
 * ------------------------------------------------------------------------------------------- */
int hbx_rs_encode_d(hbx_ctx* ctx, uint8_t* d_shards, uint32_t inst, uint32_t k, uint32_t m, uint32_t L,
                    void* stream);
int hbx_rs_reconstruct_d(hbx_ctx* ctx, uint8_t* d_shards, const uint8_t* d_present, uint32_t inst, uint32_t k,
                         uint32_t m, uint32_t L, int32_t* d_status, void* stream);
int hbx_merkle_roots_d(hbx_ctx* ctx, const uint8_t* d_shards, uint32_t inst, uint32_t n, uint32_t L,
                       uint8_t* d_roots, void* stream);
int hbx_merkle_validate_d(hbx_ctx* ctx, const uint8_t* d_values, uint32_t vlen, const uint8_t* d_node_hash,
                          const uint8_t* d_sib_hash, const uint32_t* d_sides, const uint32_t* d_depth,
                          const uint8_t* d_root, const uint32_t* d_sender, uint32_t count, uint32_t nproofs,
                          uint8_t* d_valid, void* stream);
/* hbx_merkle_build_d -- MerkleTree::from_vec over the index-prefixed shards, keeping the whole
 *   tree (SURVEY.md §8(b) hbx_merkle_build): d_nodes[inst][hbx_merkle_node_count(n)][32], the
 *   levels from the n leaf digests up to the root (last), a promoted odd node repeated on the
 *   level it moves to; d_roots[inst][32] optional.
 * hbx_merkle_proofs_d -- MerkleTree::gen_proof (src/broadcast.rs:389-401: one Value proof per
 *   node) from such trees: proof q for leaf d_req[2q + 1] of instance d_req[2q] (the proof of the
 *   first leaf with an equal digest, as merkle.rs finds the first equal value), written in the
 *   format hbx_merkle_validate_d reads (d_node_hash[q][17][32] root first, d_sib_hash[q][16][32],
 *   d_sides[q], d_depth[q], d_root[q][32]). */
uint32_t hbx_merkle_node_count(uint32_t n);
int hbx_merkle_build_d(hbx_ctx* ctx, const uint8_t* d_shards, uint32_t inst, uint32_t n, uint32_t L,
                       uint8_t* d_nodes, uint8_t* d_roots, void* stream);
int hbx_merkle_proofs_d(hbx_ctx* ctx, const uint8_t* d_nodes, uint32_t n, const uint32_t* d_req, uint32_t count,
                        uint8_t* d_node_hash, uint8_t* d_sib_hash, uint32_t* d_sides, uint32_t* d_depth,
                        uint8_t* d_root, void* stream);
int hbx_broadcast_decode_d(hbx_ctx* ctx, uint8_t* d_shards, const uint8_t* d_present,
                           const uint8_t* d_root_expect, uint32_t inst, uint32_t k, uint32_t m, uint32_t L,
                           uint8_t* d_out, uint64_t out_stride, uint64_t* d_out_len, int32_t* d_status,
                           void* stream);
/* hbx_broadcast_decode_leaves_d -- the same decode for Echo values that were validated
 *   (hbx_merkle_validate_d): d_leaf_hash[inst][k + m][32] holds, for every present shard, the leaf
 *   digest its Echo proof carries (the last lemma node, which validation proved equal to the digest
 *   of the value).  compute_output rebuilds the tree over those same bytes (broadcast.rs:530-544,
 *   :683), so only the reconstructed shards are hashed.  Same outputs as
 *   hbx_broadcast_decode_d when the digests are the values' own. */
int hbx_broadcast_decode_leaves_d(hbx_ctx* ctx, uint8_t* d_shards, const uint8_t* d_present,
                                  const uint8_t* d_leaf_hash, const uint8_t* d_root_expect, uint32_t inst,
                                  uint32_t k, uint32_t m, uint32_t L, uint8_t* d_out, uint64_t out_stride,
                                  uint64_t* d_out_len, int32_t* d_status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Broadcast, ragged forms: per-instance shard lengths in one call.  Each proposer frames its own
 * contribution with shard_len = ceil((len + 4) / (N - 2f)) (src/broadcast.rs:341-353), so the N
 * instances at one node have N shard lengths; these calls take them all at once.
 *
 * Layout: one device byte buffer d_buf[buf_bytes] holds every instance.  Instance q is described
 * by three HOST arrays of `inst` entries: off[q] (byte offset of its row 0), len[q] (its shard
 * length, >= 1) and pitch[q] (its row pitch, >= len[q]); row i (i < k + m) is at
 * off[q] + i * pitch[q].  Required, else HBX_E_INVALID_ARG before anything is launched:
 * off[q] % 4 == 0, pitch[q] % 4 == 0, pitch[q] >= len[q] >= 1, off[q] + (k + m) * pitch[q] <=
 * buf_bytes, and no two instances' ranges overlap.  The host arrays (val_off and out_off below
 * too) are consumed before the call returns.  Pad bytes [len, pitch) of a row are never part of a
 * result: they may hold anything, and their content after a call is unspecified; no byte outside
 * [off[q], off[q] + (k + m) * pitch[q]) of any instance is written.  Rows are dword rows whatever
 * their length, so every length runs the byte-permute coding kernel.  Device pointers,
 * stream-ordered; k + m <= 256, k <= 128, one (k, m) per call.
 *
 * hbx_rs_encode_ragged_d -- Coding::encode (src/broadcast.rs:632-640, called at :365) for every
 *   instance; m == 0 is a no-op.
 * hbx_rs_reconstruct_ragged_d -- Coding::reconstruct_shards (src/broadcast.rs:643-657, called at
 *   :667): d_present[inst][k + m]; d_status[inst] HBX_OK or HBX_E_TOO_FEW_SHARDS.
 * hbx_merkle_build_ragged_d -- MerkleTree::from_vec (src/broadcast.rs:381) over the leaves
 *   [i] || row i's len[q] bytes: d_nodes[inst][hbx_merkle_node_count(n)][32] and d_roots[inst][32],
 *   either may be NULL (not both); both HBX_MERKLE_* variants.  The nodes feed hbx_merkle_proofs_d.
 * hbx_merkle_validate_ragged_d -- Broadcast::validate_proof (src/broadcast.rs:555-575) for values
 *   of any lengths in one call: value j is d_values[val_off[j] .. val_off[j + 1]) (val_off: HOST
 *   array of nproofs + 1 non-decreasing offsets, val_off[nproofs] <= values_bytes); the other
 *   arrays as hbx_merkle_validate_d.  A zero-length value is invalid (d_valid[j] = 0), not an
 *   error.  The results do not depend on the order of the proofs.
 * hbx_broadcast_decode_ragged_d -- decode_from_shards + glue_shards (src/broadcast.rs:660-707) per
 *   instance, statuses as hbx_broadcast_decode_d.  Instance q's payload is written at
 *   d_out + out_off[q] (HOST array); each instance needs room for k * len[q] - 4 bytes there
 *   whenever k * len[q] >= 4 (within out_bytes, apart from the other instances' room), else
 *   HBX_E_INVALID_ARG; no other byte of d_out is written.  d_leaf_hash[inst][k + m][32] may be
 *   NULL; given, it is the leaf-sharing decode of hbx_broadcast_decode_leaves_d (only
 *   reconstructed shards are hashed).
 * ------------------------------------------------------------------------------------------- */
int hbx_rs_encode_ragged_d(hbx_ctx* ctx, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off,
                           const uint32_t* len, const uint32_t* pitch, uint32_t inst, uint32_t k, uint32_t m,
                           void* stream);
int hbx_rs_reconstruct_ragged_d(hbx_ctx* ctx, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off,
                                const uint32_t* len, const uint32_t* pitch, const uint8_t* d_present,
                                uint32_t inst, uint32_t k, uint32_t m, int32_t* d_status, void* stream);
int hbx_merkle_build_ragged_d(hbx_ctx* ctx, const uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off,
                              const uint32_t* len, const uint32_t* pitch, uint32_t inst, uint32_t n,
                              uint8_t* d_nodes, uint8_t* d_roots, void* stream);
int hbx_merkle_validate_ragged_d(hbx_ctx* ctx, const uint8_t* d_values, uint64_t values_bytes,
                                 const uint64_t* val_off, const uint8_t* d_node_hash, const uint8_t* d_sib_hash,
                                 const uint32_t* d_sides, const uint32_t* d_depth, const uint8_t* d_root,
                                 const uint32_t* d_sender, uint32_t count, uint32_t nproofs, uint8_t* d_valid,
                                 void* stream);
int hbx_broadcast_decode_ragged_d(hbx_ctx* ctx, uint8_t* d_buf, uint64_t buf_bytes, const uint64_t* off,
                                  const uint32_t* len, const uint32_t* pitch, const uint8_t* d_present,
                                  const uint8_t* d_leaf_hash, const uint8_t* d_root_expect, uint32_t inst,
                                  uint32_t k, uint32_t m, uint8_t* d_out, uint64_t out_bytes,
                                  const uint64_t* out_off, uint64_t* d_out_len, int32_t* d_status, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Broadcast, message by message: the node that is running an epoch.  Echoes arrive a few at a
 * time; each is validated once, on arrival, and its value stays on the device until its
 * instance's compute_output decodes it (src/broadcast.rs:521-551).
 *
 * hbx_prepare_broadcast -- the echo store of `inst` instances x n = k + m senders (k + m <= 256,
 *   k <= 128).  Slot (q, i) holds the first validated Echo value of sender i in instance q: a state
 *   byte (0 empty, 1 held), the shard length and bytes (the value without its index byte; rows of
 *   max_shard_len rounded up to 4), the proof's root and its leaf digest (the last lemma node).  A
 *   value longer than max_shard_len + 1 bytes cannot be held (HBX_ECHO_OVERSIZE): max_shard_len is
 *   the caller's transport bound, the store does not grow.  A second prepare with the same
 *   dimensions only empties the slots.  hbx_set_merkle_digest voids the store (its values were
 *   validated under the other digest); the calls below return HBX_E_NO_BROADCAST on a voided or
 *   never prepared store.
 *
 * hbx_add_echoes[_d] -- Broadcast::handle_echo up to echos.insert (src/broadcast.rs:439-458), and
 *   handle_value -> send_echo -> handle_echo(our_uid) (:407-436, :494-504): a Value from the
 *   proposer is an item with sender = this node.  Item j is value
 *   d_values[val_off[j] .. val_off[j + 1]) (val_off: HOST, count + 1 entries) with the flattened
 *   proof j of hbx_merkle_validate_ragged_d, for slot (inst[j], sender[j]) (HOST arrays, consumed at
 *   return).  d_status[count] (may be NULL), one HBX_ECHO_* byte per item:
 *     HBX_ECHO_DUPLICATE  the slot is already held; the bytes are not looked at (:441-448);
 *     HBX_ECHO_OVERSIZE   the value is longer than max_shard_len + 1; not validated, not stored;
 *     HBX_ECHO_INVALID    validate_proof(p, sender) is false -- the bit hbx_merkle_validate_ragged_d
 *                         writes for the same proof and sender (an empty value is invalid); the slot
 *                         stays empty, so a later Echo of that sender is still looked at;
 *     HBX_ECHO_STORED     valid and the slot was empty: it takes length, bytes, root, leaf digest.
 *   No other slot changes, so any partition of an epoch's Echoes into calls that keeps each (inst,
 *   sender) pair's own order leaves the same store.  HBX_E_INVALID_ARG before anything is launched,
 *   nothing changed: inst[j] >= the store's instance count; sender[j] >= n; the same (inst, sender)
 *   twice in one call (repeats go into later calls); val_off decreasing or ending past
 *   values_bytes.  count == 0 does nothing.  The _d form is stream-ordered and does not
 *   synchronise; the host form blocks.
 *
 * hbx_broadcast_decode_insts[_d] -- compute_output's decode_from_shards + glue_shards
 *   (src/broadcast.rs:530-551, :660-707) for the listed attempts only.  Attempt a = instance
 *   insts[a], root roots[a][32], shard length len[a] (>= 1, <= max_shard_len) and, optionally,
 *   use[a][n] bytes: the Echo senders held when the trigger fired (NULL: all).  insts, roots, len,
 *   use and out_off are HOST arrays, consumed at return.  Shard i is present iff use allows it, slot
 *   (insts[a], i) is held and its root is roots[a].  d_status[a]: HBX_E_SHARD_SIZE if a present
 *   slot's length is not len[a] (decode_from_shards returns None: the crate checks shard sizes
 *   before it counts shards, so this code wins over HBX_E_TOO_FEW_SHARDS when both apply); every
 *   other status, d_out / out_off / d_out_len as hbx_broadcast_decode_ragged_d.  The store is never
 *   written: the present rows are copied into a work buffer the context owns and reconstructed
 *   there, so a failed attempt can be retried with later Echoes (:543-550) and slots holding
 *   another root survive.  HBX_E_INVALID_ARG before any launch: an instance beyond the store's;
 *   the same (instance, root, use row) twice; len[a] == 0 or > max_shard_len; more than 65535
 *   attempts in one call; output room as in the ragged decode (d_out may be NULL only when
 *   out_bytes == 0).  na == 0 returns HBX_OK.  A use byte allows its sender iff it is non-zero; two
 *   rows that allow the same senders are the same row.
 *
 * hbx_get_echo_slots -- the store as the host sees it (diagnostics, tests): state[inst][n],
 *   len[inst][n], root[inst][n][32]; any may be NULL.  hbx_debug_get_echo_rows (tests only, like
 *   hbx_debug_live_buffers): the first `bytes` bytes of the shard rows (inst * n rows of the row
 *   pitch, then one canary row of 0xA5 that nothing may write).
 * ------------------------------------------------------------------------------------------- */
#define HBX_ECHO_INVALID 0
#define HBX_ECHO_STORED 1
#define HBX_ECHO_DUPLICATE 2
#define HBX_ECHO_OVERSIZE 3
int hbx_prepare_broadcast(hbx_ctx* ctx, uint32_t inst, uint32_t k, uint32_t m, uint32_t max_shard_len);
int hbx_add_echoes_d(hbx_ctx* ctx, const uint8_t* d_values, uint64_t values_bytes, const uint64_t* val_off,
                     const uint8_t* d_node_hash, const uint8_t* d_sib_hash, const uint32_t* d_sides,
                     const uint32_t* d_depth, const uint8_t* d_root, const uint32_t* inst, const uint32_t* sender,
                     uint32_t count, uint8_t* d_status, void* stream);
int hbx_add_echoes(hbx_ctx* ctx, const uint8_t* values, uint64_t values_bytes, const uint64_t* val_off,
                   const uint8_t* node_hash, const uint8_t* sib_hash, const uint32_t* sides, const uint32_t* depth,
                   const uint8_t* root, const uint32_t* inst, const uint32_t* sender, uint32_t count,
                   uint8_t* status);
int hbx_broadcast_decode_insts_d(hbx_ctx* ctx, const uint32_t* insts, const uint8_t* roots, const uint32_t* len,
                                 const uint8_t* use, uint32_t na, uint8_t* d_out, uint64_t out_bytes,
                                 const uint64_t* out_off, uint64_t* d_out_len, int32_t* d_status, void* stream);
int hbx_broadcast_decode_insts(hbx_ctx* ctx, const uint32_t* insts, const uint8_t* roots, const uint32_t* len,
                               const uint8_t* use, uint32_t na, uint8_t* out, uint64_t out_bytes,
                               const uint64_t* out_off, uint64_t* out_len, int32_t* status);
int hbx_get_echo_slots(hbx_ctx* ctx, uint8_t* state, uint32_t* len, uint8_t* root);
int hbx_debug_get_echo_rows(hbx_ctx* ctx, uint8_t* rows, uint64_t bytes);

/* Host-pointer forms of the Broadcast calls: the same operations and layouts on HOST buffers,
 * staged through device buffers the context owns, on the context's own stream; they block until
 * the outputs are back (the stack-A/B convention above).  What a thin Rust FFI calls from
 * Vec<u8> / &[u8] without a HIP runtime binding of its own:
 *   hbx_rs_encode          Coding::encode / ReedSolomon::encode (src/broadcast.rs:632-640, called at
 *                          :366): shards[inst][k + m][L]; reads the k data rows, writes the m parity
 *                          rows of every instance.
 *   hbx_rs_reconstruct     Coding::reconstruct_shards (src/broadcast.rs:643-657, called at :667):
 *                          present[inst][k + m] bytes; shards rewritten in place, status[inst].
 *   hbx_merkle_roots       MerkleTree::from_vec(..).root_hash() (src/broadcast.rs:381): roots[inst][32].
 *   hbx_merkle_build       the whole tree (src/broadcast.rs:381): nodes[inst][hbx_merkle_node_count(n)][32],
 *                          roots optional.
 *   hbx_merkle_proofs      MerkleTree::gen_proof (src/broadcast.rs:389-401) from hbx_merkle_build's
 *                          nodes of `inst` instances: req[count][2] = (instance, leaf); outputs as
 *                          hbx_merkle_proofs_d, sides[count] and depth[count] as uint32.
 *   hbx_merkle_validate    Broadcast::validate_proof (src/broadcast.rs:555-575, called for Value at
 *                          :430 and Echo at :451); arrays as hbx_merkle_validate_d, valid[nproofs].
 *   hbx_broadcast_decode   decode_from_shards + glue_shards (src/broadcast.rs:660-707): shards
 *                          rewritten in place (reconstructed rows), out[inst][out_stride],
 *                          out_len[inst], status[inst].
 *   hbx_broadcast_decode_leaves  the same with the validated Echo proofs' leaf digests
 *                          (leaf_hash[inst][k + m][32]). */
int hbx_rs_encode(hbx_ctx* ctx, uint8_t* shards, uint32_t inst, uint32_t k, uint32_t m, uint32_t L);
int hbx_rs_reconstruct(hbx_ctx* ctx, uint8_t* shards, const uint8_t* present, uint32_t inst, uint32_t k, uint32_t m,
                       uint32_t L, int32_t* status);
int hbx_merkle_roots(hbx_ctx* ctx, const uint8_t* shards, uint32_t inst, uint32_t n, uint32_t L, uint8_t* roots);
int hbx_merkle_build(hbx_ctx* ctx, const uint8_t* shards, uint32_t inst, uint32_t n, uint32_t L, uint8_t* nodes,
                     uint8_t* roots);
int hbx_merkle_proofs(hbx_ctx* ctx, const uint8_t* nodes, uint32_t inst, uint32_t n, const uint32_t* req,
                      uint32_t count, uint8_t* node_hash, uint8_t* sib_hash, uint32_t* sides, uint32_t* depth,
                      uint8_t* root);
int hbx_merkle_validate(hbx_ctx* ctx, const uint8_t* values, uint32_t vlen, const uint8_t* node_hash,
                        const uint8_t* sib_hash, const uint32_t* sides, const uint32_t* depth, const uint8_t* root,
                        const uint32_t* sender, uint32_t count, uint32_t nproofs, uint8_t* valid);
int hbx_broadcast_decode(hbx_ctx* ctx, uint8_t* shards, const uint8_t* present, const uint8_t* root_expect,
                         uint32_t inst, uint32_t k, uint32_t m, uint32_t L, uint8_t* out, uint64_t out_stride,
                         uint64_t* out_len, int32_t* status);
int hbx_broadcast_decode_leaves(hbx_ctx* ctx, uint8_t* shards, const uint8_t* present, const uint8_t* leaf_hash,
                                const uint8_t* root_expect, uint32_t inst, uint32_t k, uint32_t m, uint32_t L,
                                uint8_t* out, uint64_t out_stride, uint64_t* out_len, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* HBX_H */
