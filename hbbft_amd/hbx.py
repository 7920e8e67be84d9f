"""ctypes binding of the C ABI in ``include/hbx.h`` (``hbbft_amd/libhbx.so``).

This is plumbing for tests, the bench and Python callers; the product is the C ABI itself.
There is deliberately no CPU fallback: if ``libhbx.so`` is missing or no HIP device is present,
construction fails with an exception naming what is missing.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HBX_LIB_PATH: an alternative in-tree build of the same library (kernel variants under test)
LIB_PATH = os.environ.get("HBX_LIB_PATH") or os.path.join(_HERE, "libhbx.so")

HBX_OK = 0
HBX_E_INVALID_ARG = -1
HBX_E_DEVICE = -2
HBX_E_NOT_ENOUGH_SHARES = -3
HBX_E_DUPLICATE_ENTRY = -4
HBX_E_NO_KEYS = -5
HBX_E_NO_CIPHERTEXTS = -6
HBX_E_INVALID_CIPHERTEXT = -7
HBX_E_OUT_OF_MEMORY = -8
HBX_E_TOO_FEW_SHARDS = -9
HBX_E_ROOT_MISMATCH = -10
HBX_E_NO_PAYLOAD = -11
HBX_E_NO_BROADCAST = -12
HBX_E_SHARD_SIZE = -13

# Every symbol include/hbx.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "hbx_ctx_create",
    "hbx_ctx_destroy",
    "hbx_last_error",
    "hbx_version",
    "hbx_set_pk_shares",
    "hbx_set_own_share",
    "hbx_prepare_ciphertexts",
    "hbx_verify_dec_shares",
    "hbx_combine_decrypt",
    "hbx_prepare_ciphertexts_d",
    "hbx_verify_dec_shares_d",
    "hbx_combine_decrypt_d",
    "hbx_get_ct_valid_d",
    "hbx_decrypt_epoch_d",
    "hbx_public_keys",
    "hbx_encrypt",
    "hbx_decrypt_shares",
    "hbx_prepare_nonces",
    "hbx_sign",
    "hbx_verify_sig_shares",
    "hbx_combine_signatures",
    "hbx_verify_sig_shares_d",
    "hbx_combine_signatures_d",
    "hbx_get_coin_lanes_used",
    "hbx_verify_sigs",
    "hbx_bivar_rows",
    "hbx_bivar_check_acks",
    "hbx_rs_encode_d",
    "hbx_rs_reconstruct_d",
    "hbx_merkle_roots_d",
    "hbx_merkle_validate_d",
    "hbx_broadcast_decode_d",
    "hbx_broadcast_decode_leaves_d",
    "hbx_set_timing",
    "hbx_kernel_time",
    "hbx_get_share_status",
    "hbx_get_ct_status",
    "hbx_get_sig_share_status",
    "hbx_get_ct_hashes",
    "hbx_set_digest",
    "hbx_set_merkle_digest",
    "hbx_set_verify_lanes",
    "hbx_get_verify_lanes_used",
    "hbx_set_combine_lanes",
    "hbx_debug_force_fallback",
    "hbx_debug_force_degenerate",
    "hbx_get_fallback_lanes",
    "hbx_debug_set_combine_margin",
    "hbx_get_combine_slow_terms",
    "hbx_build_id",
    "hbx_merkle_node_count",
    "hbx_merkle_build_d",
    "hbx_merkle_proofs_d",
    "hbx_rs_encode",
    "hbx_rs_reconstruct",
    "hbx_merkle_roots",
    "hbx_merkle_build",
    "hbx_merkle_proofs",
    "hbx_merkle_validate",
    "hbx_broadcast_decode",
    "hbx_broadcast_decode_leaves",
    "hbx_encrypt_to",
    "hbx_sk_decrypt",
    "hbx_bivar_poly_rows",
    "hbx_fr_poly_eval",
    "hbx_keygen_generate",
    "hbx_pk_shares_from_commit",
    "hbx_set_batch_verify",
    "hbx_get_batch_stats",
    "hbx_get_batch_sums",
    "hbx_rs_encode_ragged_d",
    "hbx_rs_reconstruct_ragged_d",
    "hbx_merkle_build_ragged_d",
    "hbx_merkle_validate_ragged_d",
    "hbx_broadcast_decode_ragged_d",
    "hbx_set_ct_check",
    "hbx_get_ct_check_used",
    "hbx_verify_sigs_keyed",
    "hbx_sign_msgs",
    "hbx_add_dec_shares_d",
    "hbx_add_dec_shares",
    "hbx_combine_decrypt_cols_d",
    "hbx_combine_decrypt_cols",
    "hbx_get_verify_tiles_used",
    "hbx_debug_live_buffers",
    "hbx_add_sig_shares_d",
    "hbx_add_sig_shares",
    "hbx_combine_signatures_insts_d",
    "hbx_combine_signatures_insts",
    "hbx_get_coin_tiles_used",
    "hbx_prepare_broadcast",
    "hbx_add_echoes_d",
    "hbx_add_echoes",
    "hbx_broadcast_decode_insts_d",
    "hbx_broadcast_decode_insts",
    "hbx_get_echo_slots",
    "hbx_debug_get_echo_rows",
)

DIGEST_SHA256 = 0
DIGEST_SHA3_256 = 1
MERKLE_SHA256 = 0
MERKLE_SHA3 = 1

# Per-share / per-ciphertext status bytes (include/hbx.h HBX_SHARE_*, HBX_CT_*)
SHARE_INVALID = 0
SHARE_VALID = 1
SHARE_ABSENT = 2
SHARE_UNDECODABLE = 3
SHARE_SKIPPED_CT = 4
SHARE_UNKNOWN_SENDER = 5
# hbx_add_echoes[_d] item statuses (include/hbx.h HBX_ECHO_*)
ECHO_INVALID = 0
ECHO_STORED = 1
ECHO_DUPLICATE = 2
ECHO_OVERSIZE = 3
CT_INVALID = 0
CT_VALID = 1
CT_UNDECODABLE = 3

# Ciphertext::verify of hbx_sk_decrypt (include/hbx.h HBX_CT_CHECK_*): the wide executor over prepared
# line tables (default), or one lane pair per ciphertext
CT_CHECK_WIDE = 0
CT_CHECK_PAIR = 1
# hbx_debug_set_combine_margin (include/hbx.h HBX_COMBINE_*)
COMBINE_MARGIN_AUTO = -1
COMBINE_TABLES_OFF = -2
# ciphertexts per pass of hbx_sk_decrypt in pair mode (hbbft_amd/csrc/hbx_api.hip SK_DECRYPT_PAIR_CHUNK)
SK_DECRYPT_PAIR_CHUNK = 16384
# items per pass of hbx_verify_sigs_keyed / hbx_sign_msgs (hbbft_amd/csrc/hbx_api.hip VERIFY_SIGS_CHUNK)
VERIFY_SIGS_CHUNK = 16384
# key_idx value of an item without a key (the reference's pk_opt is None): HBX_SHARE_UNKNOWN_SENDER
NO_KEY = 0xFFFFFFFF

# kernel ids of hbx_kernel_time (include/hbx.h)
KERNELS = {"prepare_ct": 0, "prepare_lines": 1, "ct_checks": 2, "verify_shares": 3, "combine": 4,
           "verify_sig": 5, "combine_sigs": 6, "rs_code": 7, "merkle_leaves": 8, "hash_nonces": 9,
           "decode_sigs": 10, "sk_decrypt": 11, "batch_msm": 12, "batch_check": 13}

_lib = None


class HbxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"hbx error {code}: {msg}")
        self.code = code


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libhbx.so (raises OSError with the path if it was not built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OSError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    # One HIP runtime per process: torch ships its own libamdhip64.so.7 (same SONAME as
    # /opt/rocm's, which libhbx.so links).  Whichever loads first serves both; if libhbx.so came
    # first, torch later finds "No HIP GPUs".  So torch (the device-memory plumbing of the _d
    # calls) is imported before the library whenever it is installed.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    P = ctypes.c_void_p
    u8p = ctypes.POINTER(ctypes.c_uint8)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    i32p = ctypes.POINTER(ctypes.c_int32)
    u32 = ctypes.c_uint32
    lib.hbx_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(P)]
    lib.hbx_ctx_destroy.argtypes = [P]
    lib.hbx_last_error.argtypes = [P]
    lib.hbx_last_error.restype = ctypes.c_char_p
    lib.hbx_version.restype = ctypes.c_char_p
    lib.hbx_build_id.restype = ctypes.c_char_p
    lib.hbx_set_pk_shares.argtypes = [P, u8p, u32, i32p]
    lib.hbx_set_own_share.argtypes = [P, u32, u8p]
    lib.hbx_prepare_ciphertexts.argtypes = [P, u8p, u8p, u64p, u8p, u32, u8p]
    lib.hbx_verify_dec_shares.argtypes = [P, u8p, u8p, u32, u32, u8p]
    lib.hbx_combine_decrypt.argtypes = [P, u32, u8p, i32p]
    lib.hbx_prepare_ciphertexts_d.argtypes = [P, P, P, P, P, u32, ctypes.c_uint64, P, P]
    lib.hbx_verify_dec_shares_d.argtypes = [P, P, P, u32, u32, P, P]
    lib.hbx_combine_decrypt_d.argtypes = [P, u32, P, P, P]
    lib.hbx_get_ct_valid_d.argtypes = [P, P, P]
    lib.hbx_decrypt_epoch_d.argtypes = [P, P, P, P, P, u32, ctypes.c_uint64, P, P, u32, u32, P, P, P, P, P]
    lib.hbx_prepare_nonces.argtypes = [P, u8p, u64p, u32, u8p]
    lib.hbx_sign.argtypes = [P, u8p, u32, u8p]
    lib.hbx_verify_sig_shares.argtypes = [P, u8p, u8p, u32, u32, u8p]
    lib.hbx_combine_signatures.argtypes = [P, u8p, u32, u8p, i32p, u8p, u8p]
    lib.hbx_verify_sig_shares_d.argtypes = [P, P, P, u32, u32, P, P]
    lib.hbx_combine_signatures_d.argtypes = [P, u8p, u32, P, P, P, P, P, P]
    lib.hbx_get_coin_lanes_used.argtypes = [P]
    lib.hbx_verify_sigs.argtypes = [P, u8p, u8p, u64p, u8p, u32, u8p]
    lib.hbx_bivar_rows.argtypes = [P, u8p, u32, u32, ctypes.c_uint64, u8p, u8p]
    lib.hbx_bivar_check_acks.argtypes = [P, u8p, u32, u32, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32), u64p,
                                         u8p, u32, u8p]
    lib.hbx_rs_encode_d.argtypes = [P, P, u32, u32, u32, u32, P]
    lib.hbx_rs_reconstruct_d.argtypes = [P, P, P, u32, u32, u32, u32, P, P]
    lib.hbx_merkle_roots_d.argtypes = [P, P, u32, u32, u32, P, P]
    lib.hbx_merkle_validate_d.argtypes = [P, P, u32, P, P, P, P, P, P, u32, u32, P, P]
    lib.hbx_broadcast_decode_d.argtypes = [P, P, P, P, u32, u32, u32, u32, P, ctypes.c_uint64, P, P, P]
    lib.hbx_broadcast_decode_leaves_d.argtypes = [P, P, P, P, P, u32, u32, u32, u32, P, ctypes.c_uint64, P, P, P]
    lib.hbx_public_keys.argtypes = [P, u8p, u32, u8p]
    lib.hbx_encrypt.argtypes = [P, u8p, u8p, u64p, u32, u8p, u8p, u8p, u8p]
    lib.hbx_decrypt_shares.argtypes = [P, u8p, u32, u8p, u32, u8p]
    # SyncKeyGen end to end
    lib.hbx_encrypt_to.argtypes = [P, u8p, u8p, u64p, u32, u8p, u8p, u8p, u8p]
    lib.hbx_sk_decrypt.argtypes = [P, u8p, u8p, u8p, u64p, u8p, u32, u8p, u8p]
    lib.hbx_bivar_poly_rows.argtypes = [P, u8p, u32, u32, u8p]
    lib.hbx_fr_poly_eval.argtypes = [P, u8p, u32, u32, u32, u8p]
    lib.hbx_keygen_generate.argtypes = [P, u8p, u32, u32, u8p, ctypes.POINTER(ctypes.c_uint32), u64p, u8p, u8p, u8p,
                                        u8p]
    lib.hbx_pk_shares_from_commit.argtypes = [P, u8p, u32, u32, u8p]
    lib.hbx_set_timing.argtypes = [P, ctypes.c_int]
    lib.hbx_kernel_time.argtypes = [P, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_uint32)]
    lib.hbx_set_digest.argtypes = [P, ctypes.c_int]
    lib.hbx_set_merkle_digest.argtypes = [P, ctypes.c_int]
    lib.hbx_set_verify_lanes.argtypes = [P, ctypes.c_int]
    lib.hbx_get_verify_lanes_used.argtypes = [P]
    lib.hbx_set_combine_lanes.argtypes = [P, ctypes.c_int]
    lib.hbx_debug_force_fallback.argtypes = [P, u32]
    lib.hbx_debug_force_degenerate.argtypes = [P, u32]
    lib.hbx_get_fallback_lanes.argtypes = [P]
    lib.hbx_get_fallback_lanes.restype = ctypes.c_int64
    lib.hbx_debug_set_combine_margin.argtypes = [P, ctypes.c_int32]
    lib.hbx_get_combine_slow_terms.argtypes = [P]
    lib.hbx_get_combine_slow_terms.restype = ctypes.c_int64
    lib.hbx_merkle_node_count.argtypes = [u32]
    lib.hbx_merkle_node_count.restype = u32
    lib.hbx_merkle_build_d.argtypes = [P, P, u32, u32, u32, P, P, P]
    lib.hbx_merkle_proofs_d.argtypes = [P, P, u32, P, u32, P, P, P, P, P, P]
    # host-pointer Broadcast calls (numpy buffers; what a Rust FFI calls from Vec<u8>)
    lib.hbx_rs_encode.argtypes = [P, P, u32, u32, u32, u32]
    lib.hbx_rs_reconstruct.argtypes = [P, P, P, u32, u32, u32, u32, P]
    lib.hbx_merkle_roots.argtypes = [P, P, u32, u32, u32, P]
    lib.hbx_merkle_build.argtypes = [P, P, u32, u32, u32, P, P]
    lib.hbx_merkle_proofs.argtypes = [P, P, u32, u32, P, u32, P, P, P, P, P]
    lib.hbx_merkle_validate.argtypes = [P, P, u32, P, P, P, P, P, P, u32, u32, P]
    lib.hbx_broadcast_decode.argtypes = [P, P, P, P, u32, u32, u32, u32, P, ctypes.c_uint64, P, P]
    lib.hbx_broadcast_decode_leaves.argtypes = [P, P, P, P, P, u32, u32, u32, u32, P, ctypes.c_uint64, P, P]
    for name in ("hbx_get_share_status", "hbx_get_ct_status", "hbx_get_sig_share_status", "hbx_get_ct_hashes"):
        getattr(lib, name).argtypes = [P, u8p, ctypes.c_size_t]
    # batched share verification: absent from a library built before it (tools/bench_batch_verify.py
    # --lib times such a build in per-share mode)
    if hasattr(lib, "hbx_set_batch_verify"):
        lib.hbx_set_batch_verify.argtypes = [P, u8p]
        u32p = ctypes.POINTER(ctypes.c_uint32)
        lib.hbx_get_batch_stats.argtypes = [P, u32p, u32p, u32p]
        lib.hbx_get_batch_sums.argtypes = [P, u8p, ctypes.c_size_t]
    # ragged Broadcast calls (per-instance shard lengths): absent from a library built before them
    # (tools/bench_broadcast_ragged.py --lib times such a build through the uniform calls)
    if hasattr(lib, "hbx_rs_encode_ragged_d"):
        u64 = ctypes.c_uint64
        lib.hbx_rs_encode_ragged_d.argtypes = [P, P, u64, P, P, P, u32, u32, u32, P]
        lib.hbx_rs_reconstruct_ragged_d.argtypes = [P, P, u64, P, P, P, P, u32, u32, u32, P, P]
        lib.hbx_merkle_build_ragged_d.argtypes = [P, P, u64, P, P, P, u32, u32, P, P, P]
        lib.hbx_merkle_validate_ragged_d.argtypes = [P, P, u64, P, P, P, P, P, P, P, u32, u32, P, P]
        lib.hbx_broadcast_decode_ragged_d.argtypes = [P, P, u64, P, P, P, P, P, P, u32, u32, u32, P, u64, P, P, P, P]
    # pair-lane Ciphertext::verify of hbx_sk_decrypt: absent from a library built before it
    if hasattr(lib, "hbx_set_ct_check"):
        lib.hbx_set_ct_check.argtypes = [P, ctypes.c_int]
        lib.hbx_get_ct_check_used.argtypes = [P]
    # PublicKey::verify over a key table and SecretKey::sign: absent from a library built before them
    # (tools/bench_keygen.py --lib times such a build through hbx_verify_sigs)
    if hasattr(lib, "hbx_verify_sigs_keyed"):
        lib.hbx_verify_sigs_keyed.argtypes = [P, u8p, u32, ctypes.POINTER(ctypes.c_uint32), u8p, u64p, u8p, u32, u8p,
                                              i32p]
        lib.hbx_sign_msgs.argtypes = [P, u8p, u8p, u64p, u32, u8p]
    # incremental share verification: absent from a library built before it (tools/bench_incremental.py
    # --lib times such a build through the masked matrix call)
    if hasattr(lib, "hbx_add_dec_shares_d"):
        u32p = ctypes.POINTER(ctypes.c_uint32)
        lib.hbx_add_dec_shares_d.argtypes = [P, P, u32p, u32p, u32, u32, P, P]
        lib.hbx_add_dec_shares.argtypes = [P, u8p, u32p, u32p, u32, u32, u8p]
        lib.hbx_combine_decrypt_cols_d.argtypes = [P, u32, u32p, u32, P, P, P]
        lib.hbx_combine_decrypt_cols.argtypes = [P, u32, u32p, u32, u8p, i32p]
        lib.hbx_get_verify_tiles_used.argtypes = [P]
        lib.hbx_get_verify_tiles_used.restype = u32
    # the coin's incremental calls: absent from a library built before them (tools/bench_coin_incremental.py
    # --lib times such a build through the masked matrix call)
    if hasattr(lib, "hbx_add_sig_shares_d"):
        u32p = ctypes.POINTER(ctypes.c_uint32)
        lib.hbx_add_sig_shares_d.argtypes = [P, P, u32p, u32p, u32, u32, P, P]
        lib.hbx_add_sig_shares.argtypes = [P, u8p, u32p, u32p, u32, u32, u8p]
        lib.hbx_combine_signatures_insts_d.argtypes = [P, u8p, u32, u32p, u32, P, P, P, P, P, P]
        lib.hbx_combine_signatures_insts.argtypes = [P, u8p, u32, u32p, u32, u8p, u8p, i32p, u8p, u8p]
        lib.hbx_get_coin_tiles_used.argtypes = [P]
        lib.hbx_get_coin_tiles_used.restype = u32
    # Broadcast message by message (the echo store): absent from a library built before it
    if hasattr(lib, "hbx_prepare_broadcast"):
        u64 = ctypes.c_uint64
        lib.hbx_prepare_broadcast.argtypes = [P, u32, u32, u32, u32]
        lib.hbx_add_echoes_d.argtypes = [P, P, u64, P, P, P, P, P, P, P, P, u32, P, P]
        lib.hbx_add_echoes.argtypes = [P, P, u64, P, P, P, P, P, P, P, P, u32, P]
        lib.hbx_broadcast_decode_insts_d.argtypes = [P, P, P, P, P, u32, P, u64, P, P, P, P]
        lib.hbx_broadcast_decode_insts.argtypes = [P, P, P, P, P, u32, P, u64, P, P, P]
        lib.hbx_get_echo_slots.argtypes = [P, P, P, P]
        lib.hbx_debug_get_echo_rows.argtypes = [P, P, u64]
    # the live-allocation count: absent from a library built before it
    if hasattr(lib, "hbx_debug_live_buffers"):
        lib.hbx_debug_live_buffers.argtypes = []
        lib.hbx_debug_live_buffers.restype = ctypes.c_uint64
    _lib = lib
    return lib


def live_buffers() -> int:
    """hbx_debug_live_buffers: device and pinned allocations the library holds in this process."""
    return int(load_library().hbx_debug_live_buffers())


def build_info() -> dict:
    """Provenance of the loaded library: the source hash it was built from (hbx_build_id), the hash
    of the sources in this tree (hbbft_amd/buildinfo.py) and whether they match."""
    from . import buildinfo

    lib = load_library()
    built = lib.hbx_build_id().decode()
    tree = buildinfo.source_hash()
    return {"lib_source_sha256": built, "tree_source_sha256": tree, "match": built == tree,
            "lib": os.path.relpath(LIB_PATH, buildinfo.ROOT)}


def _u8(a: np.ndarray):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


def ragged_layout(lens, n: int, align: int = 16):
    """A ragged Broadcast buffer for shard lengths ``lens`` with ``n`` rows per instance, instances
    back to back: -> (off uint64[inst], pitch uint32[inst], total_bytes).  pitch = len rounded up to
    ``align`` (a multiple of 4), so every row -- and every instance -- starts ``align``-aligned."""
    if align <= 0 or align % 4:
        raise ValueError(f"ragged_layout: align {align} must be a positive multiple of 4")
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    if n < 1 or lens.size == 0 or (lens < 1).any() or (lens > 0xFFFFFFFF - align).any():
        raise ValueError("ragged_layout: need n >= 1 and shard lengths in [1, 2^32 - align)")
    pitch = (lens + align - 1) // align * align
    size = pitch * n
    off = np.concatenate(([0], np.cumsum(size)[:-1]))
    return off.astype(np.uint64), pitch.astype(np.uint32), int(size.sum())


def pack_bits(bools) -> np.ndarray:
    a = np.asarray(bools, dtype=np.uint8).reshape(-1)
    return np.packbits(a, bitorder="little")


def unpack_bits(bits: np.ndarray, n: int) -> np.ndarray:
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), bitorder="little")[:n].astype(bool)


def layers(keys) -> list:
    """An add (and a matrix verification) takes each (row, sender) position once per call, so a run
    of messages goes in as layers: layer L = the indices into ``keys``, in order, whose key occurs
    there for the L-th time (L = 0, 1, ...) -> list of index lists."""
    out, seen = [], {}
    for i, key in enumerate(keys):
        L = seen.get(key, 0)
        seen[key] = L + 1
        if L == len(out):
            out.append([])
        out[L].append(i)
    return out


class Context:
    """One hbx context bound to a HIP device (``hbx_ctx_create``)."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = ctypes.c_void_p()
        rc = self.lib.hbx_ctx_create(device, ctypes.byref(h))
        if rc != HBX_OK:
            raise HbxError(rc, f"hbx_ctx_create(device={device}) failed: no usable HIP device?")
        self.h = h
        self.device = device
        self._v_off = None  # offsets of the prepared ciphertexts' V blob (host) ...
        self._d_off = None  # ... or the caller's device tensor of them (device API)

    def close(self):
        if getattr(self, "h", None):
            self.lib.hbx_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc != HBX_OK:
            raise HbxError(rc, self.lib.hbx_last_error(self.h).decode())

    def set_digest(self, variant: int):
        """hbx_set_digest: DIGEST_SHA256 (default) or DIGEST_SHA3_256 for hash_g2 / hash_g1_g2 / hash_bytes."""
        self._check(self.lib.hbx_set_digest(self.h, variant))

    def set_verify_lanes(self, lanes: int):
        """hbx_set_verify_lanes: 0 auto (default), 1, 2, 3, 6 or 7 (one lane, single kernel) per check."""
        self._check(self.lib.hbx_set_verify_lanes(self.h, lanes))

    def verify_lanes_used(self) -> int:
        """hbx_get_verify_lanes_used: lanes per check of the last decryption-share launch."""
        return int(self.lib.hbx_get_verify_lanes_used(self.h))

    def debug_force_fallback(self, every: int):
        """hbx_debug_force_fallback (tests only): route every ``every``-th sender's one-lane check
        through the single-kernel fallback (0 = off)."""
        self._check(self.lib.hbx_debug_force_fallback(self.h, every))

    def debug_force_degenerate(self, every: int):
        """hbx_debug_force_degenerate (tests only): treat every ``every``-th proposer's lines as having
        no constant-term-1 form, so its one-lane checks go through the single-kernel fallback (0 = off)."""
        self._check(self.lib.hbx_debug_force_degenerate(self.h, every))

    def fallback_lanes(self) -> int:
        """hbx_get_fallback_lanes: checks of the last launch with a fallback path (one-lane decryption
        shares, two-lane coin, pair-lane ciphertexts of ``sk_decrypt``, pair-lane signatures of
        ``verify_sigs_keyed``) that the fallback decided."""
        v = int(self.lib.hbx_get_fallback_lanes(self.h))
        if v < 0:
            self._check(v)
        return v

    def set_ct_check(self, mode: int):
        """hbx_set_ct_check: how ``sk_decrypt`` runs Ciphertext::verify -- CT_CHECK_WIDE (default, the
        wide executor over prepared line tables) or CT_CHECK_PAIR (one lane pair per ciphertext, no
        tables).  Same statuses and plaintexts; the epoch's prepares are not affected."""
        if isinstance(mode, bool) or mode not in (CT_CHECK_WIDE, CT_CHECK_PAIR):
            raise ValueError(f"set_ct_check: CT_CHECK_WIDE (0) or CT_CHECK_PAIR (1), not {mode!r}")
        self._check(self.lib.hbx_set_ct_check(self.h, int(mode)))

    def ct_check_used(self) -> int:
        """hbx_get_ct_check_used: the mode the last ``sk_decrypt`` ran (-1 before any call)."""
        return int(self.lib.hbx_get_ct_check_used(self.h))

    def set_batch_verify(self, seed: Optional[bytes]):
        """hbx_set_batch_verify: decide each proposer's column of shares by one random-linear-combination
        equation keyed by the 32-byte ``seed`` (which no sender may be able to predict); None = per-share
        checks (default)."""
        if seed is None:
            self._check(self.lib.hbx_set_batch_verify(self.h, None))
            return
        if len(seed) != 32:
            raise ValueError("batch seed must be 32 bytes")
        buf = np.frombuffer(bytes(seed), dtype=np.uint8).copy()
        self._check(self.lib.hbx_set_batch_verify(self.h, _u8(buf)))

    def batch_stats(self):
        """hbx_get_batch_stats: (cols_batched, cols_fallback, cols_skipped) of the last share verification."""
        v = [ctypes.c_uint32() for _ in range(3)]
        self._check(self.lib.hbx_get_batch_stats(self.h, *[ctypes.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def batch_sums(self, p: int) -> np.ndarray:
        """hbx_get_batch_sums (test hook): compressed A_j of the last batched verification -> uint8[p, 48]."""
        out = np.zeros(p * 48, dtype=np.uint8)
        self._check(self.lib.hbx_get_batch_sums(self.h, _u8(out), p))
        return out.reshape(p, 48)

    def set_combine_lanes(self, lanes: int):
        """hbx_set_combine_lanes: 0 auto (default), 1 (a lane per Lagrange term) or 4 (a quad per term)."""
        self._check(self.lib.hbx_set_combine_lanes(self.h, lanes))

    def debug_set_combine_margin(self, margin: int):
        """hbx_debug_set_combine_margin (tests only): the fused epoch call precomputes the combine's
        window tables for senders below ``t + margin``; ``COMBINE_MARGIN_AUTO`` (default) or
        ``COMBINE_TABLES_OFF``."""
        self._check(self.lib.hbx_debug_set_combine_margin(self.h, margin))

    def combine_slow_terms(self) -> int:
        """hbx_get_combine_slow_terms: GLV half-terms of the last combine that had no tables."""
        v = int(self.lib.hbx_get_combine_slow_terms(self.h))
        if v < 0:
            self._check(v)
        return v

    def set_merkle_digest(self, variant: int):
        """hbx_set_merkle_digest: MERKLE_SHA256 (default, afck merkle) or MERKLE_SHA3."""
        self._check(self.lib.hbx_set_merkle_digest(self.h, variant))

    # -- instrumentation -----------------------------------------------------------------------
    def set_timing(self, on: bool = True):
        """Bracket every launch of the timed kernels with HIP events on their stream."""
        self._check(self.lib.hbx_set_timing(self.h, 1 if on else 0))

    def kernel_time(self, name: str):
        """(total_ms, launches) of a timed kernel since the last set_timing call."""
        ms = ctypes.c_double()
        cnt = ctypes.c_uint32()
        self._check(self.lib.hbx_kernel_time(self.h, KERNELS[name], ctypes.byref(ms), ctypes.byref(cnt)))
        return ms.value, cnt.value

    # -- host API ------------------------------------------------------------------------------
    def set_pk_shares(self, pk_comp: Sequence[bytes]) -> np.ndarray:
        n = len(pk_comp)
        buf = np.frombuffer(b"".join(pk_comp), dtype=np.uint8).copy()
        st = np.zeros(n, dtype=np.int32)
        self._check(self.lib.hbx_set_pk_shares(self.h, _u8(buf), n, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return st

    def prepare_ciphertexts(self, cts) -> np.ndarray:
        """cts: list of (u_comp48, v_bytes, w_comp96).  Returns bool[p] = Ciphertext::verify."""
        p = len(cts)
        u = np.frombuffer(b"".join(c[0] for c in cts), dtype=np.uint8).copy()
        w = np.frombuffer(b"".join(c[2] for c in cts), dtype=np.uint8).copy()
        off = np.zeros(p + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c[1]) for c in cts])
        vb = np.frombuffer(b"".join(c[1] for c in cts) or b"\0", dtype=np.uint8).copy()
        bits = np.zeros((p + 7) // 8, dtype=np.uint8)
        self._check(self.lib.hbx_prepare_ciphertexts(
            self.h, _u8(u), _u8(vb), off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _u8(w), p, _u8(bits)))
        self._v_off = off
        return unpack_bits(bits, p)

    def verify_dec_shares(self, shares: np.ndarray, present: Optional[np.ndarray] = None) -> np.ndarray:
        """shares: uint8[p, n, 48].  Returns bool[p, n]."""
        shares = np.ascontiguousarray(shares, dtype=np.uint8)
        p, n, _ = shares.shape
        pres = None if present is None else pack_bits(np.asarray(present, dtype=bool).reshape(-1))
        bits = np.zeros((p * n + 7) // 8, dtype=np.uint8)
        self._check(self.lib.hbx_verify_dec_shares(
            self.h, _u8(shares), None if pres is None else _u8(pres), n, p, _u8(bits)))
        return unpack_bits(bits, p * n).reshape(p, n)

    def combine_decrypt(self, t: int):
        """Returns (list of plaintext bytes or None, status int32[p])."""
        off = self._v_off
        if off is None:  # prepared through the device API: the caller's offsets tensor
            off = self._d_off.detach().cpu().numpy().astype(np.uint64)
        p = len(off) - 1
        out = np.zeros(max(int(off[-1]), 1), dtype=np.uint8)
        st = np.zeros(p, dtype=np.int32)
        self._check(self.lib.hbx_combine_decrypt(self.h, t, _u8(out), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        res = []
        for j in range(p):
            res.append(out[int(off[j]):int(off[j + 1])].tobytes() if st[j] == HBX_OK else None)
        return res, st

    # -- the incremental adds (hbx_add_dec_shares[_d], hbx_add_sig_shares[_d]) and the listed combines --
    @staticmethod
    def _index_pair(what: str, names, a, b, count: int):
        """The two index arrays of an add's items (named `names`) as contiguous uint32[count]."""
        out = []
        for name, x in zip(names, (a, b)):
            x = np.asarray(x)
            if x.ndim != 1 or x.shape[0] != count:
                raise ValueError(f"{what}: {name} must have one entry per share ({count}), not shape {x.shape}")
            if x.size and (x.dtype.kind not in "iu" or int(x.min()) < 0 or int(x.max()) > 0xFFFFFFFF):
                raise ValueError(f"{what}: {name} must hold indices (uint32)")
            out.append(np.ascontiguousarray(x, dtype=np.uint32))
        return out

    @staticmethod
    def _index_list(what: str, name: str, of: str, one: str, x):
        """A list of indices, each listed once, as contiguous uint32 (`name` a list of `of`, `one` of
        them); the library checks the bound."""
        x = np.asarray(x)
        if x.ndim != 1 or (x.size and (x.dtype.kind not in "iu" or int(x.min()) < 0 or int(x.max()) > 0xFFFFFFFF)):
            raise ValueError(f"{what}: {name} must be a list of {of}")
        if len(set(x.tolist())) != x.size:
            raise ValueError(f"{what}: {one} is listed twice")
        return np.ascontiguousarray(x, dtype=np.uint32)

    @staticmethod
    def _nodes(what: str, n):
        if not isinstance(n, (int, np.integer)) or n <= 0:
            raise ValueError(f"{what}: n must be the number of nodes")

    def _add_host(self, fn: str, width: int, names, pts, a, b, n) -> np.ndarray:
        """The host form `fn` of an add: pts uint8[count, width] and the index arrays a, b (the three
        named `names`) -> HBX_SHARE_* uint8[count]."""
        what = fn[4:]
        pts = np.asarray(pts)
        if pts.dtype != np.uint8 or pts.ndim != 2 or pts.shape[1] != width:
            raise ValueError(f"{what}: {names[0]} must be uint8[count, {width}], not {pts.dtype}{pts.shape}")
        pts = np.ascontiguousarray(pts)
        count = pts.shape[0]
        a, b = self._index_pair(what, names[1:], a, b, count)
        self._nodes(what, n)
        out = np.zeros(count, dtype=np.uint8)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(getattr(self.lib, fn)(
            self.h, _u8(pts) if count else None, a.ctypes.data_as(u32p) if count else None,
            b.ctypes.data_as(u32p) if count else None, count, int(n), _u8(out) if count else None))
        return out

    def _add_device(self, fn: str, width: int, names, d_pts, a, b, n, d_status, stream):
        """The device form `fn` of an add: d_pts a contiguous device uint8[count, width] tensor (None
        with no items), a / b host index arrays, d_status an optional device uint8[count].  The
        library reads d_pts by raw pointer, so its element size and strides are checked here."""
        what = fn[4:]
        count = 0 if d_pts is None else int(d_pts.shape[0])
        if d_pts is not None and (d_pts.dim() != 2 or d_pts.shape[1] != width or d_pts.element_size() != 1
                                  or not d_pts.is_contiguous()):
            raise ValueError(f"{what}: {names[0]} must be contiguous uint8[count, {width}], not shape {tuple(d_pts.shape)}")
        a, b = self._index_pair(what, names[1:], a, b, count)
        if d_status is not None and (d_status.numel() != count or d_status.element_size() != 1):
            raise ValueError(f"{what}: d_status must have one byte per share ({count})")
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(getattr(self.lib, fn)(
            self.h, d_pts.data_ptr() if count else None, a.ctypes.data_as(u32p) if count else None,
            b.ctypes.data_as(u32p) if count else None, count, int(n),
            None if d_status is None or not count else d_status.data_ptr(), self._stream(stream)))

    def add_dec_shares(self, shares48, proposer, sender, n: int) -> np.ndarray:
        """hbx_add_dec_shares: the shares that arrived since the last call, verified and merged into
        the epoch's matrix.  shares48 uint8[count, 48] (or what converts to it), proposer (column
        j < p) and sender (node index) one entry each -> HBX_SHARE_* uint8[count]."""
        return self._add_host("hbx_add_dec_shares", 48, ("shares48", "proposer", "sender"),
                              np.asarray(shares48, dtype=np.uint8), proposer, sender, n)

    def combine_decrypt_cols(self, t: int, cols, out=None, status=None):
        """hbx_combine_decrypt_cols: threshold decryption of the listed proposer columns only ->
        ({column: plaintext bytes or None}, {column: status}).  `out` (uint8[sum |V_j|]) and `status`
        (int32[p]), if given, are the caller's buffers: only the listed proposers' ranges and entries
        of them are written."""
        cols = self._index_list("combine_decrypt_cols", "cols", "proposer columns", "a column", cols)
        off = self._v_off
        if off is None:  # prepared through the device API: the caller's offsets tensor
            off = self._d_off.detach().cpu().numpy().astype(np.uint64)
        p = len(off) - 1
        if cols.size and int(cols.max()) >= p:
            raise ValueError(f"combine_decrypt_cols: column {int(cols.max())} of {p} prepared ciphertexts")
        out = np.zeros(max(int(off[-1]), 1), dtype=np.uint8) if out is None else out
        st = np.zeros(p, dtype=np.int32) if status is None else status
        if out.dtype != np.uint8 or out.size < max(int(off[-1]), 1) or not out.flags.c_contiguous or \
                st.dtype != np.int32 or st.shape != (p,) or not st.flags.c_contiguous:
            raise ValueError(f"combine_decrypt_cols: out must be uint8[>= {int(off[-1])}] and status int32[{p}]")
        if cols.size:
            self._check(self.lib.hbx_combine_decrypt_cols(
                self.h, t, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), cols.size, _u8(out),
                st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        plains = {int(j): (out[int(off[j]):int(off[j + 1])].tobytes() if st[j] == HBX_OK else None) for j in cols}
        return plains, {int(j): int(st[j]) for j in cols}

    def verify_tiles_used(self) -> int:
        """Check blocks of the last share-check launch (hbx_get_verify_tiles_used)."""
        return int(self.lib.hbx_get_verify_tiles_used(self.h))

    def share_status(self, p: int, n: int) -> np.ndarray:
        """HBX_SHARE_* byte of every share of the last verification -> uint8[p, n]."""
        out = np.zeros(p * n, dtype=np.uint8)
        self._check(self.lib.hbx_get_share_status(self.h, _u8(out), out.size))
        return out.reshape(p, n)

    def ct_status(self, p: int) -> np.ndarray:
        """HBX_CT_* byte of every prepared ciphertext -> uint8[p]."""
        out = np.zeros(p, dtype=np.uint8)
        self._check(self.lib.hbx_get_ct_status(self.h, _u8(out), out.size))
        return out

    def ct_hashes(self, p: int) -> np.ndarray:
        """Compressed H_j = hash_g1_g2(U_j, V_j) of the prepared ciphertexts -> uint8[p, 96]."""
        out = np.zeros(p * 96, dtype=np.uint8)
        self._check(self.lib.hbx_get_ct_hashes(self.h, _u8(out), p))
        return out.reshape(p, 96)

    def sig_share_status(self, count: int, n: int) -> np.ndarray:
        """HBX_SHARE_* byte of every signature share of the last hbx_verify_sig_shares."""
        out = np.zeros(count * n, dtype=np.uint8)
        self._check(self.lib.hbx_get_sig_share_status(self.h, _u8(out), out.size))
        return out.reshape(count, n)

    # -- producer side -------------------------------------------------------
    def public_keys(self, sk32: np.ndarray) -> np.ndarray:
        """sk32: uint8[n, 32] big-endian canonical scalars -> uint8[n, 48] compressed g1 * sk."""
        sk32 = np.ascontiguousarray(sk32, dtype=np.uint8)
        n = sk32.shape[0]
        out = np.zeros((n, 48), dtype=np.uint8)
        self._check(self.lib.hbx_public_keys(self.h, _u8(sk32), n, _u8(out)))
        return out

    def encrypt(self, pk48: bytes, msgs: Sequence[bytes], r32: np.ndarray):
        """PublicKey::encrypt for each message with randomness r32[j] -> list of (u48, v, w96)."""
        p = len(msgs)
        off = np.zeros(p + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        mb = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
        vb = np.zeros_like(mb)
        u = np.zeros((p, 48), dtype=np.uint8)
        w = np.zeros((p, 96), dtype=np.uint8)
        pk = np.frombuffer(bytes(pk48), dtype=np.uint8).copy()
        r32 = np.ascontiguousarray(r32, dtype=np.uint8)
        self._check(self.lib.hbx_encrypt(self.h, _u8(pk), _u8(mb), off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                         p, _u8(r32), _u8(u), _u8(vb), _u8(w)))
        return [(u[j].tobytes(), vb[int(off[j]):int(off[j + 1])].tobytes(), w[j].tobytes()) for j in range(p)]

    def decrypt_shares(self, sk32: np.ndarray, u48: np.ndarray) -> np.ndarray:
        """shares[j, i] = sk_i * U_j compressed -> uint8[p, n, 48]."""
        sk32 = np.ascontiguousarray(sk32, dtype=np.uint8)
        u48 = np.ascontiguousarray(u48, dtype=np.uint8)
        n, p = sk32.shape[0], u48.shape[0]
        out = np.zeros((p, n, 48), dtype=np.uint8)
        self._check(self.lib.hbx_decrypt_shares(self.h, _u8(sk32), n, _u8(u48), p, _u8(out)))
        return out

    def set_own_share(self, me: int, sk32=None):
        """hbx_set_own_share: this node's index and 32-byte big-endian secret share (None clears)."""
        if sk32 is None:
            self._check(self.lib.hbx_set_own_share(self.h, 0, None))
            return
        sk = np.frombuffer(bytes(sk32), dtype=np.uint8).copy()
        assert sk.size == 32
        self._check(self.lib.hbx_set_own_share(self.h, me, _u8(sk)))

    # -- device API (torch tensors as HBM buffers; torch is plumbing only) -----------------------
    # stream=None enqueues on torch's current stream of the context's device (the C ABI's NULL is
    # the HIP null stream, which is what torch's default stream is), so the calls are ordered
    # with the tensor uploads and reads the caller did on that stream.
    def _stream(self, stream):
        if stream is not None:
            return stream
        import torch

        return torch.cuda.current_stream(self.device).cuda_stream

    def prepare_ciphertexts_d(self, d_u, d_v, d_off, d_w, p: int, max_v_len: int, d_ct_valid=None, stream=None):
        # the host combine_decrypt sizes its output from these offsets (read back when needed)
        self._v_off, self._d_off = None, d_off
        self._check(self.lib.hbx_prepare_ciphertexts_d(
            self.h, d_u.data_ptr(), d_v.data_ptr(), d_off.data_ptr(), d_w.data_ptr(), p, max_v_len,
            None if d_ct_valid is None else d_ct_valid.data_ptr(), self._stream(stream)))

    def verify_dec_shares_d(self, d_shares, n: int, p: int, d_valid=None, d_present=None, stream=None):
        self._check(self.lib.hbx_verify_dec_shares_d(
            self.h, d_shares.data_ptr(), None if d_present is None else d_present.data_ptr(), n, p,
            None if d_valid is None else d_valid.data_ptr(), self._stream(stream)))

    # -- common coin ------------------------------------------------------------------------------
    def prepare_nonces(self, nonces: Sequence[bytes], hashes: bool = True) -> Optional[np.ndarray]:
        """hash_g2 of every nonce; returns uint8[count, 96] compressed points, or None with
        ``hashes=False`` -- then the call returns after its uploads, the share checks and the
        combine do not wait for the true H (only hbx_sign does), and the hashing runs on."""
        count = len(nonces)
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in nonces])
        blob = np.frombuffer(b"".join(nonces) or b"\0", dtype=np.uint8).copy()
        h = np.zeros((count, 96), dtype=np.uint8) if hashes else None
        self._check(self.lib.hbx_prepare_nonces(self.h, _u8(blob), off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                                count, _u8(h) if hashes else None))
        self._coin_count = count
        return h

    def sign(self, sk32: np.ndarray) -> np.ndarray:
        """uint8[n, 32] scalars -> uint8[count, n, 96] signature shares of the prepared nonces."""
        sk32 = np.ascontiguousarray(sk32, dtype=np.uint8)
        n = sk32.shape[0]
        out = np.zeros((self._coin_count, n, 96), dtype=np.uint8)
        self._check(self.lib.hbx_sign(self.h, _u8(sk32), n, _u8(out)))
        return out

    def verify_sig_shares(self, sigs: np.ndarray, present: Optional[np.ndarray] = None) -> np.ndarray:
        """sigs: uint8[count, n, 96] -> bool[count, n]."""
        sigs = np.ascontiguousarray(sigs, dtype=np.uint8)
        count, n, _ = sigs.shape
        pres = None if present is None else pack_bits(np.asarray(present, dtype=bool).reshape(-1))
        bits = np.zeros((count * n + 7) // 8, dtype=np.uint8)
        self._check(self.lib.hbx_verify_sig_shares(self.h, _u8(sigs), None if pres is None else _u8(pres), n, count,
                                                   _u8(bits)))
        return unpack_bits(bits, count * n).reshape(count, n)

    def coin_lanes_used(self) -> int:
        """hbx_get_coin_lanes_used: lanes per check of the last signature-share verification."""
        return int(self.lib.hbx_get_coin_lanes_used(self.h))

    def verify_sig_shares_d(self, d_sigs, d_present=None, d_status=None, stream=None):
        """d_sigs: uint8[count, n, 96] device tensor; d_present / d_status: uint8[count, n] (or None)."""
        import torch

        count, n, w = d_sigs.shape
        if w != 96 or d_sigs.dtype != torch.uint8 or not d_sigs.is_contiguous():
            raise ValueError("verify_sig_shares_d: d_sigs must be contiguous uint8[count, n, 96]")
        for x in (d_present, d_status):
            if x is not None and (tuple(x.shape) != (count, n) or x.dtype != torch.uint8 or not x.is_contiguous()):
                raise ValueError(f"verify_sig_shares_d: present/status must be contiguous uint8[{count}, {n}]")
        opt = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self._check(self.lib.hbx_verify_sig_shares_d(self.h, d_sigs.data_ptr(), opt(d_present), n, count,
                                                     opt(d_status), self._stream(stream)))

    def combine_signatures_d(self, master_pk48: bytes, t: int, d_use=None, d_sig=None, d_status=None, d_ok=None,
                             d_parity=None, stream=None):
        """hbx_combine_signatures_d: d_use uint8[count, n] (or None: every valid share)."""
        mpk = np.frombuffer(bytes(master_pk48), dtype=np.uint8).copy()
        opt = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self._check(self.lib.hbx_combine_signatures_d(self.h, _u8(mpk), t, opt(d_use), opt(d_sig), opt(d_status),
                                                      opt(d_ok), opt(d_parity), self._stream(stream)))

    def combine_signatures(self, master_pk48: bytes, t: int):
        """-> (sig uint8[count, 96], status int32[count], master_ok bool[count], parity bool[count])."""
        count = self._coin_count
        sig = np.zeros((count, 96), dtype=np.uint8)
        st = np.zeros(count, dtype=np.int32)
        ok = np.zeros((count + 7) // 8, dtype=np.uint8)
        par = np.zeros((count + 7) // 8, dtype=np.uint8)
        mpk = np.frombuffer(bytes(master_pk48), dtype=np.uint8).copy()
        self._check(self.lib.hbx_combine_signatures(self.h, _u8(mpk), t, _u8(sig),
                                                    st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _u8(ok), _u8(par)))
        return sig, st, unpack_bits(ok, count), unpack_bits(par, count)

    # -- common coin, incremental ------------------------------------------------------------------
    def _coin_insts(self, what: str, insts):
        return self._index_list(what, "insts", "coin instances", "an instance", insts)

    def add_sig_shares(self, sig96, inst, sender, n: int) -> np.ndarray:
        """hbx_add_sig_shares: the signature shares that arrived since the last call, verified and
        merged into the round's matrix.  sig96 uint8[count, 96], inst (< prepared nonces) and sender
        (node index) one entry each -> HBX_SHARE_* uint8[count]."""
        return self._add_host("hbx_add_sig_shares", 96, ("sig96", "inst", "sender"), sig96, inst, sender, n)

    def add_sig_shares_d(self, d_sig96, inst, sender, n: int, d_status=None, stream=None):
        """hbx_add_sig_shares_d: d_sig96 a device uint8[count, 96] tensor (None with no items), inst /
        sender host index arrays, d_status an optional device uint8[count]."""
        self._nodes("add_sig_shares_d", n)
        self._add_device("hbx_add_sig_shares_d", 96, ("d_sig96", "inst", "sender"), d_sig96, inst, sender, n, d_status,
                         stream)

    def combine_signatures_insts(self, master_pk48: bytes, t: int, insts, use=None, sig=None, status=None, ok=None,
                                 parity=None):
        """hbx_combine_signatures_insts: the listed instances only -> (sig uint8[count, 96], status
        int32[count], master_ok uint8[count], parity uint8[count]); `use` uint8[count, n] or None.  The
        four outputs, if given, are the caller's arrays: only the listed instances' entries of them
        are written."""
        insts = self._coin_insts("combine_signatures_insts", insts)
        count = getattr(self, "_coin_count", 0)
        if insts.size and int(insts.max()) >= count:
            raise ValueError(f"combine_signatures_insts: instance {int(insts.max())} of {count} prepared nonces")
        if use is not None:
            use = np.asarray(use)
            if use.dtype != np.uint8 or use.ndim != 2 or use.shape[0] != count:
                raise ValueError(f"combine_signatures_insts: use must be uint8[{count}, n], not {use.dtype}{use.shape}")
            use = np.ascontiguousarray(use)
        sig = np.zeros((count, 96), dtype=np.uint8) if sig is None else sig
        status = np.zeros(count, dtype=np.int32) if status is None else status
        ok = np.zeros(count, dtype=np.uint8) if ok is None else ok
        parity = np.zeros(count, dtype=np.uint8) if parity is None else parity
        for name, a, dt, shape in (("sig", sig, np.uint8, (count, 96)), ("status", status, np.int32, (count,)),
                                   ("ok", ok, np.uint8, (count,)), ("parity", parity, np.uint8, (count,))):
            if not isinstance(a, np.ndarray) or a.dtype != dt or a.shape != shape or not a.flags.c_contiguous:
                raise ValueError(f"combine_signatures_insts: {name} must be contiguous {np.dtype(dt).name}{list(shape)}")
        mpk = np.frombuffer(bytes(master_pk48), dtype=np.uint8).copy()
        if insts.size:
            self._check(self.lib.hbx_combine_signatures_insts(
                self.h, _u8(mpk), t, insts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), insts.size,
                None if use is None else _u8(use), _u8(sig), status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                _u8(ok), _u8(parity)))
        return sig, status, ok, parity

    def combine_signatures_insts_d(self, master_pk48: bytes, t: int, insts, d_use=None, d_sig=None, d_status=None,
                                   d_ok=None, d_parity=None, stream=None):
        """hbx_combine_signatures_insts_d: insts a host list of coin instances; d_use / outputs as for
        combine_signatures_d (only the listed instances' entries are written)."""
        insts = self._coin_insts("combine_signatures_insts_d", insts)
        import torch

        for name, x, dt in (("d_use", d_use, torch.uint8), ("d_sig", d_sig, torch.uint8), ("d_status", d_status, torch.int32),
                            ("d_ok", d_ok, torch.uint8), ("d_parity", d_parity, torch.uint8)):
            if x is not None and (x.dtype != dt or not x.is_contiguous()):
                raise ValueError(f"combine_signatures_insts_d: {name} must be a contiguous {dt} tensor")
        mpk = np.frombuffer(bytes(master_pk48), dtype=np.uint8).copy()
        opt = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self._check(self.lib.hbx_combine_signatures_insts_d(
            self.h, _u8(mpk), t, insts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if insts.size else None, insts.size,
            opt(d_use), opt(d_sig), opt(d_status), opt(d_ok), opt(d_parity), self._stream(stream)))

    def coin_tiles_used(self) -> int:
        """Check blocks of the last signature-share check launch (hbx_get_coin_tiles_used)."""
        return int(self.lib.hbx_get_coin_tiles_used(self.h))

    def verify_sigs(self, pk48: np.ndarray, msgs, sig96: np.ndarray) -> np.ndarray:
        """PublicKey::verify(sig_i, msg_i) for independent items (DHB votes, key-generation
        messages): pk48 uint8[count, 48], msgs = list of bytes, sig96 uint8[count, 96] ->
        HBX_SHARE_* status uint8[count] (VALID / INVALID / UNDECODABLE)."""
        pk48 = np.ascontiguousarray(pk48, dtype=np.uint8)
        sig96 = np.ascontiguousarray(sig96, dtype=np.uint8)
        count = pk48.shape[0]
        if len(msgs) != count or sig96.shape[0] != count:
            raise ValueError("verify_sigs: pk48, msgs and sig96 must have the same count")
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        blob = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
        out = np.zeros(count, dtype=np.uint8)
        self._check(self.lib.hbx_verify_sigs(self.h, _u8(pk48), _u8(blob),
                                             off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _u8(sig96), count,
                                             _u8(out)))
        return out

    @staticmethod
    def _msg_blob(msgs):
        off = np.zeros(len(msgs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        return np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy(), off

    def verify_sigs_keyed(self, pk48: np.ndarray, key_idx: np.ndarray, msgs, sig96: np.ndarray):
        """PublicKey::verify(sig_i, msg_i) under pk48[key_idx[i]] (hbx_verify_sigs_keyed): the signed
        key-generation messages of an era, or a batch of votes.  pk48 uint8[nkeys, 48], key_idx
        uint32[count] (NO_KEY, or any index >= nkeys: SHARE_UNKNOWN_SENDER), msgs = list of bytes,
        sig96 uint8[count, 96] -> (HBX_SHARE_* uint8[count], HBX_PT_* int32[nkeys])."""
        pk48 = np.ascontiguousarray(pk48, dtype=np.uint8)
        sig96 = np.ascontiguousarray(sig96, dtype=np.uint8)
        count = len(msgs)
        if pk48.ndim != 2 or pk48.shape[1] != 48 or pk48.shape[0] == 0:
            raise ValueError("verify_sigs_keyed: pk48 must be uint8[nkeys, 48] with nkeys > 0")
        if not isinstance(key_idx, np.ndarray) or key_idx.dtype != np.uint32 or key_idx.shape != (count,):
            raise ValueError(f"verify_sigs_keyed: key_idx must be a uint32[{count}] array")
        if count == 0 or sig96.shape != (count, 96):
            raise ValueError("verify_sigs_keyed: key_idx, msgs and sig96 must have the same non-zero count")
        key_idx = np.ascontiguousarray(key_idx)
        nkeys = pk48.shape[0]
        blob, off = self._msg_blob(msgs)
        out = np.zeros(count, dtype=np.uint8)
        kst = np.zeros(nkeys, dtype=np.int32)
        self._check(self.lib.hbx_verify_sigs_keyed(self.h, _u8(pk48), nkeys,
                                                   key_idx.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), _u8(blob),
                                                   off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _u8(sig96), count,
                                                   _u8(out), kst.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))))
        return out, kst

    def sign_msgs(self, sk32: bytes, msgs) -> np.ndarray:
        """SecretKey::sign of every message under sk32 (32 bytes, big-endian, in [1, r)) ->
        uint8[count, 96] (hbx_sign_msgs).  Leaves the coin's prepared nonces alone."""
        sk = np.frombuffer(bytes(sk32), dtype=np.uint8).copy()
        count = len(msgs)
        if sk.size != 32:
            raise ValueError("sign_msgs: sk32 must be 32 bytes")
        if count == 0:
            raise ValueError("sign_msgs: no messages")
        blob, off = self._msg_blob(msgs)
        out = np.zeros((count, 96), dtype=np.uint8)
        self._check(self.lib.hbx_sign_msgs(self.h, _u8(sk), _u8(blob), off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                           count, _u8(out)))
        return out

    def bivar_rows(self, commits: np.ndarray, t: int, x: int):
        """BivarCommitment::row(x) of p commitments uint8[p, (t+1)(t+2)/2, 48] ->
        (rows uint8[p, t + 1, 48], status uint8[p])."""
        commits = np.ascontiguousarray(commits, dtype=np.uint8)
        p = commits.shape[0]
        rows = np.zeros((p, t + 1, 48), dtype=np.uint8)
        st = np.zeros(p, dtype=np.uint8)
        self._check(self.lib.hbx_bivar_rows(self.h, _u8(commits), p, t, x, _u8(rows), _u8(st)))
        return rows, st

    def bivar_check_acks(self, commits: np.ndarray, t: int, x: int, proposer, y, vals32: np.ndarray) -> np.ndarray:
        """handle_ack's check commit[proposer].evaluate(x, y) == g1 * val -> HBX_SHARE_* uint8[count]."""
        commits = np.ascontiguousarray(commits, dtype=np.uint8)
        pr = np.ascontiguousarray(proposer, dtype=np.uint32)
        yy = np.ascontiguousarray(y, dtype=np.uint64)
        vals32 = np.ascontiguousarray(vals32, dtype=np.uint8)
        out = np.zeros(len(pr), dtype=np.uint8)
        self._check(self.lib.hbx_bivar_check_acks(self.h, _u8(commits), commits.shape[0], t, x,
                                                  pr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                  yy.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _u8(vals32),
                                                  len(pr), _u8(out)))
        return out

    # -- SyncKeyGen end to end (src/sync_key_gen.rs) ---------------------------------------------
    def encrypt_to(self, pk48: np.ndarray, msgs: Sequence[bytes], r32: np.ndarray):
        """PublicKey::encrypt of msgs[j] to pk48[j] with randomness r32[j] -> list of (u48, v, w96)."""
        pk48 = np.ascontiguousarray(pk48, dtype=np.uint8)
        r32 = np.ascontiguousarray(r32, dtype=np.uint8)
        count = len(msgs)
        if pk48.shape != (count, 48) or r32.shape != (count, 32):
            raise ValueError("encrypt_to: pk48 must be [count, 48] and r32 [count, 32] for count messages")
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(m) for m in msgs])
        mb = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
        vb = np.zeros_like(mb)
        u = np.zeros((count, 48), dtype=np.uint8)
        w = np.zeros((count, 96), dtype=np.uint8)
        self._check(self.lib.hbx_encrypt_to(self.h, _u8(pk48), _u8(mb),
                                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), count, _u8(r32),
                                            _u8(u), _u8(vb), _u8(w)))
        return [(u[j].tobytes(), vb[int(off[j]):int(off[j + 1])].tobytes(), w[j].tobytes()) for j in range(count)]

    def sk_decrypt(self, sk32: bytes, cts):
        """SecretKey::decrypt of cts = list of (u48, v, w96) under the individual key sk32 ->
        (list of plaintext bytes, zeros where the status is not CT_VALID; HBX_CT_* uint8[count]).
        Voids the prepared epoch ciphertexts."""
        count = len(cts)
        sk = np.frombuffer(bytes(sk32), dtype=np.uint8).copy()
        if sk.size != 32:
            raise ValueError("sk_decrypt: sk32 must be 32 bytes")
        u = np.frombuffer(b"".join(c[0] for c in cts), dtype=np.uint8).copy()
        w = np.frombuffer(b"".join(c[2] for c in cts), dtype=np.uint8).copy()
        if u.size != 48 * count or w.size != 96 * count:
            raise ValueError("sk_decrypt: every ciphertext is (48 bytes, bytes, 96 bytes)")
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(c[1]) for c in cts])
        vb = np.frombuffer(b"".join(c[1] for c in cts) or b"\0", dtype=np.uint8).copy()
        out = np.zeros_like(vb)
        st = np.zeros(count, dtype=np.uint8)
        self._check(self.lib.hbx_sk_decrypt(self.h, _u8(sk), _u8(u), _u8(vb),
                                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _u8(w), count,
                                            _u8(out), _u8(st)))
        return [out[int(off[j]):int(off[j + 1])].tobytes() for j in range(count)], st

    def bivar_poly_rows(self, coeff32: np.ndarray, t: int, n: int) -> np.ndarray:
        """BivarPoly::row(x), x = 1..n, of coeff32 uint8[(t+1)(t+2)/2, 32] -> uint8[n, t + 1, 32]."""
        coeff32 = np.ascontiguousarray(coeff32, dtype=np.uint8)
        if coeff32.shape != ((t + 1) * (t + 2) // 2, 32):
            raise ValueError("bivar_poly_rows: coeff32 must be [(t + 1)(t + 2)/2, 32]")
        out = np.zeros((n, t + 1, 32), dtype=np.uint8)
        self._check(self.lib.hbx_bivar_poly_rows(self.h, _u8(coeff32), t, n, _u8(out)))
        return out

    def fr_poly_eval(self, coeff32: np.ndarray, n: int) -> np.ndarray:
        """Poly::evaluate(x), x = 1..n, of p polynomials coeff32 uint8[p, t + 1, 32] -> uint8[p, n, 32]."""
        coeff32 = np.ascontiguousarray(coeff32, dtype=np.uint8)
        if coeff32.ndim != 3 or coeff32.shape[2] != 32:
            raise ValueError("fr_poly_eval: coeff32 must be [p, t + 1, 32]")
        p, t = coeff32.shape[0], coeff32.shape[1] - 1
        out = np.zeros((p, n, 32), dtype=np.uint8)
        self._check(self.lib.hbx_fr_poly_eval(self.h, _u8(coeff32), p, t, n, _u8(out)))
        return out

    def keygen_generate(self, commits: np.ndarray, t: int, complete, val_cnt=None, val_y=None, vals32=None):
        """SyncKeyGen::generate over commits uint8[p, (t+1)(t+2)/2, 48]: (pk_commit uint8[t + 1, 48],
        sk share bytes or None for an observer (val_cnt None), status uint8[p]).  On HbxError the
        per-part status of the failed call is in ``self.keygen_status``."""
        commits = np.ascontiguousarray(commits, dtype=np.uint8)
        p = commits.shape[0]
        if commits.shape != (p, (t + 1) * (t + 2) // 2, 48):
            raise ValueError("keygen_generate: commits must be [p, (t + 1)(t + 2)/2, 48]")
        comp = np.ascontiguousarray(complete, dtype=np.uint8)
        if comp.shape != (p,):
            raise ValueError("keygen_generate: complete must be [p]")
        pkc = np.zeros((t + 1, 48), dtype=np.uint8)
        st = np.zeros(p, dtype=np.uint8)
        self.keygen_status = st
        if val_cnt is None:
            self._check(self.lib.hbx_keygen_generate(self.h, _u8(commits), p, t, _u8(comp), None, None, None, _u8(pkc),
                                                     None, _u8(st)))
            return pkc, None, st
        cnt = np.ascontiguousarray(val_cnt, dtype=np.uint32)
        yy = np.ascontiguousarray(val_y, dtype=np.uint64)
        vv = np.ascontiguousarray(vals32, dtype=np.uint8)
        if cnt.shape != (p,) or yy.shape != (p, t + 1) or vv.shape != (p, t + 1, 32):
            raise ValueError("keygen_generate: val_cnt [p], val_y [p, t + 1], vals32 [p, t + 1, 32]")
        sk = np.zeros(32, dtype=np.uint8)
        self._check(self.lib.hbx_keygen_generate(self.h, _u8(commits), p, t, _u8(comp),
                                                 cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                 yy.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), _u8(vv), _u8(pkc),
                                                 _u8(sk), _u8(st)))
        return pkc, sk.tobytes(), st

    def pk_shares_from_commit(self, pk_commit48: np.ndarray, n: int) -> np.ndarray:
        """public_key_share(i) = commit.evaluate(i + 1), i < n, of pk_commit48 uint8[t + 1, 48] -> uint8[n, 48]."""
        pkc = np.ascontiguousarray(pk_commit48, dtype=np.uint8)
        if pkc.ndim != 2 or pkc.shape[1] != 48:
            raise ValueError("pk_shares_from_commit: pk_commit48 must be [t + 1, 48]")
        out = np.zeros((n, 48), dtype=np.uint8)
        self._check(self.lib.hbx_pk_shares_from_commit(self.h, _u8(pkc), pkc.shape[0] - 1, n, _u8(out)))
        return out

    # -- broadcast (torch tensors as HBM buffers) ------------------------------------------------
    def rs_encode_d(self, d_shards, k: int, m: int, stream=None):
        """d_shards: uint8[inst, k + m, L] (parity rows overwritten)."""
        inst, n, L = d_shards.shape
        if n != k + m:
            raise ValueError(f"rs_encode_d: {n} shards per instance != k + m = {k + m}")
        self._check(self.lib.hbx_rs_encode_d(self.h, d_shards.data_ptr(), inst, k, m, L, self._stream(stream)))

    def rs_reconstruct_d(self, d_shards, d_present, d_status, k: int, m: int, stream=None):
        inst, n, L = d_shards.shape
        if n != k + m:
            raise ValueError(f"rs_reconstruct_d: {n} shards per instance != k + m = {k + m}")
        self._check(self.lib.hbx_rs_reconstruct_d(self.h, d_shards.data_ptr(), d_present.data_ptr(), inst, k, m, L,
                                                  d_status.data_ptr(), self._stream(stream)))

    def merkle_roots_d(self, d_shards, d_roots, stream=None):
        inst, n, L = d_shards.shape
        self._check(self.lib.hbx_merkle_roots_d(self.h, d_shards.data_ptr(), inst, n, L, d_roots.data_ptr(), self._stream(stream)))

    def merkle_validate_d(self, d_values, d_nodes, d_sibs, d_sides, d_depth, d_root, d_sender, count: int, d_valid,
                          stream=None):
        nproofs, vlen = d_values.shape
        self._check(self.lib.hbx_merkle_validate_d(
            self.h, d_values.data_ptr(), vlen, d_nodes.data_ptr(), d_sibs.data_ptr(), d_sides.data_ptr(),
            d_depth.data_ptr(), d_root.data_ptr(), d_sender.data_ptr(), count, nproofs, d_valid.data_ptr(), self._stream(stream)))

    # -- Broadcast on host buffers (numpy; no device memory on the caller's side) ----------------
    @staticmethod
    def _host(a, dtype, shape=None, writable=False):
        """A C-contiguous numpy array of `dtype` (and `shape`), in place when it already is one."""
        if not isinstance(a, np.ndarray) or a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
            if writable:
                raise ValueError(f"need a C-contiguous {np.dtype(dtype)} numpy array (written in place)")
            a = np.ascontiguousarray(a, dtype=dtype)
        if shape is not None and tuple(a.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(a.shape)}")
        return a

    def rs_encode(self, shards: np.ndarray, k: int, m: int):
        """hbx_rs_encode: shards uint8[inst, k + m, L] on the host, parity rows written in place."""
        shards = self._host(shards, np.uint8, writable=True)
        inst, n, L = shards.shape
        if n != k + m:  # the library copies (k + m) L bytes per instance each way
            raise ValueError(f"rs_encode: {n} shards per instance != k + m = {k + m}")
        self._check(self.lib.hbx_rs_encode(self.h, shards.ctypes.data, inst, k, m, L))

    def rs_reconstruct(self, shards: np.ndarray, present, k: int, m: int) -> np.ndarray:
        """hbx_rs_reconstruct: shards rebuilt in place; returns status int32[inst]."""
        shards = self._host(shards, np.uint8, writable=True)
        inst, n, L = shards.shape
        if n != k + m:  # the library copies (k + m) L bytes per instance each way
            raise ValueError(f"rs_reconstruct: {n} shards per instance != k + m = {k + m}")
        pres = self._host(present, np.uint8, (inst, n))
        st = np.zeros(inst, dtype=np.int32)
        self._check(self.lib.hbx_rs_reconstruct(self.h, shards.ctypes.data, pres.ctypes.data, inst, k, m, L,
                                                st.ctypes.data))
        return st

    def merkle_roots(self, shards) -> np.ndarray:
        shards = self._host(shards, np.uint8)
        inst, n, L = shards.shape
        roots = np.zeros((inst, 32), dtype=np.uint8)
        self._check(self.lib.hbx_merkle_roots(self.h, shards.ctypes.data, inst, n, L, roots.ctypes.data))
        return roots

    def merkle_build(self, shards):
        """hbx_merkle_build -> (nodes uint8[inst, node_count(n), 32], roots uint8[inst, 32])."""
        shards = self._host(shards, np.uint8)
        inst, n, L = shards.shape
        nodes = np.zeros((inst, self.merkle_node_count(n), 32), dtype=np.uint8)
        roots = np.zeros((inst, 32), dtype=np.uint8)
        self._check(self.lib.hbx_merkle_build(self.h, shards.ctypes.data, inst, n, L, nodes.ctypes.data,
                                              roots.ctypes.data))
        return nodes, roots

    def merkle_proofs(self, nodes, n: int, req):
        """hbx_merkle_proofs: req uint32[count, 2] = (instance, leaf) -> (node_hash, sib_hash, sides,
        depth, root) as hbx_merkle_validate takes them."""
        nodes = self._host(nodes, np.uint8)
        inst = nodes.shape[0]
        req = self._host(req, np.uint32)
        if req.ndim != 2 or req.shape[1] != 2:  # the library reads req[2 q], req[2 q + 1] for q < count
            raise ValueError(f"merkle_proofs: req must be uint32[count, 2] (instance, leaf), got shape {req.shape}")
        count = req.shape[0]
        nh = np.zeros((count, 17, 32), dtype=np.uint8)
        sh = np.zeros((count, 16, 32), dtype=np.uint8)
        sides = np.zeros(count, dtype=np.uint32)
        depth = np.zeros(count, dtype=np.uint32)
        root = np.zeros((count, 32), dtype=np.uint8)
        self._check(self.lib.hbx_merkle_proofs(self.h, nodes.ctypes.data, inst, n, req.ctypes.data, count,
                                               nh.ctypes.data, sh.ctypes.data, sides.ctypes.data, depth.ctypes.data,
                                               root.ctypes.data))
        return nh, sh, sides, depth, root

    def merkle_validate(self, values, nodes, sibs, sides, depth, root, sender, count: int) -> np.ndarray:
        """hbx_merkle_validate: returns valid uint8[nproofs]."""
        values = self._host(values, np.uint8)
        nproofs, vlen = values.shape
        args = [self._host(nodes, np.uint8, (nproofs, 17, 32)), self._host(sibs, np.uint8, (nproofs, 16, 32)),
                self._host(sides, np.uint32, (nproofs,)), self._host(depth, np.uint32, (nproofs,)),
                self._host(root, np.uint8, (nproofs, 32)), self._host(sender, np.uint32, (nproofs,))]
        valid = np.zeros(nproofs, dtype=np.uint8)
        self._check(self.lib.hbx_merkle_validate(self.h, values.ctypes.data, vlen, *[a.ctypes.data for a in args],
                                                 count, nproofs, valid.ctypes.data))
        return valid

    def broadcast_decode(self, shards, present, root, k: int, m: int, leaf_hash=None):
        """hbx_broadcast_decode[_leaves]: shards rebuilt in place -> (out uint8[inst, k L], out_len
        uint64[inst], status int32[inst])."""
        shards = self._host(shards, np.uint8, writable=True)
        inst, n, L = shards.shape
        if n != k + m:
            raise ValueError(f"broadcast_decode: {n} shards per instance != k + m = {k + m}")
        pres = self._host(present, np.uint8, (inst, n))
        root = self._host(root, np.uint8, (inst, 32))
        stride = max(k * L, 1)
        out = np.zeros((inst, stride), dtype=np.uint8)
        out_len = np.zeros(inst, dtype=np.uint64)
        st = np.zeros(inst, dtype=np.int32)
        if leaf_hash is None:
            self._check(self.lib.hbx_broadcast_decode(self.h, shards.ctypes.data, pres.ctypes.data, root.ctypes.data,
                                                      inst, k, m, L, out.ctypes.data, stride, out_len.ctypes.data,
                                                      st.ctypes.data))
        else:
            lh = self._host(leaf_hash, np.uint8, (inst, n, 32))
            self._check(self.lib.hbx_broadcast_decode_leaves(self.h, shards.ctypes.data, pres.ctypes.data,
                                                             lh.ctypes.data, root.ctypes.data, inst, k, m, L,
                                                             out.ctypes.data, stride, out_len.ctypes.data,
                                                             st.ctypes.data))
        return out, out_len, st

    def merkle_node_count(self, n: int) -> int:
        return int(self.lib.hbx_merkle_node_count(n))

    def merkle_build_d(self, d_shards, d_nodes, d_roots=None, stream=None):
        inst, n, L = d_shards.shape
        self._check(self.lib.hbx_merkle_build_d(self.h, d_shards.data_ptr(), inst, n, L, d_nodes.data_ptr(),
                                                None if d_roots is None else d_roots.data_ptr(), self._stream(stream)))

    def merkle_proofs_d(self, d_nodes, n: int, d_req, d_node_hash, d_sib_hash, d_sides, d_depth, d_root, stream=None):
        count = d_req.shape[0]
        self._check(self.lib.hbx_merkle_proofs_d(self.h, d_nodes.data_ptr(), n, d_req.data_ptr(), count,
                                                 d_node_hash.data_ptr(), d_sib_hash.data_ptr(), d_sides.data_ptr(),
                                                 d_depth.data_ptr(), d_root.data_ptr(), self._stream(stream)))

    def broadcast_decode_d(self, d_shards, d_present, d_root, k: int, m: int, d_out, d_out_len, d_status, stream=None):
        inst, n, L = d_shards.shape
        self._check(self.lib.hbx_broadcast_decode_d(
            self.h, d_shards.data_ptr(), d_present.data_ptr(), d_root.data_ptr(), inst, k, m, L, d_out.data_ptr(),
            d_out.shape[1], d_out_len.data_ptr(), d_status.data_ptr(), self._stream(stream)))

    def broadcast_decode_leaves_d(self, d_shards, d_present, d_leaf_hash, d_root, k: int, m: int, d_out, d_out_len,
                                  d_status, stream=None):
        """hbx_broadcast_decode_leaves_d: d_leaf_hash uint8[inst, k + m, 32] = the present shards'
        leaf digests from their validated Echo proofs."""
        import torch

        inst, n, L = d_shards.shape
        # k_import_leaf_hashes reads inst * (k + m) * 32 bytes from this pointer, and the root check
        # trusts them: the layout must be exactly that
        if n != k + m:
            raise ValueError(f"broadcast_decode_leaves_d: {n} shards per instance != k + m = {k + m}")
        if (tuple(d_leaf_hash.shape) != (inst, n, 32) or d_leaf_hash.dtype != torch.uint8
                or not d_leaf_hash.is_contiguous()):
            raise ValueError(f"broadcast_decode_leaves_d: d_leaf_hash must be contiguous uint8[{inst}, {n}, 32], "
                             f"got {d_leaf_hash.dtype}{list(d_leaf_hash.shape)}")
        self._check(self.lib.hbx_broadcast_decode_leaves_d(
            self.h, d_shards.data_ptr(), d_present.data_ptr(), d_leaf_hash.data_ptr(), d_root.data_ptr(), inst, k, m,
            L, d_out.data_ptr(), d_out.shape[1], d_out_len.data_ptr(), d_status.data_ptr(), self._stream(stream)))

    # -- Broadcast, ragged forms: per-instance shard lengths in one call ----------------------------
    ragged_layout = staticmethod(ragged_layout)

    @staticmethod
    def _ragged_desc(what: str, buf_bytes: int, off, lens, pitch, n: int):
        """The descriptor rules of include/hbx.h, checked before the library is reached."""
        off = np.ascontiguousarray(off, dtype=np.uint64).reshape(-1)
        lens = np.ascontiguousarray(lens, dtype=np.uint32).reshape(-1)
        pitch = np.ascontiguousarray(pitch, dtype=np.uint32).reshape(-1)
        inst = off.size
        if inst == 0 or lens.size != inst or pitch.size != inst or n < 1:
            raise ValueError(f"{what}: off, len and pitch need one entry per instance (and n >= 1)")
        if (off % 4).any() or (pitch % 4).any():
            raise ValueError(f"{what}: off and pitch must be multiples of 4")
        if (lens == 0).any() or (pitch < lens).any():
            raise ValueError(f"{what}: need pitch >= len >= 1 for every instance")
        o, end = off.astype(object), off.astype(object) + pitch.astype(object) * n
        if (end > buf_bytes).any():
            raise ValueError(f"{what}: an instance's rows end past the buffer ({buf_bytes} bytes)")
        order = np.argsort(off, kind="stable")
        for a, b in zip(order[:-1], order[1:]):
            if o[b] < end[a]:
                raise ValueError(f"{what}: instances {a} and {b} overlap")
        return off, lens, pitch, inst

    @staticmethod
    def _flat_u8(what: str, t):
        if t.dim() != 1 or t.element_size() != 1 or not t.is_contiguous():
            raise ValueError(f"{what}: need a contiguous 1-D byte tensor")
        return t.numel()

    def rs_encode_ragged_d(self, d_buf, off, lens, pitch, k: int, m: int, stream=None):
        """hbx_rs_encode_ragged_d: d_buf uint8[buf_bytes]; off / lens / pitch host arrays [inst]."""
        nb = self._flat_u8("rs_encode_ragged_d", d_buf)
        off, lens, pitch, inst = self._ragged_desc("rs_encode_ragged_d", nb, off, lens, pitch, k + m)
        self._check(self.lib.hbx_rs_encode_ragged_d(self.h, d_buf.data_ptr(), nb, off.ctypes.data, lens.ctypes.data,
                                                    pitch.ctypes.data, inst, k, m, self._stream(stream)))

    def rs_reconstruct_ragged_d(self, d_buf, off, lens, pitch, d_present, d_status, k: int, m: int, stream=None):
        nb = self._flat_u8("rs_reconstruct_ragged_d", d_buf)
        off, lens, pitch, inst = self._ragged_desc("rs_reconstruct_ragged_d", nb, off, lens, pitch, k + m)
        if tuple(d_present.shape) != (inst, k + m) or d_status.numel() != inst:
            raise ValueError(f"rs_reconstruct_ragged_d: d_present must be [{inst}, {k + m}] and d_status [{inst}]")
        self._check(self.lib.hbx_rs_reconstruct_ragged_d(
            self.h, d_buf.data_ptr(), nb, off.ctypes.data, lens.ctypes.data, pitch.ctypes.data, d_present.data_ptr(),
            inst, k, m, d_status.data_ptr(), self._stream(stream)))

    def merkle_build_ragged_d(self, d_buf, off, lens, pitch, n: int, d_nodes=None, d_roots=None, stream=None):
        """hbx_merkle_build_ragged_d: d_nodes uint8[inst, node_count(n), 32] and / or d_roots uint8[inst, 32]."""
        nb = self._flat_u8("merkle_build_ragged_d", d_buf)
        off, lens, pitch, inst = self._ragged_desc("merkle_build_ragged_d", nb, off, lens, pitch, n)
        if d_nodes is None and d_roots is None:
            raise ValueError("merkle_build_ragged_d: give d_nodes or d_roots")
        self._check(self.lib.hbx_merkle_build_ragged_d(
            self.h, d_buf.data_ptr(), nb, off.ctypes.data, lens.ctypes.data, pitch.ctypes.data, inst, n,
            None if d_nodes is None else d_nodes.data_ptr(), None if d_roots is None else d_roots.data_ptr(),
            self._stream(stream)))

    def merkle_validate_ragged_d(self, d_values, val_off, d_nodes, d_sibs, d_sides, d_depth, d_root, d_sender,
                                 count: int, d_valid, stream=None):
        """hbx_merkle_validate_ragged_d: value j = d_values[val_off[j] : val_off[j + 1]] (val_off: host
        uint64[nproofs + 1]); the other arrays as merkle_validate_d."""
        nb = self._flat_u8("merkle_validate_ragged_d", d_values)
        nproofs = d_valid.numel()
        val_off = np.ascontiguousarray(val_off, dtype=np.uint64).reshape(-1)
        if nproofs == 0 or val_off.size != nproofs + 1:
            raise ValueError(f"merkle_validate_ragged_d: val_off needs nproofs + 1 = {nproofs + 1} entries, got {val_off.size}")
        if (val_off[1:] < val_off[:-1]).any() or int(val_off[-1]) > nb:
            raise ValueError("merkle_validate_ragged_d: val_off must be non-decreasing and end within d_values")
        self._check(self.lib.hbx_merkle_validate_ragged_d(
            self.h, d_values.data_ptr(), nb, val_off.ctypes.data, d_nodes.data_ptr(), d_sibs.data_ptr(),
            d_sides.data_ptr(), d_depth.data_ptr(), d_root.data_ptr(), d_sender.data_ptr(), count, nproofs,
            d_valid.data_ptr(), self._stream(stream)))

    def broadcast_decode_ragged_d(self, d_buf, off, lens, pitch, d_present, d_root, k: int, m: int, d_out, out_off,
                                  d_out_len, d_status, d_leaf_hash=None, stream=None):
        """hbx_broadcast_decode_ragged_d: instance q's payload at d_out[out_off[q]:] (out_off: host
        uint64[inst]); with d_leaf_hash uint8[inst, k + m, 32] only reconstructed shards are hashed."""
        nb = self._flat_u8("broadcast_decode_ragged_d", d_buf)
        ob = self._flat_u8("broadcast_decode_ragged_d", d_out)
        n = k + m
        off, lens, pitch, inst = self._ragged_desc("broadcast_decode_ragged_d", nb, off, lens, pitch, n)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64).reshape(-1)
        if out_off.size != inst or tuple(d_present.shape) != (inst, n) or d_status.numel() != inst \
                or d_out_len.numel() != inst or d_root.numel() != inst * 32:
            raise ValueError(f"broadcast_decode_ragged_d: out_off, d_present, d_root, d_out_len and d_status need {inst} "
                             f"instances of {n} shards")
        spans = sorted((int(o), int(o) + max(k * int(ln) - 4, 0)) for o, ln in zip(out_off, lens))
        if any(e > ob for _, e in spans):
            raise ValueError("broadcast_decode_ragged_d: an instance has no room for k * len - 4 bytes in d_out")
        if any(b[0] < a[1] for a, b in zip(spans[:-1], spans[1:]) if b[1] > b[0] and a[1] > a[0]):
            raise ValueError("broadcast_decode_ragged_d: output ranges overlap")
        if d_leaf_hash is not None and (tuple(d_leaf_hash.shape) != (inst, n, 32) or d_leaf_hash.element_size() != 1
                                        or not d_leaf_hash.is_contiguous()):
            raise ValueError(f"broadcast_decode_ragged_d: d_leaf_hash must be contiguous uint8[{inst}, {n}, 32]")
        self._check(self.lib.hbx_broadcast_decode_ragged_d(
            self.h, d_buf.data_ptr(), nb, off.ctypes.data, lens.ctypes.data, pitch.ctypes.data, d_present.data_ptr(),
            None if d_leaf_hash is None else d_leaf_hash.data_ptr(), d_root.data_ptr(), inst, k, m, d_out.data_ptr(), ob,
            out_off.ctypes.data, d_out_len.data_ptr(), d_status.data_ptr(), self._stream(stream)))

    # -- Broadcast, message by message: the echo store, adds and listed decodes ---------------------
    def prepare_broadcast(self, inst: int, k: int, m: int, max_shard_len: int):
        """hbx_prepare_broadcast: an empty echo store of inst x (k + m) slots of max_shard_len bytes."""
        for name, v in (("inst", inst), ("k", k), ("max_shard_len", max_shard_len)):
            if not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"prepare_broadcast: {name} must be a positive integer")
        if not isinstance(m, (int, np.integer)) or m < 0 or k > 128 or k + m > 256:
            raise ValueError("prepare_broadcast: need 1 <= k <= 128, m >= 0 and k + m <= 256")
        if max_shard_len > 0xFFFFFFF0:
            raise ValueError("prepare_broadcast: max_shard_len does not fit the store's rows")
        self._check(self.lib.hbx_prepare_broadcast(self.h, int(inst), int(k), int(m), int(max_shard_len)))
        self._bc = (int(inst), int(k) + int(m), int(k), (int(max_shard_len) + 3) // 4 * 4)

    @staticmethod
    def _echo_items(what: str, val_off, inst, sender, nbytes: int):
        """The host arrays of an add: val_off uint64[count + 1] within nbytes, (inst, sender) pairs
        each once."""
        val_off = np.asarray(val_off)
        if val_off.ndim != 1 or val_off.size < 1 or val_off.dtype.kind not in "iu" or (val_off.size and int(val_off.min()) < 0):
            raise ValueError(f"{what}: val_off must be count + 1 offsets")
        count = val_off.size - 1
        val_off = np.ascontiguousarray(val_off, dtype=np.uint64)
        if (val_off[1:] < val_off[:-1]).any() or int(val_off[-1]) > nbytes:
            raise ValueError(f"{what}: val_off must be non-decreasing and end within the values ({nbytes} bytes)")
        inst, sender = Context._index_pair(what, ("inst", "sender"), inst, sender, count)
        pairs = set(zip(inst.tolist(), sender.tolist()))
        if len(pairs) != count:
            raise ValueError(f"{what}: the same (inst, sender) twice in one call")
        return val_off, inst, sender, count

    def add_echoes(self, values, val_off, nodes, sibs, sides, depth, root, inst, sender) -> np.ndarray:
        """hbx_add_echoes: host arrays in the layout of flatten_proofs_ragged (values uint8[bytes],
        val_off [count + 1], nodes uint8[count, 17, 32], sibs uint8[count, 16, 32], sides / depth
        uint32[count], root uint8[count, 32]) and the items' (inst, sender) -> HBX_ECHO_* uint8[count]."""
        what = "add_echoes"
        values = np.asarray(values)
        if values.dtype != np.uint8 or values.ndim != 1:
            raise ValueError(f"{what}: values must be uint8[bytes], not {values.dtype}{values.shape}")
        values = np.ascontiguousarray(values)
        val_off, inst, sender, count = self._echo_items(what, val_off, inst, sender, values.size)

        def arr(name, a, dtype, shape):
            a = np.asarray(a)
            if a.dtype != dtype or a.shape != shape:
                raise ValueError(f"{what}: {name} must be {np.dtype(dtype)}{list(shape)}, not {a.dtype}{list(a.shape)}")
            return np.ascontiguousarray(a)

        nodes = arr("nodes", nodes, np.uint8, (count, 17, 32))
        sibs = arr("sibs", sibs, np.uint8, (count, 16, 32))
        sides = arr("sides", sides, np.uint32, (count,))
        depth = arr("depth", depth, np.uint32, (count,))
        root = arr("root", root, np.uint8, (count, 32))
        out = np.zeros(count, dtype=np.uint8)
        if count:
            keep = values if values.size else np.zeros(1, dtype=np.uint8)
            self._check(self.lib.hbx_add_echoes(
                self.h, keep.ctypes.data, values.size, val_off.ctypes.data, nodes.ctypes.data, sibs.ctypes.data,
                sides.ctypes.data, depth.ctypes.data, root.ctypes.data, inst.ctypes.data, sender.ctypes.data, count,
                out.ctypes.data))
        return out

    def add_echoes_d(self, d_values, val_off, d_nodes, d_sibs, d_sides, d_depth, d_root, inst, sender, d_status=None,
                     stream=None):
        """hbx_add_echoes_d: the device tensors of merkle_validate_ragged_d, host val_off / inst /
        sender, d_status an optional device uint8[count]."""
        what = "add_echoes_d"
        nb = self._flat_u8(what, d_values)
        val_off, inst, sender, count = self._echo_items(what, val_off, inst, sender, nb)
        for name, t, cells, width in (("d_nodes", d_nodes, count * 17 * 32, 1), ("d_sibs", d_sibs, count * 16 * 32, 1),
                                      ("d_sides", d_sides, count, 4), ("d_depth", d_depth, count, 4),
                                      ("d_root", d_root, count * 32, 1)):
            if t.numel() != cells or t.element_size() != width or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be contiguous with {cells} elements of {width} byte(s)")
        if d_status is not None and (d_status.numel() != count or d_status.element_size() != 1):
            raise ValueError(f"{what}: d_status must have one byte per item ({count})")
        if count:
            self._check(self.lib.hbx_add_echoes_d(
                self.h, d_values.data_ptr(), nb, val_off.ctypes.data, d_nodes.data_ptr(), d_sibs.data_ptr(),
                d_sides.data_ptr(), d_depth.data_ptr(), d_root.data_ptr(), inst.ctypes.data, sender.ctypes.data, count,
                None if d_status is None else d_status.data_ptr(), self._stream(stream)))

    @staticmethod
    def _attempts(what: str, insts, roots, lens, use, n):
        """A decode list: insts uint32[na], roots uint8[na, 32], lens uint32[na] >= 1, use None or
        uint8[na, n]; each (instance, root, use row) once."""
        insts = np.asarray(insts)
        if insts.ndim != 1 or (insts.size and (insts.dtype.kind not in "iu" or int(insts.min()) < 0)):
            raise ValueError(f"{what}: insts must be a list of instances")
        na = insts.size
        insts = np.ascontiguousarray(insts, dtype=np.uint32)
        roots = np.asarray(roots)
        if roots.dtype != np.uint8 or roots.shape != (na, 32):
            raise ValueError(f"{what}: roots must be uint8[{na}, 32], not {roots.dtype}{roots.shape}")
        roots = np.ascontiguousarray(roots)
        lens = np.asarray(lens)
        if lens.shape != (na,) or (na and (lens.dtype.kind not in "iu" or int(lens.min()) < 1 or int(lens.max()) > 0xFFFFFFFF)):
            raise ValueError(f"{what}: len must hold one shard length >= 1 per attempt")
        lens = np.ascontiguousarray(lens, dtype=np.uint32)
        if use is not None:
            use = np.asarray(use)
            if n is None or use.dtype not in (np.uint8, np.bool_) or use.shape != (na, n):
                raise ValueError(f"{what}: use must be uint8[{na}, n = {n}], not {use.dtype}{use.shape}")
            use = np.ascontiguousarray(use != 0, dtype=np.uint8)  # a byte allows its sender iff non-zero
        keys = {(int(insts[a]), roots[a].tobytes(), None if use is None else use[a].tobytes()) for a in range(na)}
        if len(keys) != na:
            raise ValueError(f"{what}: the same (instance, root, use row) is listed twice")
        return insts, roots, lens, use, na

    def _bc_dims(self, what: str):
        bc = getattr(self, "_bc", None)
        if bc is None:
            raise ValueError(f"{what}: no echo store (prepare_broadcast)")
        return bc

    def broadcast_decode_insts(self, insts, roots, lens, use=None, n=None):
        """hbx_broadcast_decode_insts: the listed attempts out of the echo store -> (payloads
        [bytes | None per attempt], status int32[na]).  n: the node count `use` rows must have
        (default: the prepared store's)."""
        what = "broadcast_decode_insts"
        if n is None:
            n = self._bc_dims(what)[1]
        insts, roots, lens, use, na = self._attempts(what, insts, roots, lens, use, n)
        if na == 0:
            return [], np.zeros(0, dtype=np.int32)
        k = self._bc_dims(what)[2]
        room = (np.maximum(k * lens.astype(np.int64) - 4, 0) + 15) // 16 * 16
        out_off = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.uint64)
        out = np.zeros(max(int(room.sum()), 16), dtype=np.uint8)
        out_len = np.zeros(na, dtype=np.uint64)
        status = np.zeros(na, dtype=np.int32)
        self._check(self.lib.hbx_broadcast_decode_insts(
            self.h, insts.ctypes.data, roots.ctypes.data, lens.ctypes.data, None if use is None else use.ctypes.data, na,
            out.ctypes.data, out.size, out_off.ctypes.data, out_len.ctypes.data, status.ctypes.data))
        vals = [out[int(o): int(o) + int(ln)].tobytes() if st == 0 else None for o, ln, st in zip(out_off, out_len, status)]
        return vals, status

    def broadcast_decode_insts_d(self, insts, roots, lens, d_out, out_off, d_out_len, d_status, use=None, n=None,
                                 stream=None):
        """hbx_broadcast_decode_insts_d: host insts / roots / lens / use / out_off; attempt a's payload at
        d_out[out_off[a]:], d_out_len int64[na], d_status int32[na]."""
        what = "broadcast_decode_insts_d"
        if n is None:
            n = self._bc_dims(what)[1]
        insts, roots, lens, use, na = self._attempts(what, insts, roots, lens, use, n)
        ob = self._flat_u8(what, d_out)
        out_off = np.ascontiguousarray(out_off, dtype=np.uint64).reshape(-1)
        if out_off.size != na or d_out_len.numel() != na or d_status.numel() != na or d_out_len.element_size() != 8 \
                or d_status.element_size() != 4:
            raise ValueError(f"{what}: out_off, d_out_len (64-bit) and d_status (32-bit) need {na} entries")
        if na:
            self._check(self.lib.hbx_broadcast_decode_insts_d(
                self.h, insts.ctypes.data, roots.ctypes.data, lens.ctypes.data, None if use is None else use.ctypes.data,
                na, d_out.data_ptr(), ob, out_off.ctypes.data, d_out_len.data_ptr(), d_status.data_ptr(),
                self._stream(stream)))

    def echo_slots(self, rows: bool = False):
        """hbx_get_echo_slots: (state uint8[inst, n], len uint32[inst, n], root uint8[inst, n, 32]) of
        the echo store; rows=True adds the shard rows uint8[inst * n + 1, pitch] (hbx_debug_get_echo_rows:
        the last one is the canary row)."""
        inst, n, _, pitch = self._bc_dims("echo_slots")
        state = np.zeros((inst, n), dtype=np.uint8)
        lens = np.zeros((inst, n), dtype=np.uint32)
        root = np.zeros((inst, n, 32), dtype=np.uint8)
        self._check(self.lib.hbx_get_echo_slots(self.h, state.ctypes.data, lens.ctypes.data, root.ctypes.data))
        if not rows:
            return state, lens, root
        buf = np.zeros((inst * n + 1, pitch), dtype=np.uint8)
        self._check(self.lib.hbx_debug_get_echo_rows(self.h, buf.ctypes.data, buf.size))
        return state, lens, root, buf

    def get_ct_valid_d(self, d_ct_valid, stream=None):
        self._check(self.lib.hbx_get_ct_valid_d(self.h, d_ct_valid.data_ptr(), self._stream(stream)))

    def combine_decrypt_d(self, t: int, d_out, d_status=None, stream=None):
        self._check(self.lib.hbx_combine_decrypt_d(
            self.h, t, d_out.data_ptr(), None if d_status is None else d_status.data_ptr(), self._stream(stream)))

    def decrypt_epoch_d(self, d_u, d_v, d_off, d_w, p: int, max_v_len: int, d_shares, n: int, t: int, d_out,
                        d_valid=None, d_ct_valid=None, d_status=None, d_present=None, stream=None):
        """One node-epoch (hbx_decrypt_epoch_d): prepare + share checks (with Ciphertext::verify) +
        combine + decrypt; same results as the three-call sequence."""
        opt = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self._v_off, self._d_off = None, d_off
        self._check(self.lib.hbx_decrypt_epoch_d(
            self.h, d_u.data_ptr(), d_v.data_ptr(), d_off.data_ptr(), d_w.data_ptr(), p, max_v_len,
            d_shares.data_ptr(), opt(d_present), n, t, opt(d_valid), opt(d_ct_valid), d_out.data_ptr(),
            opt(d_status), self._stream(stream)))

    def add_dec_shares_d(self, d_shares48, proposer, sender, n: int, d_status=None, stream=None):
        """hbx_add_dec_shares_d: d_shares48 a device uint8[count, 48] tensor (None with no items),
        proposer / sender host index arrays, d_status an optional device uint8[count]."""
        self._add_device("hbx_add_dec_shares_d", 48, ("d_shares48", "proposer", "sender"), d_shares48, proposer, sender, n,
                         d_status, stream)

    def combine_decrypt_cols_d(self, t: int, cols, d_out, d_status=None, stream=None):
        """hbx_combine_decrypt_cols_d: cols a host list of proposer columns; d_out / d_status as for
        combine_decrypt_d (only the listed proposers' ranges and entries are written)."""
        cols = self._index_list("combine_decrypt_cols_d", "cols", "proposer columns", "a column", cols)
        self._check(self.lib.hbx_combine_decrypt_cols_d(
            self.h, t, cols.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if cols.size else None, cols.size,
            d_out.data_ptr(), None if d_status is None else d_status.data_ptr(), self._stream(stream)))
