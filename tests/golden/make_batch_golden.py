"""Generate the committed fixture of the batched share verification (hbx_set_batch_verify) with the
oracle and hashlib.

    python tests/golden/make_batch_golden.py      # batch_sums.npz

For a fixed seed and the call indices 0 and 1: the coefficients
    r_i = int.from_bytes(SHA-256(seed || LE64(call_index) || LE32(i))[:16], "little")
(i = 0xFFFFFFFF is the ciphertext term r_ct) and, per proposer column j, the share-side sum
    A_j = sum_{i included} r_i S_ji
that hbx_get_batch_sums returns after hbx_prepare_ciphertexts + hbx_verify_dec_shares (the three-call
host API, no own share): included senders are present and their share decodes to a G1 point other
than the identity; a column whose ciphertext is not valid (not examined) or whose U_j / W_j is the
identity (left to the per-share path) has the identity encoding.

Inputs are committed epoch fixtures: hb_epoch_n7 (every edge case; key "n7"), hb_cols_n256 sliced
to senders [:65] ("c65": one sender past a wave of the block reduction) and hb_cols_n256 whole
("c256": four full waves).  Keys of the .npz: seed; coeff_<in>_<k> uint8[n + 1, 16] (little-endian,
r_ct last); sums_<in>_<k> uint8[p, 48], k = call index.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import bls12_381 as bls  # noqa: E402

SEED = hashlib.sha256(b"hbx batch verify golden seed").digest()
CT_INDEX = 0xFFFFFFFF
INPUTS = (("n7", "hb_epoch_n7", None), ("c65", "hb_cols_n256", 65), ("c256", "hb_cols_n256", None))


def coeff(seed: bytes, call_index: int, i: int) -> int:
    d = hashlib.sha256(seed + call_index.to_bytes(8, "little") + i.to_bytes(4, "little")).digest()
    return int.from_bytes(d[:16], "little")


def decode_share(b: bytes):
    """The G1 point of an included share, None for one that takes no part in A_j."""
    try:
        return bls.g1_decompress(b)  # None for the identity
    except ValueError:
        return None


def column_sums(d, n_slice, call_index: int):
    shares, present = d["shares"], d["present"]
    p, n = shares.shape[:2]
    n = n_slice or n
    out = np.zeros((p, 48), dtype=np.uint8)
    for j in range(p):
        acc = None
        examined = int(d["expect_ct_status"][j]) == 1 and not (d["u"][j][0] & 0x40) and not (d["w"][j][0] & 0x40)
        if examined:
            for i in range(n):
                if not present[j, i]:
                    continue
                pt = decode_share(shares[j, i].tobytes())
                if pt is not None:
                    acc = bls.g1_add(acc, bls.g1_mul(pt, coeff(SEED, call_index, i)))
        out[j] = np.frombuffer(bls.g1_compress(acc), dtype=np.uint8)
    return out


def main():
    res = {"seed": np.frombuffer(SEED, dtype=np.uint8)}
    for key, name, n_slice in INPUTS:
        d = dict(np.load(os.path.join(HERE, f"{name}.npz"), allow_pickle=False))
        n = n_slice or d["shares"].shape[1]
        for k in (0, 1):
            rs = [coeff(SEED, k, i) for i in range(n)] + [coeff(SEED, k, CT_INDEX)]
            res[f"coeff_{key}_{k}"] = np.frombuffer(b"".join(r.to_bytes(16, "little") for r in rs),
                                                    dtype=np.uint8).reshape(n + 1, 16)
            res[f"sums_{key}_{k}"] = column_sums(d, n_slice, k)
    np.savez_compressed(os.path.join(HERE, "batch_sums.npz"), **res)
    print("wrote batch_sums.npz:", {k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main()
