"""Generate the committed fixtures of PublicKey::verify over a key table (hbx_verify_sigs_keyed) and
of SecretKey::sign (hbx_sign_msgs) with the oracle.

    python tests/golden/make_kgsig_golden.py      # kgsigs_b65.npz, kgsigs_b9_sha3.npz

Dynamic HoneyBadger checks every committed SignedKeyGenMsg with `pk.verify(&sig, bincode(kg_msg))`
(src/dynamic_honey_badger/dynamic_honey_badger.rs:254-272, :395-410) under the sender's key from the
validator table (or the candidate's), and signs every Part and Ack it sends (:363).  An era has few
keys and many items, so the items name their key by index.

65 items: three 32-pair blocks of the pair-lane check, the last with one live pair.  The key table has
9 entries: six honest keys, the identity, a point off the G1 subgroup, an undecodable encoding.
Message lengths 0, 1, 55, 56, 63, 64, 65, 119, 120 (the digest's padding boundaries), 300 and 4,099 B,
then random lengths below 300 B.
Cases: valid; a signature over another message; a signature by another key of the table; sigma plus a
point of the cofactor part; a cleared compression flag; an index to the off-subgroup key; an index to
the undecodable key; identity key with identity sigma (true) and with a real sigma (false);
key_idx == nkeys and key_idx == 0xFFFFFFFF (no key: the reference's pk_opt is None).
Expected: HBX_SHARE_VALID (1) / INVALID (0) / UNDECODABLE (3) / UNKNOWN_SENDER (5) per item, HBX_PT_*
per key; `sign_sk` and `expect_sig`: all 65 messages signed under one key.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import bls12_381 as bls  # noqa: E402
from oracle import threshold as tc  # noqa: E402
from oracle.chacha_rand04 import ChaChaRng04  # noqa: E402

sys.path.insert(0, HERE)
from make_coin_golden import cofactor_point  # noqa: E402
from make_golden import off_subgroup_g1  # noqa: E402

INVALID, VALID, UNDECODABLE, UNKNOWN_SENDER = 0, 1, 3, 5
PT_OK, PT_NOT_IN_FIELD, PT_INFINITY, PT_NOT_IN_SUBGROUP = 0, 2, 4, 5
IDENTITY_G1 = bytes([0xC0]) + bytes(47)
IDENTITY_G2 = bytes([0xC0]) + bytes(95)
HONEST, K_IDENT, K_OFFSUB, K_UNDEC, NKEYS = 6, 6, 7, 8, 9
NO_KEY = 0xFFFFFFFF
LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 300, 4099]


def make(count: int = 65, digest: str = "sha256"):
    rng = ChaChaRng04([0x68626278, 0x6B67])
    sks = [tc.fr_rand(rng) for _ in range(HONEST)]
    sign_sk = tc.fr_rand(rng)
    mrng = np.random.default_rng(0x6B67)
    # always the 65 messages, then the prefix: a shorter fixture holds the same first items
    lens = LENS + [int(mrng.integers(0, 300)) for _ in range(65 - len(LENS))]
    msgs = [mrng.integers(0, 256, size=ln, dtype=np.uint8).tobytes() for ln in lens][:count]
    hs = [tc.hash_g2(m, digest) for m in msgs]
    pk = [bls.g1_compress(bls.g1_mul(bls.G1_GEN, sk)) for sk in sks]
    pk.append(IDENTITY_G1)
    pk.append(bls.g1_compress(off_subgroup_g1(4343)))
    bad = bytearray(pk[0]); bad[1:] = b"\xff" * 47; bad[0] = 0x9F; pk.append(bytes(bad))  # x >= q
    key_status = [PT_OK] * HONEST + [PT_INFINITY, PT_NOT_IN_SUBGROUP, PT_NOT_IN_FIELD]
    key_idx = [i % HONEST for i in range(count)]

    def signed(i, key=None, msg=None):
        k = key_idx[i] if key is None else key
        if msg is None:
            return bls.g2_compress(tc.sign(sks[k], msgs[i], digest, hs[i]))
        return bls.g2_compress(tc.sign(sks[k], msg, digest))

    sig = [signed(i) for i in range(count)]
    expect = [VALID] * count

    def fault(i, value, s=None, key=None):
        expect[i] = value
        if s is not None:
            sig[i] = s
        if key is not None:
            key_idx[i] = key

    # the first nine items hold one case of every status (the SHA3 fixture is this prefix)
    fault(1, INVALID, signed(1, msg=msgs[1] + b"x"))
    fault(2, INVALID, signed(2, key=(key_idx[2] + 1) % HONEST))
    fault(3, UNDECODABLE, bls.g2_compress(bls.g2_add(tc.sign(sks[key_idx[3]], msgs[3], digest, hs[3]), cofactor_point())))
    bad = bytearray(sig[4]); bad[0] &= 0x1F
    fault(4, UNDECODABLE, bytes(bad))  # compression flag cleared
    fault(5, UNDECODABLE, key=K_OFFSUB)
    fault(6, VALID, IDENTITY_G2, key=K_IDENT)
    fault(7, INVALID, key=K_IDENT)
    fault(8, UNKNOWN_SENDER, key=NKEYS)
    if count >= 65:  # and again further on, next to the block boundaries and in the last pair
        fault(12, UNDECODABLE, key=K_UNDEC)
        fault(13, UNKNOWN_SENDER, key=NO_KEY)
        fault(31, INVALID, signed(31, msg=msgs[30]))
        fault(32, UNDECODABLE, bls.g2_compress(bls.g2_add(tc.sign(sks[key_idx[32]], msgs[32], digest, hs[32]), cofactor_point())))
        fault(33, INVALID, signed(33, key=(key_idx[33] + 2) % HONEST))
        fault(40, UNKNOWN_SENDER, IDENTITY_G2, key=NO_KEY)  # nothing else of the item is examined
        fault(41, UNDECODABLE, IDENTITY_G2, key=K_UNDEC)
        fault(63, VALID, IDENTITY_G2, key=K_IDENT)
        fault(64, INVALID, signed(64, msg=b"another message"))
    # the oracle's verdict on every decodable item agrees with the table above
    for i in range(count):
        if expect[i] == UNKNOWN_SENDER:
            assert key_idx[i] >= NKEYS, i
            continue
        if expect[i] == UNDECODABLE:  # pairing 0.14 into_affine rejects the key or the signature
            bad = 0
            for dec, b in ((bls.g1_decompress, pk[key_idx[i]]), (bls.g2_decompress, sig[i])):
                try:
                    dec(b)
                except ValueError:
                    bad += 1
            assert bad, i
            continue
        P = bls.g1_decompress(pk[key_idx[i]])
        S = bls.g2_decompress(sig[i])
        assert tc.verify_sig(P, S, msgs[i], digest, hs[i]) == (expect[i] == VALID), i
    off = np.zeros(count + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    expect_sig = [bls.g2_compress(tc.sign(sign_sk, m, digest, h)) for m, h in zip(msgs, hs)]
    return dict(variant=np.array(f"digest={digest}"), count=np.int64(count),
                pk=np.frombuffer(b"".join(pk), dtype=np.uint8).reshape(NKEYS, 48),
                key_idx=np.array(key_idx, dtype=np.uint32),
                sig=np.frombuffer(b"".join(sig), dtype=np.uint8).reshape(count, 96),
                msg_blob=np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8), msg_off=off,
                expect=np.array(expect, dtype=np.uint8), expect_key_status=np.array(key_status, dtype=np.int32),
                h=np.stack([np.frombuffer(bls.g2_compress(h), dtype=np.uint8) for h in hs]),
                sign_sk=np.frombuffer(sign_sk.to_bytes(32, "big"), dtype=np.uint8),
                expect_sig=np.frombuffer(b"".join(expect_sig), dtype=np.uint8).reshape(count, 96))


def main():
    for name, kw in (("kgsigs_b65", {}), ("kgsigs_b9_sha3", dict(count=9, digest="sha3_256"))):
        d = make(**kw)
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **d)
        print(name, d["expect"].tolist())


if __name__ == "__main__":
    main()
