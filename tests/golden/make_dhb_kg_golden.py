"""Generate the committed fixtures of the signed key-generation replay with the oracle and the CPU
models (tests/skg_model.py, tests/dhb_kg_model.py).

    python tests/golden/make_dhb_kg_golden.py      # dhb_kg_n4.npz, dhb_kg_n7.npz

Each fixture takes the era messages of skg_n4 / skg_n7 (tests/skg_fixture.py load_era) as the
committed SignedKeyGenMsg items of Dynamic HoneyBadger batches
(src/dynamic_honey_badger/dynamic_honey_badger.rs:254-272): item k carries era message item_msg[k],
its serialisation (dhb_kg_model.ser_kg_msg) signed with the sender's node key, the proposer of the
batch that carried it, and an epoch.  An era message whose sender is not a node has no key.
Injected, each a copy of one of the first Acks placed in front of it, so the era goes on as before:
a wrong signature (over other bytes); another node's signature; an unknown sender; an obsolete
epoch (validly signed: skipped all the same); an undecodable sigma; sigma plus a cofactor point;
one message from a candidate's key (index n: verified, then no node of the era).  A few real Acks
of one Part also lose their signatures (LOST): that Part is left with 2t acks, so what generate()
returns differs from the unsigned era's.
Expected: per-item outcomes (KeyGenReplay's OUT_*, OBSOLETE 16, BAD_SIGNATURE 17), the HBX_SHARE_*
status of every non-obsolete item, the fault list (batch proposers), the generated keys.
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

sys.path.insert(0, os.path.dirname(HERE))
import dhb_kg_model as dhb  # noqa: E402  (tests/dhb_kg_model.py)
import skg_model as skg  # noqa: E402
from skg_fixture import load_era  # noqa: E402

START_EPOCH = 2
INVALID, VALID, UNDECODABLE, UNKNOWN_SENDER = 0, 1, 3, 5
# Acks (counted from the first one) whose real signature is replaced: one Part of the era drops to 2t
# acks, is not complete, and stays out of the generated keys
LOST = {4: (12, 13), 7: (13, 14, 15)}


def make(name: str):
    d = load_era(name)
    n, t, me = int(d["n"]), int(d["t"]), int(d["me"])
    sks = [int.from_bytes(s.tobytes(), "big") for s in d["sk_nodes"]]
    pks = [bls.g1_decompress(p.tobytes()) for p in d["pk_nodes"]]
    rng = ChaChaRng04([0x68626278, 0x64686200 + n])
    cand_sk = tc.fr_rand(rng)
    cand_pk = bls.g1_mul(bls.G1_GEN, cand_sk)
    msgs = d["msgs"]
    sers = [dhb.ser_kg_msg(kind, body) for kind, _, body in msgs]
    a0 = next(k for k, m in enumerate(msgs) if m[0] == skg.ACK)

    def sign(sk, data):
        return bls.g2_compress(tc.sign(sk, data))

    def key_of(sender):
        return sks[sender if sender is not None else 0]

    items = []  # (era message, batch proposer, epoch, sender, sig96, SHARE_* status or None)

    def add(m, sender, sig, status, epoch=None):
        k = len(items)
        items.append((m, (5 * k + 1) % n, START_EPOCH + k % 3 if epoch is None else epoch, sender, sig, status))

    for m, (kind, sender, body) in enumerate(msgs):
        good = sign(key_of(sender), sers[m])
        j = m - a0
        if j == 0:
            add(m, sender, sign(sks[sender], sers[m] + b"x"), INVALID)
        elif j == 1:
            add(m, sender, sign(sks[(sender + 1) % n], sers[m]), INVALID)
        elif j == 2:
            add(m, None, good, UNKNOWN_SENDER)
        elif j == 3:
            add(m, sender, good, None, epoch=START_EPOCH - 1)
        elif j == 4:
            bad = bytearray(good); bad[0] &= 0x1F
            add(m, sender, bytes(bad), UNDECODABLE)
        elif j == 5:
            add(m, sender, bls.g2_compress(bls.g2_add(tc.sign(sks[sender], sers[m]), cofactor_point())), UNDECODABLE)
        elif j == 6:
            add(m, n, sign(cand_sk, sers[m]), VALID)
        if j in LOST[n]:
            add(m, sender, sign(sks[sender], b"lost" + sers[m]), INVALID)
        else:
            add(m, sender, good, UNKNOWN_SENDER if sender is None else VALID)

    model = dhb.DhbKeyGenModel(skg.SyncKeyGenModel(me, sks[me], pks, t), pks, (n, cand_pk), START_EPOCH)
    run_items = [(p, e, s, msgs[m][0], msgs[m][2], sers[m], sig) for m, p, e, s, sig, _ in items]
    ack_r = {k: [int.from_bytes(r.tobytes(), "big") for r in d["ack_r_by_msg"][it[0]]]
             for k, it in enumerate(items) if msgs[it[0]][0] == skg.PART}
    outcomes, _ = model.run(run_items, ack_r)
    # the statuses written above are what the model's signature check says
    for (m, p, e, s, sig, st), o in zip(items, outcomes):
        assert (st is None) == (o == dhb.OBSOLETE), m
        assert (st == VALID) == (o not in (dhb.OBSOLETE, dhb.BAD_SIGNATURE)), m
    pk_commit, sk_me = model.skg.generate()
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(sers[it[0]]) for it in items])
    print(name, "outcomes", outcomes, "faults", [f[0] for f in model.faults])
    return dict(base=np.array(name), n=np.int64(n), start_epoch=np.int64(START_EPOCH), cand_idx=np.int64(n),
                cand_pk=np.frombuffer(bls.g1_compress(cand_pk), dtype=np.uint8),
                cand_sk=np.frombuffer(cand_sk.to_bytes(32, "big"), dtype=np.uint8),
                item_msg=np.array([it[0] for it in items], dtype=np.int64),
                item_proposer=np.array([it[1] for it in items], dtype=np.int64),
                item_epoch=np.array([it[2] for it in items], dtype=np.int64),
                item_sender=np.array([-1 if it[3] is None else it[3] for it in items], dtype=np.int64),
                item_sig=np.frombuffer(b"".join(it[4] for it in items), dtype=np.uint8).reshape(len(items), 96),
                ser_blob=np.frombuffer(b"".join(sers[it[0]] for it in items), dtype=np.uint8), ser_off=off,
                expect_status=np.array([it[5] for it in items if it[5] is not None], dtype=np.uint8),
                expect_outcome=np.array(outcomes, dtype=np.uint8),
                fault_proposer=np.array([f[0] for f in model.faults], dtype=np.int64),
                pk_commit=np.frombuffer(b"".join(bls.g1_compress(c) for c in pk_commit), dtype=np.uint8).reshape(t + 1, 48),
                sk_me=np.frombuffer(sk_me.to_bytes(32, "big"), dtype=np.uint8))


def main():
    for era in ("skg_n4", "skg_n7"):
        out = era.replace("skg", "dhb_kg")
        path = os.path.join(HERE, f"{out}.npz")
        np.savez_compressed(path, **make(era))
        print(out, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
