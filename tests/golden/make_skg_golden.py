"""Generate the committed SyncKeyGen fixtures (reference src/sync_key_gen.rs) with the oracle.

    python tests/golden/make_skg_golden.py      # skg_batch65.npz, skg_gen_n4.npz, skg_gen_n7.npz

skg_batch65 -- PublicKey::encrypt / SecretKey::decrypt (sync_key_gen.rs:295, :326, :345, :444):
  65 ciphertexts to ONE key (one more than a wave), message lengths cycling through
  {0, 1, 32, 64, 65, 96} (65 and 96 take the |m| > 64 digest branch of hash_g1_g2), index 7 with a
  flipped V bit (Ciphertext::verify false), index 21 with W off the G2 subgroup (undecodable), and
  the same 65 messages encrypted to 65 DIFFERENT keys with other randomness (hbx_encrypt_to).
  Every valid ciphertext and the tampered one are re-checked with oracle ciphertext_verify.

skg_gen_n4 (t = 1), skg_gen_n7 (t = 2) -- SyncKeyGen::generate (:396-409) and
  PublicKeySet::public_key_share (messaging.rs:251-254): n dealers' symmetric bivariate polynomials
  (coefficients in coeff_pos order; dealer 0 holds a zero coefficient), their commitments, which
  parts are complete (the last one is not), the summed commitment row(0), every node's secret key
  share sum_q f_q(i + 1, 0) and public key share, and one G1 point off the subgroup for the
  does-not-deserialise case.  Ack values are f_q(x, y) in Fr: tests compute them from the
  coefficients with Python integers.

    python tests/golden/make_skg_golden.py --era  # skg_n4.npz (t = 1, me = 1), skg_n7.npz (t = 2, me = 3)

skg_n4, skg_n7 -- one node's whole era, message by message, from the model tests/skg_model.py: every
  node's Part, the Acks honest nodes answer, the randomness of this node's own Acks, and every
  expected byte and outcome (the Acks produced, per-message outcomes, `complete`, pk_commit, the
  node's share, all public key shares, every node's share, the dealer's coefficients and
  randomness).  The n7 row plaintext is 96 B (the |m| > 64 branch of hash_g1_g2).  Faults in n7:
  part 2's row for `me` belongs to another polynomial, part 4's row ciphertext has a flipped V byte,
  part 5's row plaintext is 95 B, a duplicate Part, a Part from an unknown sender; an ack with a wrong
  value among part 0's first 2t + 1, an ack with a tampered W and one with a value >= r for part 3,
  an ack with n - 1 values and a duplicate ack for part 6, an unknown proposer, an ack from an unknown
  sender; part 1 stays at exactly 2t acks.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import bivar  # noqa: E402
from oracle import bls12_381 as bls  # noqa: E402
from oracle import threshold as tc  # noqa: E402
from oracle.chacha_rand04 import ChaChaRng04  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import off_subgroup_g1, off_subgroup_g2  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import skg_model as skg  # noqa: E402  (tests/skg_model.py)

CT_INVALID, CT_VALID, CT_UNDECODABLE = 0, 1, 3
LENS = (0, 1, 32, 64, 65, 96)


def _u8(chunks, *shape):
    return np.frombuffer(b"".join(chunks), dtype=np.uint8).reshape(*shape)


def _blob(items):
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(b) for b in items])
    return np.frombuffer(b"".join(items), dtype=np.uint8).copy(), off


def make_batch65():
    count = 65
    rng = ChaChaRng04([0x68626278, 0x736B6765])
    sk = tc.fr_rand(rng)
    pk = bls.g1_mul(bls.G1_GEN, sk)
    msgs = [bytes(rng.next_u32() & 0xFF for _ in range(LENS[j % len(LENS)])) for j in range(count)]
    r = [tc.fr_rand(rng) for _ in range(count)]
    cts = [tc.encrypt(pk, m, rj) for m, rj in zip(msgs, r)]
    enc = [(bls.g1_compress(u), v, bls.g2_compress(w)) for u, v, w in cts]  # hbx_encrypt's expected bytes
    expect = [CT_VALID] * count
    wire = list(enc)
    # index 7: a flipped bit of V (length 1)
    u7, v7, w7 = cts[7]
    v7 = bytes([v7[0] ^ 0x10]) + v7[1:]
    wire[7] = (enc[7][0], v7, enc[7][2])
    expect[7] = CT_INVALID
    assert not tc.ciphertext_verify((u7, v7, w7))
    # index 21: W on the curve but off the G2 subgroup
    wire[21] = (enc[21][0], enc[21][1], bls.g2_compress(off_subgroup_g2(6565)))
    expect[21] = CT_UNDECODABLE
    for j in range(count):
        if expect[j] == CT_VALID:
            assert tc.ciphertext_verify(cts[j]), j
            g = bls.g1_mul(cts[j][0], sk)
            assert tc.xor_bytes(tc.hash_bytes(g, len(msgs[j])), cts[j][1]) == msgs[j]
    plain = [m if e == CT_VALID else bytes(len(m)) for m, e in zip(msgs, expect)]
    # the same messages to 65 different keys
    sk_to = [tc.fr_rand(rng) for _ in range(count)]
    r_to = [tc.fr_rand(rng) for _ in range(count)]
    pk_to = [bls.g1_mul(bls.G1_GEN, s) for s in sk_to]
    cts_to = [tc.encrypt(pkj, m, rj) for pkj, m, rj in zip(pk_to, msgs, r_to)]
    msg_blob, off = _blob(msgs)
    return dict(sk=_u8([sk.to_bytes(32, "big")], 32), pk=_u8([bls.g1_compress(pk)], 48), msg_blob=msg_blob, off=off,
                r=_u8([x.to_bytes(32, "big") for x in r], count, 32),
                enc_u=_u8([c[0] for c in enc], count, 48), enc_v=_blob([c[1] for c in enc])[0],
                enc_w=_u8([c[2] for c in enc], count, 96),
                u=_u8([c[0] for c in wire], count, 48), v_blob=_blob([c[1] for c in wire])[0],
                w=_u8([c[2] for c in wire], count, 96), expect_status=np.array(expect, dtype=np.uint8),
                expect_plain=_blob(plain)[0],
                sk_to=_u8([x.to_bytes(32, "big") for x in sk_to], count, 32),
                pk_to=_u8([bls.g1_compress(x) for x in pk_to], count, 48),
                r_to=_u8([x.to_bytes(32, "big") for x in r_to], count, 32),
                to_u=_u8([bls.g1_compress(c[0]) for c in cts_to], count, 48), to_v=_blob([c[1] for c in cts_to])[0],
                to_w=_u8([bls.g2_compress(c[2]) for c in cts_to], count, 96))


def make_gen(n: int):
    t = (n - 1) // 3
    M = bivar.n_coeffs(t)
    rng = ChaChaRng04([0x68626278, 0x67656E00 + n])
    polys = [bivar.BivarPoly(t, [tc.fr_rand(rng) for _ in range(M)]) for _ in range(n)]
    polys[0].coeff[bivar.coeff_pos(0, t)] = 0  # g1 * 0: the identity encoding inside a commitment
    commits = [pl.commitment() for pl in polys]
    complete = [1] * n
    complete[n - 1] = 0
    # commit.row(0) summed over the complete parts: coefficient j is sum_q C_q[coeff_pos(0, j)]
    pk_commit = []
    for j in range(t + 1):
        acc = None
        for q in range(n):
            if complete[q]:
                acc = bls.g1_add(acc, commits[q][bivar.coeff_pos(0, j)])
        pk_commit.append(acc)
    pks = tc.PublicKeySet(pk_commit)
    sk_all = [sum(polys[q].evaluate(i + 1, 0) for q in range(n) if complete[q]) % bls.R for i in range(n)]
    pk_shares = [pks.public_key_share(i) for i in range(n)]
    for i in range(n):
        assert pk_shares[i] == bls.g1_mul(bls.G1_GEN, sk_all[i]), i
    return dict(n=np.int64(n), t=np.int64(t),
                coeffs=_u8([c.to_bytes(32, "big") for pl in polys for c in pl.coeff], n, M, 32),
                commits=_u8([bls.g1_compress(c) for cm in commits for c in cm], n, M, 48),
                complete=np.array(complete, dtype=np.uint8),
                pk_commit=_u8([bls.g1_compress(c) for c in pk_commit], t + 1, 48),
                pk_shares=_u8([bls.g1_compress(c) for c in pk_shares], n, 48),
                sk_all=_u8([s.to_bytes(32, "big") for s in sk_all], n, 32),
                bad_g1=_u8([bls.g1_compress(off_subgroup_g1(7070 + n))], 48))


def pack_era(n, t, me, sk_nodes, pk_nodes, msgs, ack_r, outcomes, acks_out, extra):
    """Flatten one node's era into arrays (read back by tests/skg_fixture.py load_era)."""
    M = bivar.n_coeffs(t)
    kind, sender, ref = [], [], []
    commits, part_cts, ack_prop, ack_start, ack_cts = [], [], [], [0], []
    for k, s, body in msgs:
        kind.append(k)
        sender.append(-1 if s is None else s)
        if k == skg.PART:
            ref.append(len(commits))
            commits.append(body[0])
            part_cts.append(body[1])
        else:
            ref.append(len(ack_prop))
            ack_prop.append(body[0])
            ack_cts.extend(body[1])
            ack_start.append(len(ack_cts))
    P = len(commits)
    flat_p = [c for rows in part_cts for c in rows]
    zero_ct = (bytes(48), bytes(32), bytes(96))
    exp = [acks_out[k][1] if k in acks_out else [zero_ct] * n for k, m in enumerate(msgs) if m[0] == skg.PART]
    r_rows = [ack_r.get(k, [0] * n) for k, m in enumerate(msgs) if m[0] == skg.PART]
    d = dict(n=np.int64(n), t=np.int64(t), me=np.int64(me),
             sk_nodes=_u8([s.to_bytes(32, "big") for s in sk_nodes], n, 32),
             pk_nodes=_u8([bls.g1_compress(p) for p in pk_nodes], n, 48),
             msg_kind=np.array(kind, dtype=np.uint8), msg_sender=np.array(sender, dtype=np.int64),
             msg_ref=np.array(ref, dtype=np.int64),
             part_commit=_u8([c for cm in commits for c in cm], P, M, 48),
             part_u=_u8([c[0] for c in flat_p], P, n, 48), part_w=_u8([c[2] for c in flat_p], P, n, 96),
             part_v=_blob([c[1] for c in flat_p])[0], part_off=_blob([c[1] for c in flat_p])[1],
             ack_proposer=np.array(ack_prop, dtype=np.int64), ack_start=np.array(ack_start, dtype=np.int64),
             ack_u=_u8([c[0] for c in ack_cts], len(ack_cts), 48), ack_w=_u8([c[2] for c in ack_cts], len(ack_cts), 96),
             ack_v=_blob([c[1] for c in ack_cts])[0], ack_off=_blob([c[1] for c in ack_cts])[1],
             ack_r=_u8([x.to_bytes(32, "big") for row in r_rows for x in row], P, n, 32),
             outcome=np.array(outcomes, dtype=np.uint8),
             exp_ack_u=_u8([c[0] for a in exp for c in a], P, n, 48),
             exp_ack_v=_u8([c[1] for a in exp for c in a], P, n, 32),
             exp_ack_w=_u8([c[2] for a in exp for c in a], P, n, 96))
    d.update(extra)
    return d


def make_era(n: int, me: int, faults: bool):
    """One node's view (`me`) of an era of n nodes: every node deals a Part; the Acks are what honest
    nodes answer (value f_q(sender + 1, i + 1) to node i), with the issue's faults in n = 7."""
    t = (n - 1) // 3
    M = bivar.n_coeffs(t)
    rng = ChaChaRng04([0x68626278, 0x65726100 + n])
    sk_nodes = [tc.fr_rand(rng) for _ in range(n)]
    pk_nodes = [bls.g1_mul(bls.G1_GEN, s) for s in sk_nodes]
    polys = [bivar.BivarPoly(t, [tc.fr_rand(rng) for _ in range(M)]) for _ in range(n)]
    model = skg.SyncKeyGenModel(me, sk_nodes[me], pk_nodes, t)
    dealer_r = {q: [tc.fr_rand(rng) for _ in range(n)] for q in range(n)}
    parts = {q: model.dealer_part(polys[q], dealer_r[q]) for q in range(n)}

    def enc(pk, data):
        return skg.ct_to_bytes(tc.encrypt(pk, data, tc.fr_rand(rng)))

    def honest_ack(q, s):
        return (q, [enc(pk_nodes[i], polys[q].evaluate(s + 1, i + 1).to_bytes(32, "big")) for i in range(n)])

    msgs = []
    ack_senders = {q: list(range(n)) for q in range(n)}
    if faults:
        assert n == 7 and me == 3
        other = bivar.BivarPoly(t, [tc.fr_rand(rng) for _ in range(M)])
        # part 2: our row is a row of another polynomial (commitment mismatch -> InvalidPartMessage)
        rows = list(parts[2][1])
        rows[me] = enc(pk_nodes[me], skg.encode_row(skg.bivar_row(other, me + 1)))
        parts[2] = (parts[2][0], rows)
        # part 4: a flipped V byte in our row ciphertext (decrypt fails: no outcome, no fault)
        rows = list(parts[4][1])
        u, v, w = rows[me]
        rows[me] = (u, bytes([v[0] ^ 1]) + v[1:], w)
        parts[4] = (parts[4][0], rows)
        # part 5: our row plaintext is 95 bytes (does not deserialise -> InvalidPartMessage)
        rows = list(parts[5][1])
        rows[me] = enc(pk_nodes[me], skg.encode_row(skg.bivar_row(polys[5], me + 1))[:95])
        parts[5] = (parts[5][0], rows)
        ack_senders = {0: list(range(n)), 1: [0, 1, 2, 3], 2: [0, 5], 3: list(range(n)), 4: [6], 5: [],
                       6: list(range(n))}  # part 1 stays at exactly 2t acks
    for q in range(n):
        msgs.append((skg.PART, q, parts[q]))
    if faults:
        msgs.append((skg.PART, 0, parts[0]))     # duplicate part: no outcome
        msgs.append((skg.PART, None, parts[1]))  # unknown sender: no outcome
    for q in range(n):
        for s in ack_senders[q]:
            ack = honest_ack(q, s)
            if faults and (q, s) == (0, 1):    # wrong value, among part 0's first 2t + 1 acks
                vals = list(ack[1])
                vals[me] = enc(pk_nodes[me], ((polys[q].evaluate(s + 1, me + 1) + 1) % bls.R).to_bytes(32, "big"))
                ack = (q, vals)
            if faults and (q, s) == (3, 5):    # tampered W: value decryption fails
                vals = list(ack[1])
                vals[me] = (vals[me][0], vals[me][1], vals[(me + 1) % n][2])
                ack = (q, vals)
            if faults and (q, s) == (3, 6):    # a value >= r does not deserialise
                vals = list(ack[1])
                vals[me] = enc(pk_nodes[me], (bls.R + 5).to_bytes(32, "big"))
                ack = (q, vals)
            if faults and (q, s) == (6, 4):    # n - 1 values first: wrong node count, sender not counted
                msgs.append((skg.ACK, s, (q, ack[1][:n - 1])))
            msgs.append((skg.ACK, s, ack))
            if faults and (q, s) == (6, 2):    # duplicate ack
                msgs.append((skg.ACK, s, ack))
    if faults:
        msgs.append((skg.ACK, 2, (9, honest_ack(0, 2)[1])))   # unknown proposer
        msgs.append((skg.ACK, None, honest_ack(0, 2)))        # unknown sender: nothing logged
    ack_r = {k: [tc.fr_rand(rng) for _ in range(n)] for k, m in enumerate(msgs) if m[0] == skg.PART}
    outcomes, acks_out = model.run(msgs, ack_r)
    pk_commit, sk_me = model.generate()
    complete = [1 if model.is_complete(q) else 0 for q in range(n)]
    sk_all = [sum(polys[q].evaluate(i + 1, 0) for q in range(n) if complete[q]) % bls.R for i in range(n)]
    assert sk_me == sk_all[me]
    pks = tc.PublicKeySet(pk_commit)
    pk_shares = [pks.public_key_share(i) for i in range(n)]
    assert all(pk_shares[i] == bls.g1_mul(bls.G1_GEN, sk_all[i]) for i in range(n))
    extra = dict(complete=np.array(complete, dtype=np.uint8), is_ready=np.int64(model.is_ready()),
                 pk_commit=_u8([bls.g1_compress(c) for c in pk_commit], t + 1, 48),
                 sk_me=_u8([sk_me.to_bytes(32, "big")], 32),
                 pk_shares=_u8([bls.g1_compress(c) for c in pk_shares], n, 48),
                 sk_all=_u8([s.to_bytes(32, "big") for s in sk_all], n, 32),
                 dealer_coeffs=_u8([c.to_bytes(32, "big") for c in polys[me].coeff], M, 32),
                 dealer_r=_u8([x.to_bytes(32, "big") for x in dealer_r[me]], n, 32),
                 dealer_msg=np.int64(me))  # message index of our own (unmodified) Part
    print(f"n={n}: outcomes", outcomes, "complete", complete)
    return pack_era(n, t, me, sk_nodes, pk_nodes, msgs, ack_r, outcomes, acks_out, extra)


def main():
    if "--era" in sys.argv:
        for name, d in (("skg_n4", make_era(4, 1, False)), ("skg_n7", make_era(7, 3, True))):
            path = os.path.join(HERE, f"{name}.npz")
            np.savez_compressed(path, **d)
            print(name, os.path.getsize(path), "bytes")
        return
    for name, d in (("skg_gen_n4", make_gen(4)), ("skg_gen_n7", make_gen(7)), ("skg_batch65", make_batch65())):
        path = os.path.join(HERE, f"{name}.npz")
        np.savez_compressed(path, **d)
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
