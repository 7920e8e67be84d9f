"""CPU restatement (TEST INFRASTRUCTURE ONLY) of the reference's SyncKeyGen (src/sync_key_gen.rs)
on the oracle (oracle/bivar.py, oracle/threshold.py, oracle/bls12_381.py), message by message.

Same message shapes and outcome codes as hbbft_amd/sync_key_gen.py, with points as compressed bytes:
Part = (commit: list of 48-byte strings in coeff_pos order, rows: list of (u48, v, w96));
Ack = (proposer_idx, values: list of (u48, v, w96)).  Plaintexts use the raw-scalar framing
(a row is (t + 1) x 32 B big-endian canonical Fr, a value 32 B).
"""
from __future__ import annotations

from oracle import bivar
from oracle import bls12_381 as bls
from oracle import threshold as tc

R = bls.R
PART, ACK = 0, 1
OUT_NONE, OUT_ACK, OUT_INVALID_PART, OUT_OK, OUT_INVALID_ACK = 0, 1, 2, 3, 4


def ct_to_bytes(ct):
    return (bls.g1_compress(ct[0]), bytes(ct[1]), bls.g2_compress(ct[2]))


def secret_key_decrypt(sk: int, ct_bytes, variant: str = tc.DEFAULT_DIGEST):
    """SecretKey::decrypt: None unless the ciphertext deserialises and Ciphertext::verify holds,
    else V xor hash_bytes(sk U, |V|)."""
    u48, v, w96 = ct_bytes
    try:
        u = bls.g1_decompress(u48)
        w = bls.g2_decompress(w96)
    except Exception:
        return None
    if not tc.ciphertext_verify((u, v, w), variant):
        return None
    return tc.xor_bytes(tc.hash_bytes(bls.g1_mul(u, sk), len(v), variant), v)


def encode_row(coeffs):
    return b"".join(int(c).to_bytes(32, "big") for c in coeffs)


def decode_row(data: bytes, t: int):
    if len(data) != 32 * (t + 1):
        return None
    out = [int.from_bytes(data[32 * j:32 * j + 32], "big") for j in range(t + 1)]
    return out if all(c < R for c in out) else None


def decode_val(data: bytes):
    if len(data) != 32:
        return None
    v = int.from_bytes(data, "big")
    return v if v < R else None


def poly_eval(coeffs, x: int) -> int:
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def bivar_row(poly: bivar.BivarPoly, x: int):
    """BivarPoly::row(x): coefficient j is sum_i a_ij x^i."""
    return [sum(poly.a(i, j) * pow(x, i, R) for i in range(poly.t + 1)) % R for j in range(poly.t + 1)]


def lagrange0(points) -> int:
    """Poly::interpolate(points).evaluate(0) over (x, value) pairs."""
    acc = 0
    for k, (xk, vk) in enumerate(points):
        num = den = 1
        for m, (xm, _) in enumerate(points):
            if m != k:
                num = num * xm % R
                den = den * (xm - xk) % R
        acc += vk * num * pow(den, -1, R)
    return acc % R


class _PartState:
    def __init__(self, commit_pts):
        self.commit = commit_pts
        self.acks = set()
        self.values = {}


class SyncKeyGenModel:
    def __init__(self, our_idx, sec_key: int, pub_keys, threshold: int, variant: str = tc.DEFAULT_DIGEST):
        self.our_idx = our_idx  # None: observer
        self.sec_key = sec_key
        self.pub_keys = list(pub_keys)  # G1 points by node index
        self.n = len(self.pub_keys)
        self.t = threshold
        self.variant = variant
        self.parts = {}

    def dealer_part(self, poly: bivar.BivarPoly, r_list):
        """SyncKeyGen::new (:290-298) with the randomness passed in."""
        commit = [bls.g1_compress(c) for c in poly.commitment()]
        rows = [ct_to_bytes(tc.encrypt(pk, encode_row(bivar_row(poly, i + 1)), r_list[i], self.variant))
                for i, pk in enumerate(self.pub_keys)]
        return commit, rows

    def handle_part(self, sender_idx, part, r_list):
        """(:307-349) -> (outcome, Ack or None)."""
        commit, rows = part
        if sender_idx is None or not 0 <= sender_idx < self.n:
            return OUT_NONE, None
        if sender_idx in self.parts:
            return OUT_NONE, None
        pts = [bls.g1_decompress(c) for c in commit]
        self.parts[sender_idx] = _PartState(pts)
        if self.our_idx is None or self.our_idx >= len(rows):
            return OUT_NONE, None
        commit_row = bivar.row(pts, self.t, self.our_idx + 1)
        ser_row = secret_key_decrypt(self.sec_key, rows[self.our_idx], self.variant)
        if ser_row is None:
            return OUT_NONE, None
        row = decode_row(ser_row, self.t)
        if row is None:
            return OUT_INVALID_PART, None
        if [bls.g1_mul(bls.G1_GEN, c) for c in row] != commit_row:
            return OUT_INVALID_PART, None
        values = [ct_to_bytes(tc.encrypt(pk, poly_eval(row, idx + 1).to_bytes(32, "big"), r_list[idx], self.variant))
                  for idx, pk in enumerate(self.pub_keys)]
        return OUT_ACK, (sender_idx, values)

    def handle_ack(self, sender_idx, ack):
        """(:355-364, :423-454) -> OUT_OK or OUT_INVALID_ACK."""
        if sender_idx is None or not 0 <= sender_idx < self.n:
            return OUT_OK
        proposer_idx, values = ack
        if len(values) != self.n:
            return OUT_INVALID_ACK  # wrong node count
        part = self.parts.get(proposer_idx)
        if part is None:
            return OUT_INVALID_ACK  # sender does not exist
        if sender_idx in part.acks:
            return OUT_INVALID_ACK  # duplicate ack
        part.acks.add(sender_idx)
        if self.our_idx is None:
            return OUT_OK
        ser_val = secret_key_decrypt(self.sec_key, values[self.our_idx], self.variant)
        if ser_val is None:
            return OUT_INVALID_ACK  # value decryption failed
        val = decode_val(ser_val)
        if val is None:
            return OUT_INVALID_ACK  # deserialization failed
        if bivar.evaluate(part.commit, self.t, self.our_idx + 1, sender_idx + 1) != bls.g1_mul(bls.G1_GEN, val):
            return OUT_INVALID_ACK  # wrong value
        part.values[sender_idx + 1] = val
        return OUT_OK

    def is_complete(self, proposer_idx) -> bool:
        part = self.parts.get(proposer_idx)
        return part is not None and len(part.acks) > 2 * self.t

    def count_complete(self) -> int:
        return sum(1 for q in self.parts if self.is_complete(q))

    def is_ready(self) -> bool:
        return self.count_complete() > self.t

    def generate(self):
        """(:396-409) -> (pk_commit points, sk share int or None)."""
        pk_commit = [None] * (self.t + 1)
        sk = None if self.our_idx is None else 0
        for q in sorted(self.parts):
            if not self.is_complete(q):
                continue
            row0 = bivar.row(self.parts[q].commit, self.t, 0)
            pk_commit = [bls.g1_add(a, b) for a, b in zip(pk_commit, row0)]
            if sk is not None:
                sk = (sk + lagrange0(sorted(self.parts[q].values.items())[:self.t + 1])) % R
        return pk_commit, sk

    def run(self, msgs, ack_randomness):
        """Replay (kind, sender, body) messages -> (outcomes, {message index: Ack})."""
        out, acks = [], {}
        for k, (kind, sender, body) in enumerate(msgs):
            if kind == PART:
                o, ack = self.handle_part(sender, body, ack_randomness.get(k))
                if ack is not None:
                    acks[k] = ack
            else:
                o = self.handle_ack(sender, body)
            out.append(o)
        return out, acks
