"""One node's view of a SyncKeyGen era (reference src/sync_key_gen.rs), batched through the engine.

``KeyGenReplay`` takes the ``Part`` and ``Ack`` messages a node received, in delivery order, and
reproduces the reference's outcome for each: the structural checks (unknown sender, duplicate part,
node count, unknown proposer, duplicate ack) replay on the host in order, and everything arithmetic
goes through the batch calls -- one ``hbx_sk_decrypt`` for every row and value addressed to this
node, ``hbx_bivar_rows`` + ``hbx_public_keys`` for the row commitments, ``hbx_fr_poly_eval`` +
``hbx_encrypt_to`` for the Acks this node answers with, ``hbx_bivar_check_acks`` for the values,
``hbx_keygen_generate`` / ``hbx_pk_shares_from_commit`` for the new keys.

Messages:  Part = (commit uint8[(t+1)(t+2)/2, 48], rows = n ciphertexts (u48, v, w96));
           Ack  = (proposer_idx, values = ciphertexts (u48, v, w96));
           a message is (PART | ACK, sender_idx, Part | Ack), sender_idx None for a sender that is not
           a node of this era (``node_index`` returned None).

Plaintext framing goes through a codec object; ``RawCodec`` (the default) is the raw-scalar form of
DESIGN.md 4.5.  A bincode codec can replace it without touching the engine.

``ct_check`` chooses how the replay's ``sk_decrypt`` runs Ciphertext::verify (``hbx.CT_CHECK_WIDE`` /
``hbx.CT_CHECK_PAIR``, set on the context before each such call); None leaves the context's mode alone.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np

from . import hbx

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

PART, ACK = 0, 1
# per-message outcomes
OUT_NONE = 0          # handle_part returned None (unknown sender, duplicate part, observer, decrypt failed)
OUT_ACK = 1           # PartOutcome::Valid(Ack)
OUT_INVALID_PART = 2  # PartOutcome::Invalid: FaultKind::InvalidPartMessage
OUT_OK = 3            # handle_ack: empty fault log
OUT_INVALID_ACK = 4   # handle_ack: FaultKind::InvalidAckMessage


class RawCodec:
    """Row = (t + 1) x 32 B big-endian canonical Fr, value = 32 B; anything else does not deserialise."""

    @staticmethod
    def encode_row(coeffs: Sequence[int]) -> bytes:
        return b"".join(int(c).to_bytes(32, "big") for c in coeffs)

    @staticmethod
    def decode_row(data: bytes, t: int) -> Optional[List[int]]:
        if len(data) != 32 * (t + 1):
            return None
        out = [int.from_bytes(data[32 * j:32 * j + 32], "big") for j in range(t + 1)]
        return out if all(c < R for c in out) else None

    @staticmethod
    def encode_val(v: int) -> bytes:
        return int(v).to_bytes(32, "big")

    @staticmethod
    def decode_val(data: bytes) -> Optional[int]:
        if len(data) != 32:
            return None
        v = int.from_bytes(data, "big")
        return v if v < R else None


def _be32(vals, *shape) -> np.ndarray:
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), dtype=np.uint8).reshape(*shape, 32)


class _PartState:
    def __init__(self, commit: np.ndarray):
        self.commit = commit
        self.acks = set()
        self.values: Dict[int, int] = {}  # sender_idx + 1 -> verified value

    def is_complete(self, t: int) -> bool:
        return len(self.acks) > 2 * t


class KeyGenReplay:
    def __init__(self, ctx: "hbx.Context", our_idx: Optional[int], sec_key: bytes, pub_keys: np.ndarray,
                 threshold: int, codec=None, ct_check: Optional[int] = None):
        if ct_check is not None and ct_check not in (hbx.CT_CHECK_WIDE, hbx.CT_CHECK_PAIR):
            raise ValueError(f"KeyGenReplay: ct_check None, CT_CHECK_WIDE (0) or CT_CHECK_PAIR (1), not {ct_check!r}")
        self.ctx = ctx
        self.ct_check = ct_check
        self.our_idx = our_idx  # None: an observer
        self.sec_key = bytes(sec_key)
        self.pub_keys = np.ascontiguousarray(pub_keys, dtype=np.uint8)
        self.n = self.pub_keys.shape[0]
        self.t = threshold
        self.codec = codec or RawCodec()
        self.parts: Dict[int, _PartState] = {}

    # -- SyncKeyGen::new (:290-298) ---------------------------------------------------------------
    def dealer_part(self, coeffs32: np.ndarray, r32: np.ndarray):
        """This node's own Part from its polynomial (coeff_pos order) and encryption randomness."""
        coeffs32 = np.ascontiguousarray(coeffs32, dtype=np.uint8)
        commit = self.ctx.public_keys(coeffs32)
        rows = self.ctx.bivar_poly_rows(coeffs32, self.t, self.n)
        msgs = [self.codec.encode_row([int.from_bytes(c.tobytes(), "big") for c in rows[i]]) for i in range(self.n)]
        return commit, self.ctx.encrypt_to(self.pub_keys, msgs, r32)

    # -- handle_part / handle_ack over a batch of messages in delivery order -----------------------
    def handle_messages(self, msgs, ack_randomness: Optional[Dict[int, np.ndarray]] = None):
        """Returns (outcomes int[len(msgs)], acks {message index: Ack} for every OUT_ACK).
        ack_randomness[k]: uint8[n, 32] for the Ack answering the Part at message index k."""
        n, t, me = self.n, self.t, self.our_idx
        out = [OUT_NONE] * len(msgs)
        part_jobs, ack_jobs = [], []  # (message index, ciphertext[, ...])
        for k, (kind, sender, body) in enumerate(msgs):
            known = sender is not None and 0 <= sender < n
            if kind == PART:
                commit, rows = body
                if not known or sender in self.parts:
                    continue
                self.parts[sender] = _PartState(np.ascontiguousarray(commit, dtype=np.uint8))
                if me is not None and me < len(rows):
                    part_jobs.append((k, sender, rows[me]))
            else:
                proposer, values = body
                if not known:
                    out[k] = OUT_OK  # node_index is None: nothing logged
                    continue
                out[k] = OUT_INVALID_ACK
                if len(values) != n or proposer not in self.parts:
                    continue  # "wrong node count" / "sender does not exist"
                part = self.parts[proposer]
                if sender in part.acks:
                    continue  # "duplicate ack"
                part.acks.add(sender)  # counted from here on, valid or not
                if me is None:
                    out[k] = OUT_OK
                else:
                    ack_jobs.append((k, sender, proposer, values[me]))
        if not part_jobs and not ack_jobs:
            return out, {}
        if self.ct_check is not None:
            self.ctx.set_ct_check(self.ct_check)
        plains, st = self.ctx.sk_decrypt(self.sec_key, [j[2] for j in part_jobs] + [j[3] for j in ack_jobs])
        acks = self._finish_parts(part_jobs, plains, st, out, ack_randomness or {})
        self._finish_acks(ack_jobs, plains[len(part_jobs):], st[len(part_jobs):], out)
        return out, acks

    def _finish_parts(self, jobs, plains, st, out, randomness):
        n, t, me = self.n, self.t, self.our_idx
        good = []  # (message index, sender, row coefficients)
        for (k, sender, _), pt, s in zip(jobs, plains, st):
            if s != hbx.CT_VALID:
                continue  # the `?` at :326: no outcome, no fault
            row = self.codec.decode_row(pt, t)
            out[k] = OUT_INVALID_PART
            if row is not None:
                good.append((k, sender, row))
        if not good:
            return {}
        commits = np.stack([self.parts[s].commit for _, s, _ in good])
        want, cst = self.ctx.bivar_rows(commits, t, me + 1)
        rows32 = _be32([c for _, _, row in good for c in row], len(good), t + 1)
        got = self.ctx.public_keys(rows32.reshape(-1, 32)).reshape(len(good), t + 1, 48)
        valid = [i for i in range(len(good)) if cst[i] == hbx.SHARE_VALID and (got[i] == want[i]).all()]
        if not valid:
            return {}
        vals = self.ctx.fr_poly_eval(rows32[valid], n)  # [part][idx][32]
        r32 = np.concatenate([np.ascontiguousarray(randomness[good[i][0]], dtype=np.uint8).reshape(n, 32) for i in valid])
        enc = [self.codec.encode_val(int.from_bytes(vals[a, i].tobytes(), "big")) for a in range(len(valid)) for i in range(n)]
        cts = self.ctx.encrypt_to(np.tile(self.pub_keys, (len(valid), 1)), enc, r32)
        acks = {}
        for a, i in enumerate(valid):
            k, sender, _ = good[i]
            out[k] = OUT_ACK
            acks[k] = (sender, cts[a * n:(a + 1) * n])
        return acks

    def _finish_acks(self, jobs, plains, st, out):
        t, me = self.t, self.our_idx
        checks = []  # (message index, sender, proposer, value)
        for (k, sender, proposer, _), pt, s in zip(jobs, plains, st):
            if s != hbx.CT_VALID:
                continue  # "value decryption failed"
            val = self.codec.decode_val(pt)
            if val is not None:
                checks.append((k, sender, proposer, val))
        if not checks:
            return
        order = sorted(self.parts)
        commits = np.stack([self.parts[q].commit for q in order])
        ok = self.ctx.bivar_check_acks(commits, t, me + 1, [order.index(c[2]) for c in checks],
                                       [c[1] + 1 for c in checks], _be32([c[3] for c in checks], len(checks)))
        for (k, sender, proposer, val), v in zip(checks, ok):
            if v == hbx.SHARE_VALID:  # otherwise "wrong value"
                out[k] = OUT_OK
                self.parts[proposer].values[sender + 1] = val

    # -- state queries (:366-385) ----------------------------------------------------------------
    def is_node_ready(self, proposer_idx: int) -> bool:
        part = self.parts.get(proposer_idx)
        return part is not None and part.is_complete(self.t)

    def count_complete(self) -> int:
        return sum(1 for p in self.parts.values() if p.is_complete(self.t))

    def is_ready(self) -> bool:
        return self.count_complete() > self.t

    # -- generate (:396-409) ---------------------------------------------------------------------
    def generate(self):
        """(pk_commit uint8[t + 1, 48], sk share bytes or None for an observer)."""
        t = self.t
        order = [q for q in sorted(self.parts) if self.parts[q].is_complete(t)]
        if not order:
            ident = np.zeros((t + 1, 48), dtype=np.uint8)
            ident[:, 0] = 0xC0  # Poly::zero().commitment()
            return ident, (None if self.our_idx is None else bytes(32))
        commits = np.stack([self.parts[q].commit for q in order])
        complete = np.ones(len(order), dtype=np.uint8)
        if self.our_idx is None:
            pkc, _, _ = self.ctx.keygen_generate(commits, t, complete)
            return pkc, None
        cnt = np.zeros(len(order), dtype=np.uint32)
        ys = np.zeros((len(order), t + 1), dtype=np.uint64)
        vals = [0] * (len(order) * (t + 1))
        for a, q in enumerate(order):
            first = sorted(self.parts[q].values.items())[:t + 1]  # values.iter().take(threshold + 1)
            cnt[a] = len(first)
            for b, (y, v) in enumerate(first):
                ys[a, b] = y
                vals[a * (t + 1) + b] = v
        pkc, sk, _ = self.ctx.keygen_generate(commits, t, complete, cnt, ys, _be32(vals, len(order), t + 1))
        return pkc, sk

    def install(self, ctx: Optional["hbx.Context"] = None):
        """into_network_info (:416-420): the new key set and this node's share into a context."""
        ctx = ctx or self.ctx
        pkc, sk = self.generate()
        pk_shares = self.ctx.pk_shares_from_commit(pkc, self.n)
        st = ctx.set_pk_shares([row.tobytes() for row in pk_shares])
        if (st != 0).any():
            raise ValueError("install: a generated public key share is the identity")
        if sk is not None:
            ctx.set_own_share(self.our_idx, sk)
        return pkc, sk, pk_shares
