"""The signature layer Dynamic HoneyBadger wraps around SyncKeyGen (reference
src/dynamic_honey_badger/dynamic_honey_badger.rs), batched through the engine.

``SignedKeyGenReplay`` stands where ``process_output`` (:243-272) stands: it takes the committed
``SignedKeyGenMsg`` items of one or more batches in order, skips the obsolete ones (``epoch <
start_epoch``), checks ``PublicKey::verify(sig, ser)`` of all the others in ONE
``hbx_verify_sigs_keyed`` call -- the key is the sender's validator key, or the joining candidate's
(``verify_signature`` :395-410) -- logs ``InvalidKeyGenMessageSignature`` against the proposer of the
batch that carried a message whose check is not VALID, and hands the survivors, in order, to ONE
``KeyGenReplay.handle_messages`` call (``handle_part`` / ``handle_ack``).

An item is ``(batch_proposer, epoch, sender_idx | None, kind, body, ser_bytes, sig96)``: ``kind`` and
``body`` as ``KeyGenReplay`` takes them, ``sender_idx`` the validator's index, ``candidate[0]`` for the
candidate, or None for anybody else (``pk_opt`` is None: the check fails without a pairing).
``ser_bytes`` is the caller's serialisation of the message: bincode framing is not pinned here, as
it is not for the plaintexts.

``sign`` is ``send_transaction``'s ``SecretKey::sign`` (:363) for the node's own Part and Acks.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import hbx
from .sync_key_gen import KeyGenReplay

# per-item outcomes beyond KeyGenReplay's OUT_* (sync_key_gen.py: 0..4)
OBSOLETE = 16       # epoch < start_epoch: skipped, nothing logged
BAD_SIGNATURE = 17  # verify_signature returned false: FaultKind::InvalidKeyGenMessageSignature

FAULT_INVALID_SIGNATURE = "InvalidKeyGenMessageSignature"


class SignedKeyGenReplay:
    def __init__(self, key_gen: KeyGenReplay, pub_keys: np.ndarray, candidate: Optional[Tuple[int, bytes]] = None,
                 start_epoch: int = 0):
        self.key_gen = key_gen
        self.ctx = key_gen.ctx
        pub_keys = np.ascontiguousarray(pub_keys, dtype=np.uint8)
        if pub_keys.ndim != 2 or pub_keys.shape[1] != 48 or pub_keys.shape[0] == 0:
            raise ValueError("SignedKeyGenReplay: pub_keys must be uint8[n, 48] with n > 0")
        self.n_validators = pub_keys.shape[0]
        # the key table: the validators' keys, then the candidate's
        self.candidate_idx = None
        if candidate is not None:
            idx, key = candidate
            key = np.frombuffer(bytes(key), dtype=np.uint8)
            if key.size != 48:
                raise ValueError("SignedKeyGenReplay: the candidate's key must be 48 bytes")
            if idx is None or 0 <= idx < self.n_validators:
                raise ValueError("SignedKeyGenReplay: the candidate's index must differ from every validator's")
            self.candidate_idx = idx
            pub_keys = np.concatenate([pub_keys, key.reshape(1, 48)])
        self.key_table = pub_keys
        self.start_epoch = start_epoch
        self.faults: List[Tuple[object, str]] = []  # (batch proposer, fault kind), in order

    def _key_slot(self, sender_idx) -> int:
        if sender_idx is None:
            return hbx.NO_KEY
        if self.candidate_idx is not None and sender_idx == self.candidate_idx:
            return self.n_validators
        return sender_idx if 0 <= sender_idx < self.n_validators else hbx.NO_KEY

    def handle_batch(self, items: Sequence[tuple], ack_randomness=None):
        """-> (outcomes int[len(items)], acks {item index: Ack}); faults accumulate in ``self.faults``.
        ack_randomness is keyed by item index."""
        out = [OBSOLETE] * len(items)
        live = [k for k, it in enumerate(items) if it[1] >= self.start_epoch]
        if not live:
            return out, {}
        key_idx = np.array([self._key_slot(items[k][2]) for k in live], dtype=np.uint32)
        sigs = np.frombuffer(b"".join(bytes(items[k][6]) for k in live), dtype=np.uint8)
        if sigs.size != 96 * len(live):
            raise ValueError("SignedKeyGenReplay: every signature is 96 bytes")
        status, _ = self.ctx.verify_sigs_keyed(self.key_table, key_idx, [bytes(items[k][5]) for k in live],
                                               sigs.reshape(-1, 96))
        good = []
        for k, st in zip(live, status):
            if st == hbx.SHARE_VALID:
                good.append(k)
            else:
                out[k] = BAD_SIGNATURE
                self.faults.append((items[k][0], FAULT_INVALID_SIGNATURE))
        if not good:
            return out, {}
        # the survivors go down with the sender index the caller gave (whether the candidate is a
        # node of the era being generated is the KeyGenReplay's business); randomness re-keyed
        rnd = None if ack_randomness is None else {a: ack_randomness[k] for a, k in enumerate(good)
                                                   if k in ack_randomness}
        res, acks = self.key_gen.handle_messages([(items[k][3], items[k][2], items[k][4]) for k in good], rnd)
        for a, k in enumerate(good):
            out[k] = res[a]
        return out, {good[a]: ack for a, ack in acks.items()}

    def sign(self, ser_list: Sequence[bytes]) -> np.ndarray:
        """The node's signatures over its own serialised Part and Acks: uint8[len(ser_list), 96]."""
        return self.ctx.sign_msgs(self.key_gen.sec_key, [bytes(s) for s in ser_list])

    def generate(self):
        return self.key_gen.generate()
