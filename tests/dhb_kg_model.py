"""CPU restatement of the signature layer Dynamic HoneyBadger puts in front of SyncKeyGen (reference
src/dynamic_honey_badger/dynamic_honey_badger.rs:254-272 process_output, :395-410 verify_signature)
over tests/skg_model.py and the oracle.  One committed item at a time, as the reference runs them:

    epoch < start_epoch                     -> OBSOLETE, skipped
    !verify_signature(s_id, sig, kg_msg)    -> BAD_SIGNATURE, InvalidKeyGenMessageSignature against the
                                               proposer of the batch that carried the message
    otherwise                               -> handle_part / handle_ack (SyncKeyGenModel)

verify_signature takes the key of a validator or of the joining candidate; anybody else has no key
(pk_opt is None) and the check is false.  A signature that does not deserialise as a G2 point counts
as false here, as the engine's status byte does (the reference would not deserialise the message).

``ser_kg_msg`` is the byte string the fixtures sign: a fixed concatenation of the message's fields.
bincode framing is not pinned (DESIGN.md 4.5 leaves it to the caller, as for the plaintexts).
"""
from oracle import bls12_381 as bls
from oracle import threshold as tc

from skg_model import PART

OBSOLETE, BAD_SIGNATURE = 16, 17
FAULT_INVALID_SIGNATURE = "InvalidKeyGenMessageSignature"


def ser_kg_msg(kind, body) -> bytes:
    """Part: b"P" | commitment points | rows (u | v | w each); Ack: b"A" | proposer u64 LE | values."""
    if kind == PART:
        commit, rows = body
        return b"P" + b"".join(bytes(c) for c in commit) + b"".join(u + v + w for u, v, w in rows)
    proposer, values = body
    return b"A" + int(proposer).to_bytes(8, "little") + b"".join(u + v + w for u, v, w in values)


class DhbKeyGenModel:
    def __init__(self, skg, pub_keys, candidate=None, start_epoch=0, variant=tc.DEFAULT_DIGEST):
        self.skg = skg  # a SyncKeyGenModel
        self.pub_keys = list(pub_keys)  # the validators' G1 points by index
        self.candidate = candidate  # (index, G1 point) or None
        self.start_epoch = start_epoch
        self.variant = variant
        self.faults = []  # (batch proposer, fault kind)

    def public_key(self, sender_idx):
        if sender_idx is None:
            return None
        if 0 <= sender_idx < len(self.pub_keys):
            return self.pub_keys[sender_idx]
        if self.candidate is not None and sender_idx == self.candidate[0]:
            return self.candidate[1]
        return None

    def verify_signature(self, sender_idx, sig96: bytes, ser: bytes) -> bool:
        pk = self.public_key(sender_idx)
        if pk is None:
            return False
        try:
            sig = bls.g2_decompress(bytes(sig96))
        except ValueError:
            return False
        return tc.verify_sig(pk, sig, ser, self.variant)

    def run(self, items, ack_randomness):
        """items: (batch_proposer, epoch, sender_idx, kind, body, ser, sig96) -> (outcomes, {index: Ack})."""
        out, acks = [], {}
        for k, (proposer, epoch, sender, kind, body, ser, sig) in enumerate(items):
            if epoch < self.start_epoch:
                out.append(OBSOLETE)
                continue
            if not self.verify_signature(sender, sig, ser):
                self.faults.append((proposer, FAULT_INVALID_SIGNATURE))
                out.append(BAD_SIGNATURE)
                continue
            if kind == PART:
                o, ack = self.skg.handle_part(sender, body, ack_randomness.get(k))
                if ack is not None:
                    acks[k] = ack
            else:
                o = self.skg.handle_ack(sender, body)
            out.append(o)
        return out, acks
