"""Batched replay of HoneyBadger's threshold-decryption sub-path for one node-epoch.

The reference handles decryption shares one message at a time (``src/honey_badger/
honey_badger.rs``: ``handle_decryption_share_message`` :186-217, ``send_decryption_shares``
:351-391, ``verify_pending_decryption_shares`` :422-444, ``try_decrypt_proposer_contribution``
:315-349).  This host-side driver gives the same FaultLog, in the same order, and the same Batch,
with ONE engine pass over the whole epoch instead of one pairing check per message:

1. the CommonSubset output (the accepted ciphertexts) goes through ``hbx_prepare_ciphertexts``
   (hash_g1_g2 hoisted per proposer, ``Ciphertext::verify``) -> one ``HBX_CT_*`` status each;
2. every DecryptionShare message of the epoch, before or after the ciphertexts, goes into one
   ``hbx_verify_dec_shares`` call (a second call per extra message of the same (proposer, sender)
   pair, which only a Byzantine sender produces) -> one ``HBX_SHARE_*`` status per message;
3. the messages are then replayed in arrival order through the reference's control flow, with the
   statuses standing in for the pairing checks: verification is deterministic, so verifying a
   share early changes no result, only when the work is done;
4. the plaintexts come from ``hbx_combine_decrypt`` (first t valid shares by index; any t valid
   shares interpolate to the same point, so the bytes equal the reference's, whichever t shares
   it had when it crossed the threshold).

Message model: see ``oracle/honey_badger.py`` (the message-at-a-time restatement this is tested
against): ``("share", sender, proposer, share48)`` and ``("acs", {proposer: (u48, v, w96)})``.
A node does not receive its own share messages (it inserts its own share itself, :394-418).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from .hbx import CT_INVALID, CT_UNDECODABLE, CT_VALID, SHARE_INVALID, SHARE_UNDECODABLE, layers

UNVERIFIED_DECRYPTION_SHARE_SENDER = "UnverifiedDecryptionShareSender"
INVALID_CIPHERTEXT = "InvalidCiphertext"
SHARE_DECRYPTION_FAILED = "ShareDecryptionFailed"
UNKNOWN_SENDER = "UnknownSender"


@dataclass
class EpochResult:
    faults: List[Tuple[int, str]] = field(default_factory=list)  # FaultLog entries, in order
    errors: List[Tuple[int, str]] = field(default_factory=list)  # handle_message -> Err
    batch: Optional[Dict[int, bytes]] = None  # proposer -> contribution, once the epoch output
    decrypt_errors: List[int] = field(default_factory=list)  # proposers whose decrypt failed (:345)
    ct_status: Dict[int, int] = field(default_factory=dict)  # proposer -> HBX_CT_*
    share_status: List[Optional[int]] = field(default_factory=list)  # per event: HBX_SHARE_* or None


class EpochReplay:
    """One node-epoch of the decryption sub-path over an ``hbx.Context``.

    ``ctx`` must hold the era's key shares (``set_pk_shares``, n keys); ``sk_me`` is this node's
    32-byte secret key share, installed with ``set_own_share`` so the engine computes our own
    decryption shares (``decrypt_share_no_verify``, :403) and checks the ciphertexts through
    them.  ``batch_seed`` (32 bytes no sender can predict, e.g. ``os.urandom(32)`` per epoch)
    switches the context to batched share verification (``hbx_set_batch_verify``) for this replay's
    verifications; the result is the same."""

    def __init__(self, ctx, n: int, me: int, sk_me: bytes, batch_seed: Optional[bytes] = None):
        self.ctx = ctx
        self.batch_seed = None if batch_seed is None else bytes(batch_seed)
        self.n = n
        self.f = (n - 1) // 3  # NetworkInfo::num_faulty, messaging.rs:258
        # PublicKeySet::decrypt needs threshold + 1 = f + 1 shares (the key set's threshold is f)
        self.t = self.f + 1
        self.me = me
        self.sk_me = bytes(sk_me)

    # ------------------------------------------------------------------------------------------
    def _engine(self, events, acs_pos):
        """Steps 1-2: ciphertext statuses and one status per share message of an ACS proposer."""
        cs_output = events[acs_pos][1]
        props = sorted(cs_output)
        col = {pid: j for j, pid in enumerate(props)}
        p, n = len(props), self.n
        self.ctx.set_own_share(self.me, self.sk_me)
        self.ctx.prepare_ciphertexts([cs_output[pid] for pid in props])
        ct_status = self.ctx.ct_status(p)
        # layer L holds the L-th message of every (proposer, sender) pair
        layers: List[Dict[Tuple[int, int], int]] = []
        seen: Dict[Tuple[int, int], int] = {}
        for k, ev in enumerate(events):
            if ev[0] != "share":
                continue
            _, sender, pid, _ = ev
            if sender >= n or pid not in col:
                continue
            if sender == self.me:
                raise ValueError("a node does not receive its own DecryptionShare messages")
            key = (col[pid], sender)
            L = seen.get(key, 0)
            seen[key] = L + 1
            if L == len(layers):
                layers.append({})
            layers[L][key] = k
        status: Dict[int, int] = {}
        for layer in layers or [{}]:
            shares = np.zeros((p, n, 48), dtype=np.uint8)
            present = np.zeros((p, n), dtype=bool)
            for (j, i), k in layer.items():
                shares[j, i] = np.frombuffer(bytes(events[k][3]), dtype=np.uint8)
                present[j, i] = True
            self.ctx.verify_dec_shares(shares, present)
            st = self.ctx.share_status(p, n)
            for (j, i), k in layer.items():
                status[k] = int(st[j, i])
        return props, {pid: int(ct_status[j]) for j, pid in enumerate(props)}, status, layers

    def run(self, events) -> EpochResult:
        if self.batch_seed is None:
            return self._run(events)
        self.ctx.set_batch_verify(self.batch_seed)
        try:
            return self._run(events)
        finally:
            self.ctx.set_batch_verify(None)

    def _run(self, events) -> EpochResult:
        events = list(events)
        res = EpochResult(share_status=[None] * len(events))
        acs = [k for k, ev in enumerate(events) if ev[0] == "acs"]
        if len(acs) > 1:
            raise ValueError("one CommonSubset output per epoch")
        acs_pos = acs[0] if acs else None
        props, ct_st, status, layers = ([], {}, {}, []) if acs_pos is None else self._engine(events, acs_pos)
        res.ct_status = ct_st
        for k, s in status.items():
            res.share_status[k] = s

        valid_cts: Optional[List[int]] = None  # proposers with a verified ciphertext, after the ACS
        received: Dict[int, Dict[int, int]] = {}  # proposer -> sender -> event index (-1 = own share)
        decrypted: set = set()
        done = False

        def try_output():
            nonlocal done
            if done or valid_cts is None:
                return
            ok = True
            for pid in valid_cts:  # all(): stops at the first proposer still short of shares
                if pid in decrypted:
                    continue
                if len(received.get(pid, {})) <= self.f:
                    ok = False
                    break
                decrypted.add(pid)
            if ok:
                done = True

        for k, ev in enumerate(events):
            if done:
                break  # messages of a past epoch are ignored (:68-76)
            if ev[0] == "share":
                _, sender, pid, _ = ev
                if sender >= self.n:
                    res.errors.append((sender, UNKNOWN_SENDER))
                    continue
                st = status.get(k)
                if st == SHARE_UNDECODABLE:
                    continue  # serde rejects the message before HoneyBadger sees it
                if valid_cts is not None and pid in valid_cts and st == SHARE_INVALID:
                    res.faults.append((sender, UNVERIFIED_DECRYPTION_SHARE_SENDER))
                    continue
                received.setdefault(pid, {})[sender] = k
                try_output()
            else:  # the CommonSubset output: send_decryption_shares
                valid_cts = []
                for pid in props:
                    if ct_st[pid] == CT_UNDECODABLE:
                        res.faults.append((pid, INVALID_CIPHERTEXT))
                        continue
                    if ct_st[pid] == CT_INVALID:
                        res.faults.append((pid, SHARE_DECRYPTION_FAILED))
                        continue
                    assert ct_st[pid] == CT_VALID
                    pending = received.get(pid, {})
                    for sender in sorted(pending):
                        if status.get(pending[sender]) == SHARE_INVALID:
                            res.faults.append((sender, UNVERIFIED_DECRYPTION_SHARE_SENDER))
                            del pending[sender]
                    received.setdefault(pid, {})[self.me] = -1  # our own share
                    valid_cts.append(pid)
                try_output()

        if done:
            res.batch = self._decrypt(events, props, received, decrypted, len(layers) > 1, res.decrypt_errors)
        return res

    def _decrypt(self, events, props, received, decrypted, relayer: bool, errors: List[int]) -> Dict[int, bytes]:
        """Step 4.  With several messages per pair, verify the final share set once more so the
        engine's combine reads exactly the shares the node ended up holding."""
        p, n = len(props), self.n
        if relayer:
            shares = np.zeros((p, n, 48), dtype=np.uint8)
            present = np.zeros((p, n), dtype=bool)
            for j, pid in enumerate(props):
                for sender, k in received.get(pid, {}).items():
                    if k >= 0:
                        shares[j, sender] = np.frombuffer(bytes(events[k][3]), dtype=np.uint8)
                        present[j, sender] = True
            self.ctx.verify_dec_shares(shares, present)
        plains, st = self.ctx.combine_decrypt(self.t)
        out = {}
        for j, pid in enumerate(props):
            if pid in decrypted:
                if st[j] != 0:
                    # PublicKeySet::decrypt returned Err: the reference only logs it (:345) and the
                    # proposer is left out of the batch
                    errors.append(pid)
                    continue
                out[pid] = plains[j]
        return out


@dataclass
class FlushResult:
    """What one ``EpochSession.flush`` added: FaultLog entries and errors in the reference's order,
    and the proposers decrypted since the last flush."""
    faults: List[Tuple[int, str]] = field(default_factory=list)
    errors: List[Tuple[int, str]] = field(default_factory=list)
    decrypted: Dict[int, bytes] = field(default_factory=dict)  # proposer -> contribution
    decrypt_errors: List[int] = field(default_factory=list)  # proposers whose decrypt failed (:345)


class EpochSession:
    """One node-epoch of the decryption sub-path, driven by messages as they arrive.

    ``EpochReplay`` decides a finished epoch in one pass; a node that is running the epoch calls
    ``handle(event)`` per message and ``flush()`` whenever it wants the engine brought up to date
    (after every message, or after a burst).  The results are the reference's, whatever the flush
    schedule:

    * before the CommonSubset output, shares are held on the host (``insert``: the last decodable
      message of a (proposer, sender) pair is the one the node holds, honey_badger.rs:205-210);
    * at the CommonSubset output: one ``prepare_ciphertexts`` and one matrix verification of the held
      shares -- the reference's own batch point, ``verify_pending_decryption_shares`` (:422-444).  A
      pair whose last message does not decode falls back to its earlier ones through adds;
    * after it: one ``add_dec_shares`` per flush (``handle_decryption_share_message``, :186-217), and
      one more per further message of the same pair within the flush;
    * within a flush the messages are replayed in arrival order over the status bytes, which gives
      the fault order, ``UnknownSender``, the ``all()`` short-circuit of ``try_output_batch`` and the
      decrypt errors as the reference emits them, and reports nothing after the batch is output;
    * the proposers that cross the threshold in a flush are decrypted by one
      ``combine_decrypt_cols`` (``try_decrypt_proposer_contribution``, :315-349).

    ``ctx`` must hold the era's key shares; ``sk_me`` is this node's 32-byte secret key share
    (own-share mode).  Message model: ``oracle/honey_badger.py``'s, as for ``EpochReplay``."""

    def __init__(self, ctx, n: int, me: int, sk_me: bytes):
        self.ctx = ctx
        self.n = n
        self.f = (n - 1) // 3
        self.t = self.f + 1
        self.me = me
        self.sk_me = bytes(sk_me)
        self.faults: List[Tuple[int, str]] = []
        self.errors: List[Tuple[int, str]] = []
        self.decrypted: Dict[int, bytes] = {}
        self.decrypt_errors: List[int] = []
        self.batch: Optional[Dict[int, bytes]] = None
        self.done = False
        self.ct_status: Dict[int, int] = {}
        self.share_status: List[Optional[int]] = []  # per handled event: HBX_SHARE_* if it was verified
        self._queue: List[tuple] = []
        self._held: Dict[Tuple[int, int], List[Tuple[int, bytes]]] = {}  # before the ACS: pair -> messages
        self._props: List[int] = []
        self._col: Dict[int, int] = {}
        self._valid_cts: Optional[List[int]] = None
        self._received: Dict[int, set] = {}  # proposer -> senders whose share the node holds
        self._reached: set = set()  # proposers past the threshold (decrypted or failed to)
        self._to_decrypt: List[int] = []

    def handle(self, event):
        """Queues one message; nothing reaches the engine before ``flush``."""
        if event[0] not in ("share", "acs"):
            raise ValueError(event[0])
        self._queue.append(event)

    # ------------------------------------------------------------------------------------------
    def _try_output(self):
        if self.done or self._valid_cts is None:
            return
        for pid in self._valid_cts:  # all(): stops at the first proposer still short of shares
            if pid in self._reached:
                continue
            if len(self._received.get(pid, ())) <= self.f:
                return
            self._reached.add(pid)
            self._to_decrypt.append(pid)
        self.done = True

    def _share_event(self, k: int, ev, status: Dict[int, int]):
        """handle_decryption_share_message over the engine's status byte of message k."""
        _, sender, pid, _ = ev
        if sender >= self.n:
            self.errors.append((sender, UNKNOWN_SENDER))
            return
        st = status.get(k)
        if pid not in self._col or st == SHARE_UNDECODABLE:
            return  # no ciphertext of that proposer this epoch / serde rejects the message
        if pid in self._valid_cts and st == SHARE_INVALID:
            self.faults.append((sender, UNVERIFIED_DECRYPTION_SHARE_SENDER))
            return
        self._received.setdefault(pid, set()).add(sender)
        self._try_output()

    def _add_layers(self, items: List[Tuple[int, int, int, bytes]], status: Dict[int, int]):
        """items (event index, column, sender, share48) in arrival order -> one add per layer, layer
        L holding the L-th message of every pair."""
        for idx in layers([(it[1], it[2]) for it in items]):
            layer = [items[i] for i in idx]
            shares = np.frombuffer(b"".join(bytes(it[3]) for it in layer), dtype=np.uint8).reshape(len(layer), 48)
            st = self.ctx.add_dec_shares(shares, np.array([it[1] for it in layer], dtype=np.uint32),
                                         np.array([it[2] for it in layer], dtype=np.uint32), self.n)
            for it, s in zip(layer, st):
                status[it[0]] = int(s)
                self.share_status[it[0]] = int(s)

    def _acs_event(self, cs_output):
        """send_decryption_shares: prepare, one matrix verification of the held shares, the faults."""
        if self._valid_cts is not None:
            raise ValueError("one CommonSubset output per epoch")
        self._props = sorted(cs_output)
        self._col = {pid: j for j, pid in enumerate(self._props)}
        p, n = len(self._props), self.n
        self.ctx.set_own_share(self.me, self.sk_me)
        self.ctx.prepare_ciphertexts([cs_output[pid] for pid in self._props])
        ct = self.ctx.ct_status(p)
        self.ct_status = {pid: int(ct[j]) for j, pid in enumerate(self._props)}
        held = {(self._col[pid], sender): msgs for (pid, sender), msgs in self._held.items() if pid in self._col}
        shares = np.zeros((p, n, 48), dtype=np.uint8)
        present = np.zeros((p, n), dtype=bool)
        for (j, i), msgs in held.items():
            shares[j, i] = np.frombuffer(bytes(msgs[-1][1]), dtype=np.uint8)
            present[j, i] = True
        self.ctx.verify_dec_shares(shares, present)
        st = self.ctx.share_status(p, n)
        pair_st: Dict[Tuple[int, int], int] = {}
        for (j, i), msgs in held.items():
            pair_st[(j, i)] = int(st[j, i])
            self.share_status[msgs[-1][0]] = int(st[j, i])
        # a pair whose last message serde rejects still holds its last decodable one
        depth = 2
        while True:
            back = [(msgs[-depth][0], j, i, msgs[-depth][1]) for (j, i), msgs in held.items()
                    if pair_st[(j, i)] == SHARE_UNDECODABLE and len(msgs) >= depth]
            if not back:
                break
            got: Dict[int, int] = {}
            self._add_layers(back, got)
            for k, j, i, _ in back:
                pair_st[(j, i)] = got[k]
            depth += 1
        self._held = {}
        self._valid_cts = []
        for j, pid in enumerate(self._props):
            if self.ct_status[pid] == CT_UNDECODABLE:
                self.faults.append((pid, INVALID_CIPHERTEXT))
                continue
            if self.ct_status[pid] == CT_INVALID:
                self.faults.append((pid, SHARE_DECRYPTION_FAILED))
                continue
            assert self.ct_status[pid] == CT_VALID
            got_from = set()
            for sender in sorted(i for (jj, i) in pair_st if jj == j):
                if pair_st[(j, sender)] == SHARE_UNDECODABLE:
                    continue
                if pair_st[(j, sender)] == SHARE_INVALID:
                    self.faults.append((sender, UNVERIFIED_DECRYPTION_SHARE_SENDER))
                    continue
                got_from.add(sender)
            got_from.add(self.me)  # our own share
            self._received[pid] = got_from
            self._valid_cts.append(pid)
        self._try_output()

    def flush(self) -> FlushResult:
        """Brings the engine up to date with the queued messages."""
        f0, e0, d0 = len(self.faults), len(self.errors), len(self.decrypt_errors)
        events, self._queue = self._queue, []
        k0 = len(self.share_status)
        self.share_status.extend([None] * len(events))
        pos = 0
        while pos < len(events) and not self.done:
            if self._valid_cts is None:
                ev = events[pos]
                if ev[0] == "acs":
                    self._acs_event(ev[1])
                else:
                    _, sender, pid, share48 = ev
                    if sender >= self.n:
                        self.errors.append((sender, UNKNOWN_SENDER))
                    elif sender == self.me:
                        raise ValueError("a node does not receive its own DecryptionShare messages")
                    else:
                        self._held.setdefault((pid, sender), []).append((k0 + pos, bytes(share48)))
                pos += 1
                continue
            # after the CommonSubset output: the rest of the flush through adds, then in arrival order
            rest = events[pos:]
            items = []
            for q, ev in enumerate(rest):
                if ev[0] == "acs":
                    raise ValueError("one CommonSubset output per epoch")
                _, sender, pid, share48 = ev
                if sender == self.me:
                    raise ValueError("a node does not receive its own DecryptionShare messages")
                if sender < self.n and pid in self._col:
                    items.append((k0 + pos + q, self._col[pid], sender, bytes(share48)))
            status: Dict[int, int] = {}
            self._add_layers(items, status)
            for q, ev in enumerate(rest):
                if self.done:
                    break  # messages of a past epoch are ignored (:68-76)
                self._share_event(k0 + pos + q, ev, status)
            pos = len(events)
        new: Dict[int, bytes] = {}
        if self._to_decrypt:
            pids, self._to_decrypt = self._to_decrypt, []
            plains, st = self.ctx.combine_decrypt_cols(self.t, [self._col[pid] for pid in pids])
            for pid in pids:
                j = self._col[pid]
                if st[j] != 0:
                    self.decrypt_errors.append(pid)  # the reference only logs it (:345)
                else:
                    new[pid] = plains[j]
            self.decrypted.update(new)
        if self.done and self.batch is None:
            self.batch = dict(self.decrypted)
        return FlushResult(self.faults[f0:], self.errors[e0:], new, self.decrypt_errors[d0:])
