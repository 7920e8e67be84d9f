"""Batched replay of the Common Coin (``src/common_coin.rs``) for every coin instance of a round at
one node.

The reference runs one ``CommonCoin`` per Agreement instance and handles its signature shares one
message at a time: each share is verified on arrival (``PublicKeyShare::verify``, :151), and as
soon as the node has had its input and holds more than f valid shares it combines them
(``combine_signatures``, :190), checks the result against the master key (:196) and outputs the
parity (:173), ignoring every later message (:105-110).  This host-side driver gives the same
FaultLog, errors, messages and outputs, in the same order, with ONE engine pass per step:

1. ``hbx_prepare_nonces``: hash_g2 of every instance's nonce, once;
2. our own share of every instance we input to: one ``hbx_sign`` call;
3. every signature share of the round -- received messages and our own shares, in arrival order
   -- in one ``hbx_verify_sig_shares_d`` call (a second call per extra message of the same
   (instance, sender) pair, which only a Byzantine sender produces) -> one HBX_SHARE_* status per
   message; verification is deterministic, so verifying early changes no result;
4. the messages are replayed in arrival order through the reference's control flow with those
   statuses; each time ``try_output`` would combine, the set of shares the instance holds at that
   moment is recorded and the instance is taken to terminate;
5. the recorded sets are combined in one ``hbx_combine_signatures_d`` call, restricted to exactly
   those shares (``d_use``); a combination that fails the master check (``VerificationFailed``:
   the reference keeps the instance open and retries on a later share) is remembered and the
   replay runs again, so the retries happen exactly where the reference would run them.

``CoinReplay`` decides a finished round.  ``CoinSession`` (below) serves a node that is running
one: the messages are fed as they arrive, each flush appends its shares to the matrix the context
holds (``hbx_add_sig_shares_d``) and combines only the instances that triggered
(``hbx_combine_signatures_insts_d``), with the same results whatever the flush schedule.

Message model: see ``oracle/common_coin.py`` (the message-at-a-time restatement this is tested
against): ``("input", inst)`` and ``("share", sender, inst, sig96)``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

from .hbx import SHARE_INVALID, SHARE_UNDECODABLE, SHARE_UNKNOWN_SENDER, SHARE_VALID, layers

UNVERIFIED_SIGNATURE_SHARE_SENDER = "UnverifiedSignatureShareSender"
UNKNOWN_SENDER = "UnknownSender"
VERIFICATION_FAILED = "VerificationFailed"
COMBINE_FAILED = "CombineAndVerifySigCrypto"


@dataclass
class CoinResult:
    faults: List[Tuple[int, str]] = field(default_factory=list)  # FaultLog entries, in order
    errors: List[Tuple[Optional[int], str]] = field(default_factory=list)  # (sender, error) in order
    sent: List[Tuple[int, bytes]] = field(default_factory=list)  # (inst, our share) sent to all
    outputs: List[Tuple[int, bool]] = field(default_factory=list)  # (inst, parity) in output order
    combines: List[Tuple[int, Tuple[int, ...], bool]] = field(default_factory=list)  # as try_output ran
    share_status: List[Optional[int]] = field(default_factory=list)  # per event: HBX_SHARE_* or None
    engine_combines: int = 0  # engine combine calls (1 unless a combination failed)


class GpuCoinEngine:
    """The batched coin operations on the GPU through ``hbx.Context`` (torch tensors are the HBM
    buffers; torch is plumbing only).  The context holds the era's key shares
    (``set_pk_shares``)."""

    def __init__(self, ctx, master_pk48: bytes, sk32: Optional[bytes] = None, stream=None):
        import torch

        self.torch = torch
        self.ctx = ctx
        self.master_pk48 = bytes(master_pk48)
        self.sk32 = None if sk32 is None else bytes(sk32)
        self.stream = stream
        self.count = 0

    def prepare(self, nonces):
        self.ctx.prepare_nonces([bytes(x) for x in nonces], hashes=False)
        self.count = len(nonces)

    def sign(self) -> np.ndarray:
        """Our share of every prepared nonce -> uint8[count, 96]."""
        sk = np.frombuffer(self.sk32, dtype=np.uint8).reshape(1, 32)
        return self.ctx.sign(sk)[:, 0]

    def verify(self, sigs: np.ndarray, present: np.ndarray) -> np.ndarray:
        torch = self.torch
        count, n, _ = sigs.shape
        dev = torch.device("cuda", self.ctx.device)
        d_sig = torch.from_numpy(np.ascontiguousarray(sigs)).to(dev)
        d_pres = torch.from_numpy(np.ascontiguousarray(present, dtype=np.uint8)).to(dev)
        d_st = torch.zeros((count, n), dtype=torch.uint8, device=dev)
        self.ctx.verify_sig_shares_d(d_sig, d_pres, d_st, stream=self.stream)
        return d_st.cpu().numpy()

    def combine(self, use: np.ndarray, t: int):
        """Over the shares of the last ``verify`` call restricted to ``use`` -> (status int32[count],
        master_ok bool[count], parity bool[count])."""
        torch = self.torch
        count = use.shape[0]
        dev = torch.device("cuda", self.ctx.device)
        d_use = torch.from_numpy(np.ascontiguousarray(use, dtype=np.uint8)).to(dev)
        d_st = torch.zeros(count, dtype=torch.int32, device=dev)
        d_ok = torch.zeros(count, dtype=torch.uint8, device=dev)
        d_par = torch.zeros(count, dtype=torch.uint8, device=dev)
        self.ctx.combine_signatures_d(self.master_pk48, t, d_use, None, d_st, d_ok, d_par, stream=self.stream)
        return d_st.cpu().numpy(), d_ok.cpu().numpy().astype(bool), d_par.cpu().numpy().astype(bool)


class _Inst:
    __slots__ = ("had_input", "terminated", "received")

    def __init__(self):
        self.had_input = False
        self.terminated = False
        self.received: Dict[int, int] = {}  # sender -> message id (BTreeMap<N, SignatureShare>)

    def copy(self) -> "_Inst":
        c = _Inst()
        c.had_input, c.terminated, c.received = self.had_input, self.terminated, dict(self.received)
        return c


def _replay(events, msgs, msg_of_event, status, insts, known, held_key, n: int, f: int, me: Optional[int]):
    """The reference's control flow over ``events`` with the engine's status of every share message
    (``status[m]``, ``m = msg_of_event[k]``) -> (CoinResult, pending).  ``insts``: the state every
    instance starts from, advanced in place.  ``known``: (inst, key of the held set) -> (error,
    parity) of the combinations run so far, ``held_key(received)`` the key of a held set in it; an
    instance whose set is not in ``known`` goes into ``pending`` (inst -> key) and is taken to
    terminate, to be combined after this pass.

    Two cases arise in ``CoinSession`` alone: an event with no message (its instance terminated
    before the flush) and the status SHARE_UNKNOWN_SENDER (our own share when ``me`` is no
    validator).  ``CoinReplay`` gives every share event a message and its engine never returns that
    status."""
    res = CoinResult()
    pending: dict = {}

    def try_output(inst, who):
        b = insts[inst]
        if not (b.had_input and len(b.received) > f):
            return
        senders, key = tuple(sorted(b.received)), held_key(b.received)
        r = known.get((inst, key))
        if r is None:
            pending[inst] = key  # combined after this pass; taken to succeed meanwhile
            b.terminated = True
            return
        err, par = r
        res.combines.append((inst, senders, err is None))
        if err is not None:
            res.errors.append((who, err))
            return
        b.terminated = True
        res.outputs.append((inst, par))

    def handle_share(inst, sender, m, who):
        st = status[m]
        if st == SHARE_UNKNOWN_SENDER:
            res.errors.append((who, UNKNOWN_SENDER))
            return
        if st != SHARE_VALID:
            if st == SHARE_INVALID:
                res.faults.append((sender, UNVERIFIED_SIGNATURE_SHARE_SENDER))
            return
        insts[inst].received[sender] = m
        try_output(inst, who)

    for k, ev in enumerate(events):
        if ev[0] == "input":
            inst = ev[1]
            b = insts[inst]
            if b.had_input:
                continue
            b.had_input = True
            if me is None:
                try_output(inst, None)
                continue
            m = msg_of_event[k]
            # get_coin (common_coin.rs:142-146): an error from our own share's handle_share
            # drops the step with the outgoing message (the `?`); the error is our input's
            n_err = len(res.errors)
            handle_share(inst, me, m, None)
            if len(res.errors) == n_err:
                res.sent.append((inst, msgs[m][2]))
        else:
            _, sender, inst, _ = ev
            m = msg_of_event.get(k)
            if m is None or status[m] == SHARE_UNDECODABLE:
                continue  # terminated before the flush, or rejected by serde before CommonCoin
            if insts[inst].terminated:
                continue  # handle_message after termination (:105-110)
            if not 0 <= sender < n:
                res.errors.append((sender, UNKNOWN_SENDER))
                continue
            handle_share(inst, sender, m, sender)
    return res, pending


class CoinReplay:
    """Every CommonCoin instance of a round at node ``me`` (None: an observer, not a validator)."""

    def __init__(self, engine, n: int, me: Optional[int]):
        self.engine = engine
        self.n = n
        self.f = (n - 1) // 3  # NetworkInfo::num_faulty, messaging.rs:258
        self.t = self.f + 1    # combine_signatures needs threshold + 1 shares
        self.me = me

    def run(self, nonces, events) -> CoinResult:
        events = list(events)
        count, n = len(nonces), self.n
        self.engine.prepare(nonces)
        inputs = {ev[1] for ev in events if ev[0] == "input"}
        own = self.engine.sign() if (self.me is not None and inputs) else None
        # the share messages: received ones and, at our first input to an instance, our own
        msgs: List[Tuple[int, int, bytes]] = []  # (inst, sender, sig96)
        msg_of_event: Dict[int, int] = {}
        seen_input = set()
        for k, ev in enumerate(events):
            if ev[0] == "input":
                inst = ev[1]
                if self.me is not None and inst not in seen_input:
                    msg_of_event[k] = len(msgs)
                    msgs.append((inst, self.me, bytes(own[inst])))
                seen_input.add(inst)
            elif ev[0] == "share":
                _, sender, inst, sig96 = ev
                msg_of_event[k] = len(msgs)
                msgs.append((inst, sender, bytes(sig96)))
            else:
                raise ValueError(ev[0])
        status, layer_of = self._verify(msgs, count)
        res_status = [None] * len(events)
        for k, m in msg_of_event.items():
            if events[k][0] == "share" and 0 <= events[k][1] < n:
                res_status[k] = int(status[m])
        # replay + combine waves until every combination the control flow runs is known
        known: Dict[Tuple[int, Tuple[Tuple[int, int], ...]], Tuple[Optional[str], bool]] = {}  # -> (error, parity)
        combines_run = 0
        while True:
            # from a fresh round each pass; a held set is keyed by its (sender, message id) pairs:
            # a sender's repeated message is another share
            res, pending = _replay(events, msgs, msg_of_event, status, [_Inst() for _ in range(count)], known,
                                   lambda received: tuple(sorted(received.items())), n, self.f, self.me)
            if not pending:
                break
            combines_run += 1
            self._combine(pending, msgs, layer_of, known, count)
        res.share_status = res_status
        res.engine_combines = combines_run
        return res

    # ------------------------------------------------------------------------------------------
    def _verify(self, msgs, count):
        """One engine call per layer (layer L = the L-th message of each (inst, sender) pair).  A
        message from a non-validator is never verified, but whether serde would have decoded it
        decides between no reaction and UnknownSender: those go first, through columns of their
        own instance's row (only the UNDECODABLE status is used), so that the real layers are the
        last verifications the engine holds."""
        n = self.n
        unknown = [m for m, (_, sender, _) in enumerate(msgs) if not 0 <= sender < n]
        status = np.full(len(msgs), SHARE_UNDECODABLE, dtype=np.int32)
        # decode-only layers: the unknown-sender messages of each instance over columns 0..n-1
        slot: Dict[int, int] = {}
        batches: List[Dict[Tuple[int, int], int]] = []
        for m in unknown:
            inst = msgs[m][0]
            q = slot.get(inst, 0)
            slot[inst] = q + 1
            if q // n == len(batches):
                batches.append({})
            batches[q // n][(inst, q % n)] = m
        for batch in batches:
            st = self._verify_layer(batch, msgs, count)
            for key, m in batch.items():
                status[m] = SHARE_UNDECODABLE if st[key] == SHARE_UNDECODABLE else SHARE_INVALID
        layer_of = [-1] * len(msgs)
        real = [m for m, (_, sender, _) in enumerate(msgs) if 0 <= sender < n]
        self._last_layer = -1
        for L, idx in enumerate(layers([msgs[m][:2] for m in real])):
            layer = {msgs[real[i]][:2]: real[i] for i in idx}
            st = self._verify_layer(layer, msgs, count)
            for key, m in layer.items():
                status[m] = st[key]
                layer_of[m] = L
            self._last_layer = L
        return status, layer_of

    def _verify_layer(self, layer, msgs, count):
        sigs = np.zeros((count, self.n, 96), dtype=np.uint8)
        present = np.zeros((count, self.n), dtype=np.uint8)
        for key, m in layer.items():
            sigs[key] = np.frombuffer(msgs[m][2], dtype=np.uint8)
            present[key] = 1
        return self.engine.verify(sigs, present)

    def _combine(self, pending, msgs, layer_of, known, count):
        """One engine combine over the pending sets.  When every held share is in the last
        verified layer (always, unless a sender repeated itself), the combination reuses that
        verification through the use mask; otherwise the held shares are verified again as one
        layer of their own (they were verified before, so their statuses do not change)."""
        n = self.n
        last = self._last_layer
        use = np.zeros((count, n), dtype=np.uint8)
        reuse = all(layer_of[m] == last for held in pending.values() for _, m in held)
        if not reuse:
            sigs = np.zeros((count, n, 96), dtype=np.uint8)
            present = np.zeros((count, n), dtype=np.uint8)
            for inst, held in pending.items():
                for s, m in held:
                    sigs[inst, s] = np.frombuffer(msgs[m][2], dtype=np.uint8)
                    present[inst, s] = 1
            self.engine.verify(sigs, present)
            self._last_layer = -1  # the engine's last verification is no longer a layer
        for inst, held in pending.items():
            for s, _ in held:
                use[inst, s] = 1
        st, ok, par = self.engine.combine(use, self.t)
        for inst, held in pending.items():
            err = COMBINE_FAILED if st[inst] != 0 else None if ok[inst] else VERIFICATION_FAILED
            known[(inst, held)] = (err, bool(par[inst]))


# ---- a node that is running its coin instances (hbx_add_sig_shares_d) -----------------------------
class GpuCoinAddEngine(GpuCoinEngine):
    """``GpuCoinEngine`` plus the incremental calls: ``add`` appends signature shares to the round's
    matrix in the context (``hbx_add_sig_shares_d``), ``combine_insts`` combines the listed
    instances (``hbx_combine_signatures_insts_d``)."""

    def add(self, sig96: np.ndarray, inst, sender, n: int) -> np.ndarray:
        """sig96 uint8[k, 96] for positions (inst[k], sender[k]) -> HBX_SHARE_* uint8[k]."""
        torch = self.torch
        dev = torch.device("cuda", self.ctx.device)
        k = len(inst)
        if k == 0:
            self.ctx.add_sig_shares_d(None, [], [], n, stream=self.stream)
            return np.zeros(0, dtype=np.uint8)
        d_sig = torch.from_numpy(np.array(sig96, dtype=np.uint8, order="C")).to(dev)  # a writable copy for torch
        d_st = torch.zeros(k, dtype=torch.uint8, device=dev)
        self.ctx.add_sig_shares_d(d_sig, inst, sender, n, d_st, stream=self.stream)
        return d_st.cpu().numpy()

    def combine_insts(self, insts, use: np.ndarray, t: int):
        """The listed instances over the matrix's VALID entries restricted to ``use`` -> (status
        int32[count], master_ok bool[count], parity bool[count]); only the listed entries mean
        anything."""
        torch = self.torch
        count = use.shape[0]
        dev = torch.device("cuda", self.ctx.device)
        d_use = torch.from_numpy(np.ascontiguousarray(use, dtype=np.uint8)).to(dev)
        d_st = torch.zeros(count, dtype=torch.int32, device=dev)
        d_ok = torch.zeros(count, dtype=torch.uint8, device=dev)
        d_par = torch.zeros(count, dtype=torch.uint8, device=dev)
        self.ctx.combine_signatures_insts_d(self.master_pk48, t, insts, d_use, None, d_st, d_ok, d_par, stream=self.stream)
        return d_st.cpu().numpy(), d_ok.cpu().numpy().astype(bool), d_par.cpu().numpy().astype(bool)


class CoinSession:
    """Every CommonCoin instance of a round at node ``me`` (None: an observer), fed as the messages
    arrive: ``prepare(nonces)`` once, ``handle(event)`` queues an event, ``flush()`` runs the queued
    events and returns what they added -- faults, errors, sent, outputs and combines, as a
    ``CoinResult``.  Whatever the flush schedule, the results in flush order are what the reference
    emits message by message (``oracle/common_coin.py`` ``CoinNode.run``).

    Per flush: our own share of the instances that get their first input goes through the same
    checks as a received one (common_coin.rs:142-146); the queued shares -- except those of an
    instance that terminated before the flush, which never reach the engine (:105-110) -- are
    appended to the round's matrix with one ``add`` per layer of repeated (instance, sender) pairs
    (``hbx_add_sig_shares_d``: only the touched tiles are checked, the shares held from earlier
    flushes stay on the device); the reference's control flow is replayed over the status bytes;
    the instances whose ``try_output`` would combine are combined in one ``combine_insts``
    (``hbx_combine_signatures_insts_d``) with ``use`` = the shares held at the trigger; a combination
    that fails the master check (``VerificationFailed``) leaves its instance open and the replay
    runs again, so the retry happens where the reference retries.

    ``ctx``: an ``hbx.Context`` holding the era's key shares, or with ``engine=`` any object with
    ``prepare`` / ``sign`` / ``add`` / ``combine_insts`` (tests)."""

    def __init__(self, ctx, master_pk48: bytes, n: int, me: Optional[int], sk32: Optional[bytes] = None, engine=None,
                 stream=None):
        self.engine = engine if engine is not None else GpuCoinAddEngine(ctx, master_pk48, sk32, stream)
        self.n = n
        self.f = (n - 1) // 3  # NetworkInfo::num_faulty, messaging.rs:258
        self.t = self.f + 1    # combine_signatures needs threshold + 1 shares
        self.me = me
        self.count = 0
        self.engine_adds = 0      # engine add calls so far (one per layer per flush)
        self.engine_combines = 0  # engine combine calls so far
        self._queue: List[tuple] = []
        self._insts: List[_Inst] = []
        self._own: Optional[np.ndarray] = None
        self._known: Dict[Tuple[int, Tuple[int, ...]], Tuple[Optional[str], bool]] = {}

    def prepare(self, nonces):
        nonces = list(nonces)
        self.engine.prepare(nonces)
        self.count = len(nonces)
        self._insts = [_Inst() for _ in range(self.count)]
        self._queue, self._own, self._known = [], None, {}
        self.engine.add(np.zeros((0, 96), dtype=np.uint8), [], [], self.n)  # the round's matrix: every share absent
        self.engine_adds = self.engine_combines = 0

    def handle(self, event):
        if event[0] not in ("input", "share"):
            raise ValueError(event[0])
        self._queue.append(event)

    # ------------------------------------------------------------------------------------------
    def flush(self) -> CoinResult:
        events, self._queue = self._queue, []
        n = self.n
        # the share messages of this flush: received ones and, at our first input to an instance, our own
        msgs: List[Tuple[int, int, bytes]] = []  # (inst, sender as the engine sees it, sig96)
        msg_of_event: Dict[int, int] = {}
        seen_input = {q for q, b in enumerate(self._insts) if b.had_input}
        for k, ev in enumerate(events):
            if ev[0] == "input":
                inst = ev[1]
                if self.me is not None and inst not in seen_input:
                    if self._own is None:
                        self._own = self.engine.sign()
                    msg_of_event[k] = len(msgs)
                    msgs.append((inst, self.me, bytes(self._own[inst])))
                seen_input.add(inst)
            else:
                _, sender, inst, sig96 = ev
                if self._insts[inst].terminated:
                    continue  # handle_message after termination (:105-110): never verified
                msg_of_event[k] = len(msgs)
                # a sender outside 0..n-1 touches no position; the engine still says whether serde decodes it
                msgs.append((inst, sender if 0 <= sender < 0xFFFFFFFF else 0xFFFFFFFF, bytes(sig96)))
        status = self._add(msgs)
        res_status: List[Optional[int]] = [None] * len(events)
        for k, m in msg_of_event.items():
            if events[k][0] == "share" and 0 <= events[k][1] < n:
                res_status[k] = int(status[m])
        combines_run = 0
        while True:
            # from the state the last flush left; a held set is keyed by its senders: the matrix
            # holds one share per sender
            insts = [b.copy() for b in self._insts]
            res, pending = _replay(events, msgs, msg_of_event, status, insts, self._known,
                                   lambda received: tuple(sorted(received)), n, self.f, self.me)
            if not pending:
                break
            combines_run += 1
            self._combine(pending)
        self._insts = insts
        self.engine_combines += combines_run
        res.share_status = res_status
        res.engine_combines = combines_run
        return res

    def _add(self, msgs) -> np.ndarray:
        """One engine add per layer (layer L = the L-th message of each (inst, sender) pair in this
        flush), in order, so the matrix ends as message-by-message delivery leaves it."""
        status = np.full(len(msgs), SHARE_UNDECODABLE, dtype=np.int32)
        for layer in layers([msg[:2] for msg in msgs]):
            sig = np.frombuffer(b"".join(msgs[m][2] for m in layer), dtype=np.uint8).reshape(len(layer), 96)
            st = self.engine.add(sig, [msgs[m][0] for m in layer], [msgs[m][1] for m in layer], self.n)
            self.engine_adds += 1
            status[layer] = st
        return status

    def _combine(self, pending):
        """One engine combine over the instances that triggered, each over the shares it held then."""
        use = np.zeros((self.count, self.n), dtype=np.uint8)
        for inst, senders in pending.items():
            use[inst, list(senders)] = 1
        st, ok, par = self.engine.combine_insts(sorted(pending), use, self.t)
        for inst, senders in pending.items():
            err = COMBINE_FAILED if st[inst] != 0 else None if ok[inst] else VERIFICATION_FAILED
            self._known[(inst, senders)] = (err, bool(par[inst]))
