"""``hbbft_amd.common_coin.CoinSession`` over a CPU stand-in engine: whatever the flush schedule, the
results in flush order are what ``src/common_coin.rs`` emits message by message
(``oracle/common_coin.py`` ``CoinNode.run``).  The stand-in keeps the round's matrix as
``hbx_add_sig_shares`` does (the merge rule of include/hbx.h) on the oracle's crypto."""
import functools

import numpy as np
import pytest

from coin_scenarios import OracleCoinEngine, check_against_oracle, coin_scenario
from hbbft_amd.common_coin import CoinResult, CoinSession
from oracle import bls12_381 as bls
from oracle import common_coin as oc
from oracle import threshold as tc
from test_coin_replay import CASES

SHARE_INVALID, SHARE_VALID, SHARE_ABSENT, SHARE_UNDECODABLE, SHARE_UNKNOWN_SENDER = 0, 1, 2, 3, 5
SCHEDULES = {"every": 1, "five": 5, "end": None}


class AddEngine(OracleCoinEngine):
    """OracleCoinEngine plus ``add`` / ``combine_insts``: the matrix persists between calls."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.adds = []  # (inst, sender) lists, one per add
        self.listed = []  # instance lists, one per combine

    def prepare(self, nonces):
        super().prepare(nonces)
        self.st, self.pts = None, {}

    def add(self, sigs, inst, sender, n):
        if self.st is None:
            self.st = np.full((len(self.nonces), n), SHARE_ABSENT, dtype=np.uint8)
        assert n == self.st.shape[1]
        pairs = list(zip(inst, sender))
        assert len(set(pairs)) == len(pairs), "the same (inst, sender) twice in one add"
        assert all(0 <= q < len(self.nonces) for q in inst)
        if pairs:
            self.adds.append(pairs)
        out = np.zeros(len(pairs), dtype=np.uint8)
        for k, (q, i) in enumerate(pairs):
            try:
                pt = bls.g2_decompress(bytes(sigs[k]))
            except ValueError:
                pt = None
            if i >= n:  # touches no position
                out[k] = SHARE_UNDECODABLE if pt is None else SHARE_UNKNOWN_SENDER
                continue
            if pt is None:
                v = SHARE_UNDECODABLE
            else:
                ok = tc.verify_sig(self.pk_set.public_key_share(i), pt, self.nonces[q], self.variant, hash_pt=self.h[q])
                v = SHARE_VALID if ok else SHARE_INVALID
            out[k] = v
            if self.st[q, i] == SHARE_VALID and v != SHARE_VALID:
                continue  # a VALID entry keeps its point and status
            self.st[q, i] = v
            if pt is not None:
                self.pts[(q, i)] = pt
        return out

    def combine_insts(self, insts, use, t):
        assert len(set(insts)) == len(insts)
        self.listed.append(list(insts))
        only = np.zeros_like(use)
        only[list(insts)] = use[list(insts)]
        return self.combine(only, t)


@functools.lru_cache(maxsize=None)
def _case(n, me, count, seed):
    ns, sks, pks, events = coin_scenario(n, me, count, seed)
    sk = None if me is None else sks.secret_key_share(me)
    node = oc.CoinNode(n, me, pks, sk, ns).run(events)
    return ns, sks, pks, events, node


def run_session(session, ns, events, every):
    """The accumulated result of the session under a flush after every `every` events (None: once)."""
    acc = CoinResult()
    session.prepare(ns)

    def flush():
        r = session.flush()
        for name in ("faults", "errors", "sent", "outputs", "combines"):
            getattr(acc, name).extend(getattr(r, name))

    for k, ev in enumerate(events):
        session.handle(ev)
        if every and (k + 1) % every == 0:
            flush()
    flush()
    assert session.flush().outputs == []  # nothing queued: nothing happens
    return acc


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("n,me,count,seed", CASES)
def test_session_matches_the_reference(n, me, count, seed, schedule):
    ns, sks, pks, events, node = _case(n, me, count, seed)
    eng = AddEngine(pks, None if me is None else sks.secret_key_share(me))
    session = CoinSession(None, None, n, me, engine=eng)
    acc = run_session(session, ns, events, SCHEDULES[schedule])
    check_against_oracle(acc, node)
    # a flush combines only the instances that triggered
    assert sorted(q for lst in eng.listed for q in lst) == sorted(q for q, _ in node.outputs)
    assert all(len(lst) < count for lst in eng.listed)  # instance 2 never gets our input
    if schedule == "end":
        # one add per layer of repeated pairs: the scenario repeats one sender once
        assert session.engine_adds == 2 and session.engine_combines == 1


def test_session_keeps_terminated_instances_from_the_engine():
    n, me, count, seed = CASES[0]
    ns, sks, pks, events, node = _case(n, me, count, seed)
    eng = AddEngine(pks, sks.secret_key_share(me))
    session = CoinSession(None, None, n, me, engine=eng)
    acc = run_session(session, ns, events, 1)
    check_against_oracle(acc, node)
    # flushing after every message: what reaches the engine is what the reference verifies
    terminated, expect = set(), 0
    replay = oc.CoinNode(n, me, pks, sks.secret_key_share(me), ns)
    for ev in events:
        if ev[0] == "share" and ev[2] not in terminated:
            expect += 1
        if ev[0] == "input" and not replay.coins[ev[1]].had_input:
            expect += 1
        replay.handle(ev)
        terminated = {q for q, c in enumerate(replay.coins) if c.terminated}
    assert sum(len(p) for p in eng.adds) == expect


class _FlakyCombine(AddEngine):
    """The first combination of instance 0 fails the master check (as a wrong share set would):
    the reference keeps the instance open, logs VerificationFailed and retries on the next share."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.calls = 0

    def combine(self, use, t):
        st, ok, par = super().combine(use, t)
        if use[0].any():
            self.calls += 1
            if self.calls == 1:
                ok[0] = False
        return st, ok, par


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_session_retries_a_failed_combination(schedule):
    n, me, count, seed = 4, 3, 4, 5
    ns, sks, pks, events = coin_scenario(n, me, count, seed)
    eng = _FlakyCombine(pks, sks.secret_key_share(me))
    acc = run_session(CoinSession(None, None, n, me, engine=eng), ns, events, SCHEDULES[schedule])

    class Node(oc.CoinNode):
        first = True

        def _master_verify(self, sig, coin):
            if coin is self.coins[0] and Node.first:
                Node.first = False
                return False
            return super()._master_verify(sig, coin)

    node = Node(n, me, pks, sks.secret_key_share(me), ns).run(events)
    check_against_oracle(acc, node)
    assert (None, oc.VERIFICATION_FAILED) in node.errors
    assert 0 not in {inst for inst, _ in acc.sent}
    assert {inst for inst, _ in node.sent} == {inst for inst, _ in acc.sent} != set()
    assert 0 in {inst for inst, _ in node.outputs}  # retried on the next share, then output
    assert sum(0 in lst for lst in eng.listed) == 2
