"""Shared pieces of the BroadcastSession tests (CPU logic and GPU): the flush schedules, the scenario
list, an oracle-backed stand-in for GpuBroadcastAddEngine and the comparison of concatenated flush
results."""
from __future__ import annotations

import numpy as np

from bc_scenarios import OracleEngine, check_against_oracle, epoch_scenario, simulate
from hbbft_amd.broadcast import (ECHO_DUPLICATE, ECHO_INVALID, ECHO_OVERSIZE, ECHO_STORED, BroadcastReplay,
                                 BroadcastResult, BroadcastSession)
from oracle import broadcast as ob
from oracle import rs_merkle as rm

SCHEDULES = [1, 7, None]  # flush after every message, after every 7, once at the end
ADVERSARIES = [("silent", "random"), ("silent", "first"), ("propose", "random"), ("propose", "first"),
               ("random", "random"), ("random", "first")]
EPOCHS = [(7, 6, 1, None), (10, 9, 2, None), (13, 5, 3, None), (10, 9, 5, 8), (13, 5, 6, 11)]  # (n, me, seed, short)
MAX_SHARD = 3004  # epoch_scenario's values are at most 3000 bytes + 4 of framing, k >= 1


def sim_value(adv):
    return b"RandomFoo" if adv == "random" else b"Foo"


class OracleAddEngine(OracleEngine):
    """The echo store as a dict with the insert rule of hbx_add_echoes, the listed decode as
    oracle.broadcast.decode_from_shards over the held values restricted to the attempt's senders."""

    def __init__(self, variant="sha256"):
        super().__init__(variant)
        self.store = {}
        self.listed = []  # every attempt decode_listed was given

    def prepare(self, inst, n, max_shard_len):
        self.n, self.max_shard_len, self.store = n, max_shard_len, {}

    def add(self, proofs, insts, senders):
        assert len(set(zip(insts, senders))) == len(proofs), "a pair twice in one add"
        out = np.zeros(len(proofs), dtype=np.uint8)
        for j, (p, q, i) in enumerate(zip(proofs, insts, senders)):
            if (q, i) in self.store:
                out[j] = ECHO_DUPLICATE
            elif len(p["value"]) > self.max_shard_len + 1:
                out[j] = ECHO_OVERSIZE
            elif len(p["value"]) and rm.validate_broadcast_proof(p, i, self.n, self.variant):
                self.store[(q, i)] = p
                out[j] = ECHO_STORED
            else:
                out[j] = ECHO_INVALID
        return out

    def decode_listed(self, attempts):
        out = []
        for q, root, length, senders in attempts:
            self.listed.append((q, bytes(root), tuple(senders)))
            vals = [None] * self.n
            for i in senders:
                p = self.store.get((q, i))
                if p is not None and p["root_hash"] == root:
                    vals[i] = p["value"]
            assert length >= 1
            out.append(ob.decode_from_shards(vals, self.n, root, self.variant))
        return out


def run_session(engine, n, me, events, every, max_shard_len=MAX_SHARD):
    """The events through a BroadcastSession flushed after every `every` messages (None: once) ->
    (the flush results concatenated, the session)."""
    ses = BroadcastSession(engine, n, me, max_shard_len)
    total = BroadcastResult()
    pending = 0

    def flush():
        res = ses.flush()
        total.faults += res.faults
        total.errors += res.errors
        total.sent += res.sent
        total.outputs += res.outputs
        total.decode_attempts += res.decode_attempts
        total.value_proofs.update(res.value_proofs)
        total.proof_valid += res.proof_valid
        total.engine_decodes += res.engine_decodes

    for ev in events:
        ses.handle(ev)
        pending += 1
        if every is not None and pending == every:
            flush()
            pending = 0
    flush()
    return total, ses


def check_equals_replay(total, events, n, me, variant):
    """Field by field against BroadcastReplay over the oracle engine."""
    ref = BroadcastReplay(OracleEngine(variant), n, me).run(events)
    assert total.faults == ref.faults
    assert total.errors == ref.errors
    assert total.sent == ref.sent
    assert total.outputs == ref.outputs
    assert total.decode_attempts == ref.decode_attempts
    return ref


__all__ = ["SCHEDULES", "ADVERSARIES", "EPOCHS", "MAX_SHARD", "sim_value", "OracleAddEngine", "run_session",
           "check_equals_replay", "check_against_oracle", "epoch_scenario", "simulate", "ob", "rm"]
