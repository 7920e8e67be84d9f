"""BroadcastSession (hbbft_amd/broadcast.py) over an oracle-backed stand-in for the add engine: under
every flush schedule the concatenated flush results are what ``src/broadcast.rs`` emits message by
message (``oracle/broadcast.py``) and what ``BroadcastReplay`` gives for the whole log."""
import pytest

from bc_session_fixture import (ADVERSARIES, EPOCHS, SCHEDULES, OracleAddEngine, check_against_oracle,
                                check_equals_replay, epoch_scenario, ob, rm, run_session, sim_value, simulate)
from hbbft_amd.broadcast import BroadcastSession


@pytest.mark.parametrize("every", SCHEDULES)
@pytest.mark.parametrize("n", [4, 7, 10])
@pytest.mark.parametrize("adv,sched", ADVERSARIES)
def test_session_simulated(n, adv, sched, every):
    received, nodes = simulate(n, adv, sched, sim_value(adv), seed=1000 * n + len(adv) + len(sched))
    for i, events in received.items():
        total, _ = run_session(OracleAddEngine(), n, i, events, every, max_shard_len=64)
        check_against_oracle(total, nodes[i], n)
        check_equals_replay(total, events, n, i, "sha256")


@pytest.mark.parametrize("every", SCHEDULES)
@pytest.mark.parametrize("variant", ["sha256", "sha3"])
@pytest.mark.parametrize("n,me,seed,short", EPOCHS)
def test_session_epoch(n, me, seed, short, variant, every):
    events, _ = epoch_scenario(n, me, seed, variant, short_leaves=short)
    node = ob.BroadcastNode(n, me, variant).run(events)
    eng = OracleAddEngine(variant)
    total, ses = run_session(eng, n, me, events, every)
    check_against_oracle(total, node, n)
    check_equals_replay(total, events, n, me, variant)
    assert set(p for p, _ in total.outputs) == set(range(n)) - {3} - ({short} if short is not None else set())
    # an attempt is handed to the engine once: a failed one is retried only with another sender set
    assert len(eng.listed) == len(set(eng.listed)) == ses.engine_decodes
    # an instance that decided is never listed again: its successful attempt is its last
    for p, value in total.outputs:
        mine = [a for a in eng.listed if a[0] == p]
        q, root, senders = mine[-1]
        vals = [eng.store[(p, i)]["value"] if i in senders else None for i in range(n)]
        assert ob.decode_from_shards(vals, n, root, variant) == value


def test_session_retries_only_with_a_new_sender_set():
    """Proposer 2 of the epoch scenario fails until every Echo is in: flushing after each message,
    every listed attempt of it has a sender set of its own, and Readys that arrive between two Echos
    (the same set again) reach the reference's decode but not the engine."""
    n, me = 7, 6
    events, _ = epoch_scenario(n, me, 1)
    eng = OracleAddEngine()
    total, ses = run_session(eng, n, me, events, 1)
    mine = [a for a in eng.listed if a[0] == 2]
    assert len(mine) >= 2 and len({a[2] for a in mine}) == len(mine)
    ran2 = [a for a in total.decode_attempts if a[0] == 2]
    assert len(ran2) >= len(mine) and ran2[-1][2] and not ran2[0][2]
    assert ses.engine_decodes <= len(total.decode_attempts)


def test_value_after_an_echo_in_our_name():
    """An Echo claiming our own id fills slot (p, me) before the proposer's Value arrives: the add
    reports the Value as a duplicate, the session validates it apart and still sends our Echo."""
    n, me, p = 4, 1, 0
    _, leaves, tree = rm.send_shards(b"some value", n)
    events = [("echo", me, p, tree.gen_proof(leaves[me])), ("value", p, p, tree.gen_proof(leaves[me]))]
    bad = dict(tree.gen_proof(leaves[me]), value=leaves[me][:-1] + bytes([leaves[me][-1] ^ 1]))
    for evs in (events, [events[0], ("value", p, p, bad)]):
        node = ob.BroadcastNode(n, me).run(evs)
        for every in (1, None):
            total, _ = run_session(OracleAddEngine(), n, me, evs, every, max_shard_len=64)
            check_against_oracle(total, node, n)


def test_oversize_value_raises():
    n, me = 4, 1
    _, leaves, tree = rm.send_shards(b"x" * 100, n)
    ses = BroadcastSession(OracleAddEngine(), n, me, max_shard_len=8)
    ses.handle(("echo", 2, 0, tree.gen_proof(leaves[2])))
    ses.handle(("ready", 3, 0, tree.root_hash()))
    with pytest.raises(ValueError, match="max_shard_len"):
        ses.flush()
    # refused before anything was taken: nothing stored, both messages still queued
    assert ses.engine.store == {} and len(ses._queue) == 2 and ses.engine_adds == 0
