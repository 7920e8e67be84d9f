"""EpochSession (hbbft_amd/honey_badger.py), the message-driven driver, on the CPU: a stand-in engine
answers from the fixtures' per-message statuses and enforces the add's merge rule itself.

* test_session_matches_fixture_under_every_schedule -- the fixture's faults in order, errors and
  batch, whatever the flush schedule;
* test_session_tracks_the_oracle_event_by_event -- oracle.honey_badger.EpochNode.handle stepped
  event by event, its crypto methods answering from the fixture (no Python pairing runs): after
  every event the faults, errors, decrypted set and `done` so far equal the session's.
"""
import numpy as np
import pytest

import replay_fixture as rf
from hbbft_amd.honey_badger import EpochSession

VALID, INVALID, ABSENT, UNDECODABLE, SKIPPED_CT = 1, 0, 2, 3, 4


def plain_of(d):
    """proposer -> the plaintext the engine (or the oracle) answers with, None for a decrypt error:
    the expected batch's, or, for an epoch that never outputs (no batch in the fixture), a marker."""
    batch = rf.expect(d)[2]
    if batch is None:
        return lambda pid: b"contribution of %d" % pid
    return batch.get


class SessionStatusEngine:
    """Stands in for hbx.Context: statuses per (column, sender, bytes) from expect_ev_status,
    ciphertext statuses from expect_ct_status, plaintexts from the expected batch.  Keeps the p x n
    status matrix as the engine does, so the combine answers from what was delivered."""

    def __init__(self, d, events):
        self.acs = [int(j) for j in d["acs_proposers"]]
        self.col = {j: q for q, j in enumerate(self.acs)}
        self.ct = d["expect_ct_status"]
        self.t = int(d["t"])
        self.by_msg = {}
        for k, ev in enumerate(events):
            st = int(d["expect_ev_status"][k])
            if ev[0] == "share" and st != rf.NO_STATUS:
                self.by_msg[(self.col[ev[2]], ev[1], ev[3])] = st
        self.plain = plain_of(d)
        self.matrix = None
        self.calls = []
        self.me = None

    def set_own_share(self, me, sk):
        self.me = me

    def prepare_ciphertexts(self, cts):
        assert len(cts) == len(self.acs)
        self.matrix = None  # a prepare voids the matrix
        self.calls.append("prepare")
        return self.ct == 1

    def ct_status(self, p):
        return self.ct.copy()

    def _own(self, st):
        for j in range(st.shape[0]):  # own-share mode: this node's share is valid iff the ciphertext is
            st[j, self.me] = VALID if self.ct[j] == 1 else SKIPPED_CT

    def verify_dec_shares(self, shares, present):
        p, n, _ = shares.shape
        st = np.full((p, n), ABSENT, dtype=np.uint8)
        for j in range(p):
            for i in range(n):
                if present[j, i]:
                    st[j, i] = self.by_msg[(j, i, shares[j, i].tobytes())]
        self._own(st)
        self.matrix = st
        self.calls.append("verify")
        return st == 1

    def share_status(self, p, n):
        return self.matrix.copy()

    def add_dec_shares(self, shares48, proposer, sender, n):
        assert self.matrix is not None, "the session verifies the pending shares before it adds"
        assert shares48.shape == (len(proposer), 48) and len(proposer) == len(sender)
        pairs = list(zip(proposer.tolist(), sender.tolist()))
        assert len(set(pairs)) == len(pairs), "the same (proposer, sender) twice in one add"
        out = np.zeros(len(pairs), dtype=np.uint8)
        for k, (j, i) in enumerate(pairs):
            assert j < self.matrix.shape[0] and i != self.me and i < n
            st = self.by_msg[(j, i, shares48[k].tobytes())]
            out[k] = st
            if not (self.matrix[j, i] == VALID and st != VALID):  # the merge rule
                self.matrix[j, i] = st
        self.calls.append("add")
        return out

    def combine_decrypt_cols(self, t, cols):
        assert t == self.t and len(set(cols)) == len(cols)
        plains, st = {}, {}
        for j in cols:
            enough = self.ct[j] == 1 and int((self.matrix[j] == VALID).sum()) >= t
            assert enough, "a proposer is decrypted only once it holds more than f valid shares"
            pt = self.plain(self.acs[j])
            plains[j], st[j] = pt, 0 if pt is not None else -3
        self.calls.append("combine")
        return plains, st


SCHEDULES = {
    "every event": lambda k, n, acs: True,
    "every 3": lambda k, n, acs: (k + 1) % 3 == 0,
    "every 7": lambda k, n, acs: (k + 1) % 7 == 0,
    "at the end": lambda k, n, acs: False,
    "after the acs and at the end": lambda k, n, acs: k == acs,
}


@pytest.mark.parametrize("schedule", list(SCHEDULES))
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_session_matches_fixture_under_every_schedule(tag, schedule):
    d = rf.load(tag)
    events = rf.events_of(d)
    acs = [k for k, ev in enumerate(events) if ev[0] == "acs"][0]
    eng = SessionStatusEngine(d, events)
    ses = EpochSession(eng, int(d["n"]), int(d["me"]), d["sk_me"].tobytes())
    faults, errors, decrypted = [], [], {}
    for k, ev in enumerate(events):
        ses.handle(ev)
        if SCHEDULES[schedule](k, len(events), acs) or k + 1 == len(events):
            res = ses.flush()
            faults += res.faults
            errors += res.errors
            assert not set(res.decrypted) & set(decrypted)
            decrypted.update(res.decrypted)
    want_faults, want_errors, want_batch = rf.expect(d)
    assert faults == ses.faults == want_faults
    assert errors == ses.errors == want_errors
    assert ses.batch == want_batch
    if want_batch is not None:
        assert decrypted == want_batch
    assert eng.calls.count("prepare") == 1 and eng.calls.count("verify") == 1
    assert eng.calls.index("prepare") < eng.calls.index("verify")
    for k, st in enumerate(ses.share_status):
        if st is not None:
            assert st == int(d["expect_ev_status"][k])


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_session_tracks_the_oracle_event_by_event(tag):
    from oracle import honey_badger as ohb
    from oracle import threshold as tc

    d = rf.load(tag)
    events = rf.events_of(d)
    ct_st = {int(j): int(d["expect_ct_status"][q]) for q, j in enumerate(d["acs_proposers"])}
    share_st = {}
    for k, ev in enumerate(events):
        if ev[0] == "share":
            share_st.setdefault((ev[1], ev[2], ev[3]), int(d["expect_ev_status"][k]))
    plain = plain_of(d)

    class FixtureNode(ohb.EpochNode):
        """The reference's control flow over the fixture's answers: no pairing, no curve arithmetic."""

        def _decode_share(self, share48):
            # a share of a proposer outside the CommonSubset output has no recorded status: it is
            # never verified, and nothing visible depends on whether it decodes
            st = [v for (s, j, b), v in share_st.items() if b == share48]
            return None if st and st[0] == UNDECODABLE else ("ok", share48)

        def _decode_ciphertext(self, ct):
            pid = [j for j, c in events[acs_pos][1].items() if c == ct][0]
            return None if ct_st[pid] == 3 else (pid, ct)

        def _ciphertext_verify(self, proposer, ct):
            return ct_st[proposer] == 1

        def _own_share(self, ct):
            return b"own"

        def _verify_share(self, sender, share, proposer, ct):
            return share_st[(sender, proposer, share)] == VALID

        def _decrypt(self, shares, ct):
            pt = plain(ct[0])
            if pt is None:
                raise tc.NotEnoughShares()
            return pt

    acs_pos = [k for k, ev in enumerate(events) if ev[0] == "acs"][0]
    node = object.__new__(FixtureNode)  # EpochNode.__init__ derives key shares: not needed here
    node.n, node.f, node.me = int(d["n"]), (int(d["n"]) - 1) // 3, int(d["me"])
    node.ciphertexts, node.hashes, node.received, node.decrypted = None, {}, {}, {}
    node.decrypt_errors, node.faults, node.errors, node.batch, node.done = [], [], [], None, False
    eng = SessionStatusEngine(d, events)
    ses = EpochSession(eng, int(d["n"]), int(d["me"]), d["sk_me"].tobytes())
    for k, ev in enumerate(events):
        node.handle(ev)
        ses.handle(ev)
        ses.flush()
        assert ses.faults == node.faults, f"event {k}"
        assert ses.errors == node.errors, f"event {k}"
        assert set(ses.decrypted) == set(node.decrypted), f"event {k}"
        assert ses.decrypt_errors == node.decrypt_errors
        assert ses.done == node.done, f"event {k}"
        assert ses.decrypted == node.decrypted
    assert node.batch == ses.batch == rf.expect(d)[2]
    assert node.done == bool(d["expect_batch"])
