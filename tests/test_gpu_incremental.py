"""Incremental share verification on the engine (hbx_add_dec_shares, hbx_combine_decrypt_cols,
hbx_get_verify_tiles_used) and the message-driven EpochSession over it.  Expectations are the
committed fixtures', or, where stated, the unchanged matrix call's on a second context."""
import hashlib
import os
import random

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

pytestmark = pytest.mark.gpu

SENDERS = {1: 64, 2: 32, 3: 21, 6: 10, 7: 64}  # senders per check block at each lanes setting
VALID, INVALID, ABSENT, UNDECODABLE, SKIPPED_CT, UNKNOWN_SENDER = 1, 0, 2, 3, 4, 5
_CACHE = {}


def _load(name):
    if name not in _CACHE:
        _CACHE[name] = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
    return _CACHE[name]


def _cts(d):
    off = d["v_off"]
    return [(d["u"][j].tobytes(), d["v_blob"][int(off[j]):int(off[j + 1])].tobytes(), d["w"][j].tobytes())
            for j in range(len(off) - 1)]


def _set_keys(ctx, d):
    ctx.set_digest(1 if str(d["digest"]) == "sha3_256" else 0)
    assert (ctx.set_pk_shares([row.tobytes() for row in d["pk_comp"]]) == 0).all()


@pytest.fixture(scope="module")
def ctx2():
    """A second context: the unchanged matrix call on the same inputs, as yardstick."""
    from hbbft_amd.hbx import Context

    c = Context(0)
    yield c
    c.close()


def _prepare(ctx, d, mode):
    """mode: eager (Ciphertext::verify in the prepare), deferred (_d with d_ct_valid NULL: decided by
    the next share verification) or own (own-share mode).  Returns what must stay alive."""
    if mode == "own":
        ctx.set_own_share(int(d["own_me"]), d["own_sk"].tobytes())
    if mode != "deferred":
        ctx.prepare_ciphertexts(_cts(d))
        return None
    import torch

    dev = torch.device("cuda", 0)
    off = d["v_off"].astype(np.int64)
    keep = [torch.from_numpy(np.ascontiguousarray(d["u"])).to(dev), torch.from_numpy(d["v_blob"].copy()).to(dev),
            torch.from_numpy(off).to(dev), torch.from_numpy(np.ascontiguousarray(d["w"])).to(dev)]
    ctx.prepare_ciphertexts_d(keep[0], keep[1], keep[2], keep[3], len(off) - 1, int(np.max(np.diff(off))))
    return keep


def _add(ctx, d, positions, n):
    """One add of the fixture's bytes at `positions` [(j, i)] -> status bytes."""
    pos = np.array(positions, dtype=np.int64).reshape(-1, 2)
    shares = np.ascontiguousarray(d["shares"][pos[:, 0], pos[:, 1]]) if len(pos) else np.zeros((0, 48), np.uint8)
    return ctx.add_dec_shares(shares, pos[:, 0].astype(np.uint32), pos[:, 1].astype(np.uint32), n)


def _mask(p, n, positions):
    m = np.zeros((p, n), dtype=bool)
    for j, i in positions:
        m[j, i] = True
    return m


def _check_plain(d, j, pt, own):
    assert hashlib.sha256(pt).digest() == d["expect_plain_sha_own" if own else "expect_plain_sha"][j].tobytes(), j


# ---- 4. partition equivalence ----------------------------------------------------------------
@pytest.mark.parametrize("first", ["matrix", "add"])
@pytest.mark.parametrize("mode", ["eager", "deferred", "own"])
@pytest.mark.parametrize("name", ["hb_epoch_n4", "hb_epoch_n7", "hb_epoch_n7_sha3", "hb_epoch_n10"])
def test_partition_into_adds_equals_one_matrix_call(hbx_ctx, ctx2, name, mode, first):
    d = _load(name)
    own = mode == "own"
    p, n = d["shares"].shape[:2]
    me = int(d["own_me"])
    expect = d["expect_share_status_own" if own else "expect_share_status"]
    positions = [(int(j), int(i)) for j, i in np.argwhere(d["present"]) if not (own and i == me)]
    random.Random(f"{name}/{mode}/{first}").shuffle(positions)
    groups = [positions[0::3], positions[1::3], positions[2::3]]
    try:
        for c in (hbx_ctx, ctx2):
            _set_keys(c, d)
        keep = _prepare(hbx_ctx, d, mode)
        delivered = []
        for g, group in enumerate(groups):
            if g == 0 and first == "matrix":
                hbx_ctx.verify_dec_shares(d["shares"], _mask(p, n, group))
                st = hbx_ctx.share_status(p, n)[tuple(np.array(group).T)]
            else:
                st = _add(hbx_ctx, d, group, n)  # on a fresh prepare the first add establishes the matrix
            delivered += group
            assert st.tolist() == [int(expect[j, i]) for j, i in group], f"group {g}"
            # the unchanged matrix call, on "present and delivered so far"
            keep2 = _prepare(ctx2, d, mode)
            ctx2.verify_dec_shares(d["shares"], _mask(p, n, delivered))
            np.testing.assert_array_equal(hbx_ctx.share_status(p, n), ctx2.share_status(p, n), err_msg=f"after group {g}")
            del keep2
        np.testing.assert_array_equal(hbx_ctx.share_status(p, n), expect)
        np.testing.assert_array_equal(hbx_ctx.ct_status(p), d["expect_ct_status"])
        plains, status = hbx_ctx.combine_decrypt(int(d["t"]))
        np.testing.assert_array_equal(status, d["expect_status_own" if own else "expect_status"])
        for j, pt in enumerate(plains):
            if status[j] == 0:
                _check_plain(d, j, pt, own)
        del keep
    finally:
        for c in (hbx_ctx, ctx2):
            c.set_own_share(0, None)


# ---- 5. merge rule -----------------------------------------------------------------------------
def test_merge_rule(hbx_ctx):
    from hbbft_amd.hbx import HBX_E_INVALID_ARG, HbxError

    d = _load("hb_epoch_n7")
    p, n = d["shares"].shape[:2]
    t = int(d["t"])
    exp = d["expect_share_status"]
    _set_keys(hbx_ctx, d)
    hbx_ctx.prepare_ciphertexts(_cts(d))
    assert _add(hbx_ctx, d, [], n).size == 0  # count == 0: only establishes the matrix
    assert (hbx_ctx.share_status(p, n) == ABSENT).all()
    J = 3  # a proposer whose every share is VALID; proposer 4 has valid shares of senders 2..5
    assert (exp[J] == VALID).all() and (exp[4, 2:6] == VALID).all()

    def add_bytes(b48, j, i):
        return int(hbx_ctx.add_dec_shares(np.frombuffer(bytes(b48), dtype=np.uint8).reshape(1, 48),
                                          np.array([j], dtype=np.uint32), np.array([i], dtype=np.uint32), n)[0])

    def plain():
        plains, st = hbx_ctx.combine_decrypt_cols(t, [J])
        assert st[J] == 0
        return plains[J]

    assert _add(hbx_ctx, d, [(J, i) for i in range(n)], n).tolist() == [VALID] * n
    before = hbx_ctx.share_status(p, n)
    pt = plain()
    _check_plain(d, J, pt, False)
    # VALID, then the sender's share of another proposer (the FaultyShareAdversary's message): the
    # item is INVALID, the entry keeps its point and status
    assert add_bytes(d["shares"][4, 3], J, 3) == INVALID
    np.testing.assert_array_equal(hbx_ctx.share_status(p, n), before)
    assert plain() == pt
    # undecodable bytes (not a field element, and the fixture's: one of them off the subgroup)
    junk = [bytes([0x9F]) + b"\xff" * 47] + [d["shares"][j, i].tobytes() for j, i in np.argwhere(exp == UNDECODABLE)]
    assert len(junk) == 3
    for b in junk:
        assert add_bytes(b, J, 0) == UNDECODABLE
        np.testing.assert_array_equal(hbx_ctx.share_status(p, n), before)
    assert plain() == pt
    # an entry that is not VALID takes the item's status: INVALID then VALID, UNDECODABLE then VALID
    assert add_bytes(d["shares"][J, 4], 4, 4) == INVALID
    assert hbx_ctx.share_status(p, n)[4, 4] == INVALID
    assert add_bytes(d["shares"][4, 4], 4, 4) == VALID
    assert add_bytes(junk[0], 4, 5) == UNDECODABLE
    assert hbx_ctx.share_status(p, n)[4, 5] == UNDECODABLE
    assert add_bytes(d["shares"][4, 5], 4, 5) == VALID
    want = before.copy()
    want[4, 4] = want[4, 5] = VALID
    np.testing.assert_array_equal(hbx_ctx.share_status(p, n), want)
    # unknown senders: the status, and no position touched
    for snd in (n, n + 5):
        assert add_bytes(d["shares"][J, 1], J, snd) == UNKNOWN_SENDER
        np.testing.assert_array_equal(hbx_ctx.share_status(p, n), want)
    # a proposer whose ciphertext is invalid
    assert d["expect_ct_status"][0] == 0
    assert add_bytes(d["shares"][0, 1], 0, 1) == SKIPPED_CT
    # argument errors, before anything is launched
    two = np.ascontiguousarray(d["shares"][J, :2])
    u32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    for prop, snd, nn in ((u32(J, J), u32(1, 1), n), (u32(J, p), u32(0, 1), n), (u32(J, J), u32(0, 1), n + 1)):
        with pytest.raises(HbxError) as e:
            hbx_ctx.add_dec_shares(two, prop, snd, nn)
        assert e.value.code == HBX_E_INVALID_ARG
    want[0, 1] = SKIPPED_CT
    np.testing.assert_array_equal(hbx_ctx.share_status(p, n), want)
    me = int(d["own_me"])
    hbx_ctx.set_own_share(me, d["own_sk"].tobytes())
    try:
        hbx_ctx.prepare_ciphertexts(_cts(d))
        with pytest.raises(HbxError) as e:
            hbx_ctx.add_dec_shares(two, u32(J, J), u32(0, me), n)
        assert e.value.code == HBX_E_INVALID_ARG
        assert _add(hbx_ctx, d, [], n).size == 0
        own = hbx_ctx.share_status(p, n)  # the matrix call with nothing present: this node's shares only
        assert (own[:, me] == d["expect_share_status_own"][:, me]).all() and (np.delete(own, me, 1) == ABSENT).all()
    finally:
        hbx_ctx.set_own_share(0, None)


# ---- 6. tile indexing at each lane shape ---------------------------------------------------------
def _model_tiles(positions, per):
    return len({(i // per, j) for j, i in positions})


def _pick_n64(d, per):
    """Present positions in at least three tiles of the shape, with the last (partial) tile and a
    position the fixture marks INVALID among them: the first seed for which that holds."""
    n = d["shares"].shape[1]
    cells = [(int(j), int(i)) for j, i in np.argwhere(d["present"])]
    for seed in range(1000):
        pick = random.Random(seed).sample(cells, 12)
        if _model_tiles(pick, per) >= 3 and any(i // per == (n - 1) // per for _, i in pick) and \
                any(d["expect_share_status"][j, i] == INVALID for j, i in pick):
            return pick
    raise AssertionError("no seed below 1000 meets the condition")


@pytest.mark.parametrize("lanes", [1, 2, 3, 6, 7])
def test_tile_list_launch_n64(hbx_ctx, lanes):
    d = _load("hb_epoch_n64")
    p, n = d["shares"].shape[:2]
    per = SENDERS[lanes]
    pick = _pick_n64(d, per)
    _set_keys(hbx_ctx, d)
    hbx_ctx.prepare_ciphertexts(_cts(d))
    hbx_ctx.set_verify_lanes(lanes)
    st = _add(hbx_ctx, d, pick, n)
    assert st.tolist() == [int(d["expect_share_status"][j, i]) for j, i in pick]
    assert hbx_ctx.verify_lanes_used() == lanes
    assert hbx_ctx.verify_tiles_used() == _model_tiles(pick, per) < -(-n // per) * p
    got = hbx_ctx.share_status(p, n)
    want = np.full((p, n), ABSENT, dtype=np.uint8)
    for (j, i), s in zip(pick, st):
        want[j, i] = s
    np.testing.assert_array_equal(got, want)


def _cols256_items(d):
    pos = [(j, i) for j in (1, 3) for i in (5, 70, 130, 255)]  # sender chunks 0, 1, 2, 3 of two columns
    assert all(d["present"][j, i] for j, i in pos)
    return pos


@pytest.mark.parametrize("lanes", [1, 7])
def test_tile_list_launch_n256(hbx_ctx, lanes):
    d = _load("hb_cols_n256")
    p, n = d["shares"].shape[:2]
    pos = _cols256_items(d)
    _set_keys(hbx_ctx, d)
    hbx_ctx.prepare_ciphertexts(_cts(d))
    hbx_ctx.set_verify_lanes(lanes)
    st = _add(hbx_ctx, d, pos, n)
    assert st.tolist() == [int(d["expect_share_status"][j, i]) for j, i in pos]
    assert hbx_ctx.verify_tiles_used() == 8 < 4 * p
    if lanes == 1:
        # the fallback path decides the even senders' checks, and counts items of the add only
        hbx_ctx.debug_force_fallback(2)
        try:
            pos2 = [(j, i + 1) for j, i in pos[:3]] + [(j, i - 1) for j, i in pos[3:4]] + [(0, 4), (2, 128)]
            st2 = _add(hbx_ctx, d, pos2, n)
            assert st2.tolist() == [int(d["expect_share_status"][j, i]) for j, i in pos2]
            assert hbx_ctx.fallback_lanes() == sum(1 for _, i in pos2 if i % 2 == 0) == 4
        finally:
            hbx_ctx.debug_force_fallback(0)


def test_lanes_follow_the_touched_tiles(hbx_ctx):
    """Automatic lanes: an add of 5 items takes six lanes per check.  (The matrix call on this shape,
    4 x 256, is 16 one-lane or 104 six-lane blocks and takes six lanes as well -- observed below; at
    256 x 256 it takes one lane, 1,024 blocks, where an add of 5 items still takes six.)"""
    d = _load("hb_cols_n256")
    p, n = d["shares"].shape[:2]
    _set_keys(hbx_ctx, d)
    hbx_ctx.prepare_ciphertexts(_cts(d))
    hbx_ctx.verify_dec_shares(d["shares"], np.zeros((p, n), dtype=bool))
    assert hbx_ctx.verify_lanes_used() == 6 and hbx_ctx.verify_tiles_used() == 26 * p
    pos = [(0, 3), (0, 200), (1, 9), (2, 77), (3, 255)]
    st = _add(hbx_ctx, d, pos, n)
    assert st.tolist() == [int(d["expect_share_status"][j, i]) for j, i in pos]
    assert hbx_ctx.verify_lanes_used() == 6
    assert hbx_ctx.verify_tiles_used() == 5


# ---- 7. column combine -------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [0, 1, 4])
@pytest.mark.parametrize("name", ["hb_epoch_n10", "hb_cols_n256"])
def test_combine_cols_writes_only_the_listed_proposers(hbx_ctx, name, lanes):
    d = _load(name)
    p, n = d["shares"].shape[:2]
    t = int(d["t"])
    off = d["v_off"].astype(np.int64)
    _set_keys(hbx_ctx, d)
    hbx_ctx.prepare_ciphertexts(_cts(d))
    hbx_ctx.verify_dec_shares(d["shares"], d["present"])
    hbx_ctx.set_combine_lanes(lanes)
    full, st_full = hbx_ctx.combine_decrypt(t)
    np.testing.assert_array_equal(st_full, d["expect_status"])
    cols = sorted(random.Random(name).sample(range(p), max(2, p // 2)))
    if name == "hb_epoch_n10":
        assert any(st_full[j] != 0 for j in cols) and any(st_full[j] == 0 for j in cols)
    out = np.full(int(off[-1]), 0xA5, dtype=np.uint8)
    status = np.full(p, -99, dtype=np.int32)
    plains, st = hbx_ctx.combine_decrypt_cols(t, cols[::-1], out=out, status=status)
    for j in range(p):
        rng = out[off[j]:off[j + 1]]
        if j in cols and st_full[j] == 0:
            assert status[j] == 0 and rng.tobytes() == full[j] == plains[j]
            _check_plain(d, j, rng.tobytes(), False)
        else:
            assert (rng == 0xA5).all(), j
            assert status[j] == (st_full[j] if j in cols else -99)
    assert hbx_ctx.combine_decrypt_cols(t, [])[0] == {}


def test_combine_cols_after_one_more_add(hbx_ctx):
    from hbbft_amd.hbx import HBX_E_NOT_ENOUGH_SHARES

    d = _load("hb_epoch_n10")
    p, n = d["shares"].shape[:2]
    t = int(d["t"])
    J = 6
    assert (d["expect_share_status"][J] == VALID).all()
    _set_keys(hbx_ctx, d)
    hbx_ctx.prepare_ciphertexts(_cts(d))
    assert _add(hbx_ctx, d, [(J, i) for i in (9, 2, 5)], n).tolist() == [VALID] * (t - 1)
    plains, st = hbx_ctx.combine_decrypt_cols(t, [J])
    assert st[J] == HBX_E_NOT_ENOUGH_SHARES and plains[J] is None
    assert _add(hbx_ctx, d, [(J, 7)], n).tolist() == [VALID]
    plains, st = hbx_ctx.combine_decrypt_cols(t, [J])
    assert st[J] == 0
    _check_plain(d, J, plains[J], False)


# ---- 8. the session on the engine -------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 5])
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_session_on_engine_matches_fixture(hbx_ctx, tag, every):
    import replay_fixture as rf

    from hbbft_amd.honey_badger import EpochSession

    d = rf.load(tag)
    hbx_ctx.set_digest(0)
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in d["pk_comp"]]) == 0).all()
    events = rf.events_of(d)
    try:
        ses = EpochSession(hbx_ctx, int(d["n"]), int(d["me"]), d["sk_me"].tobytes())
        faults, errors = [], []
        for k, ev in enumerate(events):
            ses.handle(ev)
            if (k + 1) % every == 0 or k + 1 == len(events):
                res = ses.flush()
                faults += res.faults
                errors += res.errors
    finally:
        hbx_ctx.set_own_share(0, None)
    want_faults, want_errors, want_batch = rf.expect(d)
    assert faults == ses.faults == want_faults
    assert errors == ses.errors == want_errors
    assert ses.batch == want_batch
    assert [ses.ct_status[int(j)] for j in d["acs_proposers"]] == d["expect_ct_status"].tolist()
    verified = 0
    for k, st in enumerate(ses.share_status):
        if st is not None:
            assert st == int(d["expect_ev_status"][k]) != rf.NO_STATUS, f"event {k}"
            verified += 1
    assert verified > 0
