"""The coin's incremental calls on the GPU (include/hbx.h hbx_add_sig_shares[_d],
hbx_combine_signatures_insts[_d]).  Yardsticks: the committed fixtures
tests/golden/coin_n*.npz, or, where stated, the unchanged matrix call on a second context."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
INVALID, VALID, ABSENT, UNDECODABLE, UNKNOWN_SENDER = 0, 1, 2, 3, 5
NOT_ENOUGH = -3  # HBX_E_NOT_ENOUGH_SHARES
FIXTURES = ["coin_n4", "coin_n7", "coin_n4_sha3", "coin_n128"]


@functools.lru_cache(maxsize=None)
def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def ctx2():
    """A second context: the unchanged matrix call on the same inputs, as yardstick."""
    from hbbft_amd.hbx import Context

    c = Context(0)
    yield c
    c.close()


def _setup(ctx, d, lanes=0):
    from hbbft_amd.hbx import DIGEST_SHA3_256, DIGEST_SHA256

    ctx.set_digest(DIGEST_SHA3_256 if str(d.get("digest", "sha256")) == "sha3_256" else DIGEST_SHA256)
    ctx.set_verify_lanes(lanes)
    assert (ctx.set_pk_shares([r.tobytes() for r in d["pk_comp"]]) == 0).all()
    off = d["nonce_off"]
    ctx.prepare_nonces([d["nonce_blob"][int(off[j]):int(off[j + 1])].tobytes() for j in range(len(off) - 1)], hashes=False)
    return d["sigs"].shape[:2]


def _add(ctx, d, positions, n):
    """One add of the fixture's bytes at `positions` [(inst, sender)] -> status bytes."""
    pos = np.array(positions, dtype=np.int64).reshape(-1, 2)
    sigs = np.ascontiguousarray(d["sigs"][pos[:, 0], pos[:, 1]]) if len(pos) else np.zeros((0, 96), np.uint8)
    return ctx.add_sig_shares(sigs, pos[:, 0], pos[:, 1], n)


def _mask(shape, positions):
    m = np.zeros(shape, dtype=bool)
    for q, i in positions:
        m[q, i] = True
    return m


def _check_full_combine(ctx, d):
    sig, st, ok, par = ctx.combine_signatures(d["master_pk"].tobytes(), int(d["t"]))
    np.testing.assert_array_equal(st, d["expect_status"])
    good = st == 0
    np.testing.assert_array_equal(sig[good], d["expect_sig"][good])
    np.testing.assert_array_equal(ok[good], d["expect_master_ok"][good])
    np.testing.assert_array_equal(par[good], d["expect_parity"][good])
    assert not ok[~good].any()


# ---- 1. partition equivalence ---------------------------------------------------------------------
@pytest.mark.parametrize("first", ["matrix", "add"])
@pytest.mark.parametrize("lanes", [0, 1, 2])
@pytest.mark.parametrize("name", FIXTURES)
def test_partition_into_adds_equals_one_matrix_call(hbx_ctx, ctx2, name, lanes, first):
    d = _load(name)
    count, n = _setup(hbx_ctx, d, lanes)
    _setup(ctx2, d, lanes)
    cells = [(int(q), int(i)) for q, i in np.argwhere(d["present"])]
    random.Random(20240607).shuffle(cells)
    cut = [0, len(cells) // 3, 2 * len(cells) // 3, len(cells)]
    groups = [cells[cut[g]:cut[g + 1]] for g in range(3)]
    assert all(groups) and sum(len(g) for g in groups) == int(d["present"].sum())
    exp = d["expect_share_status"]
    delivered = []
    for g, group in enumerate(groups):
        if g == 0 and first == "matrix":
            hbx_ctx.verify_sig_shares(d["sigs"], _mask((count, n), group))
            st = hbx_ctx.sig_share_status(count, n)[tuple(np.array(group).T)]
        else:
            st = _add(hbx_ctx, d, group, n)
        np.testing.assert_array_equal(st, exp[tuple(np.array(group).T)])
        delivered += group
        ctx2.verify_sig_shares(d["sigs"], _mask((count, n), delivered))
        np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), ctx2.sig_share_status(count, n))
    assert hbx_ctx.coin_lanes_used() == (lanes or 2)
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), exp)
    _check_full_combine(hbx_ctx, d)


# ---- 2. merge rule --------------------------------------------------------------------------------
def test_merge_rule(hbx_ctx):
    from hbbft_amd.hbx import HBX_E_INVALID_ARG, HbxError

    d = _load("coin_n7")
    count, n = _setup(hbx_ctx, d)
    exp, sigs, mpk, t = d["expect_share_status"], d["sigs"], d["master_pk"].tobytes(), int(d["t"])
    # a VALID share of the same sender in another instance is INVALID here; the fixture's two
    # UNDECODABLE shares are the cofactor-part one (0, 1) and the non-point (1, 0)
    assert (exp[0:2, 3:6] == VALID).all() and exp[0, 1] == UNDECODABLE and exp[1, 0] == UNDECODABLE
    foreign3, cof, junk = sigs[1, 3:4], sigs[0, 1:2], sigs[1, 0:1]

    # INVALID, UNDECODABLE (not a point) and UNDECODABLE (cofactor part) entries ...
    st = hbx_ctx.add_sig_shares(np.concatenate([foreign3, junk, cof]), [0, 0, 0], [3, 4, 5], n)
    assert st.tolist() == [INVALID, UNDECODABLE, UNDECODABLE]
    want = np.full((count, n), ABSENT, np.uint8)
    want[0, 3:6] = st
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), want)
    # ... become VALID when the valid bytes arrive in a later call
    assert _add(hbx_ctx, d, [(0, 3), (0, 4), (0, 5)], n).tolist() == [VALID] * 3
    want[0, 3:6] = VALID
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), want)
    # the rest of the round: the fixture's matrix and signatures (instance 0 combines senders 0, 2, 3)
    _add(hbx_ctx, d, [(int(q), int(i)) for q, i in np.argwhere(d["present"]) if not (q == 0 and 3 <= i <= 5)], n)
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), exp)
    _check_full_combine(hbx_ctx, d)
    sig0 = hbx_ctx.combine_signatures(mpk, t)[0].copy()

    # VALID then INVALID bytes in a later call: the entry stays, the item is INVALID, the combine unchanged
    assert hbx_ctx.add_sig_shares(foreign3, [0], [3], n).tolist() == [INVALID]
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), exp)
    np.testing.assert_array_equal(hbx_ctx.combine_signatures(mpk, t)[0], sig0)
    # ... and VALID then UNDECODABLE, both kinds
    assert hbx_ctx.add_sig_shares(np.concatenate([junk, cof]), [0, 0], [3, 2], n).tolist() == [UNDECODABLE] * 2
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), exp)
    np.testing.assert_array_equal(hbx_ctx.combine_signatures(mpk, t)[0], sig0)

    # sender >= n: what serde would say, and no position touched
    before = hbx_ctx.sig_share_status(count, n).copy()
    st = hbx_ctx.add_sig_shares(np.concatenate([sigs[0, 0:1], junk, cof, sigs[1, 1:2]]), [0, 0, 1, 2],
                                [n, n + 1, n + 5, 0xFFFFFFFF], n)
    assert st.tolist() == [UNKNOWN_SENDER, UNDECODABLE, UNDECODABLE, UNKNOWN_SENDER]
    assert hbx_ctx.coin_tiles_used() == 0
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), before)

    # rejected before anything is launched: the matrix is byte-identical
    two = np.concatenate([sigs[0, 0:1], sigs[0, 2:3]])
    for args in ((two, [0, 0], [2, 2], n), (two, [0, count], [0, 2], n), (two, [0, 0], [0, 2], n + 1),
                 (two, [1, 1], [n + 3, n + 3], n)):
        with pytest.raises(HbxError) as e:
            hbx_ctx.add_sig_shares(*args)
        assert e.value.code == HBX_E_INVALID_ARG
        np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), before)
    np.testing.assert_array_equal(hbx_ctx.combine_signatures(mpk, t)[0][:2], sig0[:2])


# ---- 3. tiles -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes,tiles", [(2, 3), (1, 2)])
def test_add_launches_the_touched_tiles(hbx_ctx, lanes, tiles):
    d = _load("coin_n128")
    count, n = _setup(hbx_ctx, d, lanes)
    exp = d["expect_share_status"]
    rest = [(int(q), int(i)) for q, i in np.argwhere(d["present"]) if not (q == 2 and i in (0, 31, 32, 127))]
    hbx_ctx.verify_sig_shares(d["sigs"], _mask((count, n), rest))
    matrix_tiles = hbx_ctx.coin_tiles_used()
    assert matrix_tiles == count * (n // (64 // lanes))
    before = hbx_ctx.sig_share_status(count, n).copy()
    pos = [(2, 127), (2, 0), (2, 32), (2, 31)]
    st = _add(hbx_ctx, d, pos, n)
    assert hbx_ctx.coin_tiles_used() == tiles and hbx_ctx.coin_lanes_used() == lanes
    np.testing.assert_array_equal(st, exp[tuple(np.array(pos).T)])
    after = hbx_ctx.sig_share_status(count, n)
    touched = _mask((count, n), pos)
    np.testing.assert_array_equal(after[~touched], before[~touched])
    np.testing.assert_array_equal(after, exp)
    # an add touching every position uses as many tiles as the matrix launch
    _add(hbx_ctx, d, [(q, i) for q in range(count) for i in range(n)], n)
    assert hbx_ctx.coin_tiles_used() == matrix_tiles
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), exp)


# ---- 4. forced fallback ---------------------------------------------------------------------------
def test_add_through_the_forced_fallback(hbx_ctx):
    d = _load("coin_n128")
    count, n = _setup(hbx_ctx, d, 2)
    cells = [(int(q), int(i)) for q, i in np.argwhere(d["present"])]
    hbx_ctx.debug_force_fallback(3)
    try:
        st = _add(hbx_ctx, d, cells, n)
        assert hbx_ctx.fallback_lanes() > 0
    finally:
        hbx_ctx.debug_force_fallback(0)
    np.testing.assert_array_equal(st, d["expect_share_status"][tuple(np.array(cells).T)])
    np.testing.assert_array_equal(hbx_ctx.sig_share_status(count, n), d["expect_share_status"])
    _add(hbx_ctx, d, cells[:40], n)
    assert hbx_ctx.fallback_lanes() == 0  # nothing reaches the fallback unforced


# ---- 5. listed combine ----------------------------------------------------------------------------
def _canaries(count):
    return (np.full((count, 96), 0xA5, np.uint8), np.full(count, 0x5A5A5A5A, np.int32), np.full(count, 0xA5, np.uint8),
            np.full(count, 0xA5, np.uint8))


@pytest.mark.parametrize("name", ["coin_n4", "coin_n128"])
def test_combine_insts_writes_only_the_listed_instances(hbx_ctx, ctx2, name):
    import torch

    from hbbft_amd.hbx import HBX_E_INVALID_ARG, HbxError

    d = _load(name)
    count, n = _setup(hbx_ctx, d)
    mpk, t = d["master_pk"].tobytes(), int(d["t"])
    _add(hbx_ctx, d, [(int(q), int(i)) for q, i in np.argwhere(d["present"])], n)
    sig, st, ok, par = hbx_ctx.combine_signatures_insts(mpk, t, [1], None, *_canaries(count))
    assert st[1] == 0 and ok[1] == 1 and par[1] == int(d["expect_parity"][1])
    np.testing.assert_array_equal(sig[1], d["expect_sig"][1])
    cs, cst, cok, cpar = _canaries(count)
    others = np.arange(count) != 1
    for got, canary in ((sig, cs), (st, cst), (ok, cok), (par, cpar)):
        np.testing.assert_array_equal(got[others], canary[others])
    # ninsts == 0 writes nothing; a repeated or out-of-range instance is rejected
    out = hbx_ctx.combine_signatures_insts(mpk, t, [], None, *_canaries(count))
    for got, canary in zip(out, _canaries(count)):
        np.testing.assert_array_equal(got, canary)
    dev = torch.device("cuda", hbx_ctx.device)
    d_st = torch.full((count,), 77, dtype=torch.int32, device=dev)
    hbx_ctx.combine_signatures_insts_d(mpk, t, [], d_status=d_st)
    for bad in ([count], [0, 0xFFFFFFFF]):
        with pytest.raises(HbxError) as e:
            hbx_ctx.combine_signatures_insts_d(mpk, t, bad, d_status=d_st)
        assert e.value.code == HBX_E_INVALID_ARG
    # a repeated instance: the binding's guard, and the library's own behind it
    with pytest.raises(ValueError, match="listed twice"):
        hbx_ctx.combine_signatures_insts_d(mpk, t, [1, 1], d_status=d_st)
    twice = (ctypes.c_uint32 * 2)(1, 1)
    key = (ctypes.c_uint8 * 48).from_buffer_copy(mpk)
    assert hbx_ctx.lib.hbx_combine_signatures_insts_d(hbx_ctx.h, key, t, twice, 2, None, None, d_st.data_ptr(), None, None,
                                                      None) == HBX_E_INVALID_ARG
    assert (d_st.cpu().numpy() == 77).all()
    if name == "coin_n4":
        # the starved instance: HBX_E_NOT_ENOUGH_SHARES in its status entry only
        starved = int(np.flatnonzero(d["expect_status"] == NOT_ENOUGH)[0])
        sig, st, ok, par = hbx_ctx.combine_signatures_insts(mpk, t, [starved], None, *_canaries(count))
        assert st[starved] == NOT_ENOUGH and ok[starved] == 0
        assert (st[np.arange(count) != starved] == 0x5A5A5A5A).all()
    # with a use mask: the matrix combine with the same mask on the second context (device forms)
    _setup(ctx2, d)
    ctx2.verify_sig_shares(d["sigs"], d["present"])
    rng = np.random.default_rng(11)
    use = (rng.random((count, n)) < 0.8).astype(np.uint8)
    dev2 = torch.device("cuda", ctx2.device)
    ref = [torch.zeros((count, 96), dtype=torch.uint8, device=dev2), torch.zeros(count, dtype=torch.int32, device=dev2),
           torch.zeros(count, dtype=torch.uint8, device=dev2), torch.zeros(count, dtype=torch.uint8, device=dev2)]
    ctx2.combine_signatures_d(mpk, t, torch.from_numpy(use).to(dev2), *ref)
    listed = [count - 1, 0]
    got = [torch.from_numpy(c).to(dev) for c in _canaries(count)]
    hbx_ctx.combine_signatures_insts_d(mpk, t, listed, torch.from_numpy(use).to(dev), *got)
    torch.cuda.synchronize()
    for g, r, canary in zip(got, ref, _canaries(count)):
        g, r = g.cpu().numpy(), r.cpu().numpy()
        np.testing.assert_array_equal(g[listed], r[listed])
        rest = np.setdiff1d(np.arange(count), listed)
        np.testing.assert_array_equal(g[rest], canary[rest])
    host = hbx_ctx.combine_signatures_insts(mpk, t, listed, use)
    for h, r in zip(host, ref):
        np.testing.assert_array_equal(h[listed], r.cpu().numpy()[listed])


# ---- 6. the threshold moment ----------------------------------------------------------------------
def test_listed_combine_at_the_threshold(hbx_ctx):
    d = _load("coin_n7")
    count, n = _setup(hbx_ctx, d)
    mpk, t = d["master_pk"].tobytes(), int(d["t"])
    valid = [int(i) for i in np.flatnonzero(d["expect_share_status"][0] == VALID)]
    assert len(valid) >= t
    hbx_ctx.add_sig_shares(np.zeros((0, 96), np.uint8), [], [], n)  # the empty matrix
    sig, st, ok, par = hbx_ctx.combine_signatures_insts(mpk, t, [0])
    assert st[0] == NOT_ENOUGH
    for i in valid[:t - 1]:
        assert _add(hbx_ctx, d, [(0, i)], n).tolist() == [VALID]
    sig, st, ok, par = hbx_ctx.combine_signatures_insts(mpk, t, [0])
    assert st[0] == NOT_ENOUGH and ok[0] == 0 and not sig[0].any()
    assert _add(hbx_ctx, d, [(0, valid[t - 1])], n).tolist() == [VALID]
    sig, st, ok, par = hbx_ctx.combine_signatures_insts(mpk, t, [0])
    assert st[0] == 0 and ok[0] == 1 and par[0] == int(d["expect_parity"][0])
    np.testing.assert_array_equal(sig[0], d["expect_sig"][0])


# ---- 7. CoinSession on the engine -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scenario(n, me, count, seed):
    from coin_scenarios import coin_scenario
    from oracle import bls12_381 as bls
    from oracle import common_coin as oc

    ns, sks, pks, events = coin_scenario(n, me, count, seed)
    sk = None if me is None else sks.secret_key_share(me)
    node = oc.CoinNode(n, me, pks, sk, ns).run(events)
    pk48 = [bls.g1_compress(pks.public_key_share(i)) for i in range(n)]
    return ns, events, node, pk48, bls.g1_compress(pks.public_key()), None if sk is None else sk.to_bytes(32, "big")


def _cases():
    from test_coin_replay import CASES

    return CASES


@pytest.mark.parametrize("every", [1, 5, None])
@pytest.mark.parametrize("case", range(4))
def test_session_on_engine_matches_the_reference(hbx_ctx, case, every):
    from coin_scenarios import check_against_oracle
    from hbbft_amd.common_coin import CoinResult, CoinSession

    n, me, count, seed = _cases()[case]
    ns, events, node, pk48, mpk, sk32 = _scenario(n, me, count, seed)
    hbx_ctx.set_pk_shares(pk48)
    session = CoinSession(hbx_ctx, mpk, n, me, sk32)
    session.prepare(ns)
    acc = CoinResult()

    def flush():
        r = session.flush()
        for name in ("faults", "errors", "sent", "outputs", "combines"):
            getattr(acc, name).extend(getattr(r, name))

    for k, ev in enumerate(events):
        session.handle(ev)
        if every and (k + 1) % every == 0:
            flush()
    flush()
    check_against_oracle(acc, node)
    assert hbx_ctx.coin_lanes_used() == 2


# ---- 8. lifetime ----------------------------------------------------------------------------------
def test_buffers_of_adds_and_listed_combines_are_freed():
    from hbbft_amd import hbx

    d = _load("coin_n7")
    start = hbx.live_buffers()
    with hbx.Context(0) as c:
        count, n = _setup(c, d)
        _add(c, d, [(int(q), int(i)) for q, i in np.argwhere(d["present"])], n)
        c.combine_signatures_insts(d["master_pk"].tobytes(), int(d["t"]), [0, 1], np.ones((count, n), np.uint8))
        assert c.add_sig_shares(d["sigs"][0, 0:1], [0], [n + 1], n).tolist() == [UNKNOWN_SENDER]
        assert hbx.live_buffers() > start
    assert hbx.live_buffers() == start


# ---- 9. both kinds of add on one context ----------------------------------------------------------
def test_interleaved_decryption_and_coin_adds_equal_separate_contexts():
    """Decryption adds and coin adds alternate on one context (each has its own add state, both pack
    their items into the same pinned staging): per-item statuses and both matrices are what two
    contexts leave that run one kind each.  One context holds one key set, so the coin shares are
    signed under hb_epoch_n4's keys at coin_n4's present positions, except where coin_n4's own bytes
    give the other statuses: its undecodable shares, and one share of its (here foreign) keys."""
    from hbbft_amd import hbx

    e, cn = _load("hb_epoch_n4"), _load("coin_n4")
    p, n = e["shares"].shape[:2]
    count = cn["sigs"].shape[0]
    keys = [r.tobytes() for r in e["pk_comp"]]
    v_off, n_off = e["v_off"], cn["nonce_off"]
    cts = [(e["u"][j].tobytes(), e["v_blob"][int(v_off[j]):int(v_off[j + 1])].tobytes(), e["w"][j].tobytes()) for j in range(p)]
    nonces = [cn["nonce_blob"][int(n_off[q]):int(n_off[q + 1])].tobytes() for q in range(count)]
    dec_pos, coin_pos = np.argwhere(e["present"]), np.argwhere(cn["present"])
    halves = {"dec": [dec_pos[0::2], dec_pos[1::2]], "coin": [coin_pos[0::2], coin_pos[1::2]]}
    assert all(0 < len(h) < len(dec_pos) for h in halves["dec"]) and all(0 < len(h) < len(coin_pos) for h in halves["coin"])

    start = hbx.live_buffers()
    with hbx.Context(0) as dec_only, hbx.Context(0) as coin_only, hbx.Context(0) as both:
        for c in (dec_only, coin_only, both):
            assert (c.set_pk_shares(keys) == 0).all()
        for c in (dec_only, both):
            c.prepare_ciphertexts(cts)
        for c in (coin_only, both):
            c.prepare_nonces(nonces, hashes=False)
        sigs = coin_only.sign(e["sk_shares"])
        other = (cn["expect_share_status"] == UNDECODABLE) | _mask((count, n), [tuple(coin_pos[0])])
        sigs[other] = cn["sigs"][other]

        def add(ctx, kind, k):
            pos = halves[kind][k]
            if kind == "dec":
                return ctx.add_dec_shares(np.ascontiguousarray(e["shares"][pos[:, 0], pos[:, 1]]), pos[:, 0], pos[:, 1], n)
            return ctx.add_sig_shares(np.ascontiguousarray(sigs[pos[:, 0], pos[:, 1]]), pos[:, 0], pos[:, 1], n)

        order = [("dec", 0), ("coin", 0), ("dec", 1), ("coin", 1)]
        want = {(kind, k): add(dec_only if kind == "dec" else coin_only, kind, k) for kind, k in order}
        for kind, k in order:
            np.testing.assert_array_equal(add(both, kind, k), want[(kind, k)], err_msg=f"{kind} add {k}")
        np.testing.assert_array_equal(both.share_status(p, n), dec_only.share_status(p, n))
        np.testing.assert_array_equal(both.sig_share_status(count, n), coin_only.sig_share_status(count, n))
        # the yardsticks themselves: the epoch fixture's matrix; every kind of coin status present
        np.testing.assert_array_equal(dec_only.share_status(p, n), e["expect_share_status"])
        coin_st = np.concatenate([want[("coin", 0)], want[("coin", 1)]])
        assert {VALID, INVALID, UNDECODABLE} <= set(coin_st.tolist())
        assert hbx.live_buffers() > start
    assert hbx.live_buffers() == start
