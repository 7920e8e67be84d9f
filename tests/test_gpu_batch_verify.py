"""GPU: batched decryption-share verification by random linear combination (hbx_set_batch_verify).

Every status the per-share path writes must come out byte-equal in batched mode, and the column
counters (hbx_get_batch_stats) must equal what the fixture arrays alone say: that is what keeps a
broken multi-scalar sum from hiding behind the per-share fallback.  Shapes: n = 4, 7, 10, 64 and 256
from the committed epoch fixtures, n = 65 and 129 as sender slices of hb_cols_n256 (statuses per
share do not depend on other senders, so the expected arrays slice too): 65 and 129 cross a wave
boundary of the block reduction, 7 and 10 leave a wave mostly empty."""
import hashlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
FIXTURES = ["hb_epoch_n4", "hb_epoch_n7", "hb_epoch_n10", "hb_epoch_n64", "hb_cols_n256", "hb_epoch_n7_sha3"]
SLICES = [("hb_cols_n256", 65), ("hb_cols_n256", 129)]
CASES = [(name, None) for name in FIXTURES] + SLICES
SEED = hashlib.sha256(b"test_gpu_batch_verify").digest()
INF48 = np.frombuffer(bytes([0xC0]) + bytes(47), dtype=np.uint8)

_cache = {}


def _load(name, n=None):
    """The fixture, optionally cut to its first n senders (keys, shares, presence, expectations)."""
    if (name, n) not in _cache:
        d = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
        if n is not None:
            d["pk_comp"] = d["pk_comp"][:n]
            for k in ("shares", "present", "expect_share_status", "expect_valid"):
                d[k] = np.ascontiguousarray(d[k][:, :n])
            # combine: the first t valid shares of the slice where it has that many (any t valid
            # shares give the fixture's plaintext), NotEnoughShares (-3) where it does not
            enough = (d["expect_share_status"] == 1).sum(axis=1) >= int(d["t"])
            d["expect_status"] = np.where((d["expect_status"] == 0) & ~enough, -3, d["expect_status"]).astype(np.int32)
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[(name, n)] = d
    return _cache[(name, n)]


def _cts(d):
    off = d["v_off"]
    return [(d["u"][j].tobytes(), d["v_blob"][int(off[j]):int(off[j + 1])].tobytes(), d["w"][j].tobytes())
            for j in range(len(off) - 1)]


def _set_keys(ctx, d):
    from hbbft_amd.hbx import DIGEST_SHA3_256, DIGEST_SHA256

    ctx.set_digest(DIGEST_SHA3_256 if str(d["digest"]) == "sha3_256" else DIGEST_SHA256)
    assert (ctx.set_pk_shares([row.tobytes() for row in d["pk_comp"]]) == 0).all()


def _classes(d, share_status, eager):
    """(batched, fallback, skipped) from the fixture arrays alone.  `eager`: Ciphertext::verify ran in
    the prepare (three-call host API); else it is part of the verification (fused call)."""
    ct = d["expect_ct_status"]
    ident = ((d["u"][:, 0] & 0x40) | (d["w"][:, 0] & 0x40)) != 0
    skipped = (ct == 3) | ((ct == 0) & eager)
    fallback = ~skipped & ((ct == 0) | (share_status == 0).any(axis=1) | ident)
    return int((~skipped & ~fallback).sum()), int(fallback.sum()), int(skipped.sum())


def _host_epoch(ctx, d, shares=None, present=None):
    """Three-call host API -> (ct valid bits, ct status, valid bits, share status, combine status, plaintexts)."""
    p, n = d["shares"].shape[:2]
    ct_ok = ctx.prepare_ciphertexts(_cts(d))
    ct_st = ctx.ct_status(p)
    valid = ctx.verify_dec_shares(d["shares"] if shares is None else shares, d["present"] if present is None else present)
    st = ctx.share_status(p, n)
    stats = ctx.batch_stats()
    plains, status = ctx.combine_decrypt(int(d["t"]))
    return dict(ct_ok=ct_ok, ct_st=ct_st, valid=valid, st=st, stats=stats, status=status, plains=plains)


def _device_epoch(ctx, d, shares=None, present=None):
    """hbx_decrypt_epoch_d -> the same arrays (Ciphertext::verify deferred into the verification)."""
    import torch

    dev = torch.device("cuda", 0)
    p, n = d["shares"].shape[:2]
    off = d["v_off"].astype(np.int64)
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)  # noqa: E731  (a writable copy)
    t_v = up(d["v_blob"].copy() if len(d["v_blob"]) else np.zeros(1, np.uint8))
    t_out = torch.zeros(max(int(off[-1]), 1), dtype=torch.uint8, device=dev)
    t_valid = torch.zeros(p * n, dtype=torch.uint8, device=dev)
    t_ct = torch.zeros(p, dtype=torch.uint8, device=dev)
    t_st = torch.zeros(p, dtype=torch.int32, device=dev)
    ctx.decrypt_epoch_d(up(d["u"]), t_v, up(off), up(d["w"]), p, int(np.max(np.diff(off))) if p else 0,
                        up(d["shares"] if shares is None else shares), n, int(d["t"]), t_out, d_valid=t_valid,
                        d_ct_valid=t_ct, d_status=t_st,
                        d_present=up(np.asarray(d["present"] if present is None else present).astype(np.uint8)))
    status = t_st.cpu().numpy()
    out = t_out.cpu().numpy()
    plains = [out[off[j]:off[j + 1]].tobytes() if status[j] == 0 else None for j in range(p)]
    st = t_valid.cpu().numpy().reshape(p, n)
    return dict(ct_st=t_ct.cpu().numpy(), st=st, valid=st == 1, stats=ctx.batch_stats(), status=status, plains=plains)


def _check(res, d, sfx="", share_status=None, valid=None):
    want_st = d["expect_share_status" + sfx] if share_status is None else share_status
    np.testing.assert_array_equal(res["ct_st"], d["expect_ct_status"])
    if "ct_ok" in res:
        np.testing.assert_array_equal(res["ct_ok"], d["expect_ct_valid"])
    np.testing.assert_array_equal(res["st"], want_st)
    np.testing.assert_array_equal(res["valid"], want_st == 1 if valid is None else valid)
    if share_status is None:
        np.testing.assert_array_equal(res["valid"], d["expect_valid" + sfx])
        np.testing.assert_array_equal(res["status"], d["expect_status" + sfx])
        key = "expect_plain_sha_own" if sfx else "expect_plain_sha"
        for j, pt in enumerate(res["plains"]):
            if res["status"][j] == 0:
                assert hashlib.sha256(pt).digest() == d[key][j].tobytes(), f"plaintext {j}"


# ---- 1. fixtures in batched mode, three forms ----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,n", CASES)
def test_batched_host_api_matches_golden(hbx_ctx, name, n):
    d = _load(name, n)
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_batch_verify(SEED)
    try:
        res = _host_epoch(hbx_ctx, d)
    finally:
        hbx_ctx.set_batch_verify(None)
    _check(res, d)
    assert res["stats"] == _classes(d, d["expect_share_status"], eager=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,n", CASES)
def test_batched_fused_call_matches_golden(hbx_ctx, name, n):
    d = _load(name, n)
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_batch_verify(SEED)
    try:
        res = _device_epoch(hbx_ctx, d)
    finally:
        hbx_ctx.set_batch_verify(None)
    _check(res, d)
    assert res["stats"] == _classes(d, d["expect_share_status"], eager=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_batched_own_share_mode_matches_golden(hbx_ctx, name):
    """The own share is included like any other, and its column's equation decides Ciphertext::verify."""
    d = _load(name)
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_own_share(int(d["own_me"]), d["own_sk"].tobytes())
    hbx_ctx.set_batch_verify(SEED)
    try:
        res_h = _host_epoch(hbx_ctx, d)
        res_d = _device_epoch(hbx_ctx, d)
    finally:
        hbx_ctx.set_batch_verify(None)
        hbx_ctx.set_own_share(0, None)
    _check(res_h, d, "_own")
    assert res_h["stats"] == _classes(d, d["expect_share_status_own"], eager=True)
    _check(res_d, d, "_own")
    assert res_d["stats"] == _classes(d, d["expect_share_status_own"], eager=False)


# ---- 2. honest columns take no fallback ----------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,n", CASES)
def test_honest_columns_take_no_fallback(hbx_ctx, name, n):
    """Every share the fixture expects INVALID marked absent: only the deferred-invalid and the
    identity ciphertexts reach the per-share path, and the statuses are the fixture's with those
    shares ABSENT."""
    d = _load(name, n)
    _set_keys(hbx_ctx, d)
    bad = d["expect_share_status"] == 0
    present = d["present"] & ~bad
    want = np.where(bad, 2, d["expect_share_status"]).astype(np.uint8)
    ct = d["expect_ct_status"]
    ident = (((d["u"][:, 0] & 0x40) | (d["w"][:, 0] & 0x40)) != 0) & (ct == 1)
    hbx_ctx.set_batch_verify(SEED)
    try:
        res_h = _host_epoch(hbx_ctx, d, present=present)
        res_d = _device_epoch(hbx_ctx, d, present=present)
    finally:
        hbx_ctx.set_batch_verify(None)
    _check(res_h, d, share_status=want)
    _check(res_d, d, share_status=want)
    assert res_h["stats"][1] == int(ident.sum())
    assert res_d["stats"][1] == int(ident.sum()) + int((ct == 0).sum())
    assert res_h["stats"] == _classes(d, want, eager=True)
    assert res_d["stats"] == _classes(d, want, eager=False)


# ---- 3. the sums against the oracle's ------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key,name,n", [("n7", "hb_epoch_n7", None), ("c65", "hb_cols_n256", 65),
                                        ("c256", "hb_cols_n256", None)])
def test_batch_sums_match_oracle(hbx_ctx, key, name, n):
    """hbx_get_batch_sums equals tests/golden/batch_sums.npz at call index 0, then 1 (the index
    advances per verification), and index 0 again after the seed is set again."""
    g = dict(np.load(os.path.join(GOLDEN, "batch_sums.npz"), allow_pickle=False))
    d = _load(name, n)
    p = d["shares"].shape[0]
    _set_keys(hbx_ctx, d)
    seed = g["seed"].tobytes()
    hbx_ctx.set_batch_verify(seed)
    try:
        hbx_ctx.prepare_ciphertexts(_cts(d))
        for k in (0, 1):
            hbx_ctx.verify_dec_shares(d["shares"], d["present"])
            np.testing.assert_array_equal(hbx_ctx.batch_sums(p), g[f"sums_{key}_{k}"], err_msg=f"call index {k}")
        hbx_ctx.set_batch_verify(seed)
        hbx_ctx.verify_dec_shares(d["shares"], d["present"])
        np.testing.assert_array_equal(hbx_ctx.batch_sums(p), g[f"sums_{key}_0"])
    finally:
        hbx_ctx.set_batch_verify(None)
    assert not (g[f"sums_{key}_0"] == g[f"sums_{key}_1"]).all()


# ---- 4. adversarial inputs made by byte moves ----------------------------------------------------
def _swap(sh, a, b):
    sh[a], sh[b] = sh[b].copy(), sh[a].copy()


def _adversarial(kind, shares):
    """Byte moves on columns 0 and 1 (clean in the fixture) -> the (column, sender) pairs now invalid."""
    n = shares.shape[1]
    a, b = 1, n - 2
    if kind == "swap_senders":
        _swap(shares, (0, a), (0, b))
        return [(0, a), (0, b)]
    if kind == "copy":
        shares[0, b] = shares[0, a]
        return [(0, b)]
    if kind == "swap_columns":
        _swap(shares, (0, a), (1, a))
        return [(0, a), (1, a)]
    if kind == "negate":
        shares[0, b, 0] ^= 0x20
        return [(0, b)]
    if kind == "negated_copy":  # S_b := -S_a: opposite points meet in the column's sum
        shares[0, b] = shares[0, a]
        shares[0, b, 0] ^= 0x20
        return [(0, b)]
    raise AssertionError(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["swap_senders", "copy", "swap_columns", "negate", "negated_copy"])
@pytest.mark.parametrize("name,n", [("hb_epoch_n64", None), ("hb_cols_n256", 129)])
def test_adversarial_byte_moves(hbx_ctx, name, n, kind):
    d = _load(name, n)
    assert (d["expect_share_status"][:2] == 1).all()  # columns 0 and 1 are clean
    shares = d["shares"].copy()
    bad = _adversarial(kind, shares)
    want = d["expect_share_status"].copy()
    for j, i in bad:
        want[j, i] = 0
    _set_keys(hbx_ctx, d)
    ref = _device_epoch(hbx_ctx, d, shares=shares)  # per-share mode: the reference
    assert ref["stats"] == (0, 0, 0)
    hbx_ctx.set_batch_verify(SEED)
    try:
        res = _device_epoch(hbx_ctx, d, shares=shares)
    finally:
        hbx_ctx.set_batch_verify(None)
    np.testing.assert_array_equal(res["st"], want)
    np.testing.assert_array_equal(res["st"], ref["st"])
    np.testing.assert_array_equal(res["ct_st"], ref["ct_st"])
    np.testing.assert_array_equal(res["status"], ref["status"])
    assert res["plains"] == ref["plains"]
    assert res["stats"] == _classes(d, want, eager=False)
    clean = _classes(d, d["expect_share_status"], eager=False)
    assert res["stats"][1] == clean[1] + len({j for j, _ in bad})


# ---- 5. mode plumbing ----------------------------------------------------------------------------
@pytest.mark.gpu
def test_clearing_the_seed_restores_per_share_mode(hbx_ctx):
    d = _load("hb_epoch_n10")
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_batch_verify(SEED)
    try:
        res = _host_epoch(hbx_ctx, d)
        assert res["stats"][0] > 0
    finally:
        hbx_ctx.set_batch_verify(None)
    res = _host_epoch(hbx_ctx, d)
    assert res["stats"] == (0, 0, 0)
    _check(res, d)
    from hbbft_amd.hbx import HbxError

    with pytest.raises(HbxError):
        hbx_ctx.batch_sums(d["shares"].shape[0])  # the last verification was not batched


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,force", [(1, 0), (6, 0), (7, 0), (1, 3)])
def test_batched_mode_keeps_lane_selection(hbx_ctx, lanes, force):
    """hbx_set_verify_lanes / hbx_debug_force_fallback apply to the per-share launch over the columns
    that failed their equation: same statuses, plain and own-share mode."""
    d = _load("hb_epoch_n10")
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_verify_lanes(lanes)
    hbx_ctx.debug_force_fallback(force)
    hbx_ctx.set_batch_verify(SEED)
    try:
        res = _device_epoch(hbx_ctx, d)
        assert hbx_ctx.verify_lanes_used() == lanes
        if force:
            assert hbx_ctx.fallback_lanes() > 0
        _check(res, d)
        assert res["stats"] == _classes(d, d["expect_share_status"], eager=False)
        hbx_ctx.set_own_share(int(d["own_me"]), d["own_sk"].tobytes())
        try:
            res = _device_epoch(hbx_ctx, d)
        finally:
            hbx_ctx.set_own_share(0, None)
        _check(res, d, "_own")
    finally:
        hbx_ctx.set_batch_verify(None)
        hbx_ctx.debug_force_fallback(0)
        hbx_ctx.set_verify_lanes(0)


@pytest.mark.gpu
def test_three_lane_and_two_lane_checks_in_batched_mode(hbx_ctx):
    d = _load("hb_epoch_n7")
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_batch_verify(SEED)
    try:
        for lanes in (2, 3):
            hbx_ctx.set_verify_lanes(lanes)
            _check(_device_epoch(hbx_ctx, d), d)
    finally:
        hbx_ctx.set_batch_verify(None)
        hbx_ctx.set_verify_lanes(0)


# ---- 6. the replay driver ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_epoch_replay_with_batch_seed(hbx_ctx, tag):
    from make_replay import load_events

    from hbbft_amd.honey_badger import EpochReplay

    d = dict(np.load(os.path.join(GOLDEN, f"hb_replay_{tag}.npz"), allow_pickle=False))
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in d["pk_comp"]]) == 0).all()
    events = load_events(d)
    args = (hbx_ctx, int(d["n"]), int(d["me"]), d["sk_me"].tobytes())
    try:
        plain = EpochReplay(*args).run(events)
        batched = EpochReplay(*args, batch_seed=SEED).run(events)
        assert sum(hbx_ctx.batch_stats()) == len(d["acs_proposers"])  # its last verification was batched
        again = EpochReplay(*args).run(events)
    finally:
        hbx_ctx.set_own_share(0, None)
    assert batched == plain
    assert again == plain
