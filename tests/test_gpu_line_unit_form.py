"""GPU: the one-lane Miller kernel over lines divided by their constant term (k_verify_shares_ml on
k_normalise_lines' second table, pairingd.hpp miller_loop2_unit_d) -- golden epochs byte for byte,
a two-wave-per-proposer case against the single-kernel check (which reads the first table), and
the path of a proposer whose lines have no such form (hbx_debug_force_degenerate)."""
import hashlib
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


def _set_keys(ctx, d):
    from hbbft_amd.hbx import DIGEST_SHA256

    ctx.set_digest(DIGEST_SHA256)
    assert (ctx.set_pk_shares([row.tobytes() for row in d["pk_comp"]]) == 0).all()


def _fused_epoch(ctx, d):
    """The fixture's epoch through hbx_decrypt_epoch_d (Ciphertext::verify deferred into the
    share-check launch): (ciphertext statuses, share statuses [p, n], combine statuses, plaintexts)."""
    import torch

    dev = torch.device("cuda", 0)
    p, n = d["shares"].shape[:2]
    off = d["v_off"].astype(np.int64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    t_u, t_w, t_off = up(d["u"]), up(d["w"]), up(off)
    t_v = up(d["v_blob"] if len(d["v_blob"]) else np.zeros(1, np.uint8))
    t_sh, t_pr = up(d["shares"]), up(d["present"].astype(np.uint8))
    t_out = torch.zeros(max(int(off[-1]), 1), dtype=torch.uint8, device=dev)
    t_valid = torch.zeros(p * n, dtype=torch.uint8, device=dev)
    t_ct = torch.zeros(p, dtype=torch.uint8, device=dev)
    t_st = torch.zeros(p, dtype=torch.int32, device=dev)
    ctx.decrypt_epoch_d(t_u, t_v, t_off, t_w, p, int(np.max(np.diff(off))), t_sh, n, int(d["t"]), t_out,
                        d_valid=t_valid, d_ct_valid=t_ct, d_status=t_st, d_present=t_pr)
    status = t_st.cpu().numpy()
    out = t_out.cpu().numpy()
    plains = [out[off[j]:off[j + 1]].tobytes() if status[j] == 0 else None for j in range(p)]
    return t_ct.cpu().numpy(), t_valid.cpu().numpy().reshape(p, n), status, plains


def _assert_golden(d, res, own):
    ct, valid, status, plains = res
    sfx = "_own" if own else ""
    np.testing.assert_array_equal(ct, d["expect_ct_status"])
    np.testing.assert_array_equal(valid, d["expect_share_status" + sfx])
    np.testing.assert_array_equal(status, d["expect_status" + sfx])
    for j, pt in enumerate(plains):
        if pt is not None:
            assert hashlib.sha256(pt).digest() == d["expect_plain_sha" + sfx][j].tobytes(), f"plaintext {j}"


def _assert_same(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    assert a[3] == b[3]


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True], ids=["plain", "own"])
@pytest.mark.parametrize("name", ["hb_epoch_n4", "hb_epoch_n10"])
def test_unit_form_kernel_matches_golden(hbx_ctx, name, own):
    """set_verify_lanes(1): share statuses, ciphertext statuses and plaintexts of the golden epochs,
    and nothing goes to the fallback."""
    d = _load(name)
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_verify_lanes(1)
    try:
        if own:
            hbx_ctx.set_own_share(int(d["own_me"]), d["own_sk"].tobytes())
        _assert_golden(d, _fused_epoch(hbx_ctx, d), own)
        assert hbx_ctx.verify_lanes_used() == 1
        assert hbx_ctx.fallback_lanes() == 0
    finally:
        hbx_ctx.set_own_share(0, None)
        hbx_ctx.set_verify_lanes(0)


@pytest.mark.gpu
def test_two_waves_per_proposer_match_single_kernel_check(hbx_ctx):
    """Two proposers at n = 65 (producer API; a few shares replaced by a foreign ciphertext's, as
    bench.py's epoch): two waves per proposer, the second with one live lane.  The one-lane step
    kernels (second table) and the single-kernel check (lanes 7, first table) agree byte for byte."""
    from hbbft_amd import netinfo

    n, p = 65, 2
    sks, sk_shares, master_sk = netinfo.generate_keys(n)
    pk_shares = hbx_ctx.public_keys(sk_shares)
    master_pk = hbx_ctx.public_keys(master_sk)[0].tobytes()
    rng = np.random.default_rng(0x756E6974)
    msgs = [rng.integers(0, 256, size=40, dtype=np.uint8).tobytes() for _ in range(p)] + [b"foreign ciphertext"]
    cts = hbx_ctx.encrypt(master_pk, msgs, netinfo.scalars_to_be32(netinfo.random_scalars(rng, p + 1)))
    u48 = np.stack([np.frombuffer(c[0], dtype=np.uint8) for c in cts])
    shares = hbx_ctx.decrypt_shares(sk_shares, u48)  # (p + 1, n, 48)
    sh = shares[:p].copy()
    swapped = [(0, 3), (0, 64), (1, 0), (1, 63), (1, 64)]  # both waves of both proposers, the lone lane included
    for j, i in swapped:
        sh[j, i] = shares[p, i]
    expect = np.ones((p, n), dtype=bool)
    for j, i in swapped:
        expect[j, i] = False
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in pk_shares]) == 0).all()
    got = {}
    try:
        for lanes in (1, 7):
            hbx_ctx.set_verify_lanes(lanes)
            assert hbx_ctx.prepare_ciphertexts(cts[:p]).all()
            valid = hbx_ctx.verify_dec_shares(sh)
            assert hbx_ctx.verify_lanes_used() == lanes
            plains, status = hbx_ctx.combine_decrypt(sks.threshold + 1)
            got[lanes] = (valid, hbx_ctx.share_status(p, n), hbx_ctx.ct_status(p), status, plains)
    finally:
        hbx_ctx.set_verify_lanes(0)
    np.testing.assert_array_equal(got[7][0], expect)
    for x, y in zip(got[1][:4], got[7][:4]):
        np.testing.assert_array_equal(x, y)
    assert got[1][4] == got[7][4] == msgs[:p]


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True], ids=["plain", "own"])
def test_forced_degenerate_proposers_take_the_fallback(hbx_ctx, own):
    """hbx_debug_force_degenerate(2) at n = 10: every second proposer's checkable shares (and in
    own-share mode its ciphertext verdict) are decided by the fallback launch -- same statuses,
    ct_valid and plaintexts as unforced and as the fixture, and hbx_get_fallback_lanes counts
    exactly the checkable lanes of the forced proposers."""
    d = _load("hb_epoch_n10")
    _set_keys(hbx_ctx, d)
    hbx_ctx.set_verify_lanes(1)
    try:
        if own:
            hbx_ctx.set_own_share(int(d["own_me"]), d["own_sk"].tobytes())
        plain = _fused_epoch(hbx_ctx, d)
        assert hbx_ctx.fallback_lanes() == 0
        hbx_ctx.debug_force_degenerate(2)
        forced = _fused_epoch(hbx_ctx, d)
        lanes = hbx_ctx.fallback_lanes()
    finally:
        hbx_ctx.debug_force_degenerate(0)
        hbx_ctx.set_own_share(0, None)
        hbx_ctx.set_verify_lanes(0)
    _assert_same(forced, plain)
    _assert_golden(d, forced, own)
    # checkable = present, known sender, decodable share, decodable ciphertext: the lanes that end
    # INVALID (0) or VALID (1), or SKIPPED_CT (4) under a ciphertext that decoded but is not valid
    ct, valid = plain[0], plain[1]
    want = sum(int(np.isin(valid[j], (0, 1, 4)).sum()) for j in range(0, len(ct), 2) if ct[j] != 3)
    assert want > 0
    assert lanes == want
