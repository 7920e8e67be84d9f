"""GPU parity: the SyncKeyGen calls (reference src/sync_key_gen.rs) against the committed oracle
fixtures of tests/golden/make_skg_golden.py and Python integers.  Bit-exact, no tolerance:
hbx_encrypt_to / hbx_sk_decrypt (skg_batch65: 65 ciphertexts, one more than a wave),
hbx_bivar_poly_rows / hbx_fr_poly_eval (the dealer's rows and the Ack values), hbx_public_keys as the
commitment of coefficients that include 0, hbx_keygen_generate / hbx_pk_shares_from_commit
(skg_gen_n4, skg_gen_n7), and the generated keys installed and used for a threshold decryption."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G1_IDENTITY = bytes([0xC0]) + bytes(47)


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


@pytest.fixture(scope="module")
def batch():
    return _load("skg_batch65")


def _split(blob, off):
    return [blob[int(off[j]):int(off[j + 1])].tobytes() for j in range(len(off) - 1)]


def _wire_cts(d):
    v = _split(d["v_blob"], d["off"])
    return [(d["u"][j].tobytes(), v[j], d["w"][j].tobytes()) for j in range(len(v))]


def _ints(a):
    """uint8[..., 32] big-endian -> nested list of Python ints."""
    a = np.asarray(a)
    if a.ndim == 1:
        return int.from_bytes(a.tobytes(), "big")
    return [_ints(x) for x in a]


def _be32(vals, *shape):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in vals), dtype=np.uint8).reshape(*shape, 32)


def _coeff_pos(i, j):
    if i > j:
        i, j = j, i
    return j * (j + 1) // 2 + i


def _bivar_eval(coeff, t, x, y):
    return sum(coeff[_coeff_pos(i, j)] * pow(x, i, R) * pow(y, j, R) for i in range(t + 1) for j in range(t + 1)) % R


def _lagrange0(ys, vs):
    acc = 0
    for k, (yk, vk) in enumerate(zip(ys, vs)):
        num = den = 1
        for m, ym in enumerate(ys):
            if m != k:
                num = num * ym % R
                den = den * (ym - yk) % R
        acc += vk * num * pow(den, -1, R)
    return acc % R


@pytest.mark.gpu
def test_encrypt_to_matches_golden(hbx_ctx, batch):
    d = batch
    msgs = _split(d["msg_blob"], d["off"])
    got = hbx_ctx.encrypt_to(d["pk_to"], msgs, d["r_to"])
    want_v = _split(d["to_v"], d["off"])
    for j, (u, v, w) in enumerate(got):
        assert u == d["to_u"][j].tobytes(), j
        assert v == want_v[j], j
        assert w == d["to_w"][j].tobytes(), j
    # one key repeated is hbx_encrypt
    same = hbx_ctx.encrypt_to(np.repeat(d["pk"][None, :], len(msgs), axis=0), msgs, d["r"])
    assert same == hbx_ctx.encrypt(d["pk"].tobytes(), msgs, d["r"])
    enc_v = _split(d["enc_v"], d["off"])
    assert same == [(d["enc_u"][j].tobytes(), enc_v[j], d["enc_w"][j].tobytes()) for j in range(len(msgs))]


@pytest.mark.gpu
def test_encrypt_to_rejects_bad_key_and_scalar(hbx_ctx, batch):
    from hbbft_amd.hbx import HBX_E_INVALID_ARG, HbxError

    d = batch
    gen = _load("skg_gen_n4")
    msgs = _split(d["msg_blob"], d["off"])[:3]
    pk = d["pk_to"][:3].copy()
    pk[1] = gen["bad_g1"]
    with pytest.raises(HbxError) as e:
        hbx_ctx.encrypt_to(pk, msgs, d["r_to"][:3])
    assert e.value.code == HBX_E_INVALID_ARG
    r = d["r_to"][:3].copy()
    r[2] = np.frombuffer(R.to_bytes(32, "big"), dtype=np.uint8)
    with pytest.raises(HbxError) as e:
        hbx_ctx.encrypt_to(d["pk_to"][:3], msgs, r)
    assert e.value.code == HBX_E_INVALID_ARG


@pytest.mark.gpu
def test_sk_decrypt_matches_golden(hbx_ctx, batch):
    d = batch
    plains, st = hbx_ctx.sk_decrypt(d["sk"].tobytes(), _wire_cts(d))
    np.testing.assert_array_equal(st, d["expect_status"])
    assert st[7] == 0 and st[21] == 3 and st[64] == 1
    want = _split(d["expect_plain"], d["off"])
    msgs = _split(d["msg_blob"], d["off"])
    for j, pt in enumerate(plains):
        assert pt == want[j], j
        assert pt == (msgs[j] if st[j] == 1 else bytes(len(msgs[j]))), j
    # each recipient of encrypt_to decrypts its own message with its own key
    to_v = _split(d["to_v"], d["off"])
    for j in (0, 5, 64):
        pt, s = hbx_ctx.sk_decrypt(d["sk_to"][j].tobytes(), [(d["to_u"][j].tobytes(), to_v[j], d["to_w"][j].tobytes())])
        assert s[0] == 1 and pt[0] == msgs[j]


@pytest.mark.gpu
def test_sk_decrypt_voids_prepared_ciphertexts_and_keeps_own_share(hbx_ctx, batch):
    from hbbft_amd.hbx import HBX_E_NO_CIPHERTEXTS, HbxError

    e4 = _load("hb_epoch_n4")
    off = e4["v_off"]
    cts = [(e4["u"][j].tobytes(), e4["v_blob"][int(off[j]):int(off[j + 1])].tobytes(), e4["w"][j].tobytes())
           for j in range(len(off) - 1)]
    p, n = e4["shares"].shape[:2]
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in e4["pk_comp"]]) == 0).all()
    me = int(e4["own_me"])
    hbx_ctx.set_own_share(me, e4["own_sk"].tobytes())
    try:
        hbx_ctx.prepare_ciphertexts(cts)
        _, st = hbx_ctx.sk_decrypt(batch["sk"].tobytes(), _wire_cts(batch)[:9])
        np.testing.assert_array_equal(st, batch["expect_status"][:9])
        with pytest.raises(HbxError) as e:
            hbx_ctx.verify_dec_shares(e4["shares"], e4["present"])
        assert e.value.code == HBX_E_NO_CIPHERTEXTS
        # own-share mode set before the call is still in effect: the column's own-share expectations
        ct_ok = hbx_ctx.prepare_ciphertexts(cts)
        np.testing.assert_array_equal(ct_ok, e4["expect_ct_valid"])
        valid = hbx_ctx.verify_dec_shares(e4["shares"], e4["present"])
        np.testing.assert_array_equal(valid, e4["expect_valid_own"])
        np.testing.assert_array_equal(hbx_ctx.share_status(p, n), e4["expect_share_status_own"])
        _, status = hbx_ctx.combine_decrypt(int(e4["t"]))
        np.testing.assert_array_equal(status, e4["expect_status_own"])
    finally:
        hbx_ctx.set_own_share(me, None)


@pytest.mark.gpu
def test_sha3_encrypt_to_sk_decrypt_roundtrip(hbx_ctx, batch):
    from hbbft_amd.hbx import DIGEST_SHA3_256

    d = batch
    hbx_ctx.set_digest(DIGEST_SHA3_256)
    msgs = _split(d["msg_blob"], d["off"])[:12]
    n = len(msgs)
    # every message to recipient 3's key: one sk_decrypt call opens them all
    cts = hbx_ctx.encrypt_to(np.repeat(d["pk_to"][3][None, :], n, axis=0), msgs, d["r_to"][:n])
    sha2 = _split(d["to_v"], d["off"])
    assert cts[3][1] != sha2[3] or len(msgs[3]) == 0  # another keystream than the SHA-256 fixture's
    plains, st = hbx_ctx.sk_decrypt(d["sk_to"][3].tobytes(), cts)
    assert (st == 1).all()
    assert plains == msgs


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["skg_gen_n4", "skg_gen_n7"])
def test_poly_rows_evals_and_commitment(hbx_ctx, name):
    g = _load(name)
    n, t = int(g["n"]), int(g["t"])
    coeff = _ints(g["coeffs"][0])
    assert 0 in coeff
    # hbx_bivar_poly_rows: row_x[j] = sum_i a_ij x^i for x = 1..n, over 65 "nodes" (more than one block)
    nn = 65
    rows = hbx_ctx.bivar_poly_rows(g["coeffs"][0], t, nn)
    want_rows = [[sum(coeff[_coeff_pos(i, j)] * pow(x, i, R) for i in range(t + 1)) % R for j in range(t + 1)]
                 for x in range(1, nn + 1)]
    assert _ints(rows) == want_rows
    # hbx_fr_poly_eval: the Ack values row_x.evaluate(idx + 1) = f(x, idx + 1), p = 65 rows x n points
    vals = hbx_ctx.fr_poly_eval(rows, n)
    assert _ints(vals) == [[_bivar_eval(coeff, t, x, y) for y in range(1, n + 1)] for x in range(1, nn + 1)]
    # the commitment (sync_key_gen.rs:291) is hbx_public_keys of the coefficients; g1 * 0 = identity
    commit = hbx_ctx.public_keys(g["coeffs"][0])
    np.testing.assert_array_equal(commit, g["commits"][0])
    assert commit[coeff.index(0)].tobytes() == G1_IDENTITY


@pytest.mark.gpu
def test_poly_calls_reject_noncanonical_scalars(hbx_ctx):
    from hbbft_amd.hbx import HBX_E_INVALID_ARG, HbxError

    g = _load("skg_gen_n4")
    bad = g["coeffs"][0].copy()
    bad[1] = np.frombuffer(R.to_bytes(32, "big"), dtype=np.uint8)
    with pytest.raises(HbxError) as e:
        hbx_ctx.bivar_poly_rows(bad, int(g["t"]), 4)
    assert e.value.code == HBX_E_INVALID_ARG
    with pytest.raises(HbxError) as e:
        hbx_ctx.fr_poly_eval(bad[None, :2], 4)
    assert e.value.code == HBX_E_INVALID_ARG


def _values_for(g, me, cnt_of=None):
    """Node `me`'s verified Ack values per part: the first cnt senders in index order."""
    n, t = int(g["n"]), int(g["t"])
    cnt = np.zeros(n, dtype=np.uint32)
    ys = np.zeros((n, t + 1), dtype=np.uint64)
    vals = []
    for q in range(n):
        c = (t + 1) if cnt_of is None else cnt_of(q)
        coeff = _ints(g["coeffs"][q])
        cnt[q] = c
        row = []
        for k in range(t + 1):
            ys[q, k] = k + 2 if q % 2 else k + 1  # odd parts skip sender 0 (its ack was invalid)
            row.append(_bivar_eval(coeff, t, me + 1, int(ys[q, k])) if k < c else 0)
        vals.append(row)
    return cnt, ys, _be32([v for row in vals for v in row], n, t + 1), vals


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["skg_gen_n4", "skg_gen_n7"])
def test_keygen_generate_and_pk_shares(hbx_ctx, name):
    from hbbft_amd.hbx import SHARE_ABSENT, SHARE_VALID

    g = _load(name)
    n, t = int(g["n"]), int(g["t"])
    want_st = np.where(g["complete"] != 0, SHARE_VALID, SHARE_ABSENT)
    for me in range(n):
        cnt, ys, vals32, _ = _values_for(g, me)
        pkc, sk, st = hbx_ctx.keygen_generate(g["commits"], t, g["complete"], cnt, ys, vals32)
        np.testing.assert_array_equal(pkc, g["pk_commit"])
        np.testing.assert_array_equal(st, want_st)
        assert sk == g["sk_all"][me].tobytes(), me
    # an observer gets the commitment only
    pkc, sk, st = hbx_ctx.keygen_generate(g["commits"], t, g["complete"])
    np.testing.assert_array_equal(pkc, g["pk_commit"])
    assert sk is None
    np.testing.assert_array_equal(st, want_st)
    # public_key_share(i) = pk_commit.evaluate(i + 1); 65 nodes also cross a block boundary
    np.testing.assert_array_equal(hbx_ctx.pk_shares_from_commit(g["pk_commit"], n), g["pk_shares"])
    more = hbx_ctx.pk_shares_from_commit(g["pk_commit"], 65)
    np.testing.assert_array_equal(more[:n], g["pk_shares"])
    np.testing.assert_array_equal(more, hbx_ctx.public_keys(_be32(
        [sum(sum(_ints(g["coeffs"][q])[_coeff_pos(0, j)] for q in range(n) if g["complete"][q]) * pow(i + 1, j, R)
             for j in range(t + 1)) % R for i in range(65)], 65)))


@pytest.mark.gpu
def test_keygen_generate_short_parts_duplicates_and_bad_commitment(hbx_ctx):
    from hbbft_amd.hbx import HBX_E_DUPLICATE_ENTRY, HBX_E_INVALID_ARG, SHARE_UNDECODABLE, HbxError

    g = _load("skg_gen_n7")
    n, t, me = int(g["n"]), int(g["t"]), 3
    # part 1 holds t values, part 2 one, part 4 none: Poly::interpolate goes through what there is
    short = {1: t, 2: 1, 4: 0}
    cnt, ys, vals32, vals = _values_for(g, me, lambda q: short.get(q, t + 1))
    _, sk, _ = hbx_ctx.keygen_generate(g["commits"], t, g["complete"], cnt, ys, vals32)
    want = sum(_lagrange0([int(y) for y in ys[q][:cnt[q]]], vals[q][:cnt[q]]) for q in range(n) if g["complete"][q]) % R
    assert int.from_bytes(sk, "big") == want
    assert sk != g["sk_all"][me].tobytes()
    # a repeated y inside a complete part; the same inside the incomplete part is not read
    cnt, ys, vals32, _ = _values_for(g, me)
    dup = ys.copy()
    dup[n - 1, 1] = dup[n - 1, 0]
    _, sk, _ = hbx_ctx.keygen_generate(g["commits"], t, g["complete"], cnt, dup, vals32)
    assert sk == g["sk_all"][me].tobytes()
    dup[2, t] = dup[2, 0]
    with pytest.raises(HbxError) as e:
        hbx_ctx.keygen_generate(g["commits"], t, g["complete"], cnt, dup, vals32)
    assert e.value.code == HBX_E_DUPLICATE_ENTRY
    # a value >= r
    badv = vals32.copy()
    badv[0, 0] = np.frombuffer(R.to_bytes(32, "big"), dtype=np.uint8)
    with pytest.raises(HbxError) as e:
        hbx_ctx.keygen_generate(g["commits"], t, g["complete"], cnt, ys, badv)
    assert e.value.code == HBX_E_INVALID_ARG
    # a non-G1 point in a complete part's commitment: status says which part, nothing is written
    commits = g["commits"].copy()
    commits[5, 2] = g["bad_g1"]
    with pytest.raises(HbxError) as e:
        hbx_ctx.keygen_generate(commits, t, g["complete"], cnt, ys, vals32)
    assert e.value.code == HBX_E_INVALID_ARG
    assert hbx_ctx.keygen_status[5] == SHARE_UNDECODABLE and (np.delete(hbx_ctx.keygen_status, 5) != SHARE_UNDECODABLE).all()
    # the same point in the part that is not complete is never examined
    commits = g["commits"].copy()
    commits[n - 1, 0] = g["bad_g1"]
    pkc, sk, _ = hbx_ctx.keygen_generate(commits, t, g["complete"], cnt, ys, vals32)
    np.testing.assert_array_equal(pkc, g["pk_commit"])
    assert sk == g["sk_all"][me].tobytes()
    with pytest.raises(HbxError) as e:
        hbx_ctx.pk_shares_from_commit(commits[n - 1, :t + 1], n)
    assert e.value.code == HBX_E_INVALID_ARG


@pytest.mark.gpu
def test_generated_keys_decrypt_end_to_end(hbx_ctx):
    """generate -> pk shares -> hbx_set_pk_shares / hbx_set_own_share -> encrypt to the new master key
    pk_commit[0] -> every node's decryption share -> prepare / verify / combine at t + 1."""
    g = _load("skg_gen_n7")
    n, t, me = int(g["n"]), int(g["t"]), 3
    cnt, ys, vals32, _ = _values_for(g, me)
    pkc, sk, _ = hbx_ctx.keygen_generate(g["commits"], t, g["complete"], cnt, ys, vals32)
    pk_shares = hbx_ctx.pk_shares_from_commit(pkc, n)
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in pk_shares]) == 0).all()
    hbx_ctx.set_own_share(me, sk)
    try:
        msg = bytes(range(97))
        r = _be32([0x1234567890ABCDEF << 64 | 77], 1)
        cts = hbx_ctx.encrypt(pkc[0].tobytes(), [msg], r)
        shares = hbx_ctx.decrypt_shares(g["sk_all"], np.frombuffer(cts[0][0], dtype=np.uint8).reshape(1, 48))
        assert hbx_ctx.prepare_ciphertexts(cts).all()
        assert hbx_ctx.verify_dec_shares(shares).all()
        plains, status = hbx_ctx.combine_decrypt(t + 1)
        assert status[0] == 0 and plains[0] == msg
    finally:
        hbx_ctx.set_own_share(me, None)
