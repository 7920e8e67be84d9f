"""GPU: the pair-lane Ciphertext::verify of hbx_sk_decrypt (hbx_set_ct_check(HBX_CT_CHECK_PAIR):
k_verify_ct2 + the two-lane final exponentiation, one lane pair per ciphertext, no prepared line
tables) against the committed oracle fixtures and against the default wide executor.  Bit-exact:
HBX_CT_* status bytes and plaintexts.  Every case puts the context back to the wide mode and
debug_force_fallback(0)."""
import contextlib
import os

import numpy as np
import pytest

from skg_fixture import load_era

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


def _split(blob, off):
    return [blob[int(off[j]):int(off[j + 1])].tobytes() for j in range(len(off) - 1)]


def _wire_cts(d, off_key="off"):
    v = _split(d["v_blob"], d[off_key])
    return [(d["u"][j].tobytes(), v[j], d["w"][j].tobytes()) for j in range(len(v))]


@pytest.fixture(scope="module")
def batch():
    d = _load("skg_batch65")
    d["cts"] = _wire_cts(d)
    d["plain"] = _split(d["expect_plain"], d["off"])
    return d


@contextlib.contextmanager
def pair_mode(ctx, force_fallback=0):
    from hbbft_amd.hbx import CT_CHECK_PAIR, CT_CHECK_WIDE

    try:
        ctx.set_ct_check(CT_CHECK_PAIR)
        ctx.debug_force_fallback(force_fallback)
        yield ctx
    finally:
        ctx.set_ct_check(CT_CHECK_WIDE)
        ctx.debug_force_fallback(0)


def _assert_prefix(batch, plains, st, count):
    np.testing.assert_array_equal(st, batch["expect_status"][:count])
    assert plains == batch["plain"][:count]


@pytest.mark.gpu
def test_batch65_pair_mode_equals_golden_and_wide(hbx_ctx, batch):
    """65 ciphertexts: three 32-pair blocks, the last with one live pair."""
    sk = batch["sk"].tobytes()
    with pair_mode(hbx_ctx):
        plains, st = hbx_ctx.sk_decrypt(sk, batch["cts"])
        assert hbx_ctx.ct_check_used() == 1
    _assert_prefix(batch, plains, st, 65)
    assert st[7] == 0 and st[21] == 3 and st[64] == 1
    plains0, st0 = hbx_ctx.sk_decrypt(sk, batch["cts"])
    assert hbx_ctx.ct_check_used() == 0
    np.testing.assert_array_equal(st0, st)
    assert plains0 == plains


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 32, 33])
def test_prefix_counts(hbx_ctx, batch, count):
    """A lone pair in a wave; two pairs; exactly one full block; one pair past it."""
    with pair_mode(hbx_ctx):
        plains, st = hbx_ctx.sk_decrypt(batch["sk"].tobytes(), batch["cts"][:count])
    _assert_prefix(batch, plains, st, count)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hb_epoch_n4", "hb_epoch_n7", "hb_epoch_n10", "hb_epoch_n64", "hb_epoch_n7_sha3"])
def test_epoch_ciphertexts_decode_and_identity_cases(hbx_ctx, batch, name):
    """The epoch fixtures' ciphertexts (an invalid one, off-subgroup and identity U / W, a W of another
    ciphertext) under the key-generation key: the fixture's statuses, and mode 0's bytes (the
    plaintexts mean nothing under that key but are deterministic, and zero where not VALID)."""
    from hbbft_amd.hbx import CT_VALID, DIGEST_SHA3_256

    e = _load(name)
    cts = _wire_cts(e, "v_off")
    sk = batch["sk"].tobytes()
    if name.endswith("_sha3"):
        hbx_ctx.set_digest(DIGEST_SHA3_256)
    with pair_mode(hbx_ctx):
        plains, st = hbx_ctx.sk_decrypt(sk, cts)
        assert hbx_ctx.ct_check_used() == 1
    np.testing.assert_array_equal(st, e["expect_ct_status"])
    plains0, st0 = hbx_ctx.sk_decrypt(sk, cts)
    assert hbx_ctx.ct_check_used() == 0
    np.testing.assert_array_equal(st0, st)
    assert plains0 == plains
    for j, pt in enumerate(plains):
        if st[j] != CT_VALID:
            assert pt == bytes(len(cts[j][1])), j


@pytest.mark.gpu
def test_forced_fallback_every_third(hbx_ctx, batch):
    from hbbft_amd.hbx import CT_UNDECODABLE

    with pair_mode(hbx_ctx, force_fallback=3):
        plains, st = hbx_ctx.sk_decrypt(batch["sk"].tobytes(), batch["cts"])
        lanes = hbx_ctx.fallback_lanes()
    _assert_prefix(batch, plains, st, 65)
    assert lanes == sum(1 for j in range(65) if j % 3 == 0 and batch["expect_status"][j] != CT_UNDECODABLE)


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 33])
def test_forced_fallback_every_pair(hbx_ctx, batch, count):
    from hbbft_amd.hbx import CT_UNDECODABLE

    with pair_mode(hbx_ctx, force_fallback=1):
        plains, st = hbx_ctx.sk_decrypt(batch["sk"].tobytes(), batch["cts"][:count])
        lanes = hbx_ctx.fallback_lanes()
    _assert_prefix(batch, plains, st, count)
    assert lanes == int((batch["expect_status"][:count] != CT_UNDECODABLE).sum())


@pytest.mark.gpu
def test_chunk_boundary(hbx_ctx, batch):
    """One ciphertext more than a pair-mode chunk: the second pass holds a single pair."""
    from hbbft_amd.hbx import SK_DECRYPT_PAIR_CHUNK

    count = SK_DECRYPT_PAIR_CHUNK + 1
    tiles = -(-count // 65)
    cts = (batch["cts"] * tiles)[:count]
    with pair_mode(hbx_ctx):
        plains, st = hbx_ctx.sk_decrypt(batch["sk"].tobytes(), cts)
    np.testing.assert_array_equal(st, np.tile(batch["expect_status"], tiles)[:count])
    rng = np.random.default_rng(0xC7)
    for tile in {0, tiles - 1, *rng.integers(1, tiles - 1, size=2).tolist()}:
        lo, hi = 65 * tile, min(65 * (tile + 1), count)
        assert plains[lo:hi] == batch["plain"][:hi - lo], tile


@pytest.mark.gpu
def test_pair_mode_voids_prepared_ciphertexts_and_keeps_own_share(hbx_ctx, batch):
    from hbbft_amd.hbx import HBX_E_NO_CIPHERTEXTS, HbxError

    e4 = _load("hb_epoch_n4")
    cts = _wire_cts(e4, "v_off")
    p, n = e4["shares"].shape[:2]
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in e4["pk_comp"]]) == 0).all()
    me = int(e4["own_me"])
    hbx_ctx.set_own_share(me, e4["own_sk"].tobytes())
    try:
        hbx_ctx.prepare_ciphertexts(cts)
        with pair_mode(hbx_ctx):
            _, st = hbx_ctx.sk_decrypt(batch["sk"].tobytes(), batch["cts"][:9])
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
@pytest.mark.parametrize("name", ["skg_n4", "skg_n7"])
def test_replay_in_pair_mode(hbx_ctx, name):
    from hbbft_amd.hbx import CT_CHECK_PAIR, CT_CHECK_WIDE
    from hbbft_amd.sync_key_gen import PART, KeyGenReplay

    d = load_era(name)
    msgs = []
    for kind, sender, body in d["msgs"]:
        if kind == PART:
            body = (np.frombuffer(b"".join(body[0]), dtype=np.uint8).reshape(-1, 48), body[1])
        msgs.append((kind, sender, body))
    try:
        kg = KeyGenReplay(hbx_ctx, int(d["me"]), d["sk_nodes"][int(d["me"])].tobytes(), d["pk_nodes"], int(d["t"]),
                          ct_check=CT_CHECK_PAIR)
        out, acks = kg.handle_messages(msgs, d["ack_r_by_msg"])
        assert hbx_ctx.ct_check_used() == 1
    finally:
        hbx_ctx.set_ct_check(CT_CHECK_WIDE)
    assert list(out) == d["outcome"].tolist()
    assert sorted(acks) == [k for k, o in enumerate(out) if o == 1]
    for k, (proposer, values) in acks.items():
        assert proposer == d["msgs"][k][1]
        assert values == d["exp_ack_by_msg"][k], k
    pkc, sk = kg.generate()
    np.testing.assert_array_equal(pkc, d["pk_commit"])
    assert sk == d["sk_me"].tobytes()
