"""GPU: PublicKey::verify over a key table (hbx_verify_sigs_keyed: k_verify_sigs2 + the two-lane final
exponentiation, one lane pair per item, no prepared line tables), SecretKey::sign (hbx_sign_msgs) and
the signed key-generation replay (hbbft_amd/dhb_keygen.py) against the committed oracle fixtures and
against hbx_verify_sigs.  Bit-exact status bytes and signatures.  Every case that sets
debug_force_fallback puts it back to 0."""
import os

import numpy as np
import pytest

from skg_fixture import load_era

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PT_OK = 0


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


def _split(blob, off):
    return [blob[int(off[j]):int(off[j + 1])].tobytes() for j in range(len(off) - 1)]


@pytest.fixture(scope="module")
def b65():
    d = _load("kgsigs_b65")
    d["msgs"] = _split(d["msg_blob"], d["msg_off"])
    return d


def _keyed(ctx, d, count):
    return ctx.verify_sigs_keyed(d["pk"], d["key_idx"][:count], d["msgs"][:count], d["sig"][:count])


def _reached_pairing(d, count):
    """Items whose pair ran its Miller loops and reached the final exponentiation: a key, both decodes
    fine, sigma in G2 -- exactly the items the fixture expects VALID or INVALID."""
    return d["expect"][:count] <= 1


@pytest.mark.gpu
def test_b65_statuses_and_key_status(hbx_ctx, b65):
    """65 items: three 32-pair blocks, the last with one live pair; every case of the fixture."""
    st, kst = _keyed(hbx_ctx, b65, 65)
    np.testing.assert_array_equal(st, b65["expect"])
    np.testing.assert_array_equal(kst, b65["expect_key_status"])
    assert st.dtype == np.uint8 and kst.dtype == np.int32
    assert set(st.tolist()) == {0, 1, 3, 5}


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 2, 32, 33])
def test_prefix_counts(hbx_ctx, b65, count):
    """A lone pair in a wave; two pairs; exactly one full block; one pair past it."""
    st, kst = _keyed(hbx_ctx, b65, count)
    np.testing.assert_array_equal(st, b65["expect"][:count])
    np.testing.assert_array_equal(kst, b65["expect_key_status"])


@pytest.mark.gpu
def test_b9_sha3(hbx_ctx):
    from hbbft_amd.hbx import DIGEST_SHA3_256

    d = _load("kgsigs_b9_sha3")
    d["msgs"] = _split(d["msg_blob"], d["msg_off"])
    hbx_ctx.set_digest(DIGEST_SHA3_256)
    st, kst = _keyed(hbx_ctx, d, 9)
    np.testing.assert_array_equal(st, d["expect"])
    np.testing.assert_array_equal(kst, d["expect_key_status"])
    sig = hbx_ctx.sign_msgs(d["sign_sk"].tobytes(), d["msgs"])
    np.testing.assert_array_equal(sig, d["expect_sig"])
    # under the default digest the valid items no longer verify
    hbx_ctx.set_digest(0)
    st0, _ = _keyed(hbx_ctx, d, 9)
    assert (st0[d["expect"] == 1] == [0, 1]).all()  # item 0 fails; item 6 is identity / identity


@pytest.mark.gpu
def test_sigs_n16_equals_fixture_and_verify_sigs(hbx_ctx):
    """One key per item (nkeys == count, key_idx = arange): hbx_verify_sigs' bytes."""
    d = _load("sigs_n16")
    msgs = _split(d["msg_blob"], d["msg_off"])
    st, _ = hbx_ctx.verify_sigs_keyed(d["pk"], np.arange(16, dtype=np.uint32), msgs, d["sig"])
    np.testing.assert_array_equal(st, d["expect"])
    np.testing.assert_array_equal(st, hbx_ctx.verify_sigs(d["pk"], msgs, d["sig"]))


@pytest.mark.gpu
@pytest.mark.parametrize("every,count", [(3, 65), (3, 33), (1, 65), (1, 33)])
def test_forced_fallback(hbx_ctx, b65, every, count):
    try:
        hbx_ctx.debug_force_fallback(every)
        st, _ = _keyed(hbx_ctx, b65, count)
        lanes = hbx_ctx.fallback_lanes()
    finally:
        hbx_ctx.debug_force_fallback(0)
    np.testing.assert_array_equal(st, b65["expect"][:count])
    reached = _reached_pairing(b65, count)
    assert lanes == int(reached[::every].sum())
    if every == 1:
        assert lanes == int(reached.sum())


@pytest.mark.gpu
def test_chunk_boundary(hbx_ctx, b65):
    """One item more than a pass: the second pass holds a single pair."""
    from hbbft_amd.hbx import VERIFY_SIGS_CHUNK

    count = VERIFY_SIGS_CHUNK + 1
    tiles = -(-count // 65)
    st, kst = hbx_ctx.verify_sigs_keyed(b65["pk"], np.tile(b65["key_idx"], tiles)[:count], (b65["msgs"] * tiles)[:count],
                                        np.tile(b65["sig"], (tiles, 1))[:count])
    np.testing.assert_array_equal(st, np.tile(b65["expect"], tiles)[:count])
    np.testing.assert_array_equal(kst, b65["expect_key_status"])
    # the lone pair of the second pass is item VERIFY_SIGS_CHUNK: with every pair forced through the
    # fallback, two items decide it alone
    lo = count - 2
    try:
        hbx_ctx.debug_force_fallback(1)
        st2, _ = hbx_ctx.verify_sigs_keyed(b65["pk"], np.tile(b65["key_idx"], tiles)[lo:count],
                                           (b65["msgs"] * tiles)[lo:count], np.tile(b65["sig"], (tiles, 1))[lo:count])
    finally:
        hbx_ctx.debug_force_fallback(0)
    np.testing.assert_array_equal(st2, st[lo:])


@pytest.mark.gpu
def test_sign_msgs_equals_oracle_and_verifies(hbx_ctx, b65):
    sk = b65["sign_sk"].tobytes()
    sig = hbx_ctx.sign_msgs(sk, b65["msgs"])
    np.testing.assert_array_equal(sig, b65["expect_sig"])
    pk = hbx_ctx.public_keys(b65["sign_sk"].reshape(1, 32))
    st, kst = hbx_ctx.verify_sigs_keyed(pk, np.zeros(65, dtype=np.uint32), b65["msgs"], sig)
    assert (st == 1).all() and kst.tolist() == [PT_OK]
    # a message apart: its signature does not verify the next one
    st, _ = hbx_ctx.verify_sigs_keyed(pk, np.zeros(2, dtype=np.uint32), b65["msgs"][1:3], sig[[1, 1]])
    assert st.tolist() == [1, 0]


@pytest.mark.gpu
def test_argument_errors(hbx_ctx, b65):
    """HBX_E_INVALID_ARG from the library itself (the binding's guards are not in the way here)."""
    import ctypes

    from hbbft_amd.hbx import HBX_E_INVALID_ARG, HbxError

    R_BE = bytes.fromhex("73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001")
    for sk in (bytes(32), R_BE, bytes([0xFF]) * 32):  # 0, r and a value above r
        with pytest.raises(HbxError) as e:
            hbx_ctx.sign_msgs(sk, b65["msgs"][:2])
        assert e.value.code == HBX_E_INVALID_ARG
    u8p, u32p, u64p = (ctypes.POINTER(t) for t in (ctypes.c_uint8, ctypes.c_uint32, ctypes.c_uint64))
    pk, idx, sig = np.ascontiguousarray(b65["pk"]), np.ascontiguousarray(b65["key_idx"][:2]), np.ascontiguousarray(b65["sig"][:2])
    blob = np.frombuffer(b"abc", dtype=np.uint8).copy()
    off = np.array([0, 1, 3], dtype=np.uint64)
    st = np.full(2, 0xEE, dtype=np.uint8)
    good = dict(pk=pk.ctypes.data_as(u8p), nkeys=9, idx=idx.ctypes.data_as(u32p), blob=blob.ctypes.data_as(u8p),
                off=off.ctypes.data_as(u64p), sig=sig.ctypes.data_as(u8p), count=2, st=st.ctypes.data_as(u8p))

    def call(**kw):
        a = dict(good, **kw)
        return hbx_ctx.lib.hbx_verify_sigs_keyed(hbx_ctx.h, a["pk"], a["nkeys"], a["idx"], a["blob"], a["off"], a["sig"],
                                                 a["count"], a["st"], None)

    down = np.array([0, 3, 1], dtype=np.uint64)
    for kw in (dict(count=0), dict(nkeys=0), dict(pk=None), dict(idx=None), dict(off=None), dict(sig=None), dict(st=None),
               dict(blob=None), dict(off=down.ctypes.data_as(u64p))):
        assert call(**kw) == HBX_E_INVALID_ARG, kw
    assert (st == 0xEE).all()  # nothing was written
    assert call() == 0 and set(st.tolist()) <= {0, 1, 3, 5}
    sk = np.frombuffer(bytes([1]) * 32, dtype=np.uint8).copy()
    out = np.zeros((2, 96), dtype=np.uint8)
    for a in ((None, good["blob"], good["off"], 2, out.ctypes.data_as(u8p)), (sk.ctypes.data_as(u8p), good["blob"], good["off"], 0, out.ctypes.data_as(u8p)),
              (sk.ctypes.data_as(u8p), good["blob"], good["off"], 2, None), (sk.ctypes.data_as(u8p), good["blob"], down.ctypes.data_as(u64p), 2, out.ctypes.data_as(u8p))):
        assert hbx_ctx.lib.hbx_sign_msgs(hbx_ctx.h, *a) == HBX_E_INVALID_ARG


@pytest.mark.gpu
def test_leaves_prepared_ciphertexts_alone(hbx_ctx, b65):
    e4 = _load("hb_epoch_n4")
    v = _split(e4["v_blob"], e4["v_off"])
    cts = [(e4["u"][j].tobytes(), v[j], e4["w"][j].tobytes()) for j in range(len(v))]
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in e4["pk_comp"]]) == 0).all()
    hbx_ctx.prepare_ciphertexts(cts)
    st, _ = _keyed(hbx_ctx, b65, 33)
    np.testing.assert_array_equal(st, b65["expect"][:33])
    hbx_ctx.sign_msgs(b65["sign_sk"].tobytes(), b65["msgs"][:3])
    valid = hbx_ctx.verify_dec_shares(e4["shares"], e4["present"])
    np.testing.assert_array_equal(valid, e4["expect_valid"])


@pytest.mark.gpu
def test_leaves_coin_state_alone(hbx_ctx, b65):
    c4 = _load("coin_n4")
    nonces = _split(c4["nonce_blob"], c4["nonce_off"])
    assert (hbx_ctx.set_pk_shares([row.tobytes() for row in c4["pk_comp"]]) == 0).all()
    hbx_ctx.prepare_nonces(nonces)
    st, _ = _keyed(hbx_ctx, b65, 33)
    np.testing.assert_array_equal(st, b65["expect"][:33])
    hbx_ctx.sign_msgs(b65["sign_sk"].tobytes(), b65["msgs"][:3])
    valid = hbx_ctx.verify_sig_shares(c4["sigs"], c4["present"])
    np.testing.assert_array_equal(valid, c4["expect_valid"])


def _items(d, era):
    ser = _split(d["ser_blob"], d["ser_off"])
    items = []
    for k, m in enumerate(d["item_msg"]):
        kind, _, body = era["msgs"][int(m)]
        if kind == 0:
            body = (np.frombuffer(b"".join(body[0]), dtype=np.uint8).reshape(-1, 48), body[1])
        sender = int(d["item_sender"][k])
        items.append((int(d["item_proposer"][k]), int(d["item_epoch"][k]), None if sender < 0 else sender, kind, body,
                      ser[k], d["item_sig"][k].tobytes()))
    return items


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["dhb_kg_n4", "dhb_kg_n7"])
def test_signed_replay_on_the_engine(hbx_ctx, name):
    from hbbft_amd.dhb_keygen import FAULT_INVALID_SIGNATURE, SignedKeyGenReplay
    from hbbft_amd.sync_key_gen import KeyGenReplay

    d = _load(name)
    era = load_era(str(d["base"]))
    me = int(era["me"])
    kg = KeyGenReplay(hbx_ctx, me, era["sk_nodes"][me].tobytes(), era["pk_nodes"], int(era["t"]))
    rp = SignedKeyGenReplay(kg, era["pk_nodes"], (int(d["cand_idx"]), d["cand_pk"].tobytes()), int(d["start_epoch"]))
    items = _items(d, era)
    rnd = {k: era["ack_r_by_msg"][int(m)] for k, m in enumerate(d["item_msg"]) if era["msgs"][int(m)][0] == 0}
    out, acks = rp.handle_batch(items, rnd)
    assert list(out) == d["expect_outcome"].tolist()
    assert rp.faults == [(int(p), FAULT_INVALID_SIGNATURE) for p in d["fault_proposer"]]
    for k, (proposer, values) in acks.items():
        assert values == era["exp_ack_by_msg"][int(d["item_msg"][k])], k
    pkc, sk = rp.generate()
    np.testing.assert_array_equal(pkc, d["pk_commit"])
    assert sk == d["sk_me"].tobytes()
    # the node's own signatures are the ones the fixture's honest items carry
    mine = [k for k, it in enumerate(items) if it[2] == me and d["expect_outcome"][k] < 16][:3]
    np.testing.assert_array_equal(rp.sign([items[k][5] for k in mine]), d["item_sig"][mine])
