"""The Python surface of the keyed PublicKey::verify and of SecretKey::sign (hbx_verify_sigs_keyed /
hbx_sign_msgs): exported names, argument guards, the fixtures' consistency with the oracle and the CPU
model, and SignedKeyGenReplay over a stand-in context that answers from the fixture's statuses.  No GPU
and no library call."""
import os

import numpy as np
import pytest

import dhb_kg_model as dhb
import skg_model as skg
from hbbft_amd import hbx
from hbbft_amd.dhb_keygen import BAD_SIGNATURE, FAULT_INVALID_SIGNATURE, OBSOLETE, SignedKeyGenReplay
from oracle import bls12_381 as bls
from oracle import threshold as tc
from skg_fixture import load_era

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))


def _split(blob, off):
    return [blob[int(off[j]):int(off[j + 1])].tobytes() for j in range(len(off) - 1)]


def test_exports_and_constants():
    assert "hbx_verify_sigs_keyed" in hbx.EXPORTS
    assert "hbx_sign_msgs" in hbx.EXPORTS
    assert hbx.VERIFY_SIGS_CHUNK == 16384 and hbx.NO_KEY == 0xFFFFFFFF
    assert (OBSOLETE, BAD_SIGNATURE) == (dhb.OBSOLETE, dhb.BAD_SIGNATURE)
    assert FAULT_INVALID_SIGNATURE == dhb.FAULT_INVALID_SIGNATURE
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "hbx.h")).read()
    assert "int hbx_verify_sigs_keyed(hbx_ctx* ctx, const uint8_t* pk48, uint32_t nkeys, const uint32_t* key_idx," in header
    assert "int hbx_sign_msgs(hbx_ctx* ctx, const uint8_t* sk32, const uint8_t* msg_blob, const uint64_t* msg_off," in header
    assert "#define HBX_K_COUNT 14" in header
    src = open(os.path.join(os.path.dirname(GOLDEN), "..", "hbbft_amd", "csrc", "hbx_api.hip")).read()
    assert f"constexpr uint32_t VERIFY_SIGS_CHUNK = {hbx.VERIFY_SIGS_CHUNK};" in src


class _NoLib:
    """Stands in for a Context's library: any call is a test failure (the guards must fire first)."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library with bad arguments")


def _bare_context():
    ctx = object.__new__(hbx.Context)  # no device: only the argument checks run
    ctx.lib, ctx.h = _NoLib(), None
    return ctx


PK = np.zeros((3, 48), dtype=np.uint8)
SIG = np.zeros((2, 96), dtype=np.uint8)
IDX = np.zeros(2, dtype=np.uint32)
MSGS = [b"a", b"bc"]


@pytest.mark.parametrize("pk48,key_idx,msgs,sig96,match", [
    (PK, IDX, MSGS[:1], SIG, "key_idx"),                       # one message, two indices
    (PK, IDX, MSGS, SIG[:1], "same non-zero count"),           # one signature short
    (PK, IDX, MSGS + [b"d"], SIG, "key_idx"),
    (PK, IDX.astype(np.int64), MSGS, SIG, "key_idx"),          # not uint32
    (PK, IDX.astype(np.int32), MSGS, SIG, "key_idx"),
    (PK, [0, 0], MSGS, SIG, "key_idx"),                        # not an array
    (PK, IDX.reshape(2, 1), MSGS, SIG, "key_idx"),
    (PK, np.zeros(0, dtype=np.uint32), [], SIG[:0], "non-zero count"),
    (PK.reshape(-1), IDX, MSGS, SIG, "pk48"),                  # not [nkeys, 48]
    (np.zeros((3, 96), dtype=np.uint8), IDX, MSGS, SIG, "pk48"),
    (PK[:0], IDX, MSGS, SIG, "pk48"),
    (PK, IDX, MSGS, np.zeros((2, 48), dtype=np.uint8), "same non-zero count"),
])
def test_verify_sigs_keyed_guards_fire_before_the_library(pk48, key_idx, msgs, sig96, match):
    with pytest.raises(ValueError, match=match):
        _bare_context().verify_sigs_keyed(pk48, key_idx, msgs, sig96)


@pytest.mark.parametrize("sk,msgs", [(bytes(31), MSGS), (bytes(33), MSGS), (bytes([1]) * 32, [])])
def test_sign_msgs_guards_fire_before_the_library(sk, msgs):
    with pytest.raises(ValueError, match="sign_msgs"):
        _bare_context().sign_msgs(sk, msgs)


# ---- kgsigs fixtures --------------------------------------------------------------------------------
def test_kgsigs_fixture_shape():
    d = _load("kgsigs_b65")
    assert int(d["count"]) == 65 and d["pk"].shape == (9, 48) and d["key_idx"].dtype == np.uint32
    lens = np.diff(d["msg_off"].astype(np.int64)).tolist()
    assert lens[:11] == [0, 1, 55, 56, 63, 64, 65, 119, 120, 300, 4099] and max(lens[11:]) < 300
    assert d["expect_key_status"].tolist() == [0] * 6 + [4, 5, 2]
    assert set(d["expect"].tolist()) == {0, 1, 3, 5}
    assert {int(k) for k in d["key_idx"] if k >= 9} == {9, 0xFFFFFFFF}
    s = _load("kgsigs_b9_sha3")
    # the SHA3 fixture is the first nine items: same keys, messages and cases, the other digest
    for key in ("pk", "sign_sk"):
        np.testing.assert_array_equal(s[key], d[key])
    np.testing.assert_array_equal(s["key_idx"], d["key_idx"][:9])
    np.testing.assert_array_equal(s["expect"], d["expect"][:9])
    assert _split(s["msg_blob"], s["msg_off"]) == _split(d["msg_blob"], d["msg_off"])[:9]
    assert not (s["h"] == d["h"][:9]).all(axis=1).any()


@pytest.mark.parametrize("name,digest,picks", [("kgsigs_b65", "sha256", [0, 1, 2, 10, 31, 33, 63, 64]),
                                               ("kgsigs_b9_sha3", "sha3_256", [0, 1, 6, 7])])
def test_kgsigs_fixture_against_the_oracle(name, digest, picks):
    d = _load(name)
    msgs = _split(d["msg_blob"], d["msg_off"])
    sk = int.from_bytes(d["sign_sk"].tobytes(), "big")
    for i in picks:
        h = tc.hash_g2(msgs[i], digest)
        assert bls.g2_compress(h) == d["h"][i].tobytes()
        P = bls.g1_decompress(d["pk"][int(d["key_idx"][i])].tobytes())
        S = bls.g2_decompress(d["sig"][i].tobytes())
        assert tc.verify_sig(P, S, msgs[i], digest, h) == (d["expect"][i] == 1), i
        assert bls.g2_compress(bls.g2_mul(h, sk)) == d["expect_sig"][i].tobytes()
    # every UNDECODABLE item has a key or a signature that does not deserialise
    for i in np.flatnonzero(d["expect"] == 3):
        bad = 0
        for dec, b in ((bls.g1_decompress, d["pk"][int(d["key_idx"][i])].tobytes()), (bls.g2_decompress, d["sig"][i].tobytes())):
            try:
                dec(b)
            except ValueError:
                bad += 1
        assert bad, i


# ---- dhb_kg fixtures and the replay -----------------------------------------------------------------
def _items(d, era):
    ser = _split(d["ser_blob"], d["ser_off"])
    items = []
    for k, m in enumerate(d["item_msg"]):
        kind, _, body = era["msgs"][int(m)]
        sender = int(d["item_sender"][k])
        items.append((int(d["item_proposer"][k]), int(d["item_epoch"][k]), None if sender < 0 else sender, kind, body,
                      ser[k], d["item_sig"][k].tobytes()))
    return items


def _model(d, era):
    t, me = int(era["t"]), int(era["me"])
    sks = [int.from_bytes(s.tobytes(), "big") for s in era["sk_nodes"]]
    pks = [bls.g1_decompress(p.tobytes()) for p in era["pk_nodes"]]
    cand = (int(d["cand_idx"]), bls.g1_decompress(d["cand_pk"].tobytes()))
    assert cand[1] == bls.g1_mul(bls.G1_GEN, int.from_bytes(d["cand_sk"].tobytes(), "big"))
    return dhb.DhbKeyGenModel(skg.SyncKeyGenModel(me, sks[me], pks, t), pks, cand, int(d["start_epoch"]))


@pytest.mark.parametrize("name", ["dhb_kg_n4", "dhb_kg_n7"])
def test_dhb_fixture_shape_and_signature_verdicts(name):
    """The fixture's own consistency, and the oracle's verdict on every item that is not a plain honest
    one plus three that are (the whole era goes through the model once, in the n = 4 test below)."""
    d = _load(name)
    era = load_era(str(d["base"]))
    items = _items(d, era)
    for it in items:
        assert it[5] == dhb.ser_kg_msg(it[3], it[4])
    out = d["expect_outcome"].tolist()
    live = [k for k, o in enumerate(out) if o != dhb.OBSOLETE]
    assert [k for k, it in enumerate(items) if it[1] >= int(d["start_epoch"])] == live
    assert len(live) == len(d["expect_status"]) and dhb.OBSOLETE in out
    assert [out[k] != dhb.BAD_SIGNATURE for k in live] == (d["expect_status"] == 1).tolist()
    assert {0, 1, 3, 5} <= set(d["expect_status"].tolist())
    bad = [k for k in live if out[k] == dhb.BAD_SIGNATURE]
    assert d["fault_proposer"].tolist() == [items[k][0] for k in bad]
    cand = [k for k in live if items[k][2] == int(d["cand_idx"])]
    assert len(cand) == 1 and out[cand[0]] == skg.OUT_OK
    model = _model(d, era)
    honest = [k for k in live if out[k] != dhb.BAD_SIGNATURE and k not in cand][:3]
    obsolete = [k for k, o in enumerate(out) if o == dhb.OBSOLETE]
    for k in bad + cand + honest + obsolete:  # an obsolete item is skipped whatever its signature says
        _, _, sender, _, _, ser, sig = items[k]
        assert model.verify_signature(sender, sig, ser) == (out[k] != dhb.BAD_SIGNATURE), k
    # the Acks that lost their signatures leave one Part incomplete: the unsigned era's keys are others
    assert d["sk_me"].tobytes() != era["sk_me"].tobytes()
    assert d["pk_commit"].tobytes() != era["pk_commit"].tobytes()


def test_model_reproduces_fixture_n4():
    d = _load("dhb_kg_n4")
    era = load_era("skg_n4")
    items = _items(d, era)
    model = _model(d, era)
    rnd = {k: [int.from_bytes(r.tobytes(), "big") for r in era["ack_r_by_msg"][int(m)]]
           for k, m in enumerate(d["item_msg"]) if era["msgs"][int(m)][0] == skg.PART}
    out, _ = model.run(items, rnd)
    assert out == d["expect_outcome"].tolist()
    assert model.faults == [(int(p), dhb.FAULT_INVALID_SIGNATURE) for p in d["fault_proposer"]]
    pk_commit, sk_me = model.skg.generate()
    assert b"".join(bls.g1_compress(c) for c in pk_commit) == d["pk_commit"].tobytes()
    assert sk_me.to_bytes(32, "big") == d["sk_me"].tobytes()


class _FixtureContext:
    """Answers verify_sigs_keyed from the fixture's statuses and records what it was asked."""

    def __init__(self, statuses):
        self.statuses = np.asarray(statuses, dtype=np.uint8)
        self.calls = []

    def verify_sigs_keyed(self, pk48, key_idx, msgs, sig96):
        assert key_idx.dtype == np.uint32 and sig96.shape == (len(msgs), 96) and len(key_idx) == len(msgs)
        self.calls.append(("verify_sigs_keyed", pk48.copy(), key_idx.copy(), list(msgs), sig96.copy()))
        return self.statuses, np.zeros(pk48.shape[0], dtype=np.int32)

    def sign_msgs(self, sk32, msgs):
        self.calls.append(("sign_msgs", sk32, list(msgs)))
        return np.zeros((len(msgs), 96), dtype=np.uint8)


class _KeyGenStub:
    """A KeyGenReplay stand-in: records the one handle_messages call, answers OUT_OK / OUT_ACK."""

    def __init__(self, ctx):
        self.ctx, self.sec_key, self.calls = ctx, bytes([7]) * 32, []

    def handle_messages(self, msgs, ack_randomness=None):
        self.calls.append((list(msgs), ack_randomness))
        out = [1 if kind == skg.PART else 3 for kind, _, _ in msgs]
        return out, {a: ("ack", a) for a, o in enumerate(out) if o == 1}


@pytest.mark.parametrize("name", ["dhb_kg_n4", "dhb_kg_n7"])
def test_replay_over_a_stand_in_context(name):
    d = _load(name)
    era = load_era(str(d["base"]))
    n = int(era["n"])
    items = _items(d, era)
    ctx = _FixtureContext(d["expect_status"])
    kg = _KeyGenStub(ctx)
    rp = SignedKeyGenReplay(kg, era["pk_nodes"], (int(d["cand_idx"]), d["cand_pk"].tobytes()), int(d["start_epoch"]))
    rnd = {k: k for k, it in enumerate(items) if it[3] == skg.PART}
    out, acks = rp.handle_batch(items, rnd)
    live = [k for k, it in enumerate(items) if it[1] >= int(d["start_epoch"])]
    good = [k for k, s in zip(live, d["expect_status"]) if s == 1]
    # one verify call, for the non-obsolete items in order, over the validators' table plus the candidate
    assert [c[0] for c in ctx.calls] == ["verify_sigs_keyed"]
    _, table, key_idx, msgs, sigs = ctx.calls[0]
    np.testing.assert_array_equal(table, np.concatenate([era["pk_nodes"], d["cand_pk"].reshape(1, 48)]))
    assert msgs == [items[k][5] for k in live]
    np.testing.assert_array_equal(sigs, d["item_sig"][live])
    want_idx = [hbx.NO_KEY if items[k][2] is None else items[k][2] for k in live]
    assert key_idx.tolist() == want_idx and n in want_idx and hbx.NO_KEY in want_idx
    # one handle_messages call with the survivors, in order, and their randomness re-keyed
    assert len(kg.calls) == 1
    passed, passed_rnd = kg.calls[0]
    assert [(m[0], m[1]) for m in passed] == [(items[k][3], items[k][2]) for k in good]
    assert all(m[2] is items[k][4] for m, k in zip(passed, good))
    assert passed_rnd == {a: k for a, k in enumerate(good) if k in rnd}
    # outcomes: obsolete skipped, bad signatures flagged, the rest what handle_messages said
    for k, it in enumerate(items):
        if k not in live:
            assert out[k] == OBSOLETE
        elif k not in good:
            assert out[k] == BAD_SIGNATURE
        else:
            assert out[k] == (1 if it[3] == skg.PART else 3)
    assert rp.faults == [(items[k][0], FAULT_INVALID_SIGNATURE) for k in live if k not in good]
    assert rp.faults == [(int(p), FAULT_INVALID_SIGNATURE) for p in d["fault_proposer"]]
    assert acks == {k: ("ack", a) for a, k in enumerate(good) if items[k][3] == skg.PART}
    # signing goes through sign_msgs with the node's key
    rp.sign([b"x", b"yz"])
    assert ctx.calls[-1] == ("sign_msgs", kg.sec_key, [b"x", b"yz"])


def test_replay_with_nothing_to_verify_makes_no_call():
    ctx = _FixtureContext([])
    kg = _KeyGenStub(ctx)
    rp = SignedKeyGenReplay(kg, np.zeros((4, 48), dtype=np.uint8), None, start_epoch=5)
    out, acks = rp.handle_batch([(0, 4, 1, skg.ACK, (0, []), b"", bytes(96))])
    assert out == [OBSOLETE] and acks == {} and ctx.calls == [] and kg.calls == [] and rp.faults == []
    assert rp._key_slot(4) == hbx.NO_KEY  # no candidate: index n has no key


def test_replay_argument_guards():
    kg = _KeyGenStub(_FixtureContext([]))
    with pytest.raises(ValueError, match="pub_keys"):
        SignedKeyGenReplay(kg, np.zeros((4, 47), dtype=np.uint8))
    with pytest.raises(ValueError, match="48 bytes"):
        SignedKeyGenReplay(kg, np.zeros((4, 48), dtype=np.uint8), (4, bytes(47)))
    with pytest.raises(ValueError, match="index"):
        SignedKeyGenReplay(kg, np.zeros((4, 48), dtype=np.uint8), (2, bytes(48)))
