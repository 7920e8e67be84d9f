"""GPU parity of the SyncKeyGen driver (hbbft_amd/sync_key_gen.py KeyGenReplay) with the model's
fixtures skg_n4 / skg_n7 (tests/skg_model.py through tests/golden/make_skg_golden.py --era): every
per-message outcome, every byte of every Ack produced, completeness, generate(), the dealer Part,
and the installed keys used for a threshold decryption.  Bit-exact."""
import numpy as np
import pytest

from skg_fixture import ACK, PART, load_era


def _to_driver(msgs):
    """Fixture messages (commit as a list of bytes) -> the driver's (commit uint8[M, 48])."""
    out = []
    for kind, sender, body in msgs:
        if kind == PART:
            commit = np.frombuffer(b"".join(body[0]), dtype=np.uint8).reshape(-1, 48)
            out.append((kind, sender, (commit, body[1])))
        else:
            out.append((kind, sender, body))
    return out


def _replay(ctx, d, our_idx="me"):
    from hbbft_amd.sync_key_gen import KeyGenReplay

    me = int(d["me"]) if our_idx == "me" else our_idx
    sk = d["sk_nodes"][int(d["me"])].tobytes()
    return KeyGenReplay(ctx, me, sk, d["pk_nodes"], int(d["t"]))


@pytest.fixture(scope="module", params=["skg_n4", "skg_n7"])
def era(request):
    return load_era(request.param)


@pytest.mark.gpu
def test_replay_outcomes_acks_and_generate(hbx_ctx, era):
    d = era
    n = int(d["n"])
    kg = _replay(hbx_ctx, d)
    out, acks = kg.handle_messages(_to_driver(d["msgs"]), d["ack_r_by_msg"])
    assert list(out) == d["outcome"].tolist()
    assert sorted(acks) == [k for k, o in enumerate(out) if o == 1]
    for k, (proposer, values) in acks.items():
        assert proposer == d["msgs"][k][1]
        assert values == d["exp_ack_by_msg"][k], k
    assert [int(kg.is_node_ready(q)) for q in range(n)] == d["complete"].tolist()
    assert kg.count_complete() == int(d["complete"].sum())
    assert int(kg.is_ready()) == int(d["is_ready"])
    pkc, sk = kg.generate()
    np.testing.assert_array_equal(pkc, d["pk_commit"])
    assert sk == d["sk_me"].tobytes()


@pytest.mark.gpu
def test_replay_message_by_message_equals_one_batch(hbx_ctx, era):
    """The state carries over between calls: one message per call gives the same outcomes."""
    d = era
    kg = _replay(hbx_ctx, d)
    msgs = _to_driver(d["msgs"])
    out = []
    for k, m in enumerate(msgs):
        r = {0: d["ack_r_by_msg"][k]} if m[0] == PART else None
        o, _ = kg.handle_messages([m], r)
        out.append(o[0])
    assert out == d["outcome"].tolist()
    assert kg.generate()[1] == d["sk_me"].tobytes()


@pytest.mark.gpu
def test_replay_observer(hbx_ctx, era):
    """An observer decrypts nothing: no Ack, every structurally sound ack passes, no secret share."""
    d = era
    n = int(d["n"])
    kg = _replay(hbx_ctx, d, our_idx=None)
    out, acks = kg.handle_messages(_to_driver(d["msgs"]), d["ack_r_by_msg"])
    assert acks == {}
    seen, counted, want = set(), {}, []
    for kind, sender, body in d["msgs"]:
        if kind == PART:
            if sender is not None and sender not in seen:
                seen.add(sender)
            want.append(0)
        elif sender is None:
            want.append(3)
        elif len(body[1]) != n or body[0] not in seen or sender in counted.setdefault(body[0], set()):
            want.append(4)
        else:
            counted[body[0]].add(sender)
            want.append(3)
    assert list(out) == want
    assert [int(kg.is_node_ready(q)) for q in range(n)] == d["complete"].tolist()
    pkc, sk = kg.generate()
    np.testing.assert_array_equal(pkc, d["pk_commit"])
    assert sk is None


@pytest.mark.gpu
def test_dealer_part_matches_fixture(hbx_ctx, era):
    d = era
    kg = _replay(hbx_ctx, d)
    commit, rows = kg.dealer_part(d["dealer_coeffs"], d["dealer_r"])
    want_commit, want_rows = d["msgs"][int(d["dealer_msg"])][2]
    assert [c.tobytes() for c in commit] == want_commit
    assert rows == want_rows


@pytest.mark.gpu
def test_install_then_threshold_decrypt(hbx_ctx):
    """install() the n7 result, encrypt to the new master key, all seven nodes' decryption shares,
    prepare / verify / combine at t + 1: the message comes back with every share valid."""
    d = load_era("skg_n7")
    n, t, me = int(d["n"]), int(d["t"]), int(d["me"])
    kg = _replay(hbx_ctx, d)
    kg.handle_messages(_to_driver(d["msgs"]), d["ack_r_by_msg"])
    try:
        pkc, sk, pk_shares = kg.install()
        np.testing.assert_array_equal(pk_shares, d["pk_shares"])
        assert sk == d["sk_all"][me].tobytes()
        msg = bytes(range(70))
        r = np.frombuffer((0xA5A5 << 200 | 12345).to_bytes(32, "big"), dtype=np.uint8).reshape(1, 32)
        cts = hbx_ctx.encrypt(pkc[0].tobytes(), [msg], r)
        shares = hbx_ctx.decrypt_shares(d["sk_all"], np.frombuffer(cts[0][0], dtype=np.uint8).reshape(1, 48))
        assert hbx_ctx.prepare_ciphertexts(cts).all()
        assert hbx_ctx.verify_dec_shares(shares).all()
        assert (hbx_ctx.share_status(1, n) == 1).all()
        plains, status = hbx_ctx.combine_decrypt(t + 1)
        assert status[0] == 0 and plains[0] == msg
    finally:
        hbx_ctx.set_own_share(me, None)


def test_raw_codec():
    from hbbft_amd.sync_key_gen import R, RawCodec

    c = RawCodec()
    row = [0, 1, R - 1]
    assert c.decode_row(c.encode_row(row), 2) == row
    assert c.decode_row(c.encode_row(row)[:95], 2) is None
    assert c.decode_row(c.encode_row(row), 1) is None
    assert c.decode_row(R.to_bytes(32, "big") * 3, 2) is None
    assert c.decode_val(c.encode_val(R - 1)) == R - 1
    assert c.decode_val(R.to_bytes(32, "big")) is None
    assert c.decode_val(bytes(31)) is None
