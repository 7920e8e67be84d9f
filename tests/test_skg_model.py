"""The CPU restatement of sync_key_gen.rs (tests/skg_model.py): the reference's own property
(tests/sync_key_gen.rs:16-92) at n = 4, and the model's outcomes against the committed fixtures."""
import numpy as np
import pytest

import skg_model as skg
from oracle import bivar
from oracle import bls12_381 as bls
from oracle import threshold as tc
from oracle.chacha_rand04 import ChaChaRng04
from skg_fixture import load_era


def test_reference_property_n4():
    """Every node deals, handles every Part and every Ack; then every generated share signs, the share
    verifies under public_key_share(i), and t + 1 signatures combine to one the master key accepts."""
    n, t = 4, 1
    rng = ChaChaRng04([0x68626278, 0x70726F70])
    sks = [tc.fr_rand(rng) for _ in range(n)]
    pks = [bls.g1_mul(bls.G1_GEN, s) for s in sks]
    nodes = [skg.SyncKeyGenModel(i, sks[i], pks, t) for i in range(n)]
    rand = lambda: [tc.fr_rand(rng) for _ in range(n)]  # noqa: E731
    parts = [nodes[q].dealer_part(bivar.BivarPoly(t, [tc.fr_rand(rng) for _ in range(bivar.n_coeffs(t))]), rand())
             for q in range(n)]
    acks = []
    for q in range(n):
        for i, node in enumerate(nodes):
            out, ack = node.handle_part(q, parts[q], rand())
            assert out == skg.OUT_ACK
            acks.append((i, ack))
    for sender, ack in acks:
        for node in nodes:
            assert node.handle_ack(sender, ack) == skg.OUT_OK
    gen = [node.generate() for node in nodes]
    assert all(node.is_ready() and node.count_complete() == n for node in nodes)
    pk_set = tc.PublicKeySet(gen[0][0])
    assert all(g[0] == gen[0][0] for g in gen)
    msg = b"Nodes 0 and 1 does not agree with this."
    sigs = []
    for i in range(t + 1):
        sig = tc.sign(gen[i][1], msg)
        assert tc.verify_sig(pk_set.public_key_share(i), sig, msg)
        sigs.append((i, sig))
    assert tc.verify_sig(pk_set.public_key(), tc.combine_signatures(pk_set, sigs), msg)


@pytest.mark.parametrize("name", ["skg_n4", "skg_n7"])
def test_model_reproduces_fixture(name):
    d = load_era(name)
    n, t, me = int(d["n"]), int(d["t"]), int(d["me"])
    pks = [bls.g1_decompress(p.tobytes()) for p in d["pk_nodes"]]
    sk = int.from_bytes(d["sk_nodes"][me].tobytes(), "big")
    model = skg.SyncKeyGenModel(me, sk, pks, t)
    ack_r = {k: [int.from_bytes(r.tobytes(), "big") for r in rows] for k, rows in d["ack_r_by_msg"].items()}
    out, acks = model.run(d["msgs"], ack_r)
    assert out == d["outcome"].tolist()
    assert sorted(acks) == [k for k, o in enumerate(out) if o == skg.OUT_ACK]
    for k, (proposer, values) in acks.items():
        assert proposer == d["msgs"][k][1]
        assert values == d["exp_ack_by_msg"][k], k
    assert [int(model.is_complete(q)) for q in range(n)] == d["complete"].tolist()
    assert int(model.is_ready()) == int(d["is_ready"])
    pk_commit, sk_share = model.generate()
    assert [bls.g1_compress(c) for c in pk_commit] == [c.tobytes() for c in d["pk_commit"]]
    assert sk_share.to_bytes(32, "big") == d["sk_me"].tobytes() == d["sk_all"][me].tobytes()
    # the dealer Part is the node's own Part of the message list
    poly = bivar.BivarPoly(t, [int.from_bytes(c.tobytes(), "big") for c in d["dealer_coeffs"]])
    part = model.dealer_part(poly, [int.from_bytes(r.tobytes(), "big") for r in d["dealer_r"]])
    assert part == d["msgs"][int(d["dealer_msg"])][2]
    if name == "skg_n7":
        kinds = {"invalid_part": skg.OUT_INVALID_PART, "invalid_ack": skg.OUT_INVALID_ACK}
        assert out.count(kinds["invalid_part"]) == 2 and out.count(kinds["invalid_ack"]) == 6
        assert len(d["msgs"][0][2][1][me][1]) == 96  # the row plaintext takes the |m| > 64 digest branch
        assert d["complete"].tolist() == [1, 0, 0, 1, 0, 0, 1]
