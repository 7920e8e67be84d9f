"""The SyncKeyGen methods of hbbft_amd.hbx.Context refuse mismatched buffers before the library is
reached (the C ABI reads count * 48 / count * 32 / p * (t + 1) * 32 bytes from them), and the
committed fixtures are what their generator's docstring says.  No GPU."""
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library with mismatched arguments")


def _bare_context():
    from hbbft_amd import hbx

    ctx = object.__new__(hbx.Context)  # no device: only the argument checks run
    ctx.lib, ctx.h = _NoLib(), None
    return ctx


def test_keygen_methods_reject_mismatched_shapes():
    ctx = _bare_context()
    z = np.zeros
    with pytest.raises(ValueError, match="encrypt_to"):
        ctx.encrypt_to(z((2, 48), np.uint8), [b"a", b"b", b"c"], z((3, 32), np.uint8))
    with pytest.raises(ValueError, match="encrypt_to"):
        ctx.encrypt_to(z((3, 48), np.uint8), [b"a", b"b", b"c"], z((2, 32), np.uint8))
    with pytest.raises(ValueError, match="sk_decrypt"):
        ctx.sk_decrypt(bytes(31), [(bytes(48), b"", bytes(96))])
    with pytest.raises(ValueError, match="sk_decrypt"):
        ctx.sk_decrypt(bytes(32), [(bytes(47), b"", bytes(96))])
    with pytest.raises(ValueError, match="bivar_poly_rows"):
        ctx.bivar_poly_rows(z((5, 32), np.uint8), 2, 7)  # t = 2 has 6 coefficients
    with pytest.raises(ValueError, match="fr_poly_eval"):
        ctx.fr_poly_eval(z((3, 32), np.uint8), 7)
    with pytest.raises(ValueError, match="keygen_generate"):
        ctx.keygen_generate(z((4, 5, 48), np.uint8), 2, np.ones(4))
    with pytest.raises(ValueError, match="keygen_generate"):
        ctx.keygen_generate(z((4, 6, 48), np.uint8), 2, np.ones(3))
    with pytest.raises(ValueError, match="keygen_generate"):
        ctx.keygen_generate(z((4, 6, 48), np.uint8), 2, np.ones(4), np.full(4, 3), z((4, 2), np.uint64),
                            z((4, 3, 32), np.uint8))
    with pytest.raises(ValueError, match="pk_shares_from_commit"):
        ctx.pk_shares_from_commit(z((3, 47), np.uint8), 7)


def test_batch65_fixture_shape():
    d = dict(np.load(os.path.join(GOLDEN, "skg_batch65.npz"), allow_pickle=False))
    lens = np.diff(d["off"]).astype(int).tolist()
    assert len(lens) == 65 and lens == [(0, 1, 32, 64, 65, 96)[j % 6] for j in range(65)]
    st = d["expect_status"]
    assert st[7] == 0 and st[21] == 3 and st[64] == 1 and int((st == 1).sum()) == 63
    assert len(d["v_blob"]) == len(d["msg_blob"]) == len(d["expect_plain"]) == len(d["to_v"]) == sum(lens)
    # the tampered entries differ from the honest encryption exactly where the docstring says
    assert (d["u"] == d["enc_u"]).all()
    assert (np.flatnonzero((d["w"] != d["enc_w"]).any(axis=1)) == [21]).all()
    assert (np.flatnonzero(d["v_blob"] != d["enc_v"]) == [int(d["off"][7])]).all()
    for key in ("sk", "r", "sk_to", "r_to"):
        for row in d[key].reshape(-1, 32):
            assert int.from_bytes(row.tobytes(), "big") < R


@pytest.mark.parametrize("n", [4, 7])
def test_gen_fixture_shares_lie_on_the_summed_polynomial(n):
    """sk_all[i] = sum over the complete parts of f_q(i + 1, 0), in Python integers."""
    g = dict(np.load(os.path.join(GOLDEN, f"skg_gen_n{n}.npz"), allow_pickle=False))
    t = int(g["t"])
    assert int(g["n"]) == n and t == (n - 1) // 3
    assert g["complete"].tolist() == [1] * (n - 1) + [0]
    for i in range(n):
        acc = 0
        for q in range(n):
            if g["complete"][q]:
                # f_q(x, 0) = sum_i a_i0 x^i, a_i0 stored at coeff_pos(0, i) = i (i + 1) / 2
                acc += sum(int.from_bytes(g["coeffs"][q][k * (k + 1) // 2].tobytes(), "big") * pow(i + 1, k, R)
                           for k in range(t + 1))
        assert int.from_bytes(g["sk_all"][i].tobytes(), "big") == acc % R
    assert g["commits"][0][t * (t + 1) // 2].tobytes() == bytes([0xC0]) + bytes(47)  # g1 * 0
