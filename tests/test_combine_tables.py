"""The combine's precomputed window tables (g1d.hpp g1d_build_tables / g1d_mul_u128_tab; built by
k_prepare_lines in hbx_decrypt_epoch_d, read by k_combine).

Host: the table path gives the same point as g1d_mul_u128_w4 and as the 12-limb multiplication.
GPU: the fused epoch call at the smallest shapes that can still go wrong -- outputs equal the
contributions and the oracle's combine, and are byte-identical with the tables off (the path
before the tables existed); terms without tables take the slow path and are counted; tables of a
fused call are not used by a later three-call sequence on other ciphertexts.

The tables belong to the one-lane-per-term combine (k_combine, what a full N = 256 epoch uses);
launches this small default to the quad combine, so the GPU tests select it by
set_combine_lanes(1) and run the default once for comparison."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import threshold as tc
from oracle.chacha_rand04 import ChaChaRng04

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck_tab") / "libhostcheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHBX_DCHECK", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "hostcheck.cpp")])
    lib = ctypes.CDLL(out)
    lib.hc_g1_mul_u128_tab_cmp.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64]
    return lib


def _k4(k):
    return (ctypes.c_uint32 * 4)(*[(k >> (32 * i)) & 0xFFFFFFFF for i in range(4)])


def test_g1_mul_u128_tables_host(hc):
    """g1d_mul_u128_tab over tables from g1d_build_tables equals g1d_mul_u128_w4 and the 12-limb
    g1_mul_u128_w4, for P and phi(P), tables from an affine and from a Jacobian point, and with the
    table of S built apart: random 128-bit scalars, zero, k_hi = 0, k_lo = 0, all-ones nibbles,
    single windows, the window boundary at 2^64; the identity has no tables and multiplies to O."""
    rnd = random.Random(41)
    ones = (1 << 128) - 1
    lo, hi = (1 << 64) - 1, ((1 << 64) - 1) << 64
    ks = [0, 1, 15, 16, lo, hi, ones, 1 << 64, (1 << 64) - 1, (1 << 64) + 1, 0xF << 60, 0xF << 124, 1 << 127,
          rnd.getrandbits(64), rnd.getrandbits(64) << 64, 0x1111_1111_1111_1111_1111_1111_1111_1111]
    ks += [rnd.getrandbits(128) for _ in range(8)]
    for z0 in (3, 0xFFFFFFFF12345678):
        p = bls.g1_compress(bls.g1_mul(bls.G1_GEN, rnd.randrange(1, bls.R)))
        for k in ks:
            assert hc.hc_g1_mul_u128_tab_cmp(p, _k4(k), z0) == 1, hex(k)
    inf = bytes([0xC0]) + bytes(47)
    for k in (0, 1, ones):
        assert hc.hc_g1_mul_u128_tab_cmp(inf, _k4(k), 3) == 2, hex(k)


# ---- GPU -----------------------------------------------------------------------------------------
SHAPES = [(5, 2), (13, 5), (70, 24)]  # (n, t): t shares combine; n = 70 crosses the 64-sender wave, cap = 64 != n
P = 2  # proposers


def _be32(x):
    return np.frombuffer(x.to_bytes(32, "big"), dtype=np.uint8)


_EPOCHS = {}


def _epoch(ctx, n, t, tag=0):
    """One epoch of P ciphertexts under a fresh (t - 1)-threshold key set, made once per shape.
    Ciphertexts by the oracle; key shares' public keys and the honest decryption shares by the
    producer kernels (pinned to the oracle by tests/test_gpu_threshold.py).  `corrupt`: senders
    inside the first t whose share is replaced by another sender's (a point of G1, so it decodes
    and fails its pairing check) -- the valid set then skips indices."""
    key = (n, t, tag)
    if key in _EPOCHS:
        return _EPOCHS[key]
    rng = ChaChaRng04([0x68626278, 0x746162, n, tag])
    sks = tc.SecretKeySet.random(t - 1, rng)
    sk = np.stack([_be32(sks.secret_key_share(i)) for i in range(n)])
    pk_comp = ctx.public_keys(sk)
    mpk = bls.g1_mul(bls.G1_GEN, sks.secret_key())
    msgs = [bytes((7 * j + i + tag) & 0xFF for i in range(33 + 20 * j)) for j in range(P)]
    cts = [tc.encrypt(mpk, m, tc.fr_rand(rng)) for m in msgs]
    wire = [(bls.g1_compress(u), v, bls.g2_compress(w)) for u, v, w in cts]
    honest = ctx.decrypt_shares(sk, np.stack([np.frombuffer(w[0], np.uint8) for w in wire]))
    corrupt = np.zeros((P, n), dtype=bool)
    corrupt[0, [0, 1] if t == 2 else [1, t - 1]] = True
    corrupt[1, 0 if t == 2 else 2] = True
    shares = honest.copy()
    for j, i in zip(*np.nonzero(corrupt)):
        shares[j, i] = honest[j, (i + 1) % n]
    ep = dict(n=n, t=t, sks=sks, sk=sk, pk_comp=[r.tobytes() for r in pk_comp], cts=cts, wire=wire, msgs=msgs,
              honest=honest, shares=shares, corrupt=corrupt)
    _EPOCHS[key] = ep
    return ep


def _fused(ctx, ep, shares):
    """hbx_decrypt_epoch_d on the epoch's ciphertexts with `shares`: (valid[P, n], ct[P], status[P], out bytes)."""
    import torch

    dev = torch.device("cuda", 0)
    n, t = ep["n"], ep["t"]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    off = np.zeros(P + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(w[1]) for w in ep["wire"]])
    t_u = up(np.frombuffer(b"".join(w[0] for w in ep["wire"]), np.uint8).copy())
    t_v = up(np.frombuffer(b"".join(w[1] for w in ep["wire"]), np.uint8).copy())
    t_w = up(np.frombuffer(b"".join(w[2] for w in ep["wire"]), np.uint8).copy())
    t_off, t_sh = up(off), up(shares)
    t_out = torch.zeros(int(off[-1]), dtype=torch.uint8, device=dev)
    t_valid = torch.zeros(P * n, dtype=torch.uint8, device=dev)
    t_ct = torch.zeros(P, dtype=torch.uint8, device=dev)
    t_st = torch.full((P,), -99, dtype=torch.int32, device=dev)
    ctx.decrypt_epoch_d(t_u, t_v, t_off, t_w, P, int(np.max(np.diff(off))), t_sh, n, t, t_out, d_valid=t_valid,
                        d_ct_valid=t_ct, d_status=t_st)
    return t_valid.cpu().numpy().reshape(P, n), t_ct.cpu().numpy(), t_st.cpu().numpy(), t_out.cpu().numpy().tobytes()


def _expect(ep, res, bad, me=None):
    """Validity = every share but the corrupted ones (the own share is computed, so valid), every
    ciphertext valid, every combine OK, plaintexts = the contributions."""
    valid, ct, st, out = res
    want = ~bad
    if me is not None:
        want = want.copy()
        want[:, me] = True
    np.testing.assert_array_equal(valid == 1, want)
    np.testing.assert_array_equal(ct, np.ones(P, np.uint8))
    np.testing.assert_array_equal(st, np.zeros(P, np.int32))
    assert out == b"".join(ep["msgs"])


def _same(a, b):
    for x, y in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(x, y)
    assert a[3] == b[3]


@pytest.fixture
def tab_ctx(hbx_ctx):
    """The session context with the one-lane-per-term combine, restored afterwards."""
    from hbbft_amd.hbx import COMBINE_MARGIN_AUTO

    hbx_ctx.set_combine_lanes(1)
    yield hbx_ctx
    hbx_ctx.set_combine_lanes(0)
    hbx_ctx.debug_set_combine_margin(COMBINE_MARGIN_AUTO)
    hbx_ctx.set_own_share(0, None)


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("n,t", SHAPES)
def test_fused_epoch_with_tables(tab_ctx, n, t, own):
    """Honest and corrupted shares (the valid set skips indices inside the first t), with and
    without the own share: expected outputs, byte-identical with the tables off and with the
    default (quad) combine; no term takes the slow path at the default margin."""
    from hbbft_amd.hbx import COMBINE_MARGIN_AUTO, COMBINE_TABLES_OFF

    ctx = tab_ctx
    ep = _epoch(ctx, n, t)
    assert (ctx.set_pk_shares(ep["pk_comp"]) == 0).all()
    me = 0 if own else None
    if own:
        ctx.set_own_share(0, ep["sk"][0].tobytes())
    none = np.zeros((P, n), dtype=bool)
    for shares, bad in ((ep["honest"], none), (ep["shares"], ep["corrupt"])):
        ctx.debug_set_combine_margin(COMBINE_MARGIN_AUTO)
        res = _fused(ctx, ep, shares)
        assert ctx.combine_slow_terms() == 0
        _expect(ep, res, bad, me)
        ctx.debug_set_combine_margin(COMBINE_TABLES_OFF)
        off = _fused(ctx, ep, shares)
        assert ctx.combine_slow_terms() == 2 * t * P
        _same(res, off)
    ctx.set_combine_lanes(0)
    ctx.debug_set_combine_margin(COMBINE_MARGIN_AUTO)
    _same(res, _fused(ctx, ep, shares))


@pytest.mark.gpu
@pytest.mark.parametrize("n,t", SHAPES)
def test_combine_matches_oracle(tab_ctx, n, t):
    """The plaintext of the table path equals oracle/threshold.py's decrypt over the valid shares
    in index order (PublicKeySet::decrypt: Lagrange over the first t)."""
    ctx = tab_ctx
    ep = _epoch(ctx, n, t)
    assert (ctx.set_pk_shares(ep["pk_comp"]) == 0).all()
    valid, _, st, out = _fused(ctx, ep, ep["shares"])
    assert ctx.combine_slow_terms() == 0
    j = 0
    items = [(i, bls.g1_decompress(ep["shares"][j, i].tobytes())) for i in range(n) if valid[j, i] == 1][:t]
    assert [i for i, _ in items] != list(range(t))  # the valid set does skip indices
    want = tc.decrypt(ep["sks"].public_keys(), items, ep["cts"][j])
    assert st[j] == 0 and out[:len(want)] == want == ep["msgs"][j]


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True])
@pytest.mark.parametrize("n,t", SHAPES)
def test_slow_path_terms(tab_ctx, n, t, own):
    """margin = 0 (tables for senders below t only) with corrupted shares among the first t: the
    valid set reaches beyond cap, those terms multiply from the point (counted), and the outputs
    do not change.  The own node is t + 1, beyond cap, so its tables sit in the spare slot; it is
    among the combined shares of proposer 0 at every shape."""
    from hbbft_amd.hbx import COMBINE_TABLES_OFF

    ctx = tab_ctx
    ep = _epoch(ctx, n, t)
    assert (ctx.set_pk_shares(ep["pk_comp"]) == 0).all()
    me = t + 1 if own else None
    if own:
        ctx.set_own_share(me, ep["sk"][me].tobytes())
    ctx.debug_set_combine_margin(0)
    res = _fused(ctx, ep, ep["shares"])
    slow = ctx.combine_slow_terms()
    _expect(ep, res, ep["corrupt"], me)
    # per proposer, the valid senders at or beyond cap = t among the first t valid ones, two GLV
    # half-terms each; the own share has tables wherever it sits
    want = 0
    for j in range(P):
        first = [i for i in range(n) if not ep["corrupt"][j, i] or i == me][:t]
        want += 2 * sum(1 for i in first if i >= t and i != me)
    assert want > 0 and slow == want
    ctx.debug_set_combine_margin(COMBINE_TABLES_OFF)
    _same(res, _fused(ctx, ep, ep["shares"]))


@pytest.mark.gpu
def test_tables_do_not_leak_into_three_call_api(tab_ctx):
    """A fused call leaves tables of its shares in the context; the three-call API on other
    ciphertexts (same keys) afterwards must decrypt its own, from the points."""
    ctx = tab_ctx
    n, t = 5, 2
    ep, other = _epoch(ctx, n, t), _epoch(ctx, n, t, tag=1)
    # the second epoch's ciphertexts under the first one's keys
    rng = ChaChaRng04([0x68626278, 0x746162, 99])
    mpk = bls.g1_mul(bls.G1_GEN, ep["sks"].secret_key())
    cts = [tc.encrypt(mpk, m, tc.fr_rand(rng)) for m in other["msgs"]]
    wire = [(bls.g1_compress(u), v, bls.g2_compress(w)) for u, v, w in cts]
    shares = ctx.decrypt_shares(ep["sk"], np.stack([np.frombuffer(w[0], np.uint8) for w in wire]))
    assert (ctx.set_pk_shares(ep["pk_comp"]) == 0).all()
    _expect(ep, _fused(ctx, ep, ep["honest"]), np.zeros((P, n), dtype=bool))
    assert ctx.combine_slow_terms() == 0
    assert ctx.prepare_ciphertexts(wire).all()
    assert ctx.verify_dec_shares(shares).all()
    plains, st = ctx.combine_decrypt(t)
    np.testing.assert_array_equal(st, np.zeros(P, np.int32))
    assert plains == other["msgs"]
    assert ctx.combine_slow_terms() == 2 * t * P
