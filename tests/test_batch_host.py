"""The batched share verification's arithmetic (hbbft_amd/csrc/batchd.hpp) compiled for the CPU by g++
(tools/hostcheck/batchcheck.cpp) and compared with the oracle: the coefficient derivation against
hashlib, one lane's 128-bit scalar multiplication, and the block reduction's complete addition
(equal, opposite and identity operands).  The -m gpu tests (test_gpu_batch_verify.py) then pin the
kernels against the fixture this same oracle wrote (tests/golden/batch_sums.npz)."""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
INF48 = bytes([0xC0]) + bytes(47)


@pytest.fixture(scope="module")
def bc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("batchcheck") / "libbatchcheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "batchcheck.cpp")])
    lib = ctypes.CDLL(out)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    lib.bc_coeff.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, u32p]
    lib.bc_term.argtypes = [ctypes.c_char_p, u32p, ctypes.c_char_p]
    lib.bc_reduce.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    lib.bc_column.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64,
                              ctypes.c_char_p]
    return lib


def _coeff(seed, call, i):
    d = hashlib.sha256(seed + call.to_bytes(8, "little") + i.to_bytes(4, "little")).digest()
    return int.from_bytes(d[:16], "little")


def _words(r):
    return (ctypes.c_uint32 * 4)(*[(r >> (32 * k)) & 0xFFFFFFFF for k in range(4)])


def _points(count, seed):
    """`count` distinct G1 points: a random start and repeated additions of a second point."""
    rnd = random.Random(seed)
    base = bls.g1_mul(bls.G1_GEN, rnd.randrange(1, bls.R))
    step = bls.g1_mul(bls.G1_GEN, rnd.randrange(1, bls.R))
    pts = []
    for _ in range(count):
        pts.append(base)
        base = bls.g1_add(base, step)
    return pts


def test_coefficients_match_hashlib(bc):
    rnd = random.Random(3)
    for seed in (bytes(32), bytes(range(32)), rnd.randbytes(32)):
        for call in (0, 1, 2, 255, 256, (1 << 32) + 5, (1 << 64) - 1):
            for i in (0, 1, 63, 64, 255, 256, 65535, 0xFFFFFFFE, 0xFFFFFFFF):
                out = (ctypes.c_uint32 * 4)()
                bc.bc_coeff(seed, call, i, out)
                assert sum(int(out[k]) << (32 * k) for k in range(4)) == _coeff(seed, call, i), (call, i)


def test_coefficients_match_committed_fixture(bc):
    g = dict(np.load(os.path.join(GOLDEN, "batch_sums.npz"), allow_pickle=False))
    seed = g["seed"].tobytes()
    for key in ("n7", "c65", "c256"):
        for call in (0, 1):
            want = g[f"coeff_{key}_{call}"]
            n = want.shape[0] - 1
            for row, i in [(k, k) for k in range(n)] + [(n, 0xFFFFFFFF)]:
                out = (ctypes.c_uint32 * 4)()
                bc.bc_coeff(seed, call, i, out)
                assert bytes(out) == want[row].tobytes(), (key, call, i)


def test_lane_scalar_multiplication(bc):
    """r in {0, 1, 2^128 - 1, scalars with zero nibbles (leading, inner, trailing), random}."""
    rnd = random.Random(5)
    rs = [0, 1, 2, 15, 16, (1 << 128) - 1, 1 << 127, 0xF << 124, 0xF000000000000000000000000000000F,
          0x0000000000000000FFFFFFFFFFFFFFFF, 0x10000000000000000000000000000000, 0x000F000F000F000F000F000F000F0000,
          0xA0B0C0D0E0F0102030405060708090A0] + [rnd.getrandbits(128) for _ in range(12)]
    for pt in _points(2, 7):
        comp = bls.g1_compress(pt)
        for r in rs:
            out = ctypes.create_string_buffer(48)
            assert bc.bc_term(comp, _words(r), out) == 0
            assert out.raw == bls.g1_compress(bls.g1_mul(pt, r) if r else None), hex(r)


def _reduce(bc, pts):
    blob = b"".join(bls.g1_compress(p) for p in pts)
    out = ctypes.create_string_buffer(48)
    assert bc.bc_reduce(blob, len(pts), out) == 0
    return out.raw


def _oracle_sum(pts):
    acc = None
    for p in pts:
        acc = bls.g1_add(acc, p)
    return bls.g1_compress(acc)


def test_reduction_special_operands(bc):
    """P + P, P + (-P), P + O, O + P and O + O, alone and at every position pair that the wave fold
    and the cross-wave sum bring together (neighbours, half a wave apart, two waves)."""
    P, Q = _points(2, 11)
    for pts in ([P, P], [P, bls.g1_neg(P)], [P, None], [None, P], [None, None], [P, P, P], [P, bls.g1_neg(P), Q],
                [None] * 5):
        assert _reduce(bc, pts) == _oracle_sum(pts)
    for a, b in ((0, 1), (0, 32), (5, 37), (0, 64), (63, 64), (10, 200), (0, 255)):
        for other in (P, bls.g1_neg(P), None):
            pts = [None] * 256
            pts[a], pts[b] = P, other
            assert _reduce(bc, pts) == _oracle_sum(pts), (a, b)
    # a whole column of one repeated point and of cancelling pairs
    assert _reduce(bc, [P] * 65) == bls.g1_compress(bls.g1_mul(P, 65))
    assert _reduce(bc, [P, bls.g1_neg(P)] * 32) == INF48


@pytest.mark.parametrize("n", [1, 7, 64, 65, 256, 257])
def test_reduction_operand_counts(bc, n):
    pts = _points(n, 100 + n)
    assert _reduce(bc, pts) == _oracle_sum(pts)


@pytest.mark.parametrize("n", [1, 7, 64, 65])
def test_column_sum_matches_oracle(bc, n):
    """The whole lane-and-reduce pipeline on one column with duplicates, negations and gaps."""
    rnd = random.Random(200 + n)
    seed = rnd.randbytes(32)
    pts = _points(n, 300 + n)
    if n >= 7:
        pts[3] = pts[1]                 # a share copied over another's
        pts[5] = bls.g1_neg(pts[2])     # a negated share
    include = bytes(0 if (n >= 7 and i == 4) else 1 for i in range(n))
    blob = b"".join(bls.g1_compress(p) for p in pts)
    for call in (0, 1):
        out = ctypes.create_string_buffer(48)
        assert bc.bc_column(blob, include, n, seed, call, out) == 0
        acc = None
        for i in range(n):
            if include[i]:
                acc = bls.g1_add(acc, bls.g1_mul(pts[i], _coeff(seed, call, i)))
        assert out.raw == bls.g1_compress(acc)


def test_column_sum_matches_committed_fixture(bc):
    """batch_sums.npz (what the GPU test compares hbx_get_batch_sums with) against the host build, on
    the n = 256 column with invalid shares and its 65-sender slice."""
    g = dict(np.load(os.path.join(GOLDEN, "batch_sums.npz"), allow_pickle=False))
    d = dict(np.load(os.path.join(GOLDEN, "hb_cols_n256.npz"), allow_pickle=False))
    j = 2
    for key, n in (("c65", 65), ("c256", 256)):
        st = d["expect_share_status"][j, :n]
        include = bytes(int(d["present"][j, i]) and int(st[i] in (0, 1)) for i in range(n))
        out = ctypes.create_string_buffer(48)
        assert bc.bc_column(d["shares"][j, :n].tobytes(), include, n, g["seed"].tobytes(), 1, out) == 0
        assert out.raw == g[f"sums_{key}_1"][j].tobytes()
