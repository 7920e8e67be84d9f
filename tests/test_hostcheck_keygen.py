"""The SyncKeyGen per-lane arithmetic (hbbft_amd/csrc/keygen.hpp, all __host__ __device__) compiled
for the CPU through tools/hostcheck and compared with Python integers and the oracle.  The -m gpu
tests (test_gpu_keygen.py) then pin the kernels that wrap these functions."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bivar
from oracle import bls12_381 as bls
from oracle import threshold as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = bls.R
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck_keygen") / "libhostcheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHBX_DCHECK", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "hostcheck.cpp")])
    lib = ctypes.CDLL(out)
    lib.hc_fr_poly_eval.argtypes = [ctypes.c_char_p, ctypes.c_uint32, U64, ctypes.c_char_p]
    lib.hc_bivar_poly_row.argtypes = [ctypes.c_char_p, ctypes.c_uint32, U64, ctypes.c_char_p]
    lib.hc_lagrange0_sum.argtypes = [ctypes.POINTER(U64), ctypes.c_char_p, ctypes.c_uint32, ctypes.c_char_p]
    lib.hc_commit_eval.argtypes = [ctypes.c_char_p, ctypes.c_uint32, U64, ctypes.c_char_p]
    lib.hc_sk_decrypt.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, U64, ctypes.c_int,
                                  ctypes.c_char_p]
    return lib


def _be(x):
    return x.to_bytes(32, "big")


def _rand_fr(rnd):
    return rnd.randrange(R)


def test_fr_poly_eval(hc):
    rnd = random.Random(0x6B67_01)
    for deg in (0, 1, 2, 5, 85):
        coeffs = [_rand_fr(rnd) for _ in range(deg + 1)]
        coeffs[rnd.randrange(deg + 1)] = R - 1
        if deg >= 2:
            coeffs[1] = 0
        blob = b"".join(_be(c) for c in coeffs)
        for x in (0, 1, 2, 7, 256, (1 << 32) + 5, (1 << 64) - 1):
            out = ctypes.create_string_buffer(32)
            hc.hc_fr_poly_eval(blob, deg, x, out)
            want = sum(c * pow(x, j, R) for j, c in enumerate(coeffs)) % R
            assert int.from_bytes(out.raw, "big") == want, (deg, x)


def test_bivar_poly_row(hc):
    rnd = random.Random(0x6B67_02)
    for t in (0, 1, 2, 5):
        coeffs = [_rand_fr(rnd) for _ in range(bivar.n_coeffs(t))]
        coeffs[0] = 0
        coeffs[-1] = R - 1
        poly = bivar.BivarPoly(t, coeffs)
        blob = b"".join(_be(c) for c in coeffs)
        for x in (0, 1, 3, 17, (1 << 64) - 1):
            out = ctypes.create_string_buffer(32 * (t + 1))
            hc.hc_bivar_poly_row(blob, t, x, out)
            got = [int.from_bytes(out.raw[32 * j:32 * j + 32], "big") for j in range(t + 1)]
            want = [sum(poly.a(i, j) * pow(x, i, R) for i in range(t + 1)) % R for j in range(t + 1)]
            assert got == want, (t, x)
            # the row is the polynomial y -> f(x, y): its value at y is the bivariate evaluation
            y = 5
            assert sum(c * pow(y, j, R) for j, c in enumerate(got)) % R == poly.evaluate(x, y)


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


def _call_lagrange(hc, ys, vs):
    arr = (U64 * max(len(ys), 1))(*ys)
    out = ctypes.create_string_buffer(32)
    dup = hc.hc_lagrange0_sum(arr, b"".join(_be(v) for v in vs) or b"\0", len(ys), out)
    return dup, int.from_bytes(out.raw, "big")


@pytest.mark.parametrize("t", [1, 2, 5, 85])
def test_lagrange0_sum(hc, t):
    rnd = random.Random(0x6B67_03 + t)
    secret_poly = [_rand_fr(rnd) for _ in range(t + 1)]

    def f(x):
        return sum(c * pow(x, j, R) for j, c in enumerate(secret_poly)) % R

    for cnt in sorted({0, 1, t, t + 1}):
        ys = rnd.sample(range(1, 3 * t + 5), cnt)
        vs = [f(y) for y in ys]
        dup, got = _call_lagrange(hc, ys, vs)
        assert dup == 0
        assert got == _lagrange0(ys, vs), (t, cnt)
        if cnt == t + 1:
            assert got == secret_poly[0]  # t + 1 points of a degree-t polynomial recover f(0)
    assert _call_lagrange(hc, [], []) == (0, 0)
    # y up to 2^64 - 1, the values r - 1 and 0
    cnt = min(t + 1, 6)
    ys = [(1 << 64) - 1, (1 << 64) - 2, 1, 1 << 63, (1 << 32), 3][:cnt]
    vs = ([R - 1, 0] + [_rand_fr(rnd) for _ in range(cnt)])[:cnt]
    dup, got = _call_lagrange(hc, ys, vs)
    assert dup == 0 and got == _lagrange0(ys, vs)
    # a repeated y is reported, not interpolated (threshold_crypto: DuplicateEntry)
    ys = [4, 9, 4][:max(cnt, 2)] if cnt >= 3 else [4, 4]
    dup, got = _call_lagrange(hc, ys, [1] * len(ys))
    assert dup == 1 and got == 0


def test_commit_eval_is_public_key_share(hc):
    rnd = random.Random(0x6B67_04)
    for t in (0, 1, 3):
        coeffs = [_rand_fr(rnd) for _ in range(t + 1)]
        if t == 3:
            coeffs[2] = 0  # an identity point inside the commitment
        pks = tc.PublicKeySet([bls.g1_mul(bls.G1_GEN, c) for c in coeffs])
        blob = b"".join(bls.g1_compress(c) for c in pks.commit)
        for i in (0, 1, 6):
            out = ctypes.create_string_buffer(48)
            assert hc.hc_commit_eval(blob, t, i + 1, out) == 0
            assert out.raw == bls.g1_compress(pks.public_key_share(i)), (t, i)


@pytest.mark.parametrize("variant,code", [("sha256", 0), ("sha3_256", 1)])
def test_sk_decrypt_inverts_encrypt(hc, variant, code):
    rnd = random.Random(0x6B67_05 + code)
    sk = _rand_fr(rnd)
    pk = bls.g1_mul(bls.G1_GEN, sk)
    for n in (0, 1, 32, 96):
        msg = bytes(rnd.randrange(256) for _ in range(n))
        u, v, _w = tc.encrypt(pk, msg, _rand_fr(rnd), variant)
        out = ctypes.create_string_buffer(max(n, 1))
        assert hc.hc_sk_decrypt(_be(sk), bls.g1_compress(u), v or b"\0", n, code, out) == 0
        assert out.raw[:n] == msg
