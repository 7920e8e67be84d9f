"""The one-lane Miller kernel's line form 1 + beta v + alpha v w (lines divided by their constant
term): the product fq12d_mul_by_1ab (fieldd.hpp), the second normalised table
(pairing.hpp g2_normalise_line_z2, the routine k_normalise_lines runs per line) and the loop
miller_loop2_unit_d (pairingd.hpp), compiled for the host with -DHBX_DCHECK
(tools/hostcheck/linecheck.cpp) and compared with field.hpp's generic tower and with the loop over
the first table's lines (miller_loop2_parked_d, the loop k_verify_shares runs).  HBX_DCHECK aborts the process on a product operand digit out of bounds."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = bls.P
RD = 1 << 392  # the digit form's Montgomery radix
D28 = 1 << 28
P13 = P >> 364  # the top digit of p


@pytest.fixture(scope="module")
def lc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("linecheck") / "liblinecheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHBX_DCHECK", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "linecheck.cpp")])
    return ctypes.CDLL(out)


def norm_digits(v):
    """The normalised digits of the integer v: 0..12 in [0, 2^28), digit 13 signed."""
    return [(v >> (28 * i)) & (D28 - 1) for i in range(13)] + [v >> 364]


def elem(x, shift=0):
    """x in [0, p) as a normalised digit-Montgomery operand shifted by shift * p."""
    return norm_digits(x * RD % P + shift * P)


def const(lo, top):
    return [lo] * 13 + [top]


def neg(d):
    return [-x for x in d]


def i32(ds):
    flat = [x for d in ds for x in d]
    assert all(-(1 << 31) <= x < (1 << 31) for x in flat)
    return (ctypes.c_int32 * len(flat))(*flat)


def _be(x):
    return x.to_bytes(48, "big")


def test_mul_by_1ab_matches_generic_product(lc):
    """fq12d_mul_by_1ab(f, alpha, beta) is the generic Fq12 product of f by 1 + beta v + alpha v w:
    one product and a chain of 24 dependent ones (each output the next input as it comes out), on
    random operands and at the stated bounds -- f reduced (value within (-1.3 p, 2.3 p)) with every
    low digit at its maximum, conjugated f (c1 negated) with digits at +-2^28, and alpha, beta, f.c0,
    f.c1 all maximal at once, so the operand sums f.c0 + f.c1 and alpha + beta are sums of two
    normalised values at their bound."""
    rnd = random.Random(9001)
    top, bot = const(D28 - 1, (23 * P13) // 10 - 1), const(0, -(13 * P13) // 10)
    edge = const(D28 - 1, 2 * P13 - 1)  # a product output at its bound: normalised, value just below 2p
    low = const(0, -P13)  # and at the other end: value just above -p
    at28 = const(D28, P13)
    rand_f = lambda: [elem(rnd.randrange(P), rnd.choice((-1, 0, 1))) for _ in range(12)]  # noqa: E731
    rand_s = lambda: [elem(rnd.randrange(P), rnd.choice((-1, 0, 1))) for _ in range(2)]  # noqa: E731
    fs = [rand_f() for _ in range(4)]
    fs += [[top] * 12, [bot] * 12, [top, bot] * 6, [top] * 6 + [neg(top)] * 6, [bot] * 6 + [neg(bot)] * 6,
           [at28] * 6 + [neg(at28)] * 6, [neg(at28)] * 6 + [at28] * 6]
    g = rand_f()
    fs.append(g[:6] + [neg(d) for d in g[6:]])  # a conjugated random value
    scalars = [(rand_s(), rand_s()) for _ in range(3)]
    scalars += [([edge, edge], [edge, edge]), ([edge, low], [low, edge]), ([low, low], [edge, edge]),
                ([[0] * 14, [0] * 14], rand_s()), (rand_s(), [[0] * 14, [0] * 14])]
    for f in fs:
        for alpha, beta in scalars:
            for n in (1, 24):
                got, want = ctypes.create_string_buffer(576), ctypes.create_string_buffer(576)
                lc.lc_mul_by_1ab(i32(f), i32(alpha), i32(beta), n, got, want)
                assert got.raw == want.raw, (n, f[0], alpha[0], beta[0])


def _points(rnd, a, valid):
    """(PA, QA, PB, QB) with e(PA, QA) e(PB, QB) == 1 iff valid: PA = a G1, QA = s G2, PB = -s' G1,
    QB = a G2 with s' = s (valid) or s + 1."""
    s = rnd.randrange(1, bls.R - 1)
    pa = bls.g1_compress(bls.g1_mul(bls.G1_GEN, a))
    qa = bls.g2_compress(bls.g2_mul(bls.G2_GEN, s))
    pb = bls.g1_compress(bls.g1_neg(bls.g1_mul(bls.G1_GEN, s if valid else s + 1)))
    qb = bls.g2_compress(bls.g2_mul(bls.G2_GEN, a))
    return pa, qa, pb, qb


@pytest.mark.parametrize("jac", [0, 1], ids=["affine", "jacobian"])
def test_unit_loop_same_verdict_as_scaled_loop(lc, jac):
    """For random G2 and G1 points the loop over lines divided by their constant term and the loop over
    the first table's lines (miller_loop2_parked_d) give the same element after the final exponentiation -- 1 for valid pairs,
    the same element other than 1 for invalid ones; the first-form table out of the combined
    normalisation equals the affine point's, and each second-form (a, b) times the raw c0 gives back
    the raw line.  `jacobian`: QA's raw lines come from a Jacobian representative with Z != 1, as
    the hash point's do."""
    rnd = random.Random(9002 + jac)
    for trial in range(4):
        valid = trial % 2 == 0
        pa, qa, pb, qb = _points(rnd, rnd.randrange(1, bls.R), valid)
        z = _be(rnd.randrange(2, P)) + _be(rnd.randrange(1, P))
        res = lc.lc_unit_loop_cmp(pa, qa, pb, qb, jac, z)
        assert res == (1 | 4 | 8 | 16) + (2 if valid else 0), (trial, res)


def test_zero_constant_term_sets_flag_and_keeps_first_form(lc):
    """A raw line whose constant term is zero, handed to the normalise routine directly: it reports
    the line degenerate (k_normalise_lines sets the proposer's flag from that), the first-form line
    is exactly what g2_normalise_line_z makes of the same input, and the second form is (0, 0).  A
    line with any other constant term -- 1, or zero in one coordinate only -- is not reported."""
    rnd = random.Random(9003)
    f2 = lambda: _be(rnd.randrange(1, P)) + _be(rnd.randrange(1, P))  # noqa: E731
    one = _be(1) + _be(0)
    for z in (one, f2()):
        assert lc.lc_normalise_flags(bytes(96), f2(), f2(), z) == 1 | 2 | 4
        assert lc.lc_normalise_flags(bytes(96), bytes(96), f2(), z) == 1 | 2 | 4
        assert lc.lc_normalise_flags(one, f2(), f2(), z) == 2
        assert lc.lc_normalise_flags(_be(0) + _be(5), f2(), f2(), z) == 2
        assert lc.lc_normalise_flags(_be(7) + _be(0), f2(), f2(), z) == 2
        assert lc.lc_normalise_flags(f2(), f2(), f2(), z) == 2
