"""The digit tower's rewritten products (fieldd.hpp: the difference-form Karatsuba of fq2d_mul, the
pre-doubled columns of fq4d_sqr_lazy, the Fq12 products whose inner Fq6 results skip the carry pass
before a reduction) on operands at the edges of their bounds, compiled for the host with
-DHBX_DCHECK (tools/hostcheck/towercheck.cpp) and compared with field.hpp's 12-limb tower as
canonical values -- and, for Fq2 / Fq4, with plain integer arithmetic."""
import ctypes
import os
import random
import subprocess

import pytest

from oracle import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = bls.P
RD = 1 << 392  # the digit form's Montgomery radix
RD_INV = pow(RD, -1, P)
D28 = 1 << 28
P13 = P >> 364  # the top digit of p


@pytest.fixture(scope="module")
def tw(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("towercheck") / "libtowercheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHBX_DCHECK", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "towercheck.cpp")])
    return ctypes.CDLL(out)


def norm_digits(v):
    """The normalised digits of the integer v: 0..12 in [0, 2^28), digit 13 signed."""
    return [(v >> (28 * i)) & (D28 - 1) for i in range(13)] + [v >> 364]


def val(d):
    return sum(x << (28 * i) for i, x in enumerate(d))


def elem(x, shift=0):
    """x in [0, p) as a normalised digit-Montgomery operand shifted by shift * p."""
    return norm_digits(x * RD % P + shift * P)


def plain(d):
    """The field element a digit vector stands for."""
    return val(d) * RD_INV % P


def i32(ds):
    flat = [x for d in ds for x in d]
    assert all(-(1 << 31) <= x < (1 << 31) for x in flat)
    return (ctypes.c_int32 * len(flat))(*flat)


def be(buf, k):
    return int.from_bytes(buf.raw[48 * k:48 * k + 48], "big")


def const(lo, top):
    return [lo] * 13 + [top]


def fq2_operand_cases(rnd, e, t):
    """Pairs (a0, a1, b0, b1) of digit vectors: digits 0..12 up to e, digit 13 up to t in magnitude."""
    hi, lo = const(e, t), const(-e, -t)
    zero, pm1 = [0] * 14, norm_digits((P - 1) * RD % P)
    cases = [
        (hi, lo, lo, hi),  # a0, b1 at the positive extreme, a1, b0 at the negative one: the widest differences
        (lo, hi, hi, lo),  # the reverse
        (hi, hi, hi, hi), (lo, lo, lo, lo), (hi, hi, lo, lo), (hi, lo, hi, lo),
        (zero, zero, zero, zero), (zero, pm1, pm1, zero), (pm1, pm1, pm1, pm1), (pm1, zero, hi, lo),
    ]
    for _ in range(40):
        cases.append(tuple(elem(rnd.randrange(P), rnd.choice((-1, 0, 1))) for _ in range(4)))
    return cases


def test_fq2d_mul_difference_form(tw):
    """fq2d_mul at its operand bound: |digit| <= 2 (2^28 - 1) (a sum of two normalised values), values
    below 2^386 (digit 13 up to 2^22) -- with a0, b1 at one extreme and a1, b0 at the other the
    difference-form cross term's column leaves int64 and only the true column must fit."""
    rnd = random.Random(2801)
    cases = fq2_operand_cases(rnd, 2 * (D28 - 1), 1 << 22)
    for _ in range(40):  # sums of two normalised values shifted by +-p
        cases.append(tuple([x + y for x, y in zip(elem(rnd.randrange(P), rnd.choice((-1, 1))),
                                                  elem(rnd.randrange(P), rnd.choice((-1, 1))))] for _ in range(4)))
    for a0, a1, b0, b1 in cases:
        got, want = ctypes.create_string_buffer(96), ctypes.create_string_buffer(96)
        tw.tw_fq2d_mul(i32([a0, a1]), i32([b0, b1]), got, want)
        A0, A1, B0, B1 = plain(a0), plain(a1), plain(b0), plain(b1)
        ref = ((A0 * B0 - A1 * B1) % P, (A0 * B1 + A1 * B0) % P)
        assert (be(want, 0), be(want, 1)) == ref
        assert (be(got, 0), be(got, 1)) == ref, (a0, a1, b0, b1)


def test_fq4d_sqr_lazy_predoubled(tw):
    """fq4d_sqr_lazy at its operand bound (normalised: |digit| < 2^28, value in (-p, 2p)), conjugated
    operands included: the doubled digits reach 2^29."""
    rnd = random.Random(2802)
    for a0, a1, b0, b1 in fq2_operand_cases(rnd, D28 - 1, P13):
        got, want = ctypes.create_string_buffer(192), ctypes.create_string_buffer(192)
        tw.tw_fq4d_sqr_lazy(i32([a0, a1, b0, b1]), got, want)
        A0, A1, B0, B1 = plain(a0), plain(a1), plain(b0), plain(b1)
        a2 = (A0 * A0 - A1 * A1, 2 * A0 * A1)
        b2 = (B0 * B0 - B1 * B1, 2 * B0 * B1)
        ref = ((a2[0] + b2[0] - b2[1]) % P, (a2[1] + b2[0] + b2[1]) % P,  # a^2 + xi b^2
               2 * (A0 * B0 - A1 * B1) % P, 2 * (A0 * B1 + A1 * B0) % P)  # 2 a b
        assert tuple(be(want, k) for k in range(4)) == ref
        assert tuple(be(got, k) for k in range(4)) == ref, (a0, a1, b0, b1)


# operation codes of tw_fq12_chain
SQR, SQR_PARKED, LINE, MUL, MUL_SLOT, LINE014, CONJ = range(7)


def fq12_starts(rnd):
    """Fq12 values in the form the Fq12 functions take ("reduced": normalised digits, value within
    (-1.3 p, 2.3 p)): random ones shifted by -p / 0 / +p, and the ends of that range with every low
    digit at its bound."""
    top, bot = const(D28 - 1, (23 * P13) // 10 - 1), const(0, -(13 * P13) // 10)
    zero, pm1 = [0] * 14, norm_digits((P - 1) * RD % P)
    starts = [[top] * 12, [bot] * 12, [top, bot] * 6, [bot, top, top, bot] * 3,
              [zero, pm1, top, zero, bot, pm1] * 2]
    for _ in range(3):
        starts.append([elem(rnd.randrange(P), rnd.choice((-1, 0, 1))) for _ in range(12)])
    return starts


@pytest.mark.parametrize("ops", [
    [SQR_PARKED, LINE, LINE],  # the one-lane Miller loop's body
    [SQR, LINE014, SQR_PARKED, LINE, CONJ, MUL, SQR, MUL_SLOT, LINE, CONJ, LINE, SQR_PARKED],
    [MUL, MUL_SLOT, SQR, CONJ],
], ids=["miller", "mixed", "products"])
def test_fq12_chains_without_canonicalisation(tw, ops):
    """72 dependent Fq12 operations, each output the next one's input as it comes out (no
    canonicalisation in between, so a bound that fails only after growth shows): the same element as
    field.hpp's tower on the same chain.  HBX_DCHECK aborts on an operand digit out of bounds."""
    rnd = random.Random(2803)
    norm = lambda n: [elem(rnd.randrange(P), rnd.choice((-1, 0, 1))) for _ in range(n)]  # noqa: E731
    edge_line = [const(D28 - 1, 2 * P13 - 1)] * 4 + [const(D28 - 1, 2 * P13 - 1)]
    code = (ctypes.c_int * len(ops))(*ops)
    for f in fq12_starts(rnd):
        for line, g in ((norm(5), norm(12)), (edge_line, [const(D28 - 1, 2 * P13 - 1)] * 12)):
            got, want = ctypes.create_string_buffer(576), ctypes.create_string_buffer(576)
            tw.tw_fq12_chain(i32(f), i32(line), i32(g), code, len(ops), 72, got, want)
            assert got.raw == want.raw, (ops, f[0], line[0])
            assert any(got.raw)  # (a product of non-zero elements)
