"""The pair-lane PublicKey::verify's arithmetic (k_verify_sigs2: H' = [m] hash_g2(msg) affine, both
pairs' lines generated on the fly by miller_loop_gen_d, sigma's G2 membership from its loop's
T = [|x|] sigma, one final exponentiation) on one CPU thread through tools/hostcheck, against the
oracle's verify_sig and [r] sigma = O on items of the committed kgsigs_b65 fixture.  The -m gpu tests
(test_gpu_sigs_keyed.py) then pin the kernel that runs it on lane pairs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import threshold as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# hc_sig_check_gen's answer -> HBX_SHARE_* (include/hbx.h)
TO_STATUS = {1: 1, 0: 0, -1: 3}


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck_sig_pair") / "libhostcheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHBX_DCHECK", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "hostcheck.cpp")])
    lib = ctypes.CDLL(out)
    lib.hc_sig_check_gen.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def b65():
    return dict(np.load(os.path.join(GOLDEN, "kgsigs_b65.npz"), allow_pickle=False))


def _item(d, i):
    off = d["msg_off"]
    return (d["pk"][int(d["key_idx"][i])].tobytes(), d["msg_blob"][int(off[i]):int(off[i + 1])].tobytes(),
            d["sig"][i].tobytes())


def _oracle(pk48, msg, sig96, digest="sha256"):
    """1 / 0 from verify_sig, -1 when sigma is on the curve but [r] sigma != O."""
    P = bls.g1_decompress(pk48)
    S = bls.g2_decompress(sig96, subgroup_check=False)
    if S is not None and bls.g2_mul(S, bls.R) is not None:
        return -1
    return 1 if tc.verify_sig(P, S, msg, digest) else 0


@pytest.mark.parametrize("i,what,want", [(0, "valid", 1), (1, "signature over another message", 0),
                                          (3, "sigma plus a cofactor point", -1),
                                          (6, "identity key, identity sigma", 1), (7, "identity key, real sigma", 0),
                                          (9, "valid, 300-byte message", 1)])
def test_fixture_items(hc, b65, i, what, want):
    pk, msg, sig = _item(b65, i)
    got = hc.hc_sig_check_gen(pk, msg, len(msg), sig, 0)
    assert got == want, what
    assert got == _oracle(pk, msg, sig), what
    assert TO_STATUS[got] == int(b65["expect"][i]), what


def test_sha3_item(hc):
    d = dict(np.load(os.path.join(GOLDEN, "kgsigs_b9_sha3.npz"), allow_pickle=False))
    pk, msg, sig = _item(d, 2)  # a signature by another key of the table
    assert hc.hc_sig_check_gen(pk, msg, len(msg), sig, 1) == 0 == _oracle(pk, msg, sig, "sha3_256")
    pk, msg, sig = _item(d, 0)
    assert hc.hc_sig_check_gen(pk, msg, len(msg), sig, 1) == 1 == _oracle(pk, msg, sig, "sha3_256")
    assert hc.hc_sig_check_gen(pk, msg, len(msg), sig, 0) == 0  # the other digest's hash


def test_undecodable_inputs(hc, b65):
    pk, msg, sig = _item(b65, 4)  # cleared compression flag
    assert hc.hc_sig_check_gen(pk, msg, len(msg), sig, 0) == -1
    pk, msg, sig = _item(b65, 5)  # key off the G1 subgroup
    assert hc.hc_sig_check_gen(pk, msg, len(msg), sig, 0) == -1
