"""The pair-lane Ciphertext::verify's arithmetic (k_verify_ct2: H' made affine, both pairs' lines
generated on the fly by miller_loop_gen_d, one final exponentiation) on one CPU thread through
tools/hostcheck, against the committed skg_batch65 fixture.  The -m gpu tests (test_gpu_ct_pair.py)
then pin the kernel that runs it on lane pairs."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

# hc_ct_check_gen's answer -> HBX_CT_* (include/hbx.h)
TO_STATUS = {1: 1, 0: 0, -1: 3}


@pytest.fixture(scope="module")
def hc(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hostcheck_ct_pair") / "libhostcheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-DHBX_DCHECK", "-shared", "-fPIC", "-o", out,
                           os.path.join(ROOT, "tools", "hostcheck", "hostcheck.cpp")])
    lib = ctypes.CDLL(out)
    lib.hc_ct_check_gen.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_int]
    return lib


@pytest.fixture(scope="module")
def batch():
    return dict(np.load(os.path.join(GOLDEN, "skg_batch65.npz"), allow_pickle=False))


def _ct(d, j):
    off = d["off"]
    return d["u"][j].tobytes(), d["v_blob"][int(off[j]):int(off[j + 1])].tobytes(), d["w"][j].tobytes()


def _check(hc, u, v, w, digest=0):
    return hc.hc_ct_check_gen(u, v, len(v), w, digest)


@pytest.mark.parametrize("j,want", [(7, 0), (21, -1), (0, 1), (64, 1)])
def test_fixture_ciphertexts(hc, batch, j, want):
    """index 7: tampered V; 21: W off the subgroup; 0 and 64: honest."""
    got = _check(hc, *_ct(batch, j))
    assert got == want
    assert TO_STATUS[got] == int(batch["expect_status"][j])


def test_w_of_another_ciphertext(hc, batch):
    u, v, _ = _ct(batch, 0)
    assert _check(hc, u, v, _ct(batch, 1)[2]) == 0
