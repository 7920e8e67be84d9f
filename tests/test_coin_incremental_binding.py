"""Argument guards of the coin's incremental bindings (hbbft_amd/hbx.py add_sig_shares[_d],
combine_signatures_insts[_d]): a mismatch is a ValueError before the library is reached; and the
header and hbx.EXPORTS name the five new entry points (what tests/test_abi.py compares)."""
import os
import re

import numpy as np
import pytest

NEW = ("hbx_add_sig_shares_d", "hbx_add_sig_shares", "hbx_combine_signatures_insts_d", "hbx_combine_signatures_insts",
       "hbx_get_coin_tiles_used")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _NoLib:
    """Stands in for a Context's library: any call is a test failure (the guards must fire first)."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library with mismatched arguments")


def _bare_context(count=4):
    from hbbft_amd import hbx

    ctx = object.__new__(hbx.Context)  # no device: only the argument checks run
    ctx.lib, ctx.h = _NoLib(), None
    ctx._coin_count = count
    return ctx


def test_exports_and_header_name_the_new_calls():
    from hbbft_amd import hbx

    header = open(os.path.join(ROOT, "include", "hbx.h")).read()
    for name in NEW:
        assert name in hbx.EXPORTS
        assert re.search(r"\b%s\(" % name, header), name
    assert len(set(hbx.EXPORTS)) == len(hbx.EXPORTS)


@pytest.mark.parametrize("sigs,inst,sender", [
    (np.zeros((3, 96), np.uint8), [0, 1], [0, 1, 2]),
    (np.zeros((3, 96), np.uint8), [0, 1, 2], [0, 1]),
    (np.zeros((3, 95), np.uint8), [0, 1, 2], [0, 1, 2]),
    (np.zeros((2, 3, 96), np.uint8), [0, 1], [0, 1]),
    (np.zeros((2, 96), np.uint8), [[0, 1]], [0, 1]),
    (np.zeros((2, 96), np.uint8), [0, -1], [0, 1]),
    (np.zeros((2, 96), np.uint8), [0, 1], [0, -1]),
    (np.zeros((2, 96), np.uint8), [0.5, 1.0], [0, 1]),
    (np.zeros((2, 96), np.int32), [0, 1], [0, 1]),
    (np.zeros((0, 96), np.uint8), [0], []),
])
def test_add_sig_shares_rejects_mismatched_shapes(sigs, inst, sender):
    with pytest.raises(ValueError, match="add_sig_shares"):
        _bare_context().add_sig_shares(sigs, inst, sender, 4)


@pytest.mark.parametrize("n", [0, -1])
def test_add_sig_shares_rejects_n_zero(n):
    with pytest.raises(ValueError, match="number of nodes"):
        _bare_context().add_sig_shares(np.zeros((1, 96), np.uint8), [0], [0], n)


@pytest.mark.parametrize("insts", [[0, 0], [1, 2, 1], [4], [-1], [[0, 1]], [0.5]])
def test_combine_signatures_insts_rejects_bad_instances(insts):
    with pytest.raises(ValueError, match="combine_signatures_insts"):
        _bare_context().combine_signatures_insts(bytes(48), 2, insts)


def test_combine_signatures_insts_rejects_wrong_buffers():
    ctx = _bare_context()
    mpk = bytes(48)
    with pytest.raises(ValueError, match="use must be uint8"):
        ctx.combine_signatures_insts(mpk, 2, [1], use=np.zeros((4, 7), np.int32))
    with pytest.raises(ValueError, match="use must be uint8"):
        ctx.combine_signatures_insts(mpk, 2, [1], use=np.zeros((3, 7), np.uint8))
    with pytest.raises(ValueError, match="sig must be"):
        ctx.combine_signatures_insts(mpk, 2, [1], sig=np.zeros((4, 95), np.uint8))
    with pytest.raises(ValueError, match="status must be"):
        ctx.combine_signatures_insts(mpk, 2, [1], status=np.zeros(4, np.int64))
    with pytest.raises(ValueError, match="ok must be"):
        ctx.combine_signatures_insts(mpk, 2, [1], ok=np.zeros(4, bool))
    with pytest.raises(ValueError, match="parity must be"):
        ctx.combine_signatures_insts(mpk, 2, [1], parity=np.zeros(3, np.uint8))
    # no instance: the library is not reached, nothing is written
    sig = np.full((4, 96), 0xA5, np.uint8)
    out = ctx.combine_signatures_insts(mpk, 2, [], sig=sig)
    assert out[0] is sig and (sig == 0xA5).all()


def test_device_forms_reject_bad_indices_before_the_library():
    ctx = _bare_context()
    with pytest.raises(ValueError, match="add_sig_shares_d"):
        ctx.add_sig_shares_d(None, [0], [], 4)
    with pytest.raises(ValueError, match="number of nodes"):
        ctx.add_sig_shares_d(None, [], [], 0)
    with pytest.raises(ValueError, match="listed twice"):
        ctx.combine_signatures_insts_d(bytes(48), 2, [3, 3])
    with pytest.raises(ValueError, match="combine_signatures_insts_d"):
        ctx.combine_signatures_insts_d(bytes(48), 2, [-2])
