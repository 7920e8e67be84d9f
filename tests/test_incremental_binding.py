"""Argument guards of the incremental-verification bindings (hbbft_amd/hbx.py): a mismatch between
the shapes of shares, proposer and sender is a ValueError before the library is reached."""
import numpy as np
import pytest


class _NoLib:
    """Stands in for a Context's library: any call is a test failure (the guards must fire first)."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library with mismatched arguments")


def _bare_context():
    from hbbft_amd import hbx

    ctx = object.__new__(hbx.Context)  # no device: only the argument checks run
    ctx.lib, ctx.h = _NoLib(), None
    ctx._v_off = np.array([0, 4, 9, 9], dtype=np.uint64)
    return ctx


def test_exports_name_the_new_calls():
    from hbbft_amd import hbx

    for name in ("hbx_add_dec_shares_d", "hbx_add_dec_shares", "hbx_combine_decrypt_cols_d", "hbx_combine_decrypt_cols",
                 "hbx_get_verify_tiles_used"):
        assert name in hbx.EXPORTS


@pytest.mark.parametrize("shares,proposer,sender", [
    (np.zeros((3, 48), np.uint8), [0, 1], [0, 1, 2]),
    (np.zeros((3, 48), np.uint8), [0, 1, 2], [0, 1]),
    (np.zeros((3, 47), np.uint8), [0, 1, 2], [0, 1, 2]),
    (np.zeros((2, 3, 48), np.uint8), [0, 1], [0, 1]),
    (np.zeros((2, 48), np.uint8), [[0, 1]], [0, 1]),
    (np.zeros((2, 48), np.uint8), [0, -1], [0, 1]),
    (np.zeros((2, 48), np.uint8), [0.5, 1.0], [0, 1]),
    (np.zeros((0, 48), np.uint8), [0], []),
])
def test_add_dec_shares_rejects_mismatched_shapes(shares, proposer, sender):
    ctx = _bare_context()
    with pytest.raises(ValueError, match="add_dec_shares"):
        ctx.add_dec_shares(shares, proposer, sender, 4)


def test_add_dec_shares_rejects_n_zero():
    with pytest.raises(ValueError, match="number of nodes"):
        _bare_context().add_dec_shares(np.zeros((1, 48), np.uint8), [0], [0], 0)


def test_add_dec_shares_d_rejects_strided_and_wide_tensors_before_the_library():
    """The library reads d_shares48 by raw pointer, one byte per element, rows 48 bytes apart."""
    import torch

    ctx = _bare_context()
    strided = torch.zeros((2, 96), dtype=torch.uint8)[:, ::2]
    transposed = torch.zeros((48, 2), dtype=torch.uint8).t()
    wide = torch.zeros((2, 48), dtype=torch.int32)
    for bad in (strided, transposed, wide):
        assert tuple(bad.shape) == (2, 48)
        with pytest.raises(ValueError, match="add_dec_shares_d: d_shares48 must be contiguous uint8"):
            ctx.add_dec_shares_d(bad, [0, 1], [0, 1], 4)
    with pytest.raises(ValueError, match="add_dec_shares_d: d_status must have one byte per share"):
        ctx.add_dec_shares_d(torch.zeros((2, 48), dtype=torch.uint8), [0, 1], [0, 1], 4,
                             d_status=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match="add_dec_shares_d"):
        ctx.add_dec_shares_d(None, [0], [], 4)


@pytest.mark.parametrize("cols", [[0, 0], [3], [-1], [[0, 1]], [0.5]])
def test_combine_decrypt_cols_rejects_bad_columns(cols):
    with pytest.raises(ValueError, match="combine_decrypt_cols"):
        _bare_context().combine_decrypt_cols(2, cols)


def test_combine_decrypt_cols_rejects_wrong_buffers():
    ctx = _bare_context()
    with pytest.raises(ValueError, match="status int32"):
        ctx.combine_decrypt_cols(2, [1], out=np.zeros(9, np.uint8), status=np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="out must be"):
        ctx.combine_decrypt_cols(2, [1], out=np.zeros(4, np.uint8), status=np.zeros(3, np.int32))
    assert ctx.combine_decrypt_cols(2, []) == ({}, {})  # no column: the library is not reached
