"""Ragged Broadcast bindings (hbx.Context.*_ragged_d): the layout helper and the descriptor rules of
include/hbx.h, which the bindings check before the library is reached.  No GPU: a bare context whose
library fails the test on any call, as tests/test_abi.py does for the host forms."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library with bad descriptors")


def _bare_context():
    from hbbft_amd import hbx

    ctx = object.__new__(hbx.Context)
    ctx.lib, ctx.h = _NoLib(), None
    return ctx


@pytest.mark.parametrize("align", [4, 16, 64])
@pytest.mark.parametrize("n", [1, 4, 128])
def test_ragged_layout(n, align):
    from hbbft_amd import hbx

    lens = [1, 2, 3, 4, 5, 63, 64, 65, 257, 2044, 2048, 2052, 4100]
    off, pitch, total = hbx.ragged_layout(lens, n, align)
    assert off.dtype == np.uint64 and pitch.dtype == np.uint32 and len(off) == len(pitch) == len(lens)
    assert not (off % align).any() and not (pitch % align).any()          # alignment
    for L, p in zip(lens, pitch):
        assert L <= p < L + align                                          # the least such pitch
    ends = off.astype(np.int64) + n * pitch.astype(np.int64)
    assert (off[1:].astype(np.int64) >= ends[:-1]).all() and off[0] == 0   # no overlap, in order
    assert total == int(ends[-1]) == int((pitch.astype(np.int64) * n).sum())  # totals: no gaps either
    assert hbx.Context.ragged_layout(lens, n, align)[2] == total


def test_ragged_layout_rejects_bad_input():
    from hbbft_amd import hbx

    for lens, n, align in [([], 4, 16), ([0], 4, 16), ([5], 0, 16), ([5], 4, 6), ([5], 4, 0)]:
        with pytest.raises(ValueError):
            hbx.ragged_layout(lens, n, align)


K, M = 2, 2
N = K + M
GOOD = dict(off=[0, 64], lens=[5, 9], pitch=[16, 16])   # two instances of 4 rows in 128 bytes
BAD = {
    "misaligned off": dict(off=[0, 66], lens=[5, 9], pitch=[16, 16], nbytes=160),
    "misaligned pitch": dict(off=[0, 64], lens=[5, 9], pitch=[16, 14]),
    "pitch < len": dict(off=[0, 64], lens=[5, 17], pitch=[16, 16]),
    "len == 0": dict(off=[0, 64], lens=[5, 0], pitch=[16, 16]),
    "past the buffer": dict(off=[0, 64], lens=[5, 9], pitch=[16, 16], nbytes=127),
    "overlap": dict(off=[0, 60], lens=[5, 9], pitch=[16, 16]),
    "overlap, unsorted": dict(off=[64, 8], lens=[5, 9], pitch=[16, 16]),
    "array sizes differ": dict(off=[0, 64], lens=[5], pitch=[16, 16]),
}


def _calls(ctx, off, lens, pitch, nbytes=128):
    buf = torch.zeros(nbytes, dtype=torch.uint8)
    inst = len(off)
    present = torch.ones((inst, N), dtype=torch.uint8)
    st = torch.zeros(inst, dtype=torch.int32)
    roots = torch.zeros((inst, 32), dtype=torch.uint8)
    out = torch.zeros(256, dtype=torch.uint8)
    out_len = torch.zeros(inst, dtype=torch.int64)
    return {
        "encode": lambda: ctx.rs_encode_ragged_d(buf, off, lens, pitch, K, M),
        "reconstruct": lambda: ctx.rs_reconstruct_ragged_d(buf, off, lens, pitch, present, st, K, M),
        "build": lambda: ctx.merkle_build_ragged_d(buf, off, lens, pitch, N, d_roots=roots),
        "decode": lambda: ctx.broadcast_decode_ragged_d(buf, off, lens, pitch, present, roots, K, M, out,
                                                        [0, 128][:inst], out_len, st),
    }


@pytest.mark.parametrize("case", sorted(BAD))
@pytest.mark.parametrize("call", ["encode", "reconstruct", "build", "decode"])
def test_ragged_bindings_reject_bad_descriptors(case, call):
    with pytest.raises(ValueError):
        _calls(_bare_context(), **BAD[case])[call]()


@pytest.mark.parametrize("call", ["encode", "reconstruct", "build", "decode"])
def test_ragged_bindings_pass_good_descriptors_on(call):
    """The same calls with valid descriptors get past the checks (and so reach the stand-in library)."""
    with pytest.raises(AssertionError, match="reached the library"):
        _calls(_bare_context(), **GOOD)[call]()


def test_decode_ragged_rejects_bad_output_ranges():
    ctx = _bare_context()
    buf = torch.zeros(128, dtype=torch.uint8)
    present = torch.ones((2, N), dtype=torch.uint8)
    st = torch.zeros(2, dtype=torch.int32)
    roots = torch.zeros((2, 32), dtype=torch.uint8)
    out_len = torch.zeros(2, dtype=torch.int64)
    out = torch.zeros(20, dtype=torch.uint8)          # needs 2 * 5 - 4 = 6 and 2 * 9 - 4 = 14 bytes
    for out_off in ([0, 7], [0, 4], [0]):             # past the end, overlapping, wrong size
        with pytest.raises(ValueError):
            ctx.broadcast_decode_ragged_d(buf, GOOD["off"], GOOD["lens"], GOOD["pitch"], present, roots, K, M, out,
                                          out_off, out_len, st)
    with pytest.raises(AssertionError, match="reached the library"):
        ctx.broadcast_decode_ragged_d(buf, GOOD["off"], GOOD["lens"], GOOD["pitch"], present, roots, K, M, out, [0, 6],
                                      out_len, st)


@pytest.mark.parametrize("val_off", [[0, 5, 4, 9], [0, 5, 9], [0, 5, 9, 12, 12], [0, 5, 9, 41]])
def test_validate_ragged_rejects_bad_val_off(val_off):
    """Three proofs over 40 value bytes: val_off must be 4 non-decreasing offsets ending within them."""
    ctx = _bare_context()
    z = lambda *shape, dt=torch.uint8: torch.zeros(shape, dtype=dt)  # noqa: E731
    args = (z(3, 17, 32), z(3, 16, 32), z(3, dt=torch.int32), z(3, dt=torch.int32), z(3, 32), z(3, dt=torch.int32))
    with pytest.raises(ValueError):
        ctx.merkle_validate_ragged_d(z(40), val_off, *args, 4, z(3))
    with pytest.raises(AssertionError, match="reached the library"):
        ctx.merkle_validate_ragged_d(z(40), [0, 5, 5, 40], *args, 4, z(3))  # an empty value is not an error
