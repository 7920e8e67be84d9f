"""The binding of the echo-store calls (hbbft_amd/hbx.py): their argument checks raise ValueError
before the library is reached (a bare context whose library refuses every call), and EXPORTS holds the
new symbols.  No GPU."""
import numpy as np
import pytest

from hbbft_amd import hbx


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library with mismatched arguments")


def _bare(prepared=True):
    ctx = object.__new__(hbx.Context)
    ctx.lib, ctx.h = _NoLib(), None
    if prepared:
        ctx._bc = (3, 7, 5, 100)  # inst, n, k, row pitch: what prepare_broadcast records
    return ctx


def _proof_arrays(count):
    return (np.zeros((count, 17, 32), dtype=np.uint8), np.zeros((count, 16, 32), dtype=np.uint8),
            np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32), np.zeros((count, 32), dtype=np.uint8))


def test_exports_hold_the_new_names():
    for name in ("hbx_prepare_broadcast", "hbx_add_echoes_d", "hbx_add_echoes", "hbx_broadcast_decode_insts_d",
                 "hbx_broadcast_decode_insts", "hbx_get_echo_slots", "hbx_debug_get_echo_rows"):
        assert name in hbx.EXPORTS
    assert (hbx.ECHO_INVALID, hbx.ECHO_STORED, hbx.ECHO_DUPLICATE, hbx.ECHO_OVERSIZE) == (0, 1, 2, 3)
    assert hbx.HBX_E_NO_BROADCAST == -12 and hbx.HBX_E_SHARD_SIZE == -13


@pytest.mark.parametrize("args", [(0, 3, 2, 10), (4, 0, 2, 10), (4, 3, -1, 10), (4, 3, 2, 0), (4, 129, 2, 10), (4, 100, 157, 10),
                                  (4, 3, 2, 1 << 32), (4.0, 3, 2, 10)])
def test_prepare_broadcast_rejects(args):
    with pytest.raises(ValueError, match="prepare_broadcast"):
        _bare(False).prepare_broadcast(*args)


def test_add_echoes_shapes_and_dtypes():
    ctx = _bare()
    vals = np.zeros(10, dtype=np.uint8)
    off = np.array([0, 5, 10], dtype=np.uint64)
    good = _proof_arrays(2)
    with pytest.raises(ValueError, match="values"):
        ctx.add_echoes(vals.astype(np.int32), off, *good, [0, 1], [0, 1])
    with pytest.raises(ValueError, match="values"):
        ctx.add_echoes(vals.reshape(2, 5), off, *good, [0, 1], [0, 1])
    with pytest.raises(ValueError, match="val_off"):
        ctx.add_echoes(vals, [0, 6, 5], *good, [0, 1], [0, 1])
    with pytest.raises(ValueError, match="val_off"):
        ctx.add_echoes(vals, [0, 5, 11], *good, [0, 1], [0, 1])
    with pytest.raises(ValueError, match="val_off"):
        ctx.add_echoes(vals, [], *good, [], [])
    with pytest.raises(ValueError, match="one entry per"):
        ctx.add_echoes(vals, off, *good, [0, 1, 2], [0, 1])
    with pytest.raises(ValueError, match="indices"):
        ctx.add_echoes(vals, off, *good, [0, -1], [0, 1])
    with pytest.raises(ValueError, match="indices"):
        ctx.add_echoes(vals, off, *good, [0.0, 1.0], [0, 1])
    with pytest.raises(ValueError, match="twice"):
        ctx.add_echoes(vals, off, *good, [1, 1], [4, 4])
    for slot, bad in ((0, np.zeros((2, 16, 32), dtype=np.uint8)), (1, np.zeros((2, 17, 32), dtype=np.uint8)),
                      (2, np.zeros(2, dtype=np.int64)), (3, np.zeros(3, dtype=np.uint32)),
                      (4, np.zeros((2, 31), dtype=np.uint8)), (0, np.zeros((2, 17, 32), dtype=np.int8))):
        arrs = list(good)
        arrs[slot] = bad
        with pytest.raises(ValueError, match="must be"):
            ctx.add_echoes(vals, off, *arrs, [0, 1], [0, 1])


def test_add_echoes_d_shapes():
    torch = pytest.importorskip("torch")
    ctx = _bare()
    vals = torch.zeros(10, dtype=torch.uint8)
    off = [0, 5, 10]
    good = [torch.from_numpy(a) for a in _proof_arrays(2)]
    good[2], good[3] = good[2].view(torch.int32), good[3].view(torch.int32)
    with pytest.raises(ValueError, match="byte tensor"):
        ctx.add_echoes_d(vals.reshape(2, 5), off, *good, [0, 1], [0, 1])
    with pytest.raises(ValueError, match="twice"):
        ctx.add_echoes_d(vals, off, *good, [2, 2], [1, 1])
    with pytest.raises(ValueError, match="d_status"):
        ctx.add_echoes_d(vals, off, *good, [0, 1], [0, 1], d_status=torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="d_sides"):
        ctx.add_echoes_d(vals, off, good[0], good[1], torch.zeros(2, dtype=torch.uint8), good[3], good[4], [0, 1], [0, 1])
    with pytest.raises(ValueError, match="d_nodes"):
        ctx.add_echoes_d(vals, off, good[0][:1], *good[1:], [0, 1], [0, 1])


def test_decode_insts_rejects():
    ctx = _bare()
    roots = np.zeros((2, 32), dtype=np.uint8)
    roots[1, 0] = 1
    with pytest.raises(ValueError, match="roots"):
        ctx.broadcast_decode_insts([0, 1], roots[:1], [5, 5])
    with pytest.raises(ValueError, match="roots"):
        ctx.broadcast_decode_insts([0, 1], roots.astype(np.int16), [5, 5])
    with pytest.raises(ValueError, match="len"):
        ctx.broadcast_decode_insts([0, 1], roots, [5, 0])
    with pytest.raises(ValueError, match="len"):
        ctx.broadcast_decode_insts([0, 1], roots, [5])
    with pytest.raises(ValueError, match="insts"):
        ctx.broadcast_decode_insts([[0, 1]], roots, [5, 5])
    with pytest.raises(ValueError, match="use"):
        ctx.broadcast_decode_insts([0, 1], roots, [5, 5], use=np.ones((2, 6), dtype=np.uint8))
    with pytest.raises(ValueError, match="use"):
        ctx.broadcast_decode_insts([0, 1], roots, [5, 5], use=np.ones((3, 7), dtype=np.uint8))
    with pytest.raises(ValueError, match="use"):
        ctx.broadcast_decode_insts([0, 1], roots, [5, 5], use=np.ones((2, 7), dtype=np.float32))
    same = np.zeros((2, 32), dtype=np.uint8)
    with pytest.raises(ValueError, match="listed twice"):
        ctx.broadcast_decode_insts([1, 1], same, [5, 5])
    with pytest.raises(ValueError, match="listed twice"):
        ctx.broadcast_decode_insts([1, 1], same, [5, 5], use=np.ones((2, 7), dtype=np.uint8))
    # the same instance and root over other senders is another attempt: it passes the checks (and
    # would reach the library)
    use = np.ones((2, 7), dtype=np.uint8)
    use[1, 0] = 0
    with pytest.raises(AssertionError, match="reached the library"):
        ctx.broadcast_decode_insts([1, 1], same, [5, 5], use=use)
    assert ctx.broadcast_decode_insts([], np.zeros((0, 32), dtype=np.uint8), [])[0] == []


def test_calls_need_a_prepared_store():
    ctx = _bare(prepared=False)
    with pytest.raises(ValueError, match="prepare_broadcast"):
        ctx.echo_slots()
    with pytest.raises(ValueError, match="prepare_broadcast"):
        ctx.broadcast_decode_insts([0], np.zeros((1, 32), dtype=np.uint8), [5])
