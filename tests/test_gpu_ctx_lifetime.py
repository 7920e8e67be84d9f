"""What a context allocates it frees: hbx_debug_live_buffers (device and pinned allocations the
library holds in this process) returns to where it was when a context is destroyed, whatever the
context did, and when a call fails after allocating its temporaries."""
import numpy as np
import pytest

from test_gpu_incremental import _add, _cts, _load, _set_keys

pytestmark = pytest.mark.gpu


def _exercise(ctx):
    """Every kind of allocation a context owns: era and epoch state, the add's buffers (the add
    establishes the matrix), the column combine (pinned staging and its event), the host-pointer
    broadcast staging, a ragged call's descriptors, a call's temporaries."""
    import torch

    from hbbft_amd.hbx import ragged_layout

    d = _load("hb_epoch_n4")
    p, n = d["shares"].shape[:2]
    _set_keys(ctx, d)
    ctx.prepare_ciphertexts(_cts(d))
    positions = [(int(j), int(i)) for j, i in np.argwhere(d["present"])]
    st = _add(ctx, d, positions, n)
    assert st.tolist() == [int(d["expect_share_status"][j, i]) for j, i in positions]
    plains, status = ctx.combine_decrypt_cols(int(d["t"]), [0])
    assert status[0] == int(d["expect_status"][0])
    shards = np.arange(1 * 4 * 8, dtype=np.uint8).reshape(1, 4, 8)
    ctx.rs_encode(shards, 2, 2)
    off, pitch, total = ragged_layout([4, 8], 4)
    d_buf = torch.arange(total, dtype=torch.int32, device="cuda:0").to(torch.uint8)
    d_roots = torch.zeros((2, 32), dtype=torch.uint8, device="cuda:0")
    ctx.merkle_build_ragged_d(d_buf, off, [4, 8], pitch, 4, d_roots=d_roots)
    torch.cuda.synchronize()
    r = np.zeros((1, 32), dtype=np.uint8)
    r[0, 31] = 5
    (u, v, w), = ctx.encrypt_to(d["pk_comp"][:1], [b"lifetime"], r)
    assert len(u) == 48 and len(v) == 8 and len(w) == 96


def test_destroy_frees_every_buffer():
    from hbbft_amd import hbx

    live0 = hbx.live_buffers()
    ctx = hbx.Context(0)
    _exercise(ctx)
    assert hbx.live_buffers() > live0
    ctx.close()
    assert hbx.live_buffers() == live0


def test_create_destroy_twice():
    from hbbft_amd import hbx

    live0 = hbx.live_buffers()
    for _ in range(2):
        ctx = hbx.Context(0)
        _exercise(ctx)
        assert hbx.live_buffers() > live0
        ctx.close()
        assert hbx.live_buffers() == live0
        ctx.close()  # a second close is harmless
        assert hbx.live_buffers() == live0


def test_failed_call_leaves_no_temporaries(hbx_ctx):
    from hbbft_amd import hbx

    r = np.zeros((1, 32), dtype=np.uint8)
    r[0, 31] = 5
    bad_pk = np.full((1, 48), 0xFF, dtype=np.uint8)  # no G1 encoding: compressed, infinity and x != 0
    before = hbx.live_buffers()
    with pytest.raises(hbx.HbxError) as e:
        hbx_ctx.encrypt_to(bad_pk, [b"lifetime"], r)
    assert e.value.code == hbx.HBX_E_INVALID_ARG and "does not decode" in str(e.value)
    assert hbx.live_buffers() == before
