"""The Python surface of the pair-lane Ciphertext::verify mode of hbx_sk_decrypt (hbx_set_ct_check /
hbx_get_ct_check_used): exported names, argument guards, and KeyGenReplay's ct_check switch.  No GPU
and no library call: the contexts here are stand-ins."""
import numpy as np
import pytest

from hbbft_amd import hbx
from hbbft_amd.sync_key_gen import PART, KeyGenReplay


def test_exports_and_constants():
    assert "hbx_set_ct_check" in hbx.EXPORTS
    assert "hbx_get_ct_check_used" in hbx.EXPORTS
    assert hbx.CT_CHECK_WIDE == 0 and hbx.CT_CHECK_PAIR == 1
    assert isinstance(hbx.SK_DECRYPT_PAIR_CHUNK, int) and hbx.SK_DECRYPT_PAIR_CHUNK > 0


class _NoLib:
    """Stands in for a Context's library: any call is a test failure (the guards must fire first)."""

    def __getattr__(self, name):
        raise AssertionError(f"{name} reached the library with a bad mode")


@pytest.mark.parametrize("mode", [2, -1, None, "pair", True])
def test_set_ct_check_rejects_other_values_before_the_library(mode):
    ctx = object.__new__(hbx.Context)  # no device: only the argument check runs
    ctx.lib, ctx.h = _NoLib(), None
    with pytest.raises(ValueError, match="set_ct_check"):
        ctx.set_ct_check(mode)


class _Recorder:
    """A context that records the calls KeyGenReplay makes; every ciphertext fails to verify."""

    def __init__(self):
        self.calls = []

    def set_ct_check(self, mode):
        self.calls.append(("set_ct_check", mode))

    def sk_decrypt(self, sk, cts):
        self.calls.append(("sk_decrypt", len(cts)))
        return [b""] * len(cts), np.zeros(len(cts), dtype=np.uint8)


def _one_part(n):
    commit = np.zeros((1, 48), dtype=np.uint8)
    rows = [(bytes(48), b"", bytes(96))] * n
    return [(PART, 1, (commit, rows))]


def _replay(ctx, **kw):
    return KeyGenReplay(ctx, 0, bytes(32), np.zeros((4, 48), dtype=np.uint8), 0, **kw)


def test_replay_sets_the_mode_before_sk_decrypt():
    for mode in (hbx.CT_CHECK_PAIR, hbx.CT_CHECK_WIDE):
        ctx = _Recorder()
        _replay(ctx, ct_check=mode).handle_messages(_one_part(4))
        assert ctx.calls == [("set_ct_check", mode), ("sk_decrypt", 1)]


def test_replay_leaves_the_mode_alone_by_default():
    for kw in ({}, {"ct_check": None}):
        ctx = _Recorder()
        _replay(ctx, **kw).handle_messages(_one_part(4))
        assert ctx.calls == [("sk_decrypt", 1)]


def test_replay_rejects_an_unknown_mode():
    with pytest.raises(ValueError, match="ct_check"):
        _replay(_Recorder(), ct_check=2)
