"""GPU tests of Broadcast message by message (include/hbx.h: hbx_prepare_broadcast, hbx_add_echoes[_d],
hbx_broadcast_decode_insts[_d]; hbbft_amd/broadcast.py: GpuBroadcastAddEngine, BroadcastSession):
the item statuses against hbx_merkle_validate_ragged_d and the oracle, the insert rule, independence
of how an epoch's Echoes are cut into calls, the listed decode against hbx_broadcast_decode_ragged_d
and oracle.broadcast.decode_from_shards, the session under three flush schedules, and the store's
lifecycle.  Shapes are small (n <= 13, values <= 300 bytes) except one n = 40 epoch."""
import random

import numpy as np
import pytest

from bc_session_fixture import (EPOCHS, MAX_SHARD, SCHEDULES, check_against_oracle, epoch_scenario, ob, rm, run_session,
                                sim_value, simulate)
from hbbft_amd import hbx
from hbbft_amd.broadcast import GpuBroadcastAddEngine, flatten_proofs_ragged, proof_shape_ok

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

VARIANTS = ["sha256", "sha3"]
INVALID, STORED, DUPLICATE, OVERSIZE = hbx.ECHO_INVALID, hbx.ECHO_STORED, hbx.ECHO_DUPLICATE, hbx.ECHO_OVERSIZE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _set_merkle(ctx, variant):
    ctx.set_merkle_digest(hbx.MERKLE_SHA3 if variant == "sha3" else hbx.MERKLE_SHA256)


def _prepare(ctx, variant, inst, n, max_shard_len):
    _set_merkle(ctx, variant)
    k, m = rm.coding_counts(n)
    ctx.prepare_broadcast(inst, k, m, max_shard_len)


def _tree(shards, variant):
    leaves = [bytes([i & 0xFF]) + bytes(s) for i, s in enumerate(shards)]
    return leaves, rm.MerkleTree(leaves, variant)


def _proofs(value, n, variant):
    _, leaves, tree = rm.send_shards(value, n, variant)
    return [tree.gen_proof(leaf) for leaf in leaves], tree.root_hash()


def _add(ctx, items):
    """items: (proof, inst, sender) through the host form -> statuses."""
    blob, val_off, *arrs = flatten_proofs_ragged([p for p, _, _ in items], [s for _, _, s in items])
    return ctx.add_echoes(blob, val_off, *arrs[:5], [q for _, q, _ in items], [s for _, _, s in items])


def _table(ctx):
    return [a.copy() for a in ctx.echo_slots(rows=True)]


def _same_table(a, b):
    """State, and length / root / shard bytes of the held slots (an empty slot's are unspecified)."""
    state, lens, root, rows = a
    if not (state == b[0]).all():
        return False
    held = state.reshape(-1) != 0
    if not ((lens.reshape(-1)[held] == b[1].reshape(-1)[held]).all() and (root.reshape(-1, 32)[held] == b[2].reshape(-1, 32)[held]).all()):
        return False
    for s in np.flatnonzero(held):
        ln = int(lens.reshape(-1)[s])
        if not (rows[s, :ln] == b[3][s, :ln]).all():
            return False
    return (rows[-1] == 0xA5).all() and (b[3][-1] == 0xA5).all()  # the canary row


# ---- statuses -----------------------------------------------------------------------------------
VALUE_LENS = [1, 2, 5, 9, 256, 257, 300]  # index byte only; non-dword tails; both sides of the in-lane hashing limit


def status_items(n, variant):
    """Per value length two instances of honest proofs and two of bad ones (corrupted sibling, wrong
    sender, wrong index byte, empty value): (proof, inst, sender)."""
    rng = random.Random(n)
    items = []
    for q, vlen in enumerate(VALUE_LENS):
        for rep in (0, 2):
            leaves, tree = _tree([rng.randbytes(vlen - 1) for _ in range(n)], variant)
            good = [tree.gen_proof(leaf) for leaf in leaves]
            items += [(p, 4 * q + rep, i) for i, p in enumerate(good)]
            lem = list(good[1]["lemma"])
            h, (side, sib) = lem[0]
            lem[0] = (h, (side, bytes([sib[0] ^ 0x80]) + sib[1:]))
            v3 = good[3]["value"]
            bad = 4 * q + rep + 1
            items += [(dict(good[1], lemma=lem), bad, 1), (good[1], bad, 2),
                      (dict(good[3], value=bytes([v3[0] ^ 1]) + v3[1:]), bad, 3), (dict(good[0], value=b""), bad, 0)]
    return items


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n", [4, 7, 13])
def test_statuses_are_the_ragged_validation(hbx_ctx, n, variant):
    _prepare(hbx_ctx, variant, 4 * len(VALUE_LENS), n, 299)
    items = status_items(n, variant)
    random.Random(5).shuffle(items)
    want = [len(p["value"]) > 0 and rm.validate_broadcast_proof(p, s, n, variant) for p, _, s in items]
    assert sum(want) == 2 * n * len(VALUE_LENS)
    got = []
    cuts = [0, 1, 65, 130, len(items)] if len(items) > 130 else [0, 1, 65, len(items)]  # calls of 1, 64, 65, the rest
    for a, b in zip(cuts[:-1], cuts[1:]):
        part = items[a:b]
        blob, val_off, *arrs = flatten_proofs_ragged([p for p, _, _ in part], [s for _, _, s in part])
        d = [dev(blob if blob.size else np.zeros(1, dtype=np.uint8))] + [dev(x) for x in arrs]
        valid = torch.full((len(part),), 9, dtype=torch.uint8, device="cuda")
        hbx_ctx.merkle_validate_ragged_d(d[0], val_off, *d[1:], n, valid)
        st = torch.full((len(part),), 9, dtype=torch.uint8, device="cuda")
        hbx_ctx.add_echoes_d(d[0], val_off, *d[1:6], [q for _, q, _ in part], [s for _, _, s in part], st)
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == STORED).tolist() == valid.cpu().numpy().astype(bool).tolist()
        got += st.cpu().numpy().tolist()
    assert got == [STORED if w else INVALID for w in want]
    state, lens, root = hbx_ctx.echo_slots()
    for (p, q, s), w in zip(items, want):
        if w:
            assert state[q, s] == 1 and lens[q, s] == len(p["value"]) - 1 and root[q, s].tobytes() == p["root_hash"]
    assert int(state.sum()) == sum(want)


# ---- the insert rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", VARIANTS)
def test_insert_rule(hbx_ctx, variant):
    n = 4
    _prepare(hbx_ctx, variant, 2, n, 20)
    pa, root_a = _proofs(b"A" * 30, n, variant)  # k = 2: shards of 17 bytes
    pb, root_b = _proofs(b"B" * 30, n, variant)
    assert _add(hbx_ctx, [(pa[1], 0, 1)]).tolist() == [STORED]
    before = _table(hbx_ctx)
    assert before[0][0, 1] == 1 and before[2][0, 1].tobytes() == root_a
    assert before[3][1, :17].tobytes() == pa[1]["value"][1:]
    # a different valid proof, then garbage, for the held slot: not looked at
    junk = dict(pb[1], root_hash=b"\x00" * 32, value=b"")
    assert _add(hbx_ctx, [(pb[1], 0, 1)]).tolist() == [DUPLICATE]
    assert _add(hbx_ctx, [(junk, 0, 1), (pb[2], 0, 2)]).tolist() == [DUPLICATE, STORED]
    after = _table(hbx_ctx)
    assert after[2][0, 1].tobytes() == root_a and after[3][1, :17].tobytes() == pa[1]["value"][1:]
    assert after[2][0, 2].tobytes() == root_b
    # invalid, then valid: the slot stayed empty and is still looked at
    bad = dict(pa[3], value=pa[3]["value"][:-1] + bytes([pa[3]["value"][-1] ^ 1]))
    assert _add(hbx_ctx, [(bad, 0, 3)]).tolist() == [INVALID]
    assert hbx_ctx.echo_slots()[0][0, 3] == 0
    assert _add(hbx_ctx, [(pa[3], 0, 3)]).tolist() == [STORED]
    # max_shard_len + 2 value bytes do not fit, max_shard_len + 1 do (the index byte is not stored)
    fit, _ = _proofs(b"F" * 36, n, variant)   # (36 + 4) / 2 = 20-byte shards: 21-byte values
    over, _ = _proofs(b"O" * 38, n, variant)  # 21-byte shards: 22-byte values
    assert len(fit[0]["value"]) == 21 and len(over[0]["value"]) == 22
    assert _add(hbx_ctx, [(over[0], 1, 0), (fit[1], 1, 1)]).tolist() == [OVERSIZE, STORED]
    state, lens, _, rows = _table(hbx_ctx)
    assert state[1].tolist() == [0, 1, 0, 0] and lens[1, 1] == 20 and rows[n + 1, :20].tobytes() == fit[1]["value"][1:]
    assert (rows[-1] == 0xA5).all()


# ---- partitions -----------------------------------------------------------------------------------
def epoch_items(events, n, me):
    """The items a session makes of a receive log (no own input: me proposes nothing here)."""
    items = []
    for ev in events:
        if ev[0] in ("value", "echo"):
            _, sender, proposer, p = ev
            if 0 <= proposer < n and 0 <= sender < n and (ev[0] == "echo" or sender == proposer) and proof_shape_ok(p):
                items.append((p, proposer, me if ev[0] == "value" else sender))
    return items


@pytest.mark.parametrize("variant", VARIANTS)
def test_partitions_leave_the_same_store(hbx_ctx, variant):
    n, me = 7, 6
    events, _ = epoch_scenario(n, me, 1, variant)
    items = epoch_items([ev for ev in events if ev[0] != "input"], n, me)
    assert len(items) > n * (n - 1)
    rnd = random.Random(3)
    cuts = sorted(rnd.sample(range(1, len(items)), 9))
    partitions = {"layers": [items], "single": [[it] for it in items],
                  "random": [items[a:b] for a, b in zip([0] + cuts, cuts + [len(items)])]}
    results = {}
    for name, chunks in partitions.items():
        _prepare(hbx_ctx, variant, n, n, MAX_SHARD)
        status = []
        for chunk in chunks:
            st = np.zeros(len(chunk), dtype=np.uint8)
            for layer in hbx.layers([it[1:] for it in chunk]):
                st[layer] = _add(hbx_ctx, [chunk[j] for j in layer])
            status += st.tolist()
        results[name] = (status, _table(hbx_ctx))
    ref_status, ref_table = results["layers"]
    assert DUPLICATE in ref_status and INVALID in ref_status and ref_status.count(STORED) == int(ref_table[0].sum())
    for name in ("single", "random"):
        assert results[name][0] == ref_status, name
        assert _same_table(results[name][1], ref_table), name


# ---- the listed decode ------------------------------------------------------------------------------
def decode_store(variant):
    """n = 7 (k = 3, m = 4): what goes into the store, (proof, inst, sender), and the attempts
    (inst, root, len, senders allowed, name)."""
    n = 7
    k, m = rm.coding_counts(n)
    rng = random.Random(17)
    items, attempts = [], []
    every = tuple(range(n))

    def tree_of(shards):
        leaves, tree = _tree(shards, variant)
        return [tree.gen_proof(leaf) for leaf in leaves], tree.root_hash()

    pr, root = _proofs(rng.randbytes(50), n, variant)  # 18-byte shards
    items += [(pr[i], 0, i) for i in range(n)]
    attempts.append((0, root, 18, every, "all present"))
    pr, root = _proofs(rng.randbytes(800), n, variant)  # 268-byte shards
    items += [(pr[i], 1, i) for i in range(n - k, n)]
    attempts.append((1, root, 268, every, "the last k: every data shard reconstructed"))
    pr, root = _proofs(rng.randbytes(95), n, variant)  # 33-byte shards
    items += [(pr[i], 2, i) for i in range(n)]
    attempts.append((2, root, 33, (1, 3, 4, 6), "use restricts a fuller store"))
    attempts.append((2, root, 33, (0, 6), "too few shards under use"))
    pa, root_a = _proofs(rng.randbytes(20), n, variant)  # 8-byte shards
    pb, root_b = _proofs(rng.randbytes(41), n, variant)  # 15-byte shards
    items += [(pa[i], 3, i) for i in range(4)] + [(pb[i], 3, i) for i in range(4, n)]
    attempts.append((3, root_a, 8, every, "first root of two"))
    attempts.append((3, root_b, 15, every, "second root of two"))
    sh = [bytes(s) for s in rm.send_shards(rng.randbytes(60), n, variant)[0]]  # 22-byte shards, one of 23
    sh[1] += b"\x00"
    pr, root = tree_of(sh)
    items += [(pr[i], 4, i) for i in range(n)]
    attempts.append((4, root, 22, every, "shard size"))
    attempts.append((4, root, 22, (0, 1), "shard size and too few"))
    # without the odd shard the sizes agree, but the rebuilt shard 1 is not the 23-byte leaf of the tree
    attempts.append((4, root, 22, (0, 2, 3, 5), "root mismatch: the odd shard left out and rebuilt"))
    pr, root = _proofs(rng.randbytes(33), n, variant)
    items += [(pr[i], 5, i) for i in (2, 5)]
    attempts.append((5, root, 13, every, "too few shards"))
    tampered = rm.send_shards(rng.randbytes(70), n, variant)[0].copy()  # epoch_scenario's proposer 2
    tampered[0, 5] ^= 0x5A
    pr, root = tree_of(tampered)
    items += [(pr[i], 6, i) for i in range(n)]
    attempts.append((6, root, tampered.shape[1], (0, 1, 2, 3, 5, 6), "root mismatch: a shard rebuilt from the tampered one"))
    attempts.append((6, root, tampered.shape[1], every, "the tampered tree with nothing to rebuild"))
    big = rm.frame_shards(b"payload of a faulty proposer" * 3, n)
    big[0, :4] = 0xFF
    pr, root = tree_of(rm.ReedSolomon(k, m).encode(big))
    items += [(pr[i], 7, i) for i in range(n) if i != 4]
    attempts.append((7, root, big.shape[1], every, "header longer than the payload"))
    return n, k, m, items, attempts


def ragged_reference(ctx, n, k, m, held, attempts, variant):
    """hbx_broadcast_decode_ragged_d(d_leaf_hash=...) on host-assembled buffers of the same values,
    for the attempts it can express (present shards of one length) -> {attempt index: (status, payload)}."""
    sel, rows_of = [], []
    for a, (q, root, length, allowed, _) in enumerate(attempts):
        vals = {i: held[(q, i)] for i in allowed if (q, i) in held and held[(q, i)]["root_hash"] == root}
        if vals and all(len(p["value"]) - 1 == length for p in vals.values()):
            sel.append(a)
            rows_of.append(vals)
    lens = np.array([attempts[a][2] for a in sel], dtype=np.uint32)
    off, pitch, total = hbx.ragged_layout(lens, n)
    buf = np.zeros(total, dtype=np.uint8)
    present = np.zeros((len(sel), n), dtype=np.uint8)
    leaf = np.zeros((len(sel), n, 32), dtype=np.uint8)
    roots = np.stack([np.frombuffer(attempts[a][1], dtype=np.uint8) for a in sel])
    for r, vals in enumerate(rows_of):
        rows = buf[int(off[r]): int(off[r]) + n * int(pitch[r])].reshape(n, int(pitch[r]))
        for i, p in vals.items():
            rows[i, : lens[r]] = np.frombuffer(p["value"], dtype=np.uint8, offset=1)
            present[r, i] = 1
            leaf[r, i] = np.frombuffer(p["lemma"][-1][0], dtype=np.uint8)
    room = (np.maximum(k * lens.astype(np.int64) - 4, 0) + 15) // 16 * 16
    out_off = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.uint64)
    d_out = torch.zeros(max(int(room.sum()), 16), dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(len(sel), dtype=torch.int64, device="cuda")
    d_st = torch.zeros(len(sel), dtype=torch.int32, device="cuda")
    ctx.broadcast_decode_ragged_d(dev(buf), off, lens, pitch, dev(present), dev(roots), k, m, d_out, out_off, d_len, d_st,
                                  d_leaf_hash=dev(leaf))
    torch.cuda.synchronize()
    st, ln, ob_ = d_st.cpu().numpy(), d_len.cpu().numpy(), d_out.cpu().numpy()
    return {a: (int(st[r]), ob_[int(out_off[r]): int(out_off[r]) + int(ln[r])].tobytes()) for r, a in enumerate(sel)}


@pytest.mark.parametrize("variant", VARIANTS)
def test_listed_decode(hbx_ctx, variant):
    n, k, m, items, attempts = decode_store(variant)
    _prepare(hbx_ctx, variant, 9, n, 300)  # instance 8 stays empty: the last used row is not the last row
    assert _add(hbx_ctx, items).tolist() == [STORED] * len(items)
    held = {(q, i): p for p, q, i in items}
    table = _table(hbx_ctx)
    insts = [a[0] for a in attempts]
    roots = np.stack([np.frombuffer(a[1], dtype=np.uint8) for a in attempts])
    lens = [a[2] for a in attempts]
    use = np.zeros((len(attempts), n), dtype=np.uint8)
    for r, a in enumerate(attempts):
        use[r, list(a[3])] = 1
    vals, status = hbx_ctx.broadcast_decode_insts(insts, roots, lens, use)
    by_name = {a[4]: int(status[r]) for r, a in enumerate(attempts)}
    assert by_name["shard size"] == by_name["shard size and too few"] == hbx.HBX_E_SHARD_SIZE
    assert by_name["too few shards"] == by_name["too few shards under use"] == hbx.HBX_E_TOO_FEW_SHARDS
    assert by_name["root mismatch: a shard rebuilt from the tampered one"] == hbx.HBX_E_ROOT_MISMATCH
    assert by_name["root mismatch: the odd shard left out and rebuilt"] == hbx.HBX_E_ROOT_MISMATCH
    assert list(by_name.values()).count(0) == 7
    # the oracle, attempt by attempt
    for r, (q, root, length, allowed, name) in enumerate(attempts):
        leaf_values = [held[(q, i)]["value"] if i in allowed and (q, i) in held and held[(q, i)]["root_hash"] == root
                       else None for i in range(n)]
        assert vals[r] == ob.decode_from_shards(leaf_values, n, root, variant), name
    assert len(vals[[a[4] for a in attempts].index("header longer than the payload")]) == k * attempts[-1][2] - 4
    # the ragged decode on host-assembled buffers
    ref = ragged_reference(hbx_ctx, n, k, m, held, attempts, variant)
    assert len(ref) == len(attempts) - 2  # all but the two shard-size attempts
    for a, (st, payload) in ref.items():
        assert st == int(status[a]) and (payload if st == 0 else None) == vals[a], attempts[a][4]
    # a decode writes nothing into the store; the same list again gives the same
    assert _same_table(_table(hbx_ctx), table)
    vals2, status2 = hbx_ctx.broadcast_decode_insts(insts, roots, lens, use)
    assert vals2 == vals and status2.tolist() == status.tolist()
    assert _same_table(_table(hbx_ctx), table)
    # without `use` every held sender of the root counts
    v, s = hbx_ctx.broadcast_decode_insts([2, 3], roots[[2, 4]], [33, 8])
    assert s.tolist() == [0, 0] and v == [vals[2], vals[4]]


# ---- the session ------------------------------------------------------------------------------------
class CountingEngine(GpuBroadcastAddEngine):
    """Checks that a listed decode uploads no value bytes."""

    def decode_listed(self, attempts):
        before = self.value_bytes_uploaded
        out = super().decode_listed(attempts)
        assert self.value_bytes_uploaded == before
        return out


def _merkle(variant):
    return hbx.MERKLE_SHA3 if variant == "sha3" else hbx.MERKLE_SHA256


def _item_bytes(events, n, me, own_len=0):
    return sum(len(p["value"]) for p, _, _ in epoch_items(events, n, me)) + own_len


@pytest.mark.parametrize("every", SCHEDULES)
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("n,me,seed,short", [e for e in EPOCHS if e[0] in (7, 13)])
def test_session_epoch(hbx_ctx, n, me, seed, short, variant, every):
    events, values = epoch_scenario(n, me, seed, variant, short_leaves=short)
    node = ob.BroadcastNode(n, me, variant).run(events)
    eng = CountingEngine(hbx_ctx, _merkle(variant))
    total, ses = run_session(eng, n, me, events, every)
    check_against_oracle(total, node, n)
    k = rm.coding_counts(n)[0]
    own = 1 + -(-(len(values[me]) + 4) // k)  # our own Value proof: index byte + shard
    assert eng.value_bytes_uploaded == _item_bytes(events, n, me, own)
    assert ses.engine_decodes <= len(node.decode_attempts)


@pytest.mark.parametrize("every", SCHEDULES)
@pytest.mark.parametrize("adv", ["silent", "propose", "random"])
def test_session_simulated(hbx_ctx, adv, every):
    n = 7
    received, nodes = simulate(n, adv, "random", sim_value(adv), seed=1000 * n + len(adv) + len("random"))
    for i in (0, max(received)):
        eng = CountingEngine(hbx_ctx, hbx.MERKLE_SHA256)
        total, _ = run_session(eng, n, i, received[i], every, max_shard_len=64)
        check_against_oracle(total, nodes[i], n)
        assert total.outputs == [(0, sim_value(adv))]


def test_session_epoch_n40(hbx_ctx):
    n, me = 40, 39
    events, values = epoch_scenario(n, me, 4)
    node = ob.BroadcastNode(n, me).run(events)
    eng = CountingEngine(hbx_ctx, hbx.MERKLE_SHA256)
    total, _ = run_session(eng, n, me, events, 40)
    check_against_oracle(total, node, n)
    k = rm.coding_counts(n)[0]
    assert eng.value_bytes_uploaded == _item_bytes(events, n, me, 1 + -(-(len(values[me]) + 4) // k))


# ---- lifecycle ----------------------------------------------------------------------------------
def test_lifecycle():
    live0 = hbx.live_buffers()
    ctx = hbx.Context(0)
    n = 4
    pr, root = _proofs(b"lifecycle", n, "sha256")
    one = [(pr[1], 0, 1)]
    roots = np.frombuffer(root, dtype=np.uint8).reshape(1, 32)

    def refused(call):
        with pytest.raises(hbx.HbxError) as e:
            call()
        return e.value.code

    # before a prepare
    assert refused(lambda: _add(ctx, one)) == hbx.HBX_E_NO_BROADCAST
    assert ctx.lib.hbx_get_echo_slots(ctx.h, None, None, None) == hbx.HBX_E_NO_BROADCAST
    i0, l7, o0 = np.zeros(1, dtype=np.uint32), np.full(1, 7, dtype=np.uint32), np.zeros(1, dtype=np.uint64)
    out, out_len, st1 = np.zeros(16, dtype=np.uint8), np.zeros(1, dtype=np.uint64), np.zeros(1, dtype=np.int32)
    assert ctx.lib.hbx_broadcast_decode_insts(ctx.h, i0.ctypes.data, roots.ctypes.data, l7.ctypes.data, None, 1,
                                              out.ctypes.data, out.size, o0.ctypes.data, out_len.ctypes.data,
                                              st1.ctypes.data) == hbx.HBX_E_NO_BROADCAST
    ctx.prepare_broadcast(2, 2, 2, 16)
    assert _add(ctx, one).tolist() == [STORED]
    vals, st = ctx.broadcast_decode_insts([0], roots, [7])
    assert st.tolist() == [hbx.HBX_E_TOO_FEW_SHARDS] and vals == [None]
    # INVALID_ARG before anything is launched: the table is unchanged
    table = _table(ctx)
    assert refused(lambda: _add(ctx, [(pr[2], 2, 2)])) == hbx.HBX_E_INVALID_ARG          # instance at the count
    assert ctx.lib.hbx_add_echoes(ctx.h, *_raw(one, sender=4)) == hbx.HBX_E_INVALID_ARG  # sender at n
    assert ctx.lib.hbx_add_echoes(ctx.h, *_raw([(pr[2], 0, 2), (pr[3], 0, 2)])) == hbx.HBX_E_INVALID_ARG  # a pair twice
    assert ctx.lib.hbx_add_echoes(ctx.h, *_raw(one, val_off=[3, 1])) == hbx.HBX_E_INVALID_ARG
    assert refused(lambda: ctx.broadcast_decode_insts([2], roots, [7])) == hbx.HBX_E_INVALID_ARG
    assert refused(lambda: ctx.broadcast_decode_insts([0], roots, [17])) == hbx.HBX_E_INVALID_ARG    # len > max_shard_len
    assert _same_table(_table(ctx), table)
    assert _add(ctx, []).tolist() == [] and ctx.broadcast_decode_insts([], roots[:0], [])[0] == []
    # a re-prepare empties the store
    ctx.prepare_broadcast(2, 2, 2, 16)
    assert int(ctx.echo_slots()[0].sum()) == 0
    assert _add(ctx, one).tolist() == [STORED]
    # a digest change voids it
    ctx.set_merkle_digest(hbx.MERKLE_SHA3)
    assert refused(lambda: _add(ctx, one)) == hbx.HBX_E_NO_BROADCAST
    assert refused(lambda: ctx.broadcast_decode_insts([0], roots, [7])) == hbx.HBX_E_NO_BROADCAST
    assert refused(lambda: ctx.echo_slots()) == hbx.HBX_E_NO_BROADCAST
    ctx.prepare_broadcast(2, 2, 2, 16)
    assert int(ctx.echo_slots()[0].sum()) == 0
    assert hbx.live_buffers() > live0
    ctx.close()
    assert hbx.live_buffers() == live0


def _raw(items, sender=None, val_off=None):
    """The raw argument list of hbx_add_echoes after the context (past the binding's own checks)."""
    blob, off, nh, sh, sides, depth, root, snd = flatten_proofs_ragged([p for p, _, _ in items], [s for _, _, s in items])
    if sender is not None:
        snd = np.full(len(items), sender, dtype=np.uint32)
    if val_off is not None:
        off = np.array(val_off, dtype=np.uint64)
    inst = np.array([q for _, q, _ in items], dtype=np.uint32)
    keep = [blob, off, nh, sh, sides, depth, root, inst, np.ascontiguousarray(snd, dtype=np.uint32)]
    _raw.keep = keep  # the arrays outlive the call
    return (blob.ctypes.data, blob.size, off.ctypes.data, nh.ctypes.data, sh.ctypes.data, sides.ctypes.data,
            depth.ctypes.data, root.ctypes.data, inst.ctypes.data, keep[-1].ctypes.data, len(items), None)


# ---- the three decode forms share one tail --------------------------------------------------------
FORM_LENS = [1, 5, 8]  # a payload too short for its header; L % 4 != 0 (the uniform byte kernel); dword rows
FORM_PATTERNS = ["all present", "one data shard missing", "k - 1 present", "tampered tree", "wrong root"]


def _form_cases(k, m, variant):
    """Per shard length and pattern: (shards uint8[n, L], present [n], expected root, leaves or None
    where the store cannot hold the case).  'tampered tree': the tree is built over shard 0 with a
    flipped byte and shard 0 is withheld, so the rebuilt shard 0 misses the root (m == 0 rebuilds
    nothing: too few shards).  'wrong root': all present under a root with a flipped byte, which no
    stored proof can carry, so the store form leaves it out."""
    n, rng, cases = k + m, random.Random(1000 * k + m), []
    for L in FORM_LENS:
        if k * L >= 4:
            shards = rm.send_shards(rng.randbytes(k * L - 4), n, variant)[0]
        else:
            shards = np.zeros((n, L), dtype=np.uint8)
            shards[:k] = np.frombuffer(rng.randbytes(k * L), dtype=np.uint8).reshape(k, L)
            if m:
                shards = rm.ReedSolomon(k, m).encode(shards)
        assert shards.shape == (n, L)
        leaves, tree = _tree(shards, variant)
        bad = shards.copy()
        bad[0, 0] ^= 0x5A
        bad_leaves, bad_tree = _tree(bad, variant)
        for pattern in FORM_PATTERNS:
            present = np.ones(n, dtype=np.uint8)
            root, lv = tree.root_hash(), leaves
            if pattern == "one data shard missing":
                present[0] = 0
            elif pattern == "k - 1 present":
                present[k - 1:] = 0
            elif pattern == "tampered tree":
                present[0] = 0
                root, lv = bad_tree.root_hash(), bad_leaves
            elif pattern == "wrong root":
                root, lv = bytes([root[0] ^ 1]) + root[1:], None
            cases.append((L, pattern, shards, present, root, lv, bad_tree if pattern == "tampered tree" else tree))
    return cases


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("k,m", [(2, 2), (3, 2), (1, 0)])
def test_decode_forms_agree(hbx_ctx, k, m, variant):
    """hbx_broadcast_decode_leaves_d (one call per shard length), hbx_broadcast_decode_ragged_d with
    and without leaf digests (all lengths in one call) and hbx_broadcast_decode_insts out of an echo
    store give the same status, out_len and payload on the same shards, and the oracle's payload where
    the oracle decodes."""
    assert rm.coding_counts(k + m) == (k, m)
    n = k + m
    _set_merkle(hbx_ctx, variant)
    cases = _form_cases(k, m, variant)
    got = {}  # form -> [(status, out_len, payload)] in the order of `cases`

    def results(st, ln, out, out_off):
        st, ln, out = st.cpu().numpy(), ln.cpu().numpy(), out.cpu().numpy().reshape(-1)
        return [(int(s), int(v), out[int(o): int(o) + int(v)].tobytes() if s == 0 else None)
                for s, v, o in zip(st, ln, out_off)]

    def digests(case):
        L, _, shards, present, _, _, _ = case
        return np.stack([np.frombuffer(rm.hash_leaf(bytes([i]) + shards[i].tobytes(), variant), dtype=np.uint8)
                         if present[i] else np.zeros(32, dtype=np.uint8) for i in range(n)])

    def held(case):  # the rows a receiver holds: withheld shards are zero bytes
        return case[2] * case[3][:, None]

    # uniform rows, leaf digests given: one call per length
    got["leaves_d"] = []
    for L in FORM_LENS:
        sel = [c for c in cases if c[0] == L]
        stride = max(k * L - 4, 0) + 16
        d_out = torch.zeros((len(sel), stride), dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(len(sel), dtype=torch.int64, device="cuda")
        d_st = torch.zeros(len(sel), dtype=torch.int32, device="cuda")
        hbx_ctx.broadcast_decode_leaves_d(dev(np.stack([held(c) for c in sel])), dev(np.stack([c[3] for c in sel])),
                                          dev(np.stack([digests(c) for c in sel])),
                                          dev(np.stack([np.frombuffer(c[4], dtype=np.uint8) for c in sel])), k, m,
                                          d_out, d_len, d_st)
        torch.cuda.synchronize()
        got["leaves_d"] += results(d_st, d_len, d_out, [r * stride for r in range(len(sel))])
    # ragged rows, with and without leaf digests: every length in one call
    lens = np.array([c[0] for c in cases], dtype=np.uint32)
    off, pitch, total = hbx.ragged_layout(lens, n)
    buf = np.zeros(total, dtype=np.uint8)
    for r, c in enumerate(cases):
        buf[int(off[r]): int(off[r]) + n * int(pitch[r])].reshape(n, int(pitch[r]))[:, : c[0]] = held(c)
    room = (np.maximum(k * lens.astype(np.int64) - 4, 0) + 15) // 16 * 16
    out_off = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.uint64)
    present = dev(np.stack([c[3] for c in cases]))
    roots = np.stack([np.frombuffer(c[4], dtype=np.uint8) for c in cases])
    for form, leaf in (("ragged_d", None), ("ragged_d leaves", dev(np.stack([digests(c) for c in cases])))):
        d_out = torch.zeros(max(int(room.sum()), 16), dtype=torch.uint8, device="cuda")
        d_len = torch.zeros(len(cases), dtype=torch.int64, device="cuda")
        d_st = torch.zeros(len(cases), dtype=torch.int32, device="cuda")
        hbx_ctx.broadcast_decode_ragged_d(dev(buf), off, lens, pitch, present, dev(roots), k, m, d_out, out_off, d_len,
                                          d_st, d_leaf_hash=leaf)
        torch.cuda.synchronize()
        got[form] = results(d_st, d_len, d_out, out_off)
    # the echo store: one instance per case, the present shards' proofs added, one attempt per case
    stored = [r for r, c in enumerate(cases) if c[5] is not None]
    hbx_ctx.prepare_broadcast(len(cases), k, m, max(FORM_LENS))
    items = [(cases[r][6].gen_proof(cases[r][5][i]), r, i) for r in stored for i in range(n) if cases[r][3][i]]
    if items:
        assert _add(hbx_ctx, items).tolist() == [STORED] * len(items)
    vals, status = hbx_ctx.broadcast_decode_insts(stored, roots[stored], lens[stored])
    # equal across the forms, and the oracle's payload where the oracle decodes
    for r, (L, pattern, shards, pres, root, lv, _) in enumerate(cases):
        what = (L, pattern)
        assert got["leaves_d"][r] == got["ragged_d"][r] == got["ragged_d leaves"][r], what
        st, ln, payload = got["ragged_d"][r]
        if r in stored:
            a = stored.index(r)
            assert (int(status[a]), vals[a]) == (st, payload), what
        leaf_values = [bytes([i]) + shards[i].tobytes() if pres[i] else None for i in range(n)]
        want = ob.decode_from_shards(leaf_values, n, root, variant)
        if want is not None:
            assert st == 0 and payload == want and ln == len(want), what
        elif k * L >= 4:  # the oracle's None is a decode error, not a payload too short for its header
            assert st != 0, what
    by = {(c[0], c[1]): got["ragged_d"][r][0] for r, c in enumerate(cases)}
    assert by[(8, "all present")] == 0 and by[(5, "all present")] == 0
    assert by[(8, "wrong root")] == hbx.HBX_E_ROOT_MISMATCH
    if m:
        assert by[(8, "k - 1 present")] == hbx.HBX_E_TOO_FEW_SHARDS
        assert by[(8, "tampered tree")] == hbx.HBX_E_ROOT_MISMATCH
        assert by[(8, "one data shard missing")] == 0
