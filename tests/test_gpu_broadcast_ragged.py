"""GPU parity for the ragged Broadcast calls (per-instance shard lengths in one call, include/hbx.h
hbx_*_ragged_d) against the oracle (oracle/rs_merkle.py) and, instance by instance, against the
uniform entry points: byte-exact.  Every buffer has its pad bytes [len, pitch) filled with 0xA5 and
64 canary bytes between the instances and after the last one, which must survive every call."""
import functools
import random

import numpy as np
import pytest

from oracle import broadcast as ob
from oracle import rs_merkle as rm

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HBX_E_TOO_FEW_SHARDS = -9
HBX_E_ROOT_MISMATCH = -10
HBX_E_NO_PAYLOAD = -11
GUARD, CANARY, PAD = 64, 0xC3, 0xA5
# not multiples of 4, and on both sides of a wave's 512-byte and a block's 2,048-byte span
LENS = [1, 2, 3, 4, 5, 63, 64, 65, 257, 2044, 2048, 2052, 4100]
CODE_CASES = [(2, 2, LENS), (3, 4, LENS), (5, 8, LENS), (44, 84, [1, 33, 1000])]  # the last: several grid.z passes


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _set_merkle(ctx, variant):
    from hbbft_amd.hbx import MERKLE_SHA3, MERKLE_SHA256

    ctx.set_merkle_digest(MERKLE_SHA3 if variant == "sha3" else MERKLE_SHA256)


class Ragged:
    """A host image of a ragged buffer: pitch = len rounded up to 16, GUARD canary bytes after every
    instance, pads PAD."""

    def __init__(self, lens, n):
        self.lens = np.asarray(lens, dtype=np.uint32)
        self.n = n
        self.pitch = ((self.lens + 15) // 16 * 16).astype(np.uint32)
        size = self.pitch.astype(np.int64) * n + GUARD
        self.off = np.concatenate(([0], np.cumsum(size)[:-1])).astype(np.uint64)
        self.buf = np.full(int(size.sum()), CANARY, dtype=np.uint8)
        for q in range(len(lens)):
            self.rows(q)[:] = PAD

    def rows(self, q, buf=None):
        """[n, pitch] view of instance q (of `buf`, an image of the same layout)."""
        o, p = int(self.off[q]), int(self.pitch[q])
        return (self.buf if buf is None else buf)[o: o + self.n * p].reshape(self.n, p)

    def data(self, q, buf=None):
        return self.rows(q, buf)[:, : int(self.lens[q])]

    def desc(self):
        return self.off, self.lens, self.pitch

    def canaries_intact(self, buf):
        mask = np.ones(buf.size, dtype=bool)
        for q in range(len(self.lens)):
            o = int(self.off[q])
            mask[o: o + self.n * int(self.pitch[q])] = False
        return mask.sum() == GUARD * len(self.lens) and (buf[mask] == CANARY).all()


@functools.lru_cache(maxsize=None)
def encoded(k, m, lens):
    """The oracle's encoded shards [n, L] of one random instance per length (shared, read-only)."""
    rs = rm.ReedSolomon(k, m)
    rng = np.random.default_rng(k * 100 + m)
    out = []
    for L in lens:
        a = np.zeros((k + m, L), dtype=np.uint8)
        a[:k] = rng.integers(0, 256, size=(k, L), dtype=np.uint8)
        a = rs.encode(a)
        a.setflags(write=False)
        out.append(a)
    return out


@pytest.mark.parametrize("k,m,lens", CODE_CASES)
def test_rs_encode_ragged(hbx_ctx, k, m, lens):
    full = encoded(k, m, tuple(lens))
    r = Ragged(lens, k + m)
    for q in range(len(lens)):
        r.data(q)[:k] = full[q][:k]
    d = dev(r.buf)
    hbx_ctx.rs_encode_ragged_d(d, *r.desc(), k, m)
    torch.cuda.synchronize()
    out = d.cpu().numpy()
    for q in range(len(lens)):
        np.testing.assert_array_equal(r.data(q, out), full[q], err_msg=f"L={lens[q]}")
    assert r.canaries_intact(out)
    # instance by instance through the uniform call
    for q in [0, len(lens) // 2, len(lens) - 1]:
        u = np.zeros((1, k + m, lens[q]), dtype=np.uint8)
        u[0, :k] = full[q][:k]
        du = dev(u)
        hbx_ctx.rs_encode_d(du, k, m)
        np.testing.assert_array_equal(du.cpu().numpy()[0], r.data(q, out))


def erasures(k, m, q):
    """A different pattern per instance: data only / parity only / mixed / exactly m / m + 1 missing."""
    n, rnd = k + m, random.Random(q)
    kind = q % 5
    if kind == 0:
        return rnd.sample(range(k), min(k, max(1, m // 2)))
    if kind == 1:
        return rnd.sample(range(k, n), max(1, m // 2))
    if kind == 2:
        return [rnd.randrange(k), k + rnd.randrange(m)]
    return rnd.sample(range(n), m if kind == 3 else m + 1)


@pytest.mark.parametrize("k,m,lens", CODE_CASES)
def test_rs_reconstruct_ragged(hbx_ctx, k, m, lens):
    if len(lens) < 5:
        lens = lens + [1000, 33]  # all five erasure patterns
    full = encoded(k, m, tuple(lens))
    n, inst = k + m, len(lens)
    r = Ragged(lens, n)
    present = np.ones((inst, n), dtype=np.uint8)
    for q in range(inst):
        r.data(q)[:] = full[q]
        for i in erasures(k, m, q):
            present[q, i] = 0
            r.rows(q)[i] = PAD
    d = dev(r.buf)
    st = torch.full((inst,), 77, dtype=torch.int32, device="cuda")
    hbx_ctx.rs_reconstruct_ragged_d(d, *r.desc(), dev(present), st, k, m)
    torch.cuda.synchronize()
    out, st = d.cpu().numpy(), st.cpu().numpy()
    for q in range(inst):
        if q % 5 == 4:
            assert st[q] == HBX_E_TOO_FEW_SHARDS, q
            np.testing.assert_array_equal(r.rows(q, out)[present[q] == 1], r.rows(q)[present[q] == 1])
        else:
            assert st[q] == 0, q
            np.testing.assert_array_equal(r.data(q, out), full[q], err_msg=f"L={lens[q]}")
    assert r.canaries_intact(out)
    q = 3  # exactly m missing, through the uniform call
    u = np.ascontiguousarray(r.data(q))[None]
    du, su = dev(u), torch.zeros(1, dtype=torch.int32, device="cuda")
    hbx_ctx.rs_reconstruct_d(du, dev(present[q: q + 1]), su, k, m)
    assert int(su[0]) == 0
    np.testing.assert_array_equal(du.cpu().numpy()[0], r.data(q, out))


# message = 2 + L bytes (SHA-256, padding block boundary at 55 / 119) or 1 + L (SHA3, rate 136)
MERKLE_LENS = [1, 52, 53, 54, 61, 62, 63, 117, 118, 134, 135, 136, 270, 271, 300]


@pytest.mark.parametrize("variant", ["sha256", "sha3"])
@pytest.mark.parametrize("n", [1, 3, 4, 7, 13])
def test_merkle_build_ragged(hbx_ctx, n, variant):
    _set_merkle(hbx_ctx, variant)
    inst = len(MERKLE_LENS)
    r = Ragged(MERKLE_LENS, n)
    rng = np.random.default_rng(n)
    for q in range(inst):
        r.data(q)[:] = rng.integers(0, 256, size=(n, MERKLE_LENS[q]), dtype=np.uint8)
    cnt = hbx_ctx.merkle_node_count(n)
    d = dev(r.buf)
    nodes = torch.zeros((inst, cnt, 32), dtype=torch.uint8, device="cuda")
    roots = torch.zeros((inst, 32), dtype=torch.uint8, device="cuda")
    roots_only = torch.zeros((inst, 32), dtype=torch.uint8, device="cuda")
    hbx_ctx.merkle_build_ragged_d(d, *r.desc(), n, nodes, roots)
    hbx_ctx.merkle_build_ragged_d(d, *r.desc(), n, d_roots=roots_only)
    req = np.array([(i, j) for i in range(inst) for j in range(n)], dtype=np.uint32)
    P = len(req)
    nh = torch.zeros((P, 17, 32), dtype=torch.uint8, device="cuda")
    sh = torch.zeros((P, 16, 32), dtype=torch.uint8, device="cuda")
    sides = torch.zeros(P, dtype=torch.int32, device="cuda")
    depth = torch.zeros(P, dtype=torch.int32, device="cuda")
    proot = torch.zeros((P, 32), dtype=torch.uint8, device="cuda")
    hbx_ctx.merkle_proofs_d(nodes, n, dev(req), nh, sh, sides, depth, proot)
    torch.cuda.synchronize()
    assert (d.cpu().numpy() == r.buf).all()  # a build reads only
    nodes, roots = nodes.cpu().numpy(), roots.cpu().numpy()
    np.testing.assert_array_equal(roots_only.cpu().numpy(), roots)
    nh, sh, sides, depth, proot = (nh.cpu().numpy(), sh.cpu().numpy(), sides.cpu().numpy().view(np.uint32),
                                   depth.cpu().numpy(), proot.cpu().numpy())
    from hbbft_amd.broadcast import unflatten_proof

    for q in range(inst):
        leaves = [bytes([j]) + r.data(q)[j].tobytes() for j in range(n)]
        tree = rm.MerkleTree(leaves, variant)
        assert [bytes(x) for x in nodes[q]] == [h for lvl in tree.levels for h in lvl], MERKLE_LENS[q]
        assert roots[q].tobytes() == tree.root_hash()
        for j in range(n):
            e = q * n + j
            p = unflatten_proof(leaves[j], nh[e], sh[e], int(sides[e]), int(depth[e]), proot[e])
            assert rm.validate_broadcast_proof(p, j, n, variant), (q, j)


@functools.lru_cache(maxsize=None)
def validate_case(variant):
    """Proofs of proposals of five sizes at n = 4, 7, 13 (values of 2 .. 100,003 bytes, on both sides
    of the 256-byte switch), with the six bad proofs per instance; and the oracle's verdicts."""
    proofs, senders, counts = [], [], []
    for n in (4, 7, 13):
        for size in (3, 32, 700, 5000, 200_003):
            value = (bytes(range(256)) * (size // 256 + 1))[:size]
            _, leaves, tree = rm.send_shards(value, n, variant)
            good = [tree.gen_proof(leaf) for leaf in leaves]
            p = good[1]
            v = p["value"]
            lem = list(p["lemma"])
            h, (side, sib) = lem[0]
            lem[0] = (h, (side, bytes([sib[0] ^ 0x80]) + sib[1:]))
            bad = [(dict(p, value=v[:-1] + bytes([v[-1] ^ 1])), 1),      # flipped value byte
                   (p, 2),                                               # wrong sender
                   (dict(p, lemma=lem), 1),                              # corrupted sibling
                   (dict(p, root_hash=b"\x11" * 32), 1),                 # wrong root
                   (dict(p, value=v[:1]), 1),                            # a value of length 1
                   (dict(p, value=b""), 1)]                              # an empty value
            for q, s in [(g, i) for i, g in enumerate(good)] + bad:
                proofs.append(q)
                senders.append(s)
                counts.append(n)
    want = [len(p["value"]) > 0 and rm.validate_broadcast_proof(p, s, n, variant)
            for p, s, n in zip(proofs, senders, counts)]
    return proofs, senders, counts, want


@pytest.mark.parametrize("variant", ["sha256", "sha3"])
def test_merkle_validate_ragged(hbx_ctx, variant):
    from hbbft_amd.broadcast import flatten_proofs_ragged

    _set_merkle(hbx_ctx, variant)
    proofs, senders, counts, want = validate_case(variant)
    assert sum(want) == 5 * (4 + 7 + 13)
    for n in (4, 7, 13):
        sel = [j for j, c in enumerate(counts) if c == n]
        got = []
        for seed in (1, 2):  # the verdicts must not depend on the order (nor on the host's grouping)
            order = list(sel)
            random.Random(seed).shuffle(order)
            blob, val_off, *arrs = flatten_proofs_ragged([proofs[j] for j in order], [senders[j] for j in order])
            assert len({int(b - a) for a, b in zip(val_off[:64], val_off[1:65])}) > 2  # lengths differ inside a block
            valid = torch.full((len(order),), 9, dtype=torch.uint8, device="cuda")
            hbx_ctx.merkle_validate_ragged_d(dev(blob), val_off, *[dev(a) for a in arrs], n, valid)
            torch.cuda.synchronize()
            v = valid.cpu().numpy()
            got.append({j: int(v[r]) for r, j in enumerate(order)})
            assert [got[-1][j] for j in sel] == [int(want[j]) for j in sel], (n, seed)
        assert got[0] == got[1]
        # the uniform call, length by length
        by_len = {}
        for j in sel:
            if proofs[j]["value"]:
                by_len.setdefault(len(proofs[j]["value"]), []).append(j)
        from hbbft_amd.broadcast import flatten_proofs

        for _, idx in sorted(by_len.items()):
            arrs = flatten_proofs([proofs[j] for j in idx], [senders[j] for j in idx])
            valid = torch.zeros(len(idx), dtype=torch.uint8, device="cuda")
            hbx_ctx.merkle_validate_d(*[dev(a) for a in arrs], n, valid)
            assert valid.cpu().numpy().tolist() == [got[0][j] for j in idx]


def decode_case(variant):
    """Seven instances at n = 4 (k = 2, m = 2) ending in every status, plus the oversized header."""
    n = 4
    k, m = rm.coding_counts(n)
    inst = []  # (shards [n, L], present, root, leaves)

    def add(shards, missing=(), bad_root=False):
        shards = np.asarray(shards, dtype=np.uint8)
        leaves = [bytes([i]) + shards[i].tobytes() for i in range(n)]
        root = bytearray(rm.MerkleTree(leaves, variant).root_hash())
        if bad_root:
            root[5] ^= 1
        present = np.ones(n, dtype=np.uint8)
        present[list(missing)] = 0
        inst.append((shards, present, bytes(root), leaves))

    add(rm.send_shards(b"Foo", n, variant)[0], missing=[0])                        # OK, one data shard rebuilt
    add(rm.send_shards(bytes(range(256)) * 9, n, variant)[0], missing=[1, 3])      # OK, exactly m missing
    add(rm.send_shards(b"x" * 301, n, variant)[0], missing=[0, 1, 2])              # too few shards
    add(rm.send_shards(b"y" * 77, n, variant)[0], missing=[2], bad_root=True)      # root mismatch
    add(rm.ReedSolomon(k, m).encode(np.array([[7], [9], [0], [0]], dtype=np.uint8)))  # L = 1: no payload
    big = rm.frame_shards(b"payload of a faulty proposer" * 3, n)
    big[0, :4] = 0xFF                                                              # header 2^32 - 1: clamped
    add(rm.ReedSolomon(k, m).encode(big), missing=[3])
    add(rm.send_shards(b"", n, variant)[0])                                        # OK, empty payload (L = 2)
    return n, k, m, inst


@pytest.mark.parametrize("with_leaves", [False, True])
@pytest.mark.parametrize("variant", ["sha256", "sha3"])
def test_broadcast_decode_ragged(hbx_ctx, variant, with_leaves):
    _set_merkle(hbx_ctx, variant)
    n, k, m, cases = decode_case(variant)
    inst = len(cases)
    lens = [c[0].shape[1] for c in cases]
    r = Ragged(lens, n)
    present = np.stack([c[1] for c in cases])
    roots = np.stack([np.frombuffer(c[2], dtype=np.uint8) for c in cases])
    leaf = np.zeros((inst, n, 32), dtype=np.uint8)
    for q, (shards, pres, _, leaves) in enumerate(cases):
        r.data(q)[:] = shards
        r.rows(q)[pres == 0] = PAD
        for i in range(n):
            if pres[i]:
                leaf[q, i] = np.frombuffer(rm.MerkleTree(leaves, variant).levels[0][i], dtype=np.uint8)
    # payload ranges in reverse order with 8 spare bytes between them
    room = [max(k * L - 4, 0) for L in lens]
    out_off = np.zeros(inst, dtype=np.uint64)
    pos = 8
    for q in reversed(range(inst)):
        out_off[q] = pos
        pos += room[q] + 8
    d_out = torch.full((pos,), CANARY, dtype=torch.uint8, device="cuda")
    d_len = torch.full((inst,), -1, dtype=torch.int64, device="cuda")
    d_st = torch.zeros(inst, dtype=torch.int32, device="cuda")
    d = dev(r.buf)
    hbx_ctx.broadcast_decode_ragged_d(d, *r.desc(), dev(present), dev(roots), k, m, d_out, out_off, d_len, d_st,
                                      d_leaf_hash=dev(leaf) if with_leaves else None)
    torch.cuda.synchronize()
    st, ln, out = d_st.cpu().numpy(), d_len.cpu().numpy(), d_out.cpu().numpy()
    assert st.tolist() == [0, 0, HBX_E_TOO_FEW_SHARDS, HBX_E_ROOT_MISMATCH, HBX_E_NO_PAYLOAD, 0, 0]
    written = np.zeros(pos, dtype=bool)
    for q, (shards, pres, root, leaves) in enumerate(cases):
        want = rm.decode_from_shards([leaves[i] if pres[i] else None for i in range(n)], n, root, variant)
        o = int(out_off[q])
        if st[q] == 0:
            assert out[o: o + int(ln[q])].tobytes() == want, q
            written[o: o + int(ln[q])] = True
        else:
            assert want is None and ln[q] == 0, q
        # the uniform call on this instance alone
        u = np.ascontiguousarray(r.data(q))[None]
        uo = torch.zeros((1, max(k * lens[q], 4)), dtype=torch.uint8, device="cuda")
        ul = torch.zeros(1, dtype=torch.int64, device="cuda")
        us = torch.zeros(1, dtype=torch.int32, device="cuda")
        args = (dev(present[q: q + 1]), dev(roots[q: q + 1]), k, m, uo, ul, us)
        if with_leaves:
            hbx_ctx.broadcast_decode_leaves_d(dev(u), args[0], dev(leaf[q: q + 1]), *args[1:])
        else:
            hbx_ctx.broadcast_decode_d(dev(u), *args)
        assert int(us[0]) == st[q] and int(ul[0]) == ln[q], q
        assert uo.cpu().numpy()[0, : int(ln[q])].tobytes() == out[o: o + int(ln[q])].tobytes()
    assert ln[5] == k * lens[5] - 4 and ln[6] == 0  # the clamp; the empty payload
    assert (out[~written] == CANARY).all()          # nothing outside the payloads
    assert r.canaries_intact(d.cpu().numpy())


def test_broadcast_decode_ragged_short_output_rejected(hbx_ctx):
    from hbbft_amd.hbx import HbxError

    n, k, m, cases = decode_case("sha256")
    r = Ragged([cases[5][0].shape[1]], n)
    need = k * int(r.lens[0]) - 4
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device="cuda")  # noqa: E731
    with pytest.raises((HbxError, ValueError)):
        hbx_ctx.broadcast_decode_ragged_d(dev(r.buf), *r.desc(), z(1, n), z(1, 32), k, m, z(need - 1), [0],
                                          z(1, dt=torch.int64), z(1, dt=torch.int32))


# ---- engine ------------------------------------------------------------------------------------
class Counting:
    """hbx.Context with its validate / decode entry points counted."""

    NAMES = ("merkle_validate_d", "merkle_validate_ragged_d", "broadcast_decode_leaves_d", "broadcast_decode_ragged_d")

    def __init__(self, ctx):
        self._ctx = ctx
        self.calls = dict.fromkeys(self.NAMES, 0)

    def __getattr__(self, name):
        f = getattr(self._ctx, name)
        if name not in self.NAMES:
            return f

        def counted(*a, **kw):
            self.calls[name] += 1
            return f(*a, **kw)

        return counted


def distinct_sizes_epoch(n=7, me=6):
    """One epoch at n = 7: seven proposals of distinct sizes, and a faulty Echo (a flipped value byte)
    from node 1 in instance 3."""
    values = [bytes([p + 1]) * s for p, s in enumerate([1, 40, 333, 1000, 2047, 5001, 12345])]
    rng = random.Random(5)
    events = []
    for p in range(n):
        _, leaves, tree = rm.send_shards(values[p], n)
        ev = [("input", values[p])] if p == me else [("value", p, p, tree.gen_proof(leaves[me]))]
        for i in range(n):
            if i == me:
                continue
            pr = tree.gen_proof(leaves[i])
            if p == 3 and i == 1:
                pr = dict(pr, value=pr["value"][:-1] + bytes([pr["value"][-1] ^ 4]))
            ev.append(("echo", i, p, pr))
        ev += [("ready", i, p, tree.root_hash()) for i in range(n) if i != me]
        events.append(ev)
    merged, cur = [], [0] * n
    while any(cur[p] < len(events[p]) for p in range(n)):
        p = rng.choice([q for q in range(n) if cur[q] < len(events[q])])
        merged.append(events[p][cur[p]])
        cur[p] += 1
    return merged, values


def _replay_both(hbx_ctx, events, n, me, variant="sha256"):
    from hbbft_amd.broadcast import BroadcastReplay, GpuBroadcastEngine
    from hbbft_amd.hbx import MERKLE_SHA3, MERKLE_SHA256

    mv = MERKLE_SHA3 if variant == "sha3" else MERKLE_SHA256
    out = []
    for ragged in (True, False):
        ctx = Counting(hbx_ctx)
        res = BroadcastReplay(GpuBroadcastEngine(ctx, mv, ragged=ragged), n, me).run(events)
        out.append((res, ctx.calls))
    return out


def _same(a, b):
    import dataclasses

    for f in dataclasses.fields(a):
        assert getattr(a, f.name) == getattr(b, f.name), f.name


def test_engine_ragged_distinct_sizes(hbx_ctx):
    n, me = 7, 6
    events, values = distinct_sizes_epoch(n, me)
    (rg, rc), (un, uc) = _replay_both(hbx_ctx, events, n, me)
    _same(rg, un)
    assert sorted(rg.outputs) == [(p, values[p]) for p in range(n)] and (1, "InvalidProof") in rg.faults
    node = ob.BroadcastNode(n, me).run(events)
    assert rg.outputs == node.outputs
    assert rc["merkle_validate_ragged_d"] == 1 and rc["merkle_validate_d"] == 0
    assert 1 <= rc["broadcast_decode_ragged_d"] <= 2 and rc["broadcast_decode_leaves_d"] == 0
    # the default engine: one call per length (seven value lengths, and the faulty Echo shares one)
    assert uc["merkle_validate_d"] == 7 and uc["broadcast_decode_leaves_d"] == 7
    assert uc["merkle_validate_ragged_d"] == 0 and uc["broadcast_decode_ragged_d"] == 0


@pytest.mark.parametrize("variant", ["sha256", "sha3"])
@pytest.mark.parametrize("n,me,seed,short", [(7, 6, 1, None), (13, 5, 3, None), (10, 2, 7, 8)])
def test_engine_ragged_epoch_scenarios(hbx_ctx, n, me, seed, short, variant):
    from bc_scenarios import check_against_oracle, epoch_scenario

    events, _ = epoch_scenario(n, me, seed, variant, short_leaves=short)
    (rg, rc), (un, uc) = _replay_both(hbx_ctx, events, n, me, variant)
    _same(rg, un)
    check_against_oracle(rg, ob.BroadcastNode(n, me, variant).run(events), n)
    assert rc["merkle_validate_ragged_d"] == 1 and rc["broadcast_decode_ragged_d"] <= 2
    assert uc["merkle_validate_d"] > 1 and uc["broadcast_decode_leaves_d"] > rc["broadcast_decode_ragged_d"]


@pytest.mark.parametrize("adv,sched", [("silent", "random"), ("propose", "first"), ("random", "random")])
def test_engine_ragged_simulated(hbx_ctx, adv, sched):
    from bc_scenarios import check_against_oracle, simulate

    n = 7
    value = b"Foo" if adv != "random" else b" " * 32
    received, nodes = simulate(n, adv, sched, value, seed=7000 + len(adv))
    for i, events in received.items():
        (rg, rc), (un, _) = _replay_both(hbx_ctx, events, n, i)
        _same(rg, un)
        check_against_oracle(rg, nodes[i], n)
        assert rc["merkle_validate_ragged_d"] <= 1 and rc["broadcast_decode_ragged_d"] <= 2
