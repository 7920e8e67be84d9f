"""Time one node's Broadcast epoch with per-instance shard lengths: the per-length loop over the
uniform entry points (what GpuBroadcastEngine does by default) against one ragged call per leg.

    python tools/bench_broadcast_ragged.py [--n 128] [--steps 10] [--warmup 2] [--shape distinct|c5]
                                           [--lib PATH]

The epoch: N = 128 proposers, RS(N - 2f, 2f) = RS(44, 84).
  --shape distinct  128 DISTINCT proposal sizes on a geometric ladder from 200 bytes to 1 MiB (ratio
                    about 1.07 per step, plus the index so that no two are equal): 24 of them are
                    below 1 KiB, half are below 14 KiB, the last is exactly 1 MiB, about 16 MB in
                    all.  Sizes that close give fewer distinct shard lengths than proposals at the
                    small end; the record states how many the per-length loop sees.
  --shape c5        128 equal 1 MiB proposals (BASELINE config C5): one uniform call per leg, so the
                    difference is the price of the descriptor indirection when nothing is ragged.
Three legs, each timed by device events around the leg and by wall time including the
synchronisations (one per engine call in the per-length loop, as the engine does; one per leg in
the ragged form):
  1. encode + Merkle build (nodes and roots) of all instances
  2. validation of all N x N Echo proofs
  3. the decode wave with the last f = 42 shards of every instance missing (leaf digests shared)
Each leg's outputs are checked (roots equal in both forms, every proof valid, payloads equal).

--lib PATH times another build of the library, e.g. one built from the parent commit; the ragged
legs are left out when that library has no ragged entry points.  Prints one JSON line; fails
without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def proposal_sizes(n: int, shape: str):
    if shape == "c5":
        return [1 << 20] * n
    lo, hi = 200.0, float(1 << 20)
    sizes = [int(round(lo * (hi / lo) ** (i / (n - 1)))) + i for i in range(n)]
    sizes[-1] = 1 << 20
    assert len(set(sizes)) == n
    return sizes


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shape", choices=("distinct", "c5"), default="distinct")
    ap.add_argument("--lib", default=None, help="path of the libhbx.so to time (default: this tree's)")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_broadcast_ragged: no GPU")
    from hbbft_amd import hbx
    from hbbft_amd.broadcast import coding_counts

    lib = hbx.load_library(args.lib) if args.lib else hbx.load_library()
    has_ragged = hasattr(lib, "hbx_rs_encode_ragged_d")
    dev = torch.device("cuda", 0)
    n = args.n
    k, m = coding_counts(n)
    f = m // 2
    ctx = hbx.Context(0)
    sizes = proposal_sizes(n, args.shape)
    lens = np.array([-(-(s + 4) // k) for s in sizes], dtype=np.uint32)
    groups = {}
    for q, L in enumerate(lens):
        groups.setdefault(int(L), []).append(q)
    groups = sorted(groups.items())
    rng = np.random.default_rng(1)
    payloads = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in sizes]
    cnt = ctx.merkle_node_count(n)
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731

    # ---- device images: one uniform tensor per shard length, and the ragged buffer ----
    off, pitch, total = hbx.ragged_layout(lens, n)
    rg = z(total)
    uni = {}
    for L, idx in groups:
        a = np.zeros((len(idx), n, L), dtype=np.uint8)
        for r, q in enumerate(idx):
            flat = a[r, :k].reshape(-1)
            flat[:4] = np.frombuffer(sizes[q].to_bytes(4, "big"), dtype=np.uint8)
            flat[4: 4 + sizes[q]] = payloads[q]
        uni[L] = torch.from_numpy(a).to(dev)
        for r, q in enumerate(idx):
            rows = rg[int(off[q]): int(off[q]) + n * int(pitch[q])].view(n, int(pitch[q]))
            rows[:k, :L] = uni[L][r, :k]
    u_nodes = {L: z(len(idx), cnt, 32) for L, idx in groups}
    u_roots = {L: z(len(idx), 32) for L, idx in groups}
    r_nodes, r_roots = z(n, cnt, 32), z(n, 32)

    def timed(fn):
        """fn(stream work + its synchronisations) -> (device ms between events around it, wall ms)."""
        dm, wm = [], []
        for step in range(args.warmup + args.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sync()
            t0 = time.perf_counter()
            e0.record()
            fn()
            e1.record()
            sync()
            t1 = time.perf_counter()
            if step >= args.warmup:
                dm.append(e0.elapsed_time(e1))
                wm.append((t1 - t0) * 1e3)
        return {"device_ms": spread(dm), "wall_ms": spread(wm)}

    # ---- leg 1: encode + build ----
    def enc_uniform():
        for L, _ in groups:
            ctx.rs_encode_d(uni[L], k, m)
            ctx.merkle_build_d(uni[L], u_nodes[L], u_roots[L])
            sync()

    def enc_ragged():
        ctx.rs_encode_ragged_d(rg, off, lens, pitch, k, m)
        ctx.merkle_build_ragged_d(rg, off, lens, pitch, n, r_nodes, r_roots)
        sync()

    legs = {"encode_build": {"per_length": timed(enc_uniform)}}
    if has_ragged:
        legs["encode_build"]["ragged"] = timed(enc_ragged)
        for L, idx in groups:
            assert torch.equal(u_roots[L], r_roots[idx]) and torch.equal(u_nodes[L], r_nodes[idx]), f"trees differ at L={L}"

    # ---- leg 2: all N x N Echo proofs (generated on the device from the uniform trees) ----
    def proofs_of(nodes, g):
        req = torch.tensor([(i, j) for i in range(g) for j in range(n)], dtype=torch.int32, device=dev)
        P = g * n
        out = (z(P, 17, 32), z(P, 16, 32), z(P, dt=torch.int32), z(P, dt=torch.int32), z(P, 32))
        ctx.merkle_proofs_d(nodes, n, req, *out)
        return out

    index = torch.arange(n, dtype=torch.uint8, device=dev)
    sender = torch.arange(n, dtype=torch.int32, device=dev)
    u_val, u_prf, u_ok = {}, {}, {}
    for L, idx in groups:
        g = len(idx)
        u_val[L] = torch.cat([index.view(1, n, 1).expand(g, n, 1), uni[L]], dim=2).reshape(g * n, 1 + L).contiguous()
        u_prf[L] = proofs_of(u_nodes[L], g) + (sender.repeat(g),)
        u_ok[L] = z(g * n)
    sync()

    def val_uniform():
        for L, _ in groups:
            ctx.merkle_validate_d(u_val[L], *u_prf[L], n, u_ok[L])
            sync()

    legs["validate"] = {"per_length": timed(val_uniform)}
    assert all(bool(v.all()) for v in u_ok.values()), "per-length validation rejected an honest proof"
    if has_ragged:
        # proofs in instance order: proof q * n + i is instance q's leaf i
        where = {q: (L, r) for L, idx in groups for r, q in enumerate(idx)}
        blob = torch.cat([u_val[where[q][0]][where[q][1] * n: (where[q][1] + 1) * n].reshape(-1) for q in range(n)])
        r_prf = tuple(torch.cat([u_prf[where[q][0]][a][where[q][1] * n: (where[q][1] + 1) * n] for q in range(n)])
                      for a in range(6))
        val_off = np.zeros(n * n + 1, dtype=np.uint64)
        val_off[1:] = np.cumsum(np.repeat(lens.astype(np.uint64) + 1, n))
        r_ok = z(n * n)

        def val_ragged():
            ctx.merkle_validate_ragged_d(blob, val_off, *r_prf, n, r_ok)
            sync()

        legs["validate"]["ragged"] = timed(val_ragged)
        assert bool(r_ok.all()), "ragged validation rejected an honest proof"

    # ---- leg 3: decode with the last f shards missing ----
    present = torch.ones((n, n), dtype=torch.uint8, device=dev)
    present[:, n - f:] = 0
    u_in = {}
    for L, idx in groups:
        g = len(idx)
        u_in[L] = (present[:g].contiguous(), u_nodes[L][:, :n].contiguous(), u_roots[L], z(g, max(k * L, 4)),
                   z(g, dt=torch.int64), z(g, dt=torch.int32))
        uni[L][:, n - f:] = 0xA5

    def dec_uniform():
        for L, _ in groups:
            p, lh, root, out, ln, st = u_in[L]
            ctx.broadcast_decode_leaves_d(uni[L], p, lh, root, k, m, out, ln, st)
            sync()

    legs["decode"] = {"per_length": timed(dec_uniform)}
    for L, idx in groups:
        _, _, _, out, ln, st = u_in[L]
        out, ln = out.cpu().numpy(), ln.cpu().numpy()
        assert not st.any(), f"per-length decode failed at L={L}"
        for r, q in enumerate(idx):
            assert ln[r] == sizes[q] and (out[r, : sizes[q]] == payloads[q]).all(), f"payload {q}"
    if has_ragged:
        room = (k * lens.astype(np.int64) - 4 + 15) // 16 * 16
        out_off = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.uint64)
        r_out, r_len, r_st = z(int(room.sum())), z(n, dt=torch.int64), z(n, dt=torch.int32)
        r_leaf = r_nodes[:, :n].contiguous()
        for q in range(n):
            rows = rg[int(off[q]): int(off[q]) + n * int(pitch[q])].view(n, int(pitch[q]))
            rows[n - f:] = 0xA5

        def dec_ragged():
            ctx.broadcast_decode_ragged_d(rg, off, lens, pitch, present, r_roots, k, m, r_out, out_off, r_len, r_st,
                                          d_leaf_hash=r_leaf)
            sync()

        legs["decode"]["ragged"] = timed(dec_ragged)
        out, ln = r_out.cpu().numpy(), r_len.cpu().numpy()
        assert not r_st.any(), "ragged decode failed"
        for q in range(n):
            o = int(out_off[q])
            assert ln[q] == sizes[q] and (out[o: o + sizes[q]] == payloads[q]).all(), f"ragged payload {q}"
    ctx.close()
    print(json.dumps({"tool": "bench_broadcast_ragged", "lib": os.path.relpath(args.lib or hbx.LIB_PATH, ROOT),
                      "build_id": lib.hbx_build_id().decode(), "has_ragged": has_ragged, "shape": args.shape, "n": n,
                      "k": k, "m": m, "proposal_bytes": {"min": min(sizes), "max": max(sizes), "total": sum(sizes),
                                                         "below_1KiB": sum(s < 1024 for s in sizes)},
                      "distinct_shard_lengths": len(groups), "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0), "legs": legs}))


if __name__ == "__main__":
    main()
