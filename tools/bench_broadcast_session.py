"""Time one node's Broadcast epoch message by message: Echoes validated and stored as they arrive
(hbx_add_echoes_d), one listed decode out of the store (hbx_broadcast_decode_insts_d), beside the
whole-epoch ragged validate + decode legs on the same inputs.

    python tools/bench_broadcast_session.py [--n 128] [--steps 3] [--warmup 1] [--shape distinct|c5]

The epoch is tools/bench_broadcast_ragged.py's: N = 128 proposers, RS(44, 84), --shape c5 (128 equal
1 MiB proposals) or distinct (the 128-size ladder from 200 bytes to 1 MiB).  One sender's Echoes for
all N instances go in per add (N adds of N items); after the first N - f senders every instance is
decoded in one listed call (the last f shards reconstructed, as in the ragged decode leg).  Each add
and the decode are timed by device events around the call and by wall time including one
synchronisation.  Every item must come back STORED and every payload equal the proposal.

Prints one JSON line: ms per add (spread over the epoch's adds of all timed epochs), ms per listed
decode, the epoch total (the adds of the N - f senders the decode needs, plus the decode; and all N
adds plus the decode), and the whole-epoch validate + decode legs.  Fails without a GPU.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_broadcast_ragged import proposal_sizes, spread  # noqa: E402  (the same epoch shapes)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shape", choices=("distinct", "c5"), default="distinct")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_broadcast_session: no GPU")
    from hbbft_amd import hbx
    from hbbft_amd.broadcast import coding_counts

    lib = hbx.load_library()
    dev = torch.device("cuda", 0)
    n = args.n
    k, m = coding_counts(n)
    f = m // 2
    ctx = hbx.Context(0)
    sizes = proposal_sizes(n, args.shape)
    lens = np.array([-(-(s + 4) // k) for s in sizes], dtype=np.uint32)
    rng = np.random.default_rng(1)
    payloads = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in sizes]
    cnt = ctx.merkle_node_count(n)
    z = lambda *s, dt=torch.uint8: torch.zeros(s, dtype=dt, device=dev)  # noqa: E731
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731

    # ---- the epoch on the device: framed proposals, encoded, trees, every Echo proof ----
    off, pitch, total = hbx.ragged_layout(lens, n)
    host = np.zeros(total, dtype=np.uint8)
    for q in range(n):
        framed = np.concatenate((np.frombuffer(sizes[q].to_bytes(4, "big"), dtype=np.uint8), payloads[q]))
        rows = host[int(off[q]): int(off[q]) + n * int(pitch[q])].reshape(n, int(pitch[q]))
        data = np.zeros(k * int(lens[q]), dtype=np.uint8)
        data[: framed.size] = framed
        rows[:k, : lens[q]] = data.reshape(k, int(lens[q]))
    rg = torch.from_numpy(host).to(dev)
    nodes, roots = z(n, cnt, 32), z(n, 32)
    ctx.rs_encode_ragged_d(rg, off, lens, pitch, k, m)
    ctx.merkle_build_ragged_d(rg, off, lens, pitch, n, nodes, roots)
    req = torch.tensor([(q, i) for q in range(n) for i in range(n)], dtype=torch.int32, device=dev)
    prf = (z(n * n, 17, 32), z(n * n, 16, 32), z(n * n, dt=torch.int32), z(n * n, dt=torch.int32), z(n * n, 32))
    ctx.merkle_proofs_d(nodes, n, req, *prf)
    sync()
    index = torch.arange(n, dtype=torch.uint8, device=dev).view(n, 1)
    vals = []  # instance q's Echo values [n, 1 + len]
    for q in range(n):
        rows = rg[int(off[q]): int(off[q]) + n * int(pitch[q])].view(n, int(pitch[q]))
        vals.append(torch.cat([index, rows[:, : int(lens[q])]], dim=1).contiguous())
    root_host = roots.cpu().numpy()

    def timed_once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        sync()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3

    def timed(fn):
        dm, wm = [], []
        for step in range(args.warmup + args.steps):
            d, w = timed_once(fn)
            if step >= args.warmup:
                dm.append(d)
                wm.append(w)
        return {"device_ms": spread(dm), "wall_ms": spread(wm)}

    # ---- the whole-epoch legs: all N x N proofs in one validation, one decode wave ----
    blob = torch.cat([v.reshape(-1) for v in vals])
    val_off = np.zeros(n * n + 1, dtype=np.uint64)
    val_off[1:] = np.cumsum(np.repeat(lens.astype(np.uint64) + 1, n))
    sender_all = torch.arange(n, dtype=torch.int32, device=dev).repeat(n)
    ok = z(n * n)
    legs = {"validate": timed(lambda: ctx.merkle_validate_ragged_d(blob, val_off, *prf, sender_all, n, ok))}
    assert bool(ok.all()), "ragged validation rejected an honest proof"
    present = torch.ones((n, n), dtype=torch.uint8, device=dev)
    present[:, n - f:] = 0
    room = (k * lens.astype(np.int64) - 4 + 15) // 16 * 16
    out_off = np.concatenate(([0], np.cumsum(room)[:-1])).astype(np.uint64)
    r_out, r_len, r_st = z(int(room.sum())), z(n, dt=torch.int64), z(n, dt=torch.int32)
    leaf = nodes[:, :n].contiguous()
    work = rg.clone()
    for q in range(n):
        work[int(off[q]): int(off[q]) + n * int(pitch[q])].view(n, int(pitch[q]))[n - f:] = 0xA5
    legs["decode"] = timed(lambda: ctx.broadcast_decode_ragged_d(work, off, lens, pitch, present, roots, k, m, r_out, out_off,
                                                                 r_len, r_st, d_leaf_hash=leaf))
    assert not r_st.any(), "ragged decode failed"
    del blob, work

    # ---- message by message: one sender's Echoes of all instances per add ----
    per_sender = []
    insts = np.arange(n, dtype=np.uint32)
    s_off = np.zeros(n + 1, dtype=np.uint64)
    s_off[1:] = np.cumsum(lens.astype(np.uint64) + 1)
    for i in range(n):
        sel = torch.arange(n, device=dev) * n + i
        per_sender.append((torch.cat([vals[q][i] for q in range(n)]), tuple(a[sel].contiguous() for a in prf)))
    del vals
    st = z(n)
    d_out, d_len, d_st = z(int(room.sum())), z(n, dt=torch.int64), z(n, dt=torch.int32)
    use = np.zeros((n, n), dtype=np.uint8)
    use[:, : n - f] = 1
    add_d, add_w, dec_d, dec_w, need_d, all_d, need_w, all_w = [], [], [], [], [], [], [], []
    for step in range(args.warmup + args.steps):
        ctx.prepare_broadcast(n, k, m, int(lens.max()))
        ad, aw = [], []
        for i in range(n):
            b, p = per_sender[i]
            d, w = timed_once(lambda: ctx.add_echoes_d(b, s_off, *p, insts, np.full(n, i, dtype=np.uint32), st))
            assert bool((st == hbx.ECHO_STORED).all()), f"sender {i}: an honest Echo was not stored"
            ad.append(d)
            aw.append(w)
        dd, dw = timed_once(lambda: ctx.broadcast_decode_insts_d(insts, root_host, lens, d_out, out_off, d_len, d_st, use=use))
        assert not d_st.any(), "listed decode failed"
        if step >= args.warmup:
            add_d += ad
            add_w += aw
            dec_d.append(dd)
            dec_w.append(dw)
            need_d.append(sum(ad[: n - f]) + dd)
            need_w.append(sum(aw[: n - f]) + dw)
            all_d.append(sum(ad) + dd)
            all_w.append(sum(aw) + dw)
    out, ln = d_out.cpu().numpy(), d_len.cpu().numpy()
    assert torch.equal(d_out, r_out) and torch.equal(d_len, r_len), "listed and ragged decode differ"
    for q in range(n):
        o = int(out_off[q])
        assert ln[q] == sizes[q] and (out[o: o + sizes[q]] == payloads[q]).all(), f"payload {q}"
    ctx.close()
    legs["add"] = {"device_ms": spread(add_d), "wall_ms": spread(add_w), "items_per_add": n,
                   "mean_device_ms": round(statistics.mean(add_d), 3)}
    legs["decode_listed"] = {"device_ms": spread(dec_d), "wall_ms": spread(dec_w)}
    legs["epoch_adds_needed_plus_decode"] = {"device_ms": spread(need_d), "wall_ms": spread(need_w), "adds": n - f}
    legs["epoch_all_adds_plus_decode"] = {"device_ms": spread(all_d), "wall_ms": spread(all_w), "adds": n}
    print(json.dumps({"tool": "bench_broadcast_session", "build_id": lib.hbx_build_id().decode(), "shape": args.shape, "n": n,
                      "k": k, "m": m, "proposal_bytes": {"min": min(sizes), "max": max(sizes), "total": sum(sizes)},
                      "value_bytes_per_add": int(s_off[-1]), "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0), "legs": legs}))


if __name__ == "__main__":
    main()
