"""Time the batched decryption-share verification (hbx_set_batch_verify) against the per-share path.

    python tools/bench_batch_verify.py [--n 256] [--steps 20] [--warmup 2] [--bad 0,1,16,256]
                                       [--lib PATH] [--no-own-share] [--repeat R]

Builds a seeded N-validator epoch (p = N proposers) from the producer-side calls (hbx_public_keys,
hbx_encrypt, hbx_decrypt_shares), as bench.py does, with every share honest; a "bad column" then
gets one sender's share overwritten by another sender's share of the same ciphertext (a byte copy).
Each configuration times hbx_decrypt_epoch_d with device events on the stream (warm-up, then
--steps steps), checks the outputs of the last step (validity matrix, ciphertext statuses,
plaintexts), and then repeats a few steps with hbx_set_timing on for the per-kernel times
(hbx_kernel_time).  Configurations: per-share mode with 0 and N bad columns, and batched mode with
each --bad count.  In batched mode with 0 bad columns the "verify_shares" time is what the per-share
launch costs when every column is masked.

--lib PATH times another build of the library, e.g. one built from the parent commit: per-share
mode needs no new symbol, and the batched configurations are left out when the library has none.
Prints one JSON line; fails without a GPU.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = bytes(range(32))  # a benchmark may use a fixed seed; a node may not
KERNELS = ("prepare_ct", "prepare_lines", "ct_checks", "batch_msm", "batch_check", "verify_shares", "combine")


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3),
            "mean": round(statistics.fmean(xs), 3), "n": len(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--vlen", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ksteps", type=int, default=3, help="steps of the per-kernel timing pass")
    ap.add_argument("--bad", default="0,1,16,256", help="bad-column counts of the batched configurations")
    ap.add_argument("--repeat", type=int, default=1, help="repeat every configuration this many times (spread)")
    ap.add_argument("--lib", default=None, help="path of the libhbx.so to time (default: this tree's)")
    ap.add_argument("--no-own-share", action="store_true")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_batch_verify: no GPU")
    from hbbft_amd import hbx

    lib = hbx.load_library(args.lib) if args.lib else hbx.load_library()
    has_batch = hasattr(lib, "hbx_set_batch_verify")
    import bench

    dev = torch.device("cuda", 0)
    n = p = args.n
    own = not args.no_own_share
    ctx = hbx.Context(0)
    ep = bench.make_epoch(ctx, n, 0, p, args.vlen, 1 << 62)  # no corrupted share
    assert not ep["corrupt"].any()
    stream = torch.cuda.Stream(dev)
    clean = ep["shares"].copy()
    eb = bench.EpochBench(ctx, ep, dev, stream, torch, 0, own)
    d_valid = torch.zeros(p * n, dtype=torch.uint8, device=dev)
    d_ct = torch.zeros(p, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(p, dtype=torch.int32, device=dev)
    eb.bind_outputs(d_valid, d_ct, d_st)
    kernels = [k for k in KERNELS if k in hbx.KERNELS and (has_batch or not k.startswith("batch_"))]

    def run(mode, bad_cols):
        sh = clean.copy()
        expect = np.ones((p, n), dtype=bool)
        for j in range(bad_cols):  # one bad share in each of the first bad_cols columns
            a, b = 1 + (j % (n - 2)), 1 + ((j + 1) % (n - 2))
            sh[j, b] = sh[j, a]
            expect[j, b] = False
        eb.d_shares = torch.from_numpy(sh).to(dev)
        if has_batch:
            ctx.set_batch_verify(SEED if mode == "batched" else None)
        ctx.set_timing(False)
        torch.cuda.synchronize(dev)
        for _ in range(args.warmup):
            eb.step()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for e in evs:
            eb.step(e)
        torch.cuda.synchronize(dev)
        ms = [a.elapsed_time(b) for a, b in evs]
        valid = d_valid.cpu().numpy().reshape(p, n) == 1
        assert (valid == expect).all(), f"{mode}/{bad_cols}: validity differs at {int((valid != expect).sum())} shares"
        assert (d_ct.cpu().numpy() == 1).all() and (d_st.cpu().numpy() == 0).all(), f"{mode}/{bad_cols}: statuses"
        out = eb.d_out.cpu().numpy()
        for j in range(p):
            assert out[eb.off[j]:eb.off[j + 1]].tobytes() == ep["msgs"][j], f"{mode}/{bad_cols}: plaintext {j}"
        rec = {"mode": mode, "bad_cols": bad_cols, "epoch_ms": spread(ms), "lanes": ctx.verify_lanes_used()}
        if has_batch:
            rec["cols"] = dict(zip(("batched", "fallback", "skipped"), ctx.batch_stats()))
        ctx.set_timing(True)
        for _ in range(args.ksteps):
            eb.step()
        torch.cuda.synchronize(dev)
        rec["kernels_ms"] = {}
        for k in kernels:
            tot, cnt = ctx.kernel_time(k)
            rec["kernels_ms"][k] = round(tot / args.ksteps, 3) if cnt else 0.0
        ctx.set_timing(False)
        return rec

    runs = []
    configs = [("per_share", 0), ("per_share", min(p, n))]
    if has_batch:
        configs += [("batched", min(int(b), p)) for b in args.bad.split(",") if b != ""]
    try:
        for _ in range(args.repeat):
            for mode, bad in configs:
                runs.append(run(mode, bad))
    finally:
        if has_batch:
            ctx.set_batch_verify(None)
        ctx.close()
    print(json.dumps({"tool": "bench_batch_verify", "lib": os.path.relpath(args.lib or hbx.LIB_PATH, ROOT),
                      "build_id": lib.hbx_build_id().decode(), "has_batch": has_batch, "n": n, "p": p,
                      "vlen": args.vlen, "own_share": own, "steps": args.steps, "warmup": args.warmup,
                      "device": torch.cuda.get_device_name(0), "runs": runs}))


if __name__ == "__main__":
    main()
