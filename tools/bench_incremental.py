"""Time incremental share verification (hbx_add_dec_shares_d, hbx_combine_decrypt_cols_d) at N = p.

    python tools/bench_incremental.py [--n 256] [--steps 20] [--warmup 2] [--sizes 1,64,256,4096]
                                      [--lib PATH] [--no-staged]

Builds bench.py's seeded N-validator epoch (own-share mode, inputs resident in HBM) and times, with
device events on the stream (warm-up, then --steps steps; median with min-max):

* small adds -- an add of `size` shares onto an established matrix (1 share; 64 and 256: one sender's
  messages to that many proposers; 4,096: 16 senders' messages), with the lanes per check and the
  check blocks it used; and the same shares decided by the matrix call under a present mask of those
  positions, the only route of a library without the add;
* staged epoch -- prepare, a matrix verification of the first 86 senders' shares, adds of the rest
  in steps of 16 senders, hbx_combine_decrypt_cols_d of all columns (plaintexts checked), against
  one hbx_decrypt_epoch_d.

--lib PATH times another build of the library, e.g. the parent commit's: the masked matrix call and
the fused epoch need no new symbol, and the add's rows are left out when the library has none.
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


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "n": len(xs)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--vlen", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,64,256,4096")
    ap.add_argument("--first", type=int, default=86, help="senders of the staged epoch's matrix verification")
    ap.add_argument("--chunk", type=int, default=16, help="senders per add of the staged epoch")
    ap.add_argument("--lib", default=None, help="path of the libhbx.so to time (default: this tree's)")
    ap.add_argument("--no-staged", action="store_true")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_incremental: no GPU")
    from hbbft_amd import hbx

    lib = hbx.load_library(args.lib) if args.lib else hbx.load_library()
    has_add = hasattr(lib, "hbx_add_dec_shares_d")
    import bench

    dev = torch.device("cuda", 0)
    n = p = args.n
    me = bench.OWN_INDEX
    ctx = hbx.Context(0)
    ep = bench.make_epoch(ctx, n, 0, p, args.vlen, 64)
    stream = torch.cuda.Stream(dev)
    eb = bench.EpochBench(ctx, ep, dev, stream, torch, 0, True)
    d_valid = torch.zeros(p * n, dtype=torch.uint8, device=dev)
    d_ct = torch.zeros(p, dtype=torch.uint8, device=dev)
    d_st = torch.zeros(p, dtype=torch.int32, device=dev)
    eb.bind_outputs(d_valid, d_ct, d_st)
    expect = np.where(ep["corrupt"], 0, 1).astype(np.uint8)
    s_ptr = stream.cuda_stream

    def timed(fn):
        torch.cuda.synchronize(dev)
        for _ in range(args.warmup):
            fn()
        evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
        for a, b in evs:
            a.record(stream)
            fn()
            b.record(stream)
        torch.cuda.synchronize(dev)
        return spread([a.elapsed_time(b) for a, b in evs])

    def items_of(senders, cols):
        """The messages of `senders` to proposers `cols`, as device bytes and host index arrays."""
        prop = np.repeat(np.asarray(cols, dtype=np.uint32), len(senders))
        snd = np.tile(np.asarray(senders, dtype=np.uint32), len(cols))
        sh = torch.from_numpy(np.ascontiguousarray(ep["shares"][prop, snd])).to(dev)
        return sh, prop, snd

    def prepare():
        ctx.prepare_ciphertexts_d(eb.d_u, eb.d_v, eb.d_off, eb.d_w, p, eb.maxv, stream=s_ptr)

    small = []
    for size in [int(s) for s in args.sizes.split(",") if s]:
        others = [i for i in range(n) if i != me]
        senders, cols = ([others[0]], list(range(min(size, p)))) if size <= p else (others[:size // p], list(range(p)))
        sh, prop, snd = items_of(senders, cols)
        mask = np.zeros((p, n), dtype=np.uint8)
        mask[prop, snd] = 1
        d_mask = torch.from_numpy(mask).to(dev)
        d_rest = torch.from_numpy(1 - mask).to(dev)
        rec = {"size": int(len(prop))}
        with torch.cuda.stream(stream):
            prepare()
            # the matrix call with a present mask of those positions: the route without the add
            rec["masked_matrix_ms"] = timed(lambda: ctx.verify_dec_shares_d(eb.d_shares, n, p, d_present=d_mask,
                                                                              stream=s_ptr))
            rec["masked_matrix_lanes"] = ctx.verify_lanes_used()
            if has_add:
                ctx.verify_dec_shares_d(eb.d_shares, n, p, d_present=d_rest, stream=s_ptr)  # everything else
                d_item_st = torch.zeros(len(prop), dtype=torch.uint8, device=dev)
                rec["add_ms"] = timed(lambda: ctx.add_dec_shares_d(sh, prop, snd, n, d_status=d_item_st, stream=s_ptr))
                rec["add_lanes"] = ctx.verify_lanes_used()
                rec["add_tiles"] = ctx.verify_tiles_used()
                assert (d_item_st.cpu().numpy() == expect[prop, snd]).all(), f"add of {size}: item statuses"
                assert (ctx.share_status(p, n) == expect).all(), f"add of {size}: matrix"
        small.append(rec)

    staged = None
    if not args.no_staged:
        staged = {"fused_epoch_ms": timed(lambda: eb.step())}
        eb.check(0)
        if has_add:
            first = np.zeros((p, n), dtype=np.uint8)
            first[:, :args.first] = 1
            d_first = torch.from_numpy(first).to(dev)
            adds = [items_of([i for i in range(lo, min(lo + args.chunk, n)) if i != me], list(range(p)))
                    for lo in range(args.first, n, args.chunk)]
            all_cols = np.arange(p, dtype=np.uint32)
            d_out = torch.zeros_like(eb.d_out)

            def staged_step():
                prepare()
                ctx.verify_dec_shares_d(eb.d_shares, n, p, d_present=d_first, stream=s_ptr)
                for sh, prop, snd in adds:
                    ctx.add_dec_shares_d(sh, prop, snd, n, stream=s_ptr)
                ctx.combine_decrypt_cols_d(eb.t, all_cols, d_out, d_status=d_st, stream=s_ptr)

            with torch.cuda.stream(stream):
                staged["staged_epoch_ms"] = timed(staged_step)
            staged["adds"] = len(adds)
            assert (ctx.share_status(p, n) == expect).all(), "staged epoch: matrix"
            assert (d_st.cpu().numpy() == 0).all(), "staged epoch: combine status"
            out = d_out.cpu().numpy()
            for j in range(p):
                assert out[eb.off[j]:eb.off[j + 1]].tobytes() == ep["msgs"][j], f"staged epoch: plaintext {j}"
    ctx.close()
    print(json.dumps({"tool": "bench_incremental", "lib": os.path.relpath(args.lib or hbx.LIB_PATH, ROOT),
                      "build_id": lib.hbx_build_id().decode(), "has_add": has_add, "n": n, "p": p, "vlen": args.vlen,
                      "steps": args.steps, "warmup": args.warmup, "device": torch.cuda.get_device_name(0),
                      "small_adds": small, "staged_epoch": staged}))


if __name__ == "__main__":
    main()
