"""Time the coin's incremental calls (hbx_add_sig_shares_d, hbx_combine_signatures_insts_d) at N = 128,
I = 256 instances (bench.py's C4 shape).

    python tools/bench_coin_incremental.py [--steps 20] [--warmup 2] [--sizes 1,256,4096] [--lists 1,16,256]
                                           [--first 43] [--chunk 16] [--lib PATH] [--label NAME]

Builds C4's seeded round (1 in 64 shares replaced by another instance's share of the same signer,
inputs resident in HBM) and times, with device events on the stream (warm-up, then --steps steps;
median with min-max):

* adds -- an add of `size` shares onto an established matrix (the first --first senders of every
  instance): 1 share; 256: one sender's shares of every instance; 4,096: 16 senders'.  With the
  lanes per check and the check blocks it used.  Against the same shares decided by the matrix call
  under a present mask of those positions, the only route of a library without the add, and against
  that call over the held shares and the new ones together (which such a library needs before a
  combine, since its matrix call replaces the matrix);
* listed combines -- hbx_combine_signatures_insts_d of 1 / 16 / 256 instances against
  hbx_combine_signatures_d of all of them;
* staged round -- a matrix call of the first --first senders, adds of --chunk senders each, the listed
  combine of every instance (signatures checked against the one-call round's); beside it the round in
  one matrix call and one combine, and the staged round as a library without the add must run it (a
  matrix call over everything delivered so far at every stage).

--lib PATH times another build of the library, e.g. the parent commit's: the rows that need a new
symbol are left out.  Prints one JSON line; fails without a GPU.
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
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--inst", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--lists", default="1,16,256")
    ap.add_argument("--first", type=int, default=43, help="senders of the established matrix / the staged round's matrix call")
    ap.add_argument("--chunk", type=int, default=16, help="senders per add of the staged round")
    ap.add_argument("--lib", default=None, help="path of the libhbx.so to time (default: this tree's)")
    ap.add_argument("--label", default=None, help="copied into the output line (e.g. parent/r1)")
    args = ap.parse_args(argv)

    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench_coin_incremental: no GPU")
    from hbbft_amd import hbx, netinfo

    lib = hbx.load_library(args.lib) if args.lib else hbx.load_library()
    has_add = hasattr(lib, "hbx_add_sig_shares_d")
    dev = torch.device("cuda", 0)
    n, inst = args.n, args.inst
    ctx = hbx.Context(0)
    sks, sk_shares, master_sk = netinfo.generate_keys(n)
    t = sks.threshold + 1
    pk = ctx.public_keys(sk_shares)
    master_pk = ctx.public_keys(master_sk)[0].tobytes()
    assert (ctx.set_pk_shares([r.tobytes() for r in pk]) == 0).all()
    inv_id = "[" + ", ".join(str(b) for b in master_pk) + "]"
    nonces = [f"Nonce for Honey Badger {inv_id}@{s}:2:{j}".encode() for s in range(inst // n + 1) for j in range(n)][:inst]
    ctx.prepare_nonces(nonces)
    sigs = ctx.sign(sk_shares)  # (inst, n, 96)
    rng = np.random.default_rng(0x68626278_00000005)
    corrupt = rng.integers(0, 64, size=(inst, n)) == 0
    bad = sigs.copy()
    ii = np.nonzero(corrupt)
    bad[ii[0], ii[1]] = sigs[(ii[0] + 1) % inst, ii[1]]
    expect = np.where(corrupt, 0, 1).astype(np.uint8)
    stream = torch.cuda.Stream(dev)
    s_ptr = stream.cuda_stream
    d_bad = torch.from_numpy(bad).to(dev)
    d_vst = torch.zeros((inst, n), dtype=torch.uint8, device=dev)

    def outs():
        return (torch.zeros((inst, 96), dtype=torch.uint8, device=dev), torch.zeros(inst, dtype=torch.int32, device=dev),
                torch.zeros(inst, dtype=torch.uint8, device=dev), torch.zeros(inst, dtype=torch.uint8, device=dev))

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

    def mask_of(senders, insts=None):
        m = np.zeros((inst, n), dtype=np.uint8)
        rows = np.arange(inst) if insts is None else np.asarray(insts)
        m[np.ix_(rows, np.asarray(senders))] = 1
        return m

    def items_of(senders, insts):
        """The shares of `senders` in `insts`, as device bytes and host index arrays."""
        q = np.repeat(np.asarray(insts, dtype=np.uint32), len(senders))
        snd = np.tile(np.asarray(senders, dtype=np.uint32), len(insts))
        return torch.from_numpy(np.ascontiguousarray(bad[q, snd])).to(dev), q, snd

    held = list(range(args.first))
    d_held = torch.from_numpy(mask_of(held)).to(dev)
    adds = []
    with torch.cuda.stream(stream):
        for size in [int(s) for s in args.sizes.split(",") if s]:
            senders = list(range(args.first, args.first + max(size // inst, 1)))
            insts = list(range(min(size, inst)))
            sh, q, snd = items_of(senders, insts)
            new = mask_of(senders, insts)
            d_new = torch.from_numpy(new).to(dev)
            d_both = torch.from_numpy(np.maximum(new, mask_of(held))).to(dev)
            rec = {"size": int(len(q))}
            # the matrix call with a present mask of those positions: the route without the add
            rec["masked_matrix_ms"] = timed(lambda: ctx.verify_sig_shares_d(d_bad, d_new, d_vst, stream=s_ptr))
            rec["masked_matrix_lanes"] = ctx.coin_lanes_used()
            assert (d_vst.cpu().numpy()[new == 1] == expect[new == 1]).all(), f"masked matrix call of {size}"
            rec["held_and_new_matrix_ms"] = timed(lambda: ctx.verify_sig_shares_d(d_bad, d_both, d_vst, stream=s_ptr))
            if has_add:
                ctx.verify_sig_shares_d(d_bad, d_held, None, stream=s_ptr)  # the established matrix
                d_item_st = torch.zeros(len(q), dtype=torch.uint8, device=dev)
                rec["add_ms"] = timed(lambda: ctx.add_sig_shares_d(sh, q, snd, n, d_status=d_item_st, stream=s_ptr))
                rec["add_lanes"] = ctx.coin_lanes_used()
                rec["add_tiles"] = ctx.coin_tiles_used()
                assert (d_item_st.cpu().numpy() == expect[q, snd]).all(), f"add of {size}: item statuses"
                want = np.where(np.maximum(new, mask_of(held)) == 1, expect, 2)
                assert (ctx.sig_share_status(inst, n) == want).all(), f"add of {size}: matrix"
            adds.append(rec)

        # listed combines against the full combine, over the whole round's matrix
        ctx.verify_sig_shares_d(d_bad, None, d_vst, stream=s_ptr)
        ref = outs()
        combines = {"full_ms": timed(lambda: ctx.combine_signatures_d(master_pk, t, None, *ref, stream=s_ptr))}
        ref_np = [x.cpu().numpy() for x in ref]
        assert (ref_np[1] == 0).all() and ref_np[2].all(), "combine / master verification"
        if has_add:
            combines["listed"] = []
            for k in [int(s) for s in args.lists.split(",") if s]:
                listed = np.arange(inst - k, inst, dtype=np.uint32)
                got = outs()
                ms = timed(lambda: ctx.combine_signatures_insts_d(master_pk, t, listed, None, *got, stream=s_ptr))
                for g, r in zip(got, ref_np):
                    assert (g.cpu().numpy()[listed] == r[listed]).all(), f"listed combine of {k}"
                combines["listed"].append({"instances": k, "ms": ms})

        # the staged round
        def one_call():
            ctx.verify_sig_shares_d(d_bad, None, None, stream=s_ptr)
            ctx.combine_signatures_d(master_pk, t, None, *ref, stream=s_ptr)

        staged = {"one_call_round_ms": timed(one_call)}
        stages = [list(range(lo, min(lo + args.chunk, n))) for lo in range(args.first, n, args.chunk)]
        cum, d_cum = mask_of(held), []
        for senders in stages:
            cum = np.maximum(cum, mask_of(senders))
            d_cum.append(torch.from_numpy(cum).to(dev))

        def staged_by_matrix():
            ctx.verify_sig_shares_d(d_bad, d_held, None, stream=s_ptr)
            for m in d_cum:
                ctx.verify_sig_shares_d(d_bad, m, None, stream=s_ptr)
            ctx.combine_signatures_d(master_pk, t, None, *ref, stream=s_ptr)

        staged["staged_by_matrix_calls_ms"] = timed(staged_by_matrix)
        staged["stages"] = len(stages)
        if has_add:
            stage_items = [items_of(senders, list(range(inst))) for senders in stages]
            every = np.arange(inst, dtype=np.uint32)
            got = outs()

            def staged_step():
                ctx.verify_sig_shares_d(d_bad, d_held, None, stream=s_ptr)
                for sh, q, snd in stage_items:
                    ctx.add_sig_shares_d(sh, q, snd, n, stream=s_ptr)
                ctx.combine_signatures_insts_d(master_pk, t, every, None, *got, stream=s_ptr)

            staged["staged_round_ms"] = timed(staged_step)
            assert (ctx.sig_share_status(inst, n) == expect).all(), "staged round: matrix"
            for g, r in zip(got, ref_np):
                assert (g.cpu().numpy() == r).all(), "staged round: signatures"
    ctx.close()
    print(json.dumps({"tool": "bench_coin_incremental", "label": args.label,
                      "lib": os.path.relpath(args.lib or hbx.LIB_PATH, ROOT), "build_id": lib.hbx_build_id().decode(),
                      "has_add": has_add, "n": n, "instances": inst, "t": t, "first": args.first, "steps": args.steps,
                      "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "adds": adds, "combines": combines,
                      "staged_round": staged}))


if __name__ == "__main__":
    main()
