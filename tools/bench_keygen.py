"""One node's SyncKeyGen era (reference src/sync_key_gen.rs) through the batch calls, stage by stage.

    python tools/bench_keygen.py [--n 64] [--try-256] [--limit-s 240] [--ct-check wide|pair|both]
                                 [--sig-path keyed|legacy|both] [--sig-msg-len 64] [--sigs-only]

Synthetic seeded data: N dealers' symmetric bivariate polynomials of degree t = (N - 1) / 3, their N
Parts (this node's row of each, encrypted to its key) and the N^2 Acks addressed to this node (one
value per (part, sender)), all built with the engine's own producer calls (hbx_bivar_poly_rows,
hbx_fr_poly_eval, hbx_public_keys, hbx_encrypt_to).  Timed stages are what ONE node does in an era
(host wall clock of the blocking host-pointer calls, transfers included):

  dealer_rows / dealer_commit / dealer_encrypt   this node's own Part (sync_key_gen.rs:290-298)
  part_decrypt      SecretKey::decrypt of our row of every Part (:326)
  part_commit_row   commit.row(our_idx + 1) of every Part (:313)
  part_row_commit   row.commitment() of every decrypted row (:334), compared on the host
  ack_values        row.evaluate(idx + 1) for every node and Part (:341)
  ack_encrypt       the N values of each of our N Acks (:345), N^2 encryptions to N keys
  ack_decrypt       SecretKey::decrypt of our value of every Ack (:444), N^2 ciphertexts; with the
                    split between the chunked Ciphertext::verify kernels and k_sk_decrypt
  ack_check         commit.evaluate(our_idx + 1, sender_idx + 1) == g1 * val (:449)
  generate          SyncKeyGen::generate (:396-409)
  pk_shares         public_key_share(i) for every node (messaging.rs:251-254)

Prints one JSON line.  Results are checked by size-independent properties: every plaintext
decrypts to what was encrypted, every Ack value passes its commitment check, and the generated
share's public key equals this node's public key share.  --try-256 attempts N = 256 afterwards under
the script's own time limit (--limit-s, counted from the start of the script): it is not started when
the measured N = 64 pass predicts it will not fit (the N^2 stages scale by 16), and once started the
limit is checked before every input-building step and every stage; a pass that runs out reports the
stages it finished and "stopped_before".  A stage already running is not interrupted.

--ct-check chooses how hbx_sk_decrypt runs Ciphertext::verify (hbx_set_ct_check): `wide` (default, the
wide executor over prepared line tables), `pair` (one lane pair per ciphertext) or `both`.  Every era
carries a "ct_check" field.  With `both` the era runs once per mode at each size and the modes
alternate (wide, pair at N = 64, then wide, pair at N = 256): "era" / "era_256" are the wide passes,
"era_pair" / "era_256_pair" the pair passes, and the N = 256 prediction counts both passes.

--sig-path adds the signature layer Dynamic HoneyBadger wraps around those messages
(dynamic_honey_badger.rs:254-272, :363), in "sigs" / "sigs_256":
  kg_sign         SecretKey::sign of this node's N + 1 messages (hbx_sign_msgs)
  kg_sig_verify   PublicKey::verify of the era's N Parts + N^2 Acks over the table of N keys
`keyed` is hbx_verify_sigs_keyed; `legacy` feeds the same items to hbx_verify_sigs with the keys
gathered per item (the only path before the keyed call: the baseline); `both` alternates them, keyed
first, two rounds in one process.  Every pass records wall time and the hbx_kernel_time sums of
hash_nonces, decode_sigs and verify_sig (hbx_verify_sigs times only its check kernel: its hash, decode
and line preparation show in its wall time alone).  Messages are --sig-msg-len seeded bytes each; a
real Ack is N ciphertexts, about 190 N bytes.  The statuses must all be VALID and equal across paths.
A pass that fails (device memory) or does not fit --limit-s is recorded as such.  --sigs-only skips the eras.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _scalars(rng, *shape):
    """Seeded canonical Fr values as uint8[..., 32] big-endian (top byte < 0x73: below r)."""
    a = rng.integers(0, 256, size=shape + (32,), dtype=np.uint8)
    a[..., 0] %= 0x73
    return a


MODE_NAMES = {0: "wide", 1: "pair"}  # hbx.CT_CHECK_WIDE / hbx.CT_CHECK_PAIR


class OutOfTime(Exception):
    pass


def era(ctx, n: int, seed: int = 1, deadline: float = None, ct_check: int = 0):
    ctx.set_ct_check(ct_check)
    t = (n - 1) // 3
    M = (t + 1) * (t + 2) // 2
    me = n // 3
    rng = np.random.default_rng(seed)
    times = {}

    def check(name):
        if deadline is not None and time.perf_counter() > deadline:
            raise OutOfTime({"n": n, "ct_check": MODE_NAMES[ct_check], "stopped_before": name, "stage_ms": times})

    def timed(name, fn, *args):
        check(name)
        t0 = time.perf_counter()
        out = fn(*args)
        times[name] = round((time.perf_counter() - t0) * 1e3, 3)
        return out

    # ---- inputs (untimed): node keys, every dealer's polynomial, commitment and rows
    sk_nodes = _scalars(rng, n)
    pk_nodes = ctx.public_keys(sk_nodes)
    coeffs = _scalars(rng, n, M)
    commits = ctx.public_keys(coeffs.reshape(n * M, 32)).reshape(n, M, 48)
    check("inputs: rows")
    rows_all = [ctx.bivar_poly_rows(coeffs[q], t, n) for q in range(n)]  # [q][x - 1][t + 1][32]
    my_rows = [rows_all[q][me].tobytes() for q in range(n)]
    part_cts = ctx.encrypt_to(np.repeat(pk_nodes[me][None, :], n, axis=0), my_rows, _scalars(rng, n))
    check("inputs: ack values")
    # value of sender s about part q for us: row_{q,s}.evaluate(me + 1)
    vals_to_me = np.stack([ctx.fr_poly_eval(rows_all[q], n)[:, me, :] for q in range(n)])  # [q][s][32]
    check("inputs: ack ciphertexts")
    ack_cts = ctx.encrypt_to(np.repeat(pk_nodes[me][None, :], n * n, axis=0),
                             [vals_to_me[q, s].tobytes() for q in range(n) for s in range(n)], _scalars(rng, n * n))

    # ---- this node's own Part
    own_rows = timed("dealer_rows", ctx.bivar_poly_rows, coeffs[me], t, n)
    own_commit = timed("dealer_commit", ctx.public_keys, coeffs[me])
    timed("dealer_encrypt", ctx.encrypt_to, pk_nodes, [own_rows[i].tobytes() for i in range(n)], _scalars(rng, n))
    assert (own_commit == commits[me]).all()

    # ---- handle_part over the N Parts
    sk_me = sk_nodes[me].tobytes()
    rows_plain, st = timed("part_decrypt", ctx.sk_decrypt, sk_me, part_cts)
    assert (st == 1).all() and rows_plain == my_rows
    commit_rows, cst = timed("part_commit_row", ctx.bivar_rows, commits, t, me + 1)
    rows32 = np.frombuffer(b"".join(rows_plain), dtype=np.uint8).reshape(n, t + 1, 32)
    row_commit = timed("part_row_commit", ctx.public_keys, rows32.reshape(n * (t + 1), 32))
    assert (cst == 1).all() and (row_commit.reshape(n, t + 1, 48) == commit_rows).all()
    vals = timed("ack_values", ctx.fr_poly_eval, rows32, n)  # [q][idx][32]
    timed("ack_encrypt", ctx.encrypt_to, np.tile(pk_nodes, (n, 1)),
          [vals[q, i].tobytes() for q in range(n) for i in range(n)], _scalars(rng, n * n))

    # ---- handle_ack over the N^2 Acks addressed to us
    ctx.set_timing(True)
    vals_plain, st = timed("ack_decrypt", ctx.sk_decrypt, sk_me, ack_cts)
    split = {k: ctx.kernel_time(k) for k in ("prepare_ct", "prepare_lines", "ct_checks", "sk_decrypt")}
    ctx.set_timing(False)
    assert (st == 1).all()
    got = np.frombuffer(b"".join(vals_plain), dtype=np.uint8).reshape(n, n, 32)
    assert (got == vals_to_me).all()
    proposer = np.repeat(np.arange(n, dtype=np.uint32), n)
    y = np.tile(np.arange(1, n + 1, dtype=np.uint64), n)
    ok = timed("ack_check", ctx.bivar_check_acks, commits, t, me + 1, proposer, y, got.reshape(n * n, 32))
    assert (ok == 1).all()

    # ---- generate and the new key set
    cnt = np.full(n, t + 1, dtype=np.uint32)
    ys = np.tile(np.arange(1, t + 2, dtype=np.uint64), (n, 1))
    pkc, sk_share, _ = timed("generate", ctx.keygen_generate, commits, t, np.ones(n, dtype=np.uint8), cnt, ys,
                             np.ascontiguousarray(got[:, :t + 1, :]))
    pk_shares = timed("pk_shares", ctx.pk_shares_from_commit, pkc, n)
    mine = ctx.public_keys(np.frombuffer(sk_share, dtype=np.uint8).reshape(1, 32))
    assert (mine[0] == pk_shares[me]).all()

    verify_ms = sum(split[k][0] for k in ("prepare_ct", "prepare_lines", "ct_checks"))
    assert ctx.ct_check_used() == ct_check
    return {"n": n, "t": t, "parts": n, "acks": n * n, "ct_check": MODE_NAMES[ct_check], "stage_ms": times,
            "era_ms": round(sum(times.values()), 3),
            "ack_decrypt_kernels_ms": {"ciphertext_verify": round(verify_ms, 3),
                                       "prepare_ct": round(split["prepare_ct"][0], 3),
                                       "prepare_lines": round(split["prepare_lines"][0], 3),
                                       "ct_checks": round(split["ct_checks"][0], 3),
                                       "k_sk_decrypt": round(split["sk_decrypt"][0], 3)}}


SIG_KERNELS = ("hash_nonces", "decode_sigs", "verify_sig")


def sig_stages(ctx, n: int, msg_len: int, paths, rounds: int = 2, seed: int = 2, deadline: float = None):
    """The era's signatures: N + 1 signed by this node, N + N^2 verified, `rounds` times per path."""
    from hbbft_amd.hbx import HbxError

    rng = np.random.default_rng(seed)
    count = n + n * n
    sk_nodes = _scalars(rng, n)
    sk_nodes[:, 31] |= 1  # not zero
    pk_nodes = ctx.public_keys(sk_nodes)
    # item k is signed by node k % n: every node's Part, then its N Acks; N + 1 messages per node
    blob = rng.integers(0, 256, size=count * msg_len, dtype=np.uint8).tobytes()
    msgs = [blob[k * msg_len:(k + 1) * msg_len] for k in range(count)]
    key_idx = (np.arange(count) % n).astype(np.uint32)
    sig = np.zeros((count, 96), dtype=np.uint8)
    out = {"n": n, "items": count, "keys": n, "msg_len": msg_len, "passes": []}
    t0 = time.perf_counter()
    for i in range(n):  # untimed but for node 0: the other nodes' signatures are inputs
        mine = np.flatnonzero(key_idx == i)
        t1 = time.perf_counter()
        sig[mine] = ctx.sign_msgs(sk_nodes[i].tobytes(), [msgs[k] for k in mine])
        if i == 0:
            out["kg_sign_ms"] = round((time.perf_counter() - t1) * 1e3, 3)
            out["kg_sign_msgs"] = len(mine)
    out["inputs_s"] = round(time.perf_counter() - t0, 3)
    pk_items = None
    first = None
    for r in range(rounds):
        for path in paths:
            rec = {"path": path, "round": r}
            out["passes"].append(rec)
            if deadline is not None and time.perf_counter() > deadline:
                rec["skipped"] = "time limit"
                continue
            if path == "legacy" and pk_items is None:
                pk_items = np.ascontiguousarray(pk_nodes[key_idx])
            ctx.set_timing(True)
            t1 = time.perf_counter()
            try:
                if path == "keyed":
                    st, _ = ctx.verify_sigs_keyed(pk_nodes, key_idx, msgs, sig)
                else:
                    st = ctx.verify_sigs(pk_items, msgs, sig)
            except HbxError as e:
                ctx.set_timing(False)
                rec["failed"] = str(e)
                continue
            rec["wall_ms"] = round((time.perf_counter() - t1) * 1e3, 3)
            kt = {k: ctx.kernel_time(k) for k in SIG_KERNELS}
            ctx.set_timing(False)
            rec["kernel_ms"] = {k: round(v[0], 3) for k, v in kt.items()}
            rec["kernel_sum_ms"] = round(sum(v[0] for v in kt.values()), 3)
            assert (st == 1).all(), f"{path}: {int((st != 1).sum())} items not VALID"
            first = st if first is None else first
            assert (st == first).all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--try-256", action="store_true")
    ap.add_argument("--limit-s", type=float, default=240.0)
    ap.add_argument("--ct-check", choices=("wide", "pair", "both"), default="wide")
    ap.add_argument("--sig-path", choices=("keyed", "legacy", "both"), default=None)
    ap.add_argument("--sig-msg-len", type=int, default=64)
    ap.add_argument("--sigs-only", action="store_true")
    args = ap.parse_args()
    from hbbft_amd.hbx import Context, build_info

    modes = {"wide": [0], "pair": [1], "both": [0, 1]}[args.ct_check]

    def key(base, mode):  # with `both`, the pair pass goes beside the wide one
        return base if mode == modes[0] else base + "_" + MODE_NAMES[mode]

    t0 = time.perf_counter()
    with Context(0) as ctx:
        try:
            out = {"metric": "keygen_era", "lib": build_info()}
            sig_paths = {None: [], "keyed": ["keyed"], "legacy": ["legacy"], "both": ["keyed", "legacy"]}[args.sig_path]
            if sig_paths:
                sig_stages(ctx, 4, args.sig_msg_len, sig_paths, rounds=1)  # warm-up
                out["sigs"] = sig_stages(ctx, args.n, args.sig_msg_len, sig_paths)
                if args.try_256:
                    out["sigs_256"] = sig_stages(ctx, 256, args.sig_msg_len, sig_paths, deadline=t0 + args.limit_s)
            if args.sigs_only:
                modes = []
            for mode in modes:
                era(ctx, 4, ct_check=mode)  # warm-up: module load, first allocations
            for mode in modes:
                out[key("era", mode)] = era(ctx, args.n, ct_check=mode)
            if args.try_256 and modes:
                spent = time.perf_counter() - t0
                # the whole N = 64 pass (inputs included, every mode) scaled by the N^2 stages' factor
                predicted = spent * (256 / args.n) ** 2
                for mode in modes:
                    if predicted <= args.limit_s:
                        try:
                            out[key("era_256", mode)] = era(ctx, 256, deadline=t0 + args.limit_s, ct_check=mode)
                        except OutOfTime as e:
                            ctx.set_timing(False)
                            out[key("era_256", mode)] = e.args[0]
                    else:
                        out[key("era_256", mode)] = {"skipped": f"predicted {predicted:.0f} s > limit {args.limit_s:.0f} s"}
        finally:
            ctx.set_ct_check(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
