"""Reader of the per-message SyncKeyGen fixtures skg_n4 / skg_n7 (tests/golden/make_skg_golden.py
pack_era): rebuilds the (kind, sender, body) messages with points as bytes."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PART, ACK = 0, 1


def load_era(name):
    d = dict(np.load(os.path.join(GOLDEN, f"{name}.npz"), allow_pickle=False))
    n = int(d["n"])

    def cts(u, v, off, w, lo, hi):
        return [(u[k].tobytes(), v[int(off[k]):int(off[k + 1])].tobytes(), w[k].tobytes()) for k in range(lo, hi)]

    pu, pw = d["part_u"].reshape(-1, 48), d["part_w"].reshape(-1, 96)
    msgs = []
    for kind, sender, ref in zip(d["msg_kind"], d["msg_sender"], d["msg_ref"]):
        s = None if sender < 0 else int(sender)
        ref = int(ref)
        if kind == PART:
            commit = [c.tobytes() for c in d["part_commit"][ref]]
            msgs.append((PART, s, (commit, cts(pu, d["part_v"], d["part_off"], pw, ref * n, ref * n + n))))
        else:
            lo, hi = int(d["ack_start"][ref]), int(d["ack_start"][ref + 1])
            msgs.append((ACK, s, (int(d["ack_proposer"][ref]), cts(d["ack_u"], d["ack_v"], d["ack_off"], d["ack_w"], lo, hi))))
    part_msgs = [k for k, m in enumerate(msgs) if m[0] == PART]
    # randomness of, and the expected Ack for, the Part at each message index
    d["ack_r_by_msg"] = {k: d["ack_r"][a] for a, k in enumerate(part_msgs)}
    d["exp_ack_by_msg"] = {
        k: [(d["exp_ack_u"][a, i].tobytes(), d["exp_ack_v"][a, i].tobytes(), d["exp_ack_w"][a, i].tobytes())
            for i in range(n)]
        for a, k in enumerate(part_msgs)}
    d["msgs"] = msgs
    return d
