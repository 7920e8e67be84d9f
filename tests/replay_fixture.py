"""Readers of the committed epoch-replay fixtures (tests/golden/hb_replay_{a,b,c}.npz) that need
nothing but numpy: the events, and the expected FaultLog, errors and Batch.  The codes are those
tests/golden/make_replay.py wrote; that module imports the oracle, which a GPU test does not."""
import os

import numpy as np

from hbbft_amd.honey_badger import (INVALID_CIPHERTEXT, SHARE_DECRYPTION_FAILED, UNKNOWN_SENDER,
                                    UNVERIFIED_DECRYPTION_SHARE_SENDER)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FAULT_NAMES = {0: UNVERIFIED_DECRYPTION_SHARE_SENDER, 1: INVALID_CIPHERTEXT, 2: SHARE_DECRYPTION_FAILED}
ERROR_NAMES = {0: UNKNOWN_SENDER}
NO_STATUS = 255


def load(tag):
    return dict(np.load(os.path.join(GOLDEN, f"hb_replay_{tag}.npz"), allow_pickle=False))


def events_of(d):
    acs = {}
    off = d["acs_v_off"]
    for q, j in enumerate(d["acs_proposers"]):
        acs[int(j)] = (d["acs_u"][q].tobytes(), d["acs_v_blob"][int(off[q]):int(off[q + 1])].tobytes(),
                       d["acs_w"][q].tobytes())
    events = []
    for k in range(len(d["ev_kind"])):
        if d["ev_kind"][k] == 0:
            events.append(("share", int(d["ev_sender"][k]), int(d["ev_proposer"][k]), d["ev_share"][k].tobytes()))
        else:
            events.append(("acs", acs))
    return events


def expect(d):
    """(faults, errors, batch or None)."""
    faults = [(int(a), FAULT_NAMES[int(b)]) for a, b in zip(d["expect_fault_node"], d["expect_fault_kind"])]
    errors = [(int(a), ERROR_NAMES[int(b)]) for a, b in zip(d["expect_error_node"], d["expect_error_kind"])]
    batch = None
    if bool(d["expect_batch"]):
        off = d["expect_batch_off"]
        batch = {int(j): d["expect_batch_blob"][int(off[q]):int(off[q + 1])].tobytes()
                 for q, j in enumerate(d["expect_batch_proposers"])}
    return faults, errors, batch
