"""The host planner of hbx_add_echoes_d / hbx_broadcast_decode_insts_d (hbbft_amd/csrc/bcplan.hpp),
compiled for the CPU by g++ (tools/hostcheck/bcplancheck.cpp) and compared with a Python model: the
duplicate and bounds checks, the offset list, the grouping of long values into hash blocks, the
work-buffer layout of a decode list, and the row descriptors of the ragged calls.  The same source builds as a stand-alone program with
-fsanitize=address,undefined, which plans the same edge sets in a subprocess (nothing sanitized is
loaded into Python)."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostcheck", "bcplancheck.cpp")
OK, BAD_INST, BAD_SENDER, DUPLICATE, BAD_OFFSETS, BAD_LEN, NO_ROOM = range(7)
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def bp(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("bcplancheck") / "libbcplancheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC])
    lib = ctypes.CDLL(out)
    P, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    lib.bp_check_items.argtypes = [P, P, u32, u32, u32]
    lib.bp_check_offsets.argtypes = [P, u32, u64]
    lib.bp_check_offsets_bad.argtypes = [P, u32, u64, P]
    lib.bp_check_rows.argtypes = [u64, P, P, P, u32, u32, P, P]
    lib.bp_group_long.argtypes = [P, u32, u32, u64, P, P, u32]
    lib.bp_check_attempts.argtypes = [P, P, P, P, u32, u32, u32, u32]
    lib.bp_work_layout.argtypes = [P, u32, u32, P, P]
    lib.bp_work_layout.restype = u64
    lib.bp_check_out.argtypes = [P, P, u32, u32, u64]
    lib.bp_check_out_bad.argtypes = [P, P, u32, u32, u64, P]
    return lib


def _u32(v):
    return np.ascontiguousarray(list(v) or [0], dtype=np.uint32)


def _u64(v):
    return np.ascontiguousarray(list(v) or [0], dtype=np.uint64)


# ---- the model ----------------------------------------------------------------------------------
def model_items(items, n, insts):
    for q, i in items:
        if q >= insts:
            return BAD_INST
        if i >= n:
            return BAD_SENDER
    return DUPLICATE if len(set(items)) != len(items) else OK


def model_offsets(off, nbytes):
    if any(b < a or b - a > 0xFFFFFFFF for a, b in zip(off[:-1], off[1:])):
        return BAD_OFFSETS
    return BAD_OFFSETS if off[-1] > nbytes else OK


def model_offsets_bad(off):
    """The first j whose off[j..j + 1] is no value; the count for a list that is one."""
    return next((j for j, (a, b) in enumerate(zip(off[:-1], off[1:])) if b < a or b - a > 0xFFFFFFFF), len(off) - 1)


ROWS_OK, ROWS_UNALIGNED, ROWS_BAD_LEN, ROWS_PAST_END, ROWS_OVERLAP = range(5)


def model_rows(buf_bytes, rows, n):
    """rows: (off, len, pitch) per instance -> (code, offending instances, longest shard)."""
    for q, (o, v, p) in enumerate(rows):
        if o % 4 or p % 4:
            return ROWS_UNALIGNED, [q], None
        if v == 0 or p < v:
            return ROWS_BAD_LEN, [q], None
        if o > buf_bytes or n * p > buf_bytes - o:
            return ROWS_PAST_END, [q], None
    order = sorted(range(len(rows)), key=lambda q: rows[q][0])
    for a, b in zip(order[:-1], order[1:]):
        if rows[b][0] < rows[a][0] + n * rows[a][2]:
            return ROWS_OVERLAP, [a, b], None
    return ROWS_OK, [], max(v for _, v, _ in rows)


def rows_check(bp, buf_bytes, rows, n):
    off, v, p = _u64(r[0] for r in rows), _u32(r[1] for r in rows), _u32(r[2] for r in rows)
    mx, bad = np.zeros(1, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    rc = bp.bp_check_rows(buf_bytes, off.ctypes.data, v.ctypes.data, p.ctypes.data, len(rows), n, mx.ctypes.data,
                          bad.ctypes.data)
    return rc, [int(x) for x in bad[:{ROWS_OK: 0, ROWS_OVERLAP: 2}.get(rc, 1)]], int(mx[0]) if rc == ROWS_OK else None


TOP = 1 << 64
ROW_SETS = [  # (name, n, buf_bytes, [(off, len, pitch)])
    ("one", 4, 64, [(0, 5, 8)]), ("off not a multiple of 4", 4, 64, [(2, 5, 8)]),
    ("pitch not a multiple of 4", 4, 64, [(0, 5, 6)]), ("len 0", 4, 64, [(0, 0, 8)]), ("pitch < len", 4, 64, [(0, 9, 8)]),
    ("ends at the buffer", 4, 64, [(32, 8, 8)]), ("one byte past", 4, 63, [(32, 8, 8)]),
    ("pitch rounds the last row past", 4, 62, [(32, 5, 8)]), ("off past the buffer", 4, 64, [(68, 4, 4)]),
    ("off at the buffer", 4, 64, [(64, 4, 4)]), ("two that touch", 4, 64, [(32, 5, 8), (0, 8, 8)]),
    ("overlap by one row", 4, 64, [(24, 5, 8), (0, 8, 8)]), ("same offset", 2, 64, [(8, 4, 4), (8, 4, 4)]),
    ("second instance wins its own rule", 4, 64, [(0, 5, 8), (32, 9, 8)]),
    ("three, the middle pair", 2, 96, [(64, 8, 8), (0, 8, 8), (12, 8, 8)]),
    ("near 2^64", 256, TOP - 1, [(TOP - 1024, 4, 4)]), ("near 2^64, one row past", 256, TOP - 1, [(TOP - 1020, 4, 4)]),
    ("off near 2^64, past the buffer", 256, 1 << 40, [(TOP - 4, 4, 4)]),
    ("wide pitch", 256, TOP - 1, [(0, 4, 0xFFFFFFFC), (256 * 0xFFFFFFFC, 0xFFFFFFFC, 0xFFFFFFFC)]),
]


def model_groups(lens, lanes, max_value):
    """[(length, [indices padded with NONE])]: the values longer than 256 bytes (and within
    max_value) by (length, index), in blocks of `lanes` of one length."""
    lng = sorted((v, j) for j, v in enumerate(lens) if v > 256 and (max_value == 0 or v <= max_value))
    out = []
    for v, j in lng:
        if out and out[-1][0] == v and len(out[-1][1]) < lanes:
            out[-1][1].append(j)
        else:
            out.append((v, [j]))
    return [(v, idx + [NONE] * (lanes - len(idx))) for v, idx in out]


def model_layout(lens, n):
    off, pitch, at = [], [], 0
    for v in lens:
        p = -(-v // 16) * 16
        off.append(at)
        pitch.append(p)
        at += n * p
    return off, pitch, at


def model_attempts(att, n, insts, max_len):
    """att: (inst, root byte, len, use bits)."""
    for q, _, v, _ in att:
        if q >= insts:
            return BAD_INST
        if v == 0 or v > max_len:
            return BAD_LEN
    keys = [(q, r, u & ((1 << n) - 1)) for q, r, _, u in att]
    return DUPLICATE if len(set(keys)) != len(keys) else OK


def model_out(lens, out_off, k, out_bytes):
    rng = []
    for v, o in zip(lens, out_off):
        need = max(k * v - 4, 0)
        if o > out_bytes or need > out_bytes - o:
            return NO_ROOM
        if need:
            rng.append((o, o + need))
    rng.sort()
    return NO_ROOM if any(b[0] < a[1] for a, b in zip(rng[:-1], rng[1:])) else OK


def model_out_bad(lens, out_off, k, out_bytes):
    """The first attempt without room; the count when every attempt has room (ranges may still overlap)."""
    return next((a for a, (v, o) in enumerate(zip(lens, out_off))
                 if o > out_bytes or max(k * v - 4, 0) > out_bytes - o), len(lens))


# ---- the planner through ctypes --------------------------------------------------------------
def groups(bp, lens, lanes, max_value):
    off = _u64(np.concatenate(([0], np.cumsum(lens))) if len(lens) else [0])
    cap = len(lens) + 1
    bl, bi = np.zeros(cap, dtype=np.uint32), np.zeros(cap * lanes, dtype=np.uint32)
    nb = bp.bp_group_long(off.ctypes.data, len(lens), lanes, max_value, bl.ctypes.data, bi.ctypes.data, cap)
    assert 0 <= nb <= cap
    return [(int(bl[b]), [int(x) for x in bi[b * lanes:(b + 1) * lanes]]) for b in range(nb)]


def attempts(bp, att, n, insts, max_len):
    na = len(att)
    roots = np.zeros((max(na, 1), 32), dtype=np.uint8)
    use = np.zeros((max(na, 1), n), dtype=np.uint8)
    for a, (_, r, _, u) in enumerate(att):
        roots[a] = r
        use[a] = [(u >> i) & 1 for i in range(n)]
    q, v = _u32(a[0] for a in att), _u32(a[2] for a in att)
    return bp.bp_check_attempts(q.ctypes.data, roots.ctypes.data, v.ctypes.data, use.ctypes.data, na, n, insts, max_len)


ITEM_SETS = [
    ("empty", 7, 3, []), ("one", 7, 3, [(2, 6)]), ("whole store", 4, 3, [(q, i) for q in range(3) for i in range(4)]),
    ("pair twice", 7, 3, [(0, 1), (1, 1), (0, 1)]), ("inst at the count", 7, 3, [(0, 1), (3, 1)]),
    ("sender at n", 7, 3, [(0, 7)]), ("inst wins over a later duplicate", 7, 3, [(0, 1), (0, 1), (9, 0)]),
]
LEN_SETS = [
    ("none long", 64, 0, [1, 2, 256, 0, 255]), ("at the limit", 64, 0, [256, 257, 256, 257]),
    ("one odd among equal", 64, 0, [300] * 5 + [301] + [300] * 4), ("65 equal", 64, 0, [400] * 65),
    ("33 equal, 32 lanes", 32, 0, [400] * 33), ("oversize left out", 64, 301, [300, 301, 302, 5000, 257]),
    ("descending", 64, 0, [900, 800, 700, 257]), ("empty call", 64, 0, []),
]
ATTEMPT_SETS = [
    ("empty", 7, 3, 100, []), ("one", 7, 3, 100, [(2, 5, 100, 0x7F)]), ("len 0", 7, 3, 100, [(0, 5, 0, 0x7F)]),
    ("len max + 1", 7, 3, 100, [(0, 5, 101, 0x7F)]), ("inst at the count", 7, 3, 100, [(3, 5, 10, 0x7F)]),
    ("two roots of one instance", 7, 3, 100, [(1, 5, 10, 0x7F), (1, 6, 12, 0x7F)]),
    ("same attempt twice", 7, 3, 100, [(1, 5, 10, 0x7F), (0, 5, 10, 0x7F), (1, 5, 10, 0x7F)]),
    ("same root, other senders", 7, 3, 100, [(1, 5, 10, 0x7F), (1, 5, 10, 0x3F)]),
]


@pytest.mark.parametrize("name,n,insts,items", ITEM_SETS, ids=[s[0] for s in ITEM_SETS])
def test_items(bp, name, n, insts, items):
    q, i = _u32(a for a, _ in items), _u32(b for _, b in items)
    assert bp.bp_check_items(q.ctypes.data, i.ctypes.data, len(items), n, insts) == model_items(items, n, insts)


def test_items_random(bp):
    rnd = random.Random(7)
    for _ in range(200):
        n, insts = rnd.choice([4, 7, 256]), rnd.choice([1, 3, 128])
        items = [(rnd.randrange(insts + (rnd.random() < 0.05)), rnd.randrange(n + (rnd.random() < 0.05)))
                 for _ in range(rnd.randrange(0, 40))]
        q, i = _u32(a for a, _ in items), _u32(b for _, b in items)
        assert bp.bp_check_items(q.ctypes.data, i.ctypes.data, len(items), n, insts) == model_items(items, n, insts)


def test_offsets(bp):
    for off, nbytes in [([0], 0), ([0, 0, 0], 0), ([0, 5, 9], 9), ([0, 5, 9], 8), ([0, 5, 4], 9), ([3, 3, 10], 10),
                        ([0, 1 << 32], 1 << 33), ([0, (1 << 32) - 1], 1 << 33), ([5, 2], 10),
                        ([0, 4, TOP - 1], TOP - 1), ([TOP - 8, TOP - 1], TOP - 2), ([0, 1, 1, 0, 9], 9)]:
        o, bad = _u64(off), np.full(1, 77, dtype=np.uint32)
        assert bp.bp_check_offsets(o.ctypes.data, len(off) - 1, nbytes) == model_offsets(off, nbytes), off
        assert bp.bp_check_offsets_bad(o.ctypes.data, len(off) - 1, nbytes, None) == model_offsets(off, nbytes), off
        assert bp.bp_check_offsets_bad(o.ctypes.data, len(off) - 1, nbytes, bad.ctypes.data) == model_offsets(off, nbytes), off
        assert int(bad[0]) == model_offsets_bad(off), off  # the pair a text names; the count: the list ends past the blob


@pytest.mark.parametrize("name,n,buf_bytes,rows", ROW_SETS, ids=[s[0] for s in ROW_SETS])
def test_rows(bp, name, n, buf_bytes, rows):
    want = model_rows(buf_bytes, rows, n)
    got = rows_check(bp, buf_bytes, rows, n)
    if name == "same offset":  # the order of equal offsets is the sort's
        got, want = (got[0], sorted(got[1]), got[2]), (want[0], sorted(want[1]), want[2])
    assert got == want


def test_rows_random(bp):
    """Distinct offsets (a tie's order is the sort's): instances laid out back to back, then one rule broken."""
    rnd = random.Random(13)
    seen = set()
    for _ in range(400):
        n, inst = rnd.choice([1, 4, 7, 256]), rnd.choice([1, 2, 3, 9])
        rows, at = [], 4 * rnd.randrange(3)
        for _ in range(inst):
            v = rnd.choice([1, 3, 4, 5, 300])
            p = (v + 3) // 4 * 4 + 4 * rnd.randrange(2)
            rows.append((at, v, p))
            at += n * p + 4 * rnd.randrange(2)
        buf_bytes = at + rnd.choice([0, 0, 1, 8])
        q, how = rnd.randrange(inst), rnd.randrange(8)
        o, v, p = rows[q]
        if how == 0:
            rows[q] = (o + 2, v, p)
        elif how == 1:
            rows[q] = (o, v, p + 2)
        elif how == 2:
            rows[q] = (o, rnd.choice([0, p + 1]), p)
        elif how == 3:
            buf_bytes = rows[-1][0] + n * rows[-1][2] - rnd.choice([1, 4])
        elif how == 4 and q:
            rows[q] = (o - 4 * rnd.randrange(1, 3), v, p)
        rnd.shuffle(rows)
        if len({r[0] for r in rows}) != len(rows):
            continue
        want = model_rows(buf_bytes, rows, n)
        assert rows_check(bp, buf_bytes, rows, n) == want, (buf_bytes, rows, n)
        seen.add(want[0])
    assert seen == {ROWS_OK, ROWS_UNALIGNED, ROWS_BAD_LEN, ROWS_PAST_END, ROWS_OVERLAP}


@pytest.mark.parametrize("name,lanes,max_value,lens", LEN_SETS, ids=[s[0] for s in LEN_SETS])
def test_length_grouping(bp, name, lanes, max_value, lens):
    got = groups(bp, lens, lanes, max_value)
    assert got == model_groups(lens, lanes, max_value)
    listed = [j for _, idx in got for j in idx if j != NONE]
    assert sorted(listed) == [j for j, v in enumerate(lens) if v > 256 and (max_value == 0 or v <= max_value)]
    for v, idx in got:
        assert idx[0] != NONE  # filled from lane 0: the SHA-256 block's idle lanes follow lane 0
        assert all(lens[j] == v for j in idx if j != NONE)


def test_length_grouping_random(bp):
    rnd = random.Random(11)
    for _ in range(100):
        lens = [rnd.choice([0, 1, 200, 256, 257, 300, 300, 300, 1000, 70000]) for _ in range(rnd.randrange(0, 150))]
        for lanes in (32, 64):
            assert groups(bp, lens, lanes, 0) == model_groups(lens, lanes, 0)
            assert groups(bp, lens, lanes, 1001) == model_groups(lens, lanes, 1001)


def test_work_layout(bp):
    for lens, n in [([1], 4), ([5, 16, 17, 300], 7), ([3004] * 13, 13), ([1, 2, 3], 256), ([0xFFFFFFF0], 2)]:
        v = _u32(lens)
        off, pitch = np.zeros(len(lens), dtype=np.uint64), np.zeros(len(lens), dtype=np.uint32)
        total = bp.bp_work_layout(v.ctypes.data, len(lens), n, off.ctypes.data, pitch.ctypes.data)
        m_off, m_pitch, m_total = model_layout(lens, n)
        assert (off.tolist(), pitch.tolist(), total) == (m_off, m_pitch, m_total)
        assert all(o % 16 == 0 for o in m_off) and all(p % 4 == 0 and p >= ln for p, ln in zip(m_pitch, lens))
        # rows of different attempts never overlap
        assert all(a + n * p <= b for a, p, b in zip(m_off[:-1], m_pitch[:-1], m_off[1:]))


@pytest.mark.parametrize("name,n,insts,max_len,att", ATTEMPT_SETS, ids=[s[0] for s in ATTEMPT_SETS])
def test_attempts(bp, name, n, insts, max_len, att):
    assert attempts(bp, att, n, insts, max_len) == model_attempts(att, n, insts, max_len)


def test_use_rows_compare_by_allowed_senders(bp):
    """A use byte allows its sender iff it is non-zero: rows of other non-zero values are the same row."""
    roots = np.zeros((2, 32), dtype=np.uint8)
    q, v = _u32([1, 1]), _u32([5, 5])
    use = np.array([[1, 0, 1, 1, 0, 0, 0], [7, 0, 255, 2, 0, 0, 0]], dtype=np.uint8)
    assert bp.bp_check_attempts(q.ctypes.data, roots.ctypes.data, v.ctypes.data, use.ctypes.data, 2, 7, 3, 100) == DUPLICATE
    use[1, 1] = 9
    assert bp.bp_check_attempts(q.ctypes.data, roots.ctypes.data, v.ctypes.data, use.ctypes.data, 2, 7, 3, 100) == OK


def test_attempts_without_use(bp):
    roots = np.zeros((2, 32), dtype=np.uint8)
    q, v = _u32([1, 1]), _u32([5, 5])
    assert bp.bp_check_attempts(q.ctypes.data, roots.ctypes.data, v.ctypes.data, None, 2, 7, 3, 100) == DUPLICATE
    roots[1, 31] = 1
    assert bp.bp_check_attempts(q.ctypes.data, roots.ctypes.data, v.ctypes.data, None, 2, 7, 3, 100) == OK


def test_output_room(bp):
    for lens, out_off, k, ob in [([10, 10], [0, 36], 4, 72), ([10, 10], [0, 35], 4, 72), ([10, 10], [0, 36], 4, 71),
                                 ([1], [0], 3, 0), ([1], [1], 3, 0), ([2], [0], 3, 2), ([2], [0], 3, 1), ([], [], 3, 0),
                                 ([10, 1, 10], [0, 0, 40], 4, 76), ([10, 10, 10], [0, 36, 200], 4, 108),
                                 ([4], [TOP - 13], 4, TOP - 1), ([4], [TOP - 12], 4, TOP - 1), ([4], [TOP - 1], 4, 8)]:
        v, o, bad = _u32(lens), _u64(out_off), np.full(1, 77, dtype=np.uint32)
        assert bp.bp_check_out(v.ctypes.data, o.ctypes.data, len(lens), k, ob) == model_out(lens, out_off, k, ob), (lens, out_off)
        assert bp.bp_check_out_bad(v.ctypes.data, o.ctypes.data, len(lens), k, ob, None) == model_out(lens, out_off, k, ob)
        assert bp.bp_check_out_bad(v.ctypes.data, o.ctypes.data, len(lens), k, ob, bad.ctypes.data) == model_out(lens, out_off, k, ob)
        assert int(bad[0]) == model_out_bad(lens, out_off, k, ob), (lens, out_off)


def test_sanitized_program_plans_the_edge_sets(tmp_path):
    """The planner as a stand-alone program under AddressSanitizer and UBSan over the edge sets:
    clean exit, nothing on stderr, the model's plans on stdout."""
    exe = str(tmp_path / "bcplancheck")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-DBCPLAN_MAIN",
                           "-o", exe, SRC])
    adds = []
    for _, n, insts, items in ITEM_SETS:
        adds.append((n, insts, 0, 64, [300] * len(items), items, None))
    for _, lanes, max_value, lens in LEN_SETS:
        adds.append((256, 4, max_value, lanes, lens, [(j // 256, j % 256) for j in range(len(lens))], None))
    adds.append((7, 3, 0, 64, [5, 4], [(0, 0), (0, 1)], [0, 5, 4]))  # decreasing val_off
    adds.append((7, 3, 0, 64, [5, 4], [(0, 0), (0, 1)], [0, 5, 20]))  # past the blob (9 bytes)
    decs = [(n, insts, max_len, 3, att) for _, n, insts, max_len, att in ATTEMPT_SETS]
    text = ""
    for n, insts, max_value, lanes, lens, items, off in adds:
        off = off if off is not None else [0] + np.cumsum(lens).tolist()
        text += f"add {n} {insts} {max_value} {lanes} {sum(lens)} {len(items)} " + \
            " ".join(f"{q} {i}" for q, i in items) + " " + " ".join(str(o) for o in off) + "\n"
    for n, insts, max_len, k, att in decs:
        room = [0]
        for _, _, v, _ in att:
            room.append(room[-1] + max(k * v - 4, 0))
        text += f"dec {n} {insts} {max_len} {k} {room[-1]} {len(att)} " + \
            " ".join(f"{q} {r} {v} {u} {o}" for (q, r, v, u), o in zip(att, room)) + "\n"
    for _, n, buf_bytes, rows in ROW_SETS:
        text += f"row {n} {buf_bytes} {len(rows)} " + " ".join(f"{o} {v} {p}" for o, v, p in rows) + "\n"
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == ""
    lines = iter(run.stdout.splitlines())
    for n, insts, max_value, lanes, lens, items, off in adds:
        bad = model_items(items, n, insts) or (model_offsets(off, sum(lens)) if off is not None else OK)
        head = next(lines).split()
        if bad:
            assert head == ["rc", str(bad)]
            continue
        want = model_groups(lens, lanes, max_value)
        assert head == ["blocks", str(len(want))]
        for v, idx in want:
            assert next(lines).split() == ["len", str(v), "idx"] + [str(j) for j in idx]
    for n, insts, max_len, k, att in decs:
        bad = model_attempts(att, n, insts, max_len)
        head = next(lines).split()
        if bad:
            assert head == ["rc", str(bad)]
            continue
        off, pitch, total = model_layout([a[2] for a in att], n)
        assert head == ["total", str(total)]
        for o, p in zip(off, pitch):
            assert next(lines).split() == ["off", str(o), "pitch", str(p)]
    for name, n, buf_bytes, rows in ROW_SETS:
        code, bad, mx = model_rows(buf_bytes, rows, n)
        head = [int(x) for x in next(lines).split()[1:]]
        if code == ROWS_OK:
            assert head == [mx]
        else:
            assert head[0] == code and (sorted(head[1:]) if name == "same offset" else head[1:1 + len(bad)]) == bad
    assert next(lines, None) is None
