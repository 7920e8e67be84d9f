"""The launch planner of hbx_add_dec_shares_d (hbbft_amd/csrc/addplan.hpp), compiled for the CPU by g++
(tools/hostcheck/addplancheck.cpp) and compared with a Python model: the touched tiles of every
lanes-per-check shape, the lane ladder at its boundaries and the rejections.  The same source builds
as a stand-alone program with -fsanitize=address,undefined, which plans the same edge sets in a
subprocess (nothing sanitized is loaded into Python)."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostcheck", "addplancheck.cpp")
SENDERS = (64, 32, 21, 10)  # per tile at 1, 2, 3, 6 lanes per check
NO_ME = 0xFFFFFFFF


@pytest.fixture(scope="module")
def ap(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("addplancheck") / "libaddplancheck.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", out, SRC])
    lib = ctypes.CDLL(out)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    u32 = ctypes.c_uint32
    lib.ap_plan.argtypes = [u32p, u32p, u32, u32, u32, u32, ctypes.c_int, u32p, u32, u32p]
    lib.ap_lanes_of.argtypes = [u32p, u32p, u32, u32, u32, u32]
    lib.ap_choose_lanes.argtypes = [ctypes.c_uint64] * 4
    lib.ap_shape_of_lanes.argtypes = [ctypes.c_int]
    lib.ap_shape_senders.argtypes = [ctypes.c_int]
    lib.ap_shape_senders.restype = u32
    return lib


def model_tiles(items, n, shape):
    """Touched tiles (x, j) of `shape`, in (j, x) order."""
    return sorted({(i // SENDERS[shape], j) for j, i in items if i < n}, key=lambda t: (t[1], t[0]))


def model_ladder(t1, t6, t3, t2):
    return 1 if t1 >= 1024 else 6 if t6 <= 1024 else 3 if t3 <= 1024 else 2 if t2 <= 1024 else 3


def model_lanes(items, n):
    t = [len(model_tiles(items, n, s)) for s in range(4)]
    return model_ladder(t[0], t[3], t[2], t[1])


def _arr(v):
    return (ctypes.c_uint32 * max(len(v), 1))(*v)


def plan(ap, items, n, p, shape, me=NO_ME):
    prop, snd = _arr([j for j, _ in items]), _arr([i for _, i in items])
    cap = len(items) + 1
    out = (ctypes.c_uint32 * (2 * cap))()
    live = ctypes.c_uint32(0)
    rc = ap.ap_plan(prop, snd, len(items), n, p, me, shape, out, cap, ctypes.byref(live))
    if rc < 0:
        return rc, None, None
    assert rc <= cap
    return rc, [(int(out[2 * k]), int(out[2 * k + 1])) for k in range(rc)], int(live.value)


def last_partial_tile_items(n, p):
    """Per shape, the senders of that shape's last (partial or not) tile, in the last column."""
    sets = []
    for per in SENDERS:
        x = (n - 1) // per
        sets.append([(p - 1, i) for i in range(x * per, n)])
    return sets


def edge_sets():
    """(name, n, p, items)."""
    out = [("empty", 7, 3, []), ("one item", 10, 4, [(2, 9)]), ("full column", 256, 4, [(1, i) for i in range(256)]),
           ("whole 4 x 256", 256, 4, [(j, i) for j in range(4) for i in range(256)])]
    for n in (7, 10, 64, 65, 256):
        for s, items in enumerate(last_partial_tile_items(n, 3)):
            out.append((f"last tile of shape {s} at n={n}", n, 3, items))
    out.append(("unknown senders only", 10, 4, [(0, 10), (3, 15)]))
    out.append(("mixed with unknown senders", 65, 2, [(1, 64), (1, 65), (0, 70), (0, 0)]))
    return out


def random_sets():
    rnd = random.Random(20)
    out = []
    for q in range(40):
        n = rnd.choice([4, 7, 10, 21, 22, 63, 64, 65, 100, 256])
        p = rnd.choice([1, 3, n])
        cells = [(j, i) for j in range(p) for i in range(n + 3)]
        items = rnd.sample(cells, rnd.randrange(0, min(len(cells), 300) + 1))
        out.append((f"random {q}", n, p, items))
    return out


@pytest.mark.parametrize("name,n,p,items", edge_sets() + random_sets(), ids=lambda v: v if isinstance(v, str) else None)
def test_tile_lists_match_model(ap, name, n, p, items):
    for shape in range(4):
        assert ap.ap_shape_senders(shape) == SENDERS[shape]
        count, tiles, live = plan(ap, items, n, p, shape)
        want = model_tiles(items, n, shape)
        assert tiles == want, (name, shape)
        assert count == len(want) and live == sum(1 for _, i in items if i < n)
        for x, j in tiles:
            assert j < p and x * SENDERS[shape] < n  # every tile lies inside the matrix
    prop, snd = _arr([j for j, _ in items]), _arr([i for _, i in items])
    assert ap.ap_lanes_of(prop, snd, len(items), n, p, NO_ME) == model_lanes(items, n)


def test_whole_matrix_is_the_matrix_calls_grid(ap):
    """An add that touches every position launches the matrix call's tiles and takes its lanes."""
    for n, p in ((256, 4), (64, 64), (10, 10), (65, 3)):
        items = [(j, i) for j in range(p) for i in range(n)]
        waves = []
        for shape in range(4):
            count, _, _ = plan(ap, items, n, p, shape)
            assert count == -(-n // SENDERS[shape]) * p
            waves.append(count)
        prop, snd = _arr([j for j, _ in items]), _arr([i for _, i in items])
        assert ap.ap_lanes_of(prop, snd, len(items), n, p, NO_ME) == model_ladder(waves[0], waves[3], waves[2], waves[1])


def test_lane_ladder_boundaries(ap):
    assert [ap.ap_shape_of_lanes(k) for k in (1, 2, 3, 6, 7)] == [0, 1, 2, 3, 0]
    # T1 = 1023 / 1024: below a full chip the most lanes that fit, from it on one lane per check
    assert ap.ap_choose_lanes(1023, 1023 * 7, 1023 * 4, 1023 * 2) == 3  # 6: 7161, 3: 4092, 2: 2046 -> 3
    assert ap.ap_choose_lanes(1023, 1024, 1023, 1023) == 6
    assert ap.ap_choose_lanes(1024, 1024, 1024, 1024) == 1
    assert ap.ap_choose_lanes(1024, 7000, 4000, 2048) == 1
    # T6 = 1024 / 1025
    assert ap.ap_choose_lanes(200, 1024, 600, 400) == 6
    assert ap.ap_choose_lanes(200, 1025, 600, 400) == 3
    assert ap.ap_choose_lanes(600, 3000, 1025, 1024) == 2
    assert ap.ap_choose_lanes(600, 3000, 1025, 1025) == 3
    for t in [(0, 0, 0, 0), (1, 1, 1, 1), (1023, 1025, 1024, 1024), (512, 2048, 1025, 1024), (1000, 5000, 3000, 2000)]:
        assert ap.ap_choose_lanes(*t) == model_ladder(*t)


# (n, p, lanes) of a full p x n matrix.  Each value is worked out by hand from the ladder the matrix
# verification has always stated (one lane when ceil(n/64) p >= 1024; else six when ceil(n/10) p <=
# 1024; else three when ceil(n/21) p <= 1024; else two when ceil(n/32) p <= 1024; else three):
#   256 x 256: t1 = 4 * 256 = 1024 -> 1        10 x 10: t6 = 10 -> 6        64 x 64: t6 = 7 * 64 = 448 -> 6
#   128 x 32: t6 = 13 * 32 = 416 -> 6          256 x 32: t6 = 26 * 32 = 832 -> 6
#   256 x 64: t6 = 1664, t3 = 13 * 64 = 832 -> 3
#   256 x 96: t6 = 2496, t3 = 1248, t2 = 8 * 96 = 768 -> 2
#   256 x 128: t6 = 3328, t3 = 1664, t2 = 8 * 128 = 1024, t1 = 512 -> 2
FULL_MATRIX_LANES = [(256, 256, 1), (10, 10, 6), (64, 64, 6), (128, 32, 6), (256, 32, 6), (256, 64, 3), (256, 96, 2),
                     (256, 128, 2)]


def test_full_matrix_lanes(ap):
    """The matrix verification takes its lanes from choose_lanes over the whole matrix's tile counts."""
    for n, p, lanes in FULL_MATRIX_LANES:
        t1, t2, t3, t6 = (-(-n // per) * p for per in SENDERS)
        assert ap.ap_choose_lanes(t1, t6, t3, t2) == lanes, (n, p)


def test_rejections(ap):
    assert plan(ap, [(0, 1), (1, 1), (0, 1)], 7, 3, 0)[0] == -2  # the same pair twice
    assert plan(ap, [(0, 9), (0, 9)], 7, 3, 0)[0] == -2  # ... also of an unknown sender
    assert plan(ap, [(0, 1), (3, 1)], 7, 3, 0)[0] == -1  # proposer >= p
    assert plan(ap, [(0, 1), (2, 1)], 7, 3, 0)[0] == 2
    assert plan(ap, [(0, 1), (2, 5)], 7, 3, 0, me=5)[0] == -3  # own sender in own-share mode
    assert plan(ap, [(0, 1), (2, 5)], 7, 3, 0, me=4)[0] == 2


def test_sanitized_program_plans_the_edge_sets(tmp_path):
    """The planner as a stand-alone program under AddressSanitizer and UBSan, over the edge sets (and
    the rejections): clean exit, nothing on stderr, the model's tile lists on stdout."""
    exe = str(tmp_path / "addplancheck")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-DADDPLAN_MAIN",
                           "-o", exe, SRC])
    sets = [(n, p, NO_ME, items) for _, n, p, items in edge_sets()]
    sets += [(7, 3, NO_ME, [(0, 1), (0, 1)]), (7, 3, NO_ME, [(3, 1)]), (7, 3, 5, [(2, 5)])]
    text = "".join(f"{n} {p} {me} {len(items)} " + " ".join(f"{j} {i}" for j, i in items) + "\n"
                   for n, p, me, items in sets)
    run = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == ""
    lines = iter(run.stdout.splitlines())
    for n, p, me, items in sets:
        head = next(lines).split()
        bad = 1 if any(j >= p for j, _ in items) else 3 if any(i == me for _, i in items) else \
            2 if len(set(items)) != len(items) else 0
        if bad:
            assert head == ["rc", str(bad)]
            continue
        assert head == ["lanes", str(model_lanes(items, n)), "live", str(sum(1 for _, i in items if i < n))]
        for shape in range(4):
            row = [int(v) for v in next(lines).split()[1:]]
            assert row[0] == shape
            got = [(row[2 + 2 * k], row[3 + 2 * k]) for k in range(row[1])]
            assert got == model_tiles(items, n, shape)
    assert next(lines, None) is None
