"""tools/kdiff.py on a toy translation unit cross-compiled for gfx950 (no GPU needed): a build
compared with the same source plus one more kernel is identical in every common symbol, and a
changed constant in one kernel shows as that kernel differing -- the other kernel and the
out-of-line device function it calls (a pc-relative call, whose literals move) stay identical."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kdiff  # noqa: E402

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
TOY = """
#include <hip/hip_runtime.h>
__device__ __noinline__ int toy_helper(int x) { return x * 3 + 1; }
#ifdef TOY_EXTRA
__global__ void toy_extra(int* p) { p[threadIdx.x] = toy_helper(p[threadIdx.x]) ^ 5; }
#endif
__global__ void toy_call(int* p, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = toy_helper(p[i]);
}
__global__ void toy_loop(float* p, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  for (int k = 0; k < n; k++)
    if (p[k] > 0) p[i] += TOY_CONST;
}
"""


@pytest.fixture(scope="module")
def builds(tmp_path_factory):
    """Object directories of the toy: as is, with a third kernel, with another constant in toy_loop."""
    root = tmp_path_factory.mktemp("kdiff")
    src = root / "toy.hip"
    src.write_text(TOY)
    procs = {}
    for name, flags in (("base", ["-DTOY_CONST=2.0f"]), ("extra", ["-DTOY_CONST=2.0f", "-DTOY_EXTRA"]),
                        ("const", ["-DTOY_CONST=4.0f"])):
        (root / name).mkdir()
        procs[name] = subprocess.Popen([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", *flags, "-c",
                                        "-o", str(root / name / "toy.o"), str(src)])
    for name, p in procs.items():
        assert p.wait() == 0, name
    return {name: str(root / name) for name in procs}


def _verdicts(rows):
    return {key.split("@")[0]: verdict for key, verdict, _ in rows}


def test_added_kernel_leaves_the_common_symbols_identical(builds):
    v = _verdicts(kdiff.compare(builds["base"], builds["extra"]))
    assert v == {"_Z10toy_helperi": "identical", "_Z8toy_callPii": "identical", "_Z8toy_loopPfi": "identical",
                 "_Z9toy_extraPi": "only in B"}
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kdiff.py"), builds["base"],
                           builds["extra"]]).returncode == 0


def test_changed_constant_differs(builds):
    rows = kdiff.compare(builds["base"], builds["const"])
    assert _verdicts(rows) == {"_Z10toy_helperi": "identical", "_Z8toy_callPii": "identical",
                               "_Z8toy_loopPfi": "differs"}
    detail = [d for key, _, d in rows if key == "_Z8toy_loopPfi"][0]
    assert "2.0" in detail and "4.0" in detail  # the first differing instruction, both sides
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kdiff.py"), builds["base"], builds["const"]],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "differs: _Z8toy_loopPfi" in r.stdout
    assert r.stdout.splitlines()[-1] == "identical 2, differs 1, only in A 0, only in B 0"
