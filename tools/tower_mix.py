"""Developer tool: instruction mix of the digit tower's functions (hbbft_amd/csrc/fieldd.hpp) on gfx950.

Compiles tools/microbench/tower_probe.hip (one kernel per tower function) device-only with the flags
of a share-check translation unit (tools/build.py TU_FLAGS) and prints, per function, its instructions
by class: 64-bit multiply-adds (``v_mad_*64*``), accumulator-register moves (``v_accvgpr_*``), scratch
accesses (``scratch_*``), wait states (``s_nop``), every other VALU instruction, and the spilled VGPRs
of the code object's metadata.  ``slots`` = multiply-adds + other VALU + s_nop: the share check is
issue-bound, so a function's cost follows its slots.  The classes are mnemonic
prefixes; the counts are static (straight-line code: the probes have no loops).  Needs no GPU.

Usage: python tools/tower_mix.py [--tu N[,N...]] [-D NAME[=V] ...] [--only FN[,FN...]]
  --tu    units whose flags to compile with (default 2,3,8: the one-lane Miller kernel, the six-lane
          check without digit laundering, the final-exponentiation steps); compiled in parallel
  --only  compile only these functions' kernels (a quick look while changing one function)
"""
from __future__ import annotations

import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import build  # noqa: E402
import isa_check  # noqa: E402
import kres  # noqa: E402

PROBE = os.path.join(HERE, "microbench", "tower_probe.hip")
CLASSES = ("mad64", "accvgpr", "scratch", "s_nop", "valu")


def classify(op: str):
    """Class of one mnemonic, by prefix; None for what is not counted (scalar, memory, waits)."""
    if op.startswith("v_mad_") and "64" in op:
        return "mad64"
    if op.startswith("v_accvgpr_"):
        return "accvgpr"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("v_"):
        return "valu"
    return None


def mix_of_listing(disasm: str):
    """{kernel: {class: count}} of an llvm-objdump listing."""
    out = {}
    for name, body in isa_check._functions(disasm):
        d = dict.fromkeys(CLASSES, 0)
        ends = [k for k, ins in enumerate(body) if ins.startswith("s_endpgm")]
        for ins in body[:ends[-1]] if ends else body:  # (after s_endpgm: padding up to the next symbol)
            c = classify(ins.split(" ", 1)[0])
            if c:
                d[c] += 1
        out[name] = d
    return out


def probe_mix(flags):
    """{function: {class: count, "vspill": n}} of the probe compiled with `flags`."""
    with tempfile.TemporaryDirectory() as tmp:
        co = os.path.join(tmp, "tower_probe.co")
        subprocess.check_call([build.HIPCC, "-O3", f"--offload-arch={build.ARCH}", "-std=c++17", "--cuda-device-only",
                               "-c", "-o", co, PROBE] + list(flags))
        res = kres.kernel_resources(co)
        with open(co, "rb") as fh:
            bundled = fh.read(19) == b"__CLANG_OFFLOAD_BUN"
        if bundled:
            raw = os.path.join(tmp, "raw.co")
            subprocess.check_call([f"{isa_check.LLVM}/clang-offload-bundler", "--type=o",
                                   f"--targets=hipv4-amdgcn-amd-amdhsa--{isa_check.ARCH}", f"--input={co}",
                                   f"--output={raw}", "--unbundle"])
            co = raw
        dis = subprocess.run([f"{isa_check.LLVM}/llvm-objdump", "-d", f"--mcpu={isa_check.ARCH}", co],
                             capture_output=True, text=True, check=True).stdout
    out = {}
    for sym, d in mix_of_listing(dis).items():
        m = re.search(r"\d+(p_\w+?)PKiPi$", sym)  # _Z10p_fq2d_mulPKiPi
        if not m or sym not in res:
            continue
        d["vspill"] = res[sym]["vspill"]
        out[m.group(1)[2:]] = d
    return out


def main(argv):
    tus, defs = [2, 3, 8], []
    k = 0
    while k < len(argv):
        if argv[k] == "--tu":
            tus = [int(x) for x in argv[k + 1].split(",")]
            k += 2
        elif argv[k] == "-D":
            defs.append("-D" + argv[k + 1])
            k += 2
        elif argv[k] == "--only":
            defs += ["-DPROBE_SELECT"] + [f"-DPROBE_SEL_{fn}=1" for fn in argv[k + 1].split(",")]
            k += 2
        else:
            raise SystemExit(__doc__)
    with concurrent.futures.ThreadPoolExecutor(len(tus)) as pool:
        mixes = list(pool.map(lambda tu: probe_mix(build.TU_FLAGS.get(tu, []) + defs), tus))
    for tu, mix in zip(tus, mixes):
        flags = build.TU_FLAGS.get(tu, []) + defs
        print(f"# unit {tu}: -O3 {' '.join(flags)}".rstrip())
        print(f"{'function':24s} {'mad64':>7s} {'valu':>7s} {'accvgpr':>7s} {'scratch':>7s} {'s_nop':>6s} {'vspill':>6s} "
              f"{'slots':>7s} {'non-mad':>7s}")
        for fn, d in sorted(mix.items()):
            slots = d["mad64"] + d["valu"] + d["s_nop"]
            print(f"{fn:24s} {d['mad64']:7d} {d['valu']:7d} {d['accvgpr']:7d} {d['scratch']:7d} {d['s_nop']:6d} "
                  f"{d['vspill']:6d} {slots:7d} {100.0 * (slots - d['mad64']) / max(slots, 1):6.1f}%")
        print()


if __name__ == "__main__":
    main(sys.argv[1:])
