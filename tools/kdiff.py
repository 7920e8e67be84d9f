"""Developer tool: do two builds hold the same gfx950 machine code?

Compares every device symbol (kernels and out-of-line device functions) that two libhbx.so files --
or two directories of object files -- have in common: the resource fields of tools/kres.py, the
symbol size and the disassembled instruction sequence.  A refactor that only deletes text the
preprocessor or the host dispatch already discarded must come out `identical` throughout.

Instructions are compared without their addresses and encodings, with branch targets written
relative to the symbol start, and with the literals of pc-relative address arithmetic (the
s_add_u32 / s_addc_u32 pair after an s_getpc_b64) as wildcards: those move when a neighbour grows,
shrinks or goes.  A name defined in several code objects (a device function compiled once per
translation unit) is told apart by the index of its code object.

Prints one line per symbol that is not identical and a summary; exit status 1 if a common symbol
differs.  It is a differ only: it looks for no particular instruction.

Usage: python tools/kdiff.py A B
"""
from __future__ import annotations

import collections
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_check  # noqa: E402
import kres  # noqa: E402

_LITERAL = re.compile(r"(?<=, )(0x[0-9a-f]+|-?\d+)$")


def _normalise(lines, start, size):
    """The instructions of one symbol ([(address, text, branch target or None)]), position-free."""
    out, pc_window = [], 0
    for addr, text, target in lines:
        if addr >= start + size:
            break  # alignment padding up to the next symbol
        op = text.split(" ", 1)[0]
        if target is not None and op.startswith(("s_branch", "s_cbranch")):
            text = f"{op} {target}"
        elif op == "s_getpc_b64":
            pc_window = 3  # the pair follows within a few instructions
        elif pc_window:
            if op in ("s_add_u32", "s_addc_u32"):
                text = _LITERAL.sub("*", text)
            pc_window -= 1
        out.append(text)
    return out


def _symbols_of(co: str):
    """{name: (size, [normalised instructions])} of one code object."""
    table = subprocess.run([f"{isa_check.LLVM}/llvm-readelf", "-sW", co], capture_output=True, text=True,
                           check=True).stdout
    funcs = {}
    for row in table.splitlines():
        f = row.split()
        if len(f) == 8 and f[3] == "FUNC" and f[6] != "UND":
            funcs[f[7]] = (int(f[1], 16), int(f[2], 0))
    dis = subprocess.run([f"{isa_check.LLVM}/llvm-objdump", "-d", f"--mcpu={isa_check.ARCH}", co],
                         capture_output=True, text=True, check=True).stdout
    res, name, body = {}, None, []
    for line in dis.splitlines() + ["0 <>:"]:
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            if name in funcs:
                res[name] = (funcs[name][1], _normalise(body, *funcs[name]))
            name, body = m.group(1), []
        elif name and line.startswith("\t") and "//" in line:
            text, note = line.strip().split("//", 1)
            t = re.search(r"<(.+)>\s*$", note)
            target = None
            if t:  # <symbol+0x74> (or <symbol>): relative to this symbol's start if it is this symbol's
                sym, _, off = t.group(1).partition("+")
                target = f"+{off or '0x0'}" if sym == name else t.group(1)
            body.append((int(note.split(":")[0], 16), text.strip(), target))
    return res


def device_symbols(path: str):
    """{key: {"res": kres fields or None, "size": int, "ins": [...]}} over the code objects of a
    library or object file, or of every *.o in a directory."""
    files = sorted(glob.glob(os.path.join(path, "*.o"))) if os.path.isdir(path) else [path]
    per_co, res = [], {}
    for f in files:
        res.update(kres.kernel_resources(f))
        with tempfile.TemporaryDirectory() as tmp:
            per_co += [_symbols_of(co) for co in isa_check._code_objects(f, tmp)]
    seen = collections.Counter(n for syms in per_co for n in syms)
    out = {}
    for k, syms in enumerate(per_co):
        for n, (size, ins) in syms.items():
            out[n if seen[n] == 1 else f"{n}@{k}"] = {"res": res.get(n), "size": size, "ins": ins}
    return out


def compare(a: str, b: str):
    """[(key, verdict, detail)] sorted by key; verdict identical / differs / only in A / only in B."""
    A, B = device_symbols(a), device_symbols(b)
    rows = []
    for key in sorted(set(A) | set(B)):
        if key not in B or key not in A:
            rows.append((key, "only in A" if key in A else "only in B", ""))
            continue
        x, y = A[key], B[key]
        detail = []
        if x["res"] != y["res"]:
            detail.append(f"resources {x['res']} -> {y['res']}")
        if x["size"] != y["size"]:
            detail.append(f"size {x['size']} -> {y['size']}")
        if x["ins"] != y["ins"]:
            i = next((i for i, (p, q) in enumerate(zip(x["ins"], y["ins"])) if p != q), min(len(x["ins"]), len(y["ins"])))
            detail.append(f"instruction {i}: {' '.join(x['ins'][i:i + 1])!r} -> {' '.join(y['ins'][i:i + 1])!r}")
        detail = "; ".join(detail)
        rows.append((key, "differs" if detail else "identical", detail))
    return rows


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    rows = compare(sys.argv[1], sys.argv[2])
    for key, verdict, detail in rows:
        if verdict != "identical":
            print(f"{verdict}: {key}" + (f" ({detail})" if detail else ""))
    count = {v: sum(1 for r in rows if r[1] == v) for v in ("identical", "differs", "only in A", "only in B")}
    print(", ".join(f"{v} {n}" for v, n in count.items()))
    sys.exit(1 if count["differs"] else 0)
