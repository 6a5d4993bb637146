"""Offline, CPU only: are the kernels of two `make asm` listings the same code?  The repeatable form of "assembly compared with
the parent's".

Both files are split per kernel (a `.type NAME,@function` symbol, from its label to its `.Lfunc_end`; a listing without `.type`
lines: every `.globl` symbol), the names demangled (c++filt), comments dropped, lines that carry the kernel's own symbol dropped,
and the `.LBB<n>_` prefix of local labels — n is the function's number in its file — reduced to `.LBB_`.  What is left is compared as
text, kernel by kernel, matched by demangled name:

    identical                           the same lines
    differs (n -> m instructions)       anything else; with the registers and scratch the listing's resource comments give
    only in A / only in B               no kernel of that name on the other side

`--rename REGEX REPLACEMENT` (any number) rewrites the demangled names of A before matching, for kernels that changed their name or
their template arguments.  Exit status 1 on any difference or unmatched kernel that no `--allow REGEX` (searched in the name B has)
names, else 0.  `--only REGEX` keeps the kernels whose name matches.  It compares text: it knows no instruction.

    python tools/asm_diff.py parent/resize.s build/resize.s --rename 'k_resize_(\\w+)_placed<' 'k_resize_\\1<' [--allow REGEX] [--only k_resize_]
"""
from __future__ import annotations

import argparse
import re
import shutil
import subprocess
import sys
from pathlib import Path

_LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
_RESOURCE = re.compile(r"^;\s*(NumVgprs|TotalNumSgprs|ScratchSize):\s*(\d+)")


def demangle(names):
    """{mangled: demangled} through c++filt (or LLVM's); the names themselves where neither is at hand"""
    names = list(names)
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt") or shutil.which("llvm-cxxfilt", path="/opt/rocm/llvm/bin")
    if not tool or not names:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def split_kernels(path):
    """{mangled name: {"lines": normalised body, "n": instructions, "res": {NumVgprs, TotalNumSgprs, ScratchSize}}} of one listing"""
    text = Path(path).read_text().splitlines()
    typed = {m.group(1) for ln in text for m in [re.match(r"\s*\.type\s+([^,\s]+),@function", ln)] if m}
    globl = {m.group(1) for ln in text for m in [re.match(r"\s*\.globl\s+(\S+)", ln)] if m}
    funcs = typed or globl
    kernels, cur = {}, None
    for ln in text:
        m = _LABEL.match(ln)
        if cur is None:
            if m and m.group(1) in funcs:
                cur = m.group(1)
                kernels[cur] = {"lines": [], "n": 0, "res": {}}
            elif kernels:
                r = _RESOURCE.match(ln)
                last = next(reversed(kernels))
                if r and r.group(1) not in kernels[last]["res"]:
                    kernels[last]["res"][r.group(1)] = int(r.group(2))
            continue
        if m and m.group(1).startswith(".Lfunc_end"):
            cur = None
            continue
        code = ln.split(";", 1)[0].strip()
        if not code or cur in code:
            continue
        code = re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s+", " ", code))
        kernels[cur]["lines"].append(code)
        if not code.startswith(".") and not code.endswith(":"):
            kernels[cur]["n"] += 1
    return kernels


def compare(path_a, path_b, renames=(), only=None):
    """[(name, verdict, detail)] sorted by name; verdict "identical", "differs", "only in A" or "only in B" """
    sides = []
    for path, ren in ((path_a, renames), (path_b, ())):
        ks = split_kernels(path)
        names = demangle(ks)
        side = {}
        for mangled, k in ks.items():
            name = names[mangled]
            for pat, rep in ren:
                name = re.sub(pat, rep, name)
            if only is None or re.search(only, name):
                side[name] = k
        sides.append(side)
    a, b = sides
    rows = []
    for name in sorted(set(a) | set(b)):
        if name not in b:
            rows.append((name, "only in A", ""))
        elif name not in a:
            rows.append((name, "only in B", ""))
        elif a[name]["lines"] == b[name]["lines"]:
            rows.append((name, "identical", ""))
        else:
            ra, rb = a[name]["res"], b[name]["res"]
            res = ", ".join(f"{key} {ra.get(key, '?')} -> {rb.get(key, '?')}" for key in ("NumVgprs", "TotalNumSgprs", "ScratchSize") if key in ra or key in rb)
            rows.append((name, "differs", f"({a[name]['n']} -> {b[name]['n']} instructions{'; ' + res if res else ''})"))
    return rows


def main(argv=None, out=sys.stdout) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--rename", nargs=2, action="append", default=[], metavar=("REGEX", "REPLACEMENT"))
    ap.add_argument("--allow", action="append", default=[], metavar="REGEX")
    ap.add_argument("--only", default=None, metavar="REGEX")
    args = ap.parse_args(argv)
    rows = compare(args.a, args.b, args.rename, args.only)
    bad = 0
    count = {}
    for name, verdict, detail in rows:
        allowed = verdict != "identical" and any(re.search(p, name) for p in args.allow)
        bad += verdict != "identical" and not allowed
        count[verdict] = count.get(verdict, 0) + 1
        print(f"{name}: {verdict}{' ' + detail if detail else ''}{' [allowed]' if allowed else ''}", file=out)
    print(f"{len(rows)} kernels: " + ", ".join(f"{v} {k}" for k, v in sorted(count.items())) + f"; {bad} not allowed", file=out)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
