"""Issue-cost model of the strip worker's hot blocks (offline, CPU only).

Reads the compiler's assembly of the kernels (`make -C pyjpegdecoder_amd/csrc asm` -> build/fused.s, build/reconstruct_fast.s)
and weighs every VALU instruction by what its FORM costs to issue on gfx950 at four waves per SIMD — the w4 column of
profiles/r02_issue_rate_probe.txt, this project's own measurement (tools/issue_rate_probe.hip).  Per basic block of each named
kernel: VALU count, cost-weighted SIMD cycles, and how many instructions fall into each expensive class.

    python tools/issue_cost.py [--asm FILE ...] [--kernel 'k_fused<2,2,false,false>' ...] [--min-valu 40] [--probe FILE]

A cost model for choosing what to change: not a check of what a binary may contain, and no test depends on its verdict.
Blocks are recognised by content: `phaseA-round` holds the SDWA int16 converts of a level-1 round, `phaseB-pixels` holds
v_cvt_pk_u8_f32."""
import argparse
import re
import sys
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PROBE = ROOT / "profiles" / "r02_issue_rate_probe.txt"
CSRC_BUILD = ROOT / "pyjpegdecoder_amd" / "csrc" / "build"
DEFAULT_KERNELS = ["k_fused<2,2,false,false>", "k_reconstruct_fast<2,2,3,false,false,false>"]      # (SEAMS, T, WIN = false)

# cost classes -> the probe line that prices them (w4 column)
CLASS_PROBE = {
    "select_vop2_vcc": "v_cndmask_b32",                   # VOP2 form, selecting on VCC
    "select_e64": "v_cndmask_b32 e64 sgpr mask",          # VOP3 form, selecting on an SGPR pair (or VCC named explicitly)
    "sgpr_operand": "v_add_u32 v, s, v",                  # a simple or fp32 op that reads an SGPR source
    "sdwa": "v_cvt_f32_i32 sdwa WORD_1",
    "dpp": "v_mov_b32 dpp",
    "packed": "v_pk_fma_f32",
    "shift_left": "v_lshlrev_b32",
    "lane_access": "v_readlane_b32",                      # v_readlane / v_writelane / v_readfirstlane (SGPR spills live here)
    "compare": "v_cmp_gt_u32",
    "compare_e64": "v_cmp_gt_u32 e64 -> sgpr",
}
EXPENSIVE = ["select_vop2_vcc", "select_e64", "sgpr_operand", "sdwa", "dpp", "packed", "shift_left", "lane_access", "compare", "compare_e64", "other"]
OTHER_DEFAULT = 2.95        # what every VOP3 / three-operand form the probe lists costs at w4; stated default for unlisted forms


def parse_probe(path=PROBE):
    """name -> SIMD cycles per wave-instruction at 4 waves per SIMD."""
    costs = {}
    for line in Path(path).read_text().splitlines():
        m = re.match(r"^(\S.*?)\s+w1:.*?\bw4:\s*([0-9.]+)", line)
        if m and not line.startswith("#"):
            costs[m.group(1).strip()] = float(m.group(2))
    if "v_cndmask_b32" not in costs or "v_add_u32" not in costs:
        raise ValueError(f"{path}: not an issue-rate probe file")
    return costs


_SGPR = re.compile(r"(?<![\w.])(s\d+|s\[\d+:\d+\]|ttmp\d+|ttmp\[\d+:\d+\]|m0)(?![\w.])")


def classify(mnemonic, operands, costs):
    """(class, cycles) of one VALU instruction.  `operands`: the operand string without comments."""
    ops = [o.strip() for o in operands.split(",")] if operands.strip() else []
    base = re.sub(r"_(e32|e64|sdwa|dpp|e64_dpp)$", "", mnemonic)
    price = lambda c: costs.get(CLASS_PROBE[c], OTHER_DEFAULT)
    if base == "v_cndmask_b32":
        if mnemonic.endswith("_e64") or (len(ops) == 4 and ops[3] != "vcc") or mnemonic.endswith("_e64_dpp"):
            return "select_e64", price("select_e64")
        return "select_vop2_vcc", price("select_vop2_vcc")
    if base in ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32"):
        return "lane_access", price("lane_access")
    if mnemonic.endswith("_sdwa"):
        return "sdwa", price("sdwa")
    if mnemonic.endswith("_dpp") or any(w in operands for w in ("quad_perm:", "row_shr:", "row_shl:", "row_ror:", "row_mirror", "row_half_mirror", "row_bcast:", "row_newbcast:")):
        return "dpp", price("dpp")
    if base.startswith("v_cmp") or base.startswith("v_cmpx"):
        to_sgpr = bool(ops) and ops[0] != "vcc" and _SGPR.search(ops[0]) is not None
        return ("compare_e64", price("compare_e64")) if to_sgpr else ("compare", price("compare"))
    if base.startswith("v_pk_"):
        return "packed", costs.get(base, price("packed"))
    own = costs.get(base)
    srcs = ", ".join(ops[1:])
    if _SGPR.search(srcs):
        return "sgpr_operand", max(own or 0.0, price("sgpr_operand"))
    if base == "v_lshlrev_b32":
        return "shift_left", price("shift_left")
    if own is None:
        return "other", OTHER_DEFAULT
    if own < 1.5:
        return "simple", own
    if own < 2.5:
        return "fp32", own
    return "full_cost", own           # listed by the probe at about three cycles: converts, min/max, VOP3 forms, fp64


def mangled_fragment(kernel):
    """'k_fused<2,2,false,false>' -> 'k_fusedILi2ELi2ELb0ELb0EE' (enough of the Itanium name to find the kernel's label)."""
    m = re.match(r"^(\w+)(?:<(.*)>)?$", kernel.replace(" ", ""))
    if not m:
        return kernel
    name, args = m.group(1), m.group(2)
    if not args:
        return name
    enc = "".join(("Lb1E" if a == "true" else "Lb0E" if a == "false" else f"Li{a}E") for a in args.split(","))
    return f"{name}I{enc}E"


def kernel_bodies(text):
    """label -> list of (line number, line) of every function in an assembly file."""
    out, cur, name = {}, None, None
    for n, line in enumerate(text.splitlines(), 1):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;\s*@.*)?$", line)
        if m and not line.startswith(".L") and m.group(2):
            name, cur = m.group(1), []
            out[name] = cur
            continue
        if cur is not None:
            if line.startswith(".Lfunc_end"):
                cur, name = None, None
                continue
            cur.append((n, line))
    return out


def blocks_of(body):
    """Basic blocks: a new one at every label and at every fall-through block the compiler marks ('; %bb.N')."""
    blocks, cur = [], {"label": "entry", "line": body[0][0] if body else 0, "insts": []}
    for n, line in body:
        m = re.match(r"^(\.LBB\d+_\d+):", line)
        mb = re.match(r"^;\s*%bb\.(\d+):", line)
        if m or mb:
            if cur["insts"]:
                blocks.append(cur)
            cur = {"label": m.group(1) if m else f"%bb.{mb.group(1)}", "line": n, "insts": []}
            continue
        code = line.split(";", 1)[0].strip()
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        parts = code.split(None, 1)
        cur["insts"].append((parts[0], parts[1] if len(parts) > 1 else ""))
    if cur["insts"]:
        blocks.append(cur)
    return blocks


def weigh(block, costs):
    cls, cyc, valu = Counter(), 0.0, 0
    names = Counter()
    for mn, ops in block["insts"]:
        names[mn] += 1
        if not mn.startswith("v_"):
            continue
        c, k = classify(mn, ops, costs)
        cls[c] += 1
        cyc += k
        valu += 1
    tag = ""
    if names["v_cvt_pk_u8_f32"] >= 8:           # (first: the pixel block converts its int16 chroma with SDWA forms too)
        tag = "phaseB-pixels"
    elif names["v_cvt_f32_i32_sdwa"] >= 8:
        tag = "phaseA-round"
    return {"label": block["label"], "line": block["line"], "valu": valu, "cycles": cyc, "classes": cls, "tag": tag, "n": len(block["insts"])}


def report(asm_path, kernels, costs, min_valu=40, out=sys.stdout):
    bodies = kernel_bodies(Path(asm_path).read_text())
    found = 0
    for k in kernels:
        frag = mangled_fragment(k)
        for name, body in bodies.items():
            if frag not in name:
                continue
            found += 1
            ws = [weigh(b, costs) for b in blocks_of(body)]
            tv, tc = sum(w["valu"] for w in ws), sum(w["cycles"] for w in ws)
            tot = Counter()
            for w in ws:
                tot.update(w["classes"])
            print(f"== {k}  ({Path(asm_path).name}: {name})", file=out)
            print(f"   static: {len(ws)} blocks, {tv} VALU, {tc:.0f} weighted cycles ({tc / max(tv, 1):.2f} per VALU); by class: "
                  + ", ".join(f"{c} {tot[c]}" for c in ["simple", "fp32", "full_cost"] + EXPENSIVE if tot[c]), file=out)
            print(f"   {'block':12s} {'line':>7s} {'VALU':>5s} {'cycles':>7s} {'cyc/VALU':>8s}  expensive classes", file=out)
            for w in ws:
                if w["valu"] < min_valu and not w["tag"] and not w["classes"]["select_vop2_vcc"]:
                    continue
                exp = ", ".join(f"{c} {w['classes'][c]}" for c in EXPENSIVE if w["classes"][c])
                print(f"   {w['label']:12s} {w['line']:7d} {w['valu']:5d} {w['cycles']:7.0f} {w['cycles'] / max(w['valu'], 1):8.2f}  {exp}  {w['tag']}", file=out)
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--asm", nargs="*", default=[str(CSRC_BUILD / "fused.s"), str(CSRC_BUILD / "reconstruct_fast.s")])
    ap.add_argument("--kernel", nargs="*", default=DEFAULT_KERNELS)
    ap.add_argument("--probe", default=str(PROBE))
    ap.add_argument("--min-valu", type=int, default=40, help="smaller blocks are listed only if tagged or holding a VOP2 select on VCC")
    args = ap.parse_args()
    costs = parse_probe(args.probe)
    print(f"# costs: w4 column of {Path(args.probe).name}; unlisted forms ('other'): {OTHER_DEFAULT} cycles", flush=True)
    found = 0
    for f in args.asm:
        if not Path(f).exists():
            print(f"# {f}: missing (make -C pyjpegdecoder_amd/csrc asm)", file=sys.stderr)
            continue
        found += report(f, args.kernel, costs, args.min_valu)
    return 0 if found else 1


if __name__ == "__main__":
    sys.exit(main())
