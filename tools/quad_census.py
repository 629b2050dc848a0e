#!/usr/bin/env python3
"""Instruction census of a kernel unit between the developer probe's stamps (no GPU: hipcc cross-compiles).

    python tools/quad_census.py [unit.hip | --asm file.s] [--kernel SUBSTRING] [--all]

compiles qpmpc_amd/csrc/<unit> (default mpcqp_quad.hip) to gfx950 assembly, as build.py compiles it, and prints for every kernel
(--kernel: those whose demangled name contains SUBSTRING; default: the lean roomy instantiation of the headline,
`mpcqp_quad_kernel<3, false, 1, false, false, false>`; --all: every kernel) the instructions of each segment of the text between two
stamps of the probe, by class. A stamp is a read of the shader clock (the probe's tick(): a mnemonic of the s_memtime family); its slot
is taken from the offset of the store behind it. The segments follow the TEXT: a block the compiler moved elsewhere is counted where it
stands, and both arms of a branch are counted. Classes are generic mnemonic prefixes:

    FMA       v_fma*, v_fmac*, v_mfma*          other f64  any other v_*_f64
    LDS       ds_*                              global load / global store   global_*, flat_*, buffer_*, scratch_* by direction
    wait      s_waitcnt*                        nop        s_nop
    branch    s_cbranch*, s_branch, s_setpc, s_endpgm   scalar   any other s_*
    move      v_mov*, v_accvgpr*, v_readlane*, v_readfirstlane*, v_writelane*   select  v_cndmask*   compare  v_cmp*
    integer   any other v_*

Two derived figures per kernel: the instructions from the kernel's entry to its LAST global load in front of stamp 8 (the build's
operand loads are requested by then), and, in the chain (stamp 9 to stamp 10), the s_nop that stand between two FMAs."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLASSES = ("FMA", "other f64", "LDS", "global load", "global store", "wait", "nop", "branch", "scalar", "move", "select", "compare",
           "integer")
HEADLINE = "mpcqp_quad_kernel<3, false, 1, false, false, false>"
_MEM = ("global_", "flat_", "buffer_", "scratch_")
_MOVES = ("v_mov", "v_accvgpr", "v_readlane", "v_readfirstlane", "v_writelane")


def classify(mn: str) -> str:
    if mn.startswith(("v_fma", "v_fmac", "v_mfma")):
        return "FMA"
    if mn.startswith("v_cmp"):
        return "compare"
    if mn.startswith("v_cndmask"):
        return "select"
    if mn.startswith(_MOVES):
        return "move"
    if mn.startswith("v_"):
        return "other f64" if "_f64" in mn else "integer"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(_MEM):
        return "global load" if "_load" in mn else "global store"
    if mn.startswith("s_waitcnt"):
        return "wait"
    if mn == "s_nop":
        return "nop"
    if mn.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
        return "branch"
    return "scalar"


def is_stamp(mn: str) -> bool:
    return mn.startswith("s_memtime")


def assembly(unit: str) -> str:
    from qpmpc_amd import build as B

    src = unit if os.path.exists(unit) else os.path.join(ROOT, "qpmpc_amd", "csrc", unit)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        subprocess.check_call([B._hipcc(), *B.FLAGS, "-S", "--cuda-device-only", "-I" + os.path.join(ROOT, "include"),
                               "-I" + os.path.join(ROOT, "qpmpc_amd", "csrc"), src, "-o", out], stderr=subprocess.DEVNULL)
        return open(out).read()


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return {n: re.sub(r"^void\s+|mpcqp::|\(.*$", "", d) for n, d in zip(names, out)}
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(text: str) -> dict:
    """{mangled name: [(mnemonic, operands)]} of every function of the assembly text, in text order"""
    out, cur = {}, None
    for raw in text.split("\n"):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = re.match(r"^(_Z\w+):$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and not line.startswith(".") and not line.endswith(":"):
            mn, _, ops = line.partition(" ")
            cur.append((mn.strip(), ops.strip()))
    return out


def segments(insts):
    """[(label, [instruction indices])]: entry -> first stamp, stamp -> stamp, last stamp -> end; a stamp's slot is the offset of the
    first store behind it, in doubles"""
    marks = []
    for i, (mn, _) in enumerate(insts):
        if is_stamp(mn):
            slot = None
            for mn2, ops2 in insts[i + 1:i + 10]:
                if classify(mn2) == "global store":
                    m = re.search(r"offset:(\d+)", ops2)
                    slot = (int(m.group(1)) if m else 0) // 8
                    break
            marks.append((i, slot))
    out, lo, name = [], 0, "entry"
    for i, slot in marks:
        out.append((f"{name} -> stamp {slot}", list(range(lo, i))))
        lo, name = i + 1, f"stamp {slot}"
    out.append((f"{name} -> end", list(range(lo, len(insts)))))
    return out


def census(insts):
    """([(label, {class: count}, total)], instructions from the entry to the last global load in front of stamp 8 (None: no such stamp),
    s_nop between two FMAs in the chain (None: no chain segment))"""
    rows, to_loads, chain_nops = [], None, None
    for label, idx in segments(insts):
        counts = dict.fromkeys(CLASSES, 0)
        for i in idx:
            counts[classify(insts[i][0])] += 1
        rows.append((label, counts, len(idx)))
        if label.endswith("-> stamp 8") and to_loads is None:
            loads = [i for i in range(idx[-1] + 1 if idx else 0) if classify(insts[i][0]) == "global load"]
            to_loads = (loads[-1] + 1, len(loads)) if loads else (0, 0)
        if label == "stamp 9 -> stamp 10":
            chain_nops = sum(1 for a, b, c in zip(idx, idx[1:], idx[2:]) if classify(insts[b][0]) == "nop"
                             and classify(insts[a][0]) == "FMA" and classify(insts[c][0]) == "FMA")
    return rows, to_loads, chain_nops


def report(name, insts):
    rows, to_loads, chain_nops = census(insts)
    print(f"## {name}: {len(insts)} instructions")
    print(f"{'segment':24s} {'total':>6s} " + " ".join(f"{c:>12s}" for c in CLASSES))
    for label, counts, total in rows:
        print(f"{label:24s} {total:6d} " + " ".join(f"{counts[c]:12d}" for c in CLASSES))
    if to_loads is not None:
        print(f"entry -> last global load in front of stamp 8: {to_loads[0]} instructions ({to_loads[1]} global loads)")
    if chain_nops is not None:
        print(f"chain (stamp 9 -> stamp 10): {chain_nops} s_nop between two FMAs")
    print()


def main(argv) -> int:
    pick, everything, unit, text = HEADLINE, "--all" in argv, "mpcqp_quad.hip", None
    args = [a for a in argv if a != "--all"]
    while args:
        a = args.pop(0)
        if a == "--kernel":
            pick = args.pop(0)
        elif a == "--asm":
            text = open(args.pop(0)).read()
        else:
            unit = a
    funcs = kernels(text if text is not None else assembly(unit))
    names = demangle(list(funcs))
    shown = 0
    for mangled, insts in funcs.items():
        if everything or pick in names[mangled]:
            report(names[mangled], insts)
            shown += 1
    if not shown:
        print("no kernel matches", repr(pick), "among", sorted(names.values()))
    return 0 if shown else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
