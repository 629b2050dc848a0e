#!/usr/bin/env python3
"""Census of the STEADY LOOP of the four-per-wavefront kernel (csrc/mpcqp_quad_steady.h) in gfx950 assembly (no GPU).

    python tools/quad_steady_census.py [--asm file.s] [--kernel SUBSTRING] [--list]

The loop is found by what identifies it: the shortest span of the kernel's text that a backward branch closes (label ... branch to that
label) and that holds exactly 103 FMAs -- a plain trip's 32 of the update, 16 + 16 of the two dot products, 32 of the row's two
products with -z, 5 of the reciprocal, 2 of the slacks. Printed: the span's instructions by the classes of tools/quad_census.py, the s_nop and
s_waitcnt inside it, and the ballot round trips (a v_cndmask_b32 of 0 and 1 under a lane mask whose only reader is a v_cmp_ne_u32
against 0: a lane mask turned into a register and back). --list prints the span with offsets from its header."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools import quad_census as QC

STEADY_FMAS, STEADY_LDS = 103, 12
PARENT_TOTAL = 257  # profiles/quad_excursions.md: the loop before the lane-mask arithmetic


def functions(text: str) -> dict:
    """{mangled name: [(label or None, mnemonic, operands)]}: the instructions of every function in text order, each with the .LBB
    label that stands in front of it"""
    out, cur, label = {}, None, None
    for raw in text.split("\n"):
        line = raw.split(";")[0].strip()
        if not line:
            continue
        m = re.match(r"^(_Z\w+):$", line)
        if m:
            cur, label = out.setdefault(m.group(1), []), None
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and re.match(r"^\.LBB\w+:$", line):
            label = line[:-1]
        elif cur is not None and not line.startswith(".") and not line.endswith(":"):
            mn, _, ops = line.partition(" ")
            cur.append((label, mn.strip(), ops.strip()))
            label = None
    return out


def steady_loop(insts):
    """(first, last) instruction indices of the steady loop: the shortest backward-branch span with STEADY_FMAS FMAs; None if absent"""
    at = {lab: i for i, (lab, _, _) in enumerate(insts) if lab}
    best = None
    for i, (_, mn, ops) in enumerate(insts):
        if mn.startswith(("s_cbranch", "s_branch")) and ops in at and at[ops] <= i:
            lo = at[ops]
            if sum(QC.classify(m) == "FMA" for _, m, _ in insts[lo:i + 1]) == STEADY_FMAS and (best is None or i - lo < best[1] - best[0]):
                best = (lo, i)
    return best


def _sregs(op: str):
    m = re.search(r"\bs\[(\d+):(\d+)\]", op)
    return set(range(int(m.group(1)), int(m.group(2)) + 1)) if m else set()


def _vregs(op: str):
    m = re.search(r"\bv\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return {int(x) for x in re.findall(r"\bv(\d+)\b", op)}


def round_trips(span):
    """indices (into span) of every `v_cndmask_b32 vX, 0, 1, <lane mask>` whose value is read, before vX is written again, by nothing
    but one `v_cmp_ne_u32 <mask>, 0, vX`"""
    out = []
    for i, (_, mn, ops) in enumerate(span):
        o = [x.strip() for x in ops.split(",")]
        if not (mn.startswith("v_cndmask_b32") and len(o) == 4 and o[1] == "0" and o[2] == "1" and (_sregs(o[3]) or o[3] == "vcc")):
            continue
        reg, readers = _vregs(o[0]), []
        for _, mn2, ops2 in span[i + 1:]:
            o2 = [x.strip() for x in ops2.split(",")]
            dst_only = mn2.startswith("v_") and not mn2.startswith("v_cmp")
            srcs = o2[1:] if dst_only else o2
            if any(_vregs(x) & reg for x in srcs):
                readers.append((mn2, o2))
            if dst_only and o2 and _vregs(o2[0]) & reg:
                break
        if len(readers) == 1 and readers[0][0].startswith("v_cmp_ne_u32") and readers[0][1][1] == "0":
            out.append(i)
    return out


def census(insts):
    """dict(total, classes {class: count}, nops, waits, round_trips) of the steady loop of one kernel's instructions; None if absent"""
    found = steady_loop(insts)
    if found is None:
        return None
    span = insts[found[0]:found[1] + 1]
    classes = dict.fromkeys(QC.CLASSES, 0)
    for _, mn, _ in span:
        classes[QC.classify(mn)] += 1
    return dict(total=len(span), classes=classes, header=span[0][0], span=span, nops=classes["nop"], waits=classes["wait"],
                round_trips=round_trips(span))


def main(argv) -> int:
    pick, text, listing = QC.HEADLINE, None, "--list" in argv
    args = [a for a in argv if a != "--list"]
    while args:
        a = args.pop(0)
        if a == "--kernel":
            pick = args.pop(0)
        elif a == "--asm":
            text = open(args.pop(0)).read()
    funcs = functions(text if text is not None else QC.assembly("mpcqp_quad.hip"))
    names = QC.demangle(list(funcs))
    for mangled, insts in funcs.items():
        if pick not in names[mangled]:
            continue
        c = census(insts)
        if c is None:
            print(f"## {names[mangled]}: no steady loop")
            continue
        print(f"## {names[mangled]}: steady loop at {c['header']}, {c['total']} instructions, {len(c['round_trips'])} ballot round trips")
        print("   " + ", ".join(f"{k} {v}" for k, v in c["classes"].items() if v))
        if listing:
            for i, (lab, mn, ops) in enumerate(c["span"]):
                print(f"   +{i:3d} {'*' if i in c['round_trips'] else ' '} {mn} {ops}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
