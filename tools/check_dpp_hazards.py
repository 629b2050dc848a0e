#!/usr/bin/env python3
"""Static check of the gfx950 assembly of a .hip file. Every DPP instruction (v_*_dpp) must
  1. read its DPP operand (src0) at least two wait states after the last VALU instruction that wrote any register of it ("VALU writes
     VGPR -> VALU DPP reads that VGPR" data hazard of the CDNA ISA), and
  2. issue at least five wait states after the last VALU instruction that wrote EXEC (v_cmpx*, or a VALU destination exec*).
The compiler guarantees both for the DPP instructions it emits itself; the hand-written v_fmac_f64_dpp (fmac_bcast of
qpmpc_amd/csrc/mpcqp_lane.h, used by the pair and quad kernels) sit in inline asm, which it cannot see into, and rely on an s_nop placed
by the source (dpp_ready, next to it).

The scan follows the control flow. Per function (a label that does not start with .L, up to the next one) the instructions are cut into
basic blocks: a block starts at every .LBB label and after every s_branch, s_cbranch_* and s_endpgm; its successors are the branch target
and, unless it ends in s_branch / s_endpgm, the block below. The state is, per VGPR, the wait states since its last VALU write
(saturating at 2) and, for EXEC, the same (saturating at 5). A function is entered in the saturated state; a block's in-state is the
element-wise minimum over its predecessors -- the worst predecessor --, iterated to a fixpoint; a block nothing reaches is scanned from
the saturated state. Every instruction is one wait state, s_nop N is N + 1, and a writer's count starts at the instruction after it.
Control flow the scan cannot follow (s_setpc*, s_swappc*, s_call*, a fork, a branch to a label that is no block of the function) in a
function that holds a DPP instruction is a violation of its own kind. The compiler's own DPP instructions (v_mov_*_dpp ...) are held to
the same rules: a flag on one of them would mean that this model is stricter than the hardware's.

usage: check_dpp_hazards.py file.hip [more.hip ...]   (exit status 1 on a violation)"""
import collections, os, re, shutil, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VGPR_WAIT, EXEC_WAIT = 2, 5

# one violation: the function, the instruction's text, the wait states seen, the kind ("vgpr": rule 1, "exec": rule 2, "flow": control
# flow the scan cannot follow), the writer's mnemonic (None for "flow") and the line of the assembly (1-based)
Hazard = collections.namedtuple("Hazard", "func line waited kind writer lineno")


def device_asm(src: str) -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "qpmpc_amd", "csrc"), src, "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(out).read()


def regs(op: str):
    """VGPR numbers named by an operand like v12, v[4:5], -v[4:5], |v3|."""
    m = re.search(r"\bv\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.search(r"\bv(\d+)\b", op)
    return {int(m.group(1))} if m else set()


class _Insn:
    __slots__ = ("op", "line", "lineno", "ws", "written", "exec_write", "src0", "hand", "target", "ends", "opaque")


def _parse(op, ops, line, lineno):
    i = _Insn()
    i.op, i.line, i.lineno = op, line, lineno
    i.ws = int(ops[0], 0) + 1 if op == "s_nop" else 1
    valu = op.startswith("v_")
    i.written = frozenset(regs(ops[0])) if valu and ops and not (op.startswith("v_cmp") and not op.startswith("v_cmpx")) else frozenset()
    if valu and "swap" in op and len(ops) >= 2:
        i.written |= regs(ops[1])  # swaps write both operands
    i.exec_write = valu and (op.startswith("v_cmpx") or bool(ops) and ops[0].startswith("exec"))
    i.src0 = frozenset(regs(ops[1])) if "_dpp" in op and len(ops) >= 2 else None
    i.hand = op.startswith("v_fmac_f64_dpp")
    branch = op == "s_branch" or op.startswith("s_cbranch_")
    i.opaque = op.startswith(("s_setpc", "s_swappc", "s_call", "s_cbranch_g_fork", "s_cbranch_i_fork", "s_cbranch_join"))
    i.target = ops[0] if branch and not i.opaque and ops else None
    i.ends = branch or op == "s_endpgm"  # the next instruction leads a block
    return i


def _functions(asm: str):
    """[(name, [(label or None, [instructions])])]: the blocks of every function, in the order of the text."""
    funcs, blocks, cur = [], None, None
    for lineno, raw in enumerate(asm.split("\n"), 1):
        line = raw.split(";")[0].strip()
        if not line or line.startswith(".") and not line.startswith(".LBB"):
            continue
        if line.endswith(":"):
            if not line.startswith(".L"):
                blocks, cur = [], None
                funcs.append((line[:-1], blocks))
            elif blocks is not None:
                cur = (line[:-1], [])
                blocks.append(cur)
            continue
        if blocks is None:
            blocks, cur = [], None
            funcs.append(("?", blocks))
        if cur is None:
            cur = (None, [])
            blocks.append(cur)
        op, _, rest = line.partition(" ")
        insn = _parse(op, [o.strip() for o in rest.split(",")] if rest.strip() else [], line, lineno)
        cur[1].append(insn)
        if insn.ends:
            cur = None
    return funcs


def _run(block, state, report=None, func=None):
    """The state after `block` entered in `state` = ({vgpr: (wait states, writer)} for the registers below VGPR_WAIT, (wait states,
    writer) of EXEC or None when saturated). With `report`, appends the violations of the block's DPP instructions."""
    vg, ex = dict(state[0]), state[1]
    for i in block:
        if i.src0 is not None and report is not None:
            hit = [vg[r] for r in i.src0 if r in vg]
            if hit:
                w = min(hit)
                report.append(Hazard(func, i.line, w[0], "vgpr", w[1], i.lineno))
            if ex is not None:
                report.append(Hazard(func, i.line, ex[0], "exec", ex[1], i.lineno))
        if vg:
            vg = {r: (c + i.ws, w) for r, (c, w) in vg.items() if c + i.ws < VGPR_WAIT}
        if ex is not None:
            ex = (ex[0] + i.ws, ex[1]) if ex[0] + i.ws < EXEC_WAIT else None
        for r in i.written:
            vg[r] = (0, i.op)
        if i.exec_write:
            ex = (0, i.op)
    return vg, ex


def _meet(a, b):
    """Element-wise minimum of two states (an absent entry is saturated)."""
    vg = dict(a[0])
    for r, cw in b[0].items():
        if r not in vg or cw[0] < vg[r][0]:
            vg[r] = cw
    ex = a[1] if b[1] is None or (a[1] is not None and a[1][0] <= b[1][0]) else b[1]
    return vg, ex


def _counts(s):
    return {r: c for r, (c, _) in s[0].items()}, None if s[1] is None else s[1][0]


def check(asm: str):
    """(violations, DPP instructions, hand-written v_fmac_f64_dpp among them) of an assembly text."""
    bad, ndpp, nasm = [], 0, 0
    for func, blocks in _functions(asm):
        dpp = sum(i.src0 is not None for _, b in blocks for i in b)
        if not dpp:
            continue
        ndpp += dpp
        nasm += sum(i.hand for _, b in blocks for i in b)
        index = {label: k for k, (label, _) in enumerate(blocks) if label is not None}
        succ = []
        for k, (_, b) in enumerate(blocks):
            last, s = b[-1] if b else None, []
            for i in b:
                if i.opaque or i.target is not None and i.target not in index:
                    bad.append(Hazard(func, i.line, None, "flow", None, i.lineno))
            if last is not None and last.target in index:
                s.append(index[last.target])
            if (last is None or last.op not in ("s_branch", "s_endpgm")) and k + 1 < len(blocks):
                s.append(k + 1)
            succ.append(s)
        # worst-predecessor in-states, to a fixpoint (the states only fall, and they are bounded below: it ends)
        top = ({}, None)
        instate = {0: top} if blocks else {}
        work = collections.deque(instate)
        while work:
            k = work.popleft()
            out = _run(blocks[k][1], instate[k])
            for s in succ[k]:
                new = _meet(instate[s], out) if s in instate else out
                if s not in instate or _counts(new) != _counts(instate[s]):
                    instate[s] = new
                    if s not in work:
                        work.append(s)
        for k, (_, b) in enumerate(blocks):
            _run(b, instate.get(k, top), bad, func)
    bad.sort(key=lambda h: h.lineno)
    return bad, ndpp, nasm


def describe(h: Hazard) -> str:
    if h.kind == "flow":
        return f"{h.func[:60]}: line {h.lineno}: '{h.line}' is control flow the scan cannot follow"
    what = "reads its DPP operand" if h.kind == "vgpr" else "issues"
    of = "that register" if h.kind == "vgpr" else "EXEC"
    return f"{h.func[:60]}: line {h.lineno}: '{h.line}' {what} {h.waited} wait state(s) after {h.writer} wrote {of} ({h.kind})"


if __name__ == "__main__":
    files = sys.argv[1:] or [os.path.join(ROOT, "qpmpc_amd", "csrc", "mpcqp_pair.hip")]
    rc = 0
    for f in files:
        bad, ndpp, nasm = check(open(f).read() if f.endswith(".s") else device_asm(f))
        print(f"{os.path.basename(f)}: {ndpp} DPP instructions ({nasm} v_fmac_f64_dpp), {len(bad)} hazard(s)")
        for h in bad[:10]:
            print("  " + describe(h))
        rc |= bool(bad)
    sys.exit(rc)
