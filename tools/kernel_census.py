#!/usr/bin/env python3
"""Join the per-kernel call counts of a kernel trace with the census of the kernels that carry hand-written DPP instructions
(tests/dpp_instantiations.py: census() from the gfx950 assembly of the five units, MANIFEST the launch that reaches each).

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python -m pytest tests/test_gpu_dpp_instantiations.py -q -m gpu
    python tools/kernel_census.py DIR [--asm ASMDIR] > profiles/dpp_instantiations.txt

reads every *kernel_stats.csv below DIR (one per traced process; columns Name, Calls), sums the calls per kernel and writes one row per
census kernel: unit, kernel, hand-written v_fmac_f64_dpp, calls. Exit status 1 if a kernel whose recipe is not marked unreachable has
no call. --asm: take <unit>.s from ASMDIR instead of compiling the units here (minutes)."""
import csv
import glob
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)  # (dpp_instantiations imports tools.check_dpp_hazards)


def trace_name(name: str) -> str:
    """'void mpcqp::mpcqp_quad_kernel<16, false, 1, true, false, true>(double const*, ...) [clone .kd]' -> the census' name"""
    name = re.sub(r"\s*\[clone[^\]]*\]|\.kd$", "", name.strip())
    name = re.sub(r"^void\s+", "", name)
    depth, cut = 0, len(name)
    for i, c in enumerate(name):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            cut = i
            break
    return name[:cut].replace("mpcqp::", "")


def calls_of(directory: str) -> dict:
    calls, files = {}, sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    for f in files:
        for row in csv.DictReader(open(f)):
            k = trace_name(row["Name"])
            calls[k] = calls.get(k, 0) + int(row["Calls"])
    return calls, files


def main(argv) -> int:
    import dpp_instantiations as DI

    if "--asm" in argv:
        at = argv.index("--asm")
        asmdir = argv[at + 1]
        argv = argv[:at] + argv[at + 2:]
        census = {}
        for unit in DI.UNITS:
            for name, count in DI.census_of(open(os.path.join(asmdir, unit.replace(".hip", ".s"))).read()).items():
                census[name] = (unit, count)
    else:
        census = DI.census()
    calls, files = calls_of(argv[0])
    print(f"# rocprofv3 --kernel-trace --stats -- python -m pytest tests/test_gpu_dpp_instantiations.py -q -m gpu ({len(files)} stats file(s)),")
    print("# joined with the census of tests/dpp_instantiations.py by tools/kernel_census.py: unit, kernel, hand-written v_fmac_f64_dpp, calls")
    missing = 0
    for name, (unit, count) in sorted(census.items(), key=lambda kv: (kv[1][0], kv[0])):
        recipe = DI.MANIFEST.get(name, {})
        n = calls.get(name, 0)
        note = "  unreachable: " + recipe["site"] if recipe.get("unreachable") else "  NO CALL" if n == 0 else ""
        missing += n == 0 and not recipe.get("unreachable")
        print(f"{unit:16s} {name:58s} {count:5d} {n:6d}{note}")
    reach = sum(1 for k in census if not DI.MANIFEST.get(k, {}).get("unreachable"))
    print(f"# {len(census)} kernels, {sum(c for _, c in census.values())} hand-written v_fmac_f64_dpp; {reach - missing} of {reach} reachable kernels called")
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
