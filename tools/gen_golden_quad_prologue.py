#!/usr/bin/env python3
"""Fixture generator (the recording needs a GPU; no reference code involved): tests/golden/quad_prologue_parent.npz -- the operands of
small problem sets that reach every path of the four-per-wavefront kernel's PROLOGUE (csrc/mpcqp_quad.hip: the operand loads and the
chain of the build) and of its refinement / acceptance block, and what the kernel computed for them, U, lam, status and iters, recorded
from the build of the commit BEFORE the operand loads went to the top of the kernel and the chain's sums were interleaved. tests/test_gpu_quad_parent_bits.py holds the kernel to these bits.
What the four fixtures of this kind share is tools/quad_parent_bits.py; the mixed family is qpmpc_amd/workloads.py's mixed_family.

Sets (LAUNCHES; every launch forced through MPCQP_OPT_FOUR_PER_WAVE; at most 32 problems each):
  shared16      lean build, (nx, nu, N, mk) = (3, 1, 16, 2), the triple integrator with every operand shared and time-invariant (all
                strides 0: the loads read one address for every step)
  a_step16      lean, A per step and C time-invariant (tests/operand_layouts.py: make()), five problems
  c_step16      lean, A time-invariant and C per step, five problems
  tight16       lean, 32 problems of the mixed family (tight, loose and inconsistent rows in every wavefront): the set of the refinement
                block. Its probe record (slot 14 of the developer probe: the kernel's `fails`) is stored as `tight16__fails`
  tight16_pad   its first 16 problems behind padded batch strides (PADS: another odd or even number of elements per operand)
  tight16_cut5, tight16_cut7   its first five / seven problems: a ragged last wavefront, idle rows
  lean1, lean2, lean15   lean, N = 1, 2, 15: the clamped loads (a load may never reach past step N - 1), eight problems each
  nx2, nx4      lean, nx = 2 and 4 at N = 16: four and six accumulators per step of the chain
  gen_mk1, gen_mk3, gen_mk4   general build, (3, 1, 16, 1), (3, 1, 10, 3), (3, 1, 8, 4) with D rows and a stage cost
  gen_nx5, gen_nx6   general build, (5, 1, 16, 2) and (6, 1, 16, 2): three / four operand registers per step, four problems each

tight16 runs under feas_tol = TIGHT_TOL (see there); every other set under the default tolerance.

Passes. The recording (no argument, or --seed K) runs on the build that is to be recorded (MPCQP_LIB names its library): it draws
seeds until the probe shows a problem of tight16 that failed an acceptance test once (or takes seed K), records every set twice (equal
bits required) and writes the fixture with `refinements` = -1. Whether a problem took the refinement arm shows only in a PROBE BUILD of
the kernel (hipcc flag -DQUAD_PROBE_REFINE=1: bit 24 of slot 14; build_library(force=True, extra_flags=["-DQUAD_PROBE_REFINE=1"]),
the library copied aside and named by MPCQP_LIB; the shipped build leaves the mark out, it costs registers). Two passes run on it:
--search, before the recording, prints the first seed whose tight16 shows both a failed acceptance test and a problem whose last
acceptance test stood behind the refinement arm; --refinements, after it, requires the recorded bits of tight16 from the probe build,
counts those problems, requires at least one and stores the count. The CPU test asserts both again from the stored arrays."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import tools.quad_parent_bits as H

PATH = os.path.join(ROOT, "tests", "golden", "quad_prologue_parent.npz")
# elements past the packed batch stride, per operand (those of tests/operand_layouts.py)
PADS = dict(A=2, B=3, C=7, e=5, x0=1, goal=6)
PAD_COUNT = 16
SMALL = 8
# the tight set's feasibility tolerance, far below the default (1e-12): at the default the acceptance test never failed in 200 draws of
# 32 problems; at this one a row that is violated by rounding alone is taken up, and the acceptance test behind it can fail
TIGHT_TOL = 1e-15
LAUNCHES = {  # (every set but tight16's four runs on operands of its own, as it is)
    **{name: H.Launch(name) for name in ("shared16", "a_step16", "c_step16")},
    "tight16": H.Launch("tight16", feas_tol=TIGHT_TOL),
    "tight16_pad": H.Launch("tight16", cut=PAD_COUNT, pads=PADS, feas_tol=TIGHT_TOL),
    "tight16_cut5": H.Launch("tight16", cut=5, feas_tol=TIGHT_TOL),
    "tight16_cut7": H.Launch("tight16", cut=7, feas_tol=TIGHT_TOL),
    **{name: H.Launch(name) for name in ("lean1", "lean2", "lean15", "nx2", "nx4", "gen_mk1", "gen_mk3", "gen_mk4", "gen_nx5", "gen_nx6")},
}
SETS = tuple(LAUNCHES)
OPERAND_SETS = tuple(dict.fromkeys(spec.on for spec in LAUNCHES.values()))


def probed(sets):
    """tight16's outputs and probe record"""
    return H.solve(sets["tight16"], probe=True, feas_tol=TIGHT_TOL)


def fails_of(probe):
    """the kernel's count of failed acceptance tests per problem, from slot 14 of its probe record"""
    return ((probe[:, 14] >> 8) & 0xFF).astype(np.int64)


def refined_of(probe):
    """true for the problems whose last acceptance test stood behind a pass through the refinement arm (bit 24 of slot 14)"""
    return ((probe[:, 14] >> 24) & 1) > 0


def layout_case(per_step, seed):
    """five problems of tests/operand_layouts.py's lean route with `per_step` ("A" or "C") per step and the other one time-invariant"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import operand_layouts as OL

    lay = dict(A="b1", B="bn", C="b1", D="bn", e="bn", goal="b", targets="b")
    lay[per_step] = "bn"
    w, _ = OL.make((3, 1, 16, 2), "c", False, lay, seed, 0.2)
    return H.cut(w, 5)


def draw(seed):
    from qpmpc_amd import workloads as W

    rng = np.random.default_rng(20261101 + seed)
    sets = {"tight16": W.mixed_family(rng, 32, 3, 1, 16, 2, False)}
    sets["shared16"] = W.triple_integrator_batch(SMALL, seed=20261101 + seed, heterogeneous=False)
    sets["shared16"]["x0"] = 2.0 * sets["shared16"]["x0"]  # (twice the benchmark's range: more rows bind)
    sets["a_step16"] = layout_case("A", 24100 + seed)
    sets["c_step16"] = layout_case("C", 24200 + seed)
    for N in (1, 2, 15):
        sets[f"lean{N}"] = W.mixed_family(rng, SMALL, 3, 1, N, 2, False)
    sets["nx2"] = W.mixed_family(rng, SMALL, 2, 1, 16, 2, False)
    sets["nx4"] = W.mixed_family(rng, SMALL, 4, 1, 16, 2, False)
    sets["gen_mk1"] = W.mixed_family(rng, SMALL, 3, 1, 16, 1, True)
    sets["gen_mk3"] = W.mixed_family(rng, SMALL, 3, 1, 10, 3, True)
    sets["gen_mk4"] = W.mixed_family(rng, SMALL, 3, 1, 8, 4, True)
    sets["gen_nx5"] = W.mixed_family(rng, 4, 5, 1, 16, 2, True)
    sets["gen_nx6"] = W.mixed_family(rng, 4, 6, 1, 16, 2, True)
    for name, w in sets.items():
        w.pop("name", None)
    return sets


def search(refinements):
    """(seed, sets, tight16's outputs and probe record) of the first draw whose tight16 shows a failed acceptance test -- and, on a
    build that counts them (`refinements`), a problem that took the refinement arm"""
    for seed in range(400):
        sets = draw(seed)
        res = probed(sets)
        fails, took = fails_of(res[4]), refined_of(res[4])
        print("seed", seed, "statuses", np.bincount(res[2], minlength=4), "problems with a failed acceptance test", int((fails > 0).sum()),
              "with a refinement", int(took.sum()), flush=True)
        if (fails > 0).any() and (res[2] == 0).sum() >= 8 and (took.any() or not refinements):
            return seed, sets, res
    raise SystemExit("no seed gave a failed acceptance test" + (" and a refinement" if refinements else ""))


def fixture():
    """(launches, operand dictionaries by set, recorded outputs by launch, failed acceptance tests per problem of tight16, problems of
    tight16 that took the refinement arm) of the stored fixture"""
    z = np.load(PATH)
    return (LAUNCHES,) + H.unpack(z, OPERAND_SETS, SETS) + (z["tight16__fails"], int(z["refinements"]))


def main(seed=None):
    if seed is None:
        seed, sets, res = search(False)
    else:
        sets = draw(seed)
        res = probed(sets)
    fails = fails_of(res[4])
    assert (fails > 0).any()
    results = H.record(lambda name: H.run(LAUNCHES[name], sets), SETS)
    assert tuple(a.tobytes() for a in res[:4]) == tuple(a.tobytes() for a in results["tight16"]), "the probe changes the outputs"
    for name in ("tight16_pad", "tight16_cut5", "tight16_cut7"):  # (a row's arithmetic: its own)
        for a, b in zip(results[name], results["tight16"]):
            assert a.tobytes() == b[:LAUNCHES[name].cut].tobytes(), name
    H.report(results)
    np.savez_compressed(PATH, **H.pack(sets, results, seed=np.int64(seed), tight16__fails=fails, refinements=np.int64(-1)))
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
    assert os.path.getsize(PATH) < 200 * 1024


def count_refinements():
    z = np.load(PATH)
    _, sets, results, fails, _ = fixture()
    res = probed(sets)
    for k, a, b in zip(H.OUTPUTS, res, results["tight16"]):
        assert a.tobytes() == b.tobytes(), f"tight16: {k} is not the recorded one"
    assert np.array_equal(fails_of(res[4]), fails), "the probe's record of failed acceptance tests is not the recorded one"
    took = refined_of(res[4])
    print("problems of tight16 that took the refinement arm:", int(took.sum()), "; failed an acceptance test:", int((fails > 0).sum()))
    assert took.any() and (fails > 0).any(), "no refinement mark: is MPCQP_LIB a probe build (-DQUAD_PROBE_REFINE=1)?"
    np.savez_compressed(PATH, **{**{k: z[k] for k in z.files}, "refinements": np.int64(took.sum())})
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    if "--search" in sys.argv:  # (on a build that counts refinements: the seed for --seed on the build to be recorded)
        print("found", search(True)[0])
    elif "--refinements" in sys.argv:
        count_refinements()
    else:
        main(int(sys.argv[sys.argv.index("--seed") + 1]) if "--seed" in sys.argv else None)
