#!/usr/bin/env python3
"""Fixture generator (the recording needs a GPU; no reference code involved): tests/golden/quad_drops_parent.npz -- the operands of a
few small problem sets in which rows DROP constraints, and what the four-per-wavefront kernel (csrc/mpcqp_quad.hip) computed for them,
U, lam, status and iters, recorded from the build of the commit BEFORE the kernel finished a non-plain trip once, dropped inside the
partial step's trip and returned to its steady loop. tests/test_gpu_quad_parent_bits.py holds the kernel to these bits,
tests/test_quad_drops_cpu.py holds the fixture to its conditions (no GPU). What the four fixtures of this kind share is
tools/quad_parent_bits.py.

Sets (launches(); every launch forced through MPCQP_OPT_FOUR_PER_WAVE):
  model        shared-model mode, the humanoid model, 64 initial states of twice the sweep's range
  lean16       lean build, (nx, nu, N, mk) = (3, 1, 16, 2), 64 problems of the mixed family (qpmpc_amd/workloads.py: mixed_family)
  gen12        general build, (4, 1, 12) with state and input rows and a stage cost, 32 problems
  lean16_slim  lean16 tiled to 4100: more wavefronts than SIMDs, the slim LDS carve; every tile must give the same bits, 64 are stored
  lean16_mi    lean16 under the iteration limit `max_iter` (stored) that falls, for the most rows, on the trip right after a partial step
The seeds are drawn on the CPU until the trip model (tools/quad_trip_model.py), run on the operands, shows conditions() below; the
recording then runs every set twice and requires equal bits, and requires that the model's iteration counts are the recorded ones for
every solved problem."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import tools.quad_parent_bits as H
import tools.quad_trip_model as TM

PATH = os.path.join(ROOT, "tests", "golden", "quad_drops_parent.npz")
SLIM_BATCH = 4100
OPERAND_SETS = ("model", "lean16", "gen12")


def launches(max_iter):
    """the table of launches, lean16_mi under the fixture's iteration limit"""
    return {
        "model": H.Launch("model", model=True),
        "lean16": H.Launch("lean16"),
        "gen12": H.Launch("gen12"),
        "lean16_slim": H.Launch("lean16", tile=SLIM_BATCH, stored=64),
        "lean16_mi": H.Launch("lean16", max_iter=max_iter),
    }


SETS = tuple(launches(None))


def model_trips(sets, max_iter=None):
    """{set: [(iters, status, kinds)]} of the trip model on the stored operands"""
    table = launches(None)
    return {name: TM.trips_of_workload(H.workload(table[name], sets), max_iter=max_iter) for name in OPERAND_SETS}


def limit_after_partial(trips):
    """the iteration limit that stops the most rows on the trip right after a partial step, and how many"""
    count = {}
    for _, _, kinds in trips:
        for k, c in enumerate(kinds):
            if c == "d" and k + 1 < len(kinds):
                count[k + 1] = count.get(k + 1, 0) + 1
    best = max(count, key=lambda k: (count[k], -k))
    return best, count[best]


def _live(wf, t):
    return [k[t] for k in wf if t < len(k)]


def conditions(trips):
    """what the model must show on the operand sets together (the names of the conditions that FAIL)"""
    kinds = [k for name in OPERAND_SETS for _, _, k in trips[name]]
    waves = [wf for name in OPERAND_SETS for wf in TM.wavefronts(trips[name])]
    ret = same = consecutive = alone = False
    for wf in waves:
        T = max(len(k) for k in wf)
        live = [_live(wf, t) for t in range(T)]
        plain = [bool(v) and all(c == "P" for c in v) for v in live]
        first = min((k.find("d") for k in wf if "d" in k), default=-1)
        if 0 <= first < 3:  # a drop within the first three trips, later eight plain trips in a row: the return to the steady loop
            run = 0
            for t in range(first + 1, T):
                run = run + 1 if plain[t] else 0
                ret |= run >= 8
        nd = [v.count("d") for v in live]
        same |= any(c >= 2 for c in nd)
        for t in range(T - 1):  # partial steps of two DIFFERENT rows in consecutive trips
            a = {i for i, k in enumerate(wf) if t < len(k) and k[t] == "d"}
            b = {i for i, k in enumerate(wf) if t + 1 < len(k) and k[t + 1] == "d"}
            consecutive |= any(i != j for i in a for j in b)
        for i, k in enumerate(wf):  # a row drops while the other three are done
            others = max(len(o) for j, o in enumerate(wf) if j != i)
            alone |= any(c == "d" and t >= others for t, c in enumerate(k))
    checks = {
        "six problems with a drop": sum("d" in k for k in kinds) >= 6,
        "two problems with two drops": sum(k.count("d") >= 2 for k in kinds) >= 2,
        "a drop within three trips, then eight plain trips of the wavefront": ret,
        "two rows of a wavefront in partial steps in the same trip": same,
        "two rows of a wavefront in partial steps in consecutive trips": consecutive,
        "a row drops while the other three are done": alone,
    }
    return [k for k, ok in checks.items() if not ok]


def draw(seed):
    from qpmpc_amd import workloads as W

    rng = np.random.default_rng(20261020 + seed)
    return {
        "model": {"x0": 2.0 * W.humanoid_batch(64, seed=20261020 + seed)["x0"]},
        "lean16": W.mixed_family(rng, 64, 3, 1, 16, 2, False),
        "gen12": W.mixed_family(rng, 32, 4, 1, 12, 2, True),
    }


def search(limit=400, verbose=True):
    """(seed, sets, trips) of the first seed whose operands satisfy conditions()"""
    for seed in range(limit):
        sets = draw(seed)
        trips = model_trips(sets)
        failed = conditions(trips)
        if verbose:
            print("seed", seed, "drops", {n: sum("d" in k for _, _, k in trips[n]) for n in OPERAND_SETS}, "fails:", failed, flush=True)
        if not failed:
            return seed, sets, trips
    raise SystemExit("no seed satisfied the conditions")


def fixture():
    """(launches, operand dictionaries by set, recorded outputs by launch, the iteration limit of lean16_mi) of the stored fixture"""
    z = np.load(PATH)
    max_iter = int(z["max_iter"])
    return (launches(max_iter),) + H.unpack(z, OPERAND_SETS, SETS) + (max_iter,)


def model_disagreements(sets, results, max_iter):
    """[(set, problem, model iters, recorded iters)] over the SOLVED problems of every recorded set"""
    bad = []
    full = model_trips(sets)
    cut = TM.trips_of_workload(sets["lean16"], max_iter=max_iter)
    for name in SETS:
        trips = cut if name == "lean16_mi" else full[{"lean16_slim": "lean16"}.get(name, name)]
        status, iters = results[name][2], results[name][3]
        bad += [(name, b, trips[b][0], int(iters[b])) for b in range(len(iters)) if status[b] == 0 and trips[b][0] != iters[b]]
    return bad


def main():
    seed, sets, trips = search()
    max_iter, rows = limit_after_partial(trips["lean16"])
    print(f"seed {seed}; max_iter {max_iter} stops {rows} rows of lean16 right after a partial step")
    if "--search" in sys.argv:
        return
    table = launches(max_iter)
    results = H.stored(table, H.record(lambda name: H.run(table[name], sets), SETS))
    H.report(results)
    bad = model_disagreements(sets, results, max_iter)
    assert not bad, bad
    np.savez_compressed(PATH, **H.pack(sets, results, seed=np.int64(seed), max_iter=np.int64(max_iter)))
    print("wrote", PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
