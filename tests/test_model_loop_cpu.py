"""CPU tests (no GPU) of the closed loop of a shared model: the export's declaration and binding, its refusal and EINVAL codes
through the export itself, the conditions the seeded cases of tests/model_loop_cases.py promise (checked with the oracle
loop), and the NumPy restatement of the warm period against the cold oracle loop.

The refusal replay runs in a process of its own that hides every device from the runtime before the library is loaded, like
tests/test_refusal_codes.py: its pointers are placeholders, and a launch that is wrongly served fails in the runtime."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import model_loop_cases as MC
import model_loop_np as ML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_export_is_declared_and_bound_and_the_abi_is_12():
    from qpmpc_amd import _capi

    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert re.search(r"^int mpcqp_model_periods_batch\(", header, re.M)
    for struct in ("MpcqpLoopPlant", "MpcqpLoopOut"):
        assert f"}} {struct};" in header
    assert "#define MPCQP_ABI_VERSION 12" in header and _capi.ABI_VERSION == 12
    assert "mpcqp_model_periods_batch" in _capi.EXPORTS
    assert [f[0] for f in _capi.LoopPlant._fields_] == ["A", "B", "d"]
    assert [f[0] for f in _capi.LoopOut._fields_] == ["X", "U0", "loop_stats"]


_REPLAY = r"""
import os, sys, json
for v in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
    os.environ[v] = "-1"
sys.path.insert(0, sys.argv[1])
import ctypes as C
from qpmpc_amd import _capi
lib = _capi.load()
P = 0x1000  # a pointer that is not NULL; never dereferenced by the host
F64, F32 = 0, 1
def call(nx=3, nu=1, N=16, mk=2, dtype=F64, flags=5, batch=8, nperiods=2, warm=0, oflags=0, warm_state=False, order=False,
         model=P, plant=True, A=P, B=P, states=P, goal=P, targets=None, U=P, status=P, opts=True, out=True):
    d = _capi.Dims(nx, nu, N, mk, dtype, flags, 1.0, 0.0, 1e-6)
    pl = _capi.LoopPlant(_capi.Operand(A, 0, 0), _capi.Operand(B, 0, 0), _capi.Operand(None, 0, 0))
    o = _capi.SolveOpts()
    o.flags = oflags
    if warm_state:
        o.warm_state, o.warm_state_bytes = P, 1 << 40
    if order:
        o.order = P
    g, t = _capi.Operand(goal, 0, 0), _capi.Operand(targets, 0, 0)
    lo = _capi.LoopOut(None, None, None)
    return lib.mpcqp_model_periods_batch(C.byref(d), model, C.byref(pl) if plant else None, states, C.byref(g), C.byref(t),
                                         batch, nperiods, warm, C.byref(o) if opts else None, U, None, status, None,
                                         C.byref(lo) if out else None, None)
rows = json.loads(sys.argv[2])
print(json.dumps([call(**kw) for kw in rows]))
"""

EINVAL, EUNSUPPORTED = -1, -6
# (arguments, code): the envelope of include/mpcqp.h; flags 5 = terminal cost (P and q), 15 = terminal + stage
REFUSALS = [
    (dict(nperiods=0), EINVAL), (dict(nperiods=-3), EINVAL), (dict(batch=-1), EINVAL), (dict(model=None), EINVAL),
    (dict(plant=False), EINVAL), (dict(A=None), EINVAL), (dict(B=None), EINVAL), (dict(states=None), EINVAL),
    (dict(U=None), EINVAL), (dict(status=None), EINVAL), (dict(goal=None), EINVAL), (dict(flags=15, targets=None), EINVAL),
    (dict(nperiods=0, dtype=1), EINVAL),  # (validation comes first)
    (dict(dtype=1), EUNSUPPORTED),                    # float32
    (dict(N=17), EUNSUPPORTED),                       # n = 17
    (dict(nu=2, N=9, mk=1), EUNSUPPORTED),            # n = 18
    (dict(N=16, mk=3), EUNSUPPORTED),                 # m = 48
    (dict(mk=0), EUNSUPPORTED),                       # no rows
    (dict(nx=17, N=4), EUNSUPPORTED),                 # nx = 17
    (dict(warm_state=True), EUNSUPPORTED), (dict(order=True), EUNSUPPORTED),
] + [(dict(oflags=1 << b), EUNSUPPORTED) for b in range(15)] + [
    (dict(oflags=1, nperiods=0), EINVAL),             # validate, then refusal()
    (dict(oflags=1, N=17), EUNSUPPORTED),
]


def test_refusal_and_einval_codes_through_the_export():
    rows = [kw for kw, _ in REFUSALS]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _REPLAY, ROOT, json.dumps(rows)], check=True, timeout=120, env=env,
                         capture_output=True, text=True)
    got = json.loads(out.stdout.strip().splitlines()[-1])
    bad = [(kw, g, want) for (kw, want), g in zip(REFUSALS, got) if g != want]
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _ref(name, batch, periods):
    c = MC.make(name, batch, periods)
    return c, ML.oracle_loop(c, periods)


@pytest.mark.parametrize("name", MC.NAMES)
@pytest.mark.parametrize("batch", MC.BATCHES)
@pytest.mark.parametrize("periods", MC.PERIODS)
def test_feasible_cases_are_solved_and_tight(name, batch, periods):
    c, ref = _ref(name, batch, periods)
    assert (ref["status"] == 0).all(), "every period of every feasible case is solved"
    active = ((ref["lam"] > 0).any(axis=2) & (ref["status"] == 0)).mean()
    print(f"{name} B={batch} P={periods}: (loop, period) pairs with an active row {active:.2f}")
    assert active >= 0.5  # (the batch of one is loop 0 of the batch of 67, which has active rows: model_loop_cases.make)


def test_the_long_triple_case_is_solved():
    c, ref = _ref("triple", 67, MC.WARM_PERIODS)
    assert (ref["status"] == 0).all()
    # (the loops settle at their goals: rows are active in the first third of the run, 0.27 of the pairs over all 24 periods)
    assert ((ref["lam"] > 0).any(axis=2))[:7].mean() >= 0.5


def test_designated_loops_are_infeasible_in_every_period_and_only_those():
    c, ref = _ref("triple_infeasible", 67, 7)
    assert c["infeasible"].sum() == 14
    assert (ref["status"][:, c["infeasible"]] == 2).all()
    assert (ref["status"][:, ~c["infeasible"]] == 0).all()
    assert ref["failed"].sum() == 7 * 14 == 98
    assert (ref["U0"][c["infeasible"]] == 0).all(), "the zero input is applied"


@pytest.mark.parametrize("name", MC.NAMES)
def test_numpy_warm_period_equals_the_cold_oracle_loop(name):
    """Trajectories within 1e-8 max(1, |ref|) -- the project's bound on a plan (the warm period ends at the same minimiser by
    another path, so the difference is the solvers' rounding) --, statuses equal, fewer iterations where the set carries over."""
    c, ref = _ref(name, 67, 7)
    w = ML.warm_loop_np(c, 7, warm=True)
    cold = ML.warm_loop_np(c, 7, warm=False)
    assert np.array_equal(w["status"], ref["status"]) and np.array_equal(cold["status"], ref["status"])
    for got in (w, cold):
        for k in ("X", "U0"):
            err = np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))
            assert err.max() <= 1e-8, (k, err.max())
    assert (w["recold"] <= 6).all()
    print(f"{name}: iterations oracle {ref['iters'].sum()}, NumPy cold {cold['iters'].sum()}, warm {w['iters'].sum()}, "
          f"warm periods solved again cold {w['recold'].sum()}")


def test_numpy_warm_period_saves_iterations_on_the_long_triple_case():
    c, ref = _ref("triple", 67, MC.WARM_PERIODS)
    w = ML.warm_loop_np(c, MC.WARM_PERIODS, warm=True)
    cold = ML.warm_loop_np(c, MC.WARM_PERIODS, warm=False)
    assert np.array_equal(w["status"], ref["status"])
    assert w["iters"].sum() < cold["iters"].sum()
    err = np.abs(w["X"] - ref["X"]) / np.maximum(1.0, np.abs(ref["X"]))
    assert err.max() <= 1e-8
