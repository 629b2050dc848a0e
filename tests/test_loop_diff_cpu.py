"""CPU tests (no GPU) of the closed-loop adjoint: the NumPy restatement of the reverse-time recursion
(tests/loop_adjoint_np.py) against central differences of the oracle loop, the pure plant adjoint of loops without a plan,
the declaration and binding of mpcqp_model_periods_vjp_batch, its refusal and EINVAL codes through the export itself (in a
process of its own that hides every device, like tests/test_model_loop_cpu.py) and the resource figures of the kernels the
new one shares its translation unit with.

Central differences: h = 1e-6 on the C-oracle loop, loss_b = <gX, X_b> + <gU0, U0_b> with seeded cotangents, bound 1e-6
relative, |fd - g| <= 1e-6 max(1, |g|). Only loops whose every period is strictly complementary by 1e-4 are compared -- the
smallest positive multiplier and the smallest slack of an inactive row with a non-zero row of M (loop_adjoint_np.margins):
next to a change of the active set the plan has a kink and a central difference straddles it. Every case at (67, 7) keeps
at least 15 loops under that filter.

Measured: box4 / box5 / tiny / wide16 at most 1.8e-8 (66 - 67 loops); triple 6.7e-7 (18 loops). The triple figure is the
ORACLE's rounding, not the recursion's error: it goes as 1 / h (2.5e-7 at h = 1e-5, 3.6e-5 at h = 1e-7 for x0), an oracle
tolerance of 1e-12 instead of 1e-9 leaves it where it is, and other seeds of the cotangents give 3e-7 .. 2e-6. With unit
cotangents on X and U0 alike -- the jerk of that family reaches 86 at w_input = 1e-6 -- it is 2.3e-5: hence the cotangents
in units of each record's range (loop_adjoint_np.cotangents)."""
import functools
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import loop_adjoint_np as LA
import model_loop_cases as MC
import model_loop_np as ML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_RTOL, FD_MARGIN, FD_MIN_LOOPS = 1e-6, 1e-4, 15


@functools.lru_cache(maxsize=None)
def _ref(name, batch=67, periods=7):
    c = MC.make(name, batch, periods)
    ref = ML.oracle_loop(c, periods)
    md = ML.condense_lti(c)
    gX, gU0 = LA.cotangents(c, periods, ref)
    return c, ref, md, gX, gU0, LA.loop_vjp(c, ref, gX, gU0, md)


def _held(fd, g, keep, what):
    err = np.abs(fd - g)[keep] / np.maximum(1.0, np.abs(g[keep]))
    print(f"{what}: max relative error {err.max():.2e} over {keep.sum()} loops")
    assert err.max() <= FD_RTOL, (what, err.max())
    return err.max()


@pytest.mark.parametrize("name", MC.NAMES)
def test_restatement_against_central_differences_of_the_oracle_loop(name):
    P = 7
    c, ref, md, gX, gU0, g = _ref(name)
    keep = LA.margins(c, ref, md) >= FD_MARGIN
    print(f"{name}: {keep.sum()} of 67 loops are strictly complementary by {FD_MARGIN:g}")
    assert keep.sum() >= FD_MIN_LOOPS
    assert (g["failed"] == 0).all()
    nx, nu = c["nx"], c["nu"]
    fd = lambda key, idx: LA.central_difference(c, P, gX, gU0, key, idx)  # noqa: E731
    worst = 0.0
    for j in range(nx):
        worst = max(worst, _held(fd("x0", (j,)), g["x0"][:, j], keep, f"x0[{j}]"))
        if c["goal_by_period"]:  # [P, nx], shared by the batch: one period's goal moves, every loop sees it
            for t in (0, P - 1):
                worst = max(worst, _held(fd("goal", (t, j)), g["goal"][:, t, j], keep, f"goal[{t}, {j}]"))
        else:  # [B, nx], the same in every period: the sum over the periods
            worst = max(worst, _held(fd("goal", (j,)), g["goal"][:, :, j].sum(1), keep, f"goal[{j}]"))
    j = nx - 2 if name == "triple" else nx - 1  # (the triple case takes no disturbance on the acceleration: x_0's row)
    for t in (0, P - 1):
        worst = max(worst, _held(fd("dist", (t, j)), g["states"][:, t + 1, j], keep, f"disturbance[{t}, {j}]"))
    i, jA, jB = nx - 1, 0, nu - 1
    if name == "triple":
        i = 0  # (d position / d velocity and d position / d jerk: the acceleration's row stays exact)
        jA = 1
    worst = max(worst, _held(fd("Ap", (i, jA)), g["Ap"][:, i, jA], keep, f"Ap[{i}, {jA}]"))
    worst = max(worst, _held(fd("Bp", (i, jB)), g["Bp"][:, i, jB], keep, f"Bp[{i}, {jB}]"))
    print(f"{name}: worst {worst:.2e}")


def test_loops_without_a_plan_have_the_pure_plant_adjoint():
    c, ref, md, gX, gU0, g = _ref("triple_infeasible")
    assert c["infeasible"].sum() == 14 and (ref["status"][:, c["infeasible"]] != 0).all()
    for b in np.flatnonzero(c["infeasible"]):
        a = LA.plant_adjoint(c, gX, b)
        assert np.array_equal(g["states"][b], a) and np.array_equal(g["x0"][b], a[0])
        assert not g["goal"][b].any() and not g["targets"][b].any()
    feasible = ~c["infeasible"]
    assert np.abs(g["goal"][feasible]).sum(axis=(1, 2)).min() > 0  # ... and the others go through their plans


def test_period_sums_and_costates_are_consistent():
    c, ref, md, gX, gU0, g = _ref("box4")
    assert np.array_equal(g["states"][:, 0], g["x0"]) and np.array_equal(g["states"][:, -1], gX[:, -1])
    a = g["states"]
    assert np.allclose(g["Ap"], np.einsum("bti,btj->bij", a[:, 1:], ref["X"][:, :-1]), rtol=1e-12, atol=1e-14)
    assert np.allclose(g["Bp"], np.einsum("bti,btj->bij", a[:, 1:], ref["U0"]), rtol=1e-12, atol=1e-14)


def test_export_is_declared_and_bound_and_the_abi_is_12():
    from qpmpc_amd import _capi
    import qpmpc_amd

    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert re.search(r"^int mpcqp_model_periods_vjp_batch\(", header, re.M)
    assert "} MpcqpPeriodGrad;" in header
    assert "#define MPCQP_ABI_VERSION 12" in header and _capi.ABI_VERSION == 12
    assert "mpcqp_model_periods_vjp_batch" in _capi.EXPORTS
    assert [f[0] for f in _capi.PeriodGrad._fields_] == ["ptr", "batch_stride", "period_stride"]
    assert "closed_loop_diff" in qpmpc_amd.__all__ and callable(qpmpc_amd.closed_loop_diff)
    lib = _capi.load()  # (built: the symbol resolves and the library reports the ABI)
    assert lib.mpcqp_abi_version() == 12 and len(lib.mpcqp_model_periods_vjp_batch.argtypes) == 19


_REPLAY = r"""
import os, sys, json
for v in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
    os.environ[v] = "-1"
sys.path.insert(0, sys.argv[1])
import ctypes as C
from qpmpc_amd import _capi
lib = _capi.load()
P = 0x1000  # a pointer that is not NULL; never dereferenced by the host
def call(nx=3, nu=1, N=16, mk=2, dtype=0, flags=5, batch=8, nperiods=2, model=P, plant=True, A=P, B=P, a_stride=0, lam=P,
         status=P, X=P, U0=P, g_x0=P, g_A=None, g_B=None, goal=(P, 3, 0), targets=None):
    d = _capi.Dims(nx, nu, N, mk, dtype, flags, 1.0, 0.0, 1e-6)
    pl = _capi.LoopPlant(_capi.Operand(A, a_stride, 0), _capi.Operand(B, 0, 0), _capi.Operand(None, 0, 0))
    gg = None if goal is None else _capi.PeriodGrad(*goal)
    gt = None if targets is None else _capi.PeriodGrad(*targets)
    return lib.mpcqp_model_periods_vjp_batch(C.byref(d), model, C.byref(pl) if plant else None, batch, nperiods, lam, status,
                                             X, U0, None, None, g_x0, None, None if gg is None else C.byref(gg),
                                             None if gt is None else C.byref(gt), g_A, g_B, None, None)
rows = json.loads(sys.argv[2])
print(json.dumps([call(**kw) for kw in rows]))
"""

EINVAL, EDTYPE, EUNSUPPORTED = -1, -3, -6
P_ = 0x1000
REFUSALS = [
    (dict(dtype=1), EDTYPE), (dict(dtype=1, N=17), EDTYPE), (dict(dtype=1, model=None), EDTYPE),  # the dtype comes first,
    (dict(N=17), EUNSUPPORTED), (dict(N=17, model=None), EUNSUPPORTED),                            # then the envelope
    (dict(nu=2, N=9, mk=1), EUNSUPPORTED), (dict(mk=3), EUNSUPPORTED), (dict(mk=0), EUNSUPPORTED),
    (dict(nx=17, N=4), EUNSUPPORTED),
    (dict(model=None), EINVAL), (dict(plant=False), EINVAL), (dict(A=None), EINVAL), (dict(B=None), EINVAL),
    (dict(lam=None), EINVAL), (dict(status=None), EINVAL), (dict(g_x0=None), EINVAL), (dict(nperiods=0), EINVAL),
    (dict(nperiods=-2), EINVAL), (dict(batch=-1), EINVAL), (dict(a_stride=-9), EINVAL),
    (dict(goal=(P_, -3, 0)), EINVAL), (dict(goal=(P_, 3, -1)), EINVAL), (dict(targets=(P_, 48, -48)), EINVAL),
    (dict(g_A=P_, X=None), EINVAL), (dict(g_B=P_, U0=None), EINVAL),
    (dict(batch=0), 0), (dict(batch=0, X=None, U0=None, goal=None), 0),  # an empty batch launches nothing
]


def test_refusal_and_einval_codes_through_the_export():
    rows = [kw for kw, _ in REFUSALS]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, "-c", _REPLAY, ROOT, json.dumps(rows)], check=True, timeout=120, env=env,
                         capture_output=True, text=True)
    got = json.loads(out.stdout.strip().splitlines()[-1])
    bad = [(kw, g, want) for (kw, want), g in zip(REFUSALS, got) if g != want]
    assert not bad, bad


def _resources(path):
    rows = {}
    for line in open(os.path.join(ROOT, "profiles", path)).read().splitlines()[1:]:
        f = line.split()
        rows[f[1]] = dict(zip(("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"), map(int, f[2:])))
    return rows


def test_resource_figures_of_the_small_kernels():
    """The two instantiations of mpcqp_model_diff_small_kernel keep the figures recorded before the loop kernel joined their
    translation unit -- 204 / 169 VGPRs, no scratch, no VGPR spill --; where the unit has been compiled here, the objects say
    the same (tools/kernel_resources.py reads their metadata notes). The loop kernel's own figures: no scratch, no VGPR spill."""
    old = _resources("model_diff_kernel_resources.txt")
    assert old["mpcqp_model_diff_small_kernel<false>"]["vgpr"] == 204 and old["mpcqp_model_diff_small_kernel<true>"]["vgpr"] == 169
    new = _resources("loop_diff_kernel_resources.txt")
    for k in ("mpcqp_model_diff_small_kernel<false>", "mpcqp_model_diff_small_kernel<true>"):
        assert new[k] == old[k], (k, new[k], old[k])
    loop = new["mpcqp::mpcqp_loop_adjoint_small_kernel"]
    assert loop["scratch"] == 0 and loop["vspill"] == 0 and loop["lds"] == 0  # (its LDS image is dynamic)
    import glob

    if not glob.glob(os.path.join(ROOT, "qpmpc_amd", "lib", "obj", "mpcqp_model_adjoint.hip.*.o")):
        return  # (a library built elsewhere: the recorded figures stand)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "_small_kernel"], check=True,
                         capture_output=True, text=True, timeout=120).stdout
    built = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if f and f[0] == "mpcqp_model_adjoint":
            built[f[1]] = dict(zip(("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"), map(int, f[2:])))
    for k, v in built.items():
        assert v == new[k], (k, v, new[k])
