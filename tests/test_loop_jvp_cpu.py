"""CPU tests (no GPU) of the closed-loop forward sensitivities: the NumPy restatement of the forward-time recursion
(tests/loop_tangent_np.py) against its transpose (tests/loop_adjoint_np.py) and against central differences of the oracle
loop, the pure plant rollout of loops without a plan, the declaration and binding of mpcqp_model_periods_jvp_batch, its
refusal and EINVAL codes through the export itself (in a process of its own that hides every device) and the resource
figures of the new kernel.

Duality: <gX, dX> + <gU0, dU0> against <g, tangents> with random tangents on all six operands, relative to
max(1, |<g, tangents>|), bound 1e-10 (the bound tests/test_model_diff_cpu.py gives its own duality). Measured: at most
3.0e-12 (tiny; 4.2e-13 on triple).

Central differences: h = 1e-6 on the C-oracle loop, unit tangents on every component of x0, on one disturbance entry of
period 0 and on one entry each of Ap and Bp (the entries tests/test_loop_diff_cpu.py moves). Only loops whose every period is
strictly complementary by 1e-4 are compared (loop_adjoint_np.margins), at least 15 of them. Each record is compared in units
of its own range, |fd - d| <= 1e-6 max(s, |d|), s = max(1, max |X|) for dX and max(1, max |U0|) for dU0: a central difference
carries the oracle's rounding of the record divided by h, and the jerk of the triple family reaches 86 (without the range
scaling its dU0 is at 1.3e-5, the effect tests/test_loop_diff_cpu.py describes). Measured for x0 and the disturbance: triple at
most 4.2e-7 (dX) and 2.0e-7 (dU0); tiny 1.2e-8; box4, box5, wide16 1.3e-9. The Ap / Bp entries: see the test's docstring."""
import functools
import glob
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import loop_adjoint_np as LA
import loop_tangent_np as LT
import model_loop_cases as MC
import model_loop_np as ML

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUAL_RTOL = 1e-10
FD_RTOL, FD_MARGIN, FD_MIN_LOOPS, FD_H = 1e-6, 1e-4, 15, 1e-6
ALL = MC.NAMES + ("triple_infeasible",)


@functools.lru_cache(maxsize=None)
def _ref(name, batch=67, periods=7):
    c = MC.make(name, batch, periods)
    return c, ML.oracle_loop(c, periods), ML.condense_lti(c)


@pytest.mark.parametrize("name", ALL)
def test_restatement_is_the_transpose_of_the_adjoint_restatement(name):
    P, T = 7, 3
    c, ref, md = _ref(name)
    tan = LT.tangents(c, P, T)
    out = LT.loop_jvp(c, ref, tan, md)
    gX, gU0 = LA.cotangents(c, P, ref)
    g = LA.loop_vjp(c, ref, gX, gU0, md)
    assert np.array_equal(out["failed"], g["failed"])
    lhs = (gX[:, None] * out["dX"]).sum(axis=(2, 3)) + (gU0[:, None] * out["dU0"]).sum(axis=(2, 3))
    rhs, _ = LT.pairing(g, tan)
    err = float((np.abs(lhs - rhs) / np.maximum(1.0, np.abs(rhs))).max())
    print(f"{name}: duality {err:.2e}")
    assert np.abs(out["dU0"]).max() > 0
    assert err <= DUAL_RTOL


def _records(case, periods, key, index, step):
    c = dict(case)
    a = np.array(case[key], dtype=float)
    per_loop = a.ndim > len(index)
    a[(slice(None),) + tuple(index) if per_loop else tuple(index)] += step
    c[key] = a
    res = ML.oracle_loop(c, periods)
    return res["X"], res["U0"]


def _central(case, periods, key, index, h=FD_H):
    """(dX [B, P+1, nx], dU0 [B, P, nu]) by central differences of the oracle loop: every loop's entry moves at once."""
    (Xp, Up), (Xm, Um) = _records(case, periods, key, index, +h), _records(case, periods, key, index, -h)
    return (Xp - Xm) / (2.0 * h), (Up - Um) / (2.0 * h)


def _fd_cases(name, c):
    """[(label, operand, index)]: the moves of the test, in the order of the tangents of `_fd_tangents`."""
    nx, nu = c["nx"], c["nu"]
    moves = [(f"x0[{j}]", "x0", (j,)) for j in range(nx)]
    j = nx - 2 if name == "triple" else nx - 1  # (the triple case takes no disturbance on the acceleration: x_0's row)
    moves.append((f"disturbance[0, {j}]", "dist", (0, j)))
    i, jA, jB = nx - 1, 0, nu - 1
    if name == "triple":
        i, jA = 0, 1  # (d position / d velocity and d position / d jerk: the acceleration's row stays exact)
    moves += [(f"Ap[{i}, {jA}]", "Ap", (i, jA)), (f"Bp[{i}, {jB}]", "Bp", (i, jB))]
    return moves


def _fd_tangents(c, periods, moves):
    """One unit tangent per move, shared by the batch: {operand: [1, T, ...]}."""
    T = len(moves)
    tan = {k: np.zeros((1, T) + s) for k, s in LT.tangent_shapes(c, periods).items() if k in ("x0", "dist", "Ap", "Bp")}
    for j, (_, key, idx) in enumerate(moves):
        tan[key][(0, j) + tuple(idx)] = 1.0
    return tan


def _fd_errors(name, h=FD_H):
    P = 7
    c, ref, md = _ref(name)
    keep = LA.margins(c, ref, md) >= FD_MARGIN
    moves = _fd_cases(name, c)
    out = LT.loop_jvp(c, ref, _fd_tangents(c, P, moves), md)
    assert (out["failed"] == 0).all()
    sX, sU = max(1.0, np.abs(ref["X"]).max()), max(1.0, np.abs(ref["U0"]).max())
    errs = {}
    for j, (label, key, idx) in enumerate(moves):
        fX, fU = _central(c, P, key, idx, h)
        dX, dU = out["dX"][keep, j], out["dU0"][keep, j]
        eX = float((np.abs(fX[keep] - dX) / np.maximum(sX, np.abs(dX))).max())
        eU = float((np.abs(fU[keep] - dU) / np.maximum(sU, np.abs(dU))).max())
        errs[label] = (eX, eU)
    return keep, errs


@pytest.mark.parametrize("name", MC.NAMES)
def test_restatement_against_central_differences_of_the_oracle_loop(name):
    """Measured (h = 1e-6, in units of each record's range, dX / dU0): x0 and the disturbance as the module's docstring says;
    the Ap and Bp entries: triple 3.0e-7 / 1.8e-7 (Ap[0, 1]) and 4.8e-8 / 9.0e-8 (Bp[0, 0]); tiny at most 9.7e-9; box4 at most
    1.3e-9; box5 and wide16 at most 3.2e-10. Every figure is inside the bound."""
    keep, errs = _fd_errors(name)
    print(f"{name}: {keep.sum()} of 67 loops are strictly complementary by {FD_MARGIN:g}")
    assert keep.sum() >= FD_MIN_LOOPS
    for label, (eX, eU) in errs.items():
        print(f"{name} {label}: dX {eX:.2e}, dU0 {eU:.2e}")
    worst = max(max(e) for e in errs.values())
    print(f"{name}: worst {worst:.2e}")
    for label, (eX, eU) in errs.items():
        assert eX <= FD_RTOL and eU <= FD_RTOL, (label, eX, eU)


def test_loops_without_a_plan_roll_the_tangent_through_the_plant_only():
    P, T = 7, 3
    c, ref, md = _ref("triple_infeasible")
    assert c["infeasible"].sum() == 14 and (ref["status"][:, c["infeasible"]] != 0).all()
    tan = LT.tangents(c, P, T)
    out = LT.loop_jvp(c, ref, tan, md)
    for b in np.flatnonzero(c["infeasible"]):
        for j in range(T):
            assert np.array_equal(out["dX"][b, j], LT.plant_rollout(c, tan, b, j, ref["X"], ref["U0"]))
        assert not out["dU0"][b].any()
    feasible = ~c["infeasible"]
    assert np.abs(out["dU0"][feasible]).sum(axis=(1, 2, 3)).min() > 0  # ... and the others go through their plans


def test_export_is_declared_and_bound_and_the_abi_is_12():
    from qpmpc_amd import _capi
    import qpmpc_amd

    header = open(os.path.join(ROOT, "include", "mpcqp.h")).read()
    assert re.search(r"^int mpcqp_model_periods_jvp_batch\(", header, re.M)
    assert "} MpcqpPeriodTangent;" in header and "} MpcqpLoopTangents;" in header
    assert "#define MPCQP_ABI_VERSION 12" in header and _capi.ABI_VERSION == 12
    assert "mpcqp_model_periods_jvp_batch" in _capi.EXPORTS
    assert [f[0] for f in _capi.PeriodTangent._fields_] == ["ptr", "batch_stride", "tangent_stride", "period_stride"]
    assert [f[0] for f in _capi.LoopTangents._fields_] == ["dx0", "dx0_stride", "dgoal", "dtargets", "dd", "dA", "dA_stride", "dB",
                                                           "dB_stride"]
    for f in ("dgoal", "dtargets", "dd"):
        assert dict(_capi.LoopTangents._fields_)[f] is _capi.PeriodTangent
    for fn in ("closed_loop_jvp", "closed_loop_jacobian"):
        assert fn in qpmpc_amd.__all__ and callable(getattr(qpmpc_amd, fn))
    lib = _capi.load()  # (built: the symbol resolves and the library reports the ABI)
    assert lib.mpcqp_abi_version() == 12 and len(lib.mpcqp_model_periods_jvp_batch.argtypes) == 15


_REPLAY = r"""
import os, sys, json
for v in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
    os.environ[v] = "-1"
sys.path.insert(0, sys.argv[1])
import ctypes as C
from qpmpc_amd import _capi
lib = _capi.load()
P = 0x1000  # a pointer that is not NULL; never dereferenced by the host
def call(nx=3, nu=1, N=16, mk=2, dtype=0, flags=5, batch=8, nperiods=2, ntan=3, model=P, plant=True, A=P, B=P, a_stride=0,
         b_stride=0, lam=P, status=P, X=P, U0=P, tan=True, dx0=(P, 9), dgoal=(P, 9, 3, 0), dtargets=(None, 0, 0, 0),
         dd=(None, 0, 0, 0), dA=(None, 0), dB=(None, 0), dX=P, dU0=P):
    d = _capi.Dims(nx, nu, N, mk, dtype, flags, 1.0, 0.0, 1e-6)
    pl = _capi.LoopPlant(_capi.Operand(A, a_stride, 0), _capi.Operand(B, b_stride, 0), _capi.Operand(None, 0, 0))
    tn = _capi.LoopTangents(*dx0, _capi.PeriodTangent(*dgoal), _capi.PeriodTangent(*dtargets), _capi.PeriodTangent(*dd),
                            *dA, *dB)
    return lib.mpcqp_model_periods_jvp_batch(C.byref(d), model, C.byref(pl) if plant else None, batch, nperiods, ntan, lam,
                                             status, X, U0, C.byref(tn) if tan else None, dX, dU0, None, None)
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
    (dict(lam=None), EINVAL), (dict(status=None), EINVAL), (dict(tan=False), EINVAL), (dict(dX=None), EINVAL),
    (dict(nperiods=0), EINVAL), (dict(nperiods=-2), EINVAL), (dict(batch=-1), EINVAL),
    (dict(ntan=0), EINVAL), (dict(ntan=-1), EINVAL), (dict(ntan=257), EINVAL),
    (dict(a_stride=-9), EINVAL), (dict(b_stride=-3), EINVAL), (dict(dx0=(P_, -9)), EINVAL),
    (dict(dgoal=(P_, -9, 3, 0)), EINVAL), (dict(dgoal=(P_, 9, -3, 0)), EINVAL), (dict(dgoal=(P_, 9, 3, -1)), EINVAL),
    (dict(dtargets=(P_, -144, 48, 0)), EINVAL), (dict(dtargets=(P_, 144, -48, 0)), EINVAL), (dict(dtargets=(P_, 288, 96, -48)), EINVAL),
    (dict(dd=(P_, -18, 6, 3)), EINVAL), (dict(dd=(P_, 18, -6, 3)), EINVAL), (dict(dd=(P_, 18, 6, -3)), EINVAL),
    (dict(dA=(P_, -27)), EINVAL), (dict(dB=(P_, -9)), EINVAL),
    (dict(dA=(P_, 27), X=None), EINVAL), (dict(dB=(P_, 9), U0=None), EINVAL),
    (dict(batch=0), 0), (dict(batch=0, X=None, U0=None, dU0=None, dx0=(None, 0)), 0),  # an empty batch launches nothing
    (dict(batch=0, ntan=256, dA=(P_, 27), dB=(P_, 9)), 0),
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


def test_resource_figures_of_the_tangent_kernel():
    """No scratch and no VGPR spill; the three kernels it shares mpcqp_model_small.h with keep their recorded figures; where
    the units have been compiled here, the objects say the same (tools/kernel_resources.py reads their metadata notes)."""
    new, old = _resources("loop_jvp_kernel_resources.txt"), _resources("loop_diff_kernel_resources.txt")
    row = new["mpcqp::mpcqp_loop_tangent_small_kernel"]
    assert row["scratch"] == 0 and row["vspill"] == 0 and row["lds"] == 0  # (its LDS image is dynamic)
    assert row["vgpr"] + row["agpr"] <= 256  # two wavefronts per SIMD
    assert len(old) == 3
    for k, v in old.items():
        assert new[k] == v, (k, new[k], v)
    if not glob.glob(os.path.join(ROOT, "qpmpc_amd", "lib", "obj", "mpcqp_loop_tangent.hip.*.o")):
        return  # (a library built elsewhere: the recorded figures stand)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "_small_kernel"], check=True,
                         capture_output=True, text=True, timeout=120).stdout
    built = {}
    for line in out.splitlines()[1:]:
        f = line.split()
        if f and f[0] in ("mpcqp_loop_tangent", "mpcqp_model_adjoint"):
            built[f[1]] = dict(zip(("vgpr", "agpr", "sgpr", "vspill", "sspill", "scratch", "lds"), map(int, f[2:])))
    assert "mpcqp::mpcqp_loop_tangent_small_kernel" in built
    for k, v in built.items():
        assert v == new[k], (k, v, new[k])
