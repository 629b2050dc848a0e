"""Unit changes of an MPC problem (test helper, NumPy only, no GPU): the same problem stated in other units.

With scalars sx (state unit), su (input unit), sc (cost unit) and a per-row factor r of shape [B, N, mk],

    A' = A            B' = (sx/su) B      C' = r C / sx     D' = r D / su     e' = r e
    x0' = sx x0       goal' = sx goal     targets' = sx targets
    wt' = sc wt/sx^2  wx' = sc wx/sx^2    wu' = sc wu/su^2
    =>  U' = su U     X' = sx X           lam' = sc lam / r      status' = status

is a symmetry of the problem, so the expected answer of a solve on the rescaled problem is known exactly from the base problem's.
Every factor is a power of two: each rescaled operand is exact in float64 and in float32 (rescale commutes with
operand_layouts.f32_view bit for bit). CHANGES names the eight changes the tests run; the exponents keep every weight above the
1e-10 weight switch of the reference (smallest: 9.5e-9) and every |e'| far below the 1e29 sentinel.

The derivative laws (cotangents gU' = gU/su, gX' = gX/sx, so that the scalar loss gU.U + gX.X is the same number):

    d/dx0' = (1/sx) d/dx0  (goal, targets alike)    d/de' = (1/r) d/de      d/dA' = d/dA
    d/dB' = (su/sx) d/dB   d/dC' = (sx/r) d/dC      d/dD' = (su/r) d/dD
    d/dwt' = (sx^2/sc) d/dwt   d/dwx' = (sx^2/sc) d/dwx   d/dwu' = (su^2/sc) d/dwu
    tangents dx0' = sx dx0, dgoal' = sx dgoal, dtargets' = sx dtargets, de' = r de  =>  dU' = su dU, dX' = sx dX

tests/test_unit_changes_cpu.py holds all of this on the C oracle and on the NumPy restatements of tests/*_np.py;
tests/test_gpu_unit_changes.py launches the rescaled problems through every forward route and the derivative API."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

# name -> (log2 sx, log2 su, log2 sc, per-row factors?)
CHANGES = OrderedDict([
    ("state+", (10, 0, 0, False)),
    ("state-", (-10, 0, 0, False)),
    ("input+", (0, 10, 0, False)),
    ("input-", (0, -10, 0, False)),
    ("cost+", (0, 0, 20, False)),
    ("cost-", (0, 0, -20, False)),
    ("rows", (0, 0, 0, True)),
    ("mixed", (-6, -8, -12, True)),
])
SCALAR = tuple(name for name, c in CHANGES.items() if not c[3])  # (the oracle maps these back bit for bit)
ROW_EXPONENTS = (-10, 11)  # rng.integers(low, high)
WEIGHT_SWITCH = 1e-10  # the reference's (and batch.py's, single.py's) "this weight is off" threshold
SENTINEL = 1e29  # the kernels' "this row is padding" threshold on h (PAD_BOUND = 1e30)

# (route, change) -> why tests/test_gpu_unit_changes.py does not run it. README: a float32 kernel's plan is within an ABSOLUTE 1e-3
# of the float64 one, in the caller's input units; with inputs stated 1024 times smaller (or larger) that bound maps to 1 (or
# 1e-6) in base units, and a base-unit measurement would hold the kernel to something it never promised.
F32_KERNELS = ("wide stage-wise f32", "dense HBM f32", "dense HBM f32, G in the workspace", "dense HBM f32, dense G")
F32_SKIPS = {(route, change): "float32 kernel: its 1e-3 bound is absolute in the caller's input units (DESIGN.md section 5)"
             for route in F32_KERNELS for change, c in CHANGES.items() if c[1] != 0}

# Entries whose iteration counts differ from the base launch's although the change is scalar: (route, change) -> what decides.
# Statuses, accuracy and certificates are still asserted for them, and that the counts DO differ (a stale entry fails); only
# cases that run are listed. One rule accounts for all of them: the stage-wise kernels
# admit "the violated row farthest from its hyperplane in the Euclidean norm of its own stage block [C_k[r] D_k[r]]"
# (oracle/stagewise_np.py:_row_inv_norms, restated as invn in mpcqp_stage.hip, mpcqp_stagew.hip and mpcqp_stageg.hip). That norm
# adds squares of state coefficients to squares of input coefficients, so it changes with the ratio sx / su (state+ and input-
# give one path, state- and input+ another; cost and row changes leave it alone). It is a documented pivoting rule that "only
# changes the iteration count, never the minimiser", and the plans under these entries agree with the oracle to 1e-13.
_ROW_NORM = ("selection metric 1 / |[C_k[r] D_k[r]]| mixes state and input units: mpcqp_stage.hip (invn, slack pass), "
             "mpcqp_stagew.hip (invn / myinvn), after oracle/stagewise_np.py:_row_inv_norms")
ITERS_MAY_DIFFER = {(route, change): _ROW_NORM
                    for route in ("narrow stage-wise", "narrow stage-wise, stage-wise entry", "wide stage-wise f64",
                                  "wide stage-wise f64, stage-wise entry", "wide stage-wise f32", "promoted f32 (6, 2, 20, 3)")
                    for change in ("state+", "state-", "input+", "input-") if (route, change) not in F32_SKIPS}


def maps_of(change, shape, seed, shared_rows=False):
    """the factors of change `change` (a name of CHANGES) for a batch of shape (B, N, mk): dict(sx, su, sc, r [B, N, mk]). The row
    exponents are drawn from default_rng(seed); shared_rows gives every problem item 0's (a shared model has one C, D)."""
    lx, lu, lc, rows = CHANGES[change] if isinstance(change, str) else change
    B, N, mk = shape
    if rows:
        k = np.random.default_rng(seed).integers(*ROW_EXPONENTS, (B, N, mk))
        if shared_rows:
            k = np.broadcast_to(k[:1], (B, N, mk))
        r = np.ldexp(1.0, k)
    else:
        r = np.ones((B, N, mk))
    return dict(sx=2.0 ** lx, su=2.0 ** lu, sc=2.0 ** lc, r=np.ascontiguousarray(r))


def inverse(maps):
    return dict(sx=1.0 / maps["sx"], su=1.0 / maps["su"], sc=1.0 / maps["sc"], r=1.0 / maps["r"])


def apply(full, maps):
    """the materialised workload `full` ([B, N, ...] operands, None operands kept) under the factors `maps`"""
    sx, su, sc, r = maps["sx"], maps["su"], maps["sc"], maps["r"]
    out = dict(full)
    assert full["e"].shape == r.shape, (full["e"].shape, r.shape)
    out["B"] = full["B"] * (sx / su)
    for X in ("x0", "goal", "targets"):
        if full[X] is not None:
            out[X] = full[X] * sx
    if full["C"] is not None:
        assert full["C"].shape[:3] == r.shape
        out["C"] = full["C"] * (r[..., None] / sx)
    if full["D"] is not None:
        assert full["D"].shape[:3] == r.shape
        out["D"] = full["D"] * (r[..., None] / su)
    out["e"] = full["e"] * r
    out["wt"] = full["wt"] * sc / sx ** 2
    if full["wx"] is not None:
        out["wx"] = full["wx"] * sc / sx ** 2
    out["wu"] = full["wu"] * sc / su ** 2
    return out


def rescale(full, change, seed=0, shared_rows=False):
    """(full', maps): `full` restated under change `change`, and the factors that took it there"""
    maps = maps_of(change, full["e"].shape, seed, shared_rows)
    return apply(full, maps), maps


def weights(w):
    return [float(w[k]) for k in ("wt", "wx", "wu") if w[k] is not None]


# ---------------------------------------------------------------------------------------------- back to base units
def back_plan(U, maps):
    return np.asarray(U, dtype=np.float64) / maps["su"]


def back_states(X, maps):
    return np.asarray(X, dtype=np.float64) / maps["sx"]


def back_multipliers(lam, maps):
    lam = np.asarray(lam, dtype=np.float64)
    return lam * maps["r"].reshape(lam.shape) / maps["sc"]


def _rows(a, r, b):
    """a (an e-, C- or D-shaped array of problem b, or of the batch if b is None, flat or not) times the row factors r"""
    a = np.asarray(a, dtype=np.float64)
    rb = r if b is None else r[b]
    lead = rb.shape  # ([B,] N, mk)
    return (a.reshape(lead + (-1,)) * rb[..., None]).reshape(a.shape)


def rescale_cotangents(gU, gX, maps):
    """the cotangents of the same scalar loss in the new units"""
    return np.asarray(gU) / maps["su"], (None if gX is None else np.asarray(gX) / maps["sx"])


def back_gradients(g, maps, b=None):
    """gradients taken on the rescaled problem (dict with keys among x0, goal, targets, e, A, B, C, D, w or wt, wx, wu; arrays of
    problem b, or of the whole batch if b is None) as gradients with respect to the base problem's operands"""
    sx, su, sc, r = maps["sx"], maps["su"], maps["sc"], maps["r"]
    wfac = np.array([sc / sx ** 2, sc / sx ** 2, sc / su ** 2])
    out = {}
    for key, v in g.items():
        if v is None:
            out[key] = None
        elif key in ("x0", "goal", "targets"):
            out[key] = np.asarray(v) * sx
        elif key == "e":
            out[key] = _rows(v, r, b)
        elif key == "A":
            out[key] = np.asarray(v)
        elif key == "B":
            out[key] = np.asarray(v) * (sx / su)
        elif key == "C":
            out[key] = _rows(v, r, b) / sx
        elif key == "D":
            out[key] = _rows(v, r, b) / su
        elif key == "w":
            out[key] = np.asarray(v) * wfac
        elif key in ("wt", "wx", "wu"):
            out[key] = np.asarray(v) * wfac[("wt", "wx", "wu").index(key)]
        else:
            out[key] = v
    return out


def rescale_tangents(tan, maps, b=None):
    """tangents of x0, goal, targets, e (dict; [..., T, size] or [size] arrays of problem b, or of the batch if b is None: then e's
    tangents are [B, T, N*mk]) in the new units"""
    sx, r = maps["sx"], maps["r"]
    out = {}
    for key, v in tan.items():
        if v is None:
            out[key] = None
        elif key in ("x0", "goal", "targets"):
            out[key] = np.asarray(v) * sx
        elif key == "e":
            v = np.asarray(v, dtype=np.float64)
            if b is None:
                out[key] = v * r.reshape(r.shape[0], 1, -1) if v.ndim == 3 else v * r.reshape(r.shape[0], -1)
            else:
                out[key] = v * r[b].reshape(-1)
        else:
            raise KeyError(key)
    return out


def back_tangents(dU, dX, maps):
    return np.asarray(dU, dtype=np.float64) / maps["su"], (None if dX is None else np.asarray(dX, dtype=np.float64) / maps["sx"])
