"""Helpers the test modules share that need no GPU and no torch: the built library and the header for the *_cpu.py tests of the
derivative exports, and random LTV workloads (NumPy only)."""
import os

import numpy as np
import pytest

from qpmpc_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    with open(os.path.join(ROOT, "include", "mpcqp.h")) as f:
        return f.read()


def _lib():
    from qpmpc_amd import build

    if not os.path.exists(build.LIB_PATH):
        pytest.fail("the library is not built (__graft_entry__.build())")
    return _capi.load()


def _dims(nx, nu, N, mk, dtype=_capi.F64):
    d = _capi.Dims()
    d.nx, d.nu, d.N, d.mk, d.dtype, d.flags = nx, nu, N, mk, dtype, 0
    d.w_terminal, d.w_stage, d.w_input = 1.0, 0.0, 1e-3
    return d


def _ltv(seed, B, nx, nu, N, mk, tight=1.0):
    from qpmpc_amd.workloads import random_ltv

    return random_ltv(np.random.default_rng(seed), B, nx, nu, N, mk, tight)


def dims_of(w):
    """(N, nx, nu, mk) of a workload; mk = 0 without bounds"""
    N = int(w["N"])
    nx, nu = np.asarray(w["x0"]).shape[1], np.asarray(w["B"]).shape[-1]
    mk = 0 if w["e"] is None else np.asarray(w["e"]).shape[-1]
    return N, nx, nu, mk


def random_ltv_workload(rng, B, nx, nu, N, mk, with_c=True, with_d=True, wt=2.0, wx=0.5):
    """per-problem, per-step random dynamics and rows whose bounds leave the free roll-out feasible by at least 0.05 (the
    families of tests/test_gpu_parity.py and tests/test_gpu_pairing.py)"""
    A = np.eye(nx) + 0.3 * rng.standard_normal((B, N, nx, nx))
    Bm = rng.standard_normal((B, N, nx, nu))
    Cm = rng.standard_normal((B, N, mk, nx)) if with_c else None
    D = rng.standard_normal((B, N, mk, nu)) if with_d else None
    x0 = 0.1 * rng.standard_normal((B, nx))
    e = np.zeros((B, N, mk))
    for b in range(B):
        x = x0[b].copy()
        for k in range(N):
            base = Cm[b, k] @ x if with_c else 0.0
            e[b, k] = base + 0.05 + 0.5 * np.abs(rng.standard_normal(mk))
            x = A[b, k] @ x
    return dict(A=A, B=Bm, C=Cm, D=D, e=e, N=N, wt=wt, wx=wx, wu=1e-2, x0=x0,
                goal=rng.standard_normal((B, nx)), targets=None if wx is None else rng.standard_normal((B, N * nx)))
