#!/usr/bin/env python3
"""Writes tests/golden/dispatch_queries.npz: the return code and value of the library's host-only size queries
(mpcqp_workspace_bytes, mpcqp_stagewise_workspace_bytes, mpcqp_warm_state_bytes, mpcqp_warm_state_kind, mpcqp_lds_bytes,
mpcqp_solve_workspace_bytes) over a grid of dimensions that crosses every branch of the launch dispatch and its edges.
tests/test_dispatch_queries.py asserts that the library still answers every entry the same: a change in what callers are
told to allocate is a change of the dispatch. Run it with the library built from the commit whose answers are to be
pinned. CPU only (the queries launch nothing): usage: gen_golden_dispatch.py [out.npz]"""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from qpmpc_amd import _capi

NX = (1, 2, 3, 4, 5, 6, 8, 12, 13, 16, 17, 32, 33)
NU = (1, 2, 3, 4, 5, 8, 9)
N_TARGETS = (16, 17, 20, 21, 24, 25, 128, 129, 160, 161, 256, 257)  # n = N nu where nu divides it
N_EXTRA = (1, 2, 3)  # short horizons: the small-problem kernels
MK = (0, 1, 2, 3, 4, 5, 8)
COST = (_capi.P_TERMINAL | _capi.Q_TERMINAL, _capi.P_STAGE | _capi.Q_STAGE,
        _capi.P_TERMINAL | _capi.Q_TERMINAL | _capi.P_STAGE | _capi.Q_STAGE)
DTYPES = (_capi.F64, _capi.F32)
BATCHES = (1, 4096)
MAX_ACTIVE = (0, 1, 64, 128, 256, -1, -64)


def horizons(nu):
    return sorted(set(N_EXTRA) | {n // nu for n in N_TARGETS if n % nu == 0})


def grid():
    """Rows of (dtype, nx, nu, N, mk, flags)."""
    rows = [(dt, nx, nu, N, mk, fl) for dt in DTYPES for nx in NX for nu in NU for N in horizons(nu) for mk in MK for fl in COST]
    return np.array(rows, dtype=np.int32)


def query(lib, dims):
    """Every query for every row of `dims`: (rc, value) arrays, int8 / int64."""
    nb, na = len(BATCHES), len(MAX_ACTIVE)
    out = {
        "workspace": np.zeros((len(dims), nb, 2, 2), np.int64),           # [row, batch, for_solve, (rc, bytes)]
        "stagewise": np.zeros((len(dims), nb, na, 2), np.int64),          # [row, batch, max_active, (rc, bytes)]
        "warm_bytes": np.zeros((len(dims), 2), np.int64),
        "warm_kind": np.zeros((len(dims), 2), np.int64),
        "lds_bytes": np.zeros((len(dims), 2), np.int64),
    }
    d = _capi.Dims()
    v = C.c_size_t()
    k = C.c_int32()
    for i, (dt, nx, nu, N, mk, fl) in enumerate(dims.tolist()):
        d.nx, d.nu, d.N, d.mk, d.dtype, d.flags = nx, nu, N, mk, dt, fl
        d.w_terminal, d.w_stage, d.w_input = 1.0, 1.0, 1e-3
        for b, batch in enumerate(BATCHES):
            for s in (0, 1):
                v.value = 0
                out["workspace"][i, b, s] = (lib.mpcqp_workspace_bytes(C.byref(d), batch, s, C.byref(v)), v.value)
            for a, ma in enumerate(MAX_ACTIVE):
                v.value = 0
                out["stagewise"][i, b, a] = (lib.mpcqp_stagewise_workspace_bytes(C.byref(d), batch, ma, C.byref(v)), v.value)
        v.value = 0
        out["warm_bytes"][i] = (lib.mpcqp_warm_state_bytes(C.byref(d), C.byref(v)), v.value)
        k.value = -99
        out["warm_kind"][i] = (lib.mpcqp_warm_state_kind(C.byref(d), C.byref(k)), k.value)
        v.value = 0
        out["lds_bytes"][i] = (lib.mpcqp_lds_bytes(C.byref(d), C.byref(v)), v.value)
    return out


def solve_grid(dims):
    """Rows of (dtype, n, m) of the dense solver's size query: the QPs the grid's problems condense into."""
    nm = {(int(dt), int(N * nu), int(N * mk)) for dt, nx, nu, N, mk, fl in dims.tolist()}
    return np.array(sorted(nm), dtype=np.int32)


def query_solve(lib, sg):
    out = np.zeros((len(sg), len(BATCHES), 2), np.int64)
    v = C.c_size_t()
    for i, (dt, n, m) in enumerate(sg.tolist()):
        for b, batch in enumerate(BATCHES):
            v.value = 0
            out[i, b] = (lib.mpcqp_solve_workspace_bytes(n, m, dt, batch, C.byref(v)), v.value)
    return out


def compute():
    lib = _capi.load()
    dims = grid()
    res = query(lib, dims)
    sg = solve_grid(dims)
    res["solve"] = query_solve(lib, sg)
    res["dims"] = dims
    res["solve_dims"] = sg
    return res


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "dispatch_queries.npz")
    res = compute()
    np.savez_compressed(out, batches=np.array(BATCHES), max_active=np.array(MAX_ACTIVE), **res)
    print(out, len(res["dims"]), "dimension rows,", len(res["solve_dims"]), "dense-solver rows,", os.path.getsize(out), "bytes")
