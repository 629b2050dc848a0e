#!/usr/bin/env python3
"""Writes tests/golden/refusal_codes.npz: the negative return code of every launch, on a grid of the five forward exports
(mpcqp_build_solve_batch, mpcqp_stagewise_solve_batch, mpcqp_solve_model_batch, mpcqp_solve_model_bounds_batch,
mpcqp_solve_batch), that the library refuses on the host before it touches a device. The grid crosses both dtypes, every
flag of MpcqpSolveOpts.flags alone and next to MPCQP_OPT_ON_CHIP_32 and MPCQP_OPT_FOUR_PER_WAVE, a pairing order, a warm
state of each warm_start mode, a missing and a roomy workspace, and dimensions at the edges of every kernel's envelope.
tests/test_refusal_codes.py asserts that the library still answers every recorded case with the same code: where two
rules refuse one launch, the code says which of them is checked first.

Only refused cases are recorded: a case that is served would reach the runtime, so it is left out. The pointers handed
over are placeholders the host never dereferences, and the process hides every device from the runtime before it loads
the library, so that a case which is (wrongly) served fails in the runtime instead of running a kernel on them. Run it
with the library built from the commit whose answers are to be pinned.
usage: gen_golden_refusals.py [out.npz] | --replay in.npz out.npy"""
import os
import sys

if __name__ == "__main__":  # (as a script only, and before anything loads the runtime: importing grid() hides nothing)
    for _var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        os.environ[_var] = "-1"

import ctypes as C
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from qpmpc_amd import _capi

EXPORTS = ("mpcqp_build_solve_batch", "mpcqp_stagewise_solve_batch", "mpcqp_solve_model_batch",
           "mpcqp_solve_model_bounds_batch", "mpcqp_solve_batch")
BUILD, STAGEWISE, MODEL, MODEL_BOUNDS, QP = range(5)
ALL_FLAGS = tuple(1 << b for b in range(15))  # MPCQP_OPT_FORCE_LDS .. MPCQP_OPT_ON_CHIP_32
FLAGS = ((0,) + ALL_FLAGS + tuple(f | _capi.OPT_ON_CHIP_32 for f in ALL_FLAGS if f != _capi.OPT_ON_CHIP_32)
         + tuple(f | _capi.OPT_FOUR_PER_WAVE for f in ALL_FLAGS if f not in (_capi.OPT_FOUR_PER_WAVE, _capi.OPT_ON_CHIP_32)))
WARM = (-1, 0, _capi.WARM_OPERATOR, _capi.WARM_ACTIVE_SET)  # -1: no warm state; else a state with this warm_start
DTYPES = (_capi.F64, _capi.F32)
BATCH = 8
PLACEHOLDER = 0x1000  # a pointer that is not NULL; never dereferenced by the host
ROOMY = 1 << 40       # bytes claimed for the workspace and the warm state where they are "there"


def shapes():
    """(nx, nu, N, mk): n = 16, 17, 32, 33, m = 32, 33, 64, 65 and mk = 4, 5, 8, 9 for each of nx = 2, 4, 5, 8, 9; no rows at
    all; one shape each for the narrow, wide, general and dense paths; one that no kernel serves (n = 260 with nu = 10)."""
    per_nx = ((1, 16, 2),   # n = 16, m = 32
              (1, 17, 2),   # n = 17
              (1, 32, 2),   # n = 32, m = 64
              (1, 33, 1),   # n = 33, m = 33
              (1, 16, 4),   # n = 16, m = 64, mk = 4
              (1, 13, 5),   # m = 65, mk = 5
              (1, 11, 3),   # m = 33
              (1, 8, 8),    # m = 64, mk = 8
              (1, 7, 9),    # mk = 9
              (2, 16, 2))   # n = 32, m = 32
    out = [(nx, nu, N, mk) for nx in (2, 4, 5, 8, 9) for nu, N, mk in per_nx]
    out += [(3, 1, 8, 0), (3, 1, 24, 2), (8, 2, 12, 2), (20, 6, 10, 2), (4, 10, 8, 2), (4, 10, 26, 1)]
    return out


QP_SIZES = tuple((n, m) for n in (1, 16, 17, 32, 33, 256, 257) for m in (0, 1, 32, 33, 64, 65))


def grid():
    """Rows of (export, dtype, nx, nu, N, mk, flags, order, warm, roomy, e). For mpcqp_solve_batch nx = 1, nu = n, N = 1,
    mk = m. `e`: the bounds are handed over (mpcqp_solve_model_batch takes none; the other exports miss them in a few
    rows only: a missing argument is refused before any option is read)."""
    rows = []
    for ex in (BUILD, STAGEWISE, MODEL, MODEL_BOUNDS):
        for dt in DTYPES:
            for nx, nu, N, mk in shapes():
                for order in (0, 1):
                    for warm in WARM:
                        for roomy in (0, 1):
                            rows += [(ex, dt, nx, nu, N, mk, fl, order, warm, roomy, ex != MODEL) for fl in FLAGS]
                if ex != MODEL:
                    rows += [(ex, dt, nx, nu, N, mk, fl, 0, -1, 0, 0) for fl in (0, _capi.OPT_ON_CHIP_32, _capi.OPT_FOUR_PER_WAVE)]
    for dt in DTYPES:
        for n, m in QP_SIZES:
            for order in (0, 1):
                for warm in WARM:
                    for roomy in (0, 1):
                        rows += [(QP, dt, 1, n, 1, m, fl, order, warm, roomy, 1) for fl in FLAGS]
    return np.array(rows, dtype=np.int32)


def codes(lib, rows):
    """The return code of every row's call."""
    out = np.zeros(len(rows), np.int32)
    d = _capi.Dims()
    d.flags = _capi.P_TERMINAL | _capi.Q_TERMINAL
    d.w_terminal, d.w_stage, d.w_input = 1.0, 1.0, 1e-3
    p = _capi.Problem()
    for name in ("A", "B", "x0", "goal"):
        getattr(p, name).ptr = PLACEHOLDER
    o = _capi.SolveOpts()
    x0, goal, e = _capi.Operand(PLACEHOLDER, 0, 0), _capi.Operand(PLACEHOLDER, 0, 0), _capi.Operand(PLACEHOLDER, 0, 0)
    ptr = C.c_void_p(PLACEHOLDER)
    build, stagewise, model, qp = (lib.mpcqp_build_solve_batch, lib.mpcqp_stagewise_solve_batch,
                                   lib.mpcqp_solve_model_bounds_batch, lib.mpcqp_solve_batch)
    plain_model = lib.mpcqp_solve_model_batch
    for i, (ex, dt, nx, nu, N, mk, fl, order, warm, roomy, has_e) in enumerate(rows.tolist()):
        d.nx, d.nu, d.N, d.mk, d.dtype = nx, nu, N, mk, dt
        o.flags = fl
        o.order = PLACEHOLDER if order else None
        o.warm_state = PLACEHOLDER if warm >= 0 else None
        o.warm_start = max(warm, 0)
        o.warm_state_bytes = ROOMY if roomy else 0
        ws, ws_bytes = (ptr, ROOMY) if roomy else (None, 0)
        if ex == BUILD or ex == STAGEWISE:
            p.C.ptr = PLACEHOLDER if mk else None
            p.e.ptr = PLACEHOLDER if mk and has_e else None
            e_block = N * mk
            p.e.batch_stride, p.e.step_stride = e_block, mk
            if ex == BUILD:
                out[i] = build(d, p, BATCH, o, ptr, ptr, ptr, ptr, ws, ws_bytes, None)
            else:
                out[i] = stagewise(d, p, BATCH, o, 0, ptr, ptr, ptr, ptr, ws, ws_bytes, None)
        elif ex == MODEL:
            out[i] = plain_model(d, ptr, x0, goal, None, BATCH, o, ptr, ptr, ptr, ptr, None)
        elif ex == MODEL_BOUNDS:
            out[i] = model(d, ptr, e if has_e else None, x0, goal, None, BATCH, o, ptr, ptr, ptr, ptr, None)
        else:
            out[i] = qp(nu, mk, dt, ptr, ptr, ptr, ptr, BATCH, o, ptr, ptr, ptr, ptr, ws, ws_bytes, None)
    return out


if __name__ == "__main__":
    lib = _capi.load()
    rows = grid()
    if len(sys.argv) > 1 and sys.argv[1] == "--replay":  # the recorded (refused) rows only, in the grid's order
        z = np.load(sys.argv[2])
        assert int(z["grid_crc"]) == zlib.crc32(rows.tobytes()), "the grid is not the one the codes were recorded on"
        np.save(sys.argv[3], codes(lib, rows[z["codes"] < 0]))
        sys.exit(0)
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "refusal_codes.npz")
    rc = codes(lib, rows)
    refused = rc < 0
    # one code per row of grid(), 0 where the launch is served (not recorded, never replayed); the grid itself is code,
    # pinned by its checksum
    np.savez_compressed(out, codes=np.where(refused, rc, 0).astype(np.int8), grid_crc=np.uint32(zlib.crc32(rows.tobytes())))
    print(out, len(rows), "cases,", int(refused.sum()), "refused,", os.path.getsize(out), "bytes;",
          "codes of the rest:", sorted(set(rc[~refused].tolist())))
