"""mpcqp_model_vjp_batch / mpcqp_model_jvp_batch held to the memory contract of include/mpcqp.h with tests/arena.py, as
tests/test_gpu_memory_discipline.py holds the other exports: every operand and output at its exact extent between
guards (the model at mpcqp_model_bytes), the outputs poisoned; afterwards the guards are intact, no NaN sits in an
output of a solved problem, the read-only buffers (the model included) are bitwise unchanged and NULL outputs are
respected. One small-kernel and one general-kernel shape, each with an odd batch."""
import ctypes as C

import numpy as np
import pytest

import arena as AR
import model_adjoint_np as MN
from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N,batch", [(8, 7), (32, 5)])  # n = 16 (sixteen lanes per problem), n = 64 (a workgroup each)
def test_model_derivatives_stay_inside_their_buffers(N, batch):
    import torch

    from qpmpc_amd import SharedModel, _capi
    from qpmpc_amd.batch import _stream_ptr

    lib = _capi.load()
    w = MN.mixed_batch(batch, seed=9 if N == 32 else 5, N=N)
    bp = W.to_batch_problem(w)
    sm = SharedModel(bp)
    plan = sm.solve(bp.initial_state, bp.goal_state, bp.target_states, return_multipliers=True)
    torch.cuda.synchronize()
    nx, nu, mk, n, m, T = 4, 2, 3, N * 2, N * 3, 3
    R = (N + 1) * nx
    f64, i32 = torch.float64, torch.int32
    sizes = dict(model=sm.model.numel(), lam=8 * batch * m, status=4 * batch, gU=8 * batch * n, gX=8 * batch * R,
                 A=8 * nx * nx, B=8 * nx * nu, dx0=8 * T * nx, dgoal=8 * batch * T * nx, dtargets=8 * batch * T * N * nx,
                 de=8 * batch * T * m, g_x0=8 * batch * nx, g_goal=8 * batch * nx, g_targets=8 * batch * N * nx,
                 g_e=8 * batch * m, vjp_status=4 * batch, dU=8 * batch * T * n, dX=8 * batch * T * R, jvp_status=4 * batch)
    ar = AR.Arena(AR.capacity_for(sizes.values()), device=bp.device)
    ints = ("status", "vjp_status", "jvp_status")
    v = {k: ar.carve(k, s, torch.uint8 if k == "model" else (i32 if k in ints else f64))[0] for k, s in sizes.items()}
    rng = np.random.default_rng(N)
    v["model"].copy_(sm.model)
    v["lam"].copy_(plan.multipliers.reshape(-1))
    status = plan.status.clone()
    status[2] = 2  # an unsolved problem among the solved ones
    v["status"].copy_(status)
    v["A"].copy_(bp.A.reshape(-1))
    v["B"].copy_(bp.B.reshape(-1))
    for k in ("gU", "gX", "dx0", "dgoal", "dtargets", "de"):
        v[k].copy_(torch.as_tensor(rng.standard_normal(v[k].numel()), device=bp.device))
    outputs = ("g_x0", "g_goal", "g_targets", "g_e", "vjp_status", "dU", "dX", "jvp_status")
    readonly = [k for k in sizes if k not in outputs]
    ar.fill(outputs, 0xFF)  # NaN / -1: a value that is not written shows
    ar.snapshot(readonly)
    dims = sm.dims
    A, B = _capi.Operand(ar.ptr("A"), 0, 0), _capi.Operand(ar.ptr("B"), 0, 0)
    tan = _capi.Tangents(ar.ptr("dx0"), ar.ptr("dgoal"), ar.ptr("dtargets"), ar.ptr("de"), 0, T * nx, T * N * nx, T * m)
    rc = lib.mpcqp_model_vjp_batch(C.byref(dims), ar.ptr("model"), batch, ar.ptr("lam"), ar.ptr("status"), ar.ptr("gU"),
                                   ar.ptr("gX"), C.byref(A), C.byref(B), ar.ptr("g_x0"), ar.ptr("g_goal"), None,
                                   ar.ptr("g_e"), ar.ptr("vjp_status"), _stream_ptr())
    assert rc == 0
    rc = lib.mpcqp_model_jvp_batch(C.byref(dims), ar.ptr("model"), batch, T, ar.ptr("lam"), ar.ptr("status"), C.byref(tan),
                                   C.byref(A), C.byref(B), ar.ptr("dU"), ar.ptr("dX"), ar.ptr("jvp_status"), _stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    assert ar.guards_intact() == []
    assert ar.unchanged() == []
    assert (ar.raw("g_targets") == 0xFF).all()  # a NULL output is not written
    np.testing.assert_array_equal(v["vjp_status"].cpu().numpy(), status.cpu().numpy())
    np.testing.assert_array_equal(v["jvp_status"].cpu().numpy(), status.cpu().numpy())
    for k in ("g_x0", "g_goal", "g_e", "dU", "dX"):
        out = v[k].reshape(batch, -1)
        assert not torch.isnan(out).any(), k
        assert (out[2] == 0).all(), k
    assert v["dU"].abs().sum() > 0 and v["g_x0"].abs().sum() > 0
    # the second launch without its optional arguments leaves their buffers alone
    ar.fill(("g_goal", "g_e", "vjp_status", "dX", "jvp_status"), 0xFF)
    assert lib.mpcqp_model_vjp_batch(C.byref(dims), ar.ptr("model"), batch, ar.ptr("lam"), ar.ptr("status"), ar.ptr("gU"),
                                     None, None, None, ar.ptr("g_x0"), None, None, None, None, _stream_ptr()) == 0
    assert lib.mpcqp_model_jvp_batch(C.byref(dims), ar.ptr("model"), batch, T, ar.ptr("lam"), ar.ptr("status"),
                                     C.byref(tan), None, None, ar.ptr("dU"), None, None, _stream_ptr()) == 0
    torch.cuda.synchronize()
    for k in ("g_goal", "g_e", "vjp_status", "dX", "jvp_status", "g_targets"):
        assert (ar.raw(k) == 0xFF).all(), k
    assert ar.guards_intact() == [] and ar.unchanged() == []
