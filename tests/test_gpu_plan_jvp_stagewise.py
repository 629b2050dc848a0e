"""The stage-wise tangent on the MI355X: mpcqp_plan_jvp_stagewise_batch (mpcqp_tangent_stagewise_kernel in
qpmpc_amd/csrc/mpcqp_adjoint_stagewise.hip) through plan_jvp / plan_jacobian(formulation="stagewise") and
solve_mpc_batch_diff(tangent="stagewise"), beyond the condensed tangent's 128 variables: against the NumPy restatement
(tests/tangent_stagewise_np.py) on the stage-wise adjoint's families, beside the condensed export where both apply, in
duality with the stage-wise adjoint, and the export's edge cases."""
import ctypes as C
import os

import numpy as np
import pytest

import adjoint_np as AN
import tangent_stagewise_np as TS
from golden_util import GOLDEN
from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from guarded_launch import _random_ltv, _torch, _triple  # noqa: E402  (needs torch)
from host_helpers import dims_of as _dims  # noqa: E402

NAMES = dict(x0="initial_state", goal="goal_state", targets="target_states", e="ineq_vector")


def _tangents(w, B, T, rng):
    """Per-problem random tangents {key: [B, T, ...]} of every operand the workload has."""
    N, nx, nu, mk = _dims(w)
    tails = dict(x0=(nx,), goal=(nx,), targets=(N * nx,), e=(N, mk))
    out = {}
    for key, tail in tails.items():
        if w[key] is None or (key == "e" and mk == 0):
            continue
        out[key] = rng.standard_normal((B, T) + tail)
    return out


def _gpu_jvp(bp, plan, tan, states=True, formulation="stagewise"):
    torch = _torch()
    from qpmpc_amd import plan_jvp

    kw = {NAMES[k]: torch.as_tensor(v, device=bp.device) for k, v in tan.items()}
    dU, dX = plan_jvp(bp, plan, states=states, formulation=formulation, **kw)
    torch.cuda.synchronize()
    return dU, dX


def _gpu_jvp64(bp, plan, tan, states=True):
    """The float64 results as the export wrote them, before plan_jvp casts them to a float32 problem's dtype."""
    torch = _torch()
    from qpmpc_amd import autodiff

    ops = [None if k not in tan else torch.as_tensor(tan[k], device=bp.device) for k in ("x0", "goal", "targets", "e")]
    dU, dX = autodiff._jvp(bp, plan, *ops, states, "stagewise")
    torch.cuda.synchronize()
    return dU, dX


def _check_path(w, seed, T=3, dtype=None, need=0.9, **solve_kw):
    """Forward solve with multipliers on the path ``solve_kw`` selects, then the stage-wise tangent against the NumPy
    restatement (1e-8 relative), with and without dX; jvp_status == status where unsolved."""
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch

    rng = np.random.default_rng(seed)
    B = np.asarray(w["x0"]).shape[0]
    bp = W.to_batch_problem(w, dtype=dtype)
    plan = solve_mpc_batch(bp, return_multipliers=True, **solve_kw)
    tan = _tangents(w, B, T, rng)
    if dtype is not None:  # the reference sees the operands the kernel sees: float32 storage, float64 arithmetic
        w = {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v)
             for k, v in w.items()}
    dU, dX = _gpu_jvp64(bp, plan, tan)
    vst = plan.jvp_status.cpu().numpy()
    dU0, none = _gpu_jvp64(bp, plan, tan, states=False)
    assert none is None and torch.equal(dU0, dU) and np.array_equal(plan.jvp_status.cpu().numpy(), vst)
    pU, pX = _gpu_jvp(bp, plan, tan)  # the public call: the same numbers in the problem's dtype
    assert pU.dtype == bp.dtype and torch.equal(pU, dU.to(bp.dtype)) and torch.equal(pX, dX.to(bp.dtype))
    dU = dU.reshape(B, T, -1).cpu().numpy()
    dX = dX.reshape(B, T, -1).cpu().numpy()
    status = plan.status.cpu().numpy()
    lam = np.zeros((B, 0)) if plan.multipliers is None else plan.multipliers.double().cpu().numpy()
    assert (status == 0).mean() >= need, status
    np.testing.assert_array_equal(vst[status != 0], status[status != 0])
    for b in np.flatnonzero(status == 0):
        fac = TS.Factorisation(AN.single(w, b), lam[b])
        assert vst[b] == fac.status, (b, vst[b], fac.status)
        if vst[b] != 0:
            continue
        for t in range(T):
            ref = fac.jvp({k: v[b, t] for k, v in tan.items()})
            for key, got in (("U", dU[b, t]), ("X", dX[b, t])):
                err = np.abs(got - ref[key]).max()
                assert err <= 1e-8 * max(1.0, np.abs(ref[key]).max()), (b, t, key, err)
    assert (vst == 0).mean() >= need, vst
    return bp, plan, tan


def test_n140_beyond_the_condensed_tangent():
    torch = _torch()
    from qpmpc_amd import BackendError, plan_jvp

    bp, plan, tan = _check_path(_random_ltv(10, 8, 3, 2, 70, 2), 10)
    with pytest.raises(BackendError, match="128"):
        plan_jvp(bp, plan, initial_state=torch.as_tensor(tan["x0"], device=bp.device))


def test_wide_stagewise_kernel_path():
    from qpmpc_amd import _capi

    _check_path(_random_ltv(11, 32, 6, 2, 80, 3), 11, formulation="stagewise", flags=_capi.OPT_STAGE_WIDE)


def test_general_stagewise_kernel_path():
    _check_path(_random_ltv(12, 8, 20, 6, 40, 4), 12, T=14, formulation="stagewise")  # 12 slots: two passes


def test_config5_shape_float32_storage():
    """float32 operands are converted; the comparison is on the float64 results, before the cast back."""
    torch = _torch()
    _check_path(W.synthetic_ltv_batch(16), 13, dtype=torch.float32)


def test_triple_integrator_n256():
    bp, plan, _ = _check_path(_triple(16, 256), 14, T=2)
    assert (plan.multipliers > 0).sum(dim=1).max() > 63  # S in the workspace, several passes of row sweeps


def test_golden_triple_integrator_n1024():
    from qpmpc_amd import MPCProblem

    z = np.load(os.path.join(GOLDEN, "stagewise_triple_n1024.npz"))
    N = int(z["nb_timesteps"])
    rng = np.random.default_rng(15)
    B = 3
    x0 = np.asarray(z["initial_state"], dtype=float)[None] + 0.05 * rng.standard_normal((B, 3))
    p = MPCProblem(z["A"], z["B"], z["C"], None, z["e"], N, float(z["terminal_cost_weight"]),
                   float(z["stage_state_cost_weight"]), float(z["stage_input_cost_weight"]), initial_state=x0[0],
                   goal_state=z["goal_state"])
    mk = np.asarray(z["e"]).reshape(-1).size
    w = dict(A=np.asarray(z["A"], dtype=float), B=np.asarray(z["B"], dtype=float), C=np.asarray(z["C"], dtype=float),
             D=None, e=np.broadcast_to(np.asarray(z["e"], dtype=float).reshape(mk), (N, mk)).copy(), N=N,
             wt=p.terminal_cost_weight, wx=p.stage_state_cost_weight, wu=p.stage_input_cost_weight, x0=x0,
             goal=np.broadcast_to(np.asarray(z["goal_state"], dtype=float), (B, 3)).copy(),
             targets=np.broadcast_to(np.asarray(z["target_states"], dtype=float).reshape(-1), (B, N * 3)).copy())
    bp, plan, _ = _check_path(w, 15, T=2, need=1.0, formulation="stagewise")
    assert (plan.multipliers > 0).sum(dim=1).min() >= 1


def test_no_constraint_rows():
    _check_path(_random_ltv(19, 4, 3, 2, 70, 0), 19, need=1.0)


def test_zero_active_rows():
    w = _random_ltv(20, 4, 3, 2, 70, 2)
    w["e"] = w["e"] + 1e3
    bp, plan, _ = _check_path(w, 20, need=1.0, formulation="stagewise")
    assert (plan.multipliers == 0).all()


@pytest.mark.parametrize("seed,dims,few", [(10, (3, 2, 70, 2), 100), (12, (20, 6, 40, 4), 13)])
def test_a_tangent_does_not_depend_on_its_slot_pass_or_T(seed, dims, few):
    """T = 1, a T that is not a multiple of the 256 / max(nx, nu) slots (85 and 12 here) and T = 256: bitwise the same
    results for the tangents they share."""
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch

    w = _random_ltv(seed, 8, *dims)  # (the batches of the path tests above)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True, formulation="stagewise")
    assert (plan.status == 0).any() and (plan.multipliers > 0).any()
    tan = _tangents(w, 8, 256, np.random.default_rng(23))
    dU, dX = _gpu_jvp(bp, plan, tan)
    assert (plan.jvp_status == plan.status).all() and dU.abs().sum() > 0
    for T in (1, few):
        dUt, dXt = _gpu_jvp(bp, plan, {k: np.ascontiguousarray(v[:, :T]) for k, v in tan.items()})
        assert torch.equal(dUt, dU[:, :T]) and torch.equal(dXt, dX[:, :T]), T
    # ... nor on its position: the last tangents alone
    dUt, dXt = _gpu_jvp(bp, plan, {k: np.ascontiguousarray(v[:, 250:]) for k, v in tan.items()})
    assert torch.equal(dUt, dU[:, 250:]) and torch.equal(dXt, dX[:, 250:])


@pytest.mark.parametrize("which", ["config2", "wip50"])
def test_agrees_with_the_condensed_export(which):
    from qpmpc_amd import solve_mpc_batch

    w = W.triple_integrator_batch(128) if which == "config2" else W.wip_batch(32, N=50)
    B = np.asarray(w["x0"]).shape[0]
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    tan = _tangents(w, B, 3, np.random.default_rng(17))
    cU, cX = _gpu_jvp(bp, plan, tan, formulation="condensed")
    vc = plan.jvp_status.clone()
    sU, sX = _gpu_jvp(bp, plan, tan)
    vs = plan.jvp_status.clone()
    assert (vc == vs).all()
    ok = (vs == 0).cpu().numpy()
    assert ok.mean() >= 0.9
    for a, b in ((cU, sU), (cX, sX)):
        a, b = a.reshape(B, -1).cpu().numpy()[ok], b.reshape(B, -1).cpu().numpy()[ok]
        scale = np.maximum(1.0, np.abs(a).max(axis=1))
        assert (np.abs(a - b).max(axis=1) <= 1e-8 * scale).all(), np.abs(a - b).max()


def test_duality_with_the_stagewise_vjp_export_beyond_128():
    torch = _torch()
    from qpmpc_amd import autodiff, solve_mpc_batch

    w = _random_ltv(10, 8, 3, 2, 70, 2)
    rng = np.random.default_rng(24)
    B = 8
    N, nx, nu, mk = _dims(w)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    tan = _tangents(w, B, 1, rng)
    dU, dX = _gpu_jvp(bp, plan, tan)
    gU = rng.standard_normal((B, N * nu))
    gX = rng.standard_normal((B, (N + 1) * nx))
    g = autodiff._plan_vjp_stagewise(bp, plan, torch.as_tensor(gU, device=bp.device),
                                     torch.as_tensor(gX, device=bp.device), {"x0", "goal", "targets", "e"})
    torch.cuda.synchronize()
    g = dict(zip(("x0", "goal", "targets", "e"), [v.reshape(B, -1).cpu().numpy() for v in g[:4]]))
    ok = (plan.vjp_status == 0).cpu().numpy() & (plan.jvp_status == 0).cpu().numpy()
    assert ok.mean() >= 0.9
    fwd = np.concatenate([gU * dU.reshape(B, -1).cpu().numpy(), gX * dX.reshape(B, -1).cpu().numpy()], axis=1)
    rev = np.concatenate([g[k] * v.reshape(B, -1) for k, v in tan.items()], axis=1)
    lhs, rhs = fwd.sum(1), rev.sum(1)
    # relative to the magnitude of the terms (the rounding bound of an inner product), as for the condensed pair
    scale = np.maximum(1.0, np.maximum(np.abs(fwd).sum(1), np.abs(rev).sum(1)))
    assert (np.abs(lhs - rhs)[ok] <= 1e-10 * scale[ok]).all(), np.abs(lhs - rhs)[ok].max()


def test_plan_jacobian_without_active_rows_is_the_riccati_gain_beyond_128():
    torch = _torch()
    from oracle.stagewise_np import Riccati, from_mpc_problem
    from qpmpc_amd import plan_jacobian, solve_mpc_batch
    from qpmpc_amd.workloads import problem_from_workload

    w = _random_ltv(7, 8, 4, 2, 80, 2)  # n = 160
    w["e"] = np.full_like(w["e"], 1e6)  # no row can be active
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    JU, JX = plan_jacobian(bp, plan, states=True, formulation="stagewise")
    torch.cuda.synchronize()
    assert JU.shape == (8, 80, 2, 4) and JX.shape == (8, 81, 4, 4)
    assert (plan.status == 0).all() and (plan.jvp_status == 0).all() and (plan.multipliers == 0).all()
    JU, JX = JU.cpu().numpy(), JX.cpu().numpy()
    for b in range(8):
        K0 = Riccati(from_mpc_problem(problem_from_workload(AN.single(w, b), 0))).K[0]
        np.testing.assert_allclose(JU[b, 0], -K0, rtol=0, atol=1e-8 * max(1.0, np.abs(K0).max()))
        np.testing.assert_array_equal(JX[b, 0], np.eye(4))


@pytest.mark.parametrize("wrt", ["initial_state", "goal_state"])
def test_plan_jacobian_with_active_rows_is_nx_plan_jvp_calls(wrt):
    torch = _torch()
    from qpmpc_amd import plan_jacobian, plan_jvp, solve_mpc_batch

    w = _random_ltv(25, 8, 4, 2, 80, 2)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    assert (plan.multipliers > 0).any()
    JU, JX = plan_jacobian(bp, plan, wrt=wrt, states=True, formulation="stagewise")
    assert (plan.jvp_status == plan.status).all() and JU.abs().sum() > 0
    for j in range(4):
        ej = torch.zeros((1, 1, 4), dtype=torch.float64, device=bp.device)
        ej[0, 0, j] = 1.0
        dU, dX = plan_jvp(bp, plan, states=True, formulation="stagewise", **{wrt: ej})
        torch.cuda.synchronize()
        assert torch.equal(JU[..., j], dU[:, 0]) and torch.equal(JX[..., j], dX[:, 0]), j


def test_shared_tangents_are_bitwise_per_problem_copies():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch

    w = _random_ltv(8, 12, 3, 2, 70, 2)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    one = {k: v[:1] for k, v in _tangents(w, 1, 4, np.random.default_rng(8)).items()}
    per = {k: np.repeat(v, 12, axis=0) for k, v in one.items()}
    dU1, dX1 = _gpu_jvp(bp, plan, one)
    dU2, dX2 = _gpu_jvp(bp, plan, per)
    assert torch.equal(dU1, dU2) and torch.equal(dX1, dX2)
    assert dU1.abs().sum() > 0


def _direct(w, lam, status, max_active, T=2):
    """mpcqp_plan_jvp_stagewise_batch called directly on the multipliers and status passed, outputs pre-filled with NaN;
    the tangents are ones in dx0 and de."""
    torch = _torch()
    from qpmpc_amd import _capi, autodiff

    lib = _capi.load()
    bp = W.to_batch_problem(w)
    Bn, N, nx, n, m = bp.batch_size, bp.nb_timesteps, bp.state_dim, bp.nb_variables, bp.nb_timesteps * bp.ineq_dim
    dev = bp.device
    dims, cp = autodiff._vjp_dims(bp), bp.c_problem()
    lam = torch.as_tensor(lam, dtype=torch.float64, device=dev).contiguous()
    status = torch.as_tensor(status, dtype=torch.int32, device=dev).contiguous()
    dx0 = torch.ones((Bn, T, nx), dtype=torch.float64, device=dev)
    de = torch.ones((T, m), dtype=torch.float64, device=dev)  # shared
    dU = torch.full((Bn, T, n), float("nan"), dtype=torch.float64, device=dev)
    dX = torch.full((Bn, T, (N + 1) * nx), float("nan"), dtype=torch.float64, device=dev)
    vst = torch.full((Bn,), -7, dtype=torch.int32, device=dev)
    nbytes = C.c_size_t(0)
    _capi.check(lib.mpcqp_plan_jvp_stagewise_workspace_bytes(C.byref(dims), Bn, max_active, T, C.byref(nbytes)), "ws")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    tan = _capi.Tangents(dx0.data_ptr(), None, None, de.data_ptr(), T * nx, 0, 0, 0)
    rc = lib.mpcqp_plan_jvp_stagewise_batch(C.byref(dims), C.byref(cp), Bn, max_active, T, lam.data_ptr(),
                                            status.data_ptr(), C.byref(tan), dU.data_ptr(), dX.data_ptr(),
                                            vst.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return vst.cpu().numpy(), dU.cpu().numpy(), dX.cpu().numpy()


def _ones(w, b, lam, T=2):
    N, nx, nu, mk = _dims(w)
    return TS.stagewise_jvp(AN.single(w, b), lam, {"x0": np.ones(nx), "e": np.ones(N * mk)})


def _close(got, ref):
    assert np.abs(got - ref).max() <= 1e-8 * max(1.0, np.abs(ref).max())


def test_unsolved_problems_get_zeros_and_their_status():
    w = _random_ltv(26, 4, 3, 2, 70, 2)
    lam = np.zeros((4, 140))
    lam[:, [5, 40]] = 1.0
    lam[1] = np.nan  # an unsolved problem's multipliers are not read
    vst, dU, dX = _direct(w, lam, [0, 2, 0, 1], 4)
    assert list(vst) == [0, 2, 0, 1]
    assert (dU[[1, 3]] == 0).all() and (dX[[1, 3]] == 0).all()
    assert np.isfinite(dU).all() and np.isfinite(dX).all()  # nothing left unwritten
    for b in (0, 2):
        ref = _ones(w, b, lam[b])
        for t in range(2):
            _close(dU[b, t], ref["U"])
            _close(dX[b, t], ref["X"])


def test_too_few_slots_gives_slots_full_and_zeros():
    w = _random_ltv(21, 2, 3, 2, 70, 2)
    lam = np.zeros((2, 140))
    lam[0, [5, 40, 90]] = 1.0
    lam[1, [7]] = 1.0
    vst, dU, dX = _direct(w, lam, [0, 0], 2)
    assert vst[0] == 4 and (dU[0] == 0).all() and (dX[0] == 0).all()  # MPCQP_SLOTS_FULL
    assert vst[1] == 0
    ref = _ones(w, 1, lam[1])
    _close(dU[1, 0], ref["U"])
    _close(dX[1, 1], ref["X"])


def test_degenerate_active_sets_give_not_pd_and_zeros():
    w = _random_ltv(22, 3, 3, 2, 6, 4)  # n = 12, m = 24
    w["C"][1, 2, 2] = 0.0
    w["D"][1, 2, 2] = 0.0  # problem 1: a zero row
    lam = np.zeros((3, 24))
    lam[0, :13] = 1.0                   # problem 0: more active rows than variables
    lam[1, [2 * 4 + 2, 3]] = 1.0        # problem 1: the zero row (step 2, row 2) is active
    lam[2, [3, 9]] = 1.0                # problem 2: fine
    vst, dU, dX = _direct(w, lam, [0, 0, 0], 16)
    assert list(vst) == [3, 3, 0], vst  # MPCQP_NOT_PD
    assert (dU[:2] == 0).all() and (dX[:2] == 0).all()
    ref = _ones(w, 2, lam[2])
    _close(dU[2, 1], ref["U"])
    _close(dX[2, 0], ref["X"])


def test_a_batch_the_host_splits_equals_the_unsplit_one(monkeypatch):
    torch = _torch()
    from qpmpc_amd import _capi, autodiff, solve_mpc_batch

    w = _random_ltv(27, 24, 3, 2, 70, 2)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    rng = np.random.default_rng(27)
    tan = _tangents(w, 24, 3, rng)
    tan["goal"] = tan["goal"][:1]  # one shared tangent among per-problem ones
    dU, dX = _gpu_jvp(bp, plan, tan)
    vst = plan.jvp_status.clone()
    max_active = autodiff._max_active(plan.multipliers, plan.status, bp.nb_variables)
    one = autodiff._workspace_bytes(_capi.load().mpcqp_plan_jvp_stagewise_workspace_bytes, autodiff._vjp_dims(bp), 1,
                                    max_active, 3)
    monkeypatch.setattr(autodiff, "STAGEWISE_WORKSPACE_CAP", 5 * one)  # launches of 5, 5, 5, 5 and 4 problems
    dU2, dX2 = _gpu_jvp(bp, plan, tan)
    assert len(plan._jvp_keep[-1]) == 1 + 5
    assert torch.equal(dU, dU2) and torch.equal(dX, dX2) and torch.equal(vst, plan.jvp_status)
    assert (vst == 0).any() and dU.abs().sum() > 0


def test_forward_ad_with_tangent_stagewise_at_n140():
    torch = _torch()
    from torch.autograd import forward_ad as fwAD

    from qpmpc_amd import BackendError, plan_jvp, solve_mpc_batch_diff

    w = _random_ltv(28, 8, 3, 2, 70, 2)
    bp = W.to_batch_problem(w)
    dev = bp.device
    rng = np.random.default_rng(28)
    prim = {k: torch.as_tensor(w[k], device=dev) for k in ("x0", "goal")}
    tan = {k: torch.as_tensor(rng.standard_normal(v.shape), device=dev) for k, v in prim.items()}
    with fwAD.dual_level():
        duals = {NAMES[k]: fwAD.make_dual(prim[k], tan[k]) for k in prim}
        with pytest.raises(BackendError, match="128"):
            solve_mpc_batch_diff(bp, states=True, **duals)
        U, X, plan = solve_mpc_batch_diff(bp, states=True, tangent="stagewise", **duals)
        tU, tX = fwAD.unpack_dual(U).tangent, fwAD.unpack_dual(X).tangent
    assert tU is not None and tX is not None
    assert (plan.status == 0).any() and (plan.jvp_status == plan.status).all()
    # bitwise the export with T = 1 on the same plan
    ref_U, ref_X = plan_jvp(bp, plan, states=True, initial_state=tan["x0"][:, None], goal_state=tan["goal"][:, None],
                            formulation="stagewise")
    torch.cuda.synchronize()
    assert torch.equal(tU, ref_U[:, 0]) and torch.equal(tX, ref_X[:, 0])
    assert tU.abs().sum() > 0
