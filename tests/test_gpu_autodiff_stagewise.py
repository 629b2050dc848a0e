"""The stage-wise adjoint on the MI355X: mpcqp_plan_vjp_stagewise_batch (qpmpc_amd/csrc/mpcqp_adjoint_stagewise.hip)
through solve_mpc_batch_diff(..., adjoint="stagewise") beyond the condensed adjoint's 128 variables, against the NumPy
restatements (tests/adjoint_stagewise_np.py, tests/adjoint_np.py, tests/adjoint_model_np.py) on every forward path, beside
the condensed adjoint where both apply, gradcheck, and the export's edge cases."""
import ctypes as C
import os

import numpy as np
import pytest

import adjoint_model_np as AM
import adjoint_np as AN
import adjoint_stagewise_np as AS
from golden_util import GOLDEN
from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from guarded_launch import _random_ltv, _torch, _triple  # noqa: E402  (needs torch)

KEYS = ("x0", "goal", "targets", "e")
MODEL = ("A", "B", "C", "D")
ALL = {"x0", "goal", "targets", "e", "A", "B", "C", "D", "wt", "wx", "wu"}


def _slack(w1, U):
    """e - C X - D U of a workload of one at its plan (rollout, no condensing)."""
    N = int(w1["N"])
    nx = w1["x0"].shape[1]
    A, B = AS._steps(w1, "A", (nx, nx)), AS._steps(w1, "B", (nx, -1))
    nu = B.shape[2]
    mk = np.asarray(w1["e"]).shape[-1]
    Cm, D = AS._steps(w1, "C", (mk, nx)), AS._steps(w1, "D", (mk, nu))
    u = np.asarray(U, dtype=float).reshape(N, nu)
    X = AS._rollout(A, B, np.asarray(w1["x0"][0], dtype=float), u)
    return (np.asarray(w1["e"], dtype=float).reshape(N, mk) - np.einsum("kri,ki->kr", Cm, X[:N])
            - np.einsum("kri,ki->kr", D, u)).ravel()


def _sw(bp, plan, gU, gX, want=frozenset(KEYS)):
    torch = _torch()
    from qpmpc_amd import autodiff

    g = autodiff._plan_vjp_stagewise(bp, plan, torch.as_tensor(gU, device=bp.device),
                                     None if gX is None else torch.as_tensor(gX, device=bp.device), set(want))
    torch.cuda.synchronize()
    return {k: (None if v is None else v.cpu().numpy().reshape(v.shape[0], -1)) for k, v in zip(autodiff.GRAD_KEYS, g)}


def _check_path(w, batch, seed, dtype=None, model=False, need=0.9, **solve_kw):
    """Forward solve with multipliers on the path ``solve_kw`` selects, then the stage-wise adjoint against the NumPy
    restatement (1e-8 relative), exact zeros of lam on slack rows, vjp_status == status where unsolved."""
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch

    rng = np.random.default_rng(seed)
    N, nx = int(w["N"]), np.asarray(w["x0"]).shape[1]
    n = N * np.asarray(w["B"]).shape[-1]
    gU = rng.standard_normal((batch, n))
    gX = rng.standard_normal((batch, (N + 1) * nx))
    bp = W.to_batch_problem(w, dtype=dtype)
    plan = solve_mpc_batch(bp, return_multipliers=True, **solve_kw)
    g = _sw(bp, plan, gU, gX, ALL if model else KEYS)
    if dtype is not None:  # the reference sees the operands the kernel sees: float32 storage, float64 arithmetic
        w = {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v)
             for k, v in w.items()}
    status = plan.status.cpu().numpy()
    vst = plan.vjp_status.cpu().numpy()
    lam = (np.zeros((batch, 0)) if plan.multipliers is None else plan.multipliers.double().cpu().numpy())
    U = plan.U.double().cpu().numpy()
    assert (status == 0).mean() >= need, status
    np.testing.assert_array_equal(vst[status != 0], status[status != 0])
    for b in np.flatnonzero(status == 0):
        w1 = AN.single(w, b)
        slack = _slack(w1, U[b])
        assert (lam[b][slack > 1e-6] == 0.0).all(), (b, lam[b][slack > 1e-6])
        ref = AS.stagewise_vjp(w1, lam[b], gU[b], gX[b], U=U[b] if model else None)
        assert vst[b] == ref["status"], (b, vst[b], ref["status"])
        if vst[b] != 0:
            continue
        for key in KEYS + (MODEL if model else ()):
            r = np.asarray(ref[key]).ravel()
            assert g[key][b].shape == r.shape, (b, key)
            if r.size == 0:  # (no constraint rows: g_e and g_C, g_D are empty)
                continue
            err = np.abs(g[key][b] - r).max()
            assert err <= 1e-8 * max(1.0, np.abs(r).max()), (b, key, err)
        if model:
            gw = np.array([g[k][b, 0] for k in ("wt", "wx", "wu")])
            assert np.abs(gw - ref["w"]).max() <= 1e-8 * max(1.0, np.abs(ref["w"]).max())
    assert (vst == 0).mean() >= need, vst
    return plan, g


def test_n140_gradients_match_the_condensed_restatement():
    """The envelope problem of test_gpu_autodiff.py::test_envelope (n = 140): BackendError by default, served here."""
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(10, 8, 3, 2, 70, 2)
    bp = W.to_batch_problem(w)
    x0 = torch.as_tensor(w["x0"], device=bp.device).clone().requires_grad_()
    goal = torch.as_tensor(w["goal"], device=bp.device).clone().requires_grad_()
    U, _, plan = solve_mpc_batch_diff(bp, initial_state=x0, goal_state=goal, adjoint="stagewise")
    wts = torch.linspace(-1.0, 2.0, U.numel(), dtype=U.dtype, device=U.device).reshape(U.shape)
    (U * wts).sum().backward()
    torch.cuda.synchronize()
    status = plan.status.cpu().numpy()
    assert (status == 0).all(), status
    assert (plan.vjp_status.cpu().numpy() == 0).all()
    lam = plan.multipliers.cpu().numpy()
    gU = wts.reshape(8, -1).cpu().numpy()
    for b in range(8):
        ref = AN.vjp(AN.single(w, b), lam[b], gU[b])
        for key, t in (("x0", x0), ("goal", goal)):
            got = t.grad[b].cpu().numpy()
            assert np.abs(got - ref[key]).max() <= 1e-8 * max(1.0, np.abs(ref[key]).max()), (b, key)


def test_wide_stagewise_kernel_path():
    from qpmpc_amd import _capi

    w = _random_ltv(11, 32, 6, 2, 80, 3)
    _check_path(w, 32, 11, formulation="stagewise", flags=_capi.OPT_STAGE_WIDE)


def test_general_stagewise_kernel_path():
    w = _random_ltv(12, 8, 20, 6, 40, 4)
    _check_path(w, 8, 12, formulation="stagewise")


def test_config5_shape_float32_storage():
    torch = _torch()
    w = W.synthetic_ltv_batch(16)
    _check_path(w, 16, 13, dtype=torch.float32)


def test_triple_integrator_n256():
    _check_path(_triple(16, 256), 16, 14, model=True)


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
    plan, _ = _check_path(w, B, 15, need=1.0, formulation="stagewise")
    assert (plan.multipliers > 0).sum(dim=1).min() >= 1


def test_model_gradients_beyond_128_with_a_shared_A():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    Bn, nx, nu, N, mk = 6, 3, 2, 70, 2
    w = _random_ltv(16, Bn, nx, nu, N, mk)
    A0 = w["A"][0, 0]
    # one A for every problem and step, scaled to spectral radius 0.98: the condensed reference multiplies A up to 70
    # times, and an unstable A (radius 1.16 here) costs it the digits this test compares
    w["A"] = (0.98 / np.abs(np.linalg.eigvals(A0)).max() * A0)[None, None]
    bp = W.to_batch_problem(w)
    dev = bp.device
    leaf = lambda a: torch.as_tensor(np.asarray(a), device=dev).clone().requires_grad_()  # noqa: E731
    A, Bm, Cm, D = leaf(w["A"]), leaf(w["B"]), leaf(w["C"]), leaf(w["D"])
    wt, wx, wu = leaf(w["wt"]), leaf(w["wx"]), leaf(w["wu"])
    x0 = leaf(w["x0"])
    U, X, plan = solve_mpc_batch_diff(bp, initial_state=x0, states=True, transition_state_matrix=A,
                                      transition_input_matrix=Bm, ineq_state_matrix=Cm, ineq_input_matrix=D,
                                      terminal_cost_weight=wt, stage_state_cost_weight=wx, stage_input_cost_weight=wu,
                                      adjoint="stagewise")
    rng = np.random.default_rng(16)
    gU = rng.standard_normal(U.shape)
    gX = rng.standard_normal(X.shape)
    ((U * torch.as_tensor(gU, device=dev)).sum() + (X * torch.as_tensor(gX, device=dev)).sum()).backward()
    torch.cuda.synchronize()
    assert (plan.status == 0).all() and (plan.vjp_status == 0).all()
    lam, Up = plan.multipliers.cpu().numpy(), plan.U.cpu().numpy()
    wref = dict(w, A=np.broadcast_to(w["A"], (Bn, N, nx, nx)).copy())
    refs = [AM.model_vjp(AN.single(wref, b), Up[b], lam[b], gU[b].ravel(), gX[b].ravel()) for b in range(Bn)]
    gA = sum(r["A"].sum(axis=0) for r in refs)

    def close(got, ref):
        assert np.abs(got - ref).max() <= 1e-8 * max(1.0, np.abs(ref).max())

    assert A.grad.shape == A.shape
    close(A.grad[0, 0].cpu().numpy(), gA)
    for b, r in enumerate(refs):
        close(Bm.grad[b].cpu().numpy(), r["B"])
        close(Cm.grad[b].cpu().numpy(), r["C"])
        close(D.grad[b].cpu().numpy(), r["D"])
        close(x0.grad[b].cpu().numpy(), r["x0"])
    gw = sum(r["w"] for r in refs)
    close(np.array([float(wt.grad), float(wx.grad), float(wu.grad)]), gw)


@pytest.mark.parametrize("which", ["config2", "wip50"])
def test_agrees_with_the_condensed_adjoint(which):
    torch = _torch()
    from qpmpc_amd import autodiff, solve_mpc_batch

    w = W.triple_integrator_batch(128) if which == "config2" else W.wip_batch(32, N=50)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    Bn, N, nx, n = bp.batch_size, bp.nb_timesteps, bp.state_dim, bp.nb_variables
    rng = np.random.default_rng(17)
    gU = torch.as_tensor(rng.standard_normal((Bn, n)), device=bp.device)
    gX = torch.as_tensor(rng.standard_normal((Bn, (N + 1) * nx)), device=bp.device)
    want = set(ALL)
    gm = autodiff._plan_vjp_model(bp, plan, gU, gX, want)
    vm = plan.vjp_status.clone()
    gs = autodiff._plan_vjp_stagewise(bp, plan, gU, gX, want)
    vs = plan.vjp_status.clone()
    gp = autodiff._plan_vjp(bp, plan, gU, gX, set(KEYS))
    torch.cuda.synchronize()
    assert torch.equal(vm, vs)
    ok = (vs == 0).cpu().numpy()
    assert ok.mean() >= 0.9
    for key, a, b in zip(autodiff.GRAD_KEYS, gm, gs):
        if a is None:
            assert b is None, key
            continue
        a, b = a.reshape(Bn, -1).cpu().numpy()[ok], b.reshape(Bn, -1).cpu().numpy()[ok]
        scale = np.maximum(1.0, np.abs(a).max(axis=1))
        assert (np.abs(a - b).max(axis=1) <= 1e-8 * scale).all(), key
    for key, a, b in zip(KEYS, gp, gs):
        a, b = a.reshape(Bn, -1).cpu().numpy()[ok], b.reshape(Bn, -1).cpu().numpy()[ok]
        assert (np.abs(a - b).max(axis=1) <= 1e-8 * np.maximum(1.0, np.abs(a).max(axis=1))).all(), key


def test_gradcheck_x0_beyond_128():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(18, 12, 3, 2, 70, 2)
    for b in range(12):
        U, lam, slack, st = AN.solve(AN.single(w, b))
        if st == 0 and AN.strictly_complementary(lam, slack):
            break
    else:
        raise AssertionError("no strictly complementary problem")
    w1 = AN.single(w, b)
    bp = W.to_batch_problem(w1)
    x0 = torch.as_tensor(w1["x0"], device=bp.device).clone().requires_grad_()

    def f(x0):
        return solve_mpc_batch_diff(bp, initial_state=x0, adjoint="stagewise")[0]

    assert torch.autograd.gradcheck(f, (x0,), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_no_constraint_rows():
    w = _random_ltv(19, 4, 3, 2, 70, 0)
    _check_path(w, 4, 19, need=1.0)


def test_zero_active_rows():
    w = _random_ltv(20, 4, 3, 2, 70, 2)
    w["e"] = w["e"] + 1e3
    plan, _ = _check_path(w, 4, 20, need=1.0, model=True, formulation="stagewise")
    assert (plan.multipliers == 0).all()


def _direct(w, lam, max_active):
    """mpcqp_plan_vjp_stagewise_batch called directly on made-up multipliers (status 0), outputs pre-filled with NaN."""
    torch = _torch()
    from qpmpc_amd import _capi, autodiff

    lib = _capi.load()
    bp = W.to_batch_problem(w)
    Bn, nx, n, m = bp.batch_size, bp.state_dim, bp.nb_variables, bp.nb_timesteps * bp.ineq_dim
    dev = bp.device
    dims, cp = autodiff._vjp_dims(bp), bp.c_problem()
    lam = torch.as_tensor(lam, dtype=torch.float64, device=dev).contiguous()
    status = torch.zeros(Bn, dtype=torch.int32, device=dev)
    gU = torch.ones((Bn, n), dtype=torch.float64, device=dev)
    g = {k: torch.full((Bn, s), float("nan"), dtype=torch.float64, device=dev) for k, s in (("x0", nx), ("e", m))}
    vst = torch.full((Bn,), -7, dtype=torch.int32, device=dev)
    nbytes = C.c_size_t(0)
    _capi.check(lib.mpcqp_plan_vjp_stagewise_workspace_bytes(C.byref(dims), Bn, max_active, C.byref(nbytes)), "ws")
    ws = torch.empty((nbytes.value,), dtype=torch.uint8, device=dev)
    out = _capi.VjpModelOut(g["x0"].data_ptr(), None, None, g["e"].data_ptr(), None, None, None, None, None)
    rc = lib.mpcqp_plan_vjp_stagewise_batch(C.byref(dims), C.byref(cp), Bn, max_active, lam.data_ptr(),
                                            status.data_ptr(), None, gU.data_ptr(), None, C.byref(out), vst.data_ptr(),
                                            ws.data_ptr(), ws.numel(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return vst.cpu().numpy(), g["x0"].cpu().numpy(), g["e"].cpu().numpy()


def test_too_few_slots_gives_slots_full_and_zeros():
    w = _random_ltv(21, 2, 3, 2, 70, 2)
    lam = np.zeros((2, 140))
    lam[0, [5, 40, 90]] = 1.0
    lam[1, [7]] = 1.0
    vst, gx0, ge = _direct(w, lam, 2)
    assert vst[0] == 4 and (gx0[0] == 0).all() and (ge[0] == 0).all()  # MPCQP_SLOTS_FULL
    assert vst[1] == 0 and np.isfinite(gx0[1]).all() and ge[1][7] != 0 and (np.delete(ge[1], 7) == 0).all()


def test_degenerate_active_sets_give_not_pd_and_zeros():
    w = _random_ltv(22, 3, 3, 2, 6, 4)  # n = 12, m = 24
    w["C"][1, 2, 2] = 0.0
    w["D"][1, 2, 2] = 0.0  # problem 1: a zero row
    lam = np.zeros((3, 24))
    lam[0, :13] = 1.0                   # problem 0: more active rows than variables
    lam[1, [2 * 4 + 2, 3]] = 1.0        # problem 1: the zero row (step 2, row 2) is active
    lam[2, [3, 9]] = 1.0                # problem 2: fine
    vst, gx0, ge = _direct(w, lam, 16)
    assert list(vst) == [3, 3, 0], vst  # MPCQP_NOT_PD
    assert (gx0[:2] == 0).all() and (ge[:2] == 0).all()
    ref = AS.stagewise_vjp(AN.single(w, 2), lam[2], np.ones(12))
    assert np.abs(gx0[2] - ref["x0"]).max() <= 1e-8 * max(1.0, np.abs(ref["x0"]).max())
    assert np.abs(ge[2] - ref["e"]).max() <= 1e-8 * max(1.0, np.abs(ref["e"]).max())
