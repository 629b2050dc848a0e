"""Model and cost gradients of batched plans on the MI355X: mpcqp_plan_vjp_model_batch (the kModel adjoint kernel of
qpmpc_amd/csrc/mpcqp_adjoint.hip) against the NumPy restatement of tests/adjoint_model_np.py on every forward path, the
four outputs it shares with mpcqp_plan_vjp_batch bitwise, torch.autograd.gradcheck with respect to A, B, C, D and the
weights, shared operands, unsolved problems, float32 storage, the routing of the backward and the envelope."""

import numpy as np
import pytest

import adjoint_model_np as AM
import adjoint_np as AN
from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from guarded_launch import _random_ltv, _torch  # noqa: E402  (needs torch)

KEYS = ("x0", "goal", "targets", "e")
MODEL = ("A", "B", "C", "D", "w")


def _check_path(w, seed, every=1, **solve_kw):
    """Forward with multipliers, then both exports on the same plan: the model export against the restatement (1e-8,
    relative to max(1, |g|)) on every ``every``-th solved problem, and the four shared outputs bitwise."""
    torch = _torch()
    from qpmpc_amd import autodiff, solve_mpc_batch

    rng = np.random.default_rng(seed)
    bp = W.to_batch_problem(w)
    Bn, N, nx, n = bp.batch_size, bp.nb_timesteps, bp.state_dim, bp.nb_variables
    gU = rng.standard_normal((Bn, n))
    gX = rng.standard_normal((Bn, (N + 1) * nx))
    plan = solve_mpc_batch(bp, return_multipliers=True, **solve_kw)
    tU, tX = torch.as_tensor(gU, device=bp.device), torch.as_tensor(gX, device=bp.device)
    plain = autodiff._plan_vjp(bp, plan, tU, tX, set(KEYS))
    vst_plain = plan.vjp_status.clone()
    model = autodiff._plan_vjp_model(bp, plan, tU, tX, set(autodiff.GRAD_KEYS))
    torch.cuda.synchronize()
    assert torch.equal(plan.vjp_status, vst_plain)
    for key, a, b in zip(KEYS, plain, model[:4]):
        assert torch.equal(a.reshape(Bn, -1), b.reshape(Bn, -1)), key
    g = dict(zip(autodiff.GRAD_KEYS, (t.cpu().numpy() for t in model)))
    g["w"] = np.stack([g["wt"], g["wx"], g["wu"]], axis=1)
    status, vst = plan.status.cpu().numpy(), plan.vjp_status.cpu().numpy()
    lam, U = plan.multipliers.cpu().numpy(), plan.U.cpu().numpy().reshape(Bn, n)
    assert (status == 0).mean() >= 0.9 and (vst == 0).mean() >= 0.9, (status, vst)
    checked = 0
    for b in np.flatnonzero(vst == 0)[::every]:
        an = AM.model_vjp(AN.single(w, b), U[b], lam[b], gU[b], gX[b])
        for key in MODEL:
            ref = an[key]
            err = np.abs(g[key][b] - ref).max() if ref.size else 0.0
            assert err <= 1e-8 * max(1.0, np.abs(ref).max() if ref.size else 0.0), (b, key, err)
        checked += 1
    assert checked >= 8, checked
    for key in MODEL:  # unsolved problems: zeros everywhere
        assert (g[key][vst != 0] == 0).all(), key
    return plan, g


def test_model_vjp_config2_four_per_wavefront():
    from qpmpc_amd import _capi

    _check_path(W.triple_integrator_batch(4096), 1, every=16, flags=_capi.OPT_FOUR_PER_WAVE)


def test_model_vjp_wip_n50():
    _check_path(W.wip_batch(1024, N=50), 2, every=16)


def test_model_vjp_random_ltv_condensed_and_stagewise():
    from qpmpc_amd import _capi

    w = _random_ltv(3, 64, 6, 2, 24, 3)
    pc, gc = _check_path(w, 3, flags=_capi.OPT_FORCE_CONDENSED)
    ps, gs = _check_path(w, 3, formulation="stagewise")
    same = ((pc.multipliers > 0) == (ps.multipliers > 0)).all(dim=1).cpu().numpy()
    same &= (pc.vjp_status == 0).cpu().numpy() & (ps.vjp_status == 0).cpu().numpy()
    assert same.mean() >= 0.9
    for key in MODEL:
        d = np.abs(gc[key] - gs[key]).reshape(64, -1).max(axis=1)
        scale = np.maximum(1.0, np.abs(gc[key]).reshape(64, -1).max(axis=1))
        assert (d[same] <= 1e-8 * scale[same]).all(), key


def test_model_vjp_stage_weight_without_targets():
    # MPCQP_P_STAGE without MPCQP_Q_STAGE: the stage term weighs the forced response
    w = _random_ltv(12, 64, 4, 2, 10, 2)
    w["targets"] = None
    _check_path(w, 12)


def test_model_vjp_n128_workspace_carve():
    # n = 128: three 128 x 129 float64 matrices alone exceed a CU's LDS, so the carve lives in the workspace
    w = _random_ltv(4, 16, 4, 2, 64, 2)
    _check_path(w, 4)


def _subset(w, idx):
    B = np.asarray(w["x0"]).shape[0]
    out = dict(w)
    for k, v in w.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B:
            out[k] = np.ascontiguousarray(v[idx])
    return out


def _leaf(a, bp, dtype=None):
    torch = _torch()
    return torch.as_tensor(np.array(a), dtype=dtype or bp.dtype, device=bp.device).requires_grad_()


@pytest.mark.parametrize("states", [False, True])
def test_gradcheck_model_and_weights(states):
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(5, 40, 3, 2, 5, 2)
    w = _subset(w, AN.complementary(w, 4))
    bp = W.to_batch_problem(w)
    ops = [_leaf(w[k], bp) for k in ("A", "B", "C", "D")] + [_leaf(w[k], bp) for k in ("wt", "wx", "wu")]

    def f(A, B, C, D, wt, wx, wu):
        U, X, _ = solve_mpc_batch_diff(bp, states=states, transition_state_matrix=A, transition_input_matrix=B,
                                       ineq_state_matrix=C, ineq_input_matrix=D, terminal_cost_weight=wt,
                                       stage_state_cost_weight=wx, stage_input_cost_weight=wu)
        return (U, X) if states else U

    assert torch.autograd.gradcheck(f, tuple(ops), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_shared_and_time_invariant_operands_get_the_sum():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(8, 24, 3, 2, 6, 2)
    A0, B0 = w["A"][0, 0], w["B"][0, 0]
    w["A"], w["B"] = A0, B0  # one A and one B for every problem and step
    bp = W.to_batch_problem(w)
    shared = [_leaf(A0, bp), _leaf(B0, bp), _leaf(np.asarray(w["wx"]), bp)]
    per = [_leaf(np.broadcast_to(A0, (24, 6, 3, 3)), bp), _leaf(np.broadcast_to(B0, (24, 6, 3, 2)), bp),
           _leaf(np.asarray(w["wx"]), bp)]
    wts = None
    for A, B, wx in (shared, per):
        U, X, plan = solve_mpc_batch_diff(bp, states=True, transition_state_matrix=A, transition_input_matrix=B,
                                          stage_state_cost_weight=wx)
        if wts is None:
            wts = torch.linspace(0.5, 1.5, U.numel(), dtype=U.dtype, device=U.device).reshape(U.shape)
        ((U * wts).sum() + X.square().sum()).backward()
        assert (plan.status == 0).double().mean() >= 0.5
    assert shared[0].grad.shape == (3, 3) and shared[1].grad.shape == (3, 2) and shared[2].grad.shape == ()
    for s, p in zip(shared, per):
        ref = p.grad.sum(dim=(0, 1)) if p.dim() == 4 else p.grad
        assert torch.allclose(s.grad, ref, rtol=1e-10, atol=1e-10 * max(1.0, float(ref.abs().max()))), (s.grad, ref)


def test_unsolved_problems_get_zero_model_gradients():
    torch = _torch()
    from qpmpc_amd import autodiff, solve_mpc_batch, solve_mpc_batch_diff

    w = _random_ltv(6, 32, 3, 2, 8, 2)
    for b in (3, 7, 20):  # two contradictory rows at step 0: c x + d u <= -1 and -(c x + d u) <= -1
        w["C"][b, 0, 1], w["D"][b, 0, 1] = -w["C"][b, 0, 0], -w["D"][b, 0, 0]
        w["e"][b, 0, :] = -1.0
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True, max_iter=3)
    gU = torch.ones((32, bp.nb_variables), dtype=torch.float64, device=bp.device)
    g = autodiff._plan_vjp_model(bp, plan, gU, None, set(autodiff.GRAD_KEYS))
    torch.cuda.synchronize()
    status = plan.status.cpu().numpy()
    assert (status[[3, 7, 20]] != 0).all() and (status == 0).any(), status
    np.testing.assert_array_equal(plan.vjp_status.cpu().numpy()[status != 0], status[status != 0])
    bad = torch.as_tensor(status != 0, device=bp.device)
    for key, t in zip(autodiff.GRAD_KEYS, g):
        assert not torch.isnan(t).any(), key
        assert (t[bad] == 0).all(), key
    assert (g[4][~bad].abs().sum(dim=(1, 2, 3)) > 0).any()
    # through the public function: the weights' sums stay finite and A's rows of unsolved problems stay zero
    A = _leaf(w["A"], bp)
    wt = _leaf(np.asarray(w["wt"]), bp)
    U, _, plan = solve_mpc_batch_diff(bp, transition_state_matrix=A, terminal_cost_weight=wt, max_iter=3)
    U.square().sum().backward()
    assert torch.isfinite(wt.grad) and (A.grad[bad] == 0).all()


def test_float32_storage_model_gradients():
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch_diff

    w = _random_ltv(9, 60, 3, 2, 6, 2)
    w = _subset(w, AN.complementary(w, 16))
    grads = {}
    for dt in (torch.float64, torch.float32):
        bp = W.to_batch_problem(w, dtype=dt)
        ops = [_leaf(w[k], bp) for k in ("A", "B", "C", "D")] + [_leaf(np.asarray(w[k]), bp) for k in ("wt", "wx", "wu")]
        U, X, plan = solve_mpc_batch_diff(bp, states=True, transition_state_matrix=ops[0], transition_input_matrix=ops[1],
                                          ineq_state_matrix=ops[2], ineq_input_matrix=ops[3], terminal_cost_weight=ops[4],
                                          stage_state_cost_weight=ops[5], stage_input_cost_weight=ops[6])
        (U.sum() + 0.5 * X.sum()).backward()
        assert (plan.status == 0).all()
        assert all(t.grad.dtype == dt for t in ops)
        grads[dt] = [t.grad.double().cpu().numpy() for t in ops]
    for g64, g32 in zip(grads[torch.float64], grads[torch.float32]):
        assert (np.abs(g32 - g64) <= 1e-3 * np.maximum(1.0, np.abs(g64).max())).all()


def test_backward_routing(monkeypatch):
    torch = _torch()
    from qpmpc_amd import autodiff, solve_mpc_batch_diff

    w = _random_ltv(13, 16, 3, 2, 6, 2)
    bp = W.to_batch_problem(w)
    calls = []
    plain, model = autodiff._plan_vjp, autodiff._plan_vjp_model
    monkeypatch.setattr(autodiff, "_plan_vjp", lambda *a: calls.append("plain") or plain(*a))
    monkeypatch.setattr(autodiff, "_plan_vjp_model", lambda *a: calls.append("model") or model(*a))
    x0 = _leaf(w["x0"], bp)
    A = torch.as_tensor(w["A"], device=bp.device)  # passed, but constant
    U, _, _ = solve_mpc_batch_diff(bp, initial_state=x0, transition_state_matrix=A)
    U.sum().backward()
    D = _leaf(w["D"], bp)
    U, _, _ = solve_mpc_batch_diff(bp, initial_state=x0, ineq_input_matrix=D)
    U.sum().backward()
    assert calls == ["plain", "model"]
    assert D.grad.shape == D.shape and torch.isfinite(D.grad).all()


def test_envelope_model_operands():
    torch = _torch()
    from qpmpc_amd import BackendError, ProblemDefinitionError, solve_mpc_batch_diff

    w = _random_ltv(10, 8, 3, 2, 70, 2)  # n = 140 > 128
    bp = W.to_batch_problem(w)
    with pytest.raises(BackendError):
        solve_mpc_batch_diff(bp, transition_state_matrix=_leaf(w["A"], bp))
    with pytest.raises(BackendError):
        solve_mpc_batch_diff(bp, stage_input_cost_weight=_leaf(np.asarray(w["wu"]), bp))
    with pytest.raises(ProblemDefinitionError):
        solve_mpc_batch_diff(bp, stage_input_cost_weight=torch.tensor(0.0, dtype=torch.float64))
    with pytest.raises(ProblemDefinitionError):
        solve_mpc_batch_diff(bp, transition_input_matrix=torch.zeros((3, 3), dtype=torch.float64))
