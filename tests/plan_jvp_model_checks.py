"""What the GPU tests of the model and weight tangents share (tests/test_gpu_plan_jvp_model.py on the condensed export,
tests/test_gpu_plan_jvp_model_stagewise.py on the stage-wise one): the tangents of every operand, the launch, and the checks
that take ``formulation``. Needs torch (through tests/guarded_launch.py): a test module puts pytest.importorskip("torch") in
front of importing it. pytest rewrites `assert` in test_*.py only, so the asserts here carry their own messages."""
import ctypes as C

import numpy as np

import adjoint_np as AN
import tangent_model_np as TM
from guarded_launch import _torch
from guarded_launch import _random_ltv as random_ltv  # noqa: F401  (the tests draw their workloads with it)
from host_helpers import dims_of
from qpmpc_amd import workloads as W

NAMES = dict(x0="initial_state", goal="goal_state", targets="target_states", e="ineq_vector",
             A="transition_state_matrix", B="transition_input_matrix", C="ineq_state_matrix", D="ineq_input_matrix")
WEIGHT_NAMES = ("terminal_cost_weight", "stage_state_cost_weight", "stage_input_cost_weight")
# the bound of tests/test_plan_jvp_model_cpu.py for central differences on the random LTV (3, 2, 5, 2) family
FD_BOUND_LTV = 1e-6


def model_tangents(w, B, T, rng, steps=None):
    """Random tangents {key: [B, T, ...]} of every operand: x0 .. e where the workload has them, A, B, C, D (of an absent
    C or D too: the tangent at zero) per step (``steps``: N, or 1 for time-invariant ones), and the weights' ``w``
    [B, T, 3], relative to each weight (zero where it is not set)."""
    N, nx, nu, mk = dims_of(w)
    steps = N if steps is None else steps
    tails = dict(x0=(nx,), goal=(nx,), targets=(N * nx,), e=(N, mk), A=(steps, nx, nx), B=(steps, nx, nu),
                 C=(steps, mk, nx), D=(steps, mk, nu))
    out = {}
    for key, tail in tails.items():
        if (key in ("x0", "goal", "targets", "e") and w[key] is None) or (key in "eCD" and mk == 0):
            continue
        out[key] = rng.standard_normal((B, T) + tail)
    scale = np.array([0.0 if w[k] is None else float(w[k]) for k in TM.WEIGHTS])
    out["w"] = rng.standard_normal((B, T, 3)) * scale
    return out


def keywords(tan, device):
    torch = _torch()
    kw = {NAMES[k]: torch.as_tensor(v, device=device) for k, v in tan.items() if k != "w"}
    if "w" in tan:
        dw = torch.as_tensor(tan["w"], device=device)
        kw.update({name: dw[..., j].contiguous() for j, name in enumerate(WEIGHT_NAMES)})
    return kw


def gpu_jvp(bp, plan, tan, formulation="condensed", states=True):
    """The float64 results as the export wrote them."""
    torch = _torch()
    from qpmpc_amd import autodiff

    kw = keywords(tan, bp.device)
    ops = [kw.get(NAMES[k]) for k in ("x0", "goal", "targets", "e")]
    dU, dX = autodiff._jvp(bp, plan, *ops, states, formulation, tuple(kw.get(NAMES[k]) for k in "ABCD"),
                           tuple(kw.get(n) for n in WEIGHT_NAMES))
    torch.cuda.synchronize()
    return dU, dX


def check_path(w, seed, T=3, limit=64, formulation="condensed", dtype=None, need=0.9, **solve_kw):
    """Forward solve with multipliers on the path ``solve_kw`` selects, then every operand's tangent at once against the
    restatement: 1e-8 max(1, |ref|) on dU and dX; at least ``need`` of the batch solved with jvp_status 0."""
    from qpmpc_amd import solve_mpc_batch

    rng = np.random.default_rng(seed)
    B = np.asarray(w["x0"]).shape[0]
    bp = W.to_batch_problem(w, dtype=dtype)
    plan = solve_mpc_batch(bp, return_multipliers=True, **solve_kw)
    tan = model_tangents(w, B, T, rng)
    if dtype is not None:  # the reference sees the operands the kernel sees: float32 storage, float64 arithmetic
        w = {k: (np.asarray(v, dtype=np.float32).astype(np.float64) if isinstance(v, np.ndarray) else v)
             for k, v in w.items()}
    dU, dX = gpu_jvp(bp, plan, tan, formulation)
    dU = dU.reshape(B, T, -1).cpu().numpy()
    dX = dX.reshape(B, T, -1).cpu().numpy()
    status = plan.status.cpu().numpy()
    vst = plan.jvp_status.cpu().numpy()
    lam = np.zeros((B, 0)) if plan.multipliers is None else plan.multipliers.double().cpu().numpy()
    U = plan.U.double().reshape(B, -1).cpu().numpy()
    assert (status == 0).mean() >= need, ("solved", status)
    np.testing.assert_array_equal(vst[status != 0], status[status != 0])
    assert (vst == 0).mean() >= need, vst
    checked = 0
    for b in np.flatnonzero(vst == 0)[:limit]:
        w1 = AN.single(w, b)
        for t in range(T):
            ref = TM.jvp_model(w1, U[b], lam[b], {k: v[b, t] for k, v in tan.items()})
            for key, got in (("U", dU[b, t]), ("X", dX[b, t])):
                err = np.abs(got - ref[key]).max()
                print(f"problem {b} tangent {t} d{key}: error {err:.3e}, |ref| {np.abs(ref[key]).max():.3e}")
                assert err <= 1e-8 * max(1.0, np.abs(ref[key]).max()), (b, t, key, err)
        checked += 1
    assert checked >= min(limit, B, 8) * need, ("problems compared", checked)
    return bp, plan, tan, dU, dX


def p_only(seed=11, B=16):
    w = random_ltv(seed, B, 3, 2, 5, 2)
    w["goal"], w["targets"] = None, None  # the P terms stay, no q term: E = Z, dE = zs
    w["e"] = w["e"].copy()
    w["e"][:, ::2, 0] -= 0.6  # (without a q term the plan is zero unless a row pushes it: these do)
    return w


def without(key, seed, B=16, dims=(3, 2, 8, 3)):
    w = random_ltv(seed, B, *dims)
    w[key] = None
    return w


def grads_of_model_vjp(bp, plan, gU, gX, backward):
    """{key: [B, ...]} of the model backward on the GPU: mpcqp_plan_vjp_model_batch or the stage-wise export."""
    torch = _torch()
    from qpmpc_amd import autodiff

    g = autodiff._vjp(bp, plan, torch.as_tensor(gU, device=bp.device), torch.as_tensor(gX, device=bp.device),
                      set(autodiff.GRAD_KEYS), backward)
    torch.cuda.synchronize()
    g = dict(zip(autodiff.GRAD_KEYS, [None if v is None else v.cpu().numpy() for v in g]))
    g["w"] = np.stack([g.pop("wt"), g.pop("wx"), g.pop("wu")], axis=1)
    return g


def check_duality(w, formulation, backward, seed=6):
    """<gU, dU> + <gX, dX> = sum over operands of <gradient, tangent>, the gradients from the GPU's model backward:
    1e-9 relative to the magnitude of the terms (the rounding bound of the inner products)."""
    from qpmpc_amd import solve_mpc_batch

    rng = np.random.default_rng(seed)
    B = np.asarray(w["x0"]).shape[0]
    N, nx, nu, mk = dims_of(w)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    tan = model_tangents(w, B, 1, rng)
    dU, dX = gpu_jvp(bp, plan, tan, formulation)
    gU = rng.standard_normal((B, N * nu))
    gX = rng.standard_normal((B, (N + 1) * nx))
    g = grads_of_model_vjp(bp, plan, gU, gX, backward)
    ok = (plan.vjp_status == 0).cpu().numpy() & (plan.jvp_status == 0).cpu().numpy()
    assert ok.mean() >= 0.9, ("solved with both statuses 0", float(ok.mean()))
    fwd = np.concatenate([gU * dU.reshape(B, -1).cpu().numpy(), gX * dX.reshape(B, -1).cpu().numpy()], axis=1)
    rev = np.concatenate([g[k].reshape(B, -1) * v.reshape(B, -1) for k, v in tan.items()], axis=1)
    lhs, rhs = fwd.sum(1), rev.sum(1)
    scale = np.maximum(1.0, np.maximum(np.abs(fwd).sum(1), np.abs(rev).sum(1)))
    print("duality: worst", (np.abs(lhs - rhs) / scale)[ok].max())
    assert (np.abs(lhs - rhs)[ok] <= 1e-9 * scale[ok]).all(), (np.abs(lhs - rhs) / scale)[ok].max()


def check_shared_and_time_invariant(w, formulation):
    """Tangents shared by the batch (stride 0) equal per-problem copies bitwise, and a step dimension of 1 equals the
    tangent expanded over the steps bitwise."""
    torch = _torch()
    from qpmpc_amd import plan_jvp, solve_mpc_batch

    B = np.asarray(w["x0"]).shape[0]
    N = int(w["N"])
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    one = keywords(model_tangents(w, 1, 4, np.random.default_rng(8)), bp.device)
    per = {k: v.expand(B, *v.shape[1:]).contiguous() for k, v in one.items()}
    dU1, dX1 = plan_jvp(bp, plan, states=True, formulation=formulation, **one)
    dU2, dX2 = plan_jvp(bp, plan, states=True, formulation=formulation, **per)
    torch.cuda.synchronize()
    assert torch.equal(dU1, dU2) and torch.equal(dX1, dX2), "tangents shared by the batch differ from their per-problem copies"
    assert dU1.abs().sum() > 0, "the tangents' responses are all zero"
    inv = keywords(model_tangents(w, B, 2, np.random.default_rng(9), steps=1), bp.device)
    full = {k: (v.expand(-1, -1, N, -1, -1).contiguous() if v.dim() == 5 else v) for k, v in inv.items()}
    dU1, dX1 = plan_jvp(bp, plan, states=True, formulation=formulation, **inv)
    dU2, dX2 = plan_jvp(bp, plan, states=True, formulation=formulation, **full)
    torch.cuda.synchronize()
    assert torch.equal(dU1, dU2) and torch.equal(dX1, dX2), "time-invariant tangents differ from their copies over the steps"
    assert dU1.abs().sum() > 0, "the tangents' responses are all zero"


def check_unsolved(w, formulation):
    """Two items with an infeasible e: zeros and jvp_status = status."""
    torch = _torch()
    from qpmpc_amd import plan_jvp, solve_mpc_batch

    B = np.asarray(w["x0"]).shape[0]
    bad_items = (3, B - 1)
    for b in bad_items:  # two contradictory rows at step 0
        w["C"][b, 0, 1], w["D"][b, 0, 1] = -w["C"][b, 0, 0], -w["D"][b, 0, 0]
        w["e"][b, 0, :] = -1.0
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    tan = keywords(model_tangents(w, B, 2, np.random.default_rng(9)), bp.device)
    dU, dX = plan_jvp(bp, plan, states=True, formulation=formulation, **tan)
    torch.cuda.synchronize()
    status = plan.status.cpu().numpy()
    assert (status[list(bad_items)] != 0).all() and (status == 0).any(), status
    np.testing.assert_array_equal(plan.jvp_status.cpu().numpy()[status != 0], status[status != 0])
    bad = torch.as_tensor(status != 0, device=bp.device)
    assert (dU[bad] == 0).all() and (dX[bad] == 0).all(), "an unsolved item's tangents are not zeros"
    assert not torch.isnan(dU).any() and not torch.isnan(dX).any(), "NaN in dU or dX"
    assert dU[~bad].abs().sum() > 0, "the solved items' tangents are all zero"


def direct_state_only(bp, plan, tan, stagewise):
    """(dU, dX, jvp_status) of the model export called with state tangents only (mtan with every pointer NULL)."""
    torch = _torch()
    from qpmpc_amd import _capi, autodiff
    from qpmpc_amd.batch import _stream_ptr

    lib = _capi.load()
    Bn, N, nx, nu, n = bp.batch_size, bp.nb_timesteps, bp.state_dim, bp.input_dim, bp.nb_variables
    ops = [torch.as_tensor(tan[k], device=bp.device).contiguous() for k in ("x0", "goal", "targets", "e")]
    T = ops[0].shape[1]
    ctan = _capi.Tangents(*[t.data_ptr() for t in ops], *[t[0].numel() for t in ops])
    mtan = _capi.ModelTangents()
    dims, cp = autodiff._vjp_dims(bp), bp.c_problem()
    f64 = dict(dtype=torch.float64, device=bp.device)
    dU, dX = torch.full((Bn, T, N, nu), np.nan, **f64), torch.full((Bn, T, N + 1, nx), np.nan, **f64)
    st = torch.full((Bn,), -9, dtype=torch.int32, device=bp.device)
    U = plan.U.reshape(Bn, n).contiguous()
    lam = plan.multipliers.contiguous()
    if stagewise:
        ka = autodiff._max_active(lam, plan.status, n)
        ws = autodiff._workspace_for(lib.mpcqp_plan_jvp_model_stagewise_workspace_bytes, dims, Bn, bp.device, ka, T)
        rc = lib.mpcqp_plan_jvp_model_stagewise_batch(
            C.byref(dims), C.byref(cp), Bn, ka, T, lam.data_ptr(), plan.status.data_ptr(), U.data_ptr(), C.byref(ctan),
            C.byref(mtan), dU.data_ptr(), dX.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
    else:
        ws = autodiff._workspace_for(lib.mpcqp_plan_jvp_model_workspace_bytes, dims, Bn, bp.device, T)
        rc = lib.mpcqp_plan_jvp_model_batch(
            C.byref(dims), C.byref(cp), Bn, T, lam.data_ptr(), plan.status.data_ptr(), U.data_ptr(), C.byref(ctan),
            C.byref(mtan), dU.data_ptr(), dX.data_ptr(), st.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
    assert rc == 0, f"return code {rc}"
    torch.cuda.synchronize()
    return dU, dX, st


def check_state_only_is_bitwise_the_old_export(w, formulation):
    torch = _torch()
    from qpmpc_amd import plan_jvp, solve_mpc_batch

    B = np.asarray(w["x0"]).shape[0]
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    tan = {k: v for k, v in model_tangents(w, B, 3, np.random.default_rng(14)).items() if k in ("x0", "goal", "targets", "e")}
    old_U, old_X = plan_jvp(bp, plan, states=True, formulation=formulation,
                            **{NAMES[k]: torch.as_tensor(v, device=bp.device) for k, v in tan.items()})
    torch.cuda.synchronize()
    old_st = plan.jvp_status.clone()
    dU, dX, st = direct_state_only(bp, plan, tan, formulation == "stagewise")
    assert torch.equal(dU, old_U) and torch.equal(dX, old_X) and torch.equal(st, old_st), "the state-only call differs from the old export"
    assert (old_st == 0).any() and old_U.abs().sum() > 0, old_st


def subset(w, idx):
    B = np.asarray(w["x0"]).shape[0]
    out = dict(w)
    for k, v in w.items():
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == B:
            out[k] = np.ascontiguousarray(v[idx])
    return out


def check_weight_jacobian(formulation):
    """plan_jacobian(wrt="cost_weights") against central differences of solve_mpc_batch in each weight (a relative step of
    1e-6) on strictly complementary problems of the random LTV (3, 2, 5, 2) family, at the bound the CPU test holds that
    family's central differences to."""
    torch = _torch()
    from qpmpc_amd import plan_jacobian, solve_mpc_batch

    w = random_ltv(11, 40, 3, 2, 5, 2)
    w = subset(w, AN.complementary(w, 8))
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    JU, JX = plan_jacobian(bp, plan, wrt="cost_weights", states=True, formulation=formulation)
    torch.cuda.synchronize()
    assert JU.shape == (8, 5, 2, 3) and JX.shape == (8, 6, 3, 3), (JU.shape, JX.shape)
    assert (plan.status == 0).all() and (plan.jvp_status == 0).all(), (plan.status, plan.jvp_status)
    step = 1e-6
    for j, key in enumerate(TM.WEIGHTS):
        ends = []
        for s in (step, -step):
            w2 = dict(w)
            w2[key] = float(w[key]) * (1.0 + s)
            bp2 = W.to_batch_problem(w2)
            p2 = solve_mpc_batch(bp2)
            assert (p2.status == 0).all(), (key, p2.status)
            ends.append((p2.U.reshape(8, -1), p2.states.reshape(8, -1)))
        for got, k in ((JU[..., j], 0), (JX[..., j], 1)):
            fd = (ends[0][k] - ends[1][k]) / (2 * step)      # dU / d(log w)
            got = got.reshape(8, -1) * float(w[key])
            scale = fd.abs().amax(dim=1).clamp(min=1.0)
            err = (got - fd).abs().amax(dim=1)
            print(f"{key} {'UX'[k]}: worst central-difference error {float((err / scale).max()):.3e}")
            assert (err <= FD_BOUND_LTV * scale).all(), (key, k, float((err / scale).max()))
        assert JU[..., j].abs().sum() > 0, (key, "a zero Jacobian")


def check_the_two_formulations_agree():
    """Each is held to the restatement at 1e-8 max(1, |ref|): to each other at twice that."""
    from qpmpc_amd import solve_mpc_batch

    w = random_ltv(5, 32, 4, 2, 12, 3)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True)
    tan = model_tangents(w, 32, 3, np.random.default_rng(13))
    dUc, dXc = gpu_jvp(bp, plan, tan, "condensed")
    okc = plan.jvp_status == 0
    dUs, dXs = gpu_jvp(bp, plan, tan, "stagewise")
    ok = okc & (plan.jvp_status == 0)
    assert ok.float().mean() >= 0.9, ("solved with both statuses 0", float(ok.float().mean()))
    for a, b in ((dUc, dUs), (dXc, dXs)):
        a, b = a[ok].flatten(2), b[ok].flatten(2)
        scale = a.abs().amax(dim=2).clamp(min=1.0)
        assert ((a - b).abs().amax(dim=2) <= 2e-8 * scale).all(), ((a - b).abs().amax(dim=2) / scale).max()
