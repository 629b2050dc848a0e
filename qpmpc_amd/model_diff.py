"""Derivatives of ``SharedModel`` plans: ``SharedModel.solve_diff``, ``.plan_jvp`` and ``.plan_jacobian``.

The forward is the model solve with multipliers (``mpcqp_solve_model_batch`` / ``_bounds_batch``); the backward is one
``mpcqp_model_vjp_batch`` call and the forward-mode pass one ``mpcqp_model_jvp_batch`` call (include/mpcqp.h): the KKT
adjoint of every plan on the factored model's whitened matrices, in HIP (qpmpc_amd/csrc/mpcqp_model_adjoint.hip) --
nothing is condensed again, P is not factored again and there is no workspace ("Shared-model
derivatives"). Gradients and tangents reach the initial state, the goal, the stage targets and the inequality vector;
the model matrices and the weights change the factorisation and stay with ``solve_mpc_batch_diff``.

The reference has no counterpart: its plans are NumPy arrays.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from .autodiff import (MAX_TANGENTS, TANGENT_NAMES, _as_float64, _detached, _is_dual, _ptr, _reduce, _tangent_operand)
from .batch import BatchMPCProblem, _as_tensor, _canon, _stream_ptr
from .exceptions import BackendError, ProblemDefinitionError

MAX_VARIABLES = 64  # envelope of mpcqp_model_vjp_batch / mpcqp_model_jvp_batch: n = N * nu <= 64


def _torch():
    import torch

    return torch


def check_envelope(model) -> None:
    """Raise ``BackendError`` unless the shared-model derivative exports serve this model (nothing is launched)."""
    n = model.template.nb_variables
    if n > MAX_VARIABLES:
        raise BackendError(f"derivatives of shared-model plans are served for n = N * nu <= {MAX_VARIABLES} variables, "
                           f"not {n}; solve_mpc_batch_diff differentiates larger problems")


MAX_VARIABLES_OWN_BOUNDS = 32  # envelope of mpcqp_solve_model_bounds_batch: n <= 16 (any dtype), float64 17 <= n <= 32 with m <= 64
MAX_ROWS_OWN_BOUNDS = 64


def per_problem_bounds(model, x0, ineq_vector):
    """``(e_canon [B|1, N|1, mk], e [B, N, mk])`` of an ``ineq_vector`` that gives every problem of a shared-model solve bounds
    of its own (the forward is then ``mpcqp_solve_model_bounds_batch``). Raises ``BackendError`` before anything is
    launched where that export refuses the model's size."""
    torch = _torch()
    t = model.template
    e_canon = _canon(_as_tensor(_detached(ineq_vector), t.dtype, t.device), (t.ineq_dim,), "ineq_vector")
    Bn = _as_tensor(_detached(x0), t.dtype, t.device).reshape(-1, t.state_dim).shape[0]
    if e_canon.shape[1] not in (1, t.nb_timesteps) or e_canon.shape[0] not in (1, Bn):
        raise ProblemDefinitionError(
            f"ineq_vector: shape {tuple(e_canon.shape)} is not [B|1, N|1, {t.ineq_dim}]")
    n, m = t.nb_variables, t.nb_constraints
    served = n <= 16 or (n <= MAX_VARIABLES_OWN_BOUNDS and m <= MAX_ROWS_OWN_BOUNDS and t.dtype == torch.float64)
    if Bn > 1 and not served:
        raise BackendError(
            f"a shared-model solve that gives every problem bounds of its own (ineq_vector) is served for n = N * nu <= 16 "
            f"variables and, in float64, for n <= {MAX_VARIABLES_OWN_BOUNDS} with at most {MAX_ROWS_OWN_BOUNDS} rows, not for "
            f"n = {n}, m = {m}; solve_mpc_batch and solve_mpc_batch_diff serve larger problems with per-problem bounds")
    return e_canon, e_canon.expand(Bn, -1, -1).contiguous()


def _float64_model(model):
    """The model the derivative exports read: ``model`` itself when it is float64, else a float64 twin factored on the
    first derivative call and kept (float32 problems are converted for the backward)."""
    torch = _torch()
    if model.template.dtype == torch.float64:
        return model
    if model._twin64 is None:
        model._twin64 = type(model)(_as_float64(model.template))
    return model._twin64


def _dynamics(m64):
    """The operands A and B of the float64 model, shared by the batch."""
    t = m64.template
    return BatchMPCProblem._operand(t.A), BatchMPCProblem._operand(t.B)


def _need_multipliers(model, plan) -> None:
    if model.template.ineq_dim > 0 and plan.multipliers is None:
        raise ProblemDefinitionError("derivatives of a plan need its multipliers: solve with return_multipliers=True")


def model_vjp(model, plan, gU, gX, want):
    """Float64 gradients ``(g_x0 [B, nx], g_goal [B, nx], g_targets [B, N*nx], g_e [B, N, mk])`` of the plan of a shared
    model, per problem, by one ``mpcqp_model_vjp_batch`` call; entries not in ``want`` (x0 is always computed) are None.
    Sets ``plan.vjp_status``."""
    torch = _torch()
    lib = _capi.load()
    check_envelope(model)
    _need_multipliers(model, plan)
    m64 = _float64_model(model)
    t = m64.template
    Bn, N, nx, mk, n = plan.U.shape[0], t.nb_timesteps, t.state_dim, t.ineq_dim, t.nb_variables
    dev = t.device
    f64 = dict(dtype=torch.float64, device=dev)
    gU = torch.zeros((Bn, n), **f64) if gU is None else gU.reshape(Bn, n).to(torch.float64).contiguous()
    gX = None if gX is None else gX.reshape(Bn, (N + 1) * nx).to(torch.float64).contiguous()
    lam = plan.multipliers.to(torch.float64).contiguous() if mk > 0 else None
    shapes = dict(x0=(nx,), goal=(nx,), targets=(N * nx,), e=(N, mk))
    want = {"x0"} | (set(want) & set(shapes))
    if mk == 0:
        want.discard("e")
    out = {k: (torch.empty((Bn,) + shp, **f64) if k in want else None) for k, shp in shapes.items()}
    vjp_status = torch.empty((Bn,), dtype=torch.int32, device=dev)
    A, B = _dynamics(m64)
    rc = lib.mpcqp_model_vjp_batch(
        C.byref(m64.dims), m64.model.data_ptr(), Bn, _ptr(lam), plan.status.data_ptr(), gU.data_ptr(), _ptr(gX),
        C.byref(A), C.byref(B), *[_ptr(out[k]) for k in ("x0", "goal", "targets", "e")], vjp_status.data_ptr(),
        _stream_ptr())
    _capi.check(rc, "mpcqp_model_vjp_batch")
    plan.vjp_status = vjp_status
    plan._vjp_keep = (m64, lam, gU, gX, A, B)  # alive until the stream has consumed them
    return tuple(out[k] for k in ("x0", "goal", "targets", "e"))


def model_jvp(model, plan, initial_state=None, goal_state=None, target_states=None, ineq_vector=None,
              states: bool = False):
    """``(dU [B, T, N, nu], dX [B, T, N+1, nx] or None)`` in float64, as ``mpcqp_model_jvp_batch`` wrote them. Sets
    ``plan.jvp_status``."""
    torch = _torch()
    lib = _capi.load()
    check_envelope(model)
    _need_multipliers(model, plan)
    m64 = _float64_model(model)
    t = m64.template
    Bn, N, nx, nu, mk = plan.U.shape[0], t.nb_timesteps, t.state_dim, t.input_dim, t.ineq_dim
    dev = t.device
    tails = ((nx,), (nx,), (N * nx,), (N, mk))
    ops = [_tangent_operand(v, nm, Bn, tail, dev) for v, nm, tail in zip(
        (initial_state, goal_state, target_states, ineq_vector), TANGENT_NAMES, tails)]
    if mk == 0:
        ops[3] = (None, 0)
    Ts = {v.shape[1] for v, _ in ops if v is not None}
    if not Ts:
        raise ProblemDefinitionError("plan_jvp: no tangent given")
    if len(Ts) > 1:
        raise ProblemDefinitionError(f"plan_jvp: the tangents disagree on T: {sorted(Ts)}")
    T = Ts.pop()
    if T > MAX_TANGENTS:
        raise ProblemDefinitionError(f"plan_jvp: T = {T} tangents, at most {MAX_TANGENTS} per call")
    f64 = dict(dtype=torch.float64, device=dev)
    lam = plan.multipliers.to(torch.float64).contiguous() if mk > 0 else None
    dU = torch.empty((Bn, T, N, nu), **f64)
    dX = torch.empty((Bn, T, N + 1, nx), **f64) if states else None
    jvp_status = torch.empty((Bn,), dtype=torch.int32, device=dev)
    tan = _capi.Tangents(*[_ptr(v) for v, _ in ops], *[st for _, st in ops])
    A, B = _dynamics(m64)
    rc = lib.mpcqp_model_jvp_batch(
        C.byref(m64.dims), m64.model.data_ptr(), Bn, T, _ptr(lam), plan.status.data_ptr(), C.byref(tan), C.byref(A),
        C.byref(B), dU.data_ptr(), _ptr(dX), jvp_status.data_ptr(), _stream_ptr())
    _capi.check(rc, "mpcqp_model_jvp_batch")
    plan.jvp_status = jvp_status
    plan._jvp_keep = (m64, lam, ops, tan, A, B)  # alive until the stream has consumed them
    return dU, dX


def plan_jvp(model, plan, initial_state=None, goal_state=None, target_states=None, ineq_vector=None,
             states: bool = False):
    dU, dX = model_jvp(model, plan, initial_state, goal_state, target_states, ineq_vector, states)
    dt = model.template.dtype
    return dU.to(dt), (None if dX is None else dX.to(dt))


JACOBIAN_WRT = ("initial_state", "goal_state")


def plan_jacobian(model, plan, wrt: str = "initial_state", states: bool = False):
    torch = _torch()
    if wrt not in JACOBIAN_WRT:
        raise ProblemDefinitionError(f"wrt: expected one of {JACOBIAN_WRT}, got {wrt!r}")
    t = model.template
    eye = torch.eye(t.state_dim, dtype=torch.float64, device=t.device)[None]
    dU, dX = plan_jvp(model, plan, states=states, **{wrt: eye})
    return dU.permute(0, 2, 3, 1), (None if dX is None else dX.permute(0, 2, 3, 1))


def _solve(model, work, solve_kw, multipliers: bool):
    run = model.prepare(work, return_multipliers=multipliers, **solve_kw)
    run.launch()
    return run.plan


def _make_function():
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class _ModelPlanFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, model, work, states, solve_kw, box, *operands):
            plan = _solve(model, work, solve_kw, True)
            U = plan.U.view(work.batch_size, work.nb_timesteps, work.input_dim)
            box["plan"] = plan
            ctx.model, ctx.work, ctx.plan, ctx.states = model, work, plan, states
            ctx.inputs = tuple(None if v is None else (v.shape, v.dtype, v.device) for v in operands)
            canon = (work.initial_state, work.goal_state, work.target_states, box["e_canon"])
            ctx.canon = tuple(None if v is None else c.shape for v, c in zip(operands, canon))
            return (U, plan.states) if states else U

        @staticmethod
        @once_differentiable
        def backward(ctx, gU, gX=None):
            need = ctx.needs_input_grad[5:]
            want = {nm for nm, nd in zip(("x0", "goal", "targets", "e"), need) if nd}
            grads = model_vjp(ctx.model, ctx.plan, gU, gX, want)
            out = [_reduce(g, like, canon) if nd else None
                   for nd, g, like, canon in zip(need, grads, ctx.inputs, ctx.canon)]
            return (None, None, None, None, None, *out)

        @staticmethod
        def jvp(ctx, *tangents):
            work = ctx.work
            Bn, N = work.batch_size, work.nb_timesteps
            args = {}
            for nm, v, canon in zip(TANGENT_NAMES, tangents[5:], ctx.canon):
                if v is None:
                    continue
                v = v.reshape(canon)
                if nm == "ineq_vector":
                    v = v.expand(-1, N, -1)
                args[nm] = v.unsqueeze(1)
            if args:
                dU, dX = plan_jvp(ctx.model, ctx.plan, states=ctx.states, **args)
                dU, dX = dU[:, 0], (None if dX is None else dX[:, 0])
            else:
                dU = torch.zeros((Bn, N, work.input_dim), dtype=work.dtype, device=work.device)
                dX = torch.zeros((Bn, N + 1, work.state_dim), dtype=work.dtype, device=work.device) if ctx.states else None
            return (dU, dX) if ctx.states else dU

    return _ModelPlanFunction


_FUNCTION = None


def solve_diff(model, x0, goal=None, targets=None, ineq_vector=None, states: bool = False, **solve_kw):
    global _FUNCTION
    torch = _torch()
    passed = (x0, goal, targets, ineq_vector)
    e_canon = e = None
    if ineq_vector is not None:
        e_canon, e = per_problem_bounds(model, x0, ineq_vector)
    work = model.problem_for(_detached(x0), _detached(goal), _detached(targets), e)
    dual = [_is_dual(v) for v in passed]
    need = any(dual) or (torch.is_grad_enabled()
                         and any(isinstance(v, torch.Tensor) and v.requires_grad for v in passed))
    if not need:
        plan = _solve(model, work, solve_kw, bool(solve_kw.pop("return_multipliers", False)))
        U = plan.U.view(work.batch_size, work.nb_timesteps, work.input_dim)
        return U, (plan.states if states else None), plan
    check_envelope(model)
    solve_kw.pop("return_multipliers", None)
    if _FUNCTION is None:
        _FUNCTION = _make_function()
    box = {"e_canon": e_canon}
    tens = [v if isinstance(v, torch.Tensor) else None for v in passed]
    out = _FUNCTION.apply(model, work, bool(states), dict(solve_kw), box, *tens)
    U, X = out if states else (out, None)
    return U, X, box["plan"]
