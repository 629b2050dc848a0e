"""Gradients through batched MPC plans: ``solve_mpc_batch_diff``.

The forward is ``solve_mpc_batch`` with multipliers; the backward is one call of ``mpcqp_plan_vjp_batch``
(include/mpcqp.h): the condensing of the batch into scratch, then one KKT adjoint solve per problem in HIP
(qpmpc_amd/csrc/mpcqp_adjoint.hip). Gradients reach the initial state, the goal, the stage targets and the inequality
vector ``e``; the model matrices and the cost weights are constants.

The reference has no counterpart: its plans are NumPy arrays.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from .batch import BatchMPCProblem, _canon, _as_tensor, _stream_ptr, solve_mpc_batch
from .exceptions import BackendError, ProblemDefinitionError

MAX_VARIABLES = 128  # envelope of mpcqp_plan_vjp_batch: n = N * nu <= 128 (and what mpcqp_condense_batch condenses)


def _torch():
    import torch

    return torch


def _detached(x):
    torch = _torch()
    return x.detach() if isinstance(x, torch.Tensor) else x


def _replaced(problem: BatchMPCProblem, x0, goal, targets, e) -> BatchMPCProblem:
    """A shallow copy of ``problem`` whose operands are replaced by the (detached) tensors passed, validated and
    canonicalised exactly as ``BatchMPCProblem`` does."""
    work = BatchMPCProblem.__new__(BatchMPCProblem)
    work.__dict__.update(problem.__dict__)
    if x0 is not None:
        work.update_initial_state(_detached(x0))
    if goal is not None:
        work.update_goal_state(_detached(goal))
    if targets is not None:
        work.update_target_states(_detached(targets))
    if e is not None:
        ev = _canon(_as_tensor(_detached(e), work.dtype, work.device), (work.ineq_dim,), "ineq_vector")
        if ev.shape[1] not in (1, work.nb_timesteps) or ev.shape[0] not in (1, work.batch_size):
            raise ProblemDefinitionError(f"ineq_vector: shape {tuple(ev.shape)} is not [B|1, N|1, {work.ineq_dim}]")
        work.e = ev
    return work


def _as_float64(problem: BatchMPCProblem) -> BatchMPCProblem:
    torch = _torch()
    if problem.dtype == torch.float64:
        return problem
    p64 = BatchMPCProblem.__new__(BatchMPCProblem)
    p64.__dict__.update(problem.__dict__)
    p64.dtype = torch.float64
    for name in ("A", "B", "C", "D", "e", "initial_state", "goal_state", "target_states"):
        t = getattr(problem, name)
        if t is not None:
            setattr(p64, name, t.to(torch.float64).contiguous())
    return p64


def _vjp_dims(problem: BatchMPCProblem) -> _capi.Dims:
    dims = problem.dims()
    dims.dtype = _capi.F64
    return dims


def check_envelope(problem: BatchMPCProblem) -> None:
    """Raise ``BackendError`` unless ``mpcqp_plan_vjp_batch`` serves this problem's dimensions (nothing is launched)."""
    lib = _capi.load()
    n = problem.nb_variables
    if n > MAX_VARIABLES:
        raise BackendError(f"gradients through plans are served for n = N * nu <= {MAX_VARIABLES} variables, not {n} "
                           "(a stage-wise adjoint for longer horizons is not built)")
    nbytes = C.c_size_t(0)
    dims = _vjp_dims(problem)
    rc = lib.mpcqp_plan_vjp_workspace_bytes(C.byref(dims), problem.batch_size, C.byref(nbytes))
    if rc != 0:
        _capi.check(rc, "mpcqp_plan_vjp_workspace_bytes")


def _reduce(g, like, canon_shape):
    """Sum the per-problem (per-step) gradient ``g`` over the dimensions the user's operand broadcast (size 1 in its
    canonical shape), then give it the user's shape, dtype and device (``like``)."""
    dims = [d for d, s in enumerate(canon_shape) if s == 1 and g.shape[d] != 1]
    if dims:
        g = g.sum(dim=dims, keepdim=True)
    shape, dtype, device = like
    return g.reshape(shape).to(dtype=dtype, device=device)


def _plan_vjp(work: BatchMPCProblem, plan, gU, gX, want):
    """(g_x0 [B,nx], g_goal [B,nx], g_targets [B,N*nx], g_e [B,N,mk]) in float64 through mpcqp_plan_vjp_batch; entries not
    in ``want`` are None. Sets ``plan.vjp_status``."""
    torch = _torch()
    lib = _capi.load()
    p64 = _as_float64(work)
    Bn, N, nx, mk, n = work.batch_size, work.nb_timesteps, work.state_dim, work.ineq_dim, work.nb_variables
    dev = work.device
    f64 = dict(dtype=torch.float64, device=dev)
    gU = torch.zeros((Bn, n), **f64) if gU is None else gU.reshape(Bn, n).to(torch.float64).contiguous()
    gX = None if gX is None else gX.reshape(Bn, (N + 1) * nx).to(torch.float64).contiguous()
    lam = plan.multipliers.to(torch.float64).contiguous() if mk > 0 else None
    g_x0 = torch.empty((Bn, nx), **f64)
    g_goal = torch.empty((Bn, nx), **f64) if "goal" in want else None
    g_tgt = torch.empty((Bn, N * nx), **f64) if "targets" in want else None
    g_e = torch.empty((Bn, N, mk), **f64) if "e" in want and mk > 0 else None
    vjp_status = torch.empty((Bn,), dtype=torch.int32, device=dev)
    dims, cp = _vjp_dims(p64), p64.c_problem()
    nbytes = C.c_size_t(0)
    _capi.check(lib.mpcqp_plan_vjp_workspace_bytes(C.byref(dims), Bn, C.byref(nbytes)), "mpcqp_plan_vjp_workspace_bytes")
    ws = torch.empty((max(nbytes.value, 1),), dtype=torch.uint8, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    rc = lib.mpcqp_plan_vjp_batch(
        C.byref(dims), C.byref(cp), Bn, ptr(lam), plan.status.data_ptr(), gU.data_ptr(), ptr(gX), g_x0.data_ptr(),
        ptr(g_goal), ptr(g_tgt), ptr(g_e), vjp_status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
    _capi.check(rc, "mpcqp_plan_vjp_batch")
    plan.vjp_status = vjp_status
    plan._vjp_keep = (ws, p64, lam, gU, gX)  # alive until the stream has consumed them
    if g_e is None and "e" in want:
        g_e = torch.zeros((Bn, N, mk), **f64)
    return g_x0, g_goal, g_tgt, g_e


def _make_function():
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class _PlanFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, work, states, solve_kw, box, x0, goal, targets, e):
            plan = solve_mpc_batch(work, return_multipliers=True, **solve_kw)
            U = plan.U.view(work.batch_size, work.nb_timesteps, work.input_dim)
            box["plan"] = plan
            ctx.work, ctx.plan, ctx.states = work, plan, states
            ctx.inputs = tuple(None if t is None else (t.shape, t.dtype, t.device) for t in (x0, goal, targets, e))
            ctx.canon = (work.initial_state.shape, work.goal_state.shape if goal is not None else None,
                         work.target_states.shape if targets is not None else None, work.e.shape if e is not None else None)
            return (U, plan.states) if states else U

        @staticmethod
        @once_differentiable
        def backward(ctx, gU, gX=None):
            need = ctx.needs_input_grad[4:]
            want = {nm for nm, nd in zip(("x0", "goal", "targets", "e"), need) if nd}
            grads = _plan_vjp(ctx.work, ctx.plan, gU, gX, want)
            out = [_reduce(g, like, canon) if nd else None
                   for nd, g, like, canon in zip(need, grads, ctx.inputs, ctx.canon)]
            return (None, None, None, None, *out)

    return _PlanFunction


_FUNCTION = None


def solve_mpc_batch_diff(problem: BatchMPCProblem, initial_state=None, goal_state=None, target_states=None,
                         ineq_vector=None, states: bool = False, **solve_kw):
    """Solve a batch like ``solve_mpc_batch`` and return ``(U, X, plan)`` whose ``U`` [B, N, nu] and, with ``states=True``,
    ``X`` [B, N+1, nx] carry a ``grad_fn`` (``X`` is None otherwise).

    ``initial_state``, ``goal_state``, ``target_states`` and ``ineq_vector`` replace the problem's own values when given
    and take the shapes ``BatchMPCProblem`` accepts (``[B, nx]``; ``[B|1, nx]`` or ``[nx]``; ``[B|1, N*nx]``;
    ``[B|1, N|1, mk]``, ``[N|1, mk]`` or ``[mk]``); the others are constants taken from ``problem``. A gradient reaching an
    operand shared by the batch (or by the steps) is the sum of the per-problem (per-step) gradients.

    The forward is ``solve_mpc_batch(..., return_multipliers=True, **solve_kw)`` on detached copies (every dispatch path
    of it returns multipliers, with exact zeros on inactive rows), then the rollout for ``X``. The backward is one
    ``mpcqp_plan_vjp_batch`` call (float64: a float32 problem's operands are converted, its gradients cast back). The
    active set is ``{i : lam_i > 0}``: at weakly active points (a tight row with a zero multiplier) the gradient is one
    element of the generalized Jacobian, as in OptNet. Problems that were not solved (``plan.status != 0``) get zero
    gradients; after the backward ``plan.vjp_status`` holds their status (and ``MPCQP_NOT_PD`` where the active rows'
    Gram matrix is singular). Envelope: n = N * nu <= 128; beyond it a request for gradients raises ``BackendError``
    before anything is launched. Only first derivatives (``once_differentiable``).

    When no operand passed requires grad (or grad mode is off), this is ``solve_mpc_batch(problem', **solve_kw)`` on the
    problem with the replaced operands, and its plan is returned as is."""
    global _FUNCTION
    torch = _torch()
    passed = (initial_state, goal_state, target_states, ineq_vector)
    work = _replaced(problem, *passed)
    need = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in passed)
    if not need:
        plan = solve_mpc_batch(work, **solve_kw)
        U = plan.U.view(work.batch_size, work.nb_timesteps, work.input_dim)
        return U, (plan.states if states else None), plan
    check_envelope(work)
    if _FUNCTION is None:
        _FUNCTION = _make_function()
    box = {}
    tens = [t if isinstance(t, torch.Tensor) else None for t in passed]
    out = _FUNCTION.apply(work, bool(states), dict(solve_kw), box, *tens)
    U, X = out if states else (out, None)
    return U, X, box["plan"]
