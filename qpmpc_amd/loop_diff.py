"""Gradients through closed loops of a ``SharedModel``: ``closed_loop_diff``.

The forward is ``ModelClosedLoop.step(nb_periods)`` -- one ``mpcqp_model_periods_batch`` launch for all periods, with
records --; the backward is one ``mpcqp_model_periods_vjp_batch`` launch (include/mpcqp.h): the reverse-time recursion
through the periods, each period the KKT adjoint of ``mpcqp_model_vjp_batch`` on the factored model, in HIP
(qpmpc_amd/csrc/mpcqp_model_adjoint.hip, ``mpcqp_loop_adjoint_small_kernel``; DESIGN.md section 9, "Closed-loop adjoint").
The fused forward keeps only the last period's multipliers, so the recorded states are solved again -- one
``mpcqp_solve_model_batch`` launch over all ``B * P`` (loop, period) pairs, fully parallel -- and that replay's multipliers
and statuses feed the backward.

Forward mode is ``closed_loop_jvp`` / ``closed_loop_jacobian``: the same forward and replay, then one
``mpcqp_model_periods_jvp_batch`` launch -- the forward-time recursion through the periods for every tangent, each period's
active rows factored once (qpmpc_amd/csrc/mpcqp_loop_tangent.hip, ``mpcqp_loop_tangent_small_kernel``; DESIGN.md section 9,
"Closed-loop forward sensitivities"). ``closed_loop_diff`` serves ``torch.autograd.forward_ad`` duals through it.

The reference has no counterpart: its closed loops are Python loops over NumPy plans.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from .autodiff import MAX_TANGENTS, _detached, _is_dual, _ptr, _reduce
from .batch import _stream_ptr
from .exceptions import BackendError, ProblemDefinitionError

OPERANDS = ("x0", "goal", "targets", "disturbance", "Ap", "Bp")


def _torch():
    import torch

    return torch


class LoopDiffInfo:
    """What ``closed_loop_diff`` reports next to the trajectories (device tensors; nothing here synchronises).

    ``status``        int32 ``[B, P]``, every period's solver status -- the replay's (``fused=True`` with a gradient) or the
                      per-period solves' (``fused=False``); None for a fused call that needed no gradient, which keeps
                      the last period's only (``loop.status``)
    ``failed``        0-d int64: periods of any loop without a plan (the zero input was applied)
    ``vjp_status``    int32 ``[B]`` after a backward, None before: per loop the number of periods with a plan whose active
                      rows' Gram matrix failed the pivot test or that had more active rows than variables (such a period
                      contributes its plant term only)
    ``jvp_status``    int32 ``[B]`` after a forward-mode pass (``closed_loop_jvp``, ``closed_loop_jacobian``, a ``forward_ad``
                      dual), None otherwise: the same count as ``vjp_status``, by ``mpcqp_model_periods_jvp_batch``
    ``replay_error``  0-d float64, ``max |U0_replay - U0| / max(1, |U0|)``: how far the replayed solves' first inputs are
                      from the recorded ones (None when nothing was replayed)
    ``loop``          the ``ModelClosedLoop`` that ran the forward (``fused=True``)"""

    def __init__(self):
        self.status = self.failed = self.vjp_status = self.jvp_status = self.replay_error = self.loop = None
        self._plans = None

    def _by_hand_vjp_status(self):
        torch = _torch()
        bad = [(p.vjp_status != p.status) for p in self._plans if getattr(p, "vjp_status", None) is not None]
        self.vjp_status = torch.stack(bad, 1).sum(1).to(torch.int32) if bad else None
        return self.vjp_status


def check_envelope(model) -> None:
    """Raise ``BackendError`` unless ``closed_loop_diff(fused=True)`` serves this model (nothing is launched)."""
    torch = _torch()
    t = model.template
    n, m, nx = t.nb_variables, t.nb_constraints, t.state_dim
    if t.dtype != torch.float64 or n > 16 or not (1 <= m <= 32) or nx > 16 or model.per_problem_bounds:
        raise BackendError(
            "closed_loop_diff(fused=True) serves float64 models with N nu <= 16, 1 <= N mk <= 32, nx <= 16 and the model's "
            f"own bounds (mpcqp_model_periods_batch / mpcqp_model_periods_vjp_batch); this one has N nu = {n}, N mk = {m}, "
            f"nx = {nx}, {t.dtype}" + (", bounds per problem" if model.per_problem_bounds else "")
            + ". fused=False composes the loop from SharedModel.solve_diff and serves everything that serves.",
            code=_capi.EUNSUPPORTED)


def _replay(model, loop, X, U0, P):
    """Solve the recorded states again, all (loop, period) pairs in one launch -> (lam [B, P, m], status [B, P], error)."""
    torch = _torch()
    B, nx, N = loop.batch, loop.nx, loop.N

    def flat(ref, w):
        if ref is None:
            return None
        a = ref[0]
        a = a[:, :P] if a.ndim == 3 else (a[:, None] if a.ndim == 2 else a[None, None])
        return a.expand(B, P, w).reshape(B * P, w)

    work = model.problem_for(X[:, :P].reshape(B * P, nx), flat(loop._goal, nx), flat(loop._targets, N * nx))
    run = model.prepare(work, return_multipliers=True, max_iter=loop._max_iter, feas_tol=loop._feas_tol)
    run.launch()
    u0 = torch.where((run.status == 0)[:, None], run.U[:, :loop.nu], torch.zeros((), dtype=U0.dtype, device=U0.device))
    err = ((u0.view(B, P, loop.nu) - U0).abs() / U0.abs().clamp_min(1.0)).max()
    return run.lam.view(B, P, -1), run.status.view(B, P), err, run


def loop_vjp(model, loop, lam, status, X, U0, gX, gU0, want):
    """One ``mpcqp_model_periods_vjp_batch`` launch. ``want``: the names of OPERANDS whose gradient is needed (x0 always
    is); goal / targets / disturbance that are constant over the periods come back with a period axis of 1 (summed in the
    kernel; the disturbance in torch). -> (dict of per-loop float64 gradients, vjp_status [B])."""
    torch = _torch()
    lib = _capi.load()
    B, P, nx, nu, N = loop.batch, U0.shape[1], loop.nx, loop.nu, loop.N
    f64 = dict(dtype=torch.float64, device=X.device)
    prep = lambda g: None if g is None else g.to(torch.float64).contiguous()  # noqa: E731
    gX, gU0 = prep(gX), prep(gU0)
    out = {"x0": torch.empty((B, nx), **f64)}
    g_states = torch.empty((B, P + 1, nx), **f64) if "disturbance" in want else None

    def period_grad(name, ref, w):
        if name not in want or ref is None:
            return None, None
        a = ref[0]
        if a.ndim == 3:  # a period axis: the periods past P keep their zeros
            g = torch.zeros((B, a.shape[1], w), **f64)
            return g, _capi.PeriodGrad(g.data_ptr(), a.shape[1] * w, w)
        g = torch.empty((B, 1, w), **f64)
        return g, _capi.PeriodGrad(g.data_ptr(), w, 0)

    out["goal"], gg = period_grad("goal", loop._goal, nx)
    out["targets"], gt = period_grad("targets", loop._targets, N * nx)
    out["Ap"] = torch.empty((B, nx, nx), **f64) if "Ap" in want else None
    out["Bp"] = torch.empty((B, nx, nu), **f64) if "Bp" in want else None
    vjp_status = torch.empty((B,), dtype=torch.int32, device=X.device)
    plant = _capi.LoopPlant(_capi.Operand(loop._Ap.data_ptr(), nx * nx if loop._Ap.ndim == 3 else 0, 0),
                            _capi.Operand(loop._Bp.data_ptr(), nx * nu if loop._Bp.ndim == 3 else 0, 0),
                            _capi.Operand(None, 0, 0))
    rc = lib.mpcqp_model_periods_vjp_batch(
        C.byref(model.dims), model.model.data_ptr(), C.byref(plant), B, P, lam.data_ptr(), status.data_ptr(),
        X.data_ptr() if out["Ap"] is not None else None, U0.data_ptr() if out["Bp"] is not None else None, _ptr(gX),
        _ptr(gU0), out["x0"].data_ptr(), _ptr(g_states), None if gg is None else C.byref(gg),
        None if gt is None else C.byref(gt), _ptr(out["Ap"]), _ptr(out["Bp"]), vjp_status.data_ptr(), _stream_ptr())
    _capi.check(rc, "mpcqp_model_periods_vjp_batch")
    out["disturbance"] = None
    if g_states is not None and loop._dist is not None:
        gd, a = g_states[:, 1:], loop._dist[0]
        if a.ndim == 3:
            if a.shape[1] > P:
                gd = torch.cat([gd, torch.zeros((B, a.shape[1] - P, nx), **f64)], dim=1)
        else:
            gd = gd.sum(dim=1, keepdim=True)
        out["disturbance"] = gd
    loop._vjp_keep = (gX, gU0, lam, status, X, U0, plant, gg, gt)  # alive until the stream has consumed them
    return out, vjp_status


TANGENTS = ("d_x0", "d_goal", "d_targets", "d_disturbance", "d_Ap", "d_Bp")


def _loop_tangents(tangents, B, P, nx, nu, N, device):
    """The six tangents (the order of TANGENTS, None = zero) as contiguous float64 tensors -> (list, T). A tangent is
    ``[B|1, T, *tail]``; one of a reference may carry a period axis, ``[B|1, T, P' >= P, w]``, or none (constant in time)."""
    torch = _torch()
    tails = ((nx,), (nx,), (N * nx,), (nx,), (nx, nx), (nx, nu))
    out, Ts = [], set()
    for name, v, tail in zip(TANGENTS, tangents, tails):
        if v is None:
            out.append(None)
            continue
        v = torch.as_tensor(v, device=device).to(torch.float64)
        periodic = name in ("d_goal", "d_targets", "d_disturbance") and v.dim() == 4
        want = 2 + len(tail) + int(periodic)
        if (v.dim() != want or tuple(v.shape[-len(tail):]) != tail or v.shape[0] not in (1, B) or v.shape[1] < 1
                or (periodic and v.shape[2] < P)):
            shape = ", ".join(str(d) for d in tail)
            raise ProblemDefinitionError(
                f"{name}: tangent of shape {tuple(v.shape)} is not [{B}|1, T, {shape}]"
                + (f" or [{B}|1, T, P >= {P}, {shape}]" if len(tail) == 1 and name != "d_x0" else ""))
        Ts.add(v.shape[1])
        out.append(v.contiguous())
    if not Ts:
        raise ProblemDefinitionError("closed_loop_jvp: no tangent given")
    if len(Ts) > 1:
        raise ProblemDefinitionError(f"closed_loop_jvp: the tangents disagree on T: {sorted(Ts)}")
    T = Ts.pop()
    if T > MAX_TANGENTS:
        raise ProblemDefinitionError(f"closed_loop_jvp: T = {T} tangents, at most {MAX_TANGENTS} per call")
    return out, T


def loop_jvp(model, loop, lam, status, X, U0, tangents):
    """One ``mpcqp_model_periods_jvp_batch`` launch. ``tangents``: what ``_loop_tangents`` returned.
    -> (dX [B, T, P+1, nx], dU0 [B, T, P, nu], jvp_status [B]), float64."""
    torch = _torch()
    lib = _capi.load()
    tans, T = tangents
    B, P, nx, nu = loop.batch, U0.shape[1], loop.nx, loop.nu
    f64 = dict(dtype=torch.float64, device=X.device)
    dX, dU0 = torch.empty((B, T, P + 1, nx), **f64), torch.empty((B, T, P, nu), **f64)
    jvp_status = torch.empty((B,), dtype=torch.int32, device=X.device)
    shared = lambda v: v.shape[0] == 1 and B > 1  # noqa: E731

    def flat(v):
        return (None, 0) if v is None else (v.data_ptr(), 0 if shared(v) else v[0].numel())

    def periodic(v):
        if v is None:
            return _capi.PeriodTangent(None, 0, 0, 0)
        return _capi.PeriodTangent(v.data_ptr(), 0 if shared(v) else v[0].numel(), v[0, 0].numel(),
                                   v.shape[-1] if v.dim() == 4 else 0)

    d_x0, d_goal, d_targets, d_dist, d_Ap, d_Bp = tans
    tan = _capi.LoopTangents(*flat(d_x0), periodic(d_goal), periodic(d_targets), periodic(d_dist), *flat(d_Ap), *flat(d_Bp))
    plant = _capi.LoopPlant(_capi.Operand(loop._Ap.data_ptr(), nx * nx if loop._Ap.ndim == 3 else 0, 0),
                            _capi.Operand(loop._Bp.data_ptr(), nx * nu if loop._Bp.ndim == 3 else 0, 0),
                            _capi.Operand(None, 0, 0))
    rc = lib.mpcqp_model_periods_jvp_batch(
        C.byref(model.dims), model.model.data_ptr(), C.byref(plant), B, P, T, lam.data_ptr(), status.data_ptr(),
        X.data_ptr() if d_Ap is not None else None, U0.data_ptr() if d_Bp is not None else None, C.byref(tan),
        dX.data_ptr(), dU0.data_ptr(), jvp_status.data_ptr(), _stream_ptr())
    _capi.check(rc, "mpcqp_model_periods_jvp_batch")
    loop._jvp_keep = (tans, lam, status, X, U0, plant, tan)  # alive until the stream has consumed them
    return dX, dU0, jvp_status


def _canon(name, v, loop):
    """The shape ``autodiff._reduce`` takes as the operand's canonical one: a size of 1 where the operand broadcasts."""
    if name == "x0":
        return (loop.batch, loop.nx)
    if name in ("Ap", "Bp"):
        return ((1,) if v.ndim == 2 else (v.shape[0],)) + tuple(v.shape[-2:])
    w = v.shape[-1]
    if v.ndim == 3:
        return (v.shape[0], v.shape[1], w)
    return (v.shape[0] if v.ndim == 2 else 1, 1, w)


def _make_function():
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class _ClosedLoopFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, model, loop, P, info, *operands):
            loop.step(P)
            X, U0 = loop.X, loop.U0
            lam, status, err, run = _replay(model, loop, X, U0, P)
            info.status, info.replay_error = status, err
            ctx.model, ctx.loop, ctx.info, ctx.keep = model, loop, info, (lam, status, X, U0, run)
            ctx.inputs = tuple(None if v is None else (v.shape, v.dtype, v.device) for v in operands)
            ctx.canon = tuple(None if v is None else _canon(nm, v, loop) for nm, v in zip(OPERANDS, operands))
            ctx.set_materialize_grads(False)
            return X, U0

        @staticmethod
        @once_differentiable
        def backward(ctx, gX, gU0):
            need = ctx.needs_input_grad[4:]
            want = {nm for nm, nd in zip(OPERANDS, need) if nd}
            lam, status, X, U0, _ = ctx.keep
            grads, ctx.info.vjp_status = loop_vjp(ctx.model, ctx.loop, lam, status, X, U0, gX, gU0, want)
            out = [_reduce(grads[nm], like, canon) if nd and grads[nm] is not None else None
                   for nm, nd, like, canon in zip(OPERANDS, need, ctx.inputs, ctx.canon)]
            return (None, None, None, None, *out)

        @staticmethod
        def jvp(ctx, *tangents):
            loop = ctx.loop
            lam, status, X, U0, _ = ctx.keep
            args = []
            for nm, v, canon in zip(OPERANDS, tangents[4:], ctx.canon):
                if v is None:
                    args.append(None)
                    continue
                v = v.reshape(canon).unsqueeze(1)  # T = 1
                if nm in ("goal", "targets", "disturbance") and canon[1] == 1:
                    v = v[:, :, 0]  # constant in time
                args.append(v)
            if all(v is None for v in args):
                return torch.zeros_like(X), torch.zeros_like(U0)
            tans = _loop_tangents(args, loop.batch, U0.shape[1], loop.nx, loop.nu, loop.N, X.device)
            dX, dU0, ctx.info.jvp_status = loop_jvp(ctx.model, loop, lam, status, X, U0, tans)
            return dX[:, 0].to(X.dtype), dU0[:, 0].to(U0.dtype)

    return _ClosedLoopFunction


_FUNCTION = None


def _by_hand(model, x0, P, goal, targets, plant, disturbance, feas_tol, max_iter, info):
    """The loop composed in torch: ``SharedModel.solve_diff`` and the plant step per period."""
    torch = _torch()
    t = model.template
    as_t = lambda v: None if v is None else torch.as_tensor(v, dtype=t.dtype, device=t.device)  # noqa: E731
    x, goal, targets, dist = as_t(x0), as_t(goal), as_t(targets), as_t(disturbance)
    Ap, Bp = (t.A[0, 0], t.B[0, 0]) if plant is None else (as_t(plant[0]), as_t(plant[1]))
    for ref, what in ((goal, "goal"), (targets, "targets"), (dist, "disturbance")):
        if ref is not None and ref.ndim == 3 and ref.shape[1] < P:
            raise ValueError(f"{what} is laid out for {ref.shape[1]} periods; {P} were asked for")
    at = lambda r, k: None if r is None else (r[:, k] if r.ndim == 3 else r)  # noqa: E731
    zero = torch.zeros((), dtype=t.dtype, device=t.device)
    X, U0, plans = [x], [], []
    for k in range(P):
        U, _, plan = model.solve_diff(x, at(goal, k), at(targets, k), return_multipliers=True, feas_tol=feas_tol,
                                      max_iter=max_iter)
        u0 = torch.where((plan.status == 0)[:, None], U[:, 0, :], zero)
        xa = torch.bmm(Ap, x[:, :, None])[:, :, 0] if Ap.ndim == 3 else x @ Ap.T
        xb = torch.bmm(Bp, u0[:, :, None])[:, :, 0] if Bp.ndim == 3 else u0 @ Bp.T
        x = xa + xb if dist is None else xa + xb + at(dist, k)
        X.append(x)
        U0.append(u0)
        plans.append(plan)
    info._plans = plans
    info.status = torch.stack([p.status for p in plans], dim=1)
    info.failed = (info.status != 0).sum()
    return torch.stack(X, dim=1), torch.stack(U0, dim=1)


def closed_loop_diff(model, x0, nb_periods, goal=None, targets=None, plant=None, disturbance=None, warm: bool = False,
                     feas_tol: float = 1e-9, max_iter=None, fused: bool = True):
    """Run ``B`` closed loops of a :class:`SharedModel` for ``nb_periods`` periods and return ``(X, U0, info)`` whose
    ``X`` [B, P+1, nx] (the state before every period and after the last) and ``U0`` [B, P, nu] (the input applied in
    every period) carry a ``grad_fn``.

    Shapes, broadcasting and the loop's rules are :class:`ModelClosedLoop`'s: ``x0`` [B, nx]; ``goal``, ``targets`` and
    ``disturbance`` constant (``[w]``, ``[B|1, w]``) or with a period axis (``[B|1, P, w]``); ``plant=(Ap, Bp)`` shared
    or per loop, the model's own A, B by default; a period without a plan applies the zero input and passes the
    gradient through the plant only. Gradients reach whichever of ``x0``, ``goal``, ``targets``, ``disturbance``,
    ``Ap`` and ``Bp`` are tensors that require grad, each reduced to the operand's own shape: summed over the batch
    where the batch shares it, over the periods (inside the kernel) where it is constant in time. The model matrices,
    the weights and the model's ``e`` are NOT differentiated here -- they change the factorisation; ``solve_mpc_batch_diff``
    differentiates single plans with respect to them. The active set of a period is ``{i : lam_i > 0}``, as in every
    derivative export. ``torch.autograd.forward_ad`` duals on the same six operands are served too (``fused=True``): the
    forward, the replay and one ``mpcqp_model_periods_jvp_batch`` launch with one tangent per call, as :func:`closed_loop_jvp`.

    ``fused=True``: the forward is ONE ``mpcqp_model_periods_batch`` launch with records (``warm`` is passed through) and
    the backward ONE ``mpcqp_model_periods_vjp_batch`` launch. When a gradient is needed the recorded states are solved
    again with multipliers -- one ``mpcqp_solve_model_batch`` launch over the ``B * P`` (loop, period) pairs with the
    loop's ``feas_tol`` / ``max_iter``, launched with the forward -- because the fused loop keeps only its last period's
    multipliers; ``info.replay_error`` says how far the replayed first inputs are from the recorded ones. Replay buffers
    are ``B * P * (n + m)`` doubles (plans and multipliers, n = N nu, m = N mk) plus ``2 B P`` int32, and where the
    problem has them ``B * P * nx`` (goal) and ``B * P * N nx`` (targets) doubles of expanded references; they live until
    the backward. Envelope: float64, N nu <= 16, 1 <= N mk <= 32, nx <= 16, the model's own bounds -- ``BackendError``
    outside it, before anything is launched. With nothing requiring grad (or under ``torch.no_grad``) the call is
    ``ModelClosedLoop.step(nb_periods)`` and returns its records.

    ``fused=False``: the loop composed in torch from ``SharedModel.solve_diff`` and the plant step, two launches and a
    dozen small torch operations per period in each direction; it serves everything ``solve_diff`` serves and is the
    baseline the fused path is measured against. ``warm`` is ignored there (every solve is cold).

    Measured (profiles/loop_diff.md, tools/bench_loop_diff.py: triple-integrator family, 50 periods, one MI355X, forward +
    backward in ms, composed / fused): B = 256: 13.8 / 1.32; 1024: 13.7 / 1.43; 4096: 15.0 / 1.98 -- the composed loop is
    bound by the host's enqueueing (about 275 us per period whatever B), the fused one by its two sequential chains
    (forward 630 - 930 us, backward kernel 460 - 500 us); the replay is 9 % to 20 % of the fused step.

    ``info`` (:class:`LoopDiffInfo`): ``status`` [B, P], ``failed``, ``vjp_status`` after a backward, ``replay_error``."""
    global _FUNCTION
    torch = _torch()
    from .closed_loop import ModelClosedLoop

    P = int(nb_periods)
    if P < 1:
        raise ValueError("nb_periods must be at least 1")
    info = LoopDiffInfo()
    if not fused:
        X, U0 = _by_hand(model, x0, P, goal, targets, plant, disturbance, feas_tol, max_iter, info)
        return X, U0, info
    check_envelope(model)
    Ap, Bp = (None, None) if plant is None else plant
    passed = (x0, goal, targets, disturbance, Ap, Bp)
    loop = ModelClosedLoop(model, _detached(x0), goal=_detached(goal), targets=_detached(targets),
                           plant=None if plant is None else (_detached(Ap), _detached(Bp)),
                           disturbance=_detached(disturbance), warm=warm, feas_tol=feas_tol, max_iter=max_iter)
    loop._check_periods(P)
    info.loop, info.failed = loop, loop._loopstats[:, 0].sum()
    tens = [v if isinstance(v, torch.Tensor) else None for v in passed]
    dual = any(_is_dual(v) for v in tens)
    if not dual and not (torch.is_grad_enabled() and any(v is not None and v.requires_grad for v in tens)):
        loop.step(P)
        info.failed = loop.failed
        return loop.X, loop.U0, info
    if _FUNCTION is None:
        _FUNCTION = _make_function()
    X, U0 = _FUNCTION.apply(model, loop, P, info, *tens)
    info.failed = loop.failed
    return X, U0, info


def _jvp_by_hand(model, x0, P, goal, targets, plant, disturbance, tangents, feas_tol, max_iter, info):
    """The loop and its tangents composed in torch: ``SharedModel.solve`` and ``SharedModel.plan_jvp`` per period, then the
    plant step of both."""
    torch = _torch()
    t = model.template
    as_t = lambda v: None if v is None else torch.as_tensor(v, dtype=t.dtype, device=t.device)  # noqa: E731
    x, goal, targets, dist = as_t(_detached(x0)), as_t(_detached(goal)), as_t(_detached(targets)), as_t(_detached(disturbance))
    Ap, Bp = (t.A[0, 0], t.B[0, 0]) if plant is None else (as_t(_detached(plant[0])), as_t(_detached(plant[1])))
    for ref, what in ((goal, "goal"), (targets, "targets"), (dist, "disturbance")):
        if ref is not None and ref.ndim == 3 and ref.shape[1] < P:
            raise ValueError(f"{what} is laid out for {ref.shape[1]} periods; {P} were asked for")
    B = x.shape[0]
    (d_x0, d_goal, d_targets, d_dist, d_Ap, d_Bp), T = _loop_tangents(tangents, B, P, t.state_dim, t.input_dim,
                                                                       t.nb_timesteps, t.device)
    at = lambda r, k: None if r is None else (r[:, k] if r.ndim == 3 else r)  # noqa: E731
    tat = lambda r, k: None if r is None else (r[:, :, k] if r.ndim == 4 else r)  # noqa: E731
    zero = torch.zeros((), dtype=t.dtype, device=t.device)
    zero64 = torch.zeros((), dtype=torch.float64, device=t.device)
    step = lambda M, v: torch.matmul(v, M.transpose(-1, -2))  # noqa: E731  ([B, T, w] by a shared or a per-loop matrix)
    dx = torch.zeros((B, T, t.state_dim), dtype=torch.float64, device=t.device) if d_x0 is None else d_x0.expand(B, -1, -1)
    X, U0, dX, dU0, plans = [x], [], [dx], [], []
    for k in range(P):
        plan = model.solve(x, at(goal, k), at(targets, k), return_multipliers=True, feas_tol=feas_tol, max_iter=max_iter)
        dU, _ = model.plan_jvp(plan, initial_state=dx.contiguous(), goal_state=tat(d_goal, k),
                               target_states=tat(d_targets, k))
        ok = (plan.status == 0)[:, None]
        u0 = torch.where(ok, plan.U.view(B, t.nb_timesteps, t.input_dim)[:, 0, :], zero)
        du0 = torch.where(ok[:, None], dU[:, :, 0, :].to(torch.float64), zero64)
        dxn = step(Ap.to(torch.float64), dx) + step(Bp.to(torch.float64), du0)
        if d_dist is not None:
            dxn = dxn + tat(d_dist, k)
        if d_Ap is not None:
            dxn = dxn + torch.matmul(d_Ap, x.to(torch.float64)[:, None, :, None])[..., 0]
        if d_Bp is not None:
            dxn = dxn + torch.matmul(d_Bp, u0.to(torch.float64)[:, None, :, None])[..., 0]
        xa = torch.bmm(Ap, x[:, :, None])[:, :, 0] if Ap.ndim == 3 else x @ Ap.T
        xb = torch.bmm(Bp, u0[:, :, None])[:, :, 0] if Bp.ndim == 3 else u0 @ Bp.T
        x = xa + xb if dist is None else xa + xb + at(dist, k)
        dx = dxn
        X.append(x)
        U0.append(u0)
        dX.append(dx)
        dU0.append(du0)
        plans.append(plan)
    info._plans = plans
    info.status = torch.stack([p.status for p in plans], dim=1)
    info.failed = (info.status != 0).sum()
    info.jvp_status = torch.stack([p.jvp_status != p.status for p in plans], 1).sum(1).to(torch.int32)
    return torch.stack(X, dim=1), torch.stack(U0, dim=1), torch.stack(dX, dim=2), torch.stack(dU0, dim=2)


def closed_loop_jvp(model, x0, nb_periods, goal=None, targets=None, plant=None, disturbance=None, *, d_x0=None, d_goal=None,
                    d_targets=None, d_disturbance=None, d_Ap=None, d_Bp=None, warm: bool = False, feas_tol: float = 1e-9,
                    max_iter=None, fused: bool = True):
    """Run ``B`` closed loops of a :class:`SharedModel` for ``nb_periods`` periods, as :func:`closed_loop_diff` does, and push
    ``T`` tangents through them: ``(X [B, P+1, nx], U0 [B, P, nu], dX [B, T, P+1, nx], dU0 [B, T, P, nu], info)`` --
    how the whole trajectory moves with ``x0``, the references, the disturbance and the plant. ``dX`` and ``dU0`` are float64.

    A tangent has its operand's shape with a ``T`` axis behind the batch axis: ``d_x0`` ``[B|1, T, nx]``; ``d_goal``,
    ``d_targets`` and ``d_disturbance`` ``[B|1, T, w]`` (constant in time) or ``[B|1, T, P, w]``; ``d_Ap`` ``[B|1, T, nx, nx]``
    and ``d_Bp`` ``[B|1, T, nx, nu]``. A leading 1 shares one set with the batch; None is zero; ``T <= 256`` and every tangent
    given agrees on it. The recursion is that of ``mpcqp_model_periods_jvp_batch`` (include/mpcqp.h): a period with a plan
    contributes the KKT tangent of the plan on its active set ``{i : lam_i > 0}`` with the model's own bounds fixed, a
    period without one passes the tangent through the plant only. The model matrices, the weights and the model's ``e`` are
    not perturbed here (they change the factorisation).

    ``fused=True``: the forward launch with records, the replay of :func:`closed_loop_diff` (``info.replay_error``) and ONE
    ``mpcqp_model_periods_jvp_batch`` launch for all periods and tangents, which factors every period's active rows once.
    Envelope: ``check_envelope`` -- ``BackendError`` outside it, before anything is launched. ``info.jvp_status`` counts, per
    loop, the periods with a plan whose active rows failed (they contribute their plant term only).

    ``fused=False``: the loop composed in torch from ``SharedModel.solve`` and ``SharedModel.plan_jvp`` per period plus the
    plant step; it serves whatever ``plan_jvp`` serves and is the baseline the fused path is measured against
    (profiles/loop_jvp.md). ``warm`` is ignored there."""
    P = int(nb_periods)
    if P < 1:
        raise ValueError("nb_periods must be at least 1")
    info = LoopDiffInfo()
    tangents = (d_x0, d_goal, d_targets, d_disturbance, d_Ap, d_Bp)
    if not fused:
        X, U0, dX, dU0 = _jvp_by_hand(model, x0, P, goal, targets, plant, disturbance, tangents, feas_tol, max_iter, info)
        return X, U0, dX, dU0, info
    from .closed_loop import ModelClosedLoop

    check_envelope(model)
    loop = ModelClosedLoop(model, _detached(x0), goal=_detached(goal), targets=_detached(targets),
                           plant=None if plant is None else (_detached(plant[0]), _detached(plant[1])),
                           disturbance=_detached(disturbance), warm=warm, feas_tol=feas_tol, max_iter=max_iter)
    loop._check_periods(P)
    tans = _loop_tangents(tangents, loop.batch, P, loop.nx, loop.nu, loop.N, loop._dev)
    loop.step(P)
    X, U0 = loop.X, loop.U0
    lam, status, info.replay_error, _ = _replay(model, loop, X, U0, P)
    dX, dU0, info.jvp_status = loop_jvp(model, loop, lam, status, X, U0, tans)
    info.loop, info.status, info.failed = loop, status, loop.failed
    return X, U0, dX, dU0, info


JACOBIAN_WRT = ("x0", "goal")


def closed_loop_jacobian(model, x0, nb_periods, goal=None, targets=None, plant=None, disturbance=None, *, wrt: str = "x0",
                         warm: bool = False, feas_tol: float = 1e-9, max_iter=None, fused: bool = True):
    """``(J_X [B, P+1, nx, nx], J_U0 [B, P, nu, nx], info)``: the Jacobians of the states and of the applied inputs of every
    loop with respect to its initial state (``wrt="x0"``) or to a goal that is constant over the periods (``wrt="goal"``) --
    :func:`closed_loop_jvp` with one identity shared by the batch, ``T = nx``, one pass of the tangent kernel.
    ``J_X[:, P]`` with ``wrt="x0"`` is the linearised return map of the loop."""
    torch = _torch()
    if wrt not in JACOBIAN_WRT:
        raise ProblemDefinitionError(f"wrt: expected one of {JACOBIAN_WRT}, got {wrt!r}")
    t = model.template
    eye = torch.eye(t.state_dim, dtype=torch.float64, device=t.device)[None]
    _, _, dX, dU0, info = closed_loop_jvp(model, x0, nb_periods, goal, targets, plant, disturbance, warm=warm,
                                          feas_tol=feas_tol, max_iter=max_iter, fused=fused,
                                          **{"d_x0" if wrt == "x0" else "d_goal": eye})
    return dX.permute(0, 2, 3, 1), dU0.permute(0, 2, 3, 1), info
