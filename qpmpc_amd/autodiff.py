"""Gradients through batched MPC plans: ``solve_mpc_batch_diff``.

The forward is ``solve_mpc_batch`` with multipliers; the backward is one call of ``mpcqp_plan_vjp_batch``
(include/mpcqp.h): the condensing of the batch into scratch, then one KKT adjoint solve per problem in HIP
(qpmpc_amd/csrc/mpcqp_adjoint.hip). Gradients reach the initial state, the goal, the stage targets and the inequality
vector ``e``; when one of the model matrices A, B, C, D or the cost weights passed requires grad, the backward is
``mpcqp_plan_vjp_model_batch`` instead, the same adjoint followed by its costate pass. With
``adjoint="stagewise"`` the backward is ``mpcqp_plan_vjp_stagewise_batch`` (qpmpc_amd/csrc/mpcqp_adjoint_stagewise.hip):
the same adjoint on each problem's Riccati recursion, at any horizon ("Stage-wise adjoint").

Forward mode: ``plan_jvp`` pushes tangents of the initial state, the goal, the targets and ``e`` through a solved plan
with one call of ``mpcqp_plan_jvp_batch`` (the same KKT system on the same active set, the tangents as right-hand sides:
``mpcqp_tangent_kernel`` in mpcqp_adjoint.hip); ``plan_jacobian`` is its feedback Jacobian ``dU/dx0`` (or ``dU/dgoal``),
and ``solve_mpc_batch_diff`` serves ``torch.autograd.forward_ad`` dual tensors through it ("Forward
sensitivities"). ``plan_jvp`` also takes tangents of the model matrices A, B, C, D and of the three cost weights
(``mpcqp_plan_jvp_model_batch`` / ``mpcqp_plan_jvp_model_stagewise_batch``; DESIGN.md section 9, "Model and weight
tangents"), and ``plan_jacobian(wrt="cost_weights")`` is the plan's derivative with respect to the weights.

The reference has no counterpart: its plans are NumPy arrays.
"""
from __future__ import annotations

import ctypes as C

from . import _capi
from .batch import BatchMPCProblem, _canon, _as_tensor, _stream_ptr, solve_mpc_batch
from .exceptions import BackendError, ProblemDefinitionError

MAX_VARIABLES = 128  # envelope of mpcqp_plan_vjp_batch: n = N * nu <= 128 (and what mpcqp_condense_batch condenses)
STAGEWISE_MAX_NX, STAGEWISE_MAX_NU = 32, 8  # envelope of mpcqp_plan_vjp_stagewise_batch (any N)
# the stage-wise backward splits its batch so that one launch's workspace stays below this many bytes
STAGEWISE_WORKSPACE_CAP = 2 << 30
ADJOINTS = ("condensed", "stagewise")
FORMULATIONS = ("condensed", "stagewise")  # of the tangent solve: plan_jvp, plan_jacobian, solve_mpc_batch_diff(tangent=)
MAX_TANGENTS = 256  # tangents per problem of one mpcqp_plan_jvp_batch / mpcqp_plan_jvp_stagewise_batch call


def _torch():
    import torch

    return torch


def _detached(x):
    torch = _torch()
    return x.detach() if isinstance(x, torch.Tensor) else x


MODEL_OPERANDS = ("transition_state_matrix", "transition_input_matrix", "ineq_state_matrix", "ineq_input_matrix")
WEIGHTS = ("terminal_cost_weight", "stage_state_cost_weight", "stage_input_cost_weight")  # the order of g_w


def _weight(value, name: str) -> float:
    torch = _torch()
    if isinstance(value, torch.Tensor):
        if value.dim() != 0:
            raise ProblemDefinitionError(f"{name}: expected a float or a 0-dim tensor, got shape {tuple(value.shape)}")
        return float(value.detach().item())
    return float(value)


def _replaced(problem: BatchMPCProblem, x0, goal, targets, e, A=None, B=None, C=None, D=None,
              wt=None, wx=None, wu=None) -> BatchMPCProblem:
    """A shallow copy of ``problem`` whose operands are replaced by the (detached) tensors or values passed, validated and
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
    nx, nu, mk = work.state_dim, work.input_dim, work.ineq_dim
    for attr, name, value, tail in (("A", MODEL_OPERANDS[0], A, (nx, nx)), ("B", MODEL_OPERANDS[1], B, (nx, nu)),
                                    ("C", MODEL_OPERANDS[2], C, (mk, nx)), ("D", MODEL_OPERANDS[3], D, (mk, nu))):
        if value is None:
            continue
        t = _canon(_as_tensor(_detached(value), work.dtype, work.device), tail, name)
        if t.shape[1] not in (1, work.nb_timesteps) or t.shape[0] not in (1, work.batch_size):
            raise ProblemDefinitionError(f"{name}: shape {tuple(t.shape)} is not [B|1, N|1, {tail[0]}, {tail[1]}]")
        setattr(work, attr, t)
    if wt is not None:
        work.terminal_cost_weight = _weight(wt, WEIGHTS[0])
    if wx is not None:
        work.stage_state_cost_weight = _weight(wx, WEIGHTS[1])
    if wu is not None:
        work.stage_input_cost_weight = _weight(wu, WEIGHTS[2])
        if work.stage_input_cost_weight <= 0.0:
            raise ProblemDefinitionError("stage non-negative control weight needed for regularization")
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


def check_envelope(problem: BatchMPCProblem, kind: str = "vjp") -> None:
    """Raise ``BackendError`` unless the export of ``kind`` serves this problem's dimensions (nothing is launched; the
    ``_model`` tangent exports have the envelopes of ``"jvp"`` and ``"jvp_stagewise"``):
    ``"vjp"``, ``mpcqp_plan_vjp_batch`` (n = N * nu <= 128); ``"jvp"``, ``mpcqp_plan_jvp_batch`` (the same);
    ``"stagewise"``, ``mpcqp_plan_vjp_stagewise_batch`` (nx <= 32, nu <= 8, any horizon); ``"jvp_stagewise"``,
    ``mpcqp_plan_jvp_stagewise_batch`` (the same)."""
    lib = _capi.load()
    n, nx, nu = problem.nb_variables, problem.state_dim, problem.input_dim
    if kind == "stagewise":
        if nx > STAGEWISE_MAX_NX or nu > STAGEWISE_MAX_NU:
            raise BackendError(f"the stage-wise adjoint serves nx <= {STAGEWISE_MAX_NX}, nu <= {STAGEWISE_MAX_NU}, "
                               f"not nx = {nx}, nu = {nu}")
        query, extra = lib.mpcqp_plan_vjp_stagewise_workspace_bytes, (0,)
    elif kind == "jvp_stagewise":
        if nx > STAGEWISE_MAX_NX or nu > STAGEWISE_MAX_NU:
            raise BackendError(f"the stage-wise tangent solve serves nx <= {STAGEWISE_MAX_NX}, nu <= {STAGEWISE_MAX_NU}, "
                               f"not nx = {nx}, nu = {nu}")
        query, extra = lib.mpcqp_plan_jvp_stagewise_workspace_bytes, (0, 1)
    elif kind == "jvp":
        if n > MAX_VARIABLES:
            raise BackendError(f"forward sensitivities of plans are served for n = N * nu <= {MAX_VARIABLES} variables, "
                               f"not {n}, by the condensed tangent solve (formulation=\"stagewise\" serves any horizon for "
                               f"nx <= {STAGEWISE_MAX_NX}, nu <= {STAGEWISE_MAX_NU})")
        query, extra = lib.mpcqp_plan_jvp_workspace_bytes, (1,)
    else:
        if n > MAX_VARIABLES:
            raise BackendError(f"gradients through plans are served for n = N * nu <= {MAX_VARIABLES} variables, not {n}, "
                               "by the condensed adjoint (adjoint=\"stagewise\" serves any horizon for nx <= 32, nu <= 8)")
        query, extra = lib.mpcqp_plan_vjp_workspace_bytes, ()
    _workspace_bytes(query, _vjp_dims(problem), problem.batch_size, *extra)


def check_envelope_stagewise(problem: BatchMPCProblem) -> None:
    """``check_envelope(problem, "stagewise")``."""
    check_envelope(problem, "stagewise")


def _reduce(g, like, canon_shape):
    """Sum the per-problem (per-step) gradient ``g`` over the dimensions the user's operand broadcast (size 1 in its
    canonical shape), then give it the user's shape, dtype and device (``like``)."""
    dims = [d for d, s in enumerate(canon_shape) if s == 1 and g.shape[d] != 1]
    if dims:
        g = g.sum(dim=dims, keepdim=True)
    shape, dtype, device = like
    return g.reshape(shape).to(dtype=dtype, device=device)


def _workspace_bytes(query, dims, Bn, *extra) -> int:
    """The byte count a ``*_workspace_bytes`` export reports for ``Bn`` problems (``extra``: its max_active or ntan)."""
    nbytes = C.c_size_t(0)
    _capi.check(query(C.byref(dims), Bn, *extra, C.byref(nbytes)), query.__name__)
    return nbytes.value


def _workspace_for(query, dims, Bn, device, *extra):
    torch = _torch()
    return torch.empty((max(_workspace_bytes(query, dims, Bn, *extra), 1),), dtype=torch.uint8, device=device)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _max_active(lam, status, n: int) -> int:
    """The largest number of active rows (lam > 0) of a solved problem, capped at n: one host sync."""
    if lam is None or lam.shape[0] == 0:
        return 0
    act = ((lam > 0) & (status == 0)[:, None]).sum(dim=1)
    return min(int(act.max().item()), n)


def _stagewise_chunks(query, dims, Bn, device, *extra):
    """``(workspace, [(b0, nb), ...])``: the batch split into launches whose workspace (``query`` with ``extra``) stays
    below ``STAGEWISE_WORKSPACE_CAP``, and one workspace for the largest of them."""
    chunk = max(1, min(Bn, STAGEWISE_WORKSPACE_CAP // max(_workspace_bytes(query, dims, 1, *extra), 1)))
    ws = _workspace_for(query, dims, chunk, device, *extra)
    return ws, [(b0, min(chunk, Bn - b0)) for b0 in range(0, Bn, chunk)]


def _at(t, b0: int):
    """The address of problem ``b0``'s part of a per-problem tensor (None stays None)."""
    return None if t is None else t[b0:].data_ptr()


GRAD_KEYS = ("x0", "goal", "targets", "e", "A", "B", "C", "D", "wt", "wx", "wu")
BACKWARDS = ("condensed", "model", "stagewise")


def _shifted(cp, b0: int):
    """A copy of the C problem ``cp`` whose per-problem operands start at problem ``b0`` (float64 elements)."""
    out = _capi.Problem()
    for name, _ in _capi.Problem._fields_:
        op = getattr(cp, name)
        ptr = None if not op.ptr else op.ptr + 8 * b0 * op.batch_stride
        setattr(out, name, _capi.Operand(ptr, op.batch_stride, op.step_stride))
    return out


def _vjp(work: BatchMPCProblem, plan, gU, gX, want, backward: str):
    """The gradients of ``GRAD_KEYS`` in float64, per problem: x0 [B,nx], goal [B,nx], targets [B,N*nx], e [B,N,mk],
    A [B,N,nx,nx], B [B,N,nx,nu], C [B,N,mk,nx], D [B,N,mk,nu] and the three weights [B]; entries not in ``want`` are
    None. Sets ``plan.vjp_status``.

    ``backward`` names the export: ``"condensed"``, mpcqp_plan_vjp_batch (x0, always returned, goal, targets and e; the
    rest None); ``"model"``, mpcqp_plan_vjp_model_batch; ``"stagewise"``, mpcqp_plan_vjp_stagewise_batch, whose
    ``max_active`` is the largest number of active rows (lam > 0) of a solved problem, capped at n: the one host sync of
    the backward. Its batch is split into launches whose workspace stays below ``STAGEWISE_WORKSPACE_CAP``."""
    torch = _torch()
    lib = _capi.load()
    if backward not in BACKWARDS:
        raise ValueError(f"backward: expected one of {BACKWARDS}, got {backward!r}")
    p64 = _as_float64(work)
    Bn, N, nx, nu, mk, n = (work.batch_size, work.nb_timesteps, work.state_dim, work.input_dim, work.ineq_dim,
                            work.nb_variables)
    dev = work.device
    f64 = dict(dtype=torch.float64, device=dev)
    gU = torch.zeros((Bn, n), **f64) if gU is None else gU.reshape(Bn, n).to(torch.float64).contiguous()
    gX = None if gX is None else gX.reshape(Bn, (N + 1) * nx).to(torch.float64).contiguous()
    lam = plan.multipliers.to(torch.float64).contiguous() if mk > 0 else None
    if backward == "condensed":
        want = {"x0"} | (set(want) & {"goal", "targets", "e"})
    shapes = dict(x0=(nx,), goal=(nx,), targets=(N * nx,), e=(N, mk), A=(N, nx, nx), B=(N, nx, nu), C=(N, mk, nx),
                  D=(N, mk, nu))
    out = {k: (torch.empty((Bn,) + shp, **f64) if k in want else None) for k, shp in shapes.items()}
    g_w = torch.empty((Bn, 3), **f64) if want & {"wt", "wx", "wu"} else None
    model = g_w is not None or any(out[k] is not None for k in ("A", "B", "C", "D"))
    U = plan.U.reshape(Bn, -1).to(torch.float64).contiguous() if backward == "model" or model else None
    status, vjp_status = plan.status, torch.empty((Bn,), dtype=torch.int32, device=dev)
    dims, cp = _vjp_dims(p64), p64.c_problem()
    keep = [cp]
    if backward == "condensed":
        ws = _workspace_for(lib.mpcqp_plan_vjp_workspace_bytes, dims, Bn, dev)
        rc = lib.mpcqp_plan_vjp_batch(
            C.byref(dims), C.byref(cp), Bn, _ptr(lam), status.data_ptr(), gU.data_ptr(), _ptr(gX),
            *[_ptr(out[k]) for k in GRAD_KEYS[:4]], vjp_status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        _capi.check(rc, "mpcqp_plan_vjp_batch")
    elif backward == "model":
        ws = _workspace_for(lib.mpcqp_plan_vjp_model_workspace_bytes, dims, Bn, dev)
        res = _capi.VjpModelOut(*[_ptr(out[k]) for k in GRAD_KEYS[:8]], _ptr(g_w))
        rc = lib.mpcqp_plan_vjp_model_batch(
            C.byref(dims), C.byref(cp), Bn, _ptr(lam), status.data_ptr(), U.data_ptr(), gU.data_ptr(), _ptr(gX),
            C.byref(res), vjp_status.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr())
        _capi.check(rc, "mpcqp_plan_vjp_model_batch")
    else:
        max_active = _max_active(lam, status, n)  # the host sync
        ws, chunks = _stagewise_chunks(lib.mpcqp_plan_vjp_stagewise_workspace_bytes, dims, Bn, dev, max_active)
        at = _at
        for b0, nb in chunks:
            cpb = _shifted(cp, b0)
            res = _capi.VjpModelOut(*[at(out[k], b0) for k in GRAD_KEYS[:8]], at(g_w, b0))
            rc = lib.mpcqp_plan_vjp_stagewise_batch(
                C.byref(dims), C.byref(cpb), nb, max_active, at(lam, b0), at(status, b0), at(U, b0), at(gU, b0),
                at(gX, b0), C.byref(res), at(vjp_status, b0), ws.data_ptr(), ws.numel(), _stream_ptr())
            _capi.check(rc, "mpcqp_plan_vjp_stagewise_batch")
            keep.append(cpb)
    plan.vjp_status = vjp_status
    plan._vjp_keep = (ws, p64, lam, U, gU, gX, keep)  # alive until the stream has consumed them
    for i, k in enumerate(("wt", "wx", "wu")):
        out[k] = g_w[:, i] if k in want else None
    return tuple(out[k] for k in GRAD_KEYS)


def _plan_vjp(work: BatchMPCProblem, plan, gU, gX, want, backward: str = "condensed"):
    """``_vjp`` through the export ``backward`` names (mpcqp_plan_vjp_batch by default)."""
    return _vjp(work, plan, gU, gX, want, backward)


def _plan_vjp_model(work: BatchMPCProblem, plan, gU, gX, want):
    """``_vjp`` through mpcqp_plan_vjp_model_batch."""
    return _vjp(work, plan, gU, gX, want, "model")


def _plan_vjp_stagewise(work: BatchMPCProblem, plan, gU, gX, want):
    """``_vjp`` through mpcqp_plan_vjp_stagewise_batch."""
    return _vjp(work, plan, gU, gX, want, "stagewise")


TANGENT_NAMES = ("initial_state", "goal_state", "target_states", "ineq_vector")


def _tangent_operand(t, name, Bn, tail, device):
    """A tangent ``[B|1, T, *tail]`` as contiguous float64 and its stride between problems (0 when shared), or
    (None, 0)."""
    torch = _torch()
    if t is None:
        return None, 0
    t = torch.as_tensor(t, device=device)
    if t.dim() != 2 + len(tail) or tuple(t.shape[2:]) != tuple(tail) or t.shape[0] not in (1, Bn) or t.shape[1] < 1:
        want = ", ".join(str(d) for d in tail)
        raise ProblemDefinitionError(f"{name}: tangent of shape {tuple(t.shape)} is not [{Bn}|1, T, {want}]")
    t = t.to(device=device, dtype=torch.float64).contiguous()
    return t, (0 if t.shape[0] == 1 else t[0].numel())


def _model_tangent_operand(t, name, Bn, N, tail, device):
    """A model tangent ``[B|1, T, N|1, *tail]`` as contiguous float64 ``[B|1, T, N, *tail]`` (a step dimension of 1 is
    expanded: a time-invariant perturbation) and its stride between problems (0 when shared), or (None, 0)."""
    torch = _torch()
    if t is None:
        return None, 0
    t = torch.as_tensor(t, device=device)
    if (t.dim() != 3 + len(tail) or tuple(t.shape[3:]) != tuple(tail) or t.shape[0] not in (1, Bn) or t.shape[1] < 1
            or t.shape[2] not in (1, N)):
        want = ", ".join(str(d) for d in tail)
        raise ProblemDefinitionError(f"{name}: tangent of shape {tuple(t.shape)} is not [{Bn}|1, T, {N}|1, {want}]")
    t = t.to(device=device, dtype=torch.float64).expand(-1, -1, N, *([-1] * len(tail))).contiguous()
    return t, (0 if t.shape[0] == 1 else t[0].numel())


def _weight_tangents(weights, Bn, device):
    """The three weights' tangents ``[B|1, T]`` (None = zero) as one contiguous float64 ``[B|1, T, 3]`` in the order of
    g_w (terminal, stage, input) and its stride between problems, or (None, 0) when none is given."""
    torch = _torch()
    given = []
    for name, t in zip(WEIGHTS, weights):
        if t is None:
            continue
        t = torch.as_tensor(t, device=device)
        if t.dim() != 2 or t.shape[0] not in (1, Bn) or t.shape[1] < 1:
            raise ProblemDefinitionError(f"{name}: tangent of shape {tuple(t.shape)} is not [{Bn}|1, T]")
        given.append((name, t.to(device=device, dtype=torch.float64)))
    if not given:
        return None, 0
    Ts = {t.shape[1] for _, t in given}
    if len(Ts) > 1:
        raise ProblemDefinitionError(f"plan_jvp: the tangents disagree on T: {sorted(Ts)}")
    lead = max(t.shape[0] for _, t in given)
    dw = torch.zeros((lead, Ts.pop(), 3), dtype=torch.float64, device=device)
    for name, t in given:
        dw[:, :, WEIGHTS.index(name)] = t
    return dw, (0 if lead == 1 else dw[0].numel())


def _formulation(value, name: str = "formulation") -> str:
    if value not in FORMULATIONS:
        raise ValueError(f"{name}: expected one of {FORMULATIONS}, got {value!r}")
    return value


def plan_jvp(problem: BatchMPCProblem, plan, initial_state=None, goal_state=None, target_states=None,
             ineq_vector=None, states: bool = False, *, formulation: str = "condensed", transition_state_matrix=None,
             transition_input_matrix=None, ineq_state_matrix=None, ineq_input_matrix=None, terminal_cost_weight=None,
             stage_state_cost_weight=None, stage_input_cost_weight=None):
    """Jacobian-vector products of a solved plan: ``(dU [B, T, N, nu], dX [B, T, N+1, nx] or None)``.

    ``plan`` is ``solve_mpc_batch(problem, ..., return_multipliers=True)``; the active set is ``{i : lam_i > 0}`` and, on
    it, the plan's response to the T tangents passed is solved in one call of ``mpcqp_plan_jvp_batch``. Tangents (each
    optional, None = zero; at least one is needed, all with the same T <= 256): ``initial_state`` and ``goal_state``
    ``[B|1, T, nx]``, ``target_states`` ``[B|1, T, N*nx]``, ``ineq_vector`` ``[B|1, T, N, mk]``; a leading 1 shares one set
    of tangents with every problem. A goal or targets that do not enter the cost get zero responses, as for the VJP.
    ``dX`` (with ``states=True``) is the rollout's tangent ``Phi dx0 + Psi dU``. Computed in float64 (a float32
    problem's operands are converted) and returned in the problem's dtype. Problems not solved get zeros, and after the
    call ``plan.jvp_status`` holds their status (``MPCQP_NOT_PD`` where the active rows' Gram matrix is singular; else
    0). Envelope: n = N * nu <= 128 (``BackendError`` before anything is launched).

    ``formulation="stagewise"`` solves the same system on each problem's Riccati recursion without condensing
    (``mpcqp_plan_jvp_stagewise_batch``: one factorisation per problem, the tangents side by side) and serves every
    horizon and every n for nx <= 32, nu <= 8 (``BackendError`` outside). Like the stage-wise backward it sizes its
    workspace from the largest number of active rows in the batch (one host sync) and splits the batch so that one
    launch's workspace stays below ``STAGEWISE_WORKSPACE_CAP``; ``plan.jvp_status`` may then also hold
    ``MPCQP_NOT_PD`` for a stage Hessian that is not positive definite. Any other value raises ``ValueError``.

    Tangents of the model and the cost weights (keyword-only, named as ``solve_mpc_batch_diff`` names the operands, the
    same T): ``transition_state_matrix`` ``[B|1, T, N|1, nx, nx]``, ``transition_input_matrix`` ``[B|1, T, N|1, nx, nu]``,
    ``ineq_state_matrix`` ``[B|1, T, N|1, mk, nx]``, ``ineq_input_matrix`` ``[B|1, T, N|1, mk, nu]`` (a step dimension
    of 1 is a time-invariant perturbation, expanded to N) and ``terminal_cost_weight``, ``stage_state_cost_weight``,
    ``stage_input_cost_weight`` ``[B|1, T]``. The plan then moves as if the pendulum were longer or the terminal weight
    doubled: the plan and its multipliers are held on the active set, and the tangents enter the same KKT system as
    right-hand sides ("Model and weight tangents"). When one of them is given the call is
    ``mpcqp_plan_jvp_model_batch`` (``mpcqp_plan_jvp_model_stagewise_batch`` with ``formulation="stagewise"``);
    otherwise it is the export above, as before. The tangent of an ``ineq_state_matrix`` or ``ineq_input_matrix`` the
    problem does not have is the one at zero; a weight whose cost term the problem does not have contributes nothing."""
    model = (transition_state_matrix, transition_input_matrix, ineq_state_matrix, ineq_input_matrix)
    weights = (terminal_cost_weight, stage_state_cost_weight, stage_input_cost_weight)
    dU, dX = _jvp(problem, plan, initial_state, goal_state, target_states, ineq_vector, states, formulation, model,
                  weights)
    dt = problem.dtype
    return dU.to(dt), (None if dX is None else dX.to(dt))


def _jvp(problem: BatchMPCProblem, plan, initial_state, goal_state, target_states, ineq_vector, states: bool,
         formulation: str, model=(None,) * 4, weights=(None,) * 3):
    """``plan_jvp`` in float64, as the export wrote it (the caller casts to the problem's dtype). ``model``: the tangents
    of A, B, C, D; ``weights``: of the three weights."""
    torch = _torch()
    lib = _capi.load()
    stagewise = _formulation(formulation) == "stagewise"
    Bn, N, nx, nu, mk = (problem.batch_size, problem.nb_timesteps, problem.state_dim, problem.input_dim,
                         problem.ineq_dim)
    n, dev = problem.nb_variables, problem.device
    if mk > 0 and plan.multipliers is None:
        raise ProblemDefinitionError("plan_jvp needs the plan's multipliers: solve with return_multipliers=True")
    check_envelope(problem, "jvp_stagewise" if stagewise else "jvp")
    tails = ((nx,), (nx,), (N * nx,), (N, mk))
    ops = [_tangent_operand(t, nm, Bn, tail, dev) for t, nm, tail in zip(
        (initial_state, goal_state, target_states, ineq_vector), TANGENT_NAMES, tails)]
    mtails = ((nx, nx), (nx, nu), (mk, nx), (mk, nu))
    mops = [_model_tangent_operand(t, nm, Bn, N, tail, dev) for t, nm, tail in zip(model, MODEL_OPERANDS, mtails)]
    mops.append(_weight_tangents(weights, Bn, dev))
    if mk == 0:
        mops[2] = mops[3] = (None, 0)
    with_model = any(t is not None for t, _ in mops)
    Ts = {t.shape[1] for t, _ in ops + mops if t is not None}
    if not Ts:
        raise ProblemDefinitionError("plan_jvp: no tangent given")
    if len(Ts) > 1:
        raise ProblemDefinitionError(f"plan_jvp: the tangents disagree on T: {sorted(Ts)}")
    T = Ts.pop()
    if T > MAX_TANGENTS:
        raise ProblemDefinitionError(f"plan_jvp: T = {T} tangents, at most {MAX_TANGENTS} per call")
    if mk == 0:
        ops[3] = (None, 0)
    p64 = _as_float64(problem)
    f64 = dict(dtype=torch.float64, device=dev)
    lam = plan.multipliers.to(torch.float64).contiguous() if mk > 0 else None
    dU = torch.empty((Bn, T, N, nu), **f64)
    dX = torch.empty((Bn, T, N + 1, nx), **f64) if states else None
    jvp_status = torch.empty((Bn,), dtype=torch.int32, device=dev)
    dims, cp = _vjp_dims(p64), p64.c_problem()
    keep = [cp]
    if with_model:
        U = plan.U.reshape(Bn, n).to(torch.float64).contiguous()
        keep.append(U)
        if stagewise:
            max_active = _max_active(lam, plan.status, n)  # the host sync
            ws, chunks = _stagewise_chunks(lib.mpcqp_plan_jvp_model_stagewise_workspace_bytes, dims, Bn, dev,
                                           max_active, T)
            for b0, nb in chunks:
                cpb = _shifted(cp, b0)
                tan = _capi.Tangents(*[(_at(t, b0) if st else _ptr(t)) for t, st in ops], *[st for _, st in ops])
                mtan = _capi.ModelTangents(*[(_at(t, b0) if st else _ptr(t)) for t, st in mops],
                                           *[st for _, st in mops])
                rc = lib.mpcqp_plan_jvp_model_stagewise_batch(
                    C.byref(dims), C.byref(cpb), nb, max_active, T, _at(lam, b0), _at(plan.status, b0), _at(U, b0),
                    C.byref(tan), C.byref(mtan), _at(dU, b0), _at(dX, b0), _at(jvp_status, b0), ws.data_ptr(),
                    ws.numel(), _stream_ptr())
                _capi.check(rc, "mpcqp_plan_jvp_model_stagewise_batch")
                keep.append(cpb)
        else:
            ws = _workspace_for(lib.mpcqp_plan_jvp_model_workspace_bytes, dims, Bn, dev, T)
            tan = _capi.Tangents(*[_ptr(t) for t, _ in ops], *[st for _, st in ops])
            mtan = _capi.ModelTangents(*[_ptr(t) for t, _ in mops], *[st for _, st in mops])
            rc = lib.mpcqp_plan_jvp_model_batch(
                C.byref(dims), C.byref(cp), Bn, T, _ptr(lam), plan.status.data_ptr(), U.data_ptr(), C.byref(tan),
                C.byref(mtan), dU.data_ptr(), _ptr(dX), jvp_status.data_ptr(), ws.data_ptr(), ws.numel(),
                _stream_ptr())
            _capi.check(rc, "mpcqp_plan_jvp_model_batch")
    elif stagewise:
        max_active = _max_active(lam, plan.status, n)  # the host sync
        ws, chunks = _stagewise_chunks(lib.mpcqp_plan_jvp_stagewise_workspace_bytes, dims, Bn, dev, max_active, T)
        for b0, nb in chunks:
            cpb = _shifted(cp, b0)
            # (a shared tangent, stride 0, is every launch's; the others move on with the problems)
            tan = _capi.Tangents(*[(_at(t, b0) if st else _ptr(t)) for t, st in ops], *[st for _, st in ops])
            rc = lib.mpcqp_plan_jvp_stagewise_batch(
                C.byref(dims), C.byref(cpb), nb, max_active, T, _at(lam, b0), _at(plan.status, b0), C.byref(tan),
                _at(dU, b0), _at(dX, b0), _at(jvp_status, b0), ws.data_ptr(), ws.numel(), _stream_ptr())
            _capi.check(rc, "mpcqp_plan_jvp_stagewise_batch")
            keep.append(cpb)
    else:
        ws = _workspace_for(lib.mpcqp_plan_jvp_workspace_bytes, dims, Bn, dev, T)
        tan = _capi.Tangents(*[_ptr(t) for t, _ in ops], *[st for _, st in ops])
        rc = lib.mpcqp_plan_jvp_batch(C.byref(dims), C.byref(cp), Bn, T, _ptr(lam), plan.status.data_ptr(),
                                      C.byref(tan), dU.data_ptr(), _ptr(dX), jvp_status.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream_ptr())
        _capi.check(rc, "mpcqp_plan_jvp_batch")
    plan.jvp_status = jvp_status
    plan._jvp_keep = (ws, p64, lam, ops, mops, keep)  # alive until the stream has consumed them
    return dU, dX


JACOBIAN_WRT = ("initial_state", "goal_state", "cost_weights")


def plan_jacobian(problem: BatchMPCProblem, plan, wrt: str = "initial_state", states: bool = False, *,
                  formulation: str = "condensed"):
    """Feedback Jacobian of a solved plan: ``(J_U [B, N, nu, nx], J_X [B, N+1, nx, nx] or None)`` with
    ``J_U[b, k, :, j] = dU_k / d(wrt)_j`` on the plan's active set. ``wrt`` is ``"initial_state"`` (``J_U[:, 0]`` is the
    local gain: ``u ~ plan.U[:, 0] + J_U[:, 0] @ (x - x0)`` while the active set holds) or ``"goal_state"``.

    This is ``plan_jvp`` with the identity as T = nx tangents shared by the batch (stride 0), returned as a permuted
    view; its rules (multipliers, status, envelope, dtype) apply, and so does its ``formulation``: ``"stagewise"`` gives
    the Jacobian at any horizon (nx <= 32, nu <= 8) on one factorisation per problem (DESIGN.md section 9 has the
    measured cost beside one stage-wise backward).

    ``wrt="cost_weights"`` gives ``J_U [B, N, nu, 3]`` (and ``J_X [B, N+1, nx, 3]``): the plan's derivative with respect
    to the terminal, stage-state and stage-input cost weights, in this order, from one 3 x 3 identity of weight tangents
    shared by the batch (``mpcqp_plan_jvp_model_batch``; a weight whose cost term the problem does not have gets zeros)."""
    torch = _torch()
    _formulation(formulation)
    if wrt not in JACOBIAN_WRT:
        raise ProblemDefinitionError(f"wrt: expected one of {JACOBIAN_WRT}, got {wrt!r}")
    if wrt == "cost_weights":
        eye = torch.eye(3, dtype=torch.float64, device=problem.device)
        dU, dX = _jvp(problem, plan, None, None, None, None, states, formulation,
                      weights=tuple(eye[j][None] for j in range(3)))
        dU, dX = dU.to(problem.dtype), (None if dX is None else dX.to(problem.dtype))
        return dU.permute(0, 2, 3, 1), (None if dX is None else dX.permute(0, 2, 3, 1))
    eye = torch.eye(problem.state_dim, dtype=torch.float64, device=problem.device)[None]
    dU, dX = plan_jvp(problem, plan, states=states, formulation=formulation, **{wrt: eye})
    return dU.permute(0, 2, 3, 1), (None if dX is None else dX.permute(0, 2, 3, 1))


def _is_dual(t) -> bool:
    torch = _torch()
    if not isinstance(t, torch.Tensor):
        return False
    from torch.autograd import forward_ad

    return forward_ad.unpack_dual(t).tangent is not None


def _forward_tangents(ctx, tangents):
    """(dU [B, N, nu], dX [B, N+1, nx] or None) of the forward-mode pass: one plan_jvp call with T = 1."""
    work = ctx.work
    Bn, N = work.batch_size, work.nb_timesteps
    args = {}
    for nm, t, canon in zip(TANGENT_NAMES, tangents, ctx.canon):
        if t is None:
            continue
        t = t.reshape(canon)
        if nm == "ineq_vector":
            t = t.expand(-1, N, -1)
        args[nm] = t.unsqueeze(1)
    if not args:
        return None, None
    dU, dX = plan_jvp(work, ctx.plan, states=ctx.states, formulation=ctx.tangent, **args)
    return dU[:, 0], (None if dX is None else dX[:, 0])


def _make_function():
    torch = _torch()
    from torch.autograd.function import once_differentiable

    class _PlanFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, work, states, solve_kw, box, *operands):
            plan = solve_mpc_batch(work, return_multipliers=True, **solve_kw)
            U = plan.U.view(work.batch_size, work.nb_timesteps, work.input_dim)
            box["plan"] = plan
            ctx.work, ctx.plan, ctx.states, ctx.adjoint = work, plan, states, box["adjoint"]
            ctx.tangent = box["tangent"]
            ctx.inputs = tuple(None if t is None else (t.shape, t.dtype, t.device) for t in operands)
            canon = (work.initial_state, work.goal_state, work.target_states, work.e, work.A, work.B, work.C, work.D)
            # a weight is one value for the batch: shape (1,) sums its per-problem gradients
            ctx.canon = (tuple(None if t is None else c.shape for t, c in zip(operands, canon))
                         + tuple(None if t is None else (1,) for t in operands[8:]))
            return (U, plan.states) if states else U

        @staticmethod
        @once_differentiable
        def backward(ctx, gU, gX=None):
            need = ctx.needs_input_grad[4:]
            want = {nm for nm, nd in zip(GRAD_KEYS, need) if nd}
            if ctx.adjoint == "stagewise":
                grads = _plan_vjp_stagewise(ctx.work, ctx.plan, gU, gX, want)
            elif any(need[4:]):
                grads = _plan_vjp_model(ctx.work, ctx.plan, gU, gX, want)
            else:
                grads = _plan_vjp(ctx.work, ctx.plan, gU, gX, want)
            out = [_reduce(g, like, canon) if nd else None
                   for nd, g, like, canon in zip(need, grads, ctx.inputs, ctx.canon)]
            return (None, None, None, None, *out)

        @staticmethod
        def jvp(ctx, *tangents):
            tangents = tangents[4:]
            if any(t is not None for t in tangents[4:]):  # (refused before the forward; kept as a guard)
                raise BackendError("forward-mode tangents reach initial_state, goal_state, target_states and "
                                   "ineq_vector only")
            dU, dX = _forward_tangents(ctx, tangents[:4])
            if dU is None:
                dU = torch.zeros((ctx.work.batch_size, ctx.work.nb_timesteps, ctx.work.input_dim),
                                 dtype=ctx.work.dtype, device=ctx.work.device)
            if ctx.states and dX is None:
                dX = torch.zeros((ctx.work.batch_size, ctx.work.nb_timesteps + 1, ctx.work.state_dim),
                                 dtype=ctx.work.dtype, device=ctx.work.device)
            return (dU, dX) if ctx.states else dU

    return _PlanFunction


_FUNCTION = None


def solve_mpc_batch_diff(problem: BatchMPCProblem, initial_state=None, goal_state=None, target_states=None,
                         ineq_vector=None, states: bool = False, *, transition_state_matrix=None,
                         transition_input_matrix=None, ineq_state_matrix=None, ineq_input_matrix=None,
                         terminal_cost_weight=None, stage_state_cost_weight=None, stage_input_cost_weight=None,
                         adjoint: str = "condensed", tangent: str = "condensed", **solve_kw):
    """Solve a batch like ``solve_mpc_batch`` and return ``(U, X, plan)`` whose ``U`` [B, N, nu] and, with ``states=True``,
    ``X`` [B, N+1, nx] carry a ``grad_fn`` (``X`` is None otherwise).

    ``initial_state``, ``goal_state``, ``target_states`` and ``ineq_vector`` replace the problem's own values when given
    and take the shapes ``BatchMPCProblem`` accepts (``[B, nx]``; ``[B|1, nx]`` or ``[nx]``; ``[B|1, N*nx]``;
    ``[B|1, N|1, mk]``, ``[N|1, mk]`` or ``[mk]``). So do the keyword-only ``transition_state_matrix``,
    ``transition_input_matrix``, ``ineq_state_matrix`` and ``ineq_input_matrix`` (``[B|1, N|1, r, c]``, ``[N|1, r, c]``
    or ``[r, c]``) and the cost weights ``terminal_cost_weight``, ``stage_state_cost_weight`` and
    ``stage_input_cost_weight`` (a float or a 0-dim tensor; the forward reads its value, and which cost terms exist follows
    from the weights and states as in ``BatchMPCProblem``). The others are constants taken from ``problem``. A gradient
    reaching an operand shared by the batch (or by the steps), or a weight, is the sum of the per-problem (per-step)
    gradients. The gradient with respect to ``ineq_state_matrix`` or ``ineq_input_matrix`` passed where the problem has
    none is the one at zero.

    The forward is ``solve_mpc_batch(..., return_multipliers=True, **solve_kw)`` on detached copies (every dispatch path
    of it returns multipliers, with exact zeros on inactive rows), then the rollout for ``X``. The backward is one
    ``mpcqp_plan_vjp_batch`` call, or ``mpcqp_plan_vjp_model_batch`` when one of the model matrices or weights passed
    requires grad (float64: a float32 problem's operands are converted, its gradients cast back). The active set is
    ``{i : lam_i > 0}``: at weakly active points (a tight row with a zero multiplier) the gradient is one element of the
    generalized Jacobian, as in OptNet. Problems that were not solved (``plan.status != 0``) get zero gradients; after the
    backward ``plan.vjp_status`` holds their status (and ``MPCQP_NOT_PD`` where the active rows' Gram matrix is singular).
    Envelope: n = N * nu <= 128; beyond it a request for gradients raises ``BackendError`` before anything is launched.
    Only first derivatives (``once_differentiable``).

    ``adjoint`` picks the backward: ``"condensed"`` (the default, as above) or ``"stagewise"``, which solves the same
    adjoint on each problem's Riccati recursion without condensing (``mpcqp_plan_vjp_stagewise_batch``) and serves every
    horizon and every n for nx <= 32, nu <= 8 (``BackendError`` outside, before anything is launched). Its backward sizes
    the workspace from the largest number of active rows in the batch, which costs one host sync. Any other value raises
    ``ProblemDefinitionError``.

    Forward mode: ``initial_state``, ``goal_state``, ``target_states`` and ``ineq_vector`` may be dual tensors of
    ``torch.autograd.forward_ad``; the tangents of ``U`` (and ``X``) are then one ``plan_jvp`` call (T = 1) on the plan.
    A dual model matrix or weight, ``adjoint="stagewise"`` with a dual operand, or n > 128 raises ``BackendError``
    before anything is launched. With ``tangent="stagewise"`` that call is the stage-wise one
    (``plan_jvp(..., formulation="stagewise")``): dual operands are then served at any horizon for nx <= 32, nu <= 8,
    whatever ``adjoint`` is (a dual model matrix or weight is still refused). Any other value of ``tangent`` raises
    ``ValueError``.

    When no operand passed requires grad (or grad mode is off) and none is dual, this is ``solve_mpc_batch(problem', **solve_kw)`` on the
    problem with the replaced operands, and its plan is returned as is."""
    global _FUNCTION
    torch = _torch()
    if adjoint not in ADJOINTS:
        raise ProblemDefinitionError(f"adjoint: expected one of {ADJOINTS}, got {adjoint!r}")
    passed = (initial_state, goal_state, target_states, ineq_vector, transition_state_matrix, transition_input_matrix,
              ineq_state_matrix, ineq_input_matrix, terminal_cost_weight, stage_state_cost_weight,
              stage_input_cost_weight)
    _formulation(tangent, "tangent")
    dual = [_is_dual(t) for t in passed]
    if any(dual[4:]):
        names = MODEL_OPERANDS + WEIGHTS
        raise BackendError("forward-mode tangents through plans reach initial_state, goal_state, target_states and "
                           f"ineq_vector; a dual {', '.join(nm for nm, d in zip(names, dual[4:]) if d)} is not served")
    if any(dual) and adjoint == "stagewise" and tangent != "stagewise":
        raise BackendError("forward-mode tangents through plans are served by the condensed tangent solve unless "
                           "tangent=\"stagewise\" is passed; adjoint=\"stagewise\" picks the backward only")
    work = _replaced(problem, *passed)
    need = any(dual) or (torch.is_grad_enabled()
                         and any(isinstance(t, torch.Tensor) and t.requires_grad for t in passed))
    if not need:
        plan = solve_mpc_batch(work, **solve_kw)
        U = plan.U.view(work.batch_size, work.nb_timesteps, work.input_dim)
        return U, (plan.states if states else None), plan
    stage_tan = any(dual) and tangent == "stagewise"
    if stage_tan:
        check_envelope(work, "jvp_stagewise")
    # the backward's envelope; with a stage-wise tangent only where an operand asks for a backward too
    if not stage_tan or (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in passed)):
        check_envelope(work, "stagewise" if adjoint == "stagewise" else "vjp")
    if any(dual) and not stage_tan:
        check_envelope(work, "jvp")
    if _FUNCTION is None:
        _FUNCTION = _make_function()
    box = {"adjoint": adjoint, "tangent": tangent}
    tens = [t if isinstance(t, torch.Tensor) else None for t in passed]
    out = _FUNCTION.apply(work, bool(states), dict(solve_kw), box, *tens)
    U, X = out if states else (out, None)
    return U, X, box["plan"]
