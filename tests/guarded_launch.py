"""The guarded-launch harness of the contract suites (memory discipline, operand layouts, padded rows, unit changes, verdicts,
degenerate active sets, streams, the on-chip 17 .. 32-variable kernel): the exports of include/mpcqp.h called through ctypes with
every operand, output, workspace, warm-state and model buffer of the call carved from one guarded arena (tests/arena.py): exact
sizes, 512-byte aligned, 64 KiB of guard on either side. A launch runs under a fill byte -- Z (guards, outputs and scratch
0x00) or F (0xFF: NaN in both float widths, -1 as an int32) --, Launch.run asserts return code 0, intact guards and untouched
read-only operands, and the comparisons below hold the outputs to the C oracle or to the NumPy restatements of tests/*_np.py.

  Launch, add_problem, arena_problem   the buffers of one call; an MpcqpProblem whose operands point into the arena
  Forward, discipline                  mpcqp_build_solve_batch / mpcqp_stagewise_solve_batch of a workload
  ModelCase                            mpcqp_factor_model + mpcqp_solve_model_batch / _bounds_batch of a shared-model workload
  QPs                                  mpcqp_solve_batch of given dense QPs
  PlanVjp, PlanJvp, plan_vjp, plan_jvp the derivative exports of batched plans

This module needs torch: a test module puts pytest.importorskip("torch") in front of importing it. pytest rewrites `assert` in
test_*.py only, so every assert here carries its own message. No launch ever gets a buffer smaller than the contract says."""
import ctypes as C

import numpy as np
import torch

import oracle
from oracle import condense_np

import adjoint_np as AN
import adjoint_stagewise_np as AS
import arena as AR
import operand_layouts as OL
import tangent_model_np as TM
import tangent_np as TN
from operand_layouts import f32_view, ltv  # noqa: F401  (re-exported: the float32 view of a reference, the random workloads)

Z, F = 0x00, 0xFF
I32, U8, F64, F32 = torch.int32, torch.uint8, torch.float64, torch.float32
OPS = (("A", "A"), ("B", "B"), ("C", "C"), ("D", "D"), ("e", "e"), ("x0", "initial_state"), ("goal", "goal_state"),
       ("targets", "target_states"))
EUNSUPPORTED = -6


def _api():
    from qpmpc_amd import _capi
    from qpmpc_amd.batch import _stream_ptr

    return _capi, _capi.load(), _stream_ptr


def _torch():
    return torch


def flags(names):
    """the MPCQP_OPT_* bits named in `names` (attributes of qpmpc_amd._capi), or-ed"""
    from qpmpc_amd import _capi

    out = 0
    for name in names:
        out |= getattr(_capi, name)
    return out


def _flag():
    from qpmpc_amd import _capi

    return _capi.OPT_ON_CHIP_32


def _random_ltv(seed, B, nx, nu, N, mk, tight=1.0):
    from qpmpc_amd.workloads import random_ltv

    return random_ltv(np.random.default_rng(seed), B, nx, nu, N, mk, tight)


def _triple(batch, N, seed=7):
    from qpmpc_amd import workloads as W

    A, B, Cm, e = W.triple_integrator_matrices(N)
    rng = np.random.default_rng(seed)
    x0 = np.stack([rng.uniform(-0.5, 0.5, batch), rng.uniform(-0.5, 0.5, batch), rng.uniform(-2.5, 2.5, batch)], 1)
    goal = np.stack([rng.uniform(0.5, 1.5, batch), np.zeros(batch), np.zeros(batch)], 1)
    return W._pack(A, B, Cm, None, e, N, 1.0, None, 1e-6, x0, goal, name=f"triple_integrator_N{N}")


def _esz(dtype):
    return torch.empty((), dtype=dtype).element_size()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def holds(a, byte):
    return bool((bits(a) == byte).all())


class Launch:
    """The buffers of one call. Roles: "in" (read-only: snapshotted, must be unchanged), "out" and "scratch" (filled before every
    run), "inout" (reloaded before every run, returned)."""

    def __init__(self):
        self.specs, self.arena = [], None

    def add(self, name, role, dtype, count=None, data=None, stride=None):
        rows = None
        if data is not None:
            data = torch.as_tensor(data).to("cuda", dtype).contiguous()
            rows = data.reshape(data.shape[0], -1) if data.dim() > 1 else data.reshape(1, -1)
            stride = int(stride or rows.shape[1])
            count = (rows.shape[0] - 1) * stride + rows.shape[1]
        self.specs.append(dict(name=name, role=role, dtype=dtype, count=int(count), rows=rows, stride=stride))

    def build(self):
        sizes = [s["count"] * _esz(s["dtype"]) for s in self.specs]
        self.arena = AR.Arena(AR.capacity_for(sizes), "cuda")
        for s, nb in zip(self.specs, sizes):
            if nb:  # (a buffer of no bytes is passed as NULL)
                self.arena.carve(s["name"], nb, s["dtype"])
        return self

    def has(self, name):
        return name in self.arena.spans

    def ptr(self, name):
        return self.arena.ptr(name) if self.has(name) else None

    def nbytes(self, name):
        return self.arena.nbytes(name) if self.has(name) else 0

    def run(self, byte, call, keep=()):
        """One launch under fill `byte`; buffers named in `keep` stay as the launch before left them. Asserts (a) and the
        read-only part of (c); returns every buffer that is not read-only as a NumPy array."""
        a = self.arena
        a.fill_guards(byte)
        live = [s for s in self.specs if self.has(s["name"])]
        for s in live:
            if s["name"] in keep:
                continue
            a.fill([s["name"]], byte)
            if s["rows"] is not None:
                a.view(s["name"]).as_strided(tuple(s["rows"].shape), (s["stride"], 1)).copy_(s["rows"])
        ro = [s["name"] for s in live if s["role"] == "in"]
        a.snapshot(ro)
        torch.cuda.synchronize()
        rc = call()
        torch.cuda.synchronize()
        assert rc == 0, f"return code {rc}"
        damaged = a.guards_intact()
        assert damaged == [], f"fill {byte:#04x}: overrun (buffer, side, first, last, bytes) {damaged}"
        changed = a.unchanged(ro)
        assert changed == [], f"fill {byte:#04x}: read-only buffer written (buffer, first byte, bytes) {changed}"
        return {s["name"]: a.view(s["name"]).clone().cpu().numpy() for s in live if s["role"] != "in"}


def pad_of(pad, name):
    """elements of batch-stride padding of operand `name`: `pad` is one int for every operand or a dict name -> elements"""
    return int(pad.get(name, 0)) if isinstance(pad, dict) else int(pad)


def add_problem(L, bp, pad=0, inout=()):
    """the operands of `bp`, read-only but for those named in `inout` (a fused period writes the next problem over them)"""
    for name, attr in OPS:
        t = getattr(bp, attr)
        if t is not None:
            rows = t.reshape(t.shape[0], -1)
            L.add("op_" + name, "inout" if name in inout else "in", bp.dtype, data=rows,
                  stride=rows.shape[1] + (pad_of(pad, name) if rows.shape[0] > 1 else 0))


def arena_problem(L, bp, pad=0):
    """MpcqpProblem of `bp` with every operand pointing into the arena (batch strides `pad` elements past the packed ones; `pad`
    as in pad_of)."""
    _capi = _api()[0]
    ops = []
    for name, attr in OPS:
        t = getattr(bp, attr)
        if t is None:
            ops.append(_capi.Operand(None, 0, 0))
            continue
        o = bp._operand(t)
        bs = 0 if t.shape[0] == 1 else t.reshape(t.shape[0], -1).shape[1] + pad_of(pad, name)
        ops.append(_capi.Operand(L.ptr("op_" + name), bs, o.step_stride))
    return _capi.Problem(*ops)


def _solve_opts(L, flags=0, max_iter=0, warm_start=0):
    """MpcqpSolveOpts with the pairing order and the warm state of the arena, where it has them"""
    o = _api()[0].SolveOpts()
    o.flags, o.max_iter = int(flags), int(max_iter)
    if L.has("order"):
        o.order = L.ptr("order")
    if L.has("warm"):
        o.warm_state, o.warm_state_bytes, o.warm_start = L.ptr("warm"), L.nbytes("warm"), int(warm_start)
    return o


def _add_outputs(L, dtype, B, n, m, ws_bytes, order, warm_bytes):
    """U, lam, status, iters and the workspace of a solve, then its pairing order and warm state where asked for"""
    L.add("U", "out", dtype, B * n)
    L.add("lam", "out", dtype, B * m)
    L.add("status", "out", I32, B)
    L.add("iters", "out", I32, B)
    L.add("ws", "scratch", U8, ws_bytes)
    if order is not None:
        L.add("order", "in", I32, data=torch.as_tensor(np.asarray(order, dtype=np.int32)))
    if warm_bytes:
        L.add("warm", "scratch", U8, warm_bytes)


# ---------------------------------------------------------------------------------------------- workloads
_ORACLE = {}


def oracle_of(key, w):
    if key not in _ORACLE:
        Uo, lamo, sto, _ = oracle.solve_workload(w)
        _ORACLE[key] = (Uo, lamo, sto)
    return _ORACLE[key]


def _dense_qps(rng, B, n, m):
    """the dense QPs of tests/test_gpu_parity.py::_random_dense_qps: h > 0, so x = 0 is feasible and every problem has a solution"""
    Ps, qs, Gs, hs = [], [], [], []
    for _ in range(B):
        M = rng.standard_normal((n, n))
        Ps.append(M @ M.T / n + 0.1 * np.eye(n))
        qs.append(rng.standard_normal(n))
        Gs.append(rng.standard_normal((m, n)))
        hs.append(np.abs(rng.standard_normal(m)) * 0.2 + 0.05)
    return [np.stack(a) for a in (Ps, qs, Gs, hs)]


def _rel(got, want):
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def condense_refs(w, count):
    from qpmpc_amd.workloads import problem_from_workload

    return [condense_np.condense(problem_from_workload(w, b)) for b in range(count)]


# ---------------------------------------------------------------------------------------------- forward exports
class Forward:
    """mpcqp_build_solve_batch (or mpcqp_stagewise_solve_batch) of a workload with everything in an arena. workspace=False:
    the workspace pointer NULL and its size 0 whatever mpcqp_workspace_bytes says for the dimensions (no query is made)."""

    def __init__(self, w, dtype=None, stagewise=False, max_active=0, query=None, pad=0, order=None, warm=False, inout=(),
                 workspace=True):
        from qpmpc_amd import workloads as W

        _capi, lib, _ = _api()
        self.bp = bp = W.to_batch_problem(w, dtype=dtype)
        self.B, self.n, self.m = bp.batch_size, bp.nb_variables, bp.nb_constraints
        self.dims, self.stagewise, self.max_active, self.pad = bp.dims(), stagewise, int(max_active), pad
        self.ws_bytes = 0
        if workspace:
            nbytes = C.c_size_t(0)
            if stagewise:
                rc = lib.mpcqp_stagewise_workspace_bytes(C.byref(self.dims), self.B, int(max_active if query is None else query),
                                                         C.byref(nbytes))
            else:
                rc = lib.mpcqp_workspace_bytes(C.byref(self.dims), self.B, 1, C.byref(nbytes))
            assert rc == 0, f"the workspace query returned {rc}"
            self.ws_bytes = nbytes.value
        wb = C.c_size_t(0)
        if warm:
            rc = lib.mpcqp_warm_state_bytes(C.byref(self.dims), C.byref(wb))
            assert rc == 0 and wb.value > 0, f"mpcqp_warm_state_bytes returned {rc}, {wb.value} bytes"
        L = self.L = Launch()
        add_problem(L, bp, pad, inout)  # (inout: operands a call rewrites itself, tests/test_gpu_streams.py)
        _add_outputs(L, bp.dtype, self.B, self.n, self.m, self.ws_bytes, order, self.B * wb.value)
        L.build()
        self.cp = arena_problem(L, bp, pad)
        if workspace:
            print(f"    batch {self.B} n {self.n} m {self.m}: workspace {self.ws_bytes} bytes")

    def run(self, byte, flags=0, lam=True, iters=True, warm_start=0, keep=(), max_iter=0, factor_slot=0, warm_shift=0):
        _capi, lib, stream = _api()
        L = self.L
        o = _solve_opts(L, flags, max_iter, warm_start)
        o.factor_slot = int(factor_slot)
        if L.has("warm"):
            o.warm_shift = int(warm_shift)
        tail = (L.ptr("U"), L.ptr("lam") if lam else None, L.ptr("status"), L.ptr("iters") if iters else None, L.ptr("ws"),
                self.ws_bytes, stream())

        def call():
            if self.stagewise:
                return lib.mpcqp_stagewise_solve_batch(C.byref(self.dims), C.byref(self.cp), self.B, C.byref(o), self.max_active,
                                                       *tail)
            return lib.mpcqp_build_solve_batch(C.byref(self.dims), C.byref(self.cp), self.B, C.byref(o), *tail)

        out = L.run(byte, call, keep)
        out["U"] = out["U"].reshape(self.B, self.n)
        out["lam"] = out["lam"].reshape(self.B, self.m)
        return out


def solve_outputs(w, flags=0, **kw):
    """(U, lam, status, iters) of solve_mpc_batch on a workload, through the Python layer, as NumPy arrays"""
    from qpmpc_amd import solve_mpc_batch
    from qpmpc_amd import workloads as W

    plan = solve_mpc_batch(W.to_batch_problem(w), flags=flags, return_multipliers=True, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (plan.U, plan.multipliers, plan.status, plan.iters))


def equal_outputs(a, b, what, items=None, lam=True, iters=True):
    """(b): status and iters of every item (of `items`), U of every item (no plan: zeros), lam of the solved ones."""
    sel = np.ones(len(a["status"]), dtype=bool) if items is None else items
    assert np.array_equal(a["status"][sel], b["status"][sel]), (what, "status", a["status"], b["status"])
    if iters:
        assert np.array_equal(a["iters"][sel], b["iters"][sel]), (what, "iters", a["iters"], b["iters"])
    bad = [i for i in np.flatnonzero(sel) if not same_bits(a["U"][i], b["U"][i])]
    assert not bad, (what, "U differs for items", bad, a["status"][bad], a["U"][bad[0]], b["U"][bad[0]])
    if lam:
        ok = sel & (a["status"] == 0)
        bad = [i for i in np.flatnonzero(ok) if not same_bits(a["lam"][i], b["lam"][i])]
        assert not bad, (what, "lam differs for items", bad)


def same_plans(a, b, what):
    """two entry points that launch the same kernel (their slot counts may differ): statuses equal, plans equal to rounding"""
    assert np.array_equal(a["status"], b["status"]), (what, a["status"], b["status"])
    ok = a["status"] == 0
    if ok.any():
        ua, ub = a["U"][ok].astype(np.float64), b["U"][ok].astype(np.float64)
        assert np.abs(ua - ub).max() <= 1e-9 * max(1.0, np.abs(ua).max()), (what, float(np.abs(ua - ub).max()))


def against_oracle(key, w, out, tol, skip_status=()):
    """(d) for a forward export; items whose status is in `skip_status` (MPCQP_SLOTS_FULL) have no counterpart in the oracle."""
    Uo, lamo, sto = oracle_of(key, w)
    st, U = out["status"], out["U"].astype(np.float64)
    cmp = ~np.isin(st, skip_status)
    assert cmp.sum() * 2 >= len(st), (key, "fewer than half of the batch has a counterpart in the oracle", st)
    assert np.array_equal(st[cmp] == 0, sto[cmp] == 0), (key, "solved / unsolved differ from the oracle", st, sto)
    ok = cmp & (sto == 0)
    assert ok.sum() * 2 >= len(st), (key, "fewer than half of the batch is compared", st, sto)
    scale = np.maximum(1.0, np.abs(Uo[ok]).max(axis=1, keepdims=True))
    err = float((np.abs(U[ok] - Uo[ok]) / scale).max())
    print(f"    {key}: {int(ok.sum())} of {len(st)} solved, max rel err vs oracle {err:.2e}")
    assert err <= tol, (key, "max rel err vs oracle", err, tol)
    assert not np.isnan(U).any() and (U[st != 0] == 0).all(), (key, "no plan: zeros, never NaN", st)
    return ok


def discipline(key, w, tol=1e-7, flags=0, skip_status=(), reference=None, **kw):
    """(a) .. (e) of one forward launch: twice under fill Z, once under fill F, once with lam and iters NULL under fill F."""
    case = Forward(w, **kw)
    z1, z2, f = case.run(Z, flags), case.run(Z, flags), case.run(F, flags)
    equal_outputs(z1, z2, key + ": run to run under fill Z")
    equal_outputs(z1, f, key + ": fill Z against fill F")
    nn = case.run(F, flags, lam=False, iters=False)
    assert holds(nn["lam"], F) and holds(nn["iters"], F), key + ": a NULL output's neighbour was written"
    equal_outputs(f, nn, key + ": lam and iters NULL", lam=False, iters=False)
    against_oracle(key, reference if reference is not None else w, f, tol, skip_status)
    return case, f


# ---------------------------------------------------------------------------------------------- shared-model solves
class ModelCase:
    """A factored model and the per-problem operands of one shared-model workload `w` (A, B, C, D shared; x0, goal, targets, e
    with 1 or B rows, `pad` elements past the packed batch stride) in a guarded arena. The model is factored from the
    pseudo-problems of include/mpcqp.h (x0 = goal = targets = 0, then unit vectors; bounds: w["e_model"], else the first
    problem's), condensed by the library once. factor_in_arena=False: mpcqp_factor_model runs once, outside the arena, and the
    model is copied in as a read-only buffer, so a solve that wrote into it is named. factor_in_arena=True: P, G, qb, hb are
    read-only buffers of the arena, the model is scratch of exactly mpcqp_model_bytes, and every run factors it again before
    it solves -- mpcqp_factor_model's own memory contract. The operands named in `inout` are reloaded before every run and may
    be rewritten inside a call (tests/test_gpu_streams.py)."""

    def __init__(self, w, pad=None, dtype=F64, order=None, warm=False, wt=None, inout=(), factor_in_arena=False):
        from qpmpc_amd import BatchMPCQP, BatchMPCProblem, _capi

        _, lib, stream = _api()
        pad = pad or {}
        N = int(w["N"])
        nx, nu, mk = w["A"].shape[-1], w["B"].shape[-1], w["e"].shape[-1]
        self.B = B = max(w[k].shape[0] for k in ("x0", "goal", "targets", "e") if w.get(k) is not None)
        self.n, self.m, self.dtype, self.factor_in_arena = N * nu, N * mk, dtype, factor_in_arena
        nb = 1 + 2 * nx + N * nx
        x0, goal, tgt = torch.zeros((nb, nx), dtype=dtype), torch.zeros((nb, nx), dtype=dtype), torch.zeros((nb, N * nx), dtype=dtype)
        x0[1:1 + nx], goal[1 + nx:1 + 2 * nx], tgt[1 + 2 * nx:] = torch.eye(nx), torch.eye(nx), torch.eye(N * nx)
        pseudo = BatchMPCProblem(w["A"], w["B"], w["C"], w["D"], w.get("e_model", w["e"][:1]), N, w["wt"] if wt is None else wt, w["wx"], w["wu"],
                                 x0, goal_state=goal, target_states=tgt if w["wx"] is not None else None, dtype=dtype)
        self.mdims = pseudo.dims()
        qp = BatchMPCQP(pseudo, keep_propagators=False)
        torch.cuda.synchronize()
        mbytes = C.c_size_t(0)
        rc = lib.mpcqp_model_bytes(C.byref(self.mdims), C.byref(mbytes))
        assert rc == 0, f"mpcqp_model_bytes returned {rc}"
        self.model_bytes = mbytes.value
        L = self.L = Launch()
        if factor_in_arena:
            L.add("P", "in", dtype, data=qp.P[0].reshape(1, -1))
            L.add("G", "in", dtype, data=qp.G[0].reshape(1, -1))
            L.add("qb", "in", dtype, data=qp.q.reshape(1, -1))
            L.add("hb", "in", dtype, data=qp.h.reshape(1, -1))
            L.add("model", "scratch", U8, mbytes.value)
        else:
            model = torch.zeros((mbytes.value,), dtype=U8, device="cuda")
            rc = lib.mpcqp_factor_model(C.byref(self.mdims), qp.P[0].data_ptr(), qp.G[0].data_ptr(), qp.q.data_ptr(), qp.h.data_ptr(),
                                        model.data_ptr(), mbytes.value, stream())
            assert rc == 0, f"mpcqp_factor_model returned {rc}"
            torch.cuda.synchronize()
            L.add("model", "in", U8, data=model)
        ops = {}
        for key, width in (("x0", nx), ("goal", nx), ("targets", N * nx), ("e", self.m)):
            if w.get(key) is None:
                ops[key] = None
                continue
            rows = np.asarray(w[key]).reshape(w[key].shape[0], -1)
            assert rows.shape[1] == width and rows.shape[0] in (1, B), (key, rows.shape, width, B)
            stride = width + int(pad.get(key, 0)) if rows.shape[0] > 1 else 0
            L.add(key, "inout" if key in inout else "in", dtype, data=rows, stride=stride or None)
            ops[key] = (stride, mk if key == "e" else 0)
        _add_outputs(L, dtype, B, self.n, self.m, 0, order, B * 4096 if warm else 0)
        L.build()
        self.ops = {key: (_capi.Operand(None, 0, 0) if v is None else _capi.Operand(L.ptr(key), v[0], v[1])) for key, v in ops.items()}

    def run(self, byte, flags=0, bounds=True, lam=True, iters=True, max_iter=0, expect=0):
        """one launch under fill `byte`: the arena's checks (guards intact, read-only buffers -- the model or P, G, qb, hb among
        them -- unchanged) and the return code `expect`; the outputs, U [B, n] and lam [B, m]"""
        _capi, lib, stream = _api()
        L = self.L
        o = _solve_opts(L, flags, max_iter)
        ops = self.ops
        tail = (C.byref(ops["x0"]), C.byref(ops["goal"]), C.byref(ops["targets"]), self.B, C.byref(o), L.ptr("U"),
                L.ptr("lam") if lam else None, L.ptr("status"), L.ptr("iters") if iters else None, stream())
        got = {}

        def call():
            if self.factor_in_arena:
                got["rc"] = lib.mpcqp_factor_model(C.byref(self.mdims), L.ptr("P"), L.ptr("G"), L.ptr("qb"), L.ptr("hb"), L.ptr("model"),
                                                   self.model_bytes, stream())
                if got["rc"]:
                    return 0
            if bounds:
                got["rc"] = lib.mpcqp_solve_model_bounds_batch(C.byref(self.mdims), L.ptr("model"), C.byref(ops["e"]), *tail)
            else:
                got["rc"] = lib.mpcqp_solve_model_batch(C.byref(self.mdims), L.ptr("model"), *tail)
            return 0

        out = L.run(byte, call)
        assert got["rc"] == expect, f"return code {got['rc']}, expected {expect}"
        out["U"], out["lam"] = out["U"].reshape(self.B, self.n), out["lam"].reshape(self.B, self.m)
        return out

    def refused(self, flags=0, bounds=True):
        """a launch that must return MPCQP_EUNSUPPORTED and write no output"""
        out = self.run(F, flags, bounds, expect=EUNSUPPORTED)
        assert all(holds(out[k], F) for k in ("U", "lam", "status", "iters")), "a refused launch wrote an output"


# ---------------------------------------------------------------------------------------------- dense QPs
class QPs:
    """The buffers of one mpcqp_solve_batch call in a guarded arena: P, q, G, h read-only (those named in `inout` reloaded before
    every run and writable), x, lam, status, iters filled before every run; with workspace=True a workspace of exactly
    mpcqp_solve_workspace_bytes, else the workspace pointer NULL and its size 0. m = 0: no G, h, lam."""

    def __init__(self, P, q, G, h, dtype=F64, inout=(), order=None, warm=False, workspace=False):
        _capi, lib, _ = _api()
        self.B, self.n = q.shape
        self.m = 0 if G is None else G.shape[1]
        self.dtype, self.code = dtype, _capi.F64 if dtype == F64 else _capi.F32
        nbytes = C.c_size_t(0)
        if workspace:
            rc = lib.mpcqp_solve_workspace_bytes(self.n, self.m, self.code, self.B, C.byref(nbytes))
            assert rc == 0, f"mpcqp_solve_workspace_bytes returned {rc}"
        self.ws_bytes = nbytes.value
        L = self.L = Launch()
        for key, a in (("P", P), ("q", q), ("G", G), ("h", h)):
            if a is not None and a.size:
                L.add(key, "inout" if key in inout else "in", dtype, data=np.array(a).reshape(self.B, -1))  # (a writable copy)
        _add_outputs(L, dtype, self.B, self.n, self.m, self.ws_bytes, order, self.B * 4096 if warm else 0)
        L.build()

    def c_call(self, flags, lam=True, iters=True, status=True, max_iter=0, stream=None):
        """the C call on the arena's buffers; its return code"""
        _capi, lib, cur = _api()
        L = self.L
        o = _solve_opts(L, flags, max_iter)
        return lib.mpcqp_solve_batch(self.n, self.m, self.code, L.ptr("P"), L.ptr("q"), L.ptr("G"), L.ptr("h"), self.B, C.byref(o),
                                     L.ptr("U"), L.ptr("lam") if lam else None, L.ptr("status") if status else None,
                                     L.ptr("iters") if iters else None, L.ptr("ws"), self.ws_bytes, cur() if stream is None else stream)

    def shaped(self, out):
        out["U"] = out["U"].reshape(self.B, self.n)
        if "lam" in out:
            out["lam"] = out["lam"].reshape(self.B, self.m)
        return out

    def run(self, byte, flags, **kw):
        return self.shaped(self.L.run(byte, lambda: self.c_call(flags, **kw)))

    def rc(self, flags, **kw):
        """(return code, outputs) of a launch that may be refused; the arena's checks run as for any launch"""
        got = {}

        def call():
            got["rc"] = self.c_call(flags, **kw)
            return 0

        out = self.L.run(F, call)
        return got["rc"], out


# ---------------------------------------------------------------------------------------------- derivative exports
def forward_on_cpu(w, unsolved=()):
    """U, lam, status of every problem by the C oracle (what a forward launch hands the derivative exports); the items of
    `unsolved` are marked MPCQP_MAX_ITER."""
    Uo, lamo, sto = oracle.solve_workload(w)[:3]
    sto = np.asarray(sto, dtype=np.int32).copy()
    for b in unsolved:
        sto[b] = 1
    return np.asarray(Uo, dtype=float), np.asarray(lamo, dtype=float), sto


def max_active_of(lam, status, n):
    return int(min(((lam > 0) & (status == 0)[:, None]).sum(axis=1).max(), n))


def close(got, want, what):
    err = float(np.abs(np.asarray(got).ravel() - np.asarray(want).ravel()).max()) if np.asarray(want).size else 0.0
    assert err <= 1e-8 * max(1.0, float(np.abs(want).max()) if np.asarray(want).size else 0.0), (what, err)


def _tangents(w, B, T, rng, model):
    N = int(w["N"])
    nx, nu, mk = np.asarray(w["x0"]).shape[-1], np.asarray(w["B"]).shape[-1], np.asarray(w["e"]).shape[-1]
    tan = dict(x0=rng.standard_normal((B, T, nx)), goal=rng.standard_normal((B, T, nx)),
               targets=rng.standard_normal((B, T, N * nx)), e=rng.standard_normal((B, T, N * mk)))
    if model:
        tan.update(A=rng.standard_normal((B, T, N, nx, nx)), B=rng.standard_normal((B, T, N, nx, nu)),
                   C=rng.standard_normal((B, T, N, mk, nx)), D=rng.standard_normal((B, T, N, mk, nu)),
                   w=rng.standard_normal((B, T, 3)))
    return tan


def SIZES(nx, nu, N, mk):
    return dict(x0=nx, goal=nx, targets=N * nx, e=N * mk, A=N * nx * nx, B=N * nx * nu, C=N * mk * nx, D=N * mk * nu, w=3)


def _derivative_status(vst, status):
    assert np.array_equal(vst[status != 0], status[status != 0]) and (vst[status == 0] == 0).all(), (vst, status)


class PlanVjp:
    """mpcqp_plan_vjp_batch ("condensed") / _vjp_model_batch ("model") / _vjp_stagewise_batch ("stagewise") on the plans U, the
    multipliers lam and the statuses of workload `w` (operands in the stored layout, batch strides padded by `pad`), with the
    seeded cotangents gU, gX, every gradient asked for: the buffers in a guarded arena, a workspace of exactly the queried size."""

    def __init__(self, kind, shape, w, U, lam, status, pad=0):
        from qpmpc_amd import _capi, autodiff
        from qpmpc_amd import workloads as W

        _, lib, _ = _api()
        nx, nu, N, mk = shape
        self.kind, self.U, self.lam, self.status = kind, U, lam, status
        bp = W.to_batch_problem(w)
        self.B = B = bp.batch_size
        n = N * nu
        assert (status == 0).sum() * 2 >= B, ("fewer than half of the batch is solved", status)
        rng = np.random.default_rng(3)
        self.gU, self.gX = rng.standard_normal((B, n)), rng.standard_normal((B, (N + 1) * nx))
        self.dims, nbytes = autodiff._vjp_dims(bp), C.c_size_t(0)
        self.ka = max_active_of(lam, status, n)
        if kind == "condensed":
            rc = lib.mpcqp_plan_vjp_workspace_bytes(C.byref(self.dims), B, C.byref(nbytes))
        elif kind == "model":
            rc = lib.mpcqp_plan_vjp_model_workspace_bytes(C.byref(self.dims), B, C.byref(nbytes))
        else:
            rc = lib.mpcqp_plan_vjp_stagewise_workspace_bytes(C.byref(self.dims), B, self.ka, C.byref(nbytes))
        assert rc == 0, f"the workspace query returned {rc}"
        self.ws_bytes = nbytes.value
        self.sizes = SIZES(*shape)
        self.outs = list(self.sizes)[:4] if kind == "condensed" else list(self.sizes)
        L = self.L = Launch()
        add_problem(L, bp, pad)
        for key, a in (("lam", lam), ("U", U), ("gU", self.gU), ("gX", self.gX)):
            L.add(key, "in", F64, data=a)
        L.add("status", "in", I32, data=torch.as_tensor(status))
        for key in self.outs:
            L.add("g_" + key, "out", F64, B * self.sizes[key])
        L.add("vjp_status", "out", I32, B)
        L.add("ws", "scratch", U8, nbytes.value)
        L.build()
        self.cp = arena_problem(L, bp, pad)

    def call(self, full=True):
        """the export's call for Launch.run; full=False: the nullable pointers NULL (gX, every gradient but g_x0)"""
        _capi, lib, stream = _api()
        L, kind = self.L, self.kind
        ptrs = [L.ptr("g_" + k) if k in (self.outs if full else ["x0"]) else None for k in self.sizes]
        head = (C.byref(self.dims), C.byref(self.cp), self.B)
        tail = (L.ptr("vjp_status"), L.ptr("ws"), self.ws_bytes, stream())
        gX = L.ptr("gX") if full else None
        if kind == "condensed":
            return lambda: lib.mpcqp_plan_vjp_batch(*head, L.ptr("lam"), L.ptr("status"), L.ptr("gU"), gX, *ptrs[:4], *tail)
        res = _capi.VjpModelOut(*ptrs)
        if kind == "model":
            return lambda: lib.mpcqp_plan_vjp_model_batch(*head, L.ptr("lam"), L.ptr("status"), L.ptr("U"), L.ptr("gU"), gX,
                                                          C.byref(res), *tail)
        return lambda: lib.mpcqp_plan_vjp_stagewise_batch(*head, self.ka, L.ptr("lam"), L.ptr("status"), L.ptr("U"), L.ptr("gU"), gX,
                                                          C.byref(res), *tail)

    def check(self, f, full, what):
        """the outputs `f` of a full call: the statuses are the forward's, an unsolved item's gradients are zeros, every other
        gradient is the NumPy restatement's on the materialised problem `full` (the sum over a shared operand is the caller's);
        the gradients {operand: [B, size]} and the statuses"""
        B, kind, U, lam, status = self.B, self.kind, self.U, self.lam, self.status
        vst = f["vjp_status"]
        _derivative_status(vst, status)
        for b in range(B):
            got = {k: f["g_" + k].reshape(B, -1)[b] for k in self.outs}
            if vst[b] != 0:
                assert all((g == 0).all() for g in got.values()), (b, "an unsolved item's gradients are zeros")
                continue
            w1 = AN.single(full, b)
            ref = AN.vjp(w1, lam[b], self.gU[b], self.gX[b]) if kind == "condensed" else AS.stagewise_vjp(w1, lam[b], self.gU[b], self.gX[b], U[b])
            for k in self.outs:
                close(got[k], ref[k], (kind, what, b, k))
        return {k: f["g_" + k].reshape(B, -1) for k in self.outs}, vst


def plan_vjp(kind, shape, case, pad, layout):
    """one launch of PlanVjp under fill F and its comparisons on `case` = (w, full, U, lam, status) of OL.BATCH problems with
    batch-stride padding `pad` (`layout` names the case in a failure); returns the gradients {operand: [B, size]} and the statuses"""
    w, full, U, lam, status = case
    p = PlanVjp(kind, shape, w, U, lam, status, pad)
    assert p.B == OL.BATCH, p.B
    return p.check(p.L.run(F, p.call()), full, layout)


class PlanJvp:
    """mpcqp_plan_jvp_batch / _jvp_stagewise_batch / _jvp_model_batch / _jvp_model_stagewise_batch on the plans of workload `w`
    with the tangents `tan` ({operand: [B, T, ...]}), set up as PlanVjp; max_active as autodiff._max_active counts it."""

    def __init__(self, model, stagewise, shape, w, U, lam, status, tan, pad=0):
        from qpmpc_amd import _capi, autodiff
        from qpmpc_amd import workloads as W

        _, lib, _ = _api()
        nx, nu, N, mk = shape
        self.model, self.stagewise, self.U, self.lam, self.status, self.tan = model, stagewise, U, lam, status, tan
        bp = W.to_batch_problem(w)
        self.B = B = bp.batch_size
        self.T = T = tan["x0"].shape[1]
        n = N * nu
        assert (status == 0).sum() * 2 >= B, ("fewer than half of the batch is solved", status)
        self.dims, nbytes = autodiff._vjp_dims(bp), C.c_size_t(0)
        self.ka = max_active_of(lam, status, n)
        query = {(False, False): lib.mpcqp_plan_jvp_workspace_bytes, (True, False): lib.mpcqp_plan_jvp_model_workspace_bytes,
                 (False, True): lib.mpcqp_plan_jvp_stagewise_workspace_bytes,
                 (True, True): lib.mpcqp_plan_jvp_model_stagewise_workspace_bytes}[(model, stagewise)]
        extra = (self.ka, T) if stagewise else (T,)
        rc = query(C.byref(self.dims), B, *extra, C.byref(nbytes))
        assert rc == 0, f"the workspace query returned {rc}"
        self.ws_bytes = nbytes.value
        L = self.L = Launch()
        add_problem(L, bp, pad)
        L.add("lam", "in", F64, data=lam)
        L.add("U", "in", F64, data=U)
        L.add("status", "in", I32, data=torch.as_tensor(status))
        for key, a in tan.items():
            L.add("d" + key, "in", F64, data=a.reshape(B, -1))
        L.add("dU", "out", F64, B * T * n)
        L.add("dX", "out", F64, B * T * (N + 1) * nx)
        L.add("jvp_status", "out", I32, B)
        L.add("ws", "scratch", U8, nbytes.value)
        L.build()
        self.cp = arena_problem(L, bp, pad)
        self.ctan = _capi.Tangents(*[L.ptr("d" + k) for k in ("x0", "goal", "targets", "e")],
                                   *[tan[k][0].size for k in ("x0", "goal", "targets", "e")])
        self.mtan = _capi.ModelTangents(*[L.ptr("d" + k) for k in ("A", "B", "C", "D", "w")],
                                        *[tan[k][0].size for k in ("A", "B", "C", "D", "w")]) if model else None

    def call(self, full=True):
        """the export's call for Launch.run; full=False: dX and jvp_status NULL"""
        _, lib, stream = _api()
        L = self.L
        head = (C.byref(self.dims), C.byref(self.cp), self.B) + ((self.ka,) if self.stagewise else ()) + (self.T, L.ptr("lam"), L.ptr("status"))
        tail = (L.ptr("dU"), L.ptr("dX") if full else None, L.ptr("jvp_status") if full else None, L.ptr("ws"), self.ws_bytes,
                stream())
        if self.model:
            fn = lib.mpcqp_plan_jvp_model_stagewise_batch if self.stagewise else lib.mpcqp_plan_jvp_model_batch
            return lambda: fn(*head, L.ptr("U"), C.byref(self.ctan), C.byref(self.mtan), *tail)
        fn = lib.mpcqp_plan_jvp_stagewise_batch if self.stagewise else lib.mpcqp_plan_jvp_batch
        return lambda: fn(*head, C.byref(self.ctan), *tail)

    def check(self, f, full, what, which=None):
        """the outputs `f` of a full call: the statuses are the forward's, an unsolved item's tangents are zeros, dU and dX of
        the tangents `which` (all of them by default) are the NumPy restatement's on the materialised problem `full`;
        dU, dX [B, T, -1] and the statuses"""
        B, T, tan, U, lam, status = self.B, self.T, self.tan, self.U, self.lam, self.status
        vst = f["jvp_status"]
        _derivative_status(vst, status)
        dU, dX = f["dU"].reshape(B, T, -1), f["dX"].reshape(B, T, -1)
        for b in range(B):
            if vst[b] != 0:
                assert (dU[b] == 0).all() and (dX[b] == 0).all(), (b, "an unsolved item's tangents are zeros")
                continue
            w1 = AN.single(full, b)
            for t in range(T) if which is None else which:
                one = {k: a[b, t] for k, a in tan.items()}
                ref = TM.jvp_model(w1, U[b], lam[b], one) if self.model else TN.jvp(w1, lam[b], one)
                close(dU[b, t], ref["U"], (what, b, t, "dU"))
                close(dX[b, t], ref["X"], (what, b, t, "dX"))
        return dU, dX, vst


def plan_jvp(model, stagewise, shape, case, pad, layout, tan=None):
    """one launch of PlanJvp under fill F and its comparisons on `case` = (w, full, U, lam, status) of OL.BATCH problems, with
    three random tangents or with `tan` ({operand: [B, 3, ...]}); returns dU, dX [B, 3, -1] and the statuses"""
    w, full, U, lam, status = case
    tan = _tangents(full, OL.BATCH, 3, np.random.default_rng(4), model) if tan is None else tan
    p = PlanJvp(model, stagewise, shape, w, U, lam, status, tan, pad)
    assert p.B == OL.BATCH and p.T == 3, (p.B, p.T)
    return p.check(p.L.run(F, p.call()), full, layout)
