"""CPU tests of the host side of the batched forward solves (qpmpc_amd/batch.py): which failures of a re-solve the retry
helpers take for "not served" and which they let through, what ``_capi.check`` raises, and that ``solve_mpc_batch`` hands the
library the arguments a ``PreparedSolve`` of the same request hands it. Nothing is launched: the re-solves and the library
are stubs, the tensors live on the CPU."""
import ctypes as C

import pytest

torch = pytest.importorskip("torch")

from qpmpc_amd import BackendError, _capi  # noqa: E402
from qpmpc_amd import batch as Bt  # noqa: E402
from qpmpc_amd import workloads as W  # noqa: E402

CPU = torch.device("cpu")


def _problem(batch=4):
    return W.to_batch_problem(W.triple_integrator_batch(batch), device=CPU)  # n = 16 variables, m = 32 rows


def _plan(status):
    """A hand-made plan of triple-integrator problems: item b holds U = b, iters = 10 + b, multipliers = -b."""
    bp = _problem(len(status))
    b = torch.arange(len(status), dtype=torch.float64)
    plan = Bt.BatchPlan(bp, b[:, None].repeat(1, bp.nb_variables), torch.tensor(status, dtype=torch.int32),
                        (10 + b).to(torch.int32), -b[:, None].repeat(1, bp.nb_constraints))
    plan._states = "stale"
    return plan


def _resolved(problem, status=_capi.SOLVED):
    """What a re-solve of ``problem`` returns: U = 7, iters = 5, multipliers = 3 for every item."""
    Bn = problem.batch_size
    return Bt.BatchPlan(problem, torch.full((Bn, problem.nb_variables), 7.0, dtype=torch.float64),
                        torch.full((Bn,), status, dtype=torch.int32), torch.full((Bn,), 5, dtype=torch.int32),
                        torch.full((Bn, problem.nb_constraints), 3.0, dtype=torch.float64))


def _refusal(code):
    return BackendError(f"stub failed with code {code}", code=code)


def test_retry_unsolved_takes_refusals_for_not_served_and_merges_the_resolve(monkeypatch):
    plan = _plan([0, _capi.MAX_ITER, 0, _capi.MAX_ITER])
    calls = []

    def stub(problem, **kw):
        calls.append(kw)
        if len(calls) == 1:
            raise _refusal(_capi.ETOOLARGE)
        if len(calls) == 2:
            raise _refusal(_capi.EUNSUPPORTED)
        assert problem.batch_size == 2 and torch.equal(problem.initial_state, plan.problem.initial_state[[1, 3]])
        return _resolved(problem)

    monkeypatch.setattr(Bt, "solve_mpc_batch", stub)
    Bt._retry_unsolved(plan, None, None, {})
    assert len(calls) == 3  # (nothing is left for the fourth formulation)
    assert [kw.get("flags") for kw in calls] == [_capi.OPT_FORCE_LDS, _capi.OPT_STAGE_GENERAL, _capi.OPT_FORCE_CONDENSED]
    assert calls[1]["formulation"] == "stagewise" and all(kw["retry_unsolved"] is False for kw in calls)
    assert plan.status.tolist() == [0, 0, 0, 0] and plan.iters.tolist() == [10, 5, 12, 5]
    for b, (u, lam) in enumerate([(0.0, 0.0), (7.0, 3.0), (2.0, -2.0), (7.0, 3.0)]):
        assert (plan.U[b] == u).all() and (plan.multipliers[b] == lam).all()
    assert plan._states is None


def test_retry_unsolved_merges_only_what_the_resolve_solved(monkeypatch):
    plan = _plan([_capi.MAX_ITER, 0, _capi.MAX_ITER])

    def stub(problem, **kw):
        again = _resolved(problem)
        again.status[0] = _capi.MAX_ITER  # (item 0 of the plan stays unsolved through every formulation)
        return again

    monkeypatch.setattr(Bt, "solve_mpc_batch", stub)
    Bt._retry_unsolved(plan, None, None, {})
    assert plan.status.tolist() == [_capi.MAX_ITER, 0, 0] and plan.iters.tolist() == [10, 11, 5]
    assert (plan.U[0] == 0.0).all() and (plan.U[1] == 1.0).all() and (plan.U[2] == 7.0).all()


@pytest.mark.parametrize("code", [_capi.EWORKSPACE, _capi.EINVAL, _capi.ELAYOUT, 1, None])
def test_retry_unsolved_lets_real_failures_through(monkeypatch, code):
    """Workspace, argument and layout errors, a HIP error (positive code) and an error raised in Python are no refusals."""
    plan = _plan([0, _capi.MAX_ITER, 0, _capi.MAX_ITER])
    exn = _refusal(code)

    def stub(problem, **kw):
        raise exn

    monkeypatch.setattr(Bt, "solve_mpc_batch", stub)
    with pytest.raises(BackendError) as caught:
        Bt._retry_unsolved(plan, None, None, {})
    assert caught.value is exn and caught.value.code == code
    assert plan.status.tolist() == [0, _capi.MAX_ITER, 0, _capi.MAX_ITER] and plan._states == "stale"


def test_retry_slots_full_doubles_up_to_the_cap_and_stops_quietly_when_not_served(monkeypatch):
    full = _capi.SLOTS_FULL
    plan = _plan([0, full, full, 0])
    cap = min(plan.problem.nb_variables, plan.problem.nb_constraints)
    assert cap == 16
    asked = []

    def never_fits(problem, **kw):
        asked.append(kw["max_active"])
        assert kw["formulation"] == "stagewise" and kw["retry_slots"] is False and problem.batch_size == 2
        return _resolved(problem, full)

    monkeypatch.setattr(Bt, "solve_mpc_batch", never_fits)
    Bt._retry_slots_full(plan, 3, None, None, {})
    assert asked == [6, 12, cap]  # twice the slots per round, never more than can be active at once
    assert plan.status.tolist() == [0, full, full, 0] and plan.iters.tolist() == [10, 5, 5, 13] and plan._states is None

    plan = _plan([0, full, full, 0])
    del asked[:]

    def refused_in_the_second_round(problem, **kw):
        asked.append(kw["max_active"])
        if len(asked) == 2:
            raise _refusal(_capi.ETOOLARGE)
        return _resolved(problem, full)

    monkeypatch.setattr(Bt, "solve_mpc_batch", refused_in_the_second_round)
    Bt._retry_slots_full(plan, 2, None, None, {})
    assert asked == [4, 8] and plan.status.tolist() == [0, full, full, 0]

    def fits_in_the_first_round(problem, **kw):
        return _resolved(problem)

    monkeypatch.setattr(Bt, "solve_mpc_batch", fits_in_the_first_round)
    Bt._retry_slots_full(plan, 2, None, None, {})
    assert plan.status.tolist() == [0, 0, 0, 0] and (plan.U[1] == 7.0).all() and (plan.U[3] == 3.0).all()


def test_retry_slots_full_lets_real_failures_through(monkeypatch):
    plan = _plan([0, _capi.SLOTS_FULL, _capi.SLOTS_FULL, 0])

    def stub(problem, **kw):
        raise _refusal(_capi.EWORKSPACE)

    monkeypatch.setattr(Bt, "solve_mpc_batch", stub)
    with pytest.raises(BackendError) as caught:
        Bt._retry_slots_full(plan, 2, None, None, {})
    assert caught.value.code == _capi.EWORKSPACE


class _ErrorStrings:
    """The library's texts for MPCQP_ETOOLARGE and MPCQP_EUNSUPPORTED (mpcqp_error_string, csrc/mpcqp_capi.hip)."""

    TEXT = {
        -2: b"no kernel for these dimensions (the stage-wise kernels serve nx <= 32, nu <= 8 at any horizon; the dense "
            b"HBM-resident path any system with n <= 256)",
        -6: b"option not available for these dimensions / this dtype (warm start: n <= 16, m <= 32, float64)",
    }

    def mpcqp_error_string(self, code):
        return self.TEXT[code]


def test_check_raises_the_code_with_the_message_unchanged(monkeypatch):
    monkeypatch.setattr(_capi, "load", lambda: _ErrorStrings())
    assert (_capi.ETOOLARGE, _capi.ELAYOUT, _capi.EUNSUPPORTED) == (-2, -4, -6)
    _capi.check(0, "mpcqp_build_solve_batch")
    with pytest.raises(BackendError) as caught:
        _capi.check(-2, "mpcqp_build_solve_batch")
    assert caught.value.code == -2
    assert str(caught.value) == (
        "mpcqp_build_solve_batch failed with code -2: no kernel for these dimensions (the stage-wise kernels serve nx <= 32, "
        "nu <= 8 at any horizon; the dense HBM-resident path any system with n <= 256). Served: everything that fits 160 KiB "
        "of LDS; beyond that any horizon for systems with nx <= 32, nu <= 8 (stage-wise kernels)")
    with pytest.raises(BackendError) as caught:
        _capi.check(-6, "mpcqp_solve_model_bounds_batch")
    assert caught.value.code == -6
    assert str(caught.value) == ("mpcqp_solve_model_bounds_batch failed with code -6: option not available for these "
                                 "dimensions / this dtype (warm start: n <= 16, m <= 32, float64)")
    assert BackendError("raised in Python").code is None


class _RecordingLibrary:
    """Stands in for the library: answers the size queries, records what the two launch entry points are handed."""

    def __init__(self, warm_kind=2):
        self.launches, self.warm_kind = [], warm_kind

    def mpcqp_workspace_bytes(self, dims, batch, for_solve, nbytes):
        nbytes._obj.value = 4096 * batch
        return 0

    def mpcqp_stagewise_workspace_bytes(self, dims, batch, max_active, nbytes):
        nbytes._obj.value = (10000 if max_active < 0 else 2000) + abs(max_active)  # (negative: the general kernel's)
        return 0

    def mpcqp_warm_state_bytes(self, dims, nbytes):
        nbytes._obj.value = 64
        return 0

    def mpcqp_warm_state_kind(self, dims, kind):
        kind._obj.value = self.warm_kind
        return 0

    def _record(self, entry, dims, cp, batch, opts, max_active, U, lam, status, iters, ws, ws_bytes, stream):
        d, o = dims._obj, opts._obj
        self.launches.append(dict(
            entry=entry, dims=bytes(d), problem=bytes(cp._obj), batch=batch, max_active=max_active, flags=o.flags,
            warm_start=o.warm_start, warm_shift=o.warm_shift, warm_state=o.warm_state, warm_state_bytes=o.warm_state_bytes,
            max_iter=o.max_iter, feas_tol=o.feas_tol, lam=lam is not None, ws=ws is not None, ws_bytes=ws_bytes))
        return 0

    def mpcqp_build_solve_batch(self, dims, cp, batch, opts, *rest):
        return self._record("mpcqp_build_solve_batch", dims, cp, batch, opts, None, *rest)

    def mpcqp_stagewise_solve_batch(self, dims, cp, batch, opts, max_active, *rest):
        return self._record("mpcqp_stagewise_solve_batch", dims, cp, batch, opts, max_active, *rest)


@pytest.fixture
def library(monkeypatch):
    """The constructors and the launch without a GPU: the residency check and the stream are the only things that need one."""
    lib = _RecordingLibrary()
    monkeypatch.setattr(_capi, "load", lambda: lib)
    monkeypatch.setattr(Bt, "_require_on_gpu", lambda *tensors: None)
    monkeypatch.setattr(Bt, "_stream_ptr", lambda: C.c_void_p(0))
    return lib


@pytest.mark.parametrize("request_kw, entry, ws_bytes", [
    ({}, "mpcqp_build_solve_batch", 4 * 4096),
    ({"flags": _capi.OPT_FORCE_CONDENSED}, "mpcqp_build_solve_batch", 4 * 4096),
    ({"formulation": "stagewise"}, "mpcqp_stagewise_solve_batch", 2000),
    ({"formulation": "stagewise", "max_active": 24}, "mpcqp_stagewise_solve_batch", 2024),
    ({"formulation": "stagewise", "flags": _capi.OPT_STAGE_GENERAL}, "mpcqp_stagewise_solve_batch", 10001),
    ({"formulation": "stagewise", "flags": _capi.OPT_STAGE_GENERAL, "max_active": 24}, "mpcqp_stagewise_solve_batch", 10024),
], ids=["plain", "force_condensed", "stagewise", "stagewise_slots", "stage_general", "stage_general_slots"])
def test_both_doors_hand_the_library_the_same_arguments(library, request_kw, entry, ws_bytes):
    bp = _problem()
    kw = dict(request_kw, return_multipliers=True, max_iter=77, feas_tol=1e-7)
    plan = Bt.solve_mpc_batch(bp, retry_slots=False, **kw)
    run = Bt.PreparedSolve(bp, **kw)
    run.launch()
    one_shot, prepared = library.launches
    assert one_shot == prepared
    assert one_shot["entry"] == entry and one_shot["ws_bytes"] == ws_bytes and one_shot["ws"] and one_shot["lam"]
    assert one_shot["flags"] == request_kw.get("flags", 0) and one_shot["max_active"] == (
        request_kw.get("max_active", 0) if "formulation" in request_kw else None)
    assert (one_shot["max_iter"], one_shot["feas_tol"], one_shot["warm_start"], one_shot["warm_shift"]) == (77, 1e-7, 0, 0)
    assert one_shot["batch"] == 4 and one_shot["dims"] == bytes(bp.dims()) and one_shot["problem"] == bytes(bp.c_problem())
    assert plan.U.shape == run.U.shape == (4, 16) and plan.multipliers.shape == run.lam.shape == (4, 32)
    assert plan._launch.U is plan.U  # (the plan keeps the launch, and with it the workspace, alive)


def test_a_stage_kind_warm_state_keeps_the_factor_through_prepared_solve_only(library):
    bp = _problem()
    ws = Bt.WarmState(bp)
    assert ws.kind == "stage" and ws.bytes_per_problem == 64
    Bt.solve_mpc_batch(bp, warm_state=ws)
    run = Bt.PreparedSolve(bp, warm_state=ws)
    run.launch()
    one_shot, prepared = library.launches
    assert one_shot["flags"] == 0 and prepared["flags"] == _capi.OPT_KEEP_FACTOR
    assert one_shot["warm_state"] == prepared["warm_state"] == ws.buffer.data_ptr()
    assert one_shot["warm_state_bytes"] == prepared["warm_state_bytes"] == 4 * 64
    del one_shot["flags"], prepared["flags"]
    assert one_shot == prepared
    # warm starts from such a state go through the object that keeps its workspace
    with pytest.raises(BackendError, match="warm-starts through PreparedSolve") as caught:
        Bt.solve_mpc_batch(bp, warm_state=ws, warm_start=True)
    assert caught.value.code is None and len(library.launches) == 2
    run.set_warm_start(True)
    run.launch()
    assert library.launches[2]["flags"] == _capi.OPT_REUSE_FACTOR and library.launches[2]["warm_start"] == _capi.WARM_OPERATOR
    # asked for at construction: the first launch keeps the factor and starts cold, the next ones re-use it
    run = Bt.PreparedSolve(bp, warm_state=ws, warm_start=True)
    run.launch()
    run.launch()
    first, second = library.launches[3:]
    assert first["flags"] == _capi.OPT_KEEP_FACTOR and second["flags"] == _capi.OPT_REUSE_FACTOR


def test_solve_mpc_batch_keeps_its_own_rules(library):
    with pytest.raises(BackendError, match="not a batched backend"):
        Bt.solve_mpc_batch(_problem(), solver="quadprog")
    assert not library.launches
