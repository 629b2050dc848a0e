"""The stage-wise tangent without a GPU: the NumPy restatement (tests/tangent_stagewise_np.py, on the whitened Riccati
recursion) against the dense KKT restatement (tests/tangent_np.py) at 1e-9 relative, its duality with the stage-wise
adjoint's restatement, central differences of the C oracle beyond n = 128, the Riccati gain, and the C exports and Python
surface of the feature."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import adjoint_np as AN
import adjoint_stagewise_np as AS
import tangent_np as TN
import tangent_stagewise_np as TS
from host_helpers import _dims, _header, _lib, _ltv
from qpmpc_amd import _capi
from qpmpc_amd import workloads as W


EXPORTS = ("mpcqp_plan_jvp_stagewise_workspace_bytes", "mpcqp_plan_jvp_stagewise_batch")
EINVAL, EDTYPE, EWORKSPACE, EUNSUPPORTED = -1, -3, _capi.EWORKSPACE, -6


def _tangents(w1, rng):
    """Each of the problem's tangents alone, then all together."""
    full = TN.random_tangent(w1, rng)
    return [{k: v} for k, v in full.items()] + [full]


def _compare(w, rng, need):
    """Solved problems of ``w`` (C oracle): dU and dX of the stage-wise restatement equal the dense KKT solve's, for
    each tangent alone and all together."""
    checked = 0
    for b in range(np.asarray(w["x0"]).shape[0]):
        w1 = AN.single(w, b)
        _, lam, _, st = AN.solve(w1)
        if st != 0:
            continue
        fac = TS.Factorisation(w1, lam)
        assert fac.status == 0
        for tan in _tangents(w1, rng):
            ref, sw = TN.jvp(w1, lam, tan), fac.jvp(tan)
            for key in ("U", "X"):  # (with and without dX: U is checked on its own)
                err = np.abs(sw[key] - ref[key]).max()
                assert err <= 1e-9 * max(1.0, np.abs(ref[key]).max()), (b, sorted(tan), key, err)
        checked += 1
        if checked == need:
            return
    raise AssertionError(f"only {checked} solved problems")


@pytest.mark.parametrize("nx,nu,N,mk", [(3, 2, 8, 2), (4, 2, 40, 3), (6, 3, 60, 2), (3, 2, 150, 2)])
def test_random_ltv(nx, nu, N, mk):
    _compare(_ltv(40 + N, 6, nx, nu, N, mk), np.random.default_rng(N), need=2)


def test_wip_n200():
    # (T = 0.005 s: at longer periods the condensed restatement itself loses digits on N = 200)
    _compare(W.wip_batch(4, N=200, sampling_period=0.005), np.random.default_rng(5), need=2)


def test_without_C_and_without_D():
    w = _ltv(51, 6, 3, 2, 30, 3)
    w["C"] = None
    _compare(w, np.random.default_rng(6), need=2)
    w = _ltv(52, 6, 3, 2, 30, 3)
    w["D"] = None
    _compare(w, np.random.default_rng(7), need=2)


def test_c_only_rows_at_step_0():
    w = W.triple_integrator_batch(8)  # C-only rows at every step (G rows of step 0 are zero: Psi_0 = 0)
    assert w["D"] is None
    _compare(w, np.random.default_rng(8), need=3)


def test_q_flag_combinations():
    from oracle.capi import FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
    from qpmpc_amd.workloads import problem_from_workload

    seen = set()
    # (targets without a goal enter no q term, a quirk of the reference; a zero terminal weight leaves the stage term alone)
    for goal, targets, wt in ((True, True, None), (True, False, None), (False, True, None), (False, False, None),
                              (True, True, 0.0)):
        w = _ltv(53, 6, 3, 2, 20, 2)
        if wt is not None:
            w["wt"] = wt
        if not goal:
            w["goal"] = None
        if not targets:
            w["targets"] = None
        seen.add(flags_of(problem_from_workload(AN.single(w, 0), 0)) & (FLAG_Q_STAGE | FLAG_Q_TERMINAL))
        _compare(w, np.random.default_rng(9), need=2)
    assert seen == {0, FLAG_Q_STAGE, FLAG_Q_TERMINAL, FLAG_Q_STAGE | FLAG_Q_TERMINAL}


def test_degenerate_multipliers_are_not_pd():
    w = _ltv(54, 1, 3, 2, 6, 2)
    w["C"][0, 3, 1], w["D"][0, 3, 1] = 0.0, 0.0
    lam = np.zeros(12)
    lam[3 * 2 + 1] = 1.0
    out = TS.stagewise_jvp(AN.single(w, 0), lam, {"x0": np.ones(3)})
    assert out["status"] == TS.NOT_PD and not out["U"].any() and not out["X"].any()
    w = _ltv(55, 1, 3, 1, 6, 4)  # n = 6 < m = 24 rows all active
    assert TS.stagewise_jvp(AN.single(w, 0), np.ones(24), {"x0": np.ones(3)})["status"] == TS.NOT_PD


@pytest.mark.parametrize("make", [lambda: W.triple_integrator_batch(6), lambda: _ltv(21, 6, 4, 2, 8, 3),
                                  lambda: _ltv(22, 4, 3, 2, 70, 2), lambda: W.wip_batch(4, N=20)])
def test_duality_with_the_stagewise_vjp(make):
    w = make()
    rng = np.random.default_rng(3)
    N = int(w["N"])
    checked = 0
    for b in range(np.asarray(w["x0"]).shape[0]):
        w1 = AN.single(w, b)
        U, lam, _, st = AN.solve(w1)
        if st != 0:
            continue
        nx = w1["x0"].shape[1]
        gU, gX = rng.standard_normal(U.size), rng.standard_normal((N + 1) * nx)
        tan = TN.random_tangent(w1, rng)
        fwd = TS.stagewise_jvp(w1, lam, tan)
        g = AS.stagewise_vjp(w1, lam, gU, gX)
        assert fwd["status"] == 0 and g["status"] == 0
        lhs = gU @ fwd["U"] + gX @ fwd["X"]
        rhs = sum(float(np.asarray(g[k]).ravel() @ tan[k]) for k in tan)
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs), abs(rhs)), (b, lhs, rhs)
        checked += 1
    assert checked >= 3


def _active_set(w1):
    return set(np.flatnonzero(AN.solve(w1)[1] > 0.0))


def test_finite_differences_beyond_128_variables():
    """n = 140 > 128: central differences of the C oracle's solve at tangent_np's 1e-6, on problems that are strictly
    complementary and whose active set is the same at both ends of the difference step (checked here)."""
    w = _ltv(71, 8, 3, 2, 70, 2)
    rng = np.random.default_rng(72)
    step, checked = 1e-6, 0
    for b in range(8):
        w1 = AN.single(w, b)
        U, lam, slack, st = AN.solve(w1)
        if st != 0 or not AN.strictly_complementary(lam, slack) or not (lam > 0).any():
            continue
        tan = TN.random_tangent(w1, rng)
        ends = []
        for s in (step, -step):
            w2 = dict(w1)
            for key, d in tan.items():
                base = np.asarray(w1[key], dtype=float)
                w2[key] = base + s * np.asarray(d).reshape(base.shape)
            ends.append(_active_set(w2))
        assert ends[0] == ends[1] == set(np.flatnonzero(lam > 0.0)), b
        an = TS.stagewise_jvp(w1, lam, tan)
        fd = TN.fd_jvp(w1, tan, step)
        for key in ("U", "X"):
            err = np.abs(fd[key] - an[key]).max() / max(1.0, np.abs(an[key]).max())
            assert err <= 1e-6, (b, key, err)
        checked += 1
    assert checked >= 2


def test_no_active_row_first_step_jacobian_is_the_riccati_gain_n256():
    from oracle.stagewise_np import Riccati, from_mpc_problem
    from qpmpc_amd.workloads import problem_from_workload

    N, nx, nu = 256, 3, 2
    w = _ltv(31, 2, nx, nu, N, 2)
    for b in range(2):
        w1 = AN.single(w, b)
        fac = TS.Factorisation(w1, np.zeros(N * 2))  # no active row
        J = np.stack([fac.jvp({"x0": np.eye(nx)[j]})["U"] for j in range(nx)], axis=1)  # [n, nx]
        K0 = Riccati(from_mpc_problem(problem_from_workload(w1, 0))).K[0]
        np.testing.assert_allclose(J[:nu], -K0, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(K0).max()))


# ---------------------------------------------------------------- public surface

def test_exports_declared_bound_and_built():
    declared = set(re.findall(r"(mpcqp_[a-z_]+)\(", _header()))
    lib = _lib()
    for name in EXPORTS:
        assert name in declared
        assert name in _capi.EXPORTS
        assert hasattr(lib, name)
    assert _capi.ABI_VERSION == 12 and lib.mpcqp_abi_version() == 12
    assert "#define MPCQP_ABI_VERSION 12" in _header()


def _query(dims, batch, max_active, ntan):
    nbytes = C.c_size_t(0)
    rc = _lib().mpcqp_plan_jvp_stagewise_workspace_bytes(C.byref(dims), batch, max_active, ntan, C.byref(nbytes))
    return rc, nbytes.value


def test_workspace_query():
    rc, b140 = _query(_dims(3, 2, 70, 2), 8, 16, 3)  # n = 140: beyond the condensed tangent
    assert rc == 0 and b140 > 0
    cond = C.c_size_t(0)
    assert _lib().mpcqp_plan_jvp_workspace_bytes(C.byref(_dims(3, 2, 70, 2)), 8, 3, C.byref(cond)) == EUNSUPPORTED
    rc, b1024 = _query(_dims(3, 1, 1024, 4), 2, 64, 3)
    assert rc == 0 and b1024 > 0
    sizes = [_query(_dims(12, 4, 64, 16), 4, k, 12)[1] for k in (0, 8, 63, 64, 200)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    # 256 / max(nx, nu) = 21 tangents run side by side: the scratch grows up to one pass of them, not beyond
    sizes = [_query(_dims(12, 4, 64, 16), 4, 8, t)[1] for t in (1, 2, 12, 21, 22, 256)]
    assert all(a < b for a, b in zip(sizes[:4], sizes[1:4])) and sizes[3] == sizes[4] == sizes[5], sizes
    # ... and less than the stage-wise adjoint's region plus one pass of xs and mu
    adj = C.c_size_t(0)
    assert _lib().mpcqp_plan_vjp_stagewise_workspace_bytes(C.byref(_dims(12, 4, 64, 16)), 4, 8, C.byref(adj)) == 0
    assert sizes[-1] <= adj.value + 4 * 8 * 21 * (65 * 12 + 9) + 256
    assert _query(_dims(12, 4, 64, 16), 0, 8, 4) == (0, 0)
    assert _lib().mpcqp_plan_jvp_stagewise_workspace_bytes(C.byref(_dims(3, 2, 70, 2)), 8, 16, 3, None) == EINVAL


def test_workspace_query_envelope():
    assert _query(_dims(3, 2, 70, 2, dtype=_capi.F32), 1, 4, 1)[0] == EDTYPE
    assert _query(_dims(33, 2, 10, 2), 1, 4, 1)[0] == EUNSUPPORTED
    assert _query(_dims(3, 9, 10, 2), 1, 4, 1)[0] == EUNSUPPORTED
    assert _query(_dims(32, 8, 10, 2), 1, 4, 1)[0] == 0
    assert _query(_dims(3, 2, 10, 2), 1, -1, 1)[0] == EINVAL
    assert _query(_dims(3, 2, 10, 2), -1, 4, 1)[0] == EINVAL
    assert _query(_dims(3, 2, 10, 2), 1, 4, 0)[0] == EINVAL
    assert _query(_dims(3, 2, 10, 2), 1, 4, 257)[0] == EINVAL
    assert _query(_dims(3, 2, 10, 2), 1, 4, 256)[0] == 0


def test_batch_argument_checks_in_order():
    """Every call below is refused before anything is launched: the pointers are NULL or dummies."""
    lib = _lib()
    call = lib.mpcqp_plan_jvp_stagewise_batch
    d = _dims(3, 2, 70, 2)
    prob, tan = _capi.Problem(), _capi.Tangents()
    nul = (None,) * 3

    def rest(dU=None, ws=None, nbytes=0):  # dU, dX, jvp_status, workspace, bytes, stream
        return (dU, None, None, ws, nbytes, None)

    # dims first: dtype, envelope, then ntan
    assert call(C.byref(_dims(3, 2, 70, 2, _capi.F32)), C.byref(prob), 4, 8, 0, *nul, *rest()) == EDTYPE
    assert call(C.byref(_dims(33, 2, 70, 2)), C.byref(prob), 4, 8, 0, *nul, *rest()) == EUNSUPPORTED
    assert call(C.byref(d), C.byref(prob), 4, -1, 1, *nul, *rest()) == EINVAL
    assert call(C.byref(d), C.byref(prob), 4, 8, 0, None, None, C.byref(tan), *rest()) == EINVAL
    assert call(C.byref(d), C.byref(prob), 4, 8, 257, None, None, C.byref(tan), *rest()) == EINVAL
    # then the problem's operands (an empty MpcqpProblem is refused), then the export's own pointers
    assert call(C.byref(d), C.byref(prob), 4, 8, 1, None, None, C.byref(tan), *rest()) != 0
    good = _capi.Problem()
    for name, _ in _capi.Problem._fields_:
        setattr(good, name, _capi.Operand(8, 0, 0))  # dummy addresses: nothing is launched
    assert call(C.byref(d), C.byref(good), 4, 8, 1, 8, 8, None, *rest(8)) == EINVAL          # tan
    assert call(C.byref(d), C.byref(good), 4, 8, 1, 8, None, C.byref(tan), *rest(8)) == EINVAL  # status
    assert call(C.byref(d), C.byref(good), 4, 8, 1, 8, 8, C.byref(tan), *rest()) == EINVAL    # dU
    assert call(C.byref(d), C.byref(good), 4, 8, 1, None, 8, C.byref(tan), *rest(8)) == EINVAL  # lam, mk > 0
    neg = _capi.Tangents()
    neg.dgoal_stride = -1
    assert call(C.byref(d), C.byref(good), 4, 8, 1, 8, 8, C.byref(neg), *rest(8)) == EINVAL
    assert call(C.byref(d), C.byref(good), 4, 8, 1, 8, 8, C.byref(tan), *rest(8)) == EWORKSPACE  # no workspace
    assert call(C.byref(d), C.byref(good), 4, 8, 1, 8, 8, C.byref(tan), *rest(8, 8, 64)) == EWORKSPACE  # short
    assert call(C.byref(d), C.byref(good), 0, 8, 1, 8, 8, C.byref(tan), *rest(8)) == 0  # empty batch: nothing to do


def test_keywords_are_keyword_only_with_condensed_defaults():
    from qpmpc_amd import autodiff, plan_jacobian, plan_jvp, solve_mpc_batch_diff

    for fn, name in ((plan_jvp, "formulation"), (plan_jacobian, "formulation"), (solve_mpc_batch_diff, "tangent")):
        prm = inspect.signature(fn).parameters[name]
        assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default == "condensed"
    assert autodiff.FORMULATIONS == ("condensed", "stagewise")


def test_bad_keywords_and_envelopes_raise_before_any_launch():
    torch = pytest.importorskip("torch")
    from torch.autograd import forward_ad as fwAD

    from qpmpc_amd import BackendError, autodiff, plan_jacobian, plan_jvp, solve_mpc_batch_diff
    from qpmpc_amd.batch import BatchPlan

    w = _ltv(60, 2, 3, 2, 5, 2)
    bp = W.to_batch_problem(w, device="cpu")
    plan = BatchPlan(bp, torch.zeros(2, 10, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), None,
                     multipliers=torch.zeros(2, 10, dtype=torch.float64))
    dx = torch.zeros(1, 1, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="formulation"):
        plan_jvp(bp, plan, initial_state=dx, formulation="dense")
    with pytest.raises(ValueError, match="formulation"):
        plan_jacobian(bp, plan, formulation="riccati")
    with pytest.raises(ValueError, match="tangent"):
        solve_mpc_batch_diff(bp, tangent="dense")
    # the envelope of the stage-wise tangent: nx <= 32, nu <= 8, any horizon
    wide = W.to_batch_problem(_ltv(61, 1, 33, 2, 3, 1), device="cpu")
    with pytest.raises(BackendError, match="nx <= 32"):
        autodiff.check_envelope(wide, "jvp_stagewise")
    wplan = BatchPlan(wide, None, None, None, multipliers=torch.zeros(1, 3, dtype=torch.float64))
    with pytest.raises(BackendError, match="nx <= 32"):
        plan_jvp(wide, wplan, initial_state=torch.zeros(1, 1, 33, dtype=torch.float64), formulation="stagewise")
    with pytest.raises(BackendError):
        autodiff.check_envelope(W.to_batch_problem(_ltv(62, 1, 3, 9, 3, 1), device="cpu"), "jvp_stagewise")
    autodiff.check_envelope(W.to_batch_problem(_ltv(63, 1, 3, 2, 500, 1), device="cpu"), "jvp_stagewise")
    # the default formulation still stops at n = 128, and now says where to go
    big = W.to_batch_problem(_ltv(63, 1, 3, 2, 70, 2), device="cpu")
    bplan = BatchPlan(big, None, None, None, multipliers=torch.zeros(1, 140, dtype=torch.float64))
    with pytest.raises(BackendError, match="128") as info:
        plan_jvp(big, bplan, initial_state=dx)
    assert 'formulation="stagewise"' in str(info.value)
    with pytest.raises(BackendError, match="128"):
        plan_jacobian(big, bplan)
    # forward AD: without tangent= everything that raised keeps raising; the stagewise message names the keyword
    x0 = torch.as_tensor(w["x0"])
    with fwAD.dual_level():
        d0 = fwAD.make_dual(x0, torch.ones_like(x0))
        with pytest.raises(BackendError, match="stagewise") as info:
            solve_mpc_batch_diff(bp, initial_state=d0, adjoint="stagewise")
        assert 'tangent="stagewise"' in str(info.value)
        A = torch.as_tensor(w["A"])
        with pytest.raises(BackendError, match="transition_state_matrix"):
            solve_mpc_batch_diff(bp, transition_state_matrix=fwAD.make_dual(A, torch.ones_like(A)), tangent="stagewise")
        x1 = torch.as_tensor(_ltv(63, 1, 3, 2, 70, 2)["x0"])
        with pytest.raises(BackendError, match="128"):
            solve_mpc_batch_diff(big, initial_state=fwAD.make_dual(x1, torch.ones_like(x1)))
        xw = torch.as_tensor(_ltv(61, 1, 33, 2, 3, 1)["x0"])
        with pytest.raises(BackendError, match="nx <= 32"):
            solve_mpc_batch_diff(wide, initial_state=fwAD.make_dual(xw, torch.ones_like(xw)), tangent="stagewise")
