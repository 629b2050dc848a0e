"""Model and weight tangents of plans without a GPU: the NumPy restatement (tests/tangent_model_np.py) by its duality
with the VJP restatements (tests/adjoint_np.py, tests/adjoint_model_np.py) and against central differences of the C
oracle's solve along a joint tangent of every operand, the stage-wise restatement (tests/tangent_model_stagewise_np.py)
against it, and the C exports and Python surface of the feature."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import adjoint_model_np as AM
import adjoint_np as AN
import tangent_model_np as TM
import tangent_model_stagewise_np as TMS
import tangent_np as TN
from host_helpers import _dims, _header, _lib, _ltv
from qpmpc_amd import _capi
from qpmpc_amd import workloads as W


EXPORTS = ("mpcqp_plan_jvp_model_workspace_bytes", "mpcqp_plan_jvp_model_batch",
           "mpcqp_plan_jvp_model_stagewise_workspace_bytes", "mpcqp_plan_jvp_model_stagewise_batch")
EINVAL, EDTYPE, EWORKSPACE, EUNSUPPORTED = -1, -3, _capi.EWORKSPACE, -6


def _p_only():
    w = _ltv(11, 10, 3, 2, 5, 2)
    w["goal"], w["targets"] = None, None
    w["e"] = w["e"].copy()
    w["e"][:, ::2, 0] -= 0.6  # (without a q term the plan is zero unless a row pushes it: these do)
    return w


def _without(key, seed):
    w = _ltv(seed, 6, 3, 2, 30, 3)
    w[key] = None
    return w


def _absent_too(w1, tan, rng, mk):
    """The tangent of a C or D the problem does not have: the tangent at zero, as the VJP has the gradient at zero."""
    N = int(w1["N"])
    nx, nu = np.asarray(w1["x0"]).shape[-1], np.asarray(w1["B"]).shape[-1]
    for key, shp in (("C", (N, mk, nx)), ("D", (N, mk, nu))):
        if key not in tan and mk:
            tan[key] = rng.standard_normal(shp)
    return tan


@pytest.mark.parametrize("make", [lambda: W.triple_integrator_batch(6), lambda: _ltv(21, 6, 4, 2, 8, 3),
                                  lambda: W.wip_batch(4, N=20), _p_only, lambda: _without("C", 51),
                                  lambda: _without("D", 52)])
def test_duality_with_the_vjp_restatements(make):
    """<gU, dU> + <gX, dX> = sum over operands of <gradient, tangent> on every solved problem."""
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
        tan = _absent_too(w1, TM.random_model_tangent(w1, rng, lam.size), rng, lam.size // N)
        fwd = TM.jvp_model(w1, U, lam, tan)
        lhs = gU @ fwd["U"] + gX @ fwd["X"]
        rhs = TM.pairing(tan, AN.vjp(w1, lam, gU, gX), AM.model_vjp(w1, U, lam, gU, gX))
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs), abs(rhs)), (b, lhs, rhs)
        checked += 1
    assert checked >= 3


def test_without_model_tangents_it_is_the_state_tangent():
    w = _ltv(21, 6, 4, 2, 8, 3)
    rng = np.random.default_rng(4)
    for b in range(3):
        w1 = AN.single(w, b)
        U, lam, _, st = AN.solve(w1)
        assert st == 0
        tan = TN.random_tangent(w1, rng)
        ref, got = TN.jvp(w1, lam, tan), TM.jvp_model(w1, U, lam, tan)
        for key in ("U", "X"):
            assert np.abs(got[key] - ref[key]).max() <= 1e-12 * max(1.0, np.abs(ref[key]).max())


def _check_against_fd(w, rng, need, bound):
    """Central differences of the C oracle along a joint random tangent of every operand, on strictly complementary
    problems."""
    checked, worst = 0, 0.0
    for b in range(np.asarray(w["x0"]).shape[0]):
        w1 = AN.single(w, b)
        U, lam, slack, st = AN.solve(w1)
        if st != 0 or not AN.strictly_complementary(lam, slack):
            continue
        tan = TM.random_model_tangent(w1, rng, lam.size)
        an = TM.jvp_model(w1, U, lam, tan)
        fd = TM.fd_jvp_model(w1, tan)
        for key in ("U", "X"):
            err = np.abs(fd[key] - an[key]).max() / max(1.0, np.abs(an[key]).max())
            worst = max(worst, err)
            assert err <= bound, (b, key, err)
        checked += 1
        if checked == need:
            print(f"central differences: worst {worst:.3e} (bound {bound:.0e})")
            return
    raise AssertionError(f"only {checked} strictly complementary problems")


def test_finite_differences_random_ltv():
    w = _ltv(11, 10, 3, 2, 5, 2)  # input rows (D), state rows (C), stage and terminal cost
    assert w["D"] is not None and w["C"] is not None and w["wx"] > 0 and w["targets"] is not None
    _check_against_fd(w, np.random.default_rng(12), need=6, bound=1e-6)


# The triple integrator and the pendulum: the error is the truncation and cancellation error of the difference quotient
# (step 1e-6 on stiff plans), not the restatement's, whose duality above holds to 1e-10. Measured with these seeds: 6.4e-6
# (triple integrator) and 3.8e-7 (pendulum); other draws gave 3.3e-7 .. 1.8e-6 and 4.7e-7 .. 7e-7. The bound is the 1e-5
# ceiling these two families' difference quotients are given.
FD_BOUND_STIFF = 1e-5


def test_finite_differences_p_only():
    w = _p_only()
    assert sum(np.abs(AN.solve(AN.single(w, b))[0]).max() > 0.1 for b in range(10)) >= 5
    _check_against_fd(w, np.random.default_rng(13), need=6, bound=1e-6)


def test_finite_differences_triple_integrator():
    _check_against_fd(W.triple_integrator_batch(12), np.random.default_rng(7), need=4, bound=FD_BOUND_STIFF)


def test_finite_differences_wip():
    _check_against_fd(W.wip_batch(8, N=20), np.random.default_rng(8), need=2, bound=FD_BOUND_STIFF)


# ---------------------------------------------------------------- the stage-wise restatement

def _tangents(w1, rng, mk):
    """Each of the new tangents alone, then every operand's together."""
    full = _absent_too(w1, TM.random_model_tangent(w1, rng, mk * int(w1["N"])), rng, mk)
    return [{k: full[k]} for k in TM.MODEL_KEYS if k in full] + [full]


def _compare(w, rng, need):
    checked = 0
    for b in range(np.asarray(w["x0"]).shape[0]):
        w1 = AN.single(w, b)
        U, lam, _, st = AN.solve(w1)
        if st != 0:
            continue
        fac = TMS.ModelFactorisation(w1, U, lam)
        assert fac.status == 0
        for tan in _tangents(w1, rng, lam.size // int(w["N"])):
            ref, sw = TM.jvp_model(w1, U, lam, tan), fac.jvp_model(tan)
            for key in ("U", "X"):
                err = np.abs(sw[key] - ref[key]).max()
                assert err <= 1e-9 * max(1.0, np.abs(ref[key]).max()), (b, sorted(tan), key, err)
        checked += 1
        if checked == need:
            return
    raise AssertionError(f"only {checked} solved problems")


@pytest.mark.parametrize("nx,nu,N,mk", [(3, 2, 8, 2), (4, 2, 40, 3), (3, 2, 150, 2)])
def test_stagewise_random_ltv(nx, nu, N, mk):
    _compare(_ltv(40 + N, 6, nx, nu, N, mk), np.random.default_rng(N), need=2)


def test_stagewise_wip_n200():
    _compare(W.wip_batch(4, N=200, sampling_period=0.005), np.random.default_rng(5), need=2)


def test_stagewise_c_only_rows_at_step_0():
    w = W.triple_integrator_batch(8)
    assert w["D"] is None
    _compare(w, np.random.default_rng(8), need=3)


def test_stagewise_q_flag_combinations():
    from oracle.capi import FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
    from qpmpc_amd.workloads import problem_from_workload

    seen = set()
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


# ---------------------------------------------------------------- public surface

def test_exports_declared_bound_and_built():
    declared = set(re.findall(r"(mpcqp_[a-z_]+)\(", _header()))
    lib = _lib()
    for name in EXPORTS:
        assert name in declared
        assert name in _capi.EXPORTS
        assert hasattr(lib, name)
    assert "typedef struct MpcqpModelTangents" in _header()
    assert [f for f, _ in _capi.ModelTangents._fields_] == ["dA", "dB", "dC", "dD", "dw", "dA_stride", "dB_stride",
                                                            "dC_stride", "dD_stride", "dw_stride"]
    assert [f for f, _ in _capi.Tangents._fields_] == ["dx0", "dgoal", "dtargets", "de", "dx0_stride", "dgoal_stride",
                                                       "dtargets_stride", "de_stride"]
    assert _capi.ABI_VERSION == 12 and lib.mpcqp_abi_version() == 12
    assert "#define MPCQP_ABI_VERSION 12" in _header()


def _query(dims, batch, ntan):
    nbytes = C.c_size_t(0)
    rc = _lib().mpcqp_plan_jvp_model_workspace_bytes(C.byref(dims), batch, ntan, C.byref(nbytes))
    return rc, nbytes.value


def _query_sw(dims, batch, max_active, ntan):
    nbytes = C.c_size_t(0)
    rc = _lib().mpcqp_plan_jvp_model_stagewise_workspace_bytes(C.byref(dims), batch, max_active, ntan, C.byref(nbytes))
    return rc, nbytes.value


def test_workspace_queries():
    assert _query(_dims(3, 1, 16, 2, dtype=_capi.F32), 8, 3)[0] == EDTYPE
    assert _query(_dims(3, 2, 65, 2), 8, 3)[0] == EUNSUPPORTED  # n = 130
    assert _query(_dims(3, 1, 16, 2), 8, 0)[0] == EINVAL
    assert _query(_dims(3, 1, 16, 2), 8, 257)[0] == EINVAL
    assert _lib().mpcqp_plan_jvp_model_workspace_bytes(C.byref(_dims(3, 1, 16, 2)), 8, 3, None) == EINVAL
    rc, small = _query(_dims(3, 1, 16, 2), 8, 3)
    old = C.c_size_t(0)
    assert _lib().mpcqp_plan_jvp_workspace_bytes(C.byref(_dims(3, 1, 16, 2)), 8, 3, C.byref(old)) == 0
    assert rc == 0 and small == old.value > 0  # both carves in LDS: the condensed segments alone
    # n = 128, 5 tangents: the carve is in the workspace and longer by X, Z, pi and the tangents' zs
    rc, big = _query(_dims(4, 2, 64, 2), 8, 5)
    assert _lib().mpcqp_plan_jvp_workspace_bytes(C.byref(_dims(4, 2, 64, 2)), 8, 5, C.byref(old)) == 0
    assert rc == 0 and big + 256 >= old.value + 8 * 8 * (3 + 5) * 65 * 4  # (segments are rounded up to 256 bytes)
    assert _query(_dims(3, 1, 16, 2), 0, 3) == (0, 0)
    # stage-wise: the envelope of the stage-wise tangent, any horizon
    assert _query_sw(_dims(3, 2, 70, 2, dtype=_capi.F32), 1, 4, 1)[0] == EDTYPE
    assert _query_sw(_dims(33, 2, 10, 2), 1, 4, 1)[0] == EUNSUPPORTED
    assert _query_sw(_dims(3, 2, 10, 2), 1, 4, 0)[0] == EINVAL
    assert _query_sw(_dims(3, 2, 10, 2), 1, 4, 257)[0] == EINVAL
    assert _query_sw(_dims(3, 2, 10, 2), 1, -1, 1)[0] == EINVAL
    rc, sw = _query_sw(_dims(3, 2, 70, 2), 8, 16, 3)
    assert _lib().mpcqp_plan_jvp_stagewise_workspace_bytes(C.byref(_dims(3, 2, 70, 2)), 8, 16, 3, C.byref(old)) == 0
    assert rc == 0 and sw + 256 >= old.value + 8 * 8 * (3 + 3) * 71 * 3  # (both sizes are rounded up to 256 bytes)
    assert _query_sw(_dims(3, 2, 70, 2), 0, 16, 3) == (0, 0)


@pytest.mark.parametrize("stagewise", [False, True])
def test_batch_argument_checks_in_order(stagewise):
    """Every call below is refused before anything is launched: the pointers are NULL or dummies."""
    lib = _lib()
    fn = lib.mpcqp_plan_jvp_model_stagewise_batch if stagewise else lib.mpcqp_plan_jvp_model_batch
    N = 70 if stagewise else 16

    def call(dims, prob, batch, ntan, lam, status, U, tan, mtan, dU=None, ws=None, nbytes=0, ka=8):
        head = (C.byref(dims), C.byref(prob), batch) + ((ka,) if stagewise else ()) + (ntan,)
        ref = lambda s: None if s is None else C.byref(s)  # noqa: E731
        return fn(*head, lam, status, U, ref(tan), ref(mtan), dU, None, None, ws, nbytes, None)

    d = _dims(3, 2, N, 2)
    prob, tan, mtan = _capi.Problem(), _capi.Tangents(), _capi.ModelTangents()
    # dims first: dtype, envelope, then ntan
    assert call(_dims(3, 2, N, 2, _capi.F32), prob, 4, 0, None, None, None, None, None) == EDTYPE
    unsupported = _dims(33, 2, N, 2) if stagewise else _dims(3, 2, 65, 2)
    assert call(unsupported, prob, 4, 0, None, None, None, None, None) == EUNSUPPORTED
    assert call(d, prob, 4, 0, None, None, None, tan, mtan) == EINVAL
    assert call(d, prob, 4, 257, None, None, None, tan, mtan) == EINVAL
    # then the problem's operands (an empty MpcqpProblem is refused), then the export's own pointers
    assert call(d, prob, 4, 1, None, None, None, tan, mtan) != 0
    good = _capi.Problem()
    for name, _ in _capi.Problem._fields_:
        setattr(good, name, _capi.Operand(8, 0, 0))  # dummy addresses: nothing is launched
    tan.dx0 = 8
    mtan.dA = 8
    assert call(d, good, 4, 1, 8, 8, 8, None, None, dU=8) == EINVAL                 # tan and mtan both NULL
    assert call(d, good, 4, 1, 8, 8, 8, _capi.Tangents(), _capi.ModelTangents(), dU=8) == EINVAL  # no tangent in them
    assert call(d, good, 4, 1, 8, None, 8, tan, mtan, dU=8) == EINVAL               # status
    assert call(d, good, 4, 1, 8, 8, None, tan, mtan, dU=8) == EINVAL               # U
    assert call(d, good, 4, 1, 8, 8, 8, tan, mtan) == EINVAL                        # dU
    assert call(d, good, 4, 1, None, 8, 8, tan, mtan, dU=8) == EINVAL               # lam, mk > 0
    neg = _capi.ModelTangents()
    neg.dw, neg.dw_stride = 8, -1
    assert call(d, good, 4, 1, 8, 8, 8, tan, neg, dU=8) == EINVAL
    # either structure alone is enough
    assert call(d, good, 4, 1, 8, 8, 8, tan, None, dU=8) == EWORKSPACE
    assert call(d, good, 4, 1, 8, 8, 8, None, mtan, dU=8) == EWORKSPACE
    assert call(d, good, 4, 1, 8, 8, 8, tan, mtan, dU=8, ws=8, nbytes=64) == EWORKSPACE  # short
    assert call(d, good, 0, 1, 8, 8, 8, tan, mtan, dU=8) == 0  # empty batch: nothing to do


def test_keywords_of_the_python_surface():
    from qpmpc_amd import autodiff, plan_jvp

    names = autodiff.MODEL_OPERANDS + autodiff.WEIGHTS
    prm = inspect.signature(plan_jvp).parameters
    for name in names:
        assert prm[name].kind is inspect.Parameter.KEYWORD_ONLY and prm[name].default is None
    assert autodiff.JACOBIAN_WRT == ("initial_state", "goal_state", "cost_weights")


def test_shape_errors_raise_before_any_launch():
    torch = pytest.importorskip("torch")
    from qpmpc_amd import ProblemDefinitionError, plan_jacobian, plan_jvp
    from qpmpc_amd.batch import BatchPlan

    w = _ltv(60, 2, 3, 2, 5, 2)
    bp = W.to_batch_problem(w, device="cpu")
    plan = BatchPlan(bp, torch.zeros(2, 10, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), None,
                     multipliers=torch.zeros(2, 10, dtype=torch.float64))
    z = lambda *shape: torch.zeros(*shape, dtype=torch.float64)  # noqa: E731
    bad = dict(transition_state_matrix=z(2, 1, 5, 3, 2), transition_input_matrix=z(2, 1, 4, 3, 2),
               ineq_state_matrix=z(3, 1, 5, 2, 3), ineq_input_matrix=z(2, 1, 5, 2), terminal_cost_weight=z(2, 1, 1),
               stage_state_cost_weight=z(3, 1), stage_input_cost_weight=z(2))
    for name, t in bad.items():
        with pytest.raises(ProblemDefinitionError, match=name):
            plan_jvp(bp, plan, **{name: t})
    with pytest.raises(ProblemDefinitionError, match="disagree on T"):
        plan_jvp(bp, plan, initial_state=z(1, 2, 3), transition_state_matrix=z(1, 3, 1, 3, 3))
    with pytest.raises(ProblemDefinitionError, match="disagree on T"):
        plan_jvp(bp, plan, terminal_cost_weight=z(1, 2), stage_input_cost_weight=z(1, 3))
    with pytest.raises(ProblemDefinitionError, match="at most 256"):
        plan_jvp(bp, plan, stage_input_cost_weight=z(1, 257))
    with pytest.raises(ProblemDefinitionError, match="wrt"):
        plan_jacobian(bp, plan, wrt="model")
    # wrt="cost_weights" is accepted: it gets as far as the launch, which needs a GPU
    from qpmpc_amd import BackendError

    with pytest.raises(BackendError):
        plan_jacobian(bp, plan, wrt="cost_weights")
