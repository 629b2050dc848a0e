"""Model and cost gradients of plans, without a GPU: the NumPy restatement (tests/adjoint_model_np.py) against central
finite differences of the C oracle's solve for every entry of A, B, C, D and the three weights, on strictly complementary
problems; and the C exports and Python surface of the feature."""
import inspect

import numpy as np

import adjoint_model_np as AM
import adjoint_np as AN
from qpmpc_amd import _capi
from qpmpc_amd import workloads as W


def _ltv(seed, B, nx=3, nu=2, N=5, mk=2):
    from qpmpc_amd.workloads import random_ltv

    return random_ltv(np.random.default_rng(seed), B, nx, nu, N, mk, 1.0)


def _check_against_fd(w, rng, need, with_gX=True):
    N = int(w["N"])
    checked = 0
    for b in range(np.asarray(w["x0"]).shape[0]):
        w1 = AN.single(w, b)
        U, lam, slack, st = AN.solve(w1)
        if st != 0 or not AN.strictly_complementary(lam, slack):
            continue
        nx = w1["x0"].shape[1]
        gU = rng.standard_normal(U.size)
        gX = rng.standard_normal((N + 1) * nx) if with_gX else None
        an = AM.model_vjp(w1, U, lam, gU, gX)
        # p_0 is the existing restatement's dL/dx0
        x0 = AN.vjp(w1, lam, gU, gX)["x0"]
        assert np.abs(an["x0"] - x0).max() <= 1e-9 * max(1.0, np.abs(x0).max())
        fd = AM.fd_model_gradients(w1, gU, gX)
        for key, g in fd.items():
            ref = an[key]
            ok = ~np.isnan(g)
            err = np.abs(g[ok] - ref[ok]).max() / max(1.0, np.abs(ref).max())
            assert err <= 1e-6, (b, key, err)
        for key in ("C", "D"):
            assert an[key].shape == (N, len(lam) // N, nx if key == "C" else U.size // N)
        checked += 1
        if checked == need:
            return
    raise AssertionError(f"only {checked} strictly complementary problems")


def test_model_np_triple_integrator_without_D():
    rng = np.random.default_rng(21)
    w = W.triple_integrator_batch(12)
    assert w["D"] is None and w["wx"] is None
    _check_against_fd(w, rng, need=3)


def test_model_np_triple_integrator_without_gX():
    rng = np.random.default_rng(22)
    _check_against_fd(W.triple_integrator_batch(12, seed=5), rng, need=3, with_gX=False)


def test_model_np_random_ltv():
    rng = np.random.default_rng(23)
    w = _ltv(31, 12)
    assert w["C"] is not None and w["D"] is not None and w["wx"] > 0 and w["wt"] > 0
    _check_against_fd(w, rng, need=4)
    _check_against_fd(w, rng, need=2, with_gX=False)


def test_model_np_random_ltv_without_C():
    rng = np.random.default_rng(24)
    w = _ltv(32, 12)
    w["C"] = None
    _check_against_fd(w, rng, need=3)


def test_model_np_stage_weight_without_targets():
    # MPCQP_P_STAGE without MPCQP_Q_STAGE: the stage term is w_x |Psi U|^2 / 2, its error trajectory the forced response
    rng = np.random.default_rng(25)
    w = _ltv(33, 12)
    w["targets"] = None
    _check_against_fd(w, rng, need=3)


def test_model_np_weights_without_goal():
    # w_t set and no goal: neither q term is accumulated (the reference raises first), both P terms stay
    rng = np.random.default_rng(26)
    w = _ltv(34, 12)
    w["goal"] = None
    _check_against_fd(w, rng, need=3)


def test_plan_vjp_model_exports_are_declared():
    assert "mpcqp_plan_vjp_model_workspace_bytes" in _capi.EXPORTS
    assert "mpcqp_plan_vjp_model_batch" in _capi.EXPORTS
    assert _capi.ABI_VERSION == 12
    assert hasattr(_capi, "VjpModelOut")
    names = [f[0] for f in _capi.VjpModelOut._fields_]
    assert names == ["g_x0", "g_goal", "g_targets", "g_e", "g_A", "g_B", "g_C", "g_D", "g_w"]


def test_plan_vjp_model_workspace_query():
    # host-only entry points: the model export's workspace holds the plain one's, and the envelope is the same
    import ctypes as C

    lib = _capi.load()
    for name in ("mpcqp_plan_vjp_model_workspace_bytes", "mpcqp_plan_vjp_model_batch"):
        assert hasattr(lib, name), name
    for nx, nu, N, mk in ((3, 1, 16, 2), (4, 1, 50, 2), (6, 2, 24, 3), (4, 2, 64, 2)):
        d = _capi.Dims(nx, nu, N, mk, _capi.F64, 15, 1.0, 0.5, 1e-3)
        plain, model = C.c_size_t(0), C.c_size_t(0)
        assert lib.mpcqp_plan_vjp_workspace_bytes(C.byref(d), 64, C.byref(plain)) == 0
        assert lib.mpcqp_plan_vjp_model_workspace_bytes(C.byref(d), 64, C.byref(model)) == 0
        assert model.value >= plain.value
    d = _capi.Dims(3, 2, 70, 2, _capi.F64, 15, 1.0, 0.5, 1e-3)  # n = 140
    assert lib.mpcqp_plan_vjp_model_workspace_bytes(C.byref(d), 8, C.byref(model)) == _capi.EUNSUPPORTED
    d = _capi.Dims(3, 1, 16, 2, _capi.F32, 15, 1.0, 0.5, 1e-3)
    assert lib.mpcqp_plan_vjp_model_workspace_bytes(C.byref(d), 8, C.byref(model)) == _capi.EDTYPE


def test_solve_mpc_batch_diff_takes_model_operands():
    from qpmpc_amd import solve_mpc_batch_diff

    params = inspect.signature(solve_mpc_batch_diff).parameters
    for name in ("transition_state_matrix", "transition_input_matrix", "ineq_state_matrix", "ineq_input_matrix",
                 "terminal_cost_weight", "stage_state_cost_weight", "stage_input_cost_weight"):
        assert name in params and params[name].kind == inspect.Parameter.KEYWORD_ONLY, name
