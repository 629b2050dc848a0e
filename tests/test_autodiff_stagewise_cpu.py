"""The stage-wise adjoint without a GPU: the NumPy restatement (tests/adjoint_stagewise_np.py, on the whitened Riccati
recursion) against the condensed restatements (tests/adjoint_np.py, tests/adjoint_model_np.py) at 1e-9 relative, and the
C exports and Python surface of the feature."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest

import adjoint_model_np as AM
import adjoint_np as AN
import adjoint_stagewise_np as AS
from host_helpers import _dims, _header, _lib, _ltv
from qpmpc_amd import _capi
from qpmpc_amd import workloads as W


EXPORTS = ("mpcqp_plan_vjp_stagewise_workspace_bytes", "mpcqp_plan_vjp_stagewise_batch")


def _compare(w, rng, need, with_gX=True):
    """Solved problems of ``w`` (C oracle): every output of the stage-wise restatement equals the condensed ones."""
    N = int(w["N"])
    checked = 0
    for b in range(np.asarray(w["x0"]).shape[0]):
        w1 = AN.single(w, b)
        U, lam, _, st = AN.solve(w1)
        if st != 0:
            continue
        nx = w1["x0"].shape[1]
        gU = rng.standard_normal(U.size)
        gX = rng.standard_normal((N + 1) * nx) if with_gX else None
        sw = AS.stagewise_vjp(w1, lam, gU, gX, U=U)
        assert sw["status"] == 0
        ref = AN.vjp(w1, lam, gU, gX)
        ref.update({k: v for k, v in AM.model_vjp(w1, U, lam, gU, gX).items() if k != "x0"})
        for key in ("x0", "goal", "targets", "e", "A", "B", "C", "D", "w"):
            r = np.asarray(ref[key]).ravel()
            err = np.abs(np.asarray(sw[key]).ravel() - r).max()
            assert err <= 1e-9 * max(1.0, np.abs(r).max()), (b, key, err)
        checked += 1
        if checked == need:
            return
    raise AssertionError(f"only {checked} solved problems")


@pytest.mark.parametrize("nx,nu,N,mk", [(3, 2, 8, 2), (4, 2, 40, 3), (6, 3, 60, 2), (3, 2, 150, 2)])
def test_random_ltv(nx, nu, N, mk):
    _compare(_ltv(40 + N, 6, nx, nu, N, mk), np.random.default_rng(N), need=2)
    _compare(_ltv(41 + N, 4, nx, nu, N, mk), np.random.default_rng(N + 1), need=1, with_gX=False)


def test_wip_n200():
    # (at the default T = 0.024 s the condensed P of N = 200 is not positive definite; on longer horizons of the unstable
    # pendulum the condensed restatement itself loses digits: 1e-8 apart at T = 0.01 s, 1e-11 at 0.005 s)
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


def test_p_only_weights():
    w = _ltv(53, 6, 3, 2, 20, 2)
    w["goal"], w["targets"] = None, None  # w_t, w_x weigh the forced response: P terms without q terms
    _compare(w, np.random.default_rng(9), need=2)


def test_zero_row_active_is_not_pd():
    w = _ltv(54, 1, 3, 2, 6, 2)
    w["C"][0, 3, 1], w["D"][0, 3, 1] = 0.0, 0.0
    lam = np.zeros(12)
    lam[3 * 2 + 1] = 1.0
    out = AS.stagewise_vjp(AN.single(w, 0), lam, np.ones(12))
    assert out["status"] == AS.NOT_PD and not out["x0"].any()
    w = _ltv(55, 1, 3, 1, 6, 4)  # n = 6 < m = 24 rows all active
    out = AS.stagewise_vjp(AN.single(w, 0), np.ones(24), np.ones(6))
    assert out["status"] == AS.NOT_PD


# ---------------------------------------------------------------- public surface

def test_exports_declared_and_bound():
    declared = set(re.findall(r"(mpcqp_[a-z_]+)\(", _header()))
    for name in EXPORTS:
        assert name in declared
        assert name in _capi.EXPORTS
    assert _capi.ABI_VERSION == 12
    assert "#define MPCQP_ABI_VERSION 12" in _header()


def _query(dims, batch, max_active):
    nbytes = C.c_size_t(0)
    rc = _lib().mpcqp_plan_vjp_stagewise_workspace_bytes(C.byref(dims), batch, max_active, C.byref(nbytes))
    return rc, nbytes.value


def test_workspace_query():
    rc, b140 = _query(_dims(3, 2, 70, 2), 8, 16)  # n = 140: beyond the condensed adjoint
    assert rc == 0 and b140 > 0
    cond = C.c_size_t(0)
    assert _lib().mpcqp_plan_vjp_workspace_bytes(C.byref(_dims(3, 2, 70, 2)), 8, C.byref(cond)) == -6
    rc, b1024 = _query(_dims(3, 1, 1024, 4), 2, 64)
    assert rc == 0 and b1024 > 0
    sizes = [_query(_dims(12, 4, 64, 16), 4, k)[1] for k in (0, 8, 63, 64, 200)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert _query(_dims(12, 4, 64, 16), 0, 8) == (0, 0)


def test_workspace_query_envelope():
    assert _query(_dims(3, 2, 70, 2, dtype=_capi.F32), 1, 4)[0] == -3  # MPCQP_EDTYPE
    assert _query(_dims(33, 2, 10, 2), 1, 4)[0] == -6                    # MPCQP_EUNSUPPORTED
    assert _query(_dims(3, 9, 10, 2), 1, 4)[0] == -6
    assert _query(_dims(32, 8, 10, 2), 1, 4)[0] == 0
    assert _query(_dims(3, 2, 10, 2), 1, -1)[0] == -1                    # MPCQP_EINVAL


def test_solve_mpc_batch_diff_has_keyword_only_adjoint():
    from qpmpc_amd import autodiff, solve_mpc_batch_diff

    prm = inspect.signature(solve_mpc_batch_diff).parameters["adjoint"]
    assert prm.kind is inspect.Parameter.KEYWORD_ONLY and prm.default == "condensed"
    assert autodiff.ADJOINTS == ("condensed", "stagewise")


def test_bad_adjoint_and_envelope_raise_before_any_launch():
    torch = pytest.importorskip("torch")
    from qpmpc_amd import BackendError, ProblemDefinitionError, solve_mpc_batch_diff
    from qpmpc_amd import autodiff

    w = _ltv(60, 2, 3, 2, 5, 2)
    bp = W.to_batch_problem(w, device="cpu")
    x0 = torch.as_tensor(w["x0"]).clone().requires_grad_()
    with pytest.raises(ProblemDefinitionError):
        solve_mpc_batch_diff(bp, initial_state=x0, adjoint="dense")
    wide = W.to_batch_problem(_ltv(61, 1, 33, 2, 3, 1), device="cpu")
    with pytest.raises(BackendError):
        autodiff.check_envelope_stagewise(wide)
    big = W.to_batch_problem(_ltv(62, 1, 3, 9, 3, 1), device="cpu")
    with pytest.raises(BackendError):
        autodiff.check_envelope_stagewise(big)
    autodiff.check_envelope_stagewise(W.to_batch_problem(_ltv(63, 1, 3, 2, 500, 1), device="cpu"))
