"""Forward sensitivities of plans without a GPU: the NumPy restatement of the Jacobian-vector product
(tests/tangent_np.py) against central differences of the C oracle's solve on strictly complementary problems, its
duality with the VJP restatement (tests/adjoint_np.py), the LQR gain on an unconstrained plan, and the C exports and
Python surface of the feature."""
import ctypes as C
import re

import numpy as np
import pytest

import adjoint_np as AN
import tangent_np as TN
from host_helpers import _dims, _header, _lib, _ltv
from qpmpc_amd import _capi
from qpmpc_amd import workloads as W


EXPORTS = ("mpcqp_plan_jvp_workspace_bytes", "mpcqp_plan_jvp_batch")


def _check_against_fd(w, rng, need):
    checked = 0
    for b in range(np.asarray(w["x0"]).shape[0]):
        w1 = AN.single(w, b)
        U, lam, slack, st = AN.solve(w1)
        if st != 0 or not AN.strictly_complementary(lam, slack):
            continue
        tan = TN.random_tangent(w1, rng)
        an = TN.jvp(w1, lam, tan)
        fd = TN.fd_jvp(w1, tan)
        for key in ("U", "X"):
            err = np.abs(fd[key] - an[key]).max() / max(1.0, np.abs(an[key]).max())
            assert err <= 1e-6, (b, key, err)
        checked += 1
        if checked == need:
            return
    raise AssertionError(f"only {checked} strictly complementary problems")


def test_tangent_np_matches_finite_differences_triple_integrator():
    _check_against_fd(W.triple_integrator_batch(12), np.random.default_rng(7), need=6)


def test_tangent_np_matches_finite_differences_random_ltv():
    w = _ltv(11, 10, 3, 2, 5, 2)  # input rows (D), state rows (C), stage and terminal cost
    assert w["D"] is not None and w["C"] is not None and w["wx"] > 0 and w["targets"] is not None
    _check_against_fd(w, np.random.default_rng(12), need=6)


@pytest.mark.parametrize("make", [lambda: W.triple_integrator_batch(6), lambda: _ltv(21, 6, 4, 2, 8, 3),
                                  lambda: W.wip_batch(4, N=20)])
def test_duality_with_the_vjp(make):
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
        fwd = TN.jvp(w1, lam, tan)
        g = AN.vjp(w1, lam, gU, gX)
        lhs = gU @ fwd["U"] + gX @ fwd["X"]
        rhs = sum(float(np.asarray(g[k]).ravel() @ tan[k]) for k in tan)
        assert abs(lhs - rhs) <= 1e-10 * max(1.0, abs(lhs), abs(rhs)), (b, lhs, rhs)
        checked += 1
    assert checked >= 3


def test_unconstrained_first_step_jacobian_is_the_lqr_gain():
    from oracle.stagewise_np import Riccati, from_mpc_problem
    from qpmpc_amd.workloads import problem_from_workload

    w = _ltv(31, 3, 4, 2, 10, 2)
    N, nx, nu = 10, 4, 2
    for b in range(3):
        w1 = AN.single(w, b)
        lam = np.zeros(N * 2)  # no active row
        J = np.stack([TN.jvp(w1, lam, {"x0": np.eye(nx)[j]})["U"] for j in range(nx)], axis=1)  # [n, nx]
        K0 = Riccati(from_mpc_problem(problem_from_workload(w1, 0))).K[0]
        np.testing.assert_allclose(J[:nu], -K0, rtol=1e-9, atol=1e-9 * max(1.0, np.abs(K0).max()))


# ---------------------------------------------------------------- public surface

def test_exports_declared_and_bound():
    declared = set(re.findall(r"(mpcqp_[a-z_]+)\(", _header()))
    for name in EXPORTS:
        assert name in declared
        assert name in _capi.EXPORTS
    assert "typedef struct MpcqpTangents" in _header()
    assert [f for f, _ in _capi.Tangents._fields_] == ["dx0", "dgoal", "dtargets", "de", "dx0_stride", "dgoal_stride",
                                                       "dtargets_stride", "de_stride"]
    assert _capi.ABI_VERSION == 12
    lib = _lib()
    for name in EXPORTS:
        assert hasattr(lib, name)


def _query(dims, batch, ntan):
    nbytes = C.c_size_t(0)
    rc = _lib().mpcqp_plan_jvp_workspace_bytes(C.byref(dims), batch, ntan, C.byref(nbytes))
    return rc, nbytes.value


def test_workspace_query():
    assert _query(_dims(3, 1, 16, 2, dtype=_capi.F32), 8, 3)[0] == -3  # MPCQP_EDTYPE
    assert _query(_dims(3, 2, 65, 2), 8, 3)[0] == -6                    # n = 130: MPCQP_EUNSUPPORTED
    assert _query(_dims(3, 1, 16, 2), 8, 0)[0] == -1                    # MPCQP_EINVAL
    assert _query(_dims(3, 1, 16, 2), 8, 257)[0] == -1
    rc, small = _query(_dims(3, 1, 16, 2), 8, 3)
    assert rc == 0 and small > 0
    vjp = C.c_size_t(0)
    assert _lib().mpcqp_plan_vjp_workspace_bytes(C.byref(_dims(3, 1, 16, 2)), 8, C.byref(vjp)) == 0
    assert small <= vjp.value  # config-2-like: both carves in LDS, the same condensed segments
    rc, big = _query(_dims(4, 2, 64, 2), 8, 256)  # n = 128, 256 tangents: carves in the workspace
    assert rc == 0 and big >= 8 * 8 * 129 * (128 + 384 + 128 + 256)
    assert _query(_dims(3, 1, 16, 2), 0, 3) == (0, 0)


def test_batch_argument_checks():
    lib = _lib()
    d = _dims(3, 1, 16, 2)
    prob = _capi.Problem()
    tan = _capi.Tangents()
    # checks run in order: dims, ntan, then the problem's operands and pointers -- before anything is launched
    assert lib.mpcqp_plan_jvp_batch(C.byref(_dims(3, 1, 16, 2, _capi.F32)), C.byref(prob), 4, 1, None, None, None,
                                    None, None, None, None, 0, None) == -3
    assert lib.mpcqp_plan_jvp_batch(C.byref(d), C.byref(prob), 4, 0, None, None, C.byref(tan), None, None, None, None,
                                    0, None) == -1


def test_new_names_are_public():
    import qpmpc_amd
    from qpmpc_amd import plan_jacobian, plan_jvp

    assert callable(plan_jvp) and callable(plan_jacobian)
    assert {"plan_jvp", "plan_jacobian"} <= set(qpmpc_amd.__all__)


def test_dual_model_operand_and_stagewise_raise_before_any_launch():
    torch = pytest.importorskip("torch")
    from torch.autograd import forward_ad as fwAD

    from qpmpc_amd import BackendError, solve_mpc_batch_diff

    w = _ltv(60, 2, 3, 2, 5, 2)
    bp = W.to_batch_problem(w, device="cpu")
    A = torch.as_tensor(w["A"])
    x0 = torch.as_tensor(w["x0"])
    with fwAD.dual_level():
        dA = fwAD.make_dual(A, torch.ones_like(A))
        with pytest.raises(BackendError, match="transition_state_matrix"):
            solve_mpc_batch_diff(bp, transition_state_matrix=dA)
        dx = fwAD.make_dual(x0, torch.ones_like(x0))
        with pytest.raises(BackendError, match="stagewise"):
            solve_mpc_batch_diff(bp, initial_state=dx, adjoint="stagewise")
        big = W.to_batch_problem(_ltv(61, 1, 3, 2, 70, 2), device="cpu")  # n = 140
        x1 = torch.as_tensor(_ltv(61, 1, 3, 2, 70, 2)["x0"])
        with pytest.raises(BackendError):
            solve_mpc_batch_diff(big, initial_state=fwAD.make_dual(x1, torch.ones_like(x1)))


def test_plan_jvp_needs_multipliers():
    pytest.importorskip("torch")
    from qpmpc_amd import BackendError, ProblemDefinitionError, plan_jvp
    from qpmpc_amd.batch import BatchPlan

    w = _ltv(62, 2, 3, 2, 5, 2)
    bp = W.to_batch_problem(w, device="cpu")
    import torch

    plan = BatchPlan(bp, torch.zeros(2, 10, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), None)
    with pytest.raises(ProblemDefinitionError, match="return_multipliers=True"):
        plan_jvp(bp, plan, initial_state=torch.zeros(1, 1, 3, dtype=torch.float64))
    big = W.to_batch_problem(_ltv(63, 1, 3, 2, 70, 2), device="cpu")
    plan = BatchPlan(big, None, None, None, multipliers=torch.zeros(1, 140, dtype=torch.float64))
    with pytest.raises(BackendError, match="128"):
        plan_jvp(big, plan, initial_state=torch.zeros(1, 1, 3, dtype=torch.float64))
