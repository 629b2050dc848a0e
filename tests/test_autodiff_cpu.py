"""Gradients through plans, without a GPU: the NumPy restatement of the vector-Jacobian product (tests/adjoint_np.py)
against central finite differences of the C oracle's solve, on strictly complementary problems (every row has a
multiplier or a slack above 1e-4, so a small step keeps the active set); and the public surface of the feature."""

import numpy as np

import adjoint_np as AN
from qpmpc_amd import _capi
from qpmpc_amd import workloads as W


def _check_against_fd(w, batch, rng, need):
    N = int(w["N"])
    checked = 0
    for b in range(batch):
        w1 = AN.single(w, b)
        U, lam, slack, st = AN.solve(w1)
        if st != 0 or not AN.strictly_complementary(lam, slack):
            continue
        nx = w1["x0"].shape[1]
        gU = rng.standard_normal(U.size)
        gX = rng.standard_normal((N + 1) * nx)
        an = AN.vjp(w1, lam, gU, gX)
        fd = AN.fd_gradients(w1, gU, gX)
        assert set(fd) >= {"x0", "e"}
        for key, g in fd.items():
            err = np.abs(g - an[key]).max() / max(1.0, np.abs(an[key]).max())
            assert err <= 1e-6, (b, key, err)
        checked += 1
    assert checked >= need, checked


def test_adjoint_np_matches_finite_differences_triple_integrator():
    rng = np.random.default_rng(7)
    _check_against_fd(W.triple_integrator_batch(12), 12, rng, need=6)


def test_adjoint_np_matches_finite_differences_random_ltv():
    from qpmpc_amd.workloads import random_ltv

    rng = np.random.default_rng(11)
    w = random_ltv(rng, 10, 3, 2, 5, 2, 1.0)  # input rows (D), state rows (C), stage and terminal cost
    assert w["D"] is not None and w["wx"] > 0
    _check_against_fd(w, 10, rng, need=6)


def test_solve_mpc_batch_diff_is_public():
    import qpmpc_amd
    from qpmpc_amd import solve_mpc_batch_diff

    assert callable(solve_mpc_batch_diff)
    assert "solve_mpc_batch_diff" in qpmpc_amd.__all__


def test_plan_vjp_exports_are_declared():
    assert "mpcqp_plan_vjp_workspace_bytes" in _capi.EXPORTS
    assert "mpcqp_plan_vjp_batch" in _capi.EXPORTS
    assert _capi.ABI_VERSION == 12
