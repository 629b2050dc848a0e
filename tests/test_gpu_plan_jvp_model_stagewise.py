"""Model and weight tangents of batched plans on the MI355X, stage-wise: mpcqp_plan_jvp_model_stagewise_batch (the kModel
instantiation of mpcqp_tangent_stagewise_kernel in qpmpc_amd/csrc/mpcqp_adjoint_stagewise.hip) against the NumPy
restatement of tests/tangent_model_np.py at 1e-8 max(1, |ref|) with every operand's tangent at once, beyond n = 128, on
the config-5 shape (float32 storage too), beyond the wide forward kernel and without an active row; a tangent's
independence of its slot, pass and T; and, through the checks of tests/plan_jvp_model_checks.py, the duality with
mpcqp_plan_vjp_stagewise_batch, shared and time-invariant tangents, unsolved problems, the state-only call and the
weight Jacobian."""

import numpy as np
import pytest

from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

import plan_jvp_model_checks as M  # noqa: E402  (needs torch)
from guarded_launch import _torch  # noqa: E402

SW = dict(formulation="stagewise")


def test_n140_beyond_the_condensed_tangent():
    M.check_path(M.random_ltv(10, 8, 3, 2, 70, 2), 10, **SW)


@pytest.mark.parametrize("f32", [False, True])
def test_config5_shape(f32):
    """(12, 4, 64). float32 operands are converted; the comparison is on the float64 results."""
    M.check_path(W.synthetic_ltv_batch(16), 13, limit=8, dtype=_torch().float32 if f32 else None, **SW)


def test_beyond_the_wide_kernel():
    M.check_path(M.random_ltv(12, 8, 20, 6, 10, 4), 12, **SW)


def test_inactive_problem():
    w = M.random_ltv(20, 4, 3, 2, 70, 2)
    w["e"] = w["e"] + 1e3  # no active row: k = 0
    bp, plan, *_ = M.check_path(w, 20, need=1.0, **SW)
    assert (plan.multipliers == 0).all()


def test_p_only_problem_and_without_C_or_D():
    M.check_path(M.p_only(), 12, limit=8, **SW)
    M.check_path(M.without("C", 51), 51, limit=8, **SW)
    M.check_path(M.without("D", 52), 52, limit=8, **SW)


@pytest.mark.parametrize("seed,dims,few", [(10, (3, 2, 70, 2), 100), (12, (20, 6, 10, 4), 13)])
def test_a_tangent_does_not_depend_on_its_slot_pass_or_T(seed, dims, few):
    """T = 1, a ragged T (no multiple of the 256 / max(nx, nu) slots: 85 and 12 here) and T = 256: bitwise the same
    results for the tangents they share, and for the last tangents alone."""
    torch = _torch()
    from qpmpc_amd import solve_mpc_batch

    w = M.random_ltv(seed, 8, *dims)
    bp = W.to_batch_problem(w)
    plan = solve_mpc_batch(bp, return_multipliers=True, formulation="stagewise")
    assert (plan.status == 0).any() and (plan.multipliers > 0).any()
    tan = M.model_tangents(w, 8, 256, np.random.default_rng(23))
    dU, dX = M.gpu_jvp(bp, plan, tan, "stagewise")
    assert (plan.jvp_status == plan.status).all() and dU.abs().sum() > 0
    for sl in (slice(0, 1), slice(0, few), slice(250, 256)):
        dUt, dXt = M.gpu_jvp(bp, plan, {k: np.ascontiguousarray(v[:, sl]) for k, v in tan.items()}, "stagewise")
        assert torch.equal(dUt, dU[:, sl]) and torch.equal(dXt, dX[:, sl]), sl


@pytest.mark.parametrize("make", [lambda: M.random_ltv(10, 8, 3, 2, 70, 2), lambda: W.wip_batch(16, N=50),
                                  lambda: M.random_ltv(5, 32, 4, 2, 12, 3), M.p_only])
def test_duality_with_the_stagewise_vjp_export(make):
    M.check_duality(make(), "stagewise", "stagewise")


def test_shared_and_time_invariant_tangents_are_bitwise_their_copies():
    M.check_shared_and_time_invariant(M.random_ltv(8, 12, 3, 2, 70, 2), "stagewise")


def test_unsolved_problems_get_zeros_and_their_status():
    M.check_unsolved(M.random_ltv(26, 8, 3, 2, 70, 2), "stagewise")


def test_state_tangents_only_are_bitwise_the_old_export():
    M.check_state_only_is_bitwise_the_old_export(M.random_ltv(8, 12, 3, 2, 70, 2), "stagewise")


def test_weight_jacobian_against_central_differences():
    M.check_weight_jacobian("stagewise")


def test_agrees_with_the_condensed_export():
    M.check_the_two_formulations_agree()
