"""Model and weight tangents of batched plans on the MI355X, condensed: mpcqp_plan_jvp_model_batch (the kModel
instantiation of mpcqp_tangent_kernel in qpmpc_amd/csrc/mpcqp_adjoint.hip) against the NumPy restatement of
tests/tangent_model_np.py at 1e-8 max(1, |ref|) with every operand's tangent at once, its duality with
mpcqp_plan_vjp_model_batch, the stage-wise formulation, shared and time-invariant tangents, unsolved problems, the
state-only call (bitwise mpcqp_plan_jvp_batch) and plan_jacobian(wrt="cost_weights") against central differences.

The checks are those of tests/plan_jvp_model_checks.py, which take ``formulation``: tests/test_gpu_plan_jvp_model_stagewise.py
runs them on the stage-wise export."""
import numpy as np
import pytest

import adjoint_np as AN
from qpmpc_amd import workloads as W

pytestmark = pytest.mark.gpu

pytest.importorskip("torch")

from plan_jvp_model_checks import (check_duality, check_path, check_shared_and_time_invariant,  # noqa: E402
                                   check_state_only_is_bitwise_the_old_export, check_the_two_formulations_agree,
                                   check_unsolved, check_weight_jacobian, p_only, random_ltv, without)


def test_config2_four_and_two_per_wavefront():
    from qpmpc_amd import _capi

    w = W.triple_integrator_batch(256)
    check_path(w, 1, limit=24, flags=_capi.OPT_FOUR_PER_WAVE)
    check_path(w, 1, limit=24, flags=_capi.OPT_TWO_PER_WAVE)


def test_random_ltv():
    check_path(random_ltv(3, 64, 6, 2, 24, 3), 3, limit=24)


def test_wip_n50():
    check_path(W.wip_batch(64, N=50), 2, limit=16)


def test_n128_workspace_carve():
    check_path(random_ltv(4, 16, 4, 2, 64, 2), 4, T=5, limit=8)


def test_p_only_problem():
    from oracle.capi import FLAG_P_STAGE, FLAG_P_TERMINAL, FLAG_Q_STAGE, FLAG_Q_TERMINAL, flags_of
    from qpmpc_amd.workloads import problem_from_workload

    w = p_only()
    f = flags_of(problem_from_workload(AN.single(w, 0), 0))
    assert f & (FLAG_P_STAGE | FLAG_P_TERMINAL) and not f & (FLAG_Q_STAGE | FLAG_Q_TERMINAL)
    bp, plan, tan, dU, dX = check_path(w, 12, limit=16)
    assert (plan.U.abs().amax(dim=1) > 0.1).float().mean() > 0.5 and (np.abs(dU).max(axis=(1, 2)) > 0.1).mean() > 0.5


@pytest.mark.parametrize("key,seed", [("C", 51), ("D", 52)])
def test_without_C_and_without_D(key, seed):
    check_path(without(key, seed), seed, limit=16)


@pytest.mark.parametrize("make", [lambda: W.triple_integrator_batch(64), lambda: W.wip_batch(16, N=50),
                                  lambda: random_ltv(5, 32, 4, 2, 12, 3), p_only])
def test_duality_with_the_model_vjp_export(make):
    check_duality(make(), "condensed", "model")


def test_the_two_formulations_agree():
    """Each is held to the restatement at 1e-8 max(1, |ref|): to each other at twice that."""
    check_the_two_formulations_agree()


def test_shared_and_time_invariant_tangents_are_bitwise_their_copies():
    check_shared_and_time_invariant(random_ltv(8, 48, 3, 2, 8, 2), "condensed")


def test_unsolved_problems_get_zeros_and_their_status():
    check_unsolved(random_ltv(6, 32, 3, 2, 8, 2), "condensed")


def test_state_tangents_only_are_bitwise_the_old_export():
    check_state_only_is_bitwise_the_old_export(random_ltv(8, 48, 3, 2, 8, 2), "condensed")


def test_weight_jacobian_against_central_differences():
    check_weight_jacobian("condensed")
