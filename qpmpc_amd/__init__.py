"""MI355X-native batched linear MPC: a drop-in for the hot path of qpmpc.

Same public names as the reference (qpmpc/__init__.py:9-21) -- ``MPCProblem``,
``MPCQP``, ``Plan``, ``solve_mpc`` -- plus the batched entry points that are the
reason this package exists: ``BatchMPCProblem``, ``solve_mpc_batch``,
``BatchMPCQP``, ``solve_qp_batch``, ``rollout_batch`` -- and ``solve_mpc_batch_diff``, whose plans
carry gradients to x0, goal, targets and e, and ``plan_jvp`` / ``plan_jacobian``, their forward sensitivities, condensed
(n <= 128) or, with ``formulation="stagewise"``, at any horizon, along tangents of the model matrices and the cost weights too
(extensions: the reference has no gradients). ``closed_loop_diff`` carries gradients through whole closed loops of a
``SharedModel`` (``ModelClosedLoop``), forward and backward one launch each; ``closed_loop_jvp`` / ``closed_loop_jacobian`` are
their forward sensitivities, every period and tangent in one launch.

All arithmetic runs in hand-written HIP kernels behind the C ABI of
``include/mpcqp.h``; without the compiled library or without a GPU every
compute entry point raises ``BackendError`` (no CPU fallback).
"""
from .batch import (  # noqa: F401
    BatchMPCProblem,
    BatchMPCQP,
    BatchPlan,
    PreparedModelSolve,
    PreparedSolve,
    WarmState,
    SharedModel,
    rollout_batch,
    pairing_order,
    solve_mpc_batch,
    solve_qp_batch,
)
from .closed_loop import ModelClosedLoop  # noqa: F401
from .loop_diff import closed_loop_diff, closed_loop_jacobian, closed_loop_jvp  # noqa: F401
from .autodiff import plan_jacobian, plan_jvp, solve_mpc_batch_diff  # noqa: F401
from .exceptions import (  # noqa: F401
    BackendError,
    PlanError,
    ProblemDefinitionError,
    QPMPCException,
    StateError,
)
from .mpc_problem import MPCProblem  # noqa: F401
from .mpc_qp import MPCQP  # noqa: F401
from .plan import Plan, Solution  # noqa: F401
from .solve_mpc import available_solvers, solve_mpc  # noqa: F401

__all__ = [
    "MPCProblem",
    "MPCQP",
    "Plan",
    "solve_mpc",
    "BatchMPCProblem",
    "BatchMPCQP",
    "BatchPlan",
    "PreparedSolve",
    "WarmState",
    "SharedModel",
    "PreparedModelSolve",
    "ModelClosedLoop",
    "closed_loop_diff",
    "closed_loop_jvp",
    "closed_loop_jacobian",
    "pairing_order",
    "solve_mpc_batch",
    "solve_qp_batch",
    "rollout_batch",
    "solve_mpc_batch_diff",
    "plan_jvp",
    "plan_jacobian",
]

__version__ = "0.1.0"
REFERENCE_VERSION = "3.1.0"  # qpmpc release whose API surface is mirrored
