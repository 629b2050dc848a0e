/*
 * mpcqp.h -- C ABI of libmpcqp_hip.so, the MI355X (gfx950) implementation of
 * qpmpc's hot path:  MPCProblem -> MPCQP (condense) -> dense QP solve -> inputs.
 *
 * The reference (stephane-caron/qpmpc v3.1.0) is pure Python and has no FFI
 * layer of its own; its operator boundary for this path is
 *     solve_mpc(problem, solver, sparse=False, **kw) -> Plan   qpmpc/solve_mpc.py:16-44
 *     MPCQP(problem, sparse=False)                             qpmpc/mpc_qp.py:39-122
 * Each entry point below names the reference code it replaces. A Python
 * maintainer binds them with ctypes.
 *
 * Conventions
 *  - plain pointers and sizes only; every pointer is DEVICE memory owned by the
 *    caller (the library never allocates or frees device memory); problems that do
 *    not fit the on-chip path need a caller-provided scratch `workspace` whose size
 *    the *_workspace_bytes functions report (0 for the on-chip path; NULL is then fine);
 *  - every call is asynchronous on the caller's hipStream_t (passed as void*;
 *    NULL = the null stream), re-entrant, no global state (nothing is read from the
 *    process environment; dispatch overrides are explicit MpcqpSolveOpts.flags);
 *  - return value: 0 ok, <0 bad argument (MPCQP_E*), >0 a hipError_t;
 *    per-problem outcome is reported in status[b], never by the return value;
 *  - matrices are row-major and densely packed; one batch item after another
 *    unless a stride says otherwise;
 *  - constraints are  G u <= h ; the QP is  min 1/2 u'Pu + q'u.
 *
 * Memory contract (tests/test_gpu_memory_discipline.py holds every export to it)
 *  - a launch reads its operands and writes its outputs inside the extents this header names and nowhere else: an operand of
 *    `batch` problems ends with the last problem's block ((batch - 1) * batch_stride + block elements), an output is packed
 *    unless a stride is named, the workspace is exactly what the matching *_workspace_bytes query reports for the same
 *    dimensions, batch and slot / tangent counts; no alignment beyond the element's own is assumed past a buffer's end;
 *  - the initial content of the workspace, of every output and of a cold launch's warm_state is never read: a launch writes
 *    what it later reads. The exceptions are the documented sequences -- MPCQP_OPT_REUSE_FACTOR / _PIPELINE_FACTOR read the
 *    factor image a launch with MPCQP_OPT_KEEP_FACTOR left in the same workspace, warm_start != 0 reads the record (and, for
 *    the narrow stage-wise kernel, the rows in the workspace) of the launch before, mpcqp_condense_phase_batch phase 2 reads
 *    what phase 1 left in Psi and the workspace, and the `states` / `stats` arguments of the closed-loop exports are in/out;
 *  - outputs per problem: status[b] and iters[b] are written for every problem; U (x) of a problem with status[b] != 0 is all
 *    zeros (an empty plan, never NaN); lam[b] is defined for solved problems only. The derivative exports write zeros and the
 *    forward status for problems that were not solved (see each of them);
 *  - an output passed as NULL where that is allowed is not written and changes nothing in the others; a problem that a pairing
 *    `order` leaves out keeps its old outputs; the elements between two rows of a strided argument (u_stride) are not touched;
 *  - read-only arguments (everything declared const, the operands, the model of the solve_model exports) are never written;
 *  - mpcqp_model_vjp_batch / mpcqp_model_jvp_batch touch nothing outside the named extents and the model (mpcqp_model_bytes).
 *    The same holds for mpcqp_model_periods_vjp_batch (tests/test_gpu_loop_diff.py).
 *
 * Stream contract (tests/test_gpu_streams.py holds every forward route, the stateful sequences and the Python layer to it)
 *  - every kernel of a call is enqueued on the stream the call is given, in order, and on no other: a call that launches several
 *    kernels (the float32 conversion around a float64 solve; propagate, Gram, transpose and solve on the dense path; the narrow
 *    stage-wise kernel and the wide kernel's second opinion; the three kernels of mpcqp_order_by_count) is one item of that
 *    stream's order -- it sees what was enqueued on the stream before it and is seen by what is enqueued behind it;
 *  - no call synchronises with the host or reads a device value on the host: the return code says what was enqueued, never what
 *    a kernel found (that is status[b]);
 *  - a call can be captured into a HIP graph (hipStreamBeginCapture on its stream) after one eager launch of the same
 *    dimensions, and the graph replayed on new operand VALUES at the captured addresses; this includes the
 *    MPCQP_OPT_KEEP_FACTOR / _REUSE_FACTOR and cold / warm pairs captured as one graph of two launches. The launchers of the
 *    kernels that can need more than 48 KiB of dynamic LDS set the kernel's hipFuncAttributeMaxDynamicSharedMemorySize to the
 *    launch's own size in front of the launch: most of them only when that size exceeds 48 KiB, the dense solver's and the
 *    general stage-wise kernel's on every launch; a refusal by the runtime is the call's return code, except in the
 *    model-factoring and the on-chip 17 .. 32-variable launchers, which ignore the result (a launch the runtime then cannot
 *    make is reported by the launch itself). The runtime takes the attribute call while a stream is capturing, and one graph
 *    may hold launches of one kernel at several sizes: the value last set does not bind a replay;
 *  - concurrent calls on distinct streams, or from distinct host threads, with distinct outputs and workspaces (and warm
 *    states) are independent: each gives the bits of the same call made alone. Operands and a factored model may be shared.
 */
#ifndef MPCQP_H_
#define MPCQP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPCQP_ABI_VERSION 12

/* element type of every floating-point buffer of a call. It is the STORAGE type: mpcqp_build_solve_batch computes
 * MPCQP_F32 problems of at most 160 variables (and every float32 problem only the general stage-wise kernel serves) in
 * float64 on copies of the operands converted into the workspace -- the float32 condensed kernels square the
 * conditioning into P and returned plans 2e-2 from the float64 ones as solved on ill-conditioned problems;
 * larger float32 problems (BASELINE config 5) run the float32 stage-wise kernel, whose acceptance test is 16 tol (1 + |e|)
 * on the active rows. Contract either way: |u - u_float64| <= 1e-3 max(1, |u|), or status != MPCQP_SOLVED. */
#define MPCQP_F64 0
#define MPCQP_F32 1

/* MpcqpDims.flags -- which cost terms enter P and q. They differ on purpose:
 * the reference adds a term to P when its weight "is not None"
 * (mpc_qp.py:102,104) but to q only when weight > 1e-10 and the matching
 * state is defined (mpc_problem.py:141-166, mpc_qp.py:119-122). */
#define MPCQP_P_TERMINAL 1
#define MPCQP_P_STAGE 2
#define MPCQP_Q_TERMINAL 4
#define MPCQP_Q_STAGE 8

/* per-problem status[b]  (Plan.is_empty <=> status != 0, plan.py:35-40) */
#define MPCQP_SOLVED 0
#define MPCQP_MAX_ITER 1
#define MPCQP_INFEASIBLE 2
#define MPCQP_NOT_PD 3
#define MPCQP_SLOTS_FULL 4 /* stage-wise kernels only: more rows wanted to be active at once than the launch's max_active
                              slots hold (possible when max_active < min(n, m), i.e. n, m > 128 / 256 with the defaults);
                              solve the problem again with a larger max_active (the Python host does: solve_mpc_batch) */

/* negative return codes */
#define MPCQP_EINVAL (-1)    /* NULL/negative/inconsistent argument           */
#define MPCQP_ETOOLARGE (-2) /* no kernel for these dimensions: does not fit a CU's LDS and nx > 32 or nu > 8 with n > 256
                                (ABI 8: systems with nx <= 32, nu <= 8 are served at any horizon -- the general stage-wise
                                kernel, float64 arithmetic, takes what the MFMA stage-wise kernels (nx <= 16, nu <= 4) and
                                the dense path (n <= 256) do not: qpmpc/solve_mpc.py:42-44 accepts any dimension) */
#define MPCQP_EDTYPE (-3)    /* dtype not MPCQP_F64 / MPCQP_F32               */
#define MPCQP_ELAYOUT (-4)   /* an operand of MpcqpProblem with a non-NULL pointer has a negative batch or step stride, a step
                                stride that is neither 0 nor the block size, or a non-zero batch stride smaller than what one
                                problem occupies (N blocks with a step stride, else one block; nx for x0 and goal, N nx for
                                targets). Every export that takes an MpcqpProblem checks this before anything is launched
                                (mpcqp_update_vectors_batch, which needs no A and B, for the operands it is given); any
                                larger batch stride is taken, in both dtypes (a float32 launch that is solved in float64 -- at
                                most 160 variables -- packs the operands on conversion). The fused WIP periods keep a stricter
                                check of their own: x0, goal and targets packed, else MPCQP_EUNSUPPORTED */
#define MPCQP_EWORKSPACE (-5) /* workspace missing or too small (see *_workspace_bytes) */
#define MPCQP_EUNSUPPORTED (-6) /* option not available for these dimensions / this dtype    */

/* Problem dimensions and cost weights (mpc_problem.py:88-139).
 * n = N*nu decision variables, m = N*mk inequality rows. Problems whose
 * per-step row count varies are padded by the host to mk rows with C=D=0 and
 * e=+1e30 (an inequality that can never be active). Held, route by route, against the
 * problem with those rows deleted by tests/test_gpu_padded_rows.py (forward kernels, shared-model
 * solves, warm starts, derivative exports: lam = 0 and zero gradients on such rows). */
typedef struct MpcqpDims {
    int32_t nx;    /* state_dim                                   */
    int32_t nu;    /* input_dim                                   */
    int32_t N;     /* nb_timesteps                                */
    int32_t mk;    /* inequality rows per step (after padding)    */
    int32_t dtype; /* MPCQP_F64 | MPCQP_F32                       */
    int32_t flags; /* MPCQP_P_* | MPCQP_Q_*                       */
    double w_terminal; /* terminal_cost_weight     (ignored unless flagged) */
    double w_stage;    /* stage_state_cost_weight  (ignored unless flagged) */
    double w_input;    /* stage_input_cost_weight  > 0                      */
} MpcqpDims;

/* One operand of a batch of problems, addressed as
 *     ptr + b*batch_stride + k*step_stride      (strides in ELEMENTS)
 * batch_stride == 0: shared by every problem of the batch;
 * step_stride  == 0: time-invariant (the reference's "array, not list" case,
 *                    mpc_problem.py:177-245); otherwise it must equal the
 *                    block size (rows*cols) so a problem's steps are packed.
 * ptr == NULL means "None" where the reference allows it (C, D, goal, targets). */
typedef struct MpcqpOperand {
    const void *ptr;
    int64_t batch_stride;
    int64_t step_stride;
} MpcqpOperand;

typedef struct MpcqpProblem {
    MpcqpOperand A;       /* [N] nx x nx   transition_state_matrix              */
    MpcqpOperand B;       /* [N] nx x nu   transition_input_matrix              */
    MpcqpOperand C;       /* [N] mk x nx   ineq_state_matrix        (nullable)  */
    MpcqpOperand D;       /* [N] mk x nu   ineq_input_matrix        (nullable)  */
    MpcqpOperand e;       /* [N] mk        ineq_vector                          */
    MpcqpOperand x0;      /* nx            initial_state   (step_stride unused) */
    MpcqpOperand goal;    /* nx            goal_state      (nullable)           */
    MpcqpOperand targets; /* N*nx          target_states   (nullable)           */
} MpcqpProblem;

/* MpcqpSolveOpts.flags -- explicit kernel-dispatch overrides. 0 in production: the library picks the
 * kernel from the dimensions. Tests set them to cross-check two formulations of the same solver on the
 * same batch (they replace the MPCQP_FORCE_* environment switches of ABI 4: no hidden process state). */
#define MPCQP_OPT_FORCE_LDS 1      /* everything that fits one CU's LDS goes to the workgroup kernel      */
#define MPCQP_OPT_FORCE_GWS 2      /* large QPs: general kernel with its arrays in the workspace          */
#define MPCQP_OPT_FORCE_DENSE_G 4  /* large fused path: form G (and its transpose) instead of applying it */
#define MPCQP_OPT_ONE_PER_WAVE 8   /* small problems: one problem per wavefront instead of two            */
#define MPCQP_OPT_FORCE_CONDENSED 16 /* keep the condensed kernels (mpcqp_build_solve_batch otherwise hands 16 < n <= 128,
                                        nx <= 4, nu <= 2, float64 -- and every other problem of more than 20 variables with
                                        nx <= 16 (float32: 12), nu <= 4 -- to the stage-wise kernels, which are faster
                                        there and return the same minimiser)                                      */

#define MPCQP_OPT_STAGE_WIDE 32   /* mpcqp_stagewise_solve_batch: take the wide kernel (nx <= 16, nu <= 4, MFMA
                                     sweeps) also where the narrow one (nx <= 4, nu <= 2, float64) applies       */

#define MPCQP_OPT_KEEP_FACTOR 64  /* stage-wise kernels: leave the Riccati factor of every problem in the workspace ...  */
#define MPCQP_OPT_REUSE_FACTOR 128 /* ... and start from it: the caller asserts that A, B and the weights are those of the
                                      launch that kept it, in the same workspace (build once, then only x0 / goal /
                                      targets / e change: the reference's update_cost_vector / update_constraint_vector
                                      usage, mpc_qp.py:129-163). Ignored by the other kernels (they rebuild).          */

#define MPCQP_OPT_PIPELINE_FACTOR 256 /* stage-wise kernel (float64, nx <= 4, nu <= 2, horizons whose factor fits LDS: N <= 64
                                      for nx = 4, nu = 1): TWO wavefronts per problem. One solves with the factor image
                                      `factor_slot` that a previous launch left in the workspace (as REUSE_FACTOR); the other,
                                      concurrently on another SIMD, factors the problem's operands as they are NOW into the
                                      other image, for the NEXT launch (which passes factor_slot ^ 1). The factor is still
                                      rebuilt once per launch -- what the reference's solve_mpc does every period,
                                      solve_mpc.py:42 -- but off the critical path. Contract: the operands A, B and the weights
                                      this launch sees are the ones the next launch will solve with (time-invariant or
                                      pre-scheduled dynamics); the first launch of a sequence uses KEEP_FACTOR.
                                      MPCQP_EUNSUPPORTED for other dimensions. */

#define MPCQP_OPT_SEED_VIOLATED 512 /* small-problem fused kernel (n <= 16, m <= 32): before the Goldfarb-Idnani iterations, the
                                 rows violated at the unconstrained minimiser enter by SEED STEPS (same rank-one updates, no
                                 selection, no ratio test; rows whose multiplier comes out negative leave again). Same
                                 minimiser; measured 5 % SLOWER than the plain iterations on BASELINE config 2,
                                 hence opt-in: the seed steps are what MPCQP_WARM_ACTIVE_SET starts from. */

#define MPCQP_OPT_EXACT_SELECTION 1024 /* accepted, no effect (ABI 11). Until ABI 10 it switched the wide stage-wise kernel from "lazy
                                 slacks" to a pass over the m slacks per step. Since round 6 that kernel never updates slacks
                                 incrementally: between two evaluations of the point it takes the most violated row among those
                                 whose whitened vectors the latest backward sweep cached (a valid Goldfarb-Idnani choice:
                                 same minimiser), see csrc/mpcqp_stagew.hip. */

#define MPCQP_OPT_TWO_PER_WAVE 2048 /* small-problem fused kernel: keep TWO problems per wavefront (mpcqp_pair.hip) where the
                                 dispatch would put FOUR on one (mpcqp_quad.hip: cold launches of problems with nx <= 16 and at
                                 most four rows per step -- BASELINE configs 1, 2, 4, the reference's WIP example -- from a few
                                 thousand problems up, see MPCQP_OPT_FOUR_PER_WAVE). Same method, same pivots: a cross-check
                                 (nx = 2 and nx >= 5 have no two-per-wavefront instantiation: the flag sends them to the one-per-wavefront kernel). */
#define MPCQP_OPT_STAGE_GENERAL 8192 /* mpcqp_stagewise_solve_batch: take the general stage-wise kernel (float64, nx <= 32, nu <= 8) also
                                 where the narrow or the wide one applies (a cross-check; until ABI 10 the formulation the host
                                 side re-solved through, when only this kernel kept a thin QR factor of the active rows -- the
                                 wide kernel does since ABI 11). MPCQP_EUNSUPPORTED for float32 and wider systems. */
#define MPCQP_OPT_FOUR_PER_WAVE 4096 /* ... and FOUR per wavefront for every batch size that kernel is eligible for (the dispatch
                                 takes it from more than two problems per SIMD of the device up: 2049 and more on an MI355X, where a
                                 wavefront per SIMD with four problems beats two wavefronts with two, and launches of several
                                 rounds keep two such wavefronts on every SIMD; smaller batches leave SIMDs idle either way;
                                 problems of 33 .. 64 rows with nx <= 8 run on its four-rows-per-lane build, mpcqp_quadg.hip, at
                                 every batch size).
                                 MPCQP_EUNSUPPORTED where the kernel does not apply (nx > 16, more than four rows per step -- eight with nx <= 8 --, warm
                                 starts, seed steps, a pairing order together with input rows / a stage cost). The shared-model solves (mpcqp_solve_model_batch / _bounds_batch) take
                                 it too, with the same batch-size rule, for every model with n <= 16, m <= 32. */

#define MPCQP_OPT_ON_CHIP_32 16384 /* mpcqp_build_solve_batch and the shared-model solves (below, after the fused launch's part):
                                 solve problems of 17 .. 32 variables on chip, TWO per wavefront
                                 (mpcqp_duo.hip: the dual active-set method of the small-problem kernels on 32-wide rows), instead of
                                 the stage-wise kernels the dispatch takes one step past n = 16. Replaces the same reference code as
                                 its siblings (qpmpc/mpc_qp.py:53-149 for the build, qpsolvers.solve_problem at qpmpc/solve_mpc.py:43
                                 for the solve). Envelope: cold fused build+solve, float64 (a float32 launch is converted and solved
                                 in float64 like every small problem), 17 <= n = N nu <= 32, m = N mk <= 64, 1 <= mk <= 4,
                                 2 <= nx <= 4; every operand layout of MpcqpProblem; lam and iters may be NULL; NO workspace (NULL is
                                 accepted whatever mpcqp_workspace_bytes reports -- the queries see no flags and answer as before).
                                 MPCQP_EUNSUPPORTED outside the envelope, with warm_state, order, MPCQP_OPT_SEED_VIOLATED, the
                                 FORCE_* / ONE_ / TWO_ / FOUR_PER_WAVE overrides and the *_FACTOR options. Additive in ABI 12.
                                 Where it is faster (MI355X, us per launch, flagged / default route on the same problems,
                                 profiles/onchip32.md): 4096 problems of (nx, nu, N, mk) = (3,1,17,2) 135 / 366,
                                 (3,1,20,2) 152 / 453, (3,1,24,2) 178 / 583, (3,1,32,2) 218 / 879, (4,2,12,2) 165 / 362,
                                 (4,2,16,2) 196 / 511, (3,1,20,3) 288 / 925; 1.9-4.0 x at 256, 4096 and 16384 problems alike.
                                 Shared-model solves (the kernel's MODEL mode: the rows of M and L^-T are read from what
                                 mpcqp_factor_model wrote, h and L^-1 q come from its linear maps; replaces update_cost_vector /
                                 update_constraint_vector + the solver call, mpc_qp.py:129-163). Envelope: float64,
                                 17 <= n <= 32, 1 <= m <= 64, ANY nx and ANY number of rows per step (the operands' layout no
                                 longer matters), cold. mpcqp_solve_model_bounds_batch with bounds per problem takes this kernel
                                 inside the envelope WITH OR WITHOUT the flag (nothing else serves those launches; at n <= 16 the
                                 small-problem kernels serve them as before and the flag changes nothing).
                                 mpcqp_solve_model_batch, and _bounds_batch with e == NULL, take it only with the flag: without
                                 it the launch goes where it always went (the workgroup kernel at these sizes); with it,
                                 MPCQP_EUNSUPPORTED outside the envelope (n <= 16 included), in float32, with warm_state or
                                 order, and next to MPCQP_OPT_FORCE_LDS, ONE_ / TWO_ / FOUR_PER_WAVE or SEED_VIOLATED.
                                 Figures: profiles/onchip32_model.md.
                                 QP given (mpcqp_solve_batch, the kernel's QP mode: packed P, q, G, h come through the LDS image to
                                 the lanes that own them, then the fused mode's elimination and iteration; replaces
                                 qpsolvers.solve_problem at qpmpc/solve_mpc.py:43). Envelope: float64, 1 <= n <= 32,
                                 1 <= m <= 64, cold; P is read in full and taken as symmetric; lam, status and iters may be
                                 NULL; NO workspace (NULL is accepted whatever mpcqp_solve_workspace_bytes reports). Taken only
                                 with the flag: without it the launch goes where it always went; with it, MPCQP_EUNSUPPORTED
                                 and nothing written for n > 32, m > 64, m == 0, float32, an order, a warm_state, and next to
                                 MPCQP_OPT_FORCE_LDS / _CONDENSED / _GWS / _DENSE_G, ONE_ / TWO_ / FOUR_PER_WAVE, SEED_VIOLATED
                                 or a *_FACTOR option. With mpcqp_condense_batch in front it is the on-chip route, in two
                                 launches, for problems of 17 .. 32 variables that the fused mode refuses (nx >= 5, more than
                                 four rows per step). Where it is faster (MI355X, us per launch, flagged / default route of
                                 mpcqp_solve_batch on the same problems, profiles/onchip32_qp.md): from seventeen variables up,
                                 where the default route is the workgroup kernel -- 4096 problems of (n, m) = (17, 33) 212 / 334,
                                 (24, 48) 309 / 948, (32, 64) 373 / 2362; 1.4-6.9 x at 256, 4096 and 16384 problems. At n <= 16
                                 it is SLOWER than the one-per-wavefront kernel the default route takes there ((16, 32):
                                 212 / 86 at 4096 problems, 0.35-0.46 x): the envelope starts at n = 1 so that one route serves
                                 whatever size a condensed problem has, not because it pays there. */

/* MpcqpSolveOpts.warm_start */
#define MPCQP_WARM_OPERATOR 1   /* begin from the stored active set AND operator N* (contract: matrices unchanged)          */
#define MPCQP_WARM_ACTIVE_SET 2 /* begin from the stored active set's ROW IDS only, moved by warm_shift rows: the rows enter
                                   by seed steps on THIS problem's matrices, so the matrices, bounds and states may all have
                                   changed -- the receding-horizon case, where row (k, i) of last period is row (k - 1, i)
                                   now: warm_shift = mk. Small-problem fused kernel only (MPCQP_EUNSUPPORTED elsewhere).   */

typedef struct MpcqpSolveOpts {
    int32_t max_iter; /* active-set iterations per problem; <=0 -> 10*(n+m)+10. One iteration is one step of the dual method (a row
                         admitted, or a blocking row dropped), counted per problem: a problem that takes `it` iterations is
                         solved under max_iter >= it and is MPCQP_MAX_ITER with iters[b] = max_iter below it (the narrow
                         stage-wise kernel's MPCQP_MAX_ITER items are solved again by the wide kernel under the same limit, and
                         iters[b] is then its count). */
    int32_t flags;    /* MPCQP_OPT_* (0 = automatic dispatch)                    */
    double feas_tol;  /* a row is violated when (h_i-G_i u)/(1+|h_i|) < -tol;
                         <=0 -> 1e-12 (f64) / 1e-5 (f32). The float32 dense condensed
                         kernels divide by |G_i|+|h_i| instead (Euclidean row norm):
                         the same verdict whatever units the row is stated in      */
    /* Warm start for receding-horizon loops (the reference reaches its backends' warm start through
     * **kwargs -> qpsolvers' initvals, qpmpc/solve_mpc.py:20,43; loops at
     * examples/wheeled_inverted_pendulum.py:99-118, examples/lipm_walking_controller.py:307-335).
     * warm_state: caller-owned DEVICE buffer of mpcqp_warm_state_bytes() per problem, packed by problem.
     *   When non-NULL every solve ENDS by storing its final active set and the active-set operator
     *   N* = (M_A M_A')^-1 M_A there (M = G L^-T); problems that were not solved store an empty set.
     * warm_start != 0: the solve BEGINS from the stored state instead of the empty set: multipliers are
     *   recomputed for the new q and h, rows whose multiplier turned negative leave, violated rows enter
     *   through the usual iterations -- a period whose active set moved by two rows costs about two
     *   iterations instead of one per active row.
     * Contract: N* depends on the matrices only, so the state is meaningful while A, B, C, D and the
     *   weights are those of the solve that stored it; e, x0, goal and targets may change freely. The
     *   contract is not trusted: with a warm start a solution is accepted only after its KKT conditions
     *   were re-checked from scratch (stationarity holds by construction, multipliers >= 0, active rows
     *   on their bounds, inactive rows feasible); a stale state costs a cold restart, never a wrong plan.
     * Supported by the small-problem fused kernel (n <= 16, m <= 32, float64) as described, and by the stage-wise kernel
     * that mpcqp_build_solve_batch picks for small systems with 16 < n <= 128 (float64, nx <= 4, nu <= 2): there the record
     * holds the active rows' ids only -- their vectors V_a = P^-1 g_a', the trajectories and W = (G_A P^-1 G_A')^-1 stay
     * in the WORKSPACE, so a warm start needs the same workspace as the launch before and MPCQP_OPT_REUSE_FACTOR (same
     * contract: matrices and weights unchanged); the multipliers are lam = -W s_A at the new unconstrained minimiser,
     * rows with a negative one leave, and a state whose active rows do not end up on their bounds (another problem's, or
     * another workspace's -- the record carries the workspace's address) costs a cold restart. Other dimensions return
     * MPCQP_EUNSUPPORTED when warm_state is given. */
    void *warm_state;
    int32_t warm_start;
    int32_t factor_slot; /* 0 | 1: the factor image of the stage-wise workspace that KEEP_FACTOR writes, REUSE_FACTOR and
                            PIPELINE_FACTOR read (PIPELINE_FACTOR writes the other one). 0 unless a loop alternates them. */
    /* Developer probe, NULL in production: DEVICE buffer of int64 per problem (16 for the small-problem
     * kernels, 32 for the mid-size / large ones) that receives shader-clock stamps at phase boundaries. */
    void *probe;
    /* Size in bytes of the buffer behind warm_state (ABI 6): a launch over `batch` problems needs
     * batch * mpcqp_warm_state_bytes(); a smaller buffer (a state allocated for another batch or other
     * dimensions) is refused with MPCQP_EWORKSPACE before anything is launched. Ignored when warm_state is NULL. */
    size_t warm_state_bytes;
    /* MPCQP_WARM_ACTIVE_SET (ABI 8): stored row id r is taken as row r - warm_shift of this launch's problem; ids that
     * fall off the horizon's start (or name a padded row) are dropped. 0: the rows kept their places.
     * (tests/test_gpu_padded_rows.py::test_small_kernel_warm_active_set_shifted_onto_padding and
     * ::test_wide_stagewise_active_set_record_shifted_onto_padding: stored ids that land on padded rows.) */
    int32_t warm_shift;
    int32_t reserved_;
    /* Pairing order (ABI 9), NULL = natural: DEVICE array of `batch` int32, a permutation of 0 .. batch-1. The small-problem
     * fused kernel (n <= 16, m <= 32) puts TWO problems on a wavefront, which then runs max(trips_a, trips_b) active-set trips --
     * 13.1 against 10.75 per problem on BASELINE config 4 (examples/humanoid_one_step.py:42-80 times 65,536). With an order,
     * half-wavefront i takes problem order[i]; outputs stay where they were (U, lam, status, iters are indexed by problem), every
     * problem's iterations are the same (the two halves of a wavefront sum in different orders: plans equal to rounding). A receding-horizon loop passes mpcqp_order_by_count() of last period's iteration counts
     * (qpmpc/solve_mpc.py:43 is called once per period, examples/lipm_walking_controller.py:307-335): launches of several rounds
     * get up to 12 % shorter, a launch that fills the machine once gains nothing. Cold launches of mpcqp_build_solve_batch and launches
     * of mpcqp_solve_model_batch / mpcqp_solve_model_bounds_batch that the small-problem kernel serves only: MPCQP_EUNSUPPORTED
     * with warm_state, with a dispatch override, for other dimensions and from every other entry point. The array is read during the launch (keep it alive until the stream has
     * passed it). It is not checked for being a permutation (a problem named twice is solved twice, one left out keeps its old
     * outputs); an index outside the batch is clamped into it. */
    const int32_t *order;
} MpcqpSolveOpts;

/* ABI version of the loaded library (== MPCQP_ABI_VERSION of its build). */
int mpcqp_abi_version(void);

/* Static text for a return code (<0: MPCQP_E*, >0: hipGetErrorString). */
const char *mpcqp_error_string(int code);

/* Dynamic LDS bytes one problem of these dimensions needs on the fused path;
 * MPCQP_ETOOLARGE when it exceeds the 160 KiB of a gfx950 CU (such problems take the
 * HBM-resident path and need a workspace). */
int mpcqp_lds_bytes(const MpcqpDims *dims, size_t *bytes);

/* Device scratch bytes that mpcqp_condense_batch (for_solve == 0) or
 * mpcqp_build_solve_batch (for_solve != 0) need for `batch` problems of these
 * dimensions: 0 for small problems solved entirely on chip; 2 n^2 elements per problem
 * (rows of the active-set operator) for the mid-size fused kernel; the propagators, P
 * and the same rows for large problems. The query sees dimensions only, so it reports the
 * largest amount any kernel the launch may pick (it depends on the operand strides) needs. */
int mpcqp_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t for_solve, size_t *bytes);

/* Same for mpcqp_solve_batch (n variables, m rows). */
int mpcqp_solve_workspace_bytes(int32_t n, int32_t m, int32_t dtype, int64_t batch, size_t *bytes);

/* Bytes per problem of MpcqpSolveOpts.warm_state for these dimensions (0: no warm start for them). */
int mpcqp_warm_state_bytes(const MpcqpDims *dims, size_t *bytes);

/* Whose record that buffer holds (ABI 10) -- the kernel mpcqp_build_solve_batch picks for these dimensions and this dtype (a
 * float32 launch of at most 160 variables is solved by the float64 kernels and keeps THEIR record):
 *   MPCQP_WARM_KIND_OPERATOR  small-problem fused kernel: the operator N* (16 x 16 float64, by slot), then 16 int32 constraint
 *                             ids (-1 = empty slot). MPCQP_WARM_OPERATOR and MPCQP_WARM_ACTIVE_SET.
 *   MPCQP_WARM_KIND_STAGE     narrow stage-wise kernel: int32 [count, slots, workspace tag (2), step of each row ..., index in its
 *                             step ...]; the rows' vectors stay in the launch's workspace (MPCQP_OPT_REUSE_FACTOR contract).
 *   MPCQP_WARM_KIND_ROWS      wide stage-wise kernel: int32 count, then the active rows' ids. MPCQP_WARM_ACTIVE_SET only.
 * A binding reads the layout from here instead of re-deriving the dispatch. */
#define MPCQP_WARM_KIND_NONE 0
#define MPCQP_WARM_KIND_OPERATOR 1
#define MPCQP_WARM_KIND_STAGE 2
#define MPCQP_WARM_KIND_ROWS 3
int mpcqp_warm_state_kind(const MpcqpDims *dims, int32_t *kind);

/* Replaces MPCQP.__init__ (mpc_qp.py:39-122) for a batch: Phi/Psi propagation
 * (:53-54,:88-90), G_k/h_k (:62-78), P (:99-105), q (:129-149).
 * Outputs per problem, packed: P[n*n], q[n], G[m*n], h[m];
 * Phi[(N+1)*nx*nx] (blocks Phi_0..Phi_N; the last one is phi_last) and
 * Psi[(N+1)*nx*n]  (blocks Psi_0..Psi_N; the last one is psi_last) may be NULL. */
int mpcqp_condense_batch(const MpcqpDims *dims, const MpcqpProblem *problem,
                         int64_t batch, void *P, void *q, void *G, void *h,
                         void *Phi, void *Psi, void *workspace,
                         size_t workspace_bytes, void *stream);

/* The two launches of mpcqp_condense_batch for problems that do not fit a CU's LDS (BASELINE config 5's size), one at a
 * time -- for measurement (bench.py times the Gram product alone: `roofline.gram_mfma`) and for callers that overlap them
 * with other work. phase 1 replaces the propagation loop of MPCQP.__init__ (qpmpc/mpc_qp.py:53-98): Psi (caller's buffer,
 * same packing as mpcqp_condense_batch), G, h and the tracking residuals (workspace: (N + 1) nx elements per problem).
 * phase 2 replaces the Hessian and cost-vector products (qpmpc/mpc_qp.py:99-105, 129-149): P = w_u I + Psi' W Psi and
 * q = Psi' W resid from what phase 1 left in Psi and the workspace -- float32 with n a multiple of 32: on the matrix cores
 * (v_mfma_f32_32x32x2_f32, the causal lower triangle only). MPCQP_EUNSUPPORTED for problems the on-chip kernel condenses. */
int mpcqp_condense_phase_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t phase,
                               void *P, void *q, void *G, void *h, void *Psi, void *workspace,
                               size_t workspace_bytes, void *stream);

/* Replaces MPCQP.update_cost_vector (mpc_qp.py:129-149) and
 * MPCQP.update_constraint_vector (mpc_qp.py:151-163) for a batch, from the
 * Phi/Psi kept by mpcqp_condense_batch (same packing; batch strides
 * phi_batch_stride/psi_batch_stride in elements, 0 = one shared copy) and new
 * x0/goal/targets. Reads problem->C, ->e, ->x0, ->goal, ->targets only.
 * q and/or h may be NULL to skip that update. */
int mpcqp_update_vectors_batch(const MpcqpDims *dims, const MpcqpProblem *problem,
                               const void *Phi, int64_t phi_batch_stride,
                               const void *Psi, int64_t psi_batch_stride,
                               int64_t batch, void *q, void *h, void *stream);

/* Replaces qpsolvers.solve_problem(Problem(P,q,G,h), solver=...) at its call
 * site qpmpc/solve_mpc.py:43 for a batch of dense strictly convex QPs:
 * x[batch*n], lam[batch*m] (multipliers of G u <= h, nullable),
 * status[batch], iters[batch] (nullable). Dual active-set method.
 * A problem with status[b] != 0 gets x[b] = zeros and its status and iters; its lam[b] is undefined. The workspace's initial
 * content is never read.
 * MPCQP_OPT_ON_CHIP_32 in opts->flags sends a float64 launch of 1 <= n <= 32, 1 <= m <= 64 to the on-chip kernel of
 * mpcqp_duo.hip (two problems per wavefront; workspace may be NULL, status may be NULL too) instead of the one-per-wavefront
 * (n <= 16) and workgroup kernels, and is MPCQP_EUNSUPPORTED, with nothing written, for every other launch (see the flag);
 * without the flag nothing changes. */
int mpcqp_solve_batch(int32_t n, int32_t m, int32_t dtype, const void *P,
                      const void *q, const void *G, const void *h, int64_t batch,
                      const MpcqpSolveOpts *opts, void *x, void *lam,
                      int32_t *status, int32_t *iters, void *workspace,
                      size_t workspace_bytes, void *stream);

/* Replaces the whole of solve_mpc (qpmpc/solve_mpc.py:42-44) for a batch, fused:
 * P, G and their factors never leave the CU. U[batch*n] is the stacked input
 * sequence (Plan.inputs = U.reshape(N, nu), plan.py:36-39).
 * status[b] is what an exact backend of the reference would report (found / not found, plan.py:35-40): problems of 17 .. 128
 * variables with nx <= 4, nu <= 2 -- the narrow stage-wise kernel, whose active-set operator is an explicit inverse -- that this
 * kernel leaves MPCQP_MAX_ITER or MPCQP_INFEASIBLE are solved once more by the wide stage-wise kernel (thin QR factor of the
 * active rows) in a second launch on the same stream, before the call returns (ABI 11). Stateful launches -- MPCQP_OPT_KEEP_FACTOR /
 * _REUSE_FACTOR / _PIPELINE_FACTOR, a warm state -- take it too: the wide kernel works in a region of the workspace after the narrow
 * kernel's (mpcqp_workspace_bytes prices the sum), so the factor images and the rows a warm record points at survive it, and it
 * leaves the warm record as the narrow kernel wrote it (the next warm start re-checks it). For an item the wide kernel re-solved,
 * U, lam, status and iters are the wide kernel's: iters counts its iterations only, the narrow kernel's are not added. The
 * multi-period launches (mpcqp_wip_periods_batch) have no second opinion.
 * A problem with status[b] != 0 gets U[b] = zeros and its status and iters; its lam[b] is undefined. lam and iters may be NULL.
 * The initial content of the workspace and of a cold launch's warm_state is never read (MPCQP_OPT_REUSE_FACTOR /
 * _PIPELINE_FACTOR and warm_start != 0 read what the launch before left there, as documented at MpcqpSolveOpts). */
int mpcqp_build_solve_batch(const MpcqpDims *dims, const MpcqpProblem *problem,
                            int64_t batch, const MpcqpSolveOpts *opts, void *U,
                            void *lam, int32_t *status, int32_t *iters,
                            void *workspace, size_t workspace_bytes, void *stream);

/* ---- stage-wise (uncondensed) formulation: long horizons -------------------------------------
 * The reference has no sparse formulation: sparse=True only wraps the dense condensed matrices in CSC
 * (qpmpc/mpc_qp.py:39,108-109; qpmpc/solve_mpc.py:31-32), so its build is O(N^2) memory, O(N^3) time.
 * This entry point solves the same QP as mpcqp_build_solve_batch -- same operands, same outputs, same
 * minimiser -- without forming P or G: Riccati gains once per problem, then per active-set iteration
 * one LQR solve (two sweeps over the horizon) and O(|A| N) vector work; O(N) memory. No cap on
 * N; float64 with 2 <= nx <= 4, 1 <= nu <= 2 (chunked scans over the horizon), or float64 / float32 with nx <= 16,
 * nu <= 4 (matrix-core sweeps; MPCQP_EUNSUPPORTED otherwise). `max_active` bounds the number of simultaneously active
 * rows (<= 0: min(n, m, 128)); a problem that needs more returns status MPCQP_SLOTS_FULL. The workspace is caller-owned
 * (mpcqp_stagewise_workspace_bytes). mpcqp_build_solve_batch reaches the same kernels by itself for every problem that
 * does not fit the on-chip condensed kernels (any n = N nu). MPCQP_OPT_STAGE_GENERAL asks for the general kernel (float64,
 * nx <= 32, nu <= 8: thin-QR active-set operator, like the wide kernel's since ABI 11) whatever
 * the width; its workspace is sized by the query with max_active = -1 (default slots) or -k (k slots). As in
 * mpcqp_build_solve_batch, what the narrow kernel leaves MPCQP_MAX_ITER / MPCQP_INFEASIBLE is solved once more by the wide kernel
 * (same slots, same stream, its own region after the narrow kernel's workspace: the query reports the sum) before the call
 * returns, stateful launches included; iters of such an item is the wide kernel's count.
 * A problem with status[b] != 0 (MPCQP_SLOTS_FULL included) gets U[b] = zeros and its status and iters; its lam[b] is undefined.
 * The workspace's initial content is never read, the stateful sequences of mpcqp_build_solve_batch apart. */
int mpcqp_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active, size_t *bytes);
int mpcqp_stagewise_solve_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                                const MpcqpSolveOpts *opts, int32_t max_active, void *U, void *lam,
                                int32_t *status, int32_t *iters, void *workspace, size_t workspace_bytes,
                                void *stream);

/* ---- shared-model path: build once, re-solve for new states ----------------------
 * The reference's own fast path (doc/src/developer-notes.rst:10, CHANGELOG.md:12,44):
 * build MPCQP once, then only update_cost_vector / update_constraint_vector
 * (mpc_qp.py:129-163) and re-solve. When A, B, C, D, e and the weights are the same for
 * every problem of a batch (an initial-state sweep, or successive steps of
 * time-invariant receding-horizon loops), everything that does not depend on
 * x0/goal/targets is computed ONCE into a "model": L = chol(P), M = G L^-T, L^-T and
 * the linear maps  h = e - Hx x0,  L^-1 q = Wx x0 - Wg goal - Wt targets.
 *
 * The model is filled from condensed data of 1 + 2 nx + N nx PSEUDO-problems sharing the
 * operands (mpcqp_condense_batch on them): pseudo-problem 0 has x0 = goal = targets = 0,
 * then x0 = e_c (c < nx), then goal = e_c, then targets = e_j (j < N nx):
 *   P, G        [n*n], [m*n]        of pseudo-problem 0
 *   q_basis     [(1+2nx+N nx) * n]  their q vectors, in that order
 *   h_basis     [(1+2nx+N nx) * m]  their h vectors                                      */
int mpcqp_model_bytes(const MpcqpDims *dims, size_t *bytes);
int mpcqp_factor_model(const MpcqpDims *dims, const void *P, const void *G,
                       const void *q_basis, const void *h_basis, void *model,
                       size_t model_bytes, void *stream);

/* Solve `batch` problems that share `model`: only x0 [nx], goal [nx] and targets [N nx]
 * differ (batch_stride 0 = shared; goal/targets may be NULL when their cost term is
 * not flagged). Replaces update_cost_vector + update_constraint_vector + the solver
 * call for every problem. Outputs as mpcqp_build_solve_batch: U[b] = zeros, status and iters for a problem with status[b] != 0,
 * its lam[b] undefined; lam and iters may be NULL. `model` is only read; there is no workspace.
 * MPCQP_OPT_ON_CHIP_32 in opts->flags sends a float64 launch of 17 <= n <= 32, 1 <= m <= 64 to the on-chip kernel of
 * mpcqp_duo.hip (two problems per wavefront) instead of the workgroup kernel, and is MPCQP_EUNSUPPORTED for every other
 * launch (see the flag); without the flag nothing changes. */
int mpcqp_solve_model_batch(const MpcqpDims *dims, const void *model,
                            const MpcqpOperand *x0, const MpcqpOperand *goal,
                            const MpcqpOperand *targets, int64_t batch,
                            const MpcqpSolveOpts *opts, void *U, void *lam,
                            int32_t *status, int32_t *iters, void *stream);

/* As mpcqp_solve_model_batch, with the inequality vectors e given PER PROBLEM ([batch, N|1, mk] through `e`'s strides)
 * instead of taken from the model: the matrices are shared and constant, the bounds move -- the per-step ZMP bounds
 * that examples/lipm_walking_controller.py:179-213 (update_goal_and_constraints) rewrites every control period while
 * A, B, C stay, i.e. update_constraint_vector (mpc_qp.py:151-163) with a new e. h = e - (C Phi) x0 uses the model's map.
 * e == NULL or e->ptr == NULL is mpcqp_solve_model_batch. Served by the small-problem kernels (n <= 16, m <= 32, float64)
 * and, for float64 models of 17 <= n <= 32 with 1 <= m <= 64 (any nx, any number of rows per step), by the MODEL mode of
 * mpcqp_duo.hip -- with or without MPCQP_OPT_ON_CHIP_32, cold, with no order and none of MPCQP_OPT_FORCE_LDS, ONE_ / TWO_ /
 * FOUR_PER_WAVE, SEED_VIOLATED; MPCQP_EUNSUPPORTED elsewhere (float32 past sixteen variables, n > 32, m > 64). Outputs
 * for unsolved problems as mpcqp_solve_model_batch. */
int mpcqp_solve_model_bounds_batch(const MpcqpDims *dims, const void *model, const MpcqpOperand *e,
                                   const MpcqpOperand *x0, const MpcqpOperand *goal,
                                   const MpcqpOperand *targets, int64_t batch,
                                   const MpcqpSolveOpts *opts, void *U, void *lam,
                                   int32_t *status, int32_t *iters, void *stream);

/* Replaces MPCProblem.integrate (mpc_problem.py:316-335) as used by Plan.states
 * (plan.py:81-109) for a batch: X[batch*(N+1)*nx], X_0 = x0,
 * X_{k+1} = A_k X_k + B_k U_k. U is packed [batch*N*nu]. */
int mpcqp_rollout_batch(const MpcqpDims *dims, const MpcqpOperand *A,
                        const MpcqpOperand *B, const MpcqpOperand *x0,
                        const void *U, int64_t batch, void *X, void *stream);

/* Vector-Jacobian product of solved plans (ABI 12). The reference has no gradients; this is an extension for callers who
 * learn through the controller. Given the forward solve's multipliers lam [batch*m] and status [batch]
 * (mpcqp_build_solve_batch / mpcqp_stagewise_solve_batch with lam != NULL), gU = dL/dU [batch*n] and gX = dL/dX
 * [batch*(N+1)*nx] (nullable; X = the rollout of mpcqp_rollout_batch), writes per problem, packed:
 *     g_x0 [nx], g_goal [nx], g_targets [N*nx], g_e [N*mk]   (all but g_x0 nullable)
 * with respect to that problem's own x0, goal, targets and e; a reduction over operands the batch shares is the caller's.
 * The active set is {i : lam_i > 0}: a row that is tight with lam_i = 0 counts as inactive, so at weakly active points
 * the result is one element of the generalized Jacobian. Terms follow dims->flags (MPCQP_Q_TERMINAL / MPCQP_Q_STAGE): a
 * goal or targets that do not enter q get zero gradients.
 * Per problem: status[b] != 0 gives all-zero gradients and vjp_status[b] = status[b]; more active rows than variables or
 * a Gram matrix of the active rows that is not positive definite gives zeros and MPCQP_NOT_PD; else vjp_status[b] = 0.
 * Dependent and weakly active rows -- the contract of the plan and shared-model derivative exports below
 * (mpcqp_plan_vjp* / mpcqp_plan_jvp* / mpcqp_model_vjp_batch / mpcqp_model_jvp_batch; tests/test_gpu_degenerate_diff.py):
 *  - "not positive definite" is decided relative to the rows: pivot j of the Gram matrix S = M_A M_A' of the whitened active
 *    rows must exceed 4 (n + k + 1) 2^-53 S_jj, k the number of active rows (the rounding a Cholesky pivot of an exactly
 *    row that is a multiple of one other active row can carry, whichever comes first; DESIGN.md section 9, "Dependent and
 *    weakly active rows"). An active row that is a multiple of another active row -- a row stated twice, a row and a multiple
 *    of it, both halves of an equality written as two inequalities, each with a positive multiplier -- is therefore
 *    MPCQP_NOT_PD with zeros, whatever the sign of the rounding: never status 0 on a division by noise. The bound does not
 *    cover a row that is a combination of several other active rows: there the verdict can still depend on rounding.
 *    mpcqp_model_periods_vjp_batch is the exception: its factorisation keeps the plain test, pivot > 0.
 *  - no forward route of this library returns such multipliers: the solvers keep an independent active set, so at a binding
 *    pair one member carries the whole multiplier. The gradients with respect to x0, goal and targets, g_e off the pair and
 *    g_e[i0] + f g_e[i1] on a pair with G_i1 = f G_i0 do not depend on which member that is, and equal the derivative of the
 *    solution map (which is differentiable there); a lone g_e[i0] or g_e[i1] depends on the member, and a tangent of e gets
 *    the unique response where it moves the pair together, de[i1] = f de[i0].
 *  - a row that is tight with lam_i = 0 (a bound through the optimum) is inactive: one element of the generalized Jacobian, the
 *    derivative of the problem without that row. With no positive multiplier at all that is the unconstrained derivative.
 * Envelope: float64 (MPCQP_EDTYPE otherwise), n <= 128 and whatever mpcqp_condense_batch condenses (MPCQP_EUNSUPPORTED
 * otherwise). The call runs mpcqp_condense_batch (Phi, Psi kept) into the workspace, then one adjoint launch. */
int mpcqp_plan_vjp_workspace_bytes(const MpcqpDims *dims, int64_t batch, size_t *bytes);
int mpcqp_plan_vjp_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                         const void *lam, const int32_t *status, const void *gU, const void *gX,
                         void *g_x0, void *g_goal, void *g_targets, void *g_e, int32_t *vjp_status,
                         void *workspace, size_t workspace_bytes, void *stream);

/* Outputs of mpcqp_plan_vjp_model_batch, every pointer nullable; per problem, packed per step whatever the operand
 * strides: the four of mpcqp_plan_vjp_batch, then
 *     g_A [N*nx*nx], g_B [N*nx*nu], g_C [N*mk*nx], g_D [N*mk*nu], g_w [3] (terminal, stage, input weight). */
typedef struct MpcqpVjpModelOut {
    void *g_x0, *g_goal, *g_targets, *g_e;
    void *g_A, *g_B, *g_C, *g_D, *g_w;
} MpcqpVjpModelOut;

/* As mpcqp_plan_vjp_batch, with gradients also with respect to that problem's A_k, B_k, C_k, D_k (an absent C or D: the
 * gradient at zero) and the three cost weights; an additive part of ABI 12 (MPCQP_ABI_VERSION is unchanged). U is the
 * forward plan [batch*n]. The four outputs shared with mpcqp_plan_vjp_batch are bitwise those it writes; envelope,
 * status and vjp_status rules are its own, and unsolved problems get zeros in every output. A cost term follows
 * dims->flags: a P term without its q term (weight set, goal or targets not) weighs the forced response Psi U, a weight
 * whose P term is not flagged gets 0. Reductions over operands the batch or the steps share are the caller's. The
 * workspace holds mpcqp_plan_vjp_batch's and the longer carve of this launch (its own size query). */
int mpcqp_plan_vjp_model_workspace_bytes(const MpcqpDims *dims, int64_t batch, size_t *bytes);
int mpcqp_plan_vjp_model_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                               const void *lam, const int32_t *status, const void *U, const void *gU,
                               const void *gX, const MpcqpVjpModelOut *out, int32_t *vjp_status,
                               void *workspace, size_t workspace_bytes, void *stream);

/* The stage-wise adjoint: mpcqp_plan_vjp_model_batch's products at any horizon, without condensing; an additive part of
 * ABI 12 (MPCQP_ABI_VERSION is unchanged). The same KKT adjoint on A = {i : lam_i > 0} is solved on the Riccati
 * recursion of each problem in whitened coordinates (P = L L' block-wise, DESIGN.md section 9 "Stage-wise adjoint"): one
 * backward sweep for L^-1 (gU + Psi' gX), one per active row for its whitened vector, the active rows' Gram matrix and its
 * Cholesky factor, then one forward sweep for L^-T; the gradients follow from costate recursions over A_k (section 9's
 * formulas for v, g_x0, g_goal, g_targets, g_e and, for the model and cost gradients, the rollouts X, Z and the costates
 * p, pz, s). Outputs are those of mpcqp_plan_vjp_model_batch, every pointer of `out` nullable; when g_A .. g_w are all
 * NULL the model phase is skipped and U may be NULL. `max_active` (>= 0) bounds |A| per problem and sizes the workspace:
 * a problem with more active rows gets zeros and vjp_status MPCQP_SLOTS_FULL. Otherwise the status and vjp_status rules
 * are mpcqp_plan_vjp_batch's (unsolved: zeros and its status; more active rows than variables, a stage Hessian or a Gram
 * matrix that is not positive definite: zeros and MPCQP_NOT_PD). Envelope: float64 (MPCQP_EDTYPE otherwise), nx <= 32,
 * nu <= 8 (MPCQP_EUNSUPPORTED otherwise), any N. The workspace is batch regions of the size the query reports. */
int mpcqp_plan_vjp_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active, size_t *bytes);
int mpcqp_plan_vjp_stagewise_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                                   int32_t max_active, const void *lam, const int32_t *status, const void *U,
                                   const void *gU, const void *gX, const MpcqpVjpModelOut *out,
                                   int32_t *vjp_status, void *workspace, size_t workspace_bytes, void *stream);

/* Jacobian-vector products of solved plans, the forward-mode counterpart of mpcqp_plan_vjp_batch; an additive part of
 * ABI 12 (MPCQP_ABI_VERSION is unchanged). Tangents of x0, goal, targets and e, ntan of them per problem (1 .. 256), each
 * pointer nullable (a NULL tangent is zero). Within one problem tangent t sits at offset t*nx (dx0, dgoal), t*N*nx
 * (dtargets) or t*N*mk (de); a stride is the number of elements between two problems' tangents, 0 = one set shared by
 * the batch (one identity gives the Jacobian of every problem). */
typedef struct MpcqpTangents {
    const void *dx0, *dgoal, *dtargets, *de;
    int64_t dx0_stride, dgoal_stride, dtargets_stride, de_stride;
} MpcqpTangents;

/* On the active set A = {i : lam_i > 0} of the forward solve (lam, status as for mpcqp_plan_vjp_batch), the plan is affine
 * in its data; this writes, packed, dU [batch][ntan][n] and dX [batch][ntan][(N+1)*nx] (nullable) for every tangent:
 *     dq = w_t psi_N'(phi_N dx0 - dgoal) + w_x Psi'(Phi dx0 - dtargets)    (terms as dims->flags has them)
 *     dh = de - C Phi dx0,   [P G_A'; G_A 0] [dU; dlam_A] = [-dq; dh_A],   dX = Phi dx0 + Psi dU
 * ("Forward sensitivities"). With dx0 the identity, dU is the feedback Jacobian dU/dx0 whose first
 * block is the local gain of the controller. At weakly active points the result is one element of the generalized
 * Jacobian, as for the VJP. Per problem: status[b] != 0 gives zeros and jvp_status[b] = status[b]; more active rows than
 * variables or a Gram matrix of the active rows that is not positive definite gives zeros and MPCQP_NOT_PD; else
 * jvp_status[b] = 0 (jvp_status nullable). Checks: MPCQP_EDTYPE unless float64; MPCQP_EUNSUPPORTED for n > 128 (or what
 * mpcqp_condense_batch does not condense); MPCQP_EINVAL for ntan outside 1 .. 256, a NULL tan, status or dU, a negative
 * stride, or a NULL lam when mk > 0; MPCQP_EWORKSPACE for a missing or short workspace. The call runs
 * mpcqp_condense_batch into the workspace, then one tangent launch (one workgroup per problem). */
int mpcqp_plan_jvp_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t ntan, size_t *bytes);
int mpcqp_plan_jvp_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t ntan,
                         const void *lam, const int32_t *status, const MpcqpTangents *tan,
                         void *dU, void *dX, int32_t *jvp_status,
                         void *workspace, size_t workspace_bytes, void *stream);

/* The stage-wise tangent: mpcqp_plan_jvp_batch's products at any horizon, without condensing; an additive part of ABI 12
 * (MPCQP_ABI_VERSION is unchanged). The same KKT system on A = {i : lam_i > 0} is solved on the Riccati recursion of each
 * problem in whitened coordinates, as mpcqp_plan_vjp_stagewise_batch solves its adjoint ("Stage-wise
 * forward sensitivities"): the factorisation, the active rows' whitened vectors, their Gram matrix and its Cholesky factor
 * once per problem; then per tangent the rollout xs of dx0, one backward sweep for r = -L^-1 dq, the multipliers
 * mu = S^-1 (Y_A r - dh_A) and one forward sweep for dU = L^-T (r - Y_A' mu), dX = xs + Psi dU, 256 / max(nx, nu) tangents
 * side by side. Inputs, outputs, packing, strides (0 = shared by the batch) and the nullable pointers are
 * mpcqp_plan_jvp_batch's; `max_active` (>= 0) bounds |A| per problem and sizes the workspace as for
 * mpcqp_plan_vjp_stagewise_batch: a problem with more active rows gets zeros and jvp_status MPCQP_SLOTS_FULL. Otherwise
 * per problem: status[b] != 0 gives zeros and jvp_status[b] = status[b] (its multipliers are not read); more active rows
 * than variables, a stage Hessian or a Gram matrix that is not positive definite gives zeros and MPCQP_NOT_PD; else 0.
 * Checks, before anything is launched: MPCQP_EINVAL for a negative batch or max_active; MPCQP_EDTYPE unless float64;
 * MPCQP_EUNSUPPORTED for nx > 32 or nu > 8 (any N is served); MPCQP_EINVAL for ntan outside 1 .. 256, a NULL tan, status
 * or dU, a negative stride, or a NULL lam when mk > 0; MPCQP_EWORKSPACE for a missing or short workspace. The workspace
 * is batch regions of the size the query reports (it grows with max_active and, up to one pass of tangents, with ntan). */
int mpcqp_plan_jvp_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active, int32_t ntan,
                                             size_t *bytes);
int mpcqp_plan_jvp_stagewise_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                                   int32_t max_active, int32_t ntan, const void *lam, const int32_t *status,
                                   const MpcqpTangents *tan, void *dU, void *dX, int32_t *jvp_status,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* Tangents of the model matrices and the cost weights, beside MpcqpTangents; an additive part of ABI 12
 * (MPCQP_ABI_VERSION is unchanged). Every pointer nullable (NULL = zero); packed per step: within one problem tangent t of
 * dA sits at offset t*N*nx*nx ([ntan][N][nx][nx]), of dB at t*N*nx*nu, of dC at t*N*mk*nx, of dD at t*N*mk*nu and of dw at
 * t*3 (dw_t, dw_x, dw_u: terminal, stage, input, the order of g_w). A stride is the number of elements between two
 * problems' tangents, 0 = one set shared by the batch. A tangent of a C or D the problem does not have is the tangent at
 * zero, as for the VJP; a weight whose P term dims->flags does not have contributes nothing. */
typedef struct MpcqpModelTangents {
    const void *dA, *dB, *dC, *dD, *dw;
    int64_t dA_stride, dB_stride, dC_stride, dD_stride, dw_stride;
} MpcqpModelTangents;

/* mpcqp_plan_jvp_batch / mpcqp_plan_jvp_stagewise_batch with tangents of A, B, C, D and the weights as well. At the plan
 * (U, lam) on A = {i : lam_i > 0}, with X = rollout(x0, U), Z = rollout(0, U) and E_k = X_k - r_k where the q term is
 * flagged, Z_k where only the P term is, 0 where neither (E_N likewise with the goal), the costate of stationarity is
 *     s_k = w_x E_k + C_k' lam_k (k < N),  s_N = w_t E_N,   pi_N = s_N,  pi_k = s_k + A_k' pi_{k+1}
 * (0 = w_u u_k + B_k' pi_{k+1} + D_k' lam_k), and per tangent, U and lam held fixed:
 *     xs_0 = dx0,  xs_{k+1} = A_k xs_k + dA_k X_k + dB_k u_k          (zs the same from 0 with Z_k: a P-only term's)
 *     dE_k = xs_k - dtargets_k (MPCQP_Q_STAGE) | zs_k (MPCQP_P_STAGE only) | 0;   dE_N likewise with dgoal
 *     c_k  = [P_STAGE] dw_x E_k + w_x dE_k + dC_k' lam_k + dA_k' pi_{k+1} (k < N),   c_N = [P_TERMINAL] dw_t E_N + w_t dE_N
 *     g_k  = dw_u u_k + dB_k' pi_{k+1} + dD_k' lam_k,   dq = Psi' c + g
 *     dh_k = de_k - C_k xs_k - dC_k X_k - dD_k u_k
 *     [P G_A'; G_A 0] [dU; dlam_A] = [-dq; dh_A],   dX = xs + Psi dU
 * ("Model and weight tangents"). `U` is the plan [batch][n]; `tan` may be NULL when `mtan` is not and
 * the other way round. Envelope, checks, their order, status and jvp_status rules, outputs and workspace rules are those
 * of the export without `_model`; in addition MPCQP_EINVAL for a NULL U, for tan and mtan both NULL or without any
 * non-NULL tangent between them, or a negative stride. With every pointer of mtan NULL (or mtan NULL) the call launches
 * what the export without `_model` launches and its outputs are bitwise the same. The workspace queries are their own
 * (the carve holds X, Z, pi and zs as well). */
int mpcqp_plan_jvp_model_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t ntan, size_t *bytes);
int mpcqp_plan_jvp_model_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t ntan,
                               const void *lam, const int32_t *status, const void *U, const MpcqpTangents *tan,
                               const MpcqpModelTangents *mtan, void *dU, void *dX, int32_t *jvp_status,
                               void *workspace, size_t workspace_bytes, void *stream);
int mpcqp_plan_jvp_model_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active,
                                                   int32_t ntan, size_t *bytes);
int mpcqp_plan_jvp_model_stagewise_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                                         int32_t max_active, int32_t ntan, const void *lam, const int32_t *status,
                                         const void *U, const MpcqpTangents *tan, const MpcqpModelTangents *mtan,
                                         void *dU, void *dX, int32_t *jvp_status,
                                         void *workspace, size_t workspace_bytes, void *stream);

/* ---- derivatives of shared-model plans: no second build, no workspace; an additive part of ABI 12
 * (MPCQP_ABI_VERSION is unchanged). What mpcqp_plan_vjp_batch / mpcqp_plan_jvp_batch compute, for problems that share a
 * factored model, from the model itself: they replace those exports' condensing of every problem (P, q, G, h, Phi, Psi
 * into a workspace) and factorisation of every P by products with the model's M = G L^-T, L^-T and maps. With
 * d = L^-1 q = Wx x0 - Wg goal - Wt targets, h = e - Hx x0 and S = M_A M_A' on A = {i : lam_i > 0} (the rule of every
 * derivative export: a tight row with lam_i = 0 is inactive, the result is one element of the generalized Jacobian),
 *     VJP:  t = L^-1 (gU + Psi' gX),  nu = S^-1 M_A t,  w = t - M_A' nu,
 *           g_x0 = -Wx' w - Hx' nu + p_0,  g_goal = Wg' w,  g_targets = Wt' w,  g_e = nu on A, 0 elsewhere
 *     JVP:  r = -(Wx dx0 - Wg dgoal - Wt dtargets),  mu = S^-1 (M_A r - (de - Hx dx0)_A),  dU = L^-T (r - M_A' mu),
 *           dX = rollout(dx0, dU)
 * ("Shared-model derivatives"). Psi' gX and p_0 come from the costate recursion p_N = gX_N,
 * p_k = gX_k + A_k' p_{k+1}, (Psi' gX)_k = B_k' p_{k+1}, and dX from the rollout, through A and B as operands (the model
 * holds neither Phi nor Psi; a batch stride of 0 shares them): A and B are read only when gX (dX) is not NULL.
 * `model` is what mpcqp_factor_model wrote for the same dims and is only read; lam [batch*m] and status [batch] are the
 * forward's (mpcqp_solve_model_batch / mpcqp_solve_model_bounds_batch with lam != NULL). Per-problem bounds need nothing
 * more: at a given active set the derivative depends on neither e nor x0. Terms follow dims->flags: a goal or targets that
 * do not enter q get zero gradients, and their tangents contribute nothing.
 * Inputs and outputs, packed: gU [batch*n], gX [batch*(N+1)*nx] (nullable), g_x0 [batch*nx], g_goal [batch*nx],
 * g_targets [batch*N*nx], g_e [batch*N*mk] (all but g_x0 nullable); the tangents, their layout ([batch][ntan][...], a
 * stride of 0 = one set shared by the batch), ntan in 1 .. 256, dU [batch][ntan][n] and dX [batch][ntan][(N+1)*nx]
 * (nullable) are mpcqp_plan_jvp_batch's. A reduction over operands the batch shares is the caller's.
 * Per problem: status[b] != 0 gives zeros in every output and vjp_status[b] / jvp_status[b] = status[b] (its multipliers
 * are not read); more active rows than variables, or an S that is not positive definite (the pivot test of the other
 * derivative exports), gives zeros and MPCQP_NOT_PD; a model whose factorisation failed gives every problem zeros and
 * MPCQP_NOT_PD; else 0. vjp_status and jvp_status are nullable.
 * Checks, before anything is launched: MPCQP_EDTYPE unless float64; MPCQP_EUNSUPPORTED for n > 64 (such problems have
 * mpcqp_plan_vjp_batch / mpcqp_plan_jvp_batch) and for a state so wide that the workgroup kernel's vectors do not fit a
 * CU's LDS beside S (8 (n (n | 1) + 4 n + 2 nx + n / 2 + 1) bytes > 160 KiB: nx beyond some ten thousand); MPCQP_EINVAL for a NULL model, status, gU, g_x0, dU or tan, a negative
 * batch, a NULL lam when mk > 0, a non-NULL gX or dX without A or B, a negative stride, or ntan outside 1 .. 256.
 * Models of at most 16 variables, 32 rows and nx <= 16 run sixteen lanes per problem, four problems per wavefront, on an
 * LDS image of the model staged once per workgroup (at most 1024 workgroups of sixteen problems a round: larger batches
 * take further rounds); the others one workgroup per problem with S in LDS. */
int mpcqp_model_vjp_batch(const MpcqpDims *dims, const void *model, int64_t batch, const void *lam,
                          const int32_t *status, const void *gU, const void *gX, const MpcqpOperand *A,
                          const MpcqpOperand *B, void *g_x0, void *g_goal, void *g_targets, void *g_e,
                          int32_t *vjp_status, void *stream);
int mpcqp_model_jvp_batch(const MpcqpDims *dims, const void *model, int64_t batch, int32_t ntan, const void *lam,
                          const int32_t *status, const MpcqpTangents *tan, const MpcqpOperand *A,
                          const MpcqpOperand *B, void *dU, void *dX, int32_t *jvp_status, void *stream);

/* One period of `batch` wheeled-inverted-pendulum control loops, fused: apply the first
 * input of each plan (U[b*u_stride]) to the nonlinear plant for `nsub` Taylor sub-steps of
 * sampling_period/nsub (WheeledInvertedPendulum.integrate,
 * qpmpc/systems/wheeled_inverted_pendulum.py:127-160, called from
 * examples/wheeled_inverted_pendulum.py:110-111), then write the next MPC problem's
 * x0 [4], goal [4] and targets [N*4] reference ramp (get_target_states, same example
 * :65-83,:101-108). states [batch*4] is updated in place; a loop whose plan was not
 * found (status[b] != 0, may be NULL) applies a zero input. nsub = 0 leaves the plant where
 * it is and writes the problem of the CURRENT state (the first problem of an episode). */
int mpcqp_wip_advance_batch(int32_t dtype, void *states, const void *U, int64_t u_stride,
                            const int32_t *status, int32_t N, double sampling_period,
                            double target_vel, double length, double gravity, int32_t nsub,
                            void *x0, void *goal, void *targets, int64_t batch, void *stream);

/* The same with the loops' bookkeeping fused in (one launch per period instead of two): if stats is not NULL,
 * stats[0] += number of loops with status != 0 and stats[1] += sum of iters (iters may be NULL), as
 * mpcqp_accumulate_stats does. */
int mpcqp_wip_advance_stats_batch(int32_t dtype, void *states, const void *U, int64_t u_stride,
                                  const int32_t *status, const int32_t *iters, int64_t *stats, int32_t N,
                                  double sampling_period, double target_vel, double length, double gravity,
                                  int32_t nsub, void *x0, void *goal, void *targets, int64_t batch, void *stream);

/* A WHOLE control period of `batch` wheeled-inverted-pendulum loops in ONE launch: mpcqp_build_solve_batch of every
 * loop's problem, then -- as the epilogue of the solver kernel, by the wavefront that solved it -- the plant step with
 * the plan's first input (zero when status != 0) and the loop's next problem written IN PLACE over x0 / goal / targets
 * of `problem`, exactly as mpcqp_wip_advance_batch does (examples/wheeled_inverted_pendulum.py:99-118, one iteration of
 * the loop). states [batch, 4] is updated in place; loop_stats (int64 [batch, 2], device, may be NULL): [b][0] += 1 if
 * the plan was not found, [b][1] += iterations. Only for problems mpcqp_build_solve_batch hands to the stage-wise
 * kernel (float64, nx = 4, nu = 1, 16 < N <= 128, per-loop x0 / goal / targets): MPCQP_EUNSUPPORTED otherwise -- the
 * caller then launches the solve and mpcqp_wip_advance_stats_batch separately. Workspace: mpcqp_workspace_bytes.
 * U, lam, status and iters as mpcqp_build_solve_batch (status[b] != 0: U[b] = zeros, lam[b] undefined; the plant then steps with
 * a zero input); the workspace's initial content is never read, MPCQP_OPT_REUSE_FACTOR / _PIPELINE_FACTOR launches apart. */
int mpcqp_wip_period_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                           const MpcqpSolveOpts *opts, void *U, void *lam, int32_t *status, int32_t *iters,
                           void *workspace, size_t workspace_bytes, void *states, int64_t *loop_stats,
                           double sampling_period, double target_vel, double length, double gravity, int32_t nsub,
                           void *stream);

/* `nperiods` consecutive control periods of every loop in ONE launch (ABI 7): what nperiods calls of
 * mpcqp_wip_period_batch do -- the epilogue writes the loop's next problem in place, so the wavefront that solved period t
 * carries on with period t + 1 -- without the launch boundary between them (a period of 1024 loops is ~30 us of work
 * behind ~8 us of dispatch; the loops never interact, so nothing has to meet at a period's end). Trajectories, U / lam /
 * status / iters (those of the LAST period) and loop_stats are bitwise what the one-period calls leave. With
 * MPCQP_OPT_PIPELINE_FACTOR the two factor images alternate from period to period starting at opts->factor_slot: the
 * caller's next launch passes factor_slot ^ (nperiods & 1). MPCQP_OPT_KEEP_FACTOR, warm_state and horizons whose factor
 * does not fit LDS (N > 64 for nx = 4, nu = 1) need nperiods == 1 (MPCQP_EUNSUPPORTED otherwise); nperiods < 1 is
 * MPCQP_EINVAL. examples/wheeled_inverted_pendulum.py:99-118, nperiods
 * iterations of the loop. */
int mpcqp_wip_periods_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                            const MpcqpSolveOpts *opts, void *U, void *lam, int32_t *status, int32_t *iters,
                            void *workspace, size_t workspace_bytes, void *states, int64_t *loop_stats,
                            double sampling_period, double target_vel, double length, double gravity, int32_t nsub,
                            int32_t nperiods, void *stream);

/* `nperiods` consecutive control periods of `batch` closed loops of ANY factored shared model in ONE launch (an additive
 * part of ABI 12: MPCQP_ABI_VERSION is unchanged) -- what mpcqp_wip_period_batch / mpcqp_wip_periods_batch do for the
 * wheeled inverted pendulum, with a linear plant given as data instead of compiled in. The plant may differ from the model. */
typedef struct MpcqpLoopPlant {
    MpcqpOperand A;  /* [B|1] nx x nx   x+ = A x + B u0 + d   (batch_stride 0 = shared; step_stride unused) */
    MpcqpOperand B;  /* [B|1] nx x nu */
    MpcqpOperand d;  /* [B|1, P|1] nx   additive disturbance, ptr NULL = none; step_stride = PERIOD stride (0: same every period) */
} MpcqpLoopPlant;

typedef struct MpcqpLoopOut {
    void    *X;          /* [batch, nperiods+1, nx]  state before every period and after the last; NULL = not recorded */
    void    *U0;         /* [batch, nperiods, nu]    the input applied in every period; NULL = not recorded */
    int64_t *loop_stats; /* [batch, 3] accumulated (+=): periods without a plan, iterations, warm periods re-solved cold; NULL ok */
} MpcqpLoopOut;

/* Period t = 0 .. nperiods-1 of loop b, by the rules of the WIP loop's exports above:
 *   1. mpcqp_solve_model_batch's problem at x0 = states[b], goal[b, t], targets[b, t] (step_stride of `goal` and `targets` is
 *      the PERIOD stride, 0 = the same every period), with the model's own bounds;
 *   2. u0 = the first nu entries of the plan, zero when the period's status is not MPCQP_SOLVED -- then loop_stats[b][0] += 1
 *      and the loop carries on;
 *   3. states[b] = A states[b] + B u0 + d[b, t];
 *   4. loop_stats[b][1] += the period's iterations.
 * U, lam, status and iters are those of the LAST period, as mpcqp_solve_model_batch leaves them (lam and iters may be NULL;
 * status[b] != 0: U[b] = zeros, lam[b] undefined). `out` may be NULL. No workspace, no allocation, no synchronisation;
 * `model`, the plant and the references are only read. One launch of nperiods periods leaves, with warm == 0, bitwise what
 * nperiods launches of one period with advanced pointers leave (the property mpcqp_wip_periods_batch states).
 * warm != 0: inside ONE launch, a period that follows a period that ended MPCQP_SOLVED starts from that period's active set
 * and operator T = N*, kept in registers (T depends on the matrices only: the contract of MpcqpSolveOpts.warm_state). The
 * kept set's multipliers are recomputed for the new state, rows with a negative one are dropped (one iteration each), and
 * the period is accepted through the from-scratch verification only; a warm period that does not end verified-solved --
 * the iteration limit, a failed verification, also an INFEASIBLE verdict -- is solved again cold in place and
 * loop_stats[b][2] += 1: a stale state costs a cold restart, never a wrong plan. Its iterations count in full (iters,
 * loop_stats[b][1]). The first period of a launch is always cold and nothing of the state is stored.
 * Served: float64, n = N nu <= 16, 1 <= m = N mk <= 32, nx <= 16, opts->flags == 0, no warm_state, no order
 * (mpcqp_w64.hip, one loop per wavefront); MPCQP_EUNSUPPORTED otherwise (float32 and every MPCQP_OPT_* flag included).
 * nperiods < 1, batch < 0 or a NULL required pointer: MPCQP_EINVAL. The reference has no counterpart beyond the Python
 * loops of its examples (examples/wheeled_inverted_pendulum.py:99-118 is one for one plant). */
int mpcqp_model_periods_batch(const MpcqpDims *dims, const void *model, const MpcqpLoopPlant *plant,
                              void *states,                 /* [batch, nx], updated in place */
                              const MpcqpOperand *goal,     /* [B|1, P|1, nx];    step_stride = period stride */
                              const MpcqpOperand *targets,  /* [B|1, P|1, N*nx];  step_stride = period stride */
                              int64_t batch, int32_t nperiods, int32_t warm, const MpcqpSolveOpts *opts,
                              void *U, void *lam, int32_t *status, int32_t *iters, /* those of the LAST period */
                              const MpcqpLoopOut *out, void *stream);

/* The vector-Jacobian product of those closed loops, one launch for all periods (an additive part of ABI 12:
 * MPCQP_ABI_VERSION is unchanged): the reverse-time recursion through `nperiods` periods of every loop, each period the
 * KKT adjoint of mpcqp_model_vjp_batch on the factored model with gU = [ubar; 0] and no gX. With the loop of
 * mpcqp_model_periods_batch -- u0_t the plan's first input, zero when status[b][t] != 0, x_{t+1} = A x_t + B u0_t + d_t --
 * and cotangents gX, gU0 of the records X, U0: a = gX_P, and for t = P-1 .. 0
 *     g_d_t = a;   g_A += a x_t';   g_B += a u0_t';   ubar = gU0_t + B' a;   a_new = gX_t + A' a
 *     status[b][t] == 0, A_t = {i : lam_i > 0}, S = M_A M_A':
 *         tt = L^-1 [ubar; 0];   nu = S^-1 M_A tt;   w = tt - M_A' nu
 *         a_new -= Wx' w + Hx_A' nu;   g_goal_t = Wg' w;   g_targets_t = Wt' w
 *     a = a_new
 * and g_x0 = a ("Closed-loop adjoint"). A period without a plan passes the costate through the plant
 * only. The loops never interact: sixteen lanes per loop, four loops per wavefront, the period loop inside the kernel
 * with the costate, the rows of g_A / g_B and the period sums in registers; no workspace, no allocation, no
 * synchronisation. The reference has no counterpart: its closed loops are Python loops over NumPy plans
 * (examples/wheeled_inverted_pendulum.py:99-118, examples/lipm_walking_controller.py:304-333) and carry no derivative.
 * A gradient that is per loop and per period, or summed over the periods in the kernel (period_stride 0: one block per loop): */
typedef struct MpcqpPeriodGrad {
    void   *ptr;            /* NULL = not wanted */
    int64_t batch_stride;   /* in elements, from loop to loop */
    int64_t period_stride;  /* in elements, from period to period; 0 = the sum over the periods, one block per loop */
} MpcqpPeriodGrad;

/* Inputs, packed: lam [batch][nperiods][m] and status [batch][nperiods], EVERY period's multipliers and status (the fused loop
 * keeps only the last period's: solve the recorded states again with mpcqp_solve_model_batch, batch * nperiods problems in
 * one launch); X [batch][nperiods+1][nx] and U0 [batch][nperiods][nu], the loop's records, read only for g_A / g_B and
 * nullable with them; gX [batch][nperiods+1][nx] and gU0 [batch][nperiods][nu], each nullable, NULL = zero. `plant`: A and B
 * as mpcqp_model_periods_batch takes them (batch_stride 0 = shared); d is not read. `model` is only read.
 * Outputs: g_x0 [batch][nx] (required); g_states [batch][nperiods+1][nx] (nullable), the costates a_0 .. a_P -- its rows
 * 1 .. P are the gradient of the disturbance of periods 0 .. P-1, row 0 is g_x0 --; g_goal (blocks of nx) and g_targets (blocks
 * of N nx), each a nullable MpcqpPeriodGrad; g_A [batch][nx][nx] and g_B [batch][nx][nu], per loop, summed over the periods,
 * nullable; vjp_status [batch] (nullable): the NUMBER of periods of the loop whose S failed the pivot test of the other
 * derivative exports or that had more active rows than variables -- such a period contributes its plant term only.
 * A sum over the batch for operands the batch shares is the caller's, as in every derivative export. Terms follow
 * dims->flags as in mpcqp_model_vjp_batch: a goal or targets that do not enter q get zeros, and Wg / Wt are not read.
 * A model whose factorisation failed gives zeros everywhere and vjp_status = nperiods.
 * Checks, before anything is launched: MPCQP_EDTYPE unless float64; MPCQP_EUNSUPPORTED outside n = N nu <= 16,
 * 1 <= m = N mk <= 32, nx <= 16 (the envelope of mpcqp_model_periods_batch: whatever the fused loop ran can be
 * differentiated); MPCQP_EINVAL for a NULL model, plant (or its A / B), lam, status or g_x0, nperiods < 1, batch < 0, a
 * negative stride, or g_A / g_B without X / U0. */
int mpcqp_model_periods_vjp_batch(const MpcqpDims *dims, const void *model, const MpcqpLoopPlant *plant, int64_t batch,
                                  int32_t nperiods, const void *lam, const int32_t *status, const void *X, const void *U0,
                                  const void *gX, const void *gU0, void *g_x0, void *g_states,
                                  const MpcqpPeriodGrad *g_goal, const MpcqpPeriodGrad *g_targets, void *g_A, void *g_B,
                                  int32_t *vjp_status, void *stream);

/* The Jacobian-vector products of those closed loops, one launch for all periods and all tangents (an additive part of ABI
 * 12: MPCQP_ABI_VERSION is unchanged): the forward-time recursion through `nperiods` periods of every loop, each period the
 * KKT tangent of mpcqp_model_jvp_batch on the factored model with dh = -Hx dx_t (the model's own bounds do not move). With
 * the loop, the maps L, M, Wx, Wg, Wt, Hx and the active-set rule of mpcqp_model_periods_vjp_batch above, and tangents dx0,
 * dgoal_t, dtargets_t, dd_t (the disturbance), dA and dB (the plant): dx_0 = dx0, and for t = 0 .. P-1
 *     status[b][t] == 0, A_t = {i : lam_i > 0}, k = |A_t| <= n, S = M_A M_A' positive definite:
 *         r = -(Wx dx_t - Wg dgoal_t - Wt dtargets_t);   mu = S^-1 (M_A r + Hx_A dx_t)
 *         du0_t = the first nu entries of L^-T (r - M_A' mu)
 *     otherwise du0_t = 0 (no plan: the tangent passes through the plant only; a failed S or k > n: likewise, and the
 *     period is counted in jvp_status)
 *     dx_{t+1} = A dx_t + B du0_t + dd_t + dA x_t + dB u0_t
 * ("Closed-loop forward sensitivities"). It is the transpose of mpcqp_model_periods_vjp_batch on the
 * same lam and status: <gX, dX> + <gU0, dU0> = <g, tangents>, and jvp_status equals vjp_status. S of a period is factored
 * ONCE and every tangent reuses the factor: sixteen lanes per loop, four loops per wavefront, the period loop inside the
 * kernel, lane l carrying component l of dx of up to sixteen tangents in registers (ntan > 16: the period loop runs again
 * per chunk of sixteen); no workspace, no allocation, no synchronisation. The reference has no counterpart: its closed loops
 * are Python loops over NumPy plans (examples/wheeled_inverted_pendulum.py:99-118,
 * examples/lipm_walking_controller.py:304-333) and carry no derivative.
 * A tangent of a reference or of the disturbance, per loop or shared, per period or constant in time: */
typedef struct MpcqpPeriodTangent {   /* [B|1][ntan][P|1][w] */
    const void *ptr;                  /* NULL = zero */
    int64_t batch_stride;             /* elements from loop to loop; 0 = one set shared by the batch */
    int64_t tangent_stride;           /* elements from tangent to tangent */
    int64_t period_stride;            /* elements from period to period; 0 = the same in every period */
} MpcqpPeriodTangent;

typedef struct MpcqpLoopTangents {
    const void *dx0; int64_t dx0_stride;     /* [B|1][ntan][nx], as MpcqpTangents */
    MpcqpPeriodTangent dgoal, dtargets, dd;  /* w = nx, N nx, nx */
    const void *dA;  int64_t dA_stride;      /* [B|1][ntan][nx][nx] */
    const void *dB;  int64_t dB_stride;      /* [B|1][ntan][nx][nu] */
} MpcqpLoopTangents;

/* Inputs: lam [batch][nperiods][m] and status [batch][nperiods], EVERY period's, as for the VJP; X [batch][nperiods+1][nx]
 * and U0 [batch][nperiods][nu], the loop's records, read only with dA / dB and nullable with them; `plant`: A and B as
 * mpcqp_model_periods_batch takes them, d is not read; `tan`: every pointer nullable, NULL = zero (a stride of 0 shares one
 * set with the batch). Terms follow dims->flags: a dgoal or dtargets whose operand does not enter q is not read.
 * Outputs: dX [batch][ntan][nperiods+1][nx] (required), dx_0 .. dx_P of every tangent; dU0 [batch][ntan][nperiods][nu]
 * (nullable); jvp_status [batch] (nullable): the NUMBER of periods with a plan whose S failed the pivot test (the plain
 * one, pivot > 0, of mpcqp_model_periods_vjp_batch) or that had more active rows than variables.
 * A model whose factorisation failed gives zeros everywhere and jvp_status = nperiods. batch == 0 launches nothing.
 * Checks, before anything is launched, in this order: MPCQP_EDTYPE unless float64; MPCQP_EUNSUPPORTED outside
 * n = N nu <= 16, 1 <= m = N mk <= 32, nx <= 16; MPCQP_EINVAL for a NULL model, plant (or its A / B), lam, status, tan or
 * dX, nperiods < 1, batch < 0, ntan outside 1 .. 256, a negative stride, or dA / dB without X / U0. */
int mpcqp_model_periods_jvp_batch(const MpcqpDims *dims, const void *model, const MpcqpLoopPlant *plant,
                                  int64_t batch, int32_t nperiods, int32_t ntan,
                                  const void *lam, const int32_t *status,   /* every period's, as for the VJP */
                                  const void *X, const void *U0,            /* records; read only with dA / dB */
                                  const MpcqpLoopTangents *tan,
                                  void *dX,                                  /* [batch][ntan][nperiods+1][nx], required */
                                  void *dU0,                                 /* [batch][ntan][nperiods][nu], nullable */
                                  int32_t *jvp_status,                       /* [batch], nullable: counted periods */
                                  void *stream);

/* Bookkeeping of closed loops (the reference's loops count nothing; ours report failures and iterations):
 * stats[0] += number of problems with status != 0, stats[1] += sum of iters. stats: two int64 in DEVICE memory. */
int mpcqp_accumulate_stats(const int32_t *status, const int32_t *iters, int64_t batch, int64_t *stats, void *stream);

/* A pairing order for MpcqpSolveOpts.order (ABI 9): order = the problems sorted by counts[] (last period's `iters`, clamped to
 * 0 .. 1023), longest first, by a counting sort on the device (three small launches, ~10 us for 65,536). Equal counts come out in
 * an unspecified order. counts, order: DEVICE int32 [batch]; workspace: mpcqp_order_workspace_bytes(batch) bytes of DEVICE memory
 * (MPCQP_EWORKSPACE if smaller). The reference has no counterpart: its solver is called per problem (qpmpc/solve_mpc.py:43). */
size_t mpcqp_order_workspace_bytes(int64_t batch);

int mpcqp_order_by_count(const int32_t *counts, int64_t batch, int32_t *order, void *workspace, size_t workspace_bytes,
                         void *stream);

/* One period of `batch` LIPM walking controllers, fused (examples/lipm_walking_controller.py:304-333):
 * if U is not NULL, apply the first jerk of each plan (U[b*u_stride], zero when status[b] != 0) to
 * the constant-jerk plant for `nsub` exact sub-steps (integrate, :216-236) and advance the footstep
 * phase (PhaseStepper.advance / advance_stride :125-132, main loop :329-332); then write the NEXT MPC
 * problem of every walker: x0 [3], goal [3] and the per-step ZMP bounds e [N, 2] of its receding
 * horizon (PhaseStepper.get_nb_steps :134-165, update_goal_and_constraints :179-213; rows without a
 * bound hold max_zmp_dist). U == NULL only writes the problem of the current phase (first period).
 * Per walker, updated in place: states [3], index, stride_index (int64), support; read: strides [2],
 * foot_size. Refuses (EINVAL) horizons spanning more than two steps, like the reference (:107-110). */
int mpcqp_lipm_advance_batch(int32_t dtype, void *states, const void *U, int64_t u_stride,
                             const int32_t *status, int32_t N, double sampling_period, int32_t nsub,
                             int32_t nb_dsp, int32_t nb_ssp, double max_zmp_dist, int64_t *index,
                             int64_t *stride_index, void *support, const void *strides,
                             const void *foot_size, void *x0, void *goal, void *e, int64_t batch,
                             void *stream);

/* The same with the loops' bookkeeping fused in: if stats is not NULL, stats[0] += number of walkers with
 * status != 0 and stats[1] += sum of iters (iters may be NULL), as mpcqp_accumulate_stats does. */
int mpcqp_lipm_advance_stats_batch(int32_t dtype, void *states, const void *U, int64_t u_stride,
                                   const int32_t *status, const int32_t *iters, int64_t *stats, int32_t N,
                                   double sampling_period, int32_t nsub, int32_t nb_dsp, int32_t nb_ssp,
                                   double max_zmp_dist, int64_t *index, int64_t *stride_index, void *support,
                                   const void *strides, const void *foot_size, void *x0, void *goal, void *e,
                                   int64_t batch, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MPCQP_H_ */
