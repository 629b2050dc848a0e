// Internal declarations shared by the kernel translation units and the C ABI.
#ifndef MPCQP_INTERNAL_H_
#define MPCQP_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpcqp.h"

namespace mpcqp {

enum { MODE_FUSED = 0, MODE_CONDENSE = 1, MODE_SOLVE = 2, MODE_MODEL = 3, MODE_LOOP = 4 };

constexpr size_t kLdsBytesPerCU = 160 * 1024;  // gfx950: 160 KiB per CU

// Feasibility tolerance of row i of the dense condensed kernels (mpcqp_bigsolve.hip dense and structured kinds, mpcqp_lds.hip
// without a prefactored model): the row counts as violated below -row_tol, its refinement and acceptance bounds are multiples
// of it. float64: tol (1 + |h_i|) with tol = 1e-12 -- the absolute term is far below every bound in any units. float32
// (tol = 1e-5): tol (|G_i| + |h_i|), which scales with the row, so a row stated in other units (r G_i u <= r h_i) is admitted,
// refined and accepted at the same distance |G_i u - h_i| / |G_i| from its hyperplane; with the absolute term a row stated
// 2^-10 times smaller stayed violated by 1e-2 in the caller's units and plans came back 'solved' 4.6e-3 off.
template <typename T>
__device__ __forceinline__ T row_tol(T tol, T gnorm, T hi)
{
    if constexpr (sizeof(T) == 4)
        return tol * (gnorm + (T)fabs(hi));
    else
        return tol + tol * (T)fabs(hi);
}

// SIMDs of the device that is current for this call (4 per compute unit). Asked per call: the library keeps no state between
// calls (include/mpcqp.h), and a process may drive several devices. 0 when the runtime cannot tell.
inline int device_simds_now()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return 4 * cus;
}

// The SIMD count as the dispatch hands it to the batch-size rule of the four-per-wavefront kernels (quad_eligible,
// quad_model_eligible): SimdCount{} asks the device on first use, so a launch whose kernel is settled without the rule makes no
// runtime call for it; SimdCount{n} is the constant n (the size queries, which launch nothing).
struct SimdCount {
    int value = -1;  // < 0: not asked yet
    int get()
    {
        if (value < 0) value = device_simds_now();
        return value;
    }
};

// INTERNAL bit of KernelArgs.opt_flags (never taken from MpcqpSolveOpts.flags: fill_opts clears it): the wide stage-wise kernel runs as
// the SECOND OPINION behind the narrow one -- a wavefront whose problem the first launch settled (solved, not positive definite,
// slots full) exits at once, the others (MPCQP_MAX_ITER, MPCQP_INFEASIBLE) are solved again from scratch. Round 6: the narrow kernel
// still keeps the explicit inverse of the active rows' Gram matrix and, when every variable is pinned, gives a wrong verdict on one
// problem in some hundreds; the wide kernel's thin-QR operator does not, for the price of a launch of wavefronts that exit.
constexpr int kOptSecondOpinion = 1 << 30;

// Everything a kernel needs, passed by value (kernarg segment, scalar loads).
struct KernelArgs {
    int nx, nu, N, mk, n, m, flags, max_iter;
    double wt, wx, wu, tol;
    MpcqpOperand A, B, C, D, e, x0, goal, targets;
    // QP buffers: outputs of CONDENSE, inputs of SOLVE
    void *P, *q, *G, *h, *Phi, *Psi;
    // solve outputs
    void *U, *lam;
    int32_t *status, *iters;
    // rollout
    void *X;
    // per-problem solver arrays in HBM (large problems): batch * Layout.total elements
    void *ws;
    // shared-model path: the factored model (ModelLayout) 
    const void *model;
    // MpcqpSolveOpts beyond max_iter / feas_tol
    int opt_flags;                // MPCQP_OPT_*
    void *warm_state;             // per-problem active set + operator (read if warm_start, written at the end), or null
    int warm_start;               // 0 | MPCQP_WARM_OPERATOR | MPCQP_WARM_ACTIVE_SET
    int warm_shift;               // MPCQP_WARM_ACTIVE_SET: rows the stored ids move down by
    int factor_slot;              // which of the two factor images of the stage-wise kernel this launch keeps / reuses
    size_t warm_state_bytes;      // size of the buffer behind warm_state (checked on the host before the launch)
    void *probe;                  // developer probe: int64 stamps per problem, or null
    // closed-loop epilogue of the stage-wise kernel (mpcqp_wip_period_batch): after its solve every wavefront applies
    // the first input of its plan to the wheeled-inverted-pendulum plant and writes its loop's NEXT problem in place
    int ep_on, ep_nsub, ep_periods;  // (ep_periods: control periods per launch, mpcqp_wip_periods_batch; 0 / 1 = one)
    double ep_Tp, ep_vel, ep_omega2, ep_g;
    void *ep_states;              // [batch, 4], updated in place
    long long *ep_loopstats;      // [batch, 2]: += (failed, iterations), or null
    // (last: the fields above keep the offsets the stage-wise kernels' hand-placed kernel-argument loads were measured with)
    const int32_t *order;         // pairing order of the small-problem fused kernel (a permutation of the batch), or null
};

// LDS carve, in elements of T. Matrices are row-major with odd row stride ld.
struct Layout {
    int ld;
    int off_A, off_B, off_x0;  // staged dynamics (build only)
    int off_X;                 // union: Psi blocks 1..N (build) | Q, S (solve)
    int off_P, off_M;          // P -> L ; G -> M = G L^-T, row m holds q -> L^-1 q
    int off_h, off_hs, off_s, off_y, off_z, off_d, off_r, off_u, off_cs, off_sn, off_inv, off_xs, off_red;
    int off_int;               // int act[n+2], where[m], redi[8]
    int total;
};

inline Layout make_layout(int nx, int nu, int N, int n, int m, bool stepA, bool stepB, int mode, size_t esz)
{
    Layout L{};
    L.ld = (n + 1) | 1;
    int o = 0;
    auto take = [&](int cnt) {
        int at = o;
        o += (cnt + 1) & ~1;  // keep 8-byte alignment for float too
        return at;
    };
    if (mode != MODE_SOLVE) {
        L.off_A = take((stepA ? N : 1) * nx * nx);
        L.off_B = take((stepB ? N : 1) * nx * nu);
        L.off_x0 = take(nx);
        const int psi = N * nx * L.ld, qs = 2 * n * L.ld;
        L.off_X = take(psi > qs ? psi : qs);
    } else {
        L.off_A = L.off_B = L.off_x0 = 0;
        L.off_X = take(2 * n * L.ld);
    }
    L.off_P = take(n * L.ld);
    L.off_M = take((m + 1) * L.ld);
    L.off_h = take(m);
    L.off_hs = take(m);
    L.off_s = take(m);
    L.off_y = take(n);
    L.off_z = take(n);
    L.off_d = take(n);
    L.off_r = take(n);
    L.off_u = take(n + 1);
    L.off_cs = take(n);
    L.off_sn = take(n);
    L.off_inv = take(n);
    L.off_xs = take(n);
    L.off_red = take(8);
    L.off_int = o;
    const int ints = (n + 2) + m + 8;
    o += (int)(((size_t)ints * 4 + esz - 1) / esz);
    o = (o + 1) & ~1;
    L.total = o;
    return L;
}

// Layout of a factored shared model, in elements of T. nc = max(n, 16) columns: models
// with n < 16 are padded with unit variables so that the wavefront kernel can use them.
struct ModelLayout {
    int nc, nb;  // padded variable count; number of pseudo-problems 1 + 2 nx + N nx
    size_t off_M, off_LinvT, off_invn, off_e, off_Hx, off_Wx, off_Wg, off_Wt, total;
};
// (constexpr, like the warm-record sizes below: the kernels compute the same layout as the host)
constexpr ModelLayout make_model_layout(int nx, int N, int n, int m)
{
    ModelLayout ml{};
    ml.nc = n < 16 ? 16 : n;
    ml.nb = 1 + 2 * nx + N * nx;
    size_t o = 0;
#define MPCQP_TAKE(field, cnt) \
    ml.field = o;              \
    o += ((size_t)(cnt) + 3) & ~(size_t)3;
    MPCQP_TAKE(off_M, (size_t)m * ml.nc)
    MPCQP_TAKE(off_LinvT, (size_t)ml.nc * ml.nc)
    MPCQP_TAKE(off_invn, m)
    MPCQP_TAKE(off_e, m)
    MPCQP_TAKE(off_Hx, (size_t)m * nx)
    MPCQP_TAKE(off_Wx, (size_t)ml.nc * nx)
    MPCQP_TAKE(off_Wg, (size_t)ml.nc * nx)
    MPCQP_TAKE(off_Wt, (size_t)ml.nc * N * nx)
#undef MPCQP_TAKE
    ml.total = o;  // one more element follows: the "P not positive definite" flag
    return ml;
}
int launch_wip_advance(int dtype, void *states, const void *U, int64_t u_stride, const int32_t *status,
                       const int32_t *iters, int64_t *stats, int N, double Tp, double vel, double length, double gravity,
                       int nsub, void *x0, void *goal, void *targets, int64_t batch, hipStream_t st);
int launch_lipm_advance(int dtype, void *states, const void *U, int64_t u_stride, const int32_t *status, int N,
                        double Tp, int nsub, int nb_dsp, int nb_ssp, double max_zmp, int64_t *index,
                        int64_t *stride_index, void *support, const void *strides, const void *foot_size, void *x0,
                        void *goal, void *e, int64_t batch, const int32_t *iters, int64_t *stats, hipStream_t st);
int launch_stats(const int32_t *status, const int32_t *iters, int64_t batch, int64_t *stats, hipStream_t st);
int launch_factor_model(const KernelArgs &ka, int dtype, const void *P, const void *G, const void *qb, const void *hb,
                        void *model, hipStream_t st);

template <int MODE>
int dispatch_lds(const KernelArgs &ka, const Layout &L, int dtype, int64_t batch, hipStream_t st);
// same solver with its arrays in a global workspace (ka.ws) instead of LDS
int dispatch_gws_solve(const KernelArgs &ka, const Layout &L, int dtype, int64_t batch, hipStream_t st);
// large-problem condensing (mpcqp_big.hip)
size_t big_condense_ws_elems(const KernelArgs &ka);
bool big_supported(const KernelArgs &ka);
// G may be null (not formed); rownorm_inv (1/|G_i|, [batch, m]) is optional
int launch_big_condense(const KernelArgs &ka, int dtype, int64_t batch, void *Psi_ws, void *res_ws, void *P, void *q,
                        void *G, void *h, void *rownorm_inv, hipStream_t st, int phase = 0);
// large-problem solver (mpcqp_bigsolve.hip): one problem per workgroup, L^-1 packed in LDS
bool bigsolve_supported(int n, int m, int dtype);
size_t bigsolve_ws_elems(int n);
bool bigsolve_struct_supported(const KernelArgs &ka, int dtype);
int launch_bigsolve_struct(const KernelArgs &ka, int dtype, int64_t batch, const void *P, const void *q,
                           const void *Psi_all, const void *h, const void *rownorm_inv, void *ws, hipStream_t st);
// mid-size fused build+solve (mpcqp_bigsolve.hip, KIND = K_MID): ws = 2 n^2 elements per problem
bool mid_supported(const KernelArgs &ka, int dtype);
int launch_mid(const KernelArgs &ka, int dtype, int64_t batch, void *ws, hipStream_t st);
int launch_transpose(const void *G, void *GT, int m, int n, int dtype, int64_t batch, hipStream_t st);
int launch_bigsolve(const KernelArgs &ka, int dtype, int64_t batch, const void *P, const void *q, const void *G,
                    const void *GT, const void *h, void *ws, hipStream_t st);
// stage-wise formulation (mpcqp_stage.hip): one problem per wavefront, O(N) per iteration
bool stage_supported(const KernelArgs &ka, int dtype);
int stage_default_maxq(const KernelArgs &ka);
bool stage_pipeline_supported(const KernelArgs &ka, int dtype);
// bytes per problem of the warm-state record (MpcqpSolveOpts.warm_state) for `maxq` slots
constexpr size_t stage_warm_bytes(int maxq) { return ((size_t)(4 + 2 * maxq) * sizeof(int) + 15) & ~(size_t)15; }
size_t stage_ws_doubles(const KernelArgs &ka, int maxq);
int launch_stage(const KernelArgs &ka, int maxq, int64_t batch, void *ws, hipStream_t st);
// ... for wider systems (mpcqp_stagew.hip): nx <= 16, nu <= 4, f64 and f32; workspace in elements of the dtype
bool stagew_supported(const KernelArgs &ka, int dtype);
size_t stagew_ws_elems(const KernelArgs &ka, int maxq, int dtype);
int launch_stagew(const KernelArgs &ka, int dtype, int maxq, int64_t batch, void *ws, hipStream_t st);
// warm-state record of the wide stage-wise kernel (MPCQP_WARM_ACTIVE_SET): int32 count, then the active rows' ids
constexpr size_t stagew_warm_bytes(int maxq) { return ((size_t)(maxq + 1) * 4 + 15) & ~(size_t)15; }
// ... and for every other system (mpcqp_stageg.hip): nx <= 32, nu <= 8, float64, any horizon; one workgroup per problem, all
// arrays in the workspace -- a general fallback, not a tuned path
bool stageg_supported(const KernelArgs &ka, int dtype);
int stageg_default_maxq(const KernelArgs &ka);
size_t stageg_ws_doubles(const KernelArgs &ka, int maxq);
int launch_stageg(const KernelArgs &ka, int maxq, int64_t batch, void *ws, hipStream_t st);
// small-problem kernel (mpcqp_pair.hip): two problems per wavefront, fused build+solve
bool pair_eligible(const KernelArgs &ka, int mode, int dtype);
constexpr size_t kPairWarmDoubles = 16 * 16 + 8;  // T (16 x 16), then 16 int32 constraint ids
int launch_pair(const KernelArgs &ka, int64_t batch, hipStream_t st);        // (pair_eligible and not quad_eligible: the dispatch)
int launch_pair_model(const KernelArgs &ka, int64_t batch, hipStream_t st);  // shared model (ka.model)
// small-problem kernel (mpcqp_quad.hip): four problems per wavefront, cold lean fused build+solve
bool quad_applies(const KernelArgs &ka);                  // the kernel serves this launch's layout
// ... and the dispatch takes it: no MPCQP_OPT_TWO_PER_WAVE, and MPCQP_OPT_FOUR_PER_WAVE, the general build or a batch of more than
// two problems per SIMD (`simds` is asked only where that last rule decides)
bool quad_eligible(const KernelArgs &ka, int64_t batch, SimdCount &simds);
int launch_quad(const KernelArgs &ka, int64_t batch, hipStream_t st);
// shared-model launches of the pair kernel's sizes (the caller has checked pair_eligible(ka, MODE_MODEL)): the same rule
bool quad_model_eligible(const KernelArgs &ka, int64_t batch, SimdCount &simds);
int launch_quad_model(const KernelArgs &ka, int64_t batch, hipStream_t st);
// ... and its general build with four rows per lane for 33 .. 64 rows (mpcqp_quadg.hip): cold launches, any batch size
bool quad4_applies(const KernelArgs &ka);
int launch_quad4(const KernelArgs &ka, int64_t batch, hipStream_t st);
// problems of 17 .. 32 variables on chip (mpcqp_duo.hip): two problems per wavefront, cold fused build+solve, no workspace;
// taken on request only (MPCQP_OPT_ON_CHIP_32)
bool duo_applies(const KernelArgs &ka);
int launch_duo(const KernelArgs &ka, int64_t batch, hipStream_t st);
// ... and its shared-model mode (ka.model; ka.e.ptr: bounds per problem, or null for the model's): 17 <= n <= 32, 1 <= m <= 64,
// any nx and any number of rows per step, float64, cold
bool duo_model_applies(const KernelArgs &ka);
int launch_duo_model(const KernelArgs &ka, int64_t batch, hipStream_t st);
// ... and its QP-given mode (ka.P, ka.q, ka.G, ka.h, packed per problem; mpcqp_solve_batch with the flag): 1 <= n <= 32,
// 1 <= m <= 64, float64, cold, no workspace
bool duo_qp_applies(const KernelArgs &ka);
int launch_duo_qp(const KernelArgs &ka, int64_t batch, hipStream_t st);
// small-problem kernel (mpcqp_w64.hip): one problem per wavefront
bool w64_eligible(const KernelArgs &ka, int mode, int dtype);
int launch_w64(const KernelArgs &ka, int mode, int dtype, int64_t batch, hipStream_t st);
// ... and its closed loop (MODE_LOOP, mpcqp_model_periods_batch): `nperiods` control periods of a shared model per launch, the
// wavefront that solved period t stepping its plant and carrying on with period t + 1. What the loop adds to KernelArgs is a
// kernel argument of its own, so the other kernels' argument layouts stay what they were. ka.goal / ka.targets: step_stride is
// the PERIOD stride here.
struct LoopArgs {
    MpcqpOperand A, B, d;  // the plant x+ = A x + B u0 + d (d.ptr null: none; d.step_stride: period stride)
    void *states;          // [batch, nx], updated in place
    void *X, *U0;          // recorded trajectories, or null
    long long *stats;      // [batch, 3] += (periods without a plan, iterations, warm periods re-solved cold), or null
    int nperiods, warm;
    int off_xs;            // LDS: the state (16) and the applied input (16), behind the kernel's own carve
};
bool w64_loop_eligible(const KernelArgs &ka, int dtype);  // float64, n <= 16, 1 <= m <= 32, nx <= 16
int launch_w64_loop(const KernelArgs &ka, const LoopArgs &lp, int64_t batch, hipStream_t st);
int launch_phi(const KernelArgs &ka, int dtype, int64_t batch, hipStream_t st);
int launch_update(const KernelArgs &ka, int dtype, int64_t phi_bs, int64_t psi_bs, int64_t batch, hipStream_t st);
int launch_rollout(const KernelArgs &ka, int dtype, int64_t batch, hipStream_t st);
// The condensed KKT inputs of the adjoint and tangent kernels (mpcqp_adjoint.hip; float64), passed to them as they are
struct CondensedKkt {
    int nx, nu, N, mk, n, m, flags;  // n = N nu, m = N mk
    double wt, wx;
    const double *P, *G, *Phi, *Psi;  // mpcqp_condense_batch's outputs, packed per problem (G null when m = 0)
    MpcqpOperand C;
    const double *lam;                // null when m = 0
    const int32_t *status;
    double *carve_ws;                 // the per-problem carves when they do not fit LDS (else null)
};
// vector-Jacobian product of solved plans (mpcqp_adjoint.hip): one problem per workgroup on the condensed matrices
struct AdjointLaunch {
    CondensedKkt kkt;
    const double *gU, *gX;  // gX nullable
    int32_t *vjp_status;    // nullable
    // model and cost gradients (mpcqp_plan_vjp_model_batch): the kModel kernel, which also reads A, x0, goal, targets
    // and the plan U
    bool model;
    MpcqpOperand A, x0, goal, targets;
    const double *U;
    MpcqpVjpModelOut out;   // g_x0 set, the rest nullable; g_A .. g_w are written only with `model`
};
size_t adjoint_carve_bytes(int n, int N, int nx, int m = 0, bool model = false);
bool adjoint_carve_in_lds(int n, int N, int nx, int m = 0, bool model = false);
int launch_adjoint(const AdjointLaunch &l, int64_t batch, hipStream_t st);
// Jacobian-vector product of solved plans (mpcqp_adjoint.hip, mpcqp_tangent_kernel): the adjoint's KKT system with ntan
// tangents as right-hand sides
struct TangentLaunch {
    CondensedKkt kkt;
    int ntan;
    MpcqpTangents tan;
    double *dU, *dX;  // dX nullable
    int32_t *jvp_status;
};
size_t tangent_carve_bytes(int n, int N, int nx, int ntan, bool model = false);
bool tangent_carve_in_lds(int n, int N, int nx, int ntan, bool model = false);
int launch_tangent(const TangentLaunch &l, int64_t batch, hipStream_t st);
// ... with tangents of A, B, C, D and the weights as well (mpcqp_plan_jvp_model_batch): the kModel kernel, which also reads
// A, x0, goal, targets and the plan U. The kernel without them takes TangentLaunch as it always did.
struct TangentModelLaunch : TangentLaunch {
    MpcqpModelTangents mtan;
    MpcqpOperand A, x0, goal, targets;
    const double *U;
};
int launch_tangent_model(const TangentModelLaunch &l, int64_t batch, hipStream_t st);
// the stage-wise adjoint (mpcqp_adjoint_stagewise.hip; float64, nx <= 32, nu <= 8, any N): one problem per workgroup on its
// Riccati recursion, the records and the active rows' whitened vectors in a per-problem region of the workspace; passed to
// the kernel as it is
struct StagewiseAdjointLaunch {
    int nx, nu, N, mk, n, m, flags, ka;  // n = N nu, m = N mk; ka = max(max_active, 1)
    double wt, wx, wu;
    MpcqpProblem problem;
    const double *lam, *gU, *gX, *U;  // lam nullable when mk = 0, gX nullable, U needed when `model`
    const int32_t *status;
    MpcqpVjpModelOut out;  // every pointer nullable
    bool model;            // one of g_A .. g_w requested
    int32_t *vjp_status;
    double *workspace;     // batch * stagewise_adjoint_bytes
};
bool stagewise_adjoint_applies(int nx, int nu);
size_t stagewise_adjoint_bytes(int nx, int nu, int N, int mk, int max_active);  // per problem
int launch_adjoint_stagewise(const StagewiseAdjointLaunch &l, int64_t batch, hipStream_t st);
// the stage-wise tangent (mpcqp_adjoint_stagewise.hip, mpcqp_tangent_stagewise_kernel; the same envelope): ntan tangents per
// problem on the adjoint's factorisation -- its records, whitened rows and Gram factor -- in passes of 256 / max(nx, nu)
struct StagewiseTangentLaunch {
    int nx, nu, N, mk, n, m, flags, ka, ntan;  // ka = max(max_active, 1)
    double wt, wx, wu;
    MpcqpProblem problem;
    const double *lam;  // nullable when mk = 0
    const int32_t *status;
    MpcqpTangents tan;
    double *dU, *dX;  // dX nullable
    int32_t *jvp_status;
    double *workspace;  // batch * stagewise_tangent_bytes
};
size_t stagewise_tangent_bytes(int nx, int nu, int N, int max_active, int ntan, bool model = false);  // per problem
int launch_tangent_stagewise(const StagewiseTangentLaunch &l, int64_t batch, hipStream_t st);
// ... with tangents of A, B, C, D and the weights as well (mpcqp_plan_jvp_model_stagewise_batch): the kModel kernel
struct StagewiseTangentModelLaunch : StagewiseTangentLaunch {
    MpcqpModelTangents mtan;
    const double *U;
};
int launch_tangent_model_stagewise(const StagewiseTangentModelLaunch &l, int64_t batch, hipStream_t st);
// derivatives of plans of a factored shared model (mpcqp_model_adjoint.hip; float64, n <= 64): the KKT adjoint (ntan == 0)
// or ntan tangents on the model's whitened matrices, without a workspace; passed to the kernels as it is
struct ModelDiffLaunch {
    int nx, nu, N, mk, n, m, flags, ntan;  // n = N nu, m = N mk; ntan: 0 = the VJP
    int64_t batch;
    const double *model;                   // what mpcqp_factor_model wrote (ModelLayout)
    const double *lam;                     // null when m = 0
    const int32_t *status;
    MpcqpOperand A, B;                     // read with gX / dX only (else their ptr may be null)
    const double *gU, *gX;                 // VJP; gX nullable
    double *g_x0, *g_goal, *g_targets, *g_e;  // VJP; all but g_x0 nullable
    MpcqpTangents tan;                     // JVP
    double *dU, *dX;                       // JVP; dX nullable
    int32_t *out_status;                   // vjp_status / jvp_status, nullable
};
// the small kernel (sixteen lanes per problem; n <= 16, m <= 32, nx <= 16) runs at most this many workgroups of sixteen
// problems a round: larger batches take further rounds on the same workgroups, whose LDS image of the model is staged once
constexpr int kModelDiffMaxGrid = 1024;
bool model_diff_small_applies(int nx, int n, int m);
int launch_model_diff_small(const ModelDiffLaunch &l, hipStream_t st);
size_t model_diff_general_lds_bytes(int nx, int n);
int launch_model_diff_general(const ModelDiffLaunch &l, hipStream_t st);
// the adjoint of the closed loops of a shared model (mpcqp_model_periods_vjp_batch; mpcqp_model_adjoint.hip,
// mpcqp_loop_adjoint_small_kernel: the small kernel's layout and envelope, the period loop inside); passed to the kernel as it is
struct LoopAdjointLaunch {
    int nx, nu, N, n, m, flags, nperiods;
    int64_t batch;
    const double *model;
    MpcqpOperand A, B;                 // the plant (batch_stride 0: shared)
    const double *lam;                 // [batch][nperiods][m]
    const int32_t *status;             // [batch][nperiods]
    const double *X, *U0;              // the records; read for g_A / g_B only (else null)
    const double *gX, *gU0;            // nullable: zero
    double *g_x0, *g_states;           // g_states nullable
    MpcqpPeriodGrad g_goal, g_targets; // ptr nullable
    double *g_A, *g_B;                 // nullable
    int32_t *out_status;               // nullable
};
int launch_loop_adjoint_small(const LoopAdjointLaunch &l, hipStream_t st);
// the tangents of those closed loops (mpcqp_model_periods_jvp_batch; mpcqp_loop_tangent.hip, mpcqp_loop_tangent_small_kernel:
// the same layout and envelope, the period loop running forwards inside); passed to the kernel as it is
struct LoopTangentLaunch {
    int nx, nu, N, n, m, flags, nperiods, ntan;
    int64_t batch;
    const double *model;
    MpcqpOperand A, B;                 // the plant (batch_stride 0: shared)
    const double *lam;                 // [batch][nperiods][m]
    const int32_t *status;             // [batch][nperiods]
    const double *X, *U0;              // the records; read with dA / dB only (else null)
    MpcqpLoopTangents tan;             // every pointer nullable: zero
    double *dX, *dU0;                  // dU0 nullable
    int32_t *out_status;               // nullable
};
int launch_loop_tangent_small(const LoopTangentLaunch &l, hipStream_t st);

}  // namespace mpcqp
#endif
