// mpcqp_capi.hip -- the extern "C" boundary declared in include/mpcqp.h.
// Argument validation happens here, on the host, before any launch; kernels
// live in mpcqp_lds.hip.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "mpcqp.h"
#include "mpcqp_internal.h"

using namespace mpcqp;

namespace {

size_t elem_size(int dtype) { return dtype == MPCQP_F64 ? 8 : 4; }

int check_dims(const MpcqpDims *d)
{
    if (!d) return MPCQP_EINVAL;
    if (d->dtype != MPCQP_F64 && d->dtype != MPCQP_F32) return MPCQP_EDTYPE;
    if (d->nx <= 0 || d->nu <= 0 || d->N <= 0 || d->mk < 0) return MPCQP_EINVAL;
    if (!(d->w_input > 0.0)) return MPCQP_EINVAL;  // mpc_problem.py:104-107
    return 0;
}

// One operand against the addressing contract of include/mpcqp.h: no negative stride, a step stride of 0 or the block, and a
// batch stride of 0 or at least what one problem occupies (`steps` = N; 0 for x0, goal and targets, whose step stride no
// kernel reads)
int check_operand(const MpcqpOperand &op, int64_t block, int64_t steps)
{
    if (!op.ptr) return 0;
    if (op.step_stride < 0 || op.batch_stride < 0) return MPCQP_ELAYOUT;
    if (steps && op.step_stride != 0 && op.step_stride != block) return MPCQP_ELAYOUT;
    const int64_t extent = (steps && op.step_stride) ? steps * block : block;
    if (op.batch_stride != 0 && op.batch_stride < extent) return MPCQP_ELAYOUT;
    return 0;
}

// the strides of every operand that is there (mpcqp_update_vectors_batch, which needs no A and B, stops at this)
int check_layout(const MpcqpDims *d, const MpcqpProblem *p)
{
    int rc;
    const int64_t nx = d->nx, nu = d->nu, mk = d->mk, N = d->N;
    if ((rc = check_operand(p->A, nx * nx, N))) return rc;
    if ((rc = check_operand(p->B, nx * nu, N))) return rc;
    if ((rc = check_operand(p->C, mk * nx, N))) return rc;
    if ((rc = check_operand(p->D, mk * nu, N))) return rc;
    if ((rc = check_operand(p->e, mk, N))) return rc;
    if ((rc = check_operand(p->x0, nx, 0))) return rc;
    if ((rc = check_operand(p->goal, nx, 0))) return rc;
    if ((rc = check_operand(p->targets, N * nx, 0))) return rc;
    return 0;
}

int check_problem(const MpcqpDims *d, const MpcqpProblem *p)
{
    if (!p || !p->A.ptr || !p->B.ptr || !p->x0.ptr) return MPCQP_EINVAL;
    if (d->mk > 0 && !p->e.ptr) return MPCQP_EINVAL;
    if ((d->flags & MPCQP_Q_TERMINAL) && !p->goal.ptr) return MPCQP_EINVAL;
    if ((d->flags & MPCQP_Q_STAGE) && !p->targets.ptr) return MPCQP_EINVAL;
    return check_layout(d, p);
}

void fill_args(KernelArgs &ka, const MpcqpDims *d, const MpcqpProblem *p)
{
    memset(&ka, 0, sizeof(ka));
    ka.nx = d->nx;
    ka.nu = d->nu;
    ka.N = d->N;
    ka.mk = d->mk;
    ka.n = d->N * d->nu;
    ka.m = d->N * d->mk;
    ka.flags = d->flags;
    ka.wt = d->w_terminal;
    ka.wx = d->w_stage;
    ka.wu = d->w_input;
    if (p) {
        ka.A = p->A;
        ka.B = p->B;
        ka.C = p->C;
        ka.D = p->D;
        ka.e = p->e;
        ka.x0 = p->x0;
        ka.goal = p->goal;
        ka.targets = p->targets;
    }
}

// (what a launch may not combine is refused by refusal(), which every export calls right after this)
int fill_opts(KernelArgs &ka, const MpcqpSolveOpts *o, int dtype)
{
    ka.max_iter = (o && o->max_iter > 0) ? o->max_iter : 10 * (ka.n + ka.m) + 10;
    ka.tol = (o && o->feas_tol > 0.0) ? o->feas_tol : (dtype == MPCQP_F64 ? 1e-12 : 1e-5);
    if (!o) return 0;
    ka.opt_flags = o->flags & ~kOptSecondOpinion;
    ka.probe = o->probe;
    ka.warm_state = o->warm_state;
    ka.warm_start = o->warm_state ? o->warm_start : 0;
    ka.warm_shift = o->warm_state ? o->warm_shift : 0;
    if (ka.warm_start < 0 || ka.warm_start > MPCQP_WARM_ACTIVE_SET) return MPCQP_EINVAL;
    ka.warm_state_bytes = o->warm_state ? o->warm_state_bytes : 0;
    ka.factor_slot = o->factor_slot & 1;
    ka.order = o->order;
    return 0;
}

int layout_for(const KernelArgs &ka, bool stepA, bool stepB, int mode, int dtype, Layout &L)
{
    L = make_layout(ka.nx, ka.nu, ka.N, ka.n, ka.m, stepA, stepB, mode, elem_size(dtype));
    if ((size_t)L.total * elem_size(dtype) > kLdsBytesPerCU) return MPCQP_ETOOLARGE;
    if (ka.n > 256) return MPCQP_ETOOLARGE;
    return 0;
}

// Dispatch overrides are explicit bits of MpcqpSolveOpts.flags (no process-wide state):
// MPCQP_OPT_FORCE_LDS routes small problems through the general LDS kernel too, MPCQP_OPT_FORCE_GWS keeps
// large QPs on the general kernel with its arrays in the workspace, MPCQP_OPT_FORCE_DENSE_G makes the fused
// large path form G instead of applying it through the roll-out (cross-checks of two formulations).
bool force_lds(int fl) { return fl & MPCQP_OPT_FORCE_LDS; }
bool force_gws(int fl) { return fl & MPCQP_OPT_FORCE_GWS; }
bool force_dense_g(int fl) { return fl & MPCQP_OPT_FORCE_DENSE_G; }
// the overrides that take a launch off the automatic choice of kernel (the cross-check tests of the kernels)
constexpr int kOverrideFlags =
    MPCQP_OPT_FORCE_LDS | MPCQP_OPT_FORCE_GWS | MPCQP_OPT_FORCE_DENSE_G | MPCQP_OPT_FORCE_CONDENSED | MPCQP_OPT_ONE_PER_WAVE;
// the flags by which a launch names its small-problem kernel or its start itself
constexpr int kChoiceFlags =
    MPCQP_OPT_FORCE_LDS | MPCQP_OPT_ONE_PER_WAVE | MPCQP_OPT_TWO_PER_WAVE | MPCQP_OPT_FOUR_PER_WAVE | MPCQP_OPT_SEED_VIOLATED;
// what a launch keeps of, or takes from, the stage-wise kernels' factor
constexpr int kFactorFlags = MPCQP_OPT_KEEP_FACTOR | MPCQP_OPT_REUSE_FACTOR | MPCQP_OPT_PIPELINE_FACTOR;
// MPCQP_OPT_ON_CHIP_32 in the fused and the QP-given export: no other choice of kernel, start or factor next to it (the
// shared-model exports hold it to kChoiceFlags only: the other flags have no meaning there and are ignored as ever)
constexpr int kOnChip32Alone = kOverrideFlags | kChoiceFlags | kFactorFlags;
// every combination of overrides a launch may carry: the workspace queries, which see no opts, report the
// largest amount any of them needs
const int kFlagVariants[] = {0, MPCQP_OPT_FORCE_LDS, MPCQP_OPT_FORCE_GWS, MPCQP_OPT_FORCE_DENSE_G, MPCQP_OPT_FORCE_CONDENSED};

// A size query carries the dimensions only, no operands (a launch always carries A: check_problem). It is priced for the
// bulkiest operand layout (per-step A and B on chip, both layouts of the wide kernel) and for the second opinion.
bool size_query(const KernelArgs &ka) { return !ka.A.ptr; }

// float64 problems that would take the dense HBM-resident path (nx <= 16, nu > 4, n <= 256: condense + one QP per workgroup)
// go to the general stage-wise kernel instead, unless an override flag asks for the dense solvers: since its second version
// (round 4) it is 15-20x faster there (512 problems of nx = 12, nu = 6, N = 40: 124 against 8.4 ms). float32 keeps the dense
// path (MFMA Gram, float32 solver), which is what makes that size affordable in float32.
static bool prefer_general(const KernelArgs &ka, int dtype)
{
    return dtype == MPCQP_F64 && !(ka.opt_flags & kOverrideFlags) && !ka.warm_state && stageg_supported(ka, MPCQP_F64);
}

// Fused build+solve of mid-size problems of small systems goes to the stage-wise kernel (mpcqp_stage.hip): same
// minimiser (tests), 1.5-1.9x the mid-size condensed kernel on config 3. Its slots hold min(n, m) <= 128 active rows, i.e.
// every row that can be active at once, so nothing is lost against the condensed kernels.
// Beyond n = 128 (round 3) the wide kernel is 1.3-2x faster where many rows become active and ties where few do
// (tools/probe_long_narrow.py, tools/probe_narrow_vs_wide.py); the narrow one stays reachable through mpcqp_stagewise_solve_batch.
bool use_stage_auto(const KernelArgs &ka, int dtype)
{
    return !(ka.opt_flags & kOverrideFlags) && stage_supported(ka, dtype) && ka.n > 16 && ka.n <= 128 && ka.m >= 1;
}

// Fused build+solve of problems that do NOT fit the on-chip condensed kernels goes to the wide stage-wise kernel
// (mpcqp_stagew.hip) when the system fits it (nx <= 16, nu <= 4): same minimiser (tests), 7-10x the HBM-resident
// condensed path at BASELINE config 5's size, and float32 errors ~300x smaller (nothing is squared into P). Its slots
// hold min(n, m, 256) active rows -- every row that can be active at once where the condensed path exists (n <= 256).
bool fits_on_chip(const KernelArgs &ka, bool stepA, bool stepB, int mode, int dtype);
bool use_stagew_auto(const KernelArgs &ka, int dtype)
{
    // Round 3: ... and what DOES fit on chip but is no small problem (n > 24, n > 20 since round 6): measured on batches of 512 random LTV problems
    // (tools/probe_f32_dispatch.py), the stage-wise kernel is 2-2.5x the mid-size / LDS condensed kernels in float64 (nx = 6 .. 12,
    // n = 37 .. 64: 590-980 us against 1180-2170 us) and 2-3x in float32, where it is also 5-30x closer to the float64 oracle
    // (the condensed float32 path squares the conditioning into P: 1e-3 at n ~ 130). Small problems stay on chip: up to n = 20 since
    // round 6 (4096 problems, float64, default / wide stage-wise, us: (nx, nu, N) = (8, 2, 10) n = 20: 824 / 843; (8, 2, 12) n = 24:
    // 1471 / 1087; (12, 4, 6): 860 / 490; (7, 1, 24): 2332 / 1123; (6, 2, 12): 683 / 535; n <= 16: the on-chip kernels by 1.2-2.3x).
    return !(ka.opt_flags & kOverrideFlags) && !(ka.warm_state && ka.warm_start == MPCQP_WARM_OPERATOR) && stagew_supported(ka, dtype) && ka.m >= 1 &&
           ((ka.n > 20 && (dtype == MPCQP_F64 || ka.nx <= 12)) || !fits_on_chip(ka, true, true, MODE_FUSED, dtype));
    // (float32 with nx > 12 -- the LDS-tiled Riccati recursion -- stays on chip while it fits: on borderline problems of that size
    // the condensed float32 kernel was the closer one, 1e-3 against 3e-3)
}
// the narrow stage-wise kernel's unsolved verdicts get a second opinion from the wide one (kOptSecondOpinion) in every launch of
// mpcqp_build_solve_batch / mpcqp_stagewise_solve_batch that it serves, the stateful ones included (KEEP / REUSE / PIPELINE_FACTOR,
// a warm state): the wide kernel runs in a region of its own after the narrow kernel's workspace (Route::off2), so the
// factor images and the vectors a warm record points at survive it, and it neither reads nor writes the warm record
bool second_opinion_applies(const KernelArgs &ka, int dtype)
{
    // (a size query carries neither outputs nor options: it prices the launch that takes the second opinion)
    return stagew_supported(ka, dtype) && (size_query(ka) || ka.status);
}
int64_t al256(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
// the wide kernel's arguments behind the narrow one: only what the narrow kernel left unsolved, nothing kept, no warm record
KernelArgs second_opinion_args(const KernelArgs &ka)
{
    KernelArgs kb = ka;
    kb.opt_flags = (ka.opt_flags | kOptSecondOpinion) & ~kFactorFlags;
    kb.warm_state = nullptr;
    kb.warm_state_bytes = 0;
    kb.warm_start = 0;
    kb.probe = nullptr;
    return kb;
}
int stagew_auto_maxq(const KernelArgs &ka)
{
    const int q = ka.n < ka.m ? ka.n : ka.m;
    return q < 256 ? q : 256;
}

bool use_bigsolve(int n, int m, int dtype, int fl) { return !force_gws(fl) && m > 0 && bigsolve_supported(n, m, dtype); }

// Per-problem solver scratch (elements) for QPs that do not fit the on-chip kernels.
size_t solver_ws_elems(int n, int m, int dtype, int fl)
{
    if (use_bigsolve(n, m, dtype, fl)) return (size_t)m * n + bigsolve_ws_elems(n);  // G' + M_A + N*
    const Layout L = make_layout(1, 1, n, n, m, false, false, MODE_SOLVE, elem_size(dtype));
    return (size_t)L.total;
}

bool use_struct(const KernelArgs &ka, int dtype)
{
    return !force_gws(ka.opt_flags) && !force_dense_g(ka.opt_flags) && bigsolve_struct_supported(ka, dtype);
}

// Sizes (in elements) of the pieces of the large-path workspace, per problem.
struct BigPlan {
    size_t psi, P, q, G, h, nrm, solver;  // psi includes the residual vector
    bool matrix_free;                     // G applied through the roll-out, never formed
    size_t total(bool with_qp) const { return psi + (with_qp ? P + q + G + h + nrm : 0) + solver; }
};

BigPlan big_plan(const KernelArgs &ka, int dtype, bool condense, bool solve)
{
    BigPlan b{};
    if (condense) b.psi = big_condense_ws_elems(ka);
    if (solve) {
        b.matrix_free = use_struct(ka, dtype);
        b.P = (size_t)ka.n * ka.n;
        b.q = ka.n;
        b.h = ka.m;
        if (b.matrix_free) {
            b.nrm = ka.m;
            b.solver = bigsolve_ws_elems(ka.n);
        } else {
            b.G = (size_t)ka.m * ka.n;
            b.solver = solver_ws_elems(ka.n, ka.m, dtype, ka.opt_flags);
        }
    }
    return b;
}

// Mid-size fused problems (config 3) go to the lean one-launch kernel unless the small-problem kernel
// takes them or MPCQP_OPT_FORCE_LDS asks for the all-in-LDS kernel (cross-checks).
bool use_mid(const KernelArgs &ka, int dtype)
{
    return !force_lds(ka.opt_flags) && !w64_eligible(ka, MODE_FUSED, dtype) && mid_supported(ka, dtype);
}

bool fits_on_chip(const KernelArgs &ka, bool stepA, bool stepB, int mode, int dtype)
{
    if (!force_lds(ka.opt_flags) && w64_eligible(ka, mode, dtype)) return true;
    Layout L;
    return layout_for(ka, stepA, stepB, mode, dtype, L) == 0;
}

// Solve QPs given in HBM (ka.P/q/G/h) with the solver arrays in the workspace (n <= 256 and the workspace's size: route()).
int run_gws_solve(KernelArgs ka, int dtype, int64_t batch, void *ws, hipStream_t st)
{
    const size_t esz = elem_size(dtype);
    if (use_bigsolve(ka.n, ka.m, dtype, ka.opt_flags)) {
        // L^-1 packed in LDS, lazy rows of M; needs G transposed (coalesced slack updates)
        void *GT = ws;
        void *rest = (char *)ws + (size_t)ka.m * ka.n * esz * (size_t)batch;
        int rc = launch_transpose(ka.G, GT, ka.m, ka.n, dtype, batch, st);
        if (rc) return rc;
        return launch_bigsolve(ka, dtype, batch, ka.P, ka.q, ka.G, GT, ka.h, rest, st);
    }
    const Layout L = make_layout(ka.nx, ka.nu, ka.N, ka.n, ka.m, false, false, MODE_SOLVE, esz);
    ka.ws = ws;
    return dispatch_gws_solve(ka, L, dtype, batch, st);
}

// the workgroup kernel with everything in LDS (the shared-model mode carves like the solver: the model stays in HBM)
template <int MODE>
int run_lds(const KernelArgs &ka, bool stepA, bool stepB, int dtype, int64_t batch, hipStream_t st)
{
    Layout L;
    int rc = layout_for(ka, stepA, stepB, MODE == MODE_MODEL ? MODE_SOLVE : MODE, dtype, L);
    if (rc) return rc;
    return dispatch_lds<MODE>(ka, L, dtype, batch, st);
}

// ---- float32 problems of the on-chip condensed kernels' sizes are SOLVED IN FLOAT64 (round 4). Those kernels form
// P = w_u I + Psi' W Psi in the launch's arithmetic, which squares the conditioning: a stress run (tools/stress_f32.py)
// returned float32 plans 2e-2 from the float64 ones as SOLVED on ill-conditioned small problems, and nothing the float32
// kernel holds can certify such a plan. The problems in question are a few KB each, so the launch converts the operands
// into the caller's workspace (one kernel), runs the float64 dispatch on the copies and rounds the plan (and the
// multipliers) back: the float32 contract (1e-3) is then met with five digits to spare. Large problems that the wide
// stage-wise kernel takes (n > 160: BASELINE config 5) stay in float32 -- nothing is squared there --, and so does every
// launch that carries a dispatch override (the cross-check tests of the float32 kernels).
struct ConvSeg {
    const void *src;
    void *dst;
    int64_t count;       // elements written (densely packed)
    int64_t row = 0;     // > 0: the source is `count / row` runs of `row` elements, `src_stride` elements apart (a padded batch stride)
    int64_t src_stride = 0;
};
struct ConvPlan {
    ConvSeg seg[10];
    int nseg;
    int to_double;  // float -> double, else double -> float
};
__global__ void __launch_bounds__(256) mpcqp_convert_kernel(const ConvPlan cp)
{
    const ConvSeg sg = cp.seg[blockIdx.y];
    const int64_t stride = (int64_t)gridDim.x * 256;
    if (cp.to_double) {
        const float *a = (const float *)sg.src;
        double *b = (double *)sg.dst;
        if (sg.row > 0) {  // (rows of a padded source packed densely)
            for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < sg.count; i += stride) {
                const int64_t r = i / sg.row;
                b[i] = (double)a[r * sg.src_stride + (i - r * sg.row)];
            }
            return;
        }
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < sg.count; i += stride) b[i] = (double)a[i];
    } else {
        const double *a = (const double *)sg.src;
        float *b = (float *)sg.dst;
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < sg.count; i += stride) b[i] = (float)a[i];
    }
}
int launch_convert(const ConvPlan &cp, hipStream_t st)
{
    if (cp.nseg == 0) return 0;
    int64_t mx = 0;
    for (int i = 0; i < cp.nseg; ++i) mx = cp.seg[i].count > mx ? cp.seg[i].count : mx;
    int64_t gx = (mx + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 1024 ? 1024 : gx);
    hipLaunchKernelGGL(mpcqp_convert_kernel, dim3((unsigned)gx, (unsigned)cp.nseg), dim3(256), 0, st, cp);
    return (int)hipGetLastError();
}

// elements one operand occupies: `block` per step, N steps unless shared along the horizon, `batch` problems unless shared
int64_t operand_elems(const MpcqpOperand &op, int64_t block, int N, int64_t batch, bool per_step)
{
    if (!op.ptr) return 0;
    const int64_t per_problem = (per_step && op.step_stride) ? (int64_t)N * block : block;
    return op.batch_stride ? (batch - 1) * op.batch_stride + per_problem : per_problem;
}

// ---- The dispatch table. route() decides, for one launch, which path runs, with how many slots, and the workspace that
// path needs, laid out. The launch entry points follow it, and the size queries report the largest route over what they
// cannot see (the override flags, the operands' bulk). A new path or kernel is one entry here. What a launch may not combine is
// refused by refusal(), before the route is made (and, for the rules that read the route, after).
// Paths: Refused (Route::rc), OnChip (no workspace: Route::kernel names the launcher), Narrow (narrow stage-wise kernel, then the
// wide one as its second opinion where that applies), Wide, Mid (mid-size condensed kernel), General (general stage-wise kernel),
// the dense HBM-resident path with G applied through the roll-out (DenseStruct) or formed (DenseGws; for a QP that is given:
// Kernel::GwsSolve alone), and Promote (promote_f32).
enum class Path { Refused, OnChip, Narrow, Wide, Mid, General, DenseStruct, DenseGws, Promote };
// The launchers behind Path::OnChip, one value each: launch_quad4, launch_quad, launch_pair, launch_w64 and the workgroup kernel
// (run_lds) in their modes, launch_duo and its shared-model and QP-given modes, launch_quad_model, launch_pair_model;
// run_gws_solve for a given QP that does not fit on chip; and launch_w64_loop (run() hands it the export's LoopArgs).
// None: the path is the launcher.
enum class Kernel { None, Quad4, Quad, Pair, W64Fused, W64Solve, W64Model, LdsFused, LdsSolve, LdsModel, Duo, DuoModel, DuoQp, QuadModel, PairModel, GwsSolve, W64Loop };

struct Entry {
    // mpcqp_build_solve_batch, mpcqp_stagewise_solve_batch, mpcqp_wip_periods_batch, the shared-model solves, mpcqp_solve_batch,
    // mpcqp_model_periods_batch
    enum Kind { BUILD_SOLVE, STAGEWISE, WIP_PERIODS, MODEL, QP_GIVEN, MODEL_PERIODS } kind = BUILD_SOLVE;
    int max_active = 0;                  // STAGEWISE: slots asked for (<= 0: the kernel's default)
    bool general = false, wide = false;  // STAGEWISE: MPCQP_OPT_STAGE_GENERAL / MPCQP_OPT_STAGE_WIDE
    bool bulky = false;                  // BUILD_SOLVE size queries: operands too bulky for the mid-size kernel's LDS
    bool own_e = false;                  // MODEL: bounds per problem (mpcqp_solve_model_bounds_batch with e)
};

struct Route {
    Path path = Path::Refused;
    Kernel kernel = Kernel::None;
    int rc = 0;         // Refused: the launch's return code; Promote: that of the float64 size query
    int maxq = 0;       // slots of the stage-wise kernel
    int maxq2 = 0;      // Narrow: slots of the second opinion (0: no second opinion)
    size_t off2 = 0;    // Narrow: byte offset of the second opinion's region
    size_t bytes = 0;   // workspace (Promote: the operand copies at their largest -- the launch packs the ones it makes)
    size_t inner = 0;   // Promote: workspace of the float64 launch, after the copies
};

// (simds: for the batch-size rule of the four-per-wavefront kernels. A launch hands over SimdCount{}, which asks the device on first
// use; the size queries a constant, since no on-chip route needs a workspace)
Route route(const KernelArgs &ka, int dtype, int64_t batch, const Entry &e, SimdCount simds = SimdCount{0});

bool promote_f32(const KernelArgs &ka, int dtype)
{
    if (dtype != MPCQP_F32 || (ka.opt_flags & kOverrideFlags) || ka.m < 1) return false;
    // The wide stage-wise kernel squares nothing, and BASELINE config 5 (n = 256) comes out 1e-6 from the float64 plan in
    // float32 -- but on adversarial mid-size families (bounds at the edge of consistency, 60-270 iterations) one plan in
    // ~1500 came back SOLVED 1.4e-3 .. 3.6e-3 away with every active row on its bound to rounding noise: the error sits in the
    // float32 Riccati sweeps themselves (V_a = P^-1 g_a'), where no residual this kernel can evaluate in float32 sees it.
    // Mid-size float32 problems (n <= kPromoteN) are therefore solved in float64 as well (1.5x the float32 time at
    // nx = 8, n = 40); float32 arithmetic is kept where it is what makes the size affordable.
    constexpr int kPromoteN = 160;
    if (use_stagew_auto(ka, MPCQP_F32)) return ka.n <= kPromoteN && use_stagew_auto(ka, MPCQP_F64);
    if (!fits_on_chip(ka, true, true, MODE_FUSED, MPCQP_F32) && !use_mid(ka, MPCQP_F32))
        // Round 5: whatever the general stage-wise kernel serves (nx <= 32, nu <= 8; float64 only) goes there, converted -- also
        // the float32 launches the dense HBM-resident path could hold (nx <= 16, 4 < nu <= 8, n <= 256): that path solves 330 k
        // problems/s where the general kernel, in float64, is an order of magnitude faster (tools/probe_dense_vs_general.py). The
        // dense solvers are left with nu > 8, MPCQP_OPT_FORCE_CONDENSED / _GWS / _DENSE_G and mpcqp_condense_batch + mpcqp_solve_batch.
        return stageg_supported(ka, MPCQP_F64);
    // ... and the float64 dispatch must have a stage-wise / mid-size kernel for it, or an on-chip one for the bulkiest operand layout
    const Path p = route(ka, MPCQP_F64, 1, Entry{}).path;
    return p == Path::Narrow || p == Path::Wide || p == Path::Mid || fits_on_chip(ka, true, true, MODE_FUSED, MPCQP_F64);
}

// Every refusal that reads the options: flag, order and warm-state combinations, the envelope of MPCQP_OPT_ON_CHIP_32, a kernel
// asked for by name where it does not apply. Without a route: the rules that need none (right after fill_opts); with the launch's
// route: the rules that read it. Where two rules refuse one launch the code tells which came first, so each kind keeps the order
// its export always had (tests/test_refusal_codes.py).
int warm_kind(const Route &r);
int refusal(const KernelArgs &ka, int dtype, const Entry &e, const Route *r = nullptr)
{
    const int fl = ka.opt_flags;
    if (r) {
        if (e.kind != Entry::BUILD_SOLVE) return 0;
        // a warm state: on a kernel that keeps a record, and row ids (MPCQP_WARM_ACTIVE_SET) not on the narrow stage-wise kernel, whose
        // record is of its own kind. FORCE_LDS / ONE_PER_WAVE at the pair kernel's sizes is left to the export, which refuses it after
        // the record's size (kept apart: refused here, a short record would answer EUNSUPPORTED instead of EWORKSPACE)
        if (ka.warm_state && !(r->path == Path::OnChip && pair_eligible(ka, MODE_FUSED, dtype))) {
            const int kind = warm_kind(*r);
            if (kind == MPCQP_WARM_KIND_NONE || (ka.warm_start == MPCQP_WARM_ACTIVE_SET && kind == MPCQP_WARM_KIND_STAGE)) return MPCQP_EUNSUPPORTED;
        }
        if ((fl & MPCQP_OPT_PIPELINE_FACTOR) && !(r->path == Path::Narrow && stage_pipeline_supported(ka, dtype))) return MPCQP_EUNSUPPORTED;
        return 0;
    }
    switch (e.kind) {
    case Entry::BUILD_SOLVE: {
        // (MPCQP_F64: float32 launches of the small-problem kernels' size arrive here converted)
        auto pairs = [&] { return pair_eligible(ka, MODE_FUSED, MPCQP_F64); };
        // a pairing order: cold launches of the small-problem fused kernel
        if (ka.order && (ka.warm_state || (fl & (MPCQP_OPT_FORCE_LDS | MPCQP_OPT_ONE_PER_WAVE | MPCQP_OPT_SEED_VIOLATED)) || !pairs())) return MPCQP_EUNSUPPORTED;
        // four problems per wavefront by name: no other kernel named, and one of those kernels applies (nx = 3, 4 reach the one with
        // two rows per lane from the pair kernel's sizes only)
        if ((fl & MPCQP_OPT_FOUR_PER_WAVE) &&
            ((fl & (MPCQP_OPT_FORCE_LDS | MPCQP_OPT_ONE_PER_WAVE | MPCQP_OPT_TWO_PER_WAVE)) ||
             !(quad4_applies(ka) || (quad_applies(ka) && (ka.nx == 2 || ka.nx > 4 || pairs())))))
            return MPCQP_EUNSUPPORTED;
        // 17 .. 32 variables on chip by name: cold launches inside the kernel's envelope, float64 (a float32 launch is converted,
        // promote_f32, and arrives here again in float64 with the flag)
        if ((fl & MPCQP_OPT_ON_CHIP_32) && (!duo_applies(ka) || ka.warm_state || ka.order || (fl & kOnChip32Alone) ||
                                           (dtype != MPCQP_F64 && !promote_f32(ka, dtype))))
            return MPCQP_EUNSUPPORTED;
        return 0;
    }
    case Entry::STAGEWISE: return (ka.order || ka.warm_state) ? MPCQP_EUNSUPPORTED : 0;
    case Entry::WIP_PERIODS: return ka.order ? MPCQP_EUNSUPPORTED : 0;
    // the closed loop of a shared model: the automatic kernel, cold or with the warm start it carries itself
    case Entry::MODEL_PERIODS: return (fl || ka.order || ka.warm_state) ? MPCQP_EUNSUPPORTED : 0;
    case Entry::MODEL: {
        if (ka.warm_state) return MPCQP_EUNSUPPORTED;
        const bool small = pair_eligible(ka, MODE_MODEL, dtype);
        // (a pairing order: the pair kernel's model mode only)
        if (ka.order && ((fl & (MPCQP_OPT_FORCE_LDS | MPCQP_OPT_ONE_PER_WAVE)) || !small)) return MPCQP_EUNSUPPORTED;
        // (the four-per-wavefront kernel has no seed steps: asked for by name, it is refused by name)
        if ((fl & MPCQP_OPT_FOUR_PER_WAVE) && ((fl & kChoiceFlags & ~MPCQP_OPT_FOUR_PER_WAVE) || !small)) return MPCQP_EUNSUPPORTED;
        // (an argument check, kept at its place between the rules: next to an order or FOUR_PER_WAVE such a launch is EUNSUPPORTED)
        if (e.own_e && ka.m < 1) return MPCQP_EINVAL;
        // 17 .. 32 variables on chip (mpcqp_duo.hip, its shared-model mode): float64 inside the kernel's envelope, with no pairing order
        // and no other choice of kernel or start. Bounds per problem past sixteen variables: nothing else serves them, with or without
        // the flag; the model's own bounds: by name only
        const bool on_chip_32 = dtype == MPCQP_F64 && duo_model_applies(ka) && !ka.order && !(fl & kChoiceFlags);
        if ((e.own_e ? !small : (fl & MPCQP_OPT_ON_CHIP_32)) && !on_chip_32) return MPCQP_EUNSUPPORTED;
        return 0;
    }
    case Entry::QP_GIVEN:
        if (ka.order || ka.warm_state) return MPCQP_EUNSUPPORTED;
        // the QP-given mode of the on-chip kernel (mpcqp_duo.hip), by name: float64 inside its envelope
        if ((fl & MPCQP_OPT_ON_CHIP_32) && (dtype != MPCQP_F64 || !duo_qp_applies(ka) || (fl & kOnChip32Alone))) return MPCQP_EUNSUPPORTED;
        return 0;
    }
    return 0;
}

Route route(const KernelArgs &ka, int dtype, int64_t batch, const Entry &e, SimdCount simds)
{
    Route r;
    const size_t nb = (size_t)batch, esz = elem_size(dtype);
    const int fl = ka.opt_flags;
    auto refuse = [&](int rc) {  // (r.path is still Path::Refused)
        r.rc = rc;
        return r;
    };
    auto take = [&](Path p, int maxq, size_t bytes_per_problem) {
        r.path = p;
        r.maxq = maxq;
        r.bytes = bytes_per_problem * nb;
        return r;
    };
    auto wide = [&](int maxq) { return take(Path::Wide, maxq, stagew_ws_elems(ka, maxq, dtype) * esz); };
    auto general = [&](int maxq) { return take(Path::General, maxq, stageg_ws_doubles(ka, maxq) * sizeof(double)); };
    // the narrow kernel's workspace, then -- where the second opinion applies -- the wide kernel's in a region of its own
    auto narrow = [&](int maxq, int maxq2) {
        take(Path::Narrow, maxq, stage_ws_doubles(ka, maxq) * sizeof(double));
        if (maxq2 && second_opinion_applies(ka, dtype)) {
            r.maxq2 = maxq2;
            r.off2 = (size_t)al256((int64_t)r.bytes);
            r.bytes = r.off2 + stagew_ws_elems(ka, maxq2, dtype) * esz * nb;
        }
        return r;
    };
    auto on_chip = [&](Kernel k) {
        r.kernel = k;
        return take(Path::OnChip, 0, 0);
    };
    const bool per_wave_ok = !(fl & (MPCQP_OPT_FORCE_LDS | MPCQP_OPT_ONE_PER_WAVE));  // (no flag against two or four problems per wavefront)
    switch (e.kind) {
    case Entry::QP_GIVEN:  // (refusal() holds MPCQP_OPT_ON_CHIP_32 to the kernel's envelope, here and below)
        if (fl & MPCQP_OPT_ON_CHIP_32) return on_chip(Kernel::DuoQp);
        if (fits_on_chip(ka, false, false, MODE_SOLVE, dtype))
            return on_chip(!force_lds(fl) && w64_eligible(ka, MODE_SOLVE, dtype) ? Kernel::W64Solve : Kernel::LdsSolve);
        if (ka.n > 256) return refuse(MPCQP_ETOOLARGE);
        r.kernel = Kernel::GwsSolve;
        return take(Path::DenseGws, 0, solver_ws_elems(ka.n, ka.m, dtype, fl) * esz);
    case Entry::MODEL: {
        const bool small = pair_eligible(ka, MODE_MODEL, dtype);
        // 17 .. 32 variables on chip: bounds per problem past the small-problem kernels, the model's own bounds by name only (the
        // default route of these sizes, the workgroup kernel below, stays)
        if (e.own_e ? !small : (fl & MPCQP_OPT_ON_CHIP_32)) return on_chip(Kernel::DuoModel);
        // (bounds per problem: the model modes of the small-problem kernels, whatever the flags)
        if (small && (e.own_e || per_wave_ok)) return on_chip(quad_model_eligible(ka, batch, simds) ? Kernel::QuadModel : Kernel::PairModel);
        if (!force_lds(fl) && w64_eligible(ka, MODE_MODEL, dtype)) return on_chip(Kernel::W64Model);
        Layout L;
        if (int rc = layout_for(ka, false, false, MODE_SOLVE, dtype, L)) return refuse(rc);
        return on_chip(Kernel::LdsModel);
    }
    case Entry::MODEL_PERIODS:  // (one loop per wavefront: the period loop is compiled into the one-per-wavefront kernel's MODEL mode)
        return w64_loop_eligible(ka, dtype) ? on_chip(Kernel::W64Loop) : refuse(MPCQP_EUNSUPPORTED);
    case Entry::WIP_PERIODS:  // (the closed-loop epilogue is compiled into the narrow kernel; no second opinion)
        return use_stage_auto(ka, dtype) ? narrow(stage_default_maxq(ka), 0) : refuse(MPCQP_EUNSUPPORTED);
    case Entry::STAGEWISE: {
        // (float32 problems the general kernel would take: through mpcqp_build_solve_batch, which converts)
        const bool narrow_ok = stage_supported(ka, dtype), wide_ok = stagew_supported(ka, dtype);
        if (e.general || (!narrow_ok && !wide_ok))
            return stageg_supported(ka, dtype) ? general(e.max_active > 0 ? e.max_active : stageg_default_maxq(ka)) : refuse(MPCQP_EUNSUPPORTED);
        const int maxq = e.max_active > 0 ? e.max_active : stage_default_maxq(ka);
        return (!narrow_ok || (e.wide && wide_ok)) ? wide(maxq) : narrow(maxq, maxq);
    }
    case Entry::BUILD_SOLVE: break;
    }
    if (promote_f32(ka, dtype)) {
        // the copies at their largest (nothing shared, every segment 256-byte aligned), the float64 plan and multipliers, then
        // the float64 launch's own workspace
        r.path = Path::Promote;
        const MpcqpDims d64{ka.nx, ka.nu, ka.N, ka.mk, MPCQP_F64, ka.flags, ka.wt, ka.wx, ka.wu};
        r.rc = mpcqp_workspace_bytes(&d64, batch, 1, &r.inner);
        const int64_t N = ka.N, nx = ka.nx, nu = ka.nu, mk = ka.mk;
        const int64_t per = N * (nx * nx + nx * nu + mk * nx + mk * nu + mk) + 2 * nx + N * nx + ka.n + ka.m;
        r.bytes = (size_t)(per * 8 * batch + 10 * 256) + r.inner;
        return r;
    }
    // MPCQP_OPT_ON_CHIP_32: the on-chip kernel for 17 .. 32 variables, no workspace (the size queries carry no flags and never get here)
    if (fl & MPCQP_OPT_ON_CHIP_32) return on_chip(Kernel::Duo);
    if (use_stage_auto(ka, dtype)) return narrow(stage_default_maxq(ka), stagew_auto_maxq(ka));
    if (use_stagew_auto(ka, dtype)) return wide(stagew_auto_maxq(ka));
    if (!e.bulky && use_mid(ka, dtype)) return take(Path::Mid, 0, bigsolve_ws_elems(ka.n) * esz);
    const bool q = size_query(ka);
    if (fits_on_chip(ka, q || ka.A.step_stride, q || ka.B.step_stride, MODE_FUSED, dtype)) {
        // The on-chip tier. Four problems per wavefront with four rows per lane (more than 32 rows, or five to eight per step, at
        // n <= 16) at every batch size: the workgroup / one-per-wavefront kernels it replaces there are 5-9 x slower. With two rows
        // per lane where it pays -- the general layouts and nx > 4 at every batch size, the lean layout from more than two problems
        // per SIMD (quad_eligible) --: on its own for nx = 2 and nx > 4, which have no two-per-wavefront instantiation, and from the
        // pair kernel's sizes for nx = 3, 4. Then two per wavefront, one per wavefront, one per workgroup. (A warm state on the last
        // two is refused by the export.)
        if (dtype == MPCQP_F64 && per_wave_ok) {
            if (quad4_applies(ka)) return on_chip(Kernel::Quad4);
            if ((ka.nx == 2 || ka.nx > 4) && quad_eligible(ka, batch, simds)) return on_chip(Kernel::Quad);
        }
        if (per_wave_ok && pair_eligible(ka, MODE_FUSED, dtype)) return on_chip(quad_eligible(ka, batch, simds) ? Kernel::Quad : Kernel::Pair);
        return on_chip(!force_lds(fl) && w64_eligible(ka, MODE_FUSED, dtype) ? Kernel::W64Fused : Kernel::LdsFused);
    }
    // wide systems on horizons the dense path cannot hold -- and every float64 problem it could hold (prefer_general): the
    // general stage-wise kernel (float64; float32 launches of these dimensions arrive here converted, promote_f32)
    if (!big_supported(ka) || ka.n > 256 || prefer_general(ka, dtype))
        return (stageg_supported(ka, dtype) && !ka.warm_state) ? general(stageg_default_maxq(ka)) : refuse(MPCQP_ETOOLARGE);
    const BigPlan b = big_plan(ka, dtype, true, true);
    return take(b.matrix_free ? Path::DenseStruct : Path::DenseGws, 0, b.total(true) * esz);
}

// whose warm-state record a launch on this route reads and writes (MPCQP_WARM_KIND_*): the small-problem pair kernel's
// (operator + slot ids), the narrow stage-wise kernel's (row ids; the rows' vectors stay in its workspace) or the wide one's
// (row ids only, MPCQP_WARM_ACTIVE_SET)
int warm_kind(const Route &r)
{
    switch (r.path) {
    case Path::Narrow: return MPCQP_WARM_KIND_STAGE;
    case Path::Wide: return MPCQP_WARM_KIND_ROWS;
    case Path::OnChip: return r.kernel == Kernel::Pair ? MPCQP_WARM_KIND_OPERATOR : MPCQP_WARM_KIND_NONE;
    default: return MPCQP_WARM_KIND_NONE;
    }
}

// the warm-state record of the automatic dispatch, per problem; 0 = not offered for these dimensions
// (kind: MPCQP_WARM_KIND_* -- whose record it is; the host side reads it instead of re-deriving the dispatch)
size_t warm_bytes_per_problem(KernelArgs ka, int dtype, int *kind = nullptr)
{
    ka.opt_flags = 0;
    ka.warm_start = 0;
    if (dtype == MPCQP_F32 && promote_f32(ka, dtype)) dtype = MPCQP_F64;  // (the launch that is solved in float64: its kernel's record)
    // routed as the launch that carries a record: the four-per-wavefront kernels, which keep none, step aside for the pair kernel
    // (any pointer will do: route() reads it as a flag)
    ka.warm_state = &ka;
    const Route r = route(ka, dtype, 1, Entry{});
    const int k = warm_kind(r);
    if (kind) *kind = k;
    switch (k) {
    case MPCQP_WARM_KIND_OPERATOR: return kPairWarmDoubles * sizeof(double);
    case MPCQP_WARM_KIND_STAGE: return stage_warm_bytes(r.maxq);
    case MPCQP_WARM_KIND_ROWS: return stagew_warm_bytes(r.maxq);
    default: return 0;
    }
}

// mpcqp_workspace_bytes of a fused build+solve. The query sees dimensions, not operand strides or MpcqpSolveOpts.flags, while
// the launch picks its kernel with both: it reports the largest workspace of the routes over the override flags and over the
// operands' bulk -- the mid-size kernel's LDS holds the most compact operands (LTI, no C / D) where bulkier ones may not fit,
// and such a launch takes the path behind it. Only the automatic dispatch with compact operands refuses: an override
// combination that has no kernel for these dimensions is refused by the launch that carries it, not by the size query.
int workspace_query(const KernelArgs &ka, int dtype, int64_t batch, size_t *bytes)
{
    size_t need = 0;
    for (int fl : kFlagVariants) {
        KernelArgs kv = ka;
        kv.opt_flags = fl;
        for (const bool bulky : {false, true}) {
            const Route r = route(kv, dtype, batch, {Entry::BUILD_SOLVE, 0, false, false, bulky});
            if (r.path == Path::Refused || r.rc) {
                if (fl == 0 && !bulky) return r.rc;
                continue;
            }
            if (r.bytes > need) need = r.bytes;
        }
    }
    *bytes = need;
    return 0;
}

// the narrow stage-wise kernel, then its second opinion (mpcqp_internal.h, kOptSecondOpinion) on the same stream, in the
// region the route set aside after the narrow kernel's workspace
int run_narrow(const KernelArgs &ka, int dtype, const Route &r, int64_t batch, void *ws, hipStream_t st)
{
    int rc = launch_stage(ka, r.maxq, batch, ws, st);
    if (rc || !r.maxq2) return rc;
    rc = launch_stagew(second_opinion_args(ka), dtype, r.maxq2, batch, (char *)ws + r.off2, st);
    return rc == MPCQP_ETOOLARGE ? 0 : rc;  // (a horizon beyond the wide kernel's 32-bit offsets: the narrow kernel's verdicts stand)
}

// HBM-resident path: propagate + Gram (MFMA for f32) into the workspace, then the general solver with its arrays in the
// workspace as well
int run_dense(KernelArgs ka, int dtype, int64_t batch, void *workspace, hipStream_t st)
{
    const size_t esz = elem_size(dtype), nb = (size_t)batch;
    const BigPlan b = big_plan(ka, dtype, true, true);
    char *w = (char *)workspace;
    void *psi_ws = w;
    void *res_ws = w + (size_t)(ka.N + 1) * ka.nx * ka.n * nb * esz;
    w += b.psi * nb * esz;
    void *Pw = w;
    w += b.P * nb * esz;
    void *qw = w;
    w += b.q * nb * esz;
    void *Gw = w;
    w += b.G * nb * esz;
    void *hw = w;
    w += b.h * nb * esz;
    int rc;
    if (b.matrix_free) {
        void *nw = w;
        w += b.nrm * nb * esz;
        if ((rc = launch_big_condense(ka, dtype, batch, psi_ws, res_ws, Pw, qw, nullptr, hw, nw, st))) return rc;
        return launch_bigsolve_struct(ka, dtype, batch, Pw, qw, psi_ws, hw, nw, w, st);
    }
    if ((rc = launch_big_condense(ka, dtype, batch, psi_ws, res_ws, Pw, qw, Gw, hw, nullptr, st))) return rc;
    ka.P = Pw;
    ka.q = qw;
    ka.G = Gw;
    ka.h = hw;
    return run_gws_solve(ka, dtype, batch, w, st);
}

// The launch of a route: its kernel's launcher, or the path's where the path is the launcher. stepA / stepB: A and B per step
// (the workgroup kernel's carve in the fused mode).
int run(const Route &r, const KernelArgs &ka, bool stepA, bool stepB, int dtype, int64_t batch, void *ws, hipStream_t st,
        const LoopArgs *loop = nullptr)  // (loop: what Kernel::W64Loop takes next to KernelArgs)
{
    switch (r.kernel) {
    case Kernel::Quad4: return launch_quad4(ka, batch, st);
    case Kernel::Quad: return launch_quad(ka, batch, st);
    case Kernel::Pair: return launch_pair(ka, batch, st);
    case Kernel::W64Fused: return launch_w64(ka, MODE_FUSED, dtype, batch, st);
    case Kernel::W64Solve: return launch_w64(ka, MODE_SOLVE, dtype, batch, st);
    case Kernel::W64Model: return launch_w64(ka, MODE_MODEL, dtype, batch, st);
    case Kernel::LdsFused: return run_lds<MODE_FUSED>(ka, stepA, stepB, dtype, batch, st);
    case Kernel::LdsSolve: return run_lds<MODE_SOLVE>(ka, false, false, dtype, batch, st);
    case Kernel::LdsModel: return run_lds<MODE_MODEL>(ka, false, false, dtype, batch, st);
    case Kernel::Duo: return launch_duo(ka, batch, st);
    case Kernel::DuoModel: return launch_duo_model(ka, batch, st);
    case Kernel::DuoQp: return launch_duo_qp(ka, batch, st);
    case Kernel::QuadModel: return launch_quad_model(ka, batch, st);
    case Kernel::PairModel: return launch_pair_model(ka, batch, st);
    case Kernel::GwsSolve: return run_gws_solve(ka, dtype, batch, ws, st);
    case Kernel::W64Loop: return loop ? launch_w64_loop(ka, *loop, batch, st) : MPCQP_EINVAL;
    case Kernel::None: break;
    }
    switch (r.path) {
    case Path::Narrow: return run_narrow(ka, dtype, r, batch, ws, st);
    case Path::Wide: return launch_stagew(ka, dtype, r.maxq, batch, ws, st);
    case Path::Mid: return launch_mid(ka, dtype, batch, ws, st);
    case Path::General: return launch_stageg(ka, r.maxq, batch, ws, st);
    case Path::DenseStruct:
    case Path::DenseGws: return run_dense(ka, dtype, batch, ws, st);
    default: return MPCQP_ETOOLARGE;  // (Refused and Promote are the exports' business)
    }
}

}  // namespace

extern "C" {

int mpcqp_abi_version(void) { return MPCQP_ABI_VERSION; }

const char *mpcqp_error_string(int code)
{
    switch (code) {
    case 0: return "ok";
    case MPCQP_EINVAL: return "invalid argument";
    case MPCQP_ETOOLARGE: return "no kernel for these dimensions (the stage-wise kernels serve nx <= 32, nu <= 8 at any horizon; the dense HBM-resident path any system with n <= 256)";
    case MPCQP_EDTYPE: return "dtype must be MPCQP_F64 or MPCQP_F32";
    case MPCQP_ELAYOUT: return "step stride must be 0 or the block size, batch stride 0 or at least a problem's extent, neither negative (the fused WIP periods take packed x0 / goal / targets only: MPCQP_EUNSUPPORTED)";
    case MPCQP_EWORKSPACE: return "workspace missing or too small (see mpcqp_workspace_bytes)";
    case MPCQP_EUNSUPPORTED: return "option not available for these dimensions / this dtype (warm start: n <= 16, m <= 32, float64)";
    default: break;
    }
    if (code > 0) return hipGetErrorString((hipError_t)code);
    return "unknown error";
}

int mpcqp_lds_bytes(const MpcqpDims *dims, size_t *bytes)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!bytes) return MPCQP_EINVAL;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    Layout L = make_layout(ka.nx, ka.nu, ka.N, ka.n, ka.m, true, true, MODE_FUSED, elem_size(dims->dtype));
    *bytes = (size_t)L.total * elem_size(dims->dtype);
    return (*bytes > kLdsBytesPerCU || ka.n > 256) ? MPCQP_ETOOLARGE : 0;
}

int mpcqp_warm_state_bytes(const MpcqpDims *dims, size_t *bytes)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!bytes) return MPCQP_EINVAL;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    *bytes = warm_bytes_per_problem(ka, dims->dtype);
    return 0;
}

int mpcqp_warm_state_kind(const MpcqpDims *dims, int32_t *kind)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!kind) return MPCQP_EINVAL;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    int k = MPCQP_WARM_KIND_NONE;
    warm_bytes_per_problem(ka, dims->dtype, &k);
    *kind = k;
    return 0;
}

int mpcqp_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t for_solve, size_t *bytes)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!bytes || batch < 0) return MPCQP_EINVAL;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    *bytes = 0;
    if (for_solve) return workspace_query(ka, dims->dtype, batch, bytes);
    // mpcqp_condense_batch: on chip, or the HBM-resident propagation
    if (fits_on_chip(ka, true, true, MODE_CONDENSE, dims->dtype)) return 0;
    if (!big_supported(ka)) return MPCQP_ETOOLARGE;
    *bytes = big_condense_ws_elems(ka) * elem_size(dims->dtype) * (size_t)batch;
    return 0;
}

int mpcqp_solve_workspace_bytes(int32_t n, int32_t m, int32_t dtype, int64_t batch, size_t *bytes)
{
    if (dtype != MPCQP_F64 && dtype != MPCQP_F32) return MPCQP_EDTYPE;
    if (n <= 0 || m < 0 || batch < 0 || !bytes) return MPCQP_EINVAL;
    KernelArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.n = n;
    ka.m = m;
    ka.nx = ka.nu = 1;
    ka.N = n;
    *bytes = 0;
    if (fits_on_chip(ka, false, false, MODE_SOLVE, dtype)) return 0;
    if (n > 256) return MPCQP_ETOOLARGE;
    size_t need = 0;
    for (int fl : kFlagVariants) {
        const size_t v = solver_ws_elems(n, m, dtype, fl) * elem_size(dtype) * (size_t)batch;
        if (v > need) need = v;
    }
    *bytes = need;
    return 0;
}

int mpcqp_condense_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, void *P,
                         void *q, void *G, void *h, void *Phi, void *Psi, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    if (batch < 0 || !P || !q || (dims->mk > 0 && (!G || !h))) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    fill_args(ka, dims, problem);
    ka.P = P;
    ka.q = q;
    ka.G = G;
    ka.h = h;
    ka.Phi = Phi;
    ka.Psi = Psi;
    hipStream_t st = (hipStream_t)stream;
    Layout L;
    rc = layout_for(ka, problem->A.step_stride != 0, problem->B.step_stride != 0, MODE_CONDENSE, dims->dtype, L);
    if (rc == 0) {
        if ((rc = dispatch_lds<MODE_CONDENSE>(ka, L, dims->dtype, batch, st))) return rc;
    } else if (rc == MPCQP_ETOOLARGE && big_supported(ka)) {
        // HBM-resident path: Psi goes to the caller's Psi buffer when given, else to the workspace
        const size_t esz = elem_size(dims->dtype);
        const size_t psi_el = (size_t)(ka.N + 1) * ka.nx * ka.n * (size_t)batch;
        const size_t res_el = (size_t)(ka.N + 1) * ka.nx * (size_t)batch;
        const size_t need = (Psi ? res_el : psi_el + res_el) * esz;
        if (!workspace || workspace_bytes < need) return MPCQP_EWORKSPACE;
        void *psi_ws = Psi ? Psi : workspace;
        void *res_ws = Psi ? workspace : (void *)((char *)workspace + psi_el * esz);
        if ((rc = launch_big_condense(ka, dims->dtype, batch, psi_ws, res_ws, P, q, G, h, nullptr, st))) return rc;
    } else {
        return rc;
    }
    if (Phi) rc = launch_phi(ka, dims->dtype, batch, st);
    return rc;
}

int mpcqp_update_vectors_batch(const MpcqpDims *dims, const MpcqpProblem *problem, const void *Phi,
                               int64_t phi_batch_stride, const void *Psi, int64_t psi_batch_stride,
                               int64_t batch, void *q, void *h, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!problem || !problem->x0.ptr || !Phi || batch < 0) return MPCQP_EINVAL;
    if (q && !Psi) return MPCQP_EINVAL;
    if (h && dims->mk > 0 && !problem->e.ptr) return MPCQP_EINVAL;
    if ((dims->flags & MPCQP_Q_TERMINAL) && q && !problem->goal.ptr) return MPCQP_EINVAL;
    if ((dims->flags & MPCQP_Q_STAGE) && q && !problem->targets.ptr) return MPCQP_EINVAL;
    if ((rc = check_layout(dims, problem))) return rc;
    if (batch == 0 || (!q && !h)) return 0;
    KernelArgs ka;
    fill_args(ka, dims, problem);
    ka.Phi = const_cast<void *>(Phi);
    ka.Psi = const_cast<void *>(Psi);
    ka.q = q;
    ka.h = h;
    return launch_update(ka, dims->dtype, phi_batch_stride, psi_batch_stride, batch, (hipStream_t)stream);
}

int mpcqp_condense_phase_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t phase, void *P,
                               void *q, void *G, void *h, void *Psi, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    if (batch < 0 || (phase != 1 && phase != 2) || !Psi) return MPCQP_EINVAL;
    if (phase == 1 && dims->mk > 0 && (!G || !h)) return MPCQP_EINVAL;
    if (phase == 2 && (!P || !q)) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    fill_args(ka, dims, problem);
    ka.P = P;
    ka.q = q;
    ka.G = G;
    ka.h = h;
    ka.Psi = Psi;
    Layout L;
    // only where mpcqp_condense_batch itself runs as two launches: problems that do not fit a CU's LDS
    if (layout_for(ka, problem->A.step_stride != 0, problem->B.step_stride != 0, MODE_CONDENSE, dims->dtype, L) == 0 || !big_supported(ka))
        return MPCQP_EUNSUPPORTED;
    const size_t need = (size_t)(ka.N + 1) * ka.nx * (size_t)batch * elem_size(dims->dtype);  // the tracking residuals
    if (!workspace || workspace_bytes < need) return MPCQP_EWORKSPACE;
    return launch_big_condense(ka, dims->dtype, batch, Psi, workspace, P, q, G, h, nullptr, (hipStream_t)stream, phase);
}

int mpcqp_solve_batch(int32_t n, int32_t m, int32_t dtype, const void *P, const void *q, const void *G,
                      const void *h, int64_t batch, const MpcqpSolveOpts *opts, void *x, void *lam,
                      int32_t *status, int32_t *iters, void *workspace, size_t workspace_bytes, void *stream)
{
    if (dtype != MPCQP_F64 && dtype != MPCQP_F32) return MPCQP_EDTYPE;
    if (n <= 0 || m < 0 || batch < 0 || !P || !q || !x || (m > 0 && (!G || !h))) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    memset(&ka, 0, sizeof(ka));
    ka.n = n;
    ka.m = m;
    ka.nx = 1;
    ka.nu = 1;
    ka.N = n;
    ka.P = const_cast<void *>(P);
    ka.q = const_cast<void *>(q);
    ka.G = const_cast<void *>(G);
    ka.h = const_cast<void *>(h);
    ka.U = x;
    ka.lam = lam;
    ka.status = status;
    ka.iters = iters;
    const Entry entry{Entry::QP_GIVEN};
    int rc = fill_opts(ka, opts, dtype);
    if (rc || (rc = refusal(ka, dtype, entry))) return rc;
    const Route r = route(ka, dtype, batch, entry, SimdCount{});
    if (r.path == Path::Refused) return r.rc;
    if (r.path != Path::OnChip && (!workspace || workspace_bytes < r.bytes)) return MPCQP_EWORKSPACE;
    return run(r, ka, false, false, dtype, batch, workspace, (hipStream_t)stream);
}

int mpcqp_build_solve_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                            const MpcqpSolveOpts *opts, void *U, void *lam, int32_t *status,
                            int32_t *iters, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    if (batch < 0 || !U) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    fill_args(ka, dims, problem);
    ka.U = U;
    ka.lam = lam;
    ka.status = status;
    ka.iters = iters;
    const Entry entry{Entry::BUILD_SOLVE};
    if ((rc = fill_opts(ka, opts, dims->dtype)) || (rc = refusal(ka, dims->dtype, entry))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Route r = route(ka, dims->dtype, batch, entry, SimdCount{});
    if (r.path == Path::Promote) {
        // float32 at an on-chip condensed kernel's size: solved in float64 on converted copies (see promote_f32)
        const int64_t N = ka.N, nx = ka.nx, nu = ka.nu, mk = ka.mk;
        const MpcqpOperand *src[8] = {&problem->A, &problem->B, &problem->C, &problem->D, &problem->e, &problem->x0, &problem->goal, &problem->targets};
        const int64_t block[8] = {nx * nx, nx * nu, mk * nx, mk * nu, mk, nx, nx, N * nx};
        const bool per_step[8] = {true, true, true, true, true, false, false, false};
        MpcqpProblem p64 = *problem;
        MpcqpOperand *dst[8] = {&p64.A, &p64.B, &p64.C, &p64.D, &p64.e, &p64.x0, &p64.goal, &p64.targets};
        ConvPlan in{};
        in.to_double = 1;
        char *w = (char *)workspace;
        int64_t off = 0;
        for (int i = 0; i < 8; ++i) {
            if (!operand_elems(*src[i], block[i], (int)N, batch, per_step[i])) continue;
            // (mpcqp_workspace_bytes prices the copies densely packed. A source with a PADDED batch stride is packed on the way --
            // round 6; until then it was refused, MPCQP_ELAYOUT --; a padded step stride still is: no caller of this library makes one)
            const int64_t dense = (per_step[i] && src[i]->step_stride) ? N * block[i] : block[i];
            if (per_step[i] && src[i]->step_stride && src[i]->step_stride != block[i]) return MPCQP_ELAYOUT;
            const bool padded = src[i]->batch_stride != 0 && src[i]->batch_stride != dense;
            if (src[i]->batch_stride != 0 && src[i]->batch_stride < dense) return MPCQP_ELAYOUT;
            const int64_t cnt = src[i]->batch_stride ? batch * dense : dense;
            if (w) dst[i]->ptr = w + off;
            if (padded) dst[i]->batch_stride = dense;
            ConvSeg sg{src[i]->ptr, w ? w + off : nullptr, cnt};
            if (padded) {
                sg.row = dense;
                sg.src_stride = src[i]->batch_stride;
            }
            in.seg[in.nseg++] = sg;
            off += al256(cnt * 8);
        }
        const int64_t offU = off;
        off += al256(batch * ka.n * 8);
        const int64_t offL = off;
        if (lam) off += al256(batch * ka.m * 8);
        MpcqpDims d64 = *dims;
        d64.dtype = MPCQP_F64;
        const size_t inner = r.inner;
        if (r.rc) return r.rc;
        if (!workspace || workspace_bytes < (size_t)off + inner) return MPCQP_EWORKSPACE;
        if ((rc = launch_convert(in, st))) return rc;
        MpcqpSolveOpts o64{};
        if (opts) o64 = *opts;
        if (!(o64.feas_tol > 0.0)) o64.feas_tol = 1e-9;  // (float64 arithmetic; the float32 default of 1e-5 would only loosen the plan)
        rc = mpcqp_build_solve_batch(&d64, &p64, batch, &o64, w + offU, lam ? w + offL : nullptr, status, iters,
                                     inner ? w + off : nullptr, inner, stream);
        if (rc) return rc;
        ConvPlan out{};
        out.to_double = 0;
        out.seg[out.nseg++] = ConvSeg{w + offU, U, batch * ka.n};
        if (lam) out.seg[out.nseg++] = ConvSeg{w + offL, lam, batch * ka.m};
        return launch_convert(out, st);
    }
    if ((rc = refusal(ka, dims->dtype, entry, &r))) return rc;
    // the state is indexed by problem: a buffer made for a smaller batch would be read and written out of bounds
    if (ka.warm_state && ka.warm_state_bytes < (size_t)batch * warm_bytes_per_problem(ka, dims->dtype)) return MPCQP_EWORKSPACE;
    if (r.path == Path::Refused) return r.rc;
    if (r.path != Path::OnChip && (!workspace || workspace_bytes < r.bytes)) return MPCQP_EWORKSPACE;
    // (FORCE_LDS / ONE_PER_WAVE at the pair kernel's sizes: the one warm-state refusal that comes after the record's size, see refusal())
    if (ka.warm_state && warm_kind(r) == MPCQP_WARM_KIND_NONE) return MPCQP_EUNSUPPORTED;
    return run(r, ka, problem->A.step_stride != 0, problem->B.step_stride != 0, dims->dtype, batch, workspace, st);
}

int mpcqp_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active, size_t *bytes)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!bytes || batch < 0) return MPCQP_EINVAL;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    // (max_active < 0: the general kernel's workspace, MPCQP_OPT_STAGE_GENERAL: -1 default slots, -k: k slots)
    Entry e{Entry::STAGEWISE, max_active < -1 ? -max_active : max_active, max_active < 0};
    const Route r = route(ka, dims->dtype, batch, e);
    if (r.path == Path::Refused) return r.rc;
    // (the query does not see MpcqpSolveOpts.flags: where both kernels apply it reports the larger workspace)
    e.wide = true;
    const Route w = route(ka, dims->dtype, batch, e);
    *bytes = r.bytes > w.bytes ? r.bytes : w.bytes;
    return 0;
}

int mpcqp_stagewise_solve_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                                const MpcqpSolveOpts *opts, int32_t max_active, void *U, void *lam, int32_t *status,
                                int32_t *iters, void *workspace, size_t workspace_bytes, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    if (batch < 0 || !U) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    fill_args(ka, dims, problem);
    ka.U = U;
    ka.lam = lam;
    ka.status = status;
    ka.iters = iters;
    const bool general = opts && (opts->flags & MPCQP_OPT_STAGE_GENERAL), wide = opts && (opts->flags & MPCQP_OPT_STAGE_WIDE);
    // (as in mpcqp_build_solve_batch: what the narrow kernel leaves MPCQP_MAX_ITER / MPCQP_INFEASIBLE goes through the wide one, with
    // the same slots, in a region of its own after the narrow kernel's workspace -- mpcqp_stagewise_workspace_bytes reports the sum)
    // (this export has always routed first: a system no stage-wise kernel serves is refused as such whatever its options)
    const Entry entry{Entry::STAGEWISE, max_active, general, wide};
    const Route r = route(ka, dims->dtype, batch, entry, SimdCount{});
    if (r.path == Path::Refused) return r.rc;
    if ((rc = fill_opts(ka, opts, dims->dtype)) || (rc = refusal(ka, dims->dtype, entry))) return rc;
    if (!workspace || workspace_bytes < r.bytes) return MPCQP_EWORKSPACE;
    return run(r, ka, false, false, dims->dtype, batch, workspace, (hipStream_t)stream);
}

int mpcqp_model_bytes(const MpcqpDims *dims, size_t *bytes)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!bytes) return MPCQP_EINVAL;
    const ModelLayout ml = make_model_layout(dims->nx, dims->N, dims->N * dims->nu, dims->N * dims->mk);
    *bytes = (ml.total + 4) * elem_size(dims->dtype);
    return 0;
}

int mpcqp_factor_model(const MpcqpDims *dims, const void *P, const void *G, const void *q_basis,
                       const void *h_basis, void *model, size_t model_bytes, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!P || !q_basis || !model || (dims->mk > 0 && (!G || !h_basis))) return MPCQP_EINVAL;
    size_t need = 0;
    mpcqp_model_bytes(dims, &need);
    if (model_bytes < need) return MPCQP_EWORKSPACE;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    return launch_factor_model(ka, dims->dtype, P, G, q_basis, h_basis, model, (hipStream_t)stream);
}

int mpcqp_solve_model_batch(const MpcqpDims *dims, const void *model, const MpcqpOperand *x0,
                            const MpcqpOperand *goal, const MpcqpOperand *targets, int64_t batch,
                            const MpcqpSolveOpts *opts, void *U, void *lam, int32_t *status, int32_t *iters,
                            void *stream)
{
    return mpcqp_solve_model_bounds_batch(dims, model, nullptr, x0, goal, targets, batch, opts, U, lam, status, iters,
                                          stream);
}

int mpcqp_solve_model_bounds_batch(const MpcqpDims *dims, const void *model, const MpcqpOperand *e,
                                   const MpcqpOperand *x0, const MpcqpOperand *goal, const MpcqpOperand *targets,
                                   int64_t batch, const MpcqpSolveOpts *opts, void *U, void *lam, int32_t *status,
                                   int32_t *iters, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!model || !x0 || !x0->ptr || !U || batch < 0) return MPCQP_EINVAL;
    if ((dims->flags & MPCQP_Q_TERMINAL) && !(goal && goal->ptr)) return MPCQP_EINVAL;
    if ((dims->flags & MPCQP_Q_STAGE) && !(targets && targets->ptr)) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    ka.x0 = *x0;
    if (goal) ka.goal = *goal;
    if (targets) ka.targets = *targets;
    ka.model = model;
    ka.U = U;
    ka.lam = lam;
    ka.status = status;
    ka.iters = iters;
    // per-problem bounds: the model modes of the small-problem kernels and of the on-chip-32 kernel
    Entry entry{Entry::MODEL};
    entry.own_e = e && e->ptr;
    if ((rc = fill_opts(ka, opts, dims->dtype)) || (rc = refusal(ka, dims->dtype, entry))) return rc;
    if (entry.own_e) ka.e = *e;
    const Route r = route(ka, dims->dtype, batch, entry, SimdCount{});
    if (r.path == Path::Refused) return r.rc;
    return run(r, ka, false, false, dims->dtype, batch, nullptr, (hipStream_t)stream);
}

int mpcqp_rollout_batch(const MpcqpDims *dims, const MpcqpOperand *A, const MpcqpOperand *B,
                        const MpcqpOperand *x0, const void *U, int64_t batch, void *X, void *stream)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!A || !B || !x0 || !A->ptr || !B->ptr || !x0->ptr || !U || !X || batch < 0) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    ka.A = *A;
    ka.B = *B;
    ka.x0 = *x0;
    ka.U = const_cast<void *>(U);
    ka.X = X;
    return launch_rollout(ka, dims->dtype, batch, (hipStream_t)stream);
}

namespace {
// mpcqp_plan_vjp_batch's workspace, per launch: the condensed P, q, G, h, Phi, Psi of every problem (256-byte aligned
// segments), mpcqp_condense_batch's own scratch, then the adjoint carves when they do not fit LDS. The model export's
// carve is the longer one of the kModel kernel, and a g_x0 the caller did not ask for goes to a scratch segment after it.
struct VjpPlan {
    int64_t P, q, G, h, Phi, Psi, cws, carve, gx0, total;
    size_t cws_bytes;
};

// the condensed segments and mpcqp_condense_batch's scratch: every field up to `carve`
static int condensed_plan(const MpcqpDims *dims, int64_t batch, VjpPlan &v)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (batch < 0) return MPCQP_EINVAL;
    if (dims->dtype != MPCQP_F64) return MPCQP_EDTYPE;
    const int64_t nx = dims->nx, N = dims->N, n = N * dims->nu, m = N * dims->mk;
    if (n > 128) return MPCQP_EUNSUPPORTED;
    size_t cws = 0;
    if ((rc = mpcqp_workspace_bytes(dims, batch, 0, &cws))) return rc == MPCQP_ETOOLARGE ? MPCQP_EUNSUPPORTED : rc;
    const int64_t d = 8 * batch;
    v.P = 0;
    v.q = v.P + al256(d * n * n);
    v.G = v.q + al256(d * n);
    v.h = v.G + al256(d * m * n);
    v.Phi = v.h + al256(d * m);
    v.Psi = v.Phi + al256(d * (N + 1) * nx * nx);
    v.cws = v.Psi + al256(d * (N + 1) * nx * n);
    v.cws_bytes = cws;
    v.carve = v.cws + al256((int64_t)cws);
    return 0;
}

static int vjp_plan(const MpcqpDims *dims, int64_t batch, VjpPlan &v, bool model = false)
{
    const int rc = condensed_plan(dims, batch, v);
    if (rc) return rc;
    const int64_t nx = dims->nx, N = dims->N, n = N * dims->nu, m = N * dims->mk, d = 8 * batch;
    const bool lds = adjoint_carve_in_lds((int)n, (int)N, (int)nx, (int)m, model);
    v.gx0 = v.carve + (lds ? 0 : al256((int64_t)adjoint_carve_bytes((int)n, (int)N, (int)nx, (int)m, model) * batch));
    v.total = v.gx0 + (model ? al256(d * nx) : 0);
    return 0;
}

// The condensed exports (mpcqp_plan_vjp_batch, its model twin, mpcqp_plan_jvp_batch) once their plan `v` is made: the
// problem's checks, the export's own (args_ok), nothing more for an empty batch, else the workspace's size,
// mpcqp_condense_batch into its segments and the KKT inputs that point at them
static int condense_kkt(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, const void *lam,
                        const int32_t *status, bool args_ok, const VjpPlan &v, void *workspace, size_t workspace_bytes,
                        void *stream, CondensedKkt &k)
{
    int rc = check_problem(dims, problem);
    if (rc) return rc;
    if (!args_ok || !status || (dims->mk > 0 && !lam)) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    if (!workspace || workspace_bytes < (size_t)v.total) return MPCQP_EWORKSPACE;
    char *w = (char *)workspace;
    rc = mpcqp_condense_batch(dims, problem, batch, w + v.P, w + v.q, w + v.G, w + v.h, w + v.Phi, w + v.Psi,
                              v.cws_bytes ? w + v.cws : nullptr, v.cws_bytes, stream);
    if (rc) return rc;
    k.nx = dims->nx;
    k.nu = dims->nu;
    k.N = dims->N;
    k.mk = dims->mk;
    k.n = dims->N * dims->nu;
    k.m = dims->N * dims->mk;
    k.flags = dims->flags;
    k.wt = dims->w_terminal;
    k.wx = dims->w_stage;
    k.P = (const double *)(w + v.P);
    k.G = dims->mk > 0 ? (const double *)(w + v.G) : nullptr;
    k.Phi = (const double *)(w + v.Phi);
    k.Psi = (const double *)(w + v.Psi);
    k.C = problem->C;
    k.lam = dims->mk > 0 ? (const double *)lam : nullptr;
    k.status = status;
    k.carve_ws = v.gx0 > v.carve ? (double *)(w + v.carve) : nullptr;
    return 0;
}

// Both VJP exports: `l` carries the outputs (and, for the model export, model = true and U); the rest is filled here
static int plan_vjp(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, const void *lam,
                    const int32_t *status, const void *gU, const void *gX, AdjointLaunch &l, void *workspace,
                    size_t workspace_bytes, void *stream)
{
    VjpPlan v;
    int rc = vjp_plan(dims, batch, v, l.model);
    if (rc) return rc;
    const bool ok = gU && (l.model ? l.U != nullptr : l.out.g_x0 != nullptr);
    if ((rc = condense_kkt(dims, problem, batch, lam, status, ok, v, workspace, workspace_bytes, stream, l.kkt)) ||
        batch == 0)
        return rc;
    l.gU = (const double *)gU;
    l.gX = (const double *)gX;
    if (!l.out.g_x0) l.out.g_x0 = (char *)workspace + v.gx0;
    l.A = problem->A;
    l.x0 = problem->x0;
    l.goal = problem->goal;
    l.targets = problem->targets;
    return launch_adjoint(l, batch, (hipStream_t)stream);
}
}  // namespace

int mpcqp_plan_vjp_workspace_bytes(const MpcqpDims *dims, int64_t batch, size_t *bytes)
{
    if (!bytes) return MPCQP_EINVAL;
    VjpPlan v;
    const int rc = vjp_plan(dims, batch, v);
    if (rc) return rc;
    *bytes = (size_t)v.total;
    return 0;
}

int mpcqp_plan_vjp_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, const void *lam,
                         const int32_t *status, const void *gU, const void *gX, void *g_x0, void *g_goal, void *g_targets,
                         void *g_e, int32_t *vjp_status, void *workspace, size_t workspace_bytes, void *stream)
{
    AdjointLaunch l{};
    l.out = MpcqpVjpModelOut{g_x0, g_goal, g_targets, g_e};
    l.vjp_status = vjp_status;
    return plan_vjp(dims, problem, batch, lam, status, gU, gX, l, workspace, workspace_bytes, stream);
}

int mpcqp_plan_vjp_model_workspace_bytes(const MpcqpDims *dims, int64_t batch, size_t *bytes)
{
    if (!bytes) return MPCQP_EINVAL;
    VjpPlan v;
    const int rc = vjp_plan(dims, batch, v, true);
    if (rc) return rc;
    *bytes = (size_t)v.total;
    return 0;
}

int mpcqp_plan_vjp_model_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, const void *lam,
                               const int32_t *status, const void *U, const void *gU, const void *gX,
                               const MpcqpVjpModelOut *out, int32_t *vjp_status, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    if (!out) return MPCQP_EINVAL;
    AdjointLaunch l{};
    l.out = *out;
    l.vjp_status = vjp_status;
    l.model = true;
    l.U = (const double *)U;
    return plan_vjp(dims, problem, batch, lam, status, gU, gX, l, workspace, workspace_bytes, stream);
}

namespace {
constexpr int32_t kMaxTangents = 256;

// mpcqp_plan_jvp_batch's workspace: mpcqp_plan_vjp_batch's condensed segments, then the tangent carves when they do not
// fit LDS
// (model: the longer carve of the kModel kernel, mpcqp_plan_jvp_model_batch)
static int jvp_plan(const MpcqpDims *dims, int64_t batch, int32_t ntan, VjpPlan &v, bool model = false)
{
    const int rc = condensed_plan(dims, batch, v);
    if (rc) return rc;
    if (ntan < 1 || ntan > kMaxTangents) return MPCQP_EINVAL;
    const int n = dims->N * dims->nu;
    const bool lds = tangent_carve_in_lds(n, dims->N, dims->nx, ntan, model);
    v.gx0 = v.carve + (lds ? 0 : al256((int64_t)tangent_carve_bytes(n, dims->N, dims->nx, ntan, model) * batch));
    v.total = v.gx0;  // (no g_x0 segment)
    return 0;
}

static bool tangents_ok(const MpcqpTangents *t)
{
    return t->dx0_stride >= 0 && t->dgoal_stride >= 0 && t->dtargets_stride >= 0 && t->de_stride >= 0;
}

// what the two model exports ask of their tangents: one of the structures, a tangent in one of them, no negative stride.
// `tan` and `mtan` come back as copies (zeroed where NULL), `model` as whether mtan holds a tangent.
static bool model_tangents_ok(const MpcqpTangents *tan_in, const MpcqpModelTangents *mtan_in, MpcqpTangents &tan,
                              MpcqpModelTangents &mtan, bool &model)
{
    tan = tan_in ? *tan_in : MpcqpTangents{};
    mtan = mtan_in ? *mtan_in : MpcqpModelTangents{};
    model = mtan.dA || mtan.dB || mtan.dC || mtan.dD || mtan.dw;
    const bool any = model || tan.dx0 || tan.dgoal || tan.dtargets || tan.de;
    return any && tangents_ok(&tan) && mtan.dA_stride >= 0 && mtan.dB_stride >= 0 && mtan.dC_stride >= 0 &&
           mtan.dD_stride >= 0 && mtan.dw_stride >= 0;
}
}  // namespace

int mpcqp_plan_jvp_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t ntan, size_t *bytes)
{
    if (!bytes) return MPCQP_EINVAL;
    VjpPlan v;
    const int rc = jvp_plan(dims, batch, ntan, v);
    if (rc) return rc;
    *bytes = (size_t)v.total;
    return 0;
}

int mpcqp_plan_jvp_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t ntan,
                         const void *lam, const int32_t *status, const MpcqpTangents *tan, void *dU, void *dX,
                         int32_t *jvp_status, void *workspace, size_t workspace_bytes, void *stream)
{
    VjpPlan v;
    int rc = jvp_plan(dims, batch, ntan, v);
    if (rc) return rc;
    const bool ok = tan && dU && tan->dx0_stride >= 0 && tan->dgoal_stride >= 0 && tan->dtargets_stride >= 0 &&
                    tan->de_stride >= 0;
    TangentLaunch l{};
    if ((rc = condense_kkt(dims, problem, batch, lam, status, ok, v, workspace, workspace_bytes, stream, l.kkt)) ||
        batch == 0)
        return rc;
    l.ntan = ntan;
    l.tan = *tan;
    l.dU = (double *)dU;
    l.dX = (double *)dX;
    l.jvp_status = jvp_status;
    return launch_tangent(l, batch, (hipStream_t)stream);
}

int mpcqp_plan_jvp_model_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t ntan, size_t *bytes)
{
    if (!bytes) return MPCQP_EINVAL;
    VjpPlan v;
    const int rc = jvp_plan(dims, batch, ntan, v, true);
    if (rc) return rc;
    *bytes = (size_t)v.total;
    return 0;
}

int mpcqp_plan_jvp_model_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t ntan,
                               const void *lam, const int32_t *status, const void *U, const MpcqpTangents *tan,
                               const MpcqpModelTangents *mtan, void *dU, void *dX, int32_t *jvp_status, void *workspace,
                               size_t workspace_bytes, void *stream)
{
    VjpPlan v;
    int rc = jvp_plan(dims, batch, ntan, v, true);
    if (rc) return rc;
    TangentModelLaunch l{};
    bool model = false;
    const bool ok = model_tangents_ok(tan, mtan, l.tan, l.mtan, model) && dU && U;
    if ((rc = condense_kkt(dims, problem, batch, lam, status, ok, v, workspace, workspace_bytes, stream, l.kkt)) ||
        batch == 0)
        return rc;
    l.ntan = ntan;
    l.dU = (double *)dU;
    l.dX = (double *)dX;
    l.jvp_status = jvp_status;
    // without a model tangent: mpcqp_plan_jvp_batch's launch (its carve fits wherever the longer one does)
    if (!model) return launch_tangent(l, batch, (hipStream_t)stream);
    if (dims->mk == 0) l.mtan.dC = l.mtan.dD = nullptr;
    l.A = problem->A;
    l.x0 = problem->x0;
    l.goal = problem->goal;
    l.targets = problem->targets;
    l.U = (const double *)U;
    return launch_tangent_model(l, batch, (hipStream_t)stream);
}

namespace {
// what both shared-model derivative exports check of their dimensions, in this order, and the fields they share
static int model_diff_checks(const MpcqpDims *dims, ModelDiffLaunch &l)
{
    int rc = check_dims(dims);
    if (rc) return rc;
    if (dims->dtype != MPCQP_F64) return MPCQP_EDTYPE;
    const int64_t n = (int64_t)dims->N * dims->nu, m = (int64_t)dims->N * dims->mk;
    if (n > 64) return MPCQP_EUNSUPPORTED;
    if (!model_diff_small_applies(dims->nx, (int)n, (int)m) &&
        model_diff_general_lds_bytes(dims->nx, (int)n) > kLdsBytesPerCU)
        return MPCQP_EUNSUPPORTED;
    l.nx = dims->nx;
    l.nu = dims->nu;
    l.N = dims->N;
    l.mk = dims->mk;
    l.n = (int)n;
    l.m = (int)m;
    l.flags = dims->flags;
    return 0;
}

static bool strides_ok(const MpcqpOperand *A, const MpcqpOperand *B)
{
    return A->batch_stride >= 0 && A->step_stride >= 0 && B->batch_stride >= 0 && B->step_stride >= 0;
}

// the kernel by the model's size: sixteen lanes per problem where the model has the small-problem kernels' 16 columns
static int launch_model_diff(const ModelDiffLaunch &l, void *stream)
{
    if (model_diff_small_applies(l.nx, l.n, l.m)) return launch_model_diff_small(l, (hipStream_t)stream);
    return launch_model_diff_general(l, (hipStream_t)stream);
}
}  // namespace

int mpcqp_model_vjp_batch(const MpcqpDims *dims, const void *model, int64_t batch, const void *lam,
                          const int32_t *status, const void *gU, const void *gX, const MpcqpOperand *A,
                          const MpcqpOperand *B, void *g_x0, void *g_goal, void *g_targets, void *g_e,
                          int32_t *vjp_status, void *stream)
{
    ModelDiffLaunch l{};
    int rc = model_diff_checks(dims, l);
    if (rc) return rc;
    if (!model || !status || !gU || !g_x0 || batch < 0 || (dims->mk > 0 && !lam)) return MPCQP_EINVAL;
    if (gX && (!A || !B || !A->ptr || !B->ptr || !strides_ok(A, B))) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    l.batch = batch;
    l.model = (const double *)model;
    l.lam = dims->mk > 0 ? (const double *)lam : nullptr;
    l.status = status;
    l.gU = (const double *)gU;
    l.gX = (const double *)gX;
    if (gX) {
        l.A = *A;
        l.B = *B;
    }
    l.g_x0 = (double *)g_x0;
    l.g_goal = (double *)g_goal;
    l.g_targets = (double *)g_targets;
    l.g_e = dims->mk > 0 ? (double *)g_e : nullptr;
    l.out_status = vjp_status;
    return launch_model_diff(l, stream);
}

int mpcqp_model_jvp_batch(const MpcqpDims *dims, const void *model, int64_t batch, int32_t ntan, const void *lam,
                          const int32_t *status, const MpcqpTangents *tan, const MpcqpOperand *A,
                          const MpcqpOperand *B, void *dU, void *dX, int32_t *jvp_status, void *stream)
{
    ModelDiffLaunch l{};
    int rc = model_diff_checks(dims, l);
    if (rc) return rc;
    if (!model || !status || !dU || !tan || batch < 0 || (dims->mk > 0 && !lam)) return MPCQP_EINVAL;
    if (dX && (!A || !B || !A->ptr || !B->ptr || !strides_ok(A, B))) return MPCQP_EINVAL;
    if (!tangents_ok(tan) || ntan < 1 || ntan > kMaxTangents) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    l.batch = batch;
    l.ntan = ntan;
    l.model = (const double *)model;
    l.lam = dims->mk > 0 ? (const double *)lam : nullptr;
    l.status = status;
    l.tan = *tan;
    if (dims->mk == 0) l.tan.de = nullptr;
    if (dX) {
        l.A = *A;
        l.B = *B;
    }
    l.dU = (double *)dU;
    l.dX = (double *)dX;
    l.out_status = jvp_status;
    return launch_model_diff(l, stream);
}

namespace {
// what both stage-wise plan-derivative exports check of their dimensions, in this order
static int stagewise_checks(const MpcqpDims *dims, int64_t batch, int32_t max_active)
{
    const int rc = check_dims(dims);
    if (rc) return rc;
    if (batch < 0 || max_active < 0) return MPCQP_EINVAL;
    if (dims->dtype != MPCQP_F64) return MPCQP_EDTYPE;
    if (!stagewise_adjoint_applies(dims->nx, dims->nu)) return MPCQP_EUNSUPPORTED;
    return 0;
}

// mpcqp_plan_vjp_stagewise_batch's workspace: one region per problem (mpcqp_adjoint_stagewise.hip's carve, phase 6 included)
static int vjp_stagewise_plan(const MpcqpDims *dims, int64_t batch, int32_t max_active, size_t &total)
{
    const int rc = stagewise_checks(dims, batch, max_active);
    if (rc) return rc;
    total = (size_t)al256((int64_t)stagewise_adjoint_bytes(dims->nx, dims->nu, dims->N, dims->mk, max_active) * batch);
    return 0;
}
}  // namespace

int mpcqp_plan_vjp_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active, size_t *bytes)
{
    if (!bytes) return MPCQP_EINVAL;
    size_t total = 0;
    const int rc = vjp_stagewise_plan(dims, batch, max_active, total);
    if (rc) return rc;
    *bytes = total;
    return 0;
}

int mpcqp_plan_vjp_stagewise_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t max_active,
                                   const void *lam, const int32_t *status, const void *U, const void *gU, const void *gX,
                                   const MpcqpVjpModelOut *out, int32_t *vjp_status, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    size_t total = 0;
    int rc = vjp_stagewise_plan(dims, batch, max_active, total);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    if (!out || !status || !gU || (dims->mk > 0 && !lam)) return MPCQP_EINVAL;
    const bool model = out->g_A || out->g_B || out->g_C || out->g_D || out->g_w;
    if (model && !U) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    if (!workspace || workspace_bytes < total) return MPCQP_EWORKSPACE;
    StagewiseAdjointLaunch l{};
    l.nx = dims->nx;
    l.nu = dims->nu;
    l.N = dims->N;
    l.mk = dims->mk;
    l.n = dims->N * dims->nu;
    l.m = dims->N * dims->mk;
    l.flags = dims->flags;
    l.ka = max_active > 0 ? max_active : 1;
    l.wt = dims->w_terminal;
    l.wx = dims->w_stage;
    l.wu = dims->w_input;
    l.problem = *problem;
    l.lam = (const double *)lam;
    l.gU = (const double *)gU;
    l.gX = (const double *)gX;
    l.U = (const double *)U;
    l.status = status;
    l.out = *out;
    l.model = model;
    l.vjp_status = vjp_status;
    l.workspace = (double *)workspace;
    return launch_adjoint_stagewise(l, batch, (hipStream_t)stream);
}

namespace {
// mpcqp_plan_jvp_stagewise_batch's workspace: one region per problem (mpcqp_adjoint_stagewise.hip's tangent carve)
// (model: the longer region of the kModel kernel, mpcqp_plan_jvp_model_stagewise_batch)
static int jvp_stagewise_plan(const MpcqpDims *dims, int64_t batch, int32_t max_active, int32_t ntan, size_t &total,
                              bool model = false)
{
    const int rc = stagewise_checks(dims, batch, max_active);
    if (rc) return rc;
    if (ntan < 1 || ntan > kMaxTangents) return MPCQP_EINVAL;
    total = (size_t)al256((int64_t)stagewise_tangent_bytes(dims->nx, dims->nu, dims->N, max_active, ntan, model) * batch);
    return 0;
}

// the fields of a stage-wise tangent launch that both exports fill alike
static void fill_stagewise_tangent(StagewiseTangentLaunch &l, const MpcqpDims *dims, const MpcqpProblem *problem,
                                   int32_t max_active, int32_t ntan, const void *lam, const int32_t *status, void *dU,
                                   void *dX, int32_t *jvp_status, void *workspace)
{
    l.nx = dims->nx;
    l.nu = dims->nu;
    l.N = dims->N;
    l.mk = dims->mk;
    l.n = dims->N * dims->nu;
    l.m = dims->N * dims->mk;
    l.flags = dims->flags;
    l.ka = max_active > 0 ? max_active : 1;
    l.ntan = ntan;
    l.wt = dims->w_terminal;
    l.wx = dims->w_stage;
    l.wu = dims->w_input;
    l.problem = *problem;
    l.lam = dims->mk > 0 ? (const double *)lam : nullptr;
    l.status = status;
    if (dims->mk == 0) l.tan.de = nullptr;
    l.dU = (double *)dU;
    l.dX = (double *)dX;
    l.jvp_status = jvp_status;
    l.workspace = (double *)workspace;
}
}  // namespace

int mpcqp_plan_jvp_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active, int32_t ntan,
                                             size_t *bytes)
{
    if (!bytes) return MPCQP_EINVAL;
    size_t total = 0;
    const int rc = jvp_stagewise_plan(dims, batch, max_active, ntan, total);
    if (rc) return rc;
    *bytes = total;
    return 0;
}

int mpcqp_plan_jvp_stagewise_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, int32_t max_active,
                                   int32_t ntan, const void *lam, const int32_t *status, const MpcqpTangents *tan,
                                   void *dU, void *dX, int32_t *jvp_status, void *workspace, size_t workspace_bytes,
                                   void *stream)
{
    size_t total = 0;
    int rc = jvp_stagewise_plan(dims, batch, max_active, ntan, total);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    if (!tan || !status || !dU || (dims->mk > 0 && !lam) || tan->dx0_stride < 0 || tan->dgoal_stride < 0 ||
        tan->dtargets_stride < 0 || tan->de_stride < 0)
        return MPCQP_EINVAL;
    if (batch == 0) return 0;
    if (!workspace || workspace_bytes < total) return MPCQP_EWORKSPACE;
    StagewiseTangentLaunch l{};
    l.tan = *tan;
    fill_stagewise_tangent(l, dims, problem, max_active, ntan, lam, status, dU, dX, jvp_status, workspace);
    return launch_tangent_stagewise(l, batch, (hipStream_t)stream);
}

int mpcqp_plan_jvp_model_stagewise_workspace_bytes(const MpcqpDims *dims, int64_t batch, int32_t max_active,
                                                   int32_t ntan, size_t *bytes)
{
    if (!bytes) return MPCQP_EINVAL;
    size_t total = 0;
    const int rc = jvp_stagewise_plan(dims, batch, max_active, ntan, total, true);
    if (rc) return rc;
    *bytes = total;
    return 0;
}

int mpcqp_plan_jvp_model_stagewise_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch,
                                         int32_t max_active, int32_t ntan, const void *lam, const int32_t *status,
                                         const void *U, const MpcqpTangents *tan, const MpcqpModelTangents *mtan,
                                         void *dU, void *dX, int32_t *jvp_status, void *workspace,
                                         size_t workspace_bytes, void *stream)
{
    size_t total = 0;
    int rc = jvp_stagewise_plan(dims, batch, max_active, ntan, total, true);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    StagewiseTangentModelLaunch l{};
    bool model = false;
    if (!model_tangents_ok(tan, mtan, l.tan, l.mtan, model) || !status || !dU || !U || (dims->mk > 0 && !lam))
        return MPCQP_EINVAL;
    if (batch == 0) return 0;
    if (!workspace || workspace_bytes < total) return MPCQP_EWORKSPACE;
    fill_stagewise_tangent(l, dims, problem, max_active, ntan, lam, status, dU, dX, jvp_status, workspace);
    // without a model tangent: mpcqp_plan_jvp_stagewise_batch's launch (its regions fit in the longer ones)
    if (!model) return launch_tangent_stagewise(l, batch, (hipStream_t)stream);
    if (dims->mk == 0) l.mtan.dC = l.mtan.dD = nullptr;
    l.U = (const double *)U;
    return launch_tangent_model_stagewise(l, batch, (hipStream_t)stream);
}

int mpcqp_wip_period_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, const MpcqpSolveOpts *opts,
                           void *U, void *lam, int32_t *status, int32_t *iters, void *workspace, size_t workspace_bytes,
                           void *states, int64_t *loop_stats, double sampling_period, double target_vel, double length,
                           double gravity, int32_t nsub, void *stream)
{
    return mpcqp_wip_periods_batch(dims, problem, batch, opts, U, lam, status, iters, workspace, workspace_bytes, states,
                                   loop_stats, sampling_period, target_vel, length, gravity, nsub, 1, stream);
}

int mpcqp_wip_periods_batch(const MpcqpDims *dims, const MpcqpProblem *problem, int64_t batch, const MpcqpSolveOpts *opts,
                            void *U, void *lam, int32_t *status, int32_t *iters, void *workspace, size_t workspace_bytes,
                            void *states, int64_t *loop_stats, double sampling_period, double target_vel, double length,
                            double gravity, int32_t nsub, int32_t nperiods, void *stream)
{
    if (nperiods < 1) return MPCQP_EINVAL;
    int rc = check_dims(dims);
    if (rc) return rc;
    if ((rc = check_problem(dims, problem))) return rc;
    if (batch < 0 || !U || !states || nsub <= 0 || !(length > 0) || !(gravity > 0)) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    KernelArgs ka;
    fill_args(ka, dims, problem);
    ka.U = U;
    ka.lam = lam;
    ka.status = status;
    ka.iters = iters;
    const Entry entry{Entry::WIP_PERIODS};
    if ((rc = fill_opts(ka, opts, dims->dtype)) || (rc = refusal(ka, dims->dtype, entry))) return rc;
    // the plant is the 4-state, 1-input pendulum, every loop with its own x0, goal and targets; only the stage-wise
    // kernel carries the epilogue
    const Route r = route(ka, dims->dtype, batch, entry, SimdCount{});
    if (ka.nx != 4 || ka.nu != 1 || !problem->x0.ptr || !problem->goal.ptr || !problem->targets.ptr ||
        problem->x0.batch_stride != 4 || problem->goal.batch_stride != 4 || problem->targets.batch_stride != (int64_t)ka.N * 4 ||
        r.path == Path::Refused)
        return MPCQP_EUNSUPPORTED;
    if (!workspace || workspace_bytes < r.bytes) return MPCQP_EWORKSPACE;
    // (as in mpcqp_build_solve_batch: the warm-state record is indexed by problem and written by the kernel, so a buffer
    // that is too small -- or an old caller that leaves warm_state_bytes at zero -- is refused before anything is launched)
    if (ka.warm_state && ka.warm_state_bytes < (size_t)batch * warm_bytes_per_problem(ka, dims->dtype)) return MPCQP_EWORKSPACE;
    // several periods per launch: a factor that is kept is the FIRST period's business (the caller's next launch reuses
    // or pipelines it), and the warm-state record is per launch
    if (nperiods > 1 && ((ka.opt_flags & MPCQP_OPT_KEEP_FACTOR) || ka.warm_state || !stage_pipeline_supported(ka, dims->dtype)))
        return MPCQP_EUNSUPPORTED;  // (... and the period loop is compiled into the short-horizon instantiations only)
    ka.ep_on = 1;
    ka.ep_periods = nperiods;
    ka.ep_nsub = nsub;
    ka.ep_Tp = sampling_period;
    ka.ep_vel = target_vel;
    ka.ep_omega2 = gravity / length;
    ka.ep_g = gravity;
    ka.ep_states = states;
    ka.ep_loopstats = (long long *)loop_stats;
    return run_narrow(ka, dims->dtype, r, batch, workspace, (hipStream_t)stream);
}

int mpcqp_model_periods_batch(const MpcqpDims *dims, const void *model, const MpcqpLoopPlant *plant, void *states,
                              const MpcqpOperand *goal, const MpcqpOperand *targets, int64_t batch, int32_t nperiods, int32_t warm,
                              const MpcqpSolveOpts *opts, void *U, void *lam, int32_t *status, int32_t *iters,
                              const MpcqpLoopOut *out, void *stream)
{
    if (nperiods < 1) return MPCQP_EINVAL;
    int rc = check_dims(dims);
    if (rc) return rc;
    if (!model || !plant || !plant->A.ptr || !plant->B.ptr || !states || !U || !status || batch < 0) return MPCQP_EINVAL;
    if ((dims->flags & MPCQP_Q_TERMINAL) && !(goal && goal->ptr)) return MPCQP_EINVAL;
    if ((dims->flags & MPCQP_Q_STAGE) && !(targets && targets->ptr)) return MPCQP_EINVAL;
    KernelArgs ka;
    fill_args(ka, dims, nullptr);
    if (goal) ka.goal = *goal;
    if (targets) ka.targets = *targets;
    ka.model = model;
    ka.U = U;
    ka.lam = lam;
    ka.status = status;
    ka.iters = iters;
    const Entry entry{Entry::MODEL_PERIODS};
    if ((rc = fill_opts(ka, opts, dims->dtype)) || (rc = refusal(ka, dims->dtype, entry))) return rc;
    ka.probe = nullptr;
    const Route r = route(ka, dims->dtype, batch, entry, SimdCount{});
    if (r.path == Path::Refused) return r.rc;
    if (batch == 0) return 0;
    LoopArgs lp{};
    lp.A = plant->A;
    lp.B = plant->B;
    lp.d = plant->d;
    lp.states = states;
    if (out) {
        lp.X = out->X;
        lp.U0 = out->U0;
        lp.stats = (long long *)out->loop_stats;
    }
    lp.nperiods = nperiods;
    lp.warm = warm != 0;
    return run(r, ka, false, false, dims->dtype, batch, nullptr, (hipStream_t)stream, &lp);
}

int mpcqp_model_periods_vjp_batch(const MpcqpDims *dims, const void *model, const MpcqpLoopPlant *plant, int64_t batch,
                                  int32_t nperiods, const void *lam, const int32_t *status, const void *X, const void *U0,
                                  const void *gX, const void *gU0, void *g_x0, void *g_states,
                                  const MpcqpPeriodGrad *g_goal, const MpcqpPeriodGrad *g_targets, void *g_A, void *g_B,
                                  int32_t *vjp_status, void *stream)
{
    const int rc = check_dims(dims);
    if (rc) return rc;
    if (dims->dtype != MPCQP_F64) return MPCQP_EDTYPE;
    const int64_t n = (int64_t)dims->N * dims->nu, m = (int64_t)dims->N * dims->mk;
    if (n > 16 || m < 1 || m > 32 || dims->nx > 16) return MPCQP_EUNSUPPORTED;  // mpcqp_model_periods_batch's envelope
    if (!model || !plant || !plant->A.ptr || !plant->B.ptr || !lam || !status || !g_x0 || nperiods < 1 || batch < 0)
        return MPCQP_EINVAL;
    if (plant->A.batch_stride < 0 || plant->B.batch_stride < 0) return MPCQP_EINVAL;
    for (const MpcqpPeriodGrad *g : {g_goal, g_targets})
        if (g && (g->batch_stride < 0 || g->period_stride < 0)) return MPCQP_EINVAL;
    if ((g_A && !X) || (g_B && !U0)) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    LoopAdjointLaunch l{};
    l.nx = dims->nx;
    l.nu = dims->nu;
    l.N = dims->N;
    l.n = (int)n;
    l.m = (int)m;
    l.flags = dims->flags;
    l.nperiods = nperiods;
    l.batch = batch;
    l.model = (const double *)model;
    l.A = plant->A;
    l.B = plant->B;
    l.lam = (const double *)lam;
    l.status = status;
    l.X = (const double *)X;
    l.U0 = (const double *)U0;
    l.gX = (const double *)gX;
    l.gU0 = (const double *)gU0;
    l.g_x0 = (double *)g_x0;
    l.g_states = (double *)g_states;
    if (g_goal) l.g_goal = *g_goal;
    if (g_targets) l.g_targets = *g_targets;
    l.g_A = (double *)g_A;
    l.g_B = (double *)g_B;
    l.out_status = vjp_status;
    return launch_loop_adjoint_small(l, (hipStream_t)stream);
}

int mpcqp_model_periods_jvp_batch(const MpcqpDims *dims, const void *model, const MpcqpLoopPlant *plant, int64_t batch,
                                  int32_t nperiods, int32_t ntan, const void *lam, const int32_t *status, const void *X,
                                  const void *U0, const MpcqpLoopTangents *tan, void *dX, void *dU0, int32_t *jvp_status,
                                  void *stream)
{
    const int rc = check_dims(dims);
    if (rc) return rc;
    if (dims->dtype != MPCQP_F64) return MPCQP_EDTYPE;
    const int64_t n = (int64_t)dims->N * dims->nu, m = (int64_t)dims->N * dims->mk;
    if (n > 16 || m < 1 || m > 32 || dims->nx > 16) return MPCQP_EUNSUPPORTED;  // mpcqp_model_periods_vjp_batch's envelope
    if (!model || !plant || !plant->A.ptr || !plant->B.ptr || !lam || !status || !tan || !dX || nperiods < 1 || batch < 0 ||
        ntan < 1 || ntan > 256)
        return MPCQP_EINVAL;
    if (plant->A.batch_stride < 0 || plant->B.batch_stride < 0) return MPCQP_EINVAL;
    if (tan->dx0_stride < 0 || tan->dA_stride < 0 || tan->dB_stride < 0) return MPCQP_EINVAL;
    for (const MpcqpPeriodTangent *p : {&tan->dgoal, &tan->dtargets, &tan->dd})
        if (p->batch_stride < 0 || p->tangent_stride < 0 || p->period_stride < 0) return MPCQP_EINVAL;
    if ((tan->dA && !X) || (tan->dB && !U0)) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    LoopTangentLaunch l{};
    l.nx = dims->nx;
    l.nu = dims->nu;
    l.N = dims->N;
    l.n = (int)n;
    l.m = (int)m;
    l.flags = dims->flags;
    l.nperiods = nperiods;
    l.ntan = ntan;
    l.batch = batch;
    l.model = (const double *)model;
    l.A = plant->A;
    l.B = plant->B;
    l.lam = (const double *)lam;
    l.status = status;
    l.X = (const double *)X;
    l.U0 = (const double *)U0;
    l.tan = *tan;
    l.dX = (double *)dX;
    l.dU0 = (double *)dU0;
    l.out_status = jvp_status;
    return launch_loop_tangent_small(l, (hipStream_t)stream);
}

int mpcqp_wip_advance_stats_batch(int32_t dtype, void *states, const void *U, int64_t u_stride, const int32_t *status,
                                  const int32_t *iters, int64_t *stats, int32_t N, double sampling_period,
                                  double target_vel, double length, double gravity, int32_t nsub, void *x0, void *goal,
                                  void *targets, int64_t batch, void *stream)
{
    if (dtype != MPCQP_F64 && dtype != MPCQP_F32) return MPCQP_EDTYPE;
    if (!states || !U || !x0 || !goal || !targets || N <= 0 || nsub < 0 || batch < 0 || !(length > 0) || !(gravity > 0))
        return MPCQP_EINVAL;
    if (stats && !status) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    return launch_wip_advance(dtype, states, U, u_stride, status, iters, stats, N, sampling_period, target_vel, length,
                              gravity, nsub, x0, goal, targets, batch, (hipStream_t)stream);
}

int mpcqp_wip_advance_batch(int32_t dtype, void *states, const void *U, int64_t u_stride, const int32_t *status,
                            int32_t N, double sampling_period, double target_vel, double length, double gravity,
                            int32_t nsub, void *x0, void *goal, void *targets, int64_t batch, void *stream)
{
    return mpcqp_wip_advance_stats_batch(dtype, states, U, u_stride, status, nullptr, nullptr, N, sampling_period,
                                         target_vel, length, gravity, nsub, x0, goal, targets, batch, stream);
}

int mpcqp_accumulate_stats(const int32_t *status, const int32_t *iters, int64_t batch, int64_t *stats, void *stream)
{
    if (!status || !iters || !stats || batch < 0) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    return launch_stats(status, iters, batch, stats, (hipStream_t)stream);
}

// ---- mpcqp_order_by_count: a counting sort of the batch by (clamped) count, longest first. Three small launches: per-chunk
// histograms, one workgroup that turns them into start offsets (bucket-major, chunk-minor), the scatter. Inside one (bucket, chunk)
// cell the places are handed out by an LDS atomic, so the order of equal counts within a chunk is not reproducible -- it is a
// pairing hint, every order is a valid one.
namespace {
constexpr int kOrdBuckets = 1024, kOrdChunk = 4096, kOrdThreads = 256;
__device__ __forceinline__ int ord_bucket(int c) { return kOrdBuckets - 1 - (c < 0 ? 0 : (c > kOrdBuckets - 1 ? kOrdBuckets - 1 : c)); }

__global__ void __launch_bounds__(kOrdThreads) order_hist_kernel(const int32_t *__restrict__ counts, int64_t batch, int32_t *__restrict__ hist, int chunks)
{
    __shared__ int h[kOrdBuckets];
    for (int b = threadIdx.x; b < kOrdBuckets; b += kOrdThreads) h[b] = 0;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * kOrdChunk;
    for (int i = threadIdx.x; i < kOrdChunk && first + i < batch; i += kOrdThreads) atomicAdd(&h[ord_bucket(counts[first + i])], 1);
    __syncthreads();
    for (int b = threadIdx.x; b < kOrdBuckets; b += kOrdThreads) hist[(int64_t)blockIdx.x * kOrdBuckets + b] = h[b];
}

__global__ void __launch_bounds__(kOrdBuckets) order_scan_kernel(int32_t *__restrict__ hist, int chunks)
{
    __shared__ int tot[kOrdBuckets];
    const int b = threadIdx.x;
    int sum = 0;
#pragma unroll 8
    for (int g = 0; g < chunks; ++g) sum += hist[(int64_t)g * kOrdBuckets + b];  // (independent, coalesced loads)
    tot[b] = sum;
    __syncthreads();
    for (int d = 1; d < kOrdBuckets; d <<= 1) {  // inclusive scan over the buckets
        const int v = b >= d ? tot[b - d] : 0;
        __syncthreads();
        tot[b] += v;
        __syncthreads();
    }
    int run = tot[b] - sum;
#pragma unroll 8
    for (int g = 0; g < chunks; ++g) {
        const int c = hist[(int64_t)g * kOrdBuckets + b];
        hist[(int64_t)g * kOrdBuckets + b] = run;
        run += c;
    }
}

__global__ void __launch_bounds__(kOrdThreads) order_scatter_kernel(const int32_t *__restrict__ counts, int64_t batch, const int32_t *__restrict__ hist,
                                                                     int chunks, int32_t *__restrict__ order)
{
    __shared__ int off[kOrdBuckets];
    for (int b = threadIdx.x; b < kOrdBuckets; b += kOrdThreads) off[b] = hist[(int64_t)blockIdx.x * kOrdBuckets + b];
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * kOrdChunk;
    for (int i = threadIdx.x; i < kOrdChunk && first + i < batch; i += kOrdThreads) {
        const int at = atomicAdd(&off[ord_bucket(counts[first + i])], 1);
        order[at] = (int32_t)(first + i);
    }
}
}  // namespace

size_t mpcqp_order_workspace_bytes(int64_t batch)
{
    return batch <= 0 ? 0 : (size_t)kOrdBuckets * sizeof(int32_t) * (size_t)((batch + kOrdChunk - 1) / kOrdChunk);
}

int mpcqp_order_by_count(const int32_t *counts, int64_t batch, int32_t *order, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!counts || !order || batch < 0 || batch > INT32_MAX) return MPCQP_EINVAL;
    if (batch == 0) return 0;
    if (!workspace || workspace_bytes < mpcqp_order_workspace_bytes(batch)) return MPCQP_EWORKSPACE;
    const int chunks = (int)((batch + kOrdChunk - 1) / kOrdChunk);
    hipStream_t st = (hipStream_t)stream;
    int32_t *hist = (int32_t *)workspace;
    hipLaunchKernelGGL(order_hist_kernel, dim3(chunks), dim3(kOrdThreads), 0, st, counts, batch, hist, chunks);
    hipLaunchKernelGGL(order_scan_kernel, dim3(1), dim3(kOrdBuckets), 0, st, hist, chunks);
    hipLaunchKernelGGL(order_scatter_kernel, dim3(chunks), dim3(kOrdThreads), 0, st, counts, batch, hist, chunks, order);
    return (int)hipGetLastError();
}

int mpcqp_lipm_advance_stats_batch(int32_t dtype, void *states, const void *U, int64_t u_stride, const int32_t *status,
                                   const int32_t *iters, int64_t *stats, int32_t N, double sampling_period, int32_t nsub,
                                   int32_t nb_dsp, int32_t nb_ssp, double max_zmp_dist, int64_t *index,
                                   int64_t *stride_index, void *support, const void *strides, const void *foot_size,
                                   void *x0, void *goal, void *e, int64_t batch, void *stream)
{
    if (dtype != MPCQP_F64 && dtype != MPCQP_F32) return MPCQP_EDTYPE;
    if (!states || !index || !stride_index || !support || !strides || !foot_size || !x0 || !goal || !e || N <= 0 ||
        nsub <= 0 || nb_dsp < 0 || nb_ssp < 0 || batch < 0)
        return MPCQP_EINVAL;
    if (stats && !status) return MPCQP_EINVAL;
    if (2 * (nb_dsp + nb_ssp) < N) return MPCQP_EINVAL;  // more than two steps in the receding horizon
    if (batch == 0) return 0;
    return launch_lipm_advance(dtype, states, U, u_stride, status, N, sampling_period, nsub, nb_dsp, nb_ssp,
                               max_zmp_dist, index, stride_index, support, strides, foot_size, x0, goal, e, batch,
                               iters, stats, (hipStream_t)stream);
}

int mpcqp_lipm_advance_batch(int32_t dtype, void *states, const void *U, int64_t u_stride, const int32_t *status,
                             int32_t N, double sampling_period, int32_t nsub, int32_t nb_dsp, int32_t nb_ssp,
                             double max_zmp_dist, int64_t *index, int64_t *stride_index, void *support,
                             const void *strides, const void *foot_size, void *x0, void *goal, void *e,
                             int64_t batch, void *stream)
{
    return mpcqp_lipm_advance_stats_batch(dtype, states, U, u_stride, status, nullptr, nullptr, N, sampling_period, nsub,
                                          nb_dsp, nb_ssp, max_zmp_dist, index, stride_index, support, strides,
                                          foot_size, x0, goal, e, batch, stream);
}

}  // extern "C"
