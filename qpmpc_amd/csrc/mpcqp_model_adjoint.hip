// mpcqp_model_adjoint.hip -- derivatives of plans of a factored shared model: mpcqp_model_vjp_batch and
// mpcqp_model_jvp_batch (include/mpcqp.h; DESIGN.md section 9, "Shared-model derivatives").
//
// The model of mpcqp_factor_model holds M = G L^-T, L^-T and the maps d = L^-1 q = Wx x0 - Wg goal - Wt targets,
// h = e - Hx x0. In whitened coordinates (U = L^-T u~) the KKT system of a plan on its active set A = {i : lam_i > 0} is
//     [I M_A'; M_A 0] [u~; lam_A] = [-d; h_A],     S = M_A M_A'  (k x k, k <= n),
// so both derivatives are one Cholesky factorisation of S and products with rows of the shared matrices: nothing is
// condensed, P is not factored again and there is no workspace.
//   VJP:  t = L^-1 (gU + Psi' gX),  nu = S^-1 M_A t,  w~ = t - M_A' nu,
//         g_x0 = -Wx' w~ - Hx' nu + p_0,  g_goal = Wg' w~,  g_targets = Wt' w~,  g_e = nu scattered over the rows
//         (p: the costate p_N = gX_N, p_k = gX_k + A_k' p_{k+1}; (Psi' gX)_k = B_k' p_{k+1})
//   JVP:  r = -(Wx dx0 - Wg dgoal - Wt dtargets),  mu = S^-1 (M_A r - dh_A),  dh = de - Hx dx0,
//         dU = L^-T (r - M_A' mu),  dX = rollout(dx0, dU)
// Two kernels, one template each with the direction as a flag:
//   mpcqp_model_diff_small_kernel    n <= 16, m <= 32, nx <= 16 (the model's 16 padded columns): sixteen lanes per problem,
//                                    four problems per wavefront, the shared matrices staged once per workgroup in LDS,
//                                    workgroups striding over the batch;
//   mpcqp_model_diff_general_kernel  every other model up to n = 64: one workgroup per problem, S and the vectors in LDS,
//                                    the rows of M read in place from the model.
// and the adjoint of closed loops of such a model, mpcqp_model_periods_vjp_batch:
//   mpcqp_loop_adjoint_small_kernel  the small kernel's envelope and layout, sixteen lanes per LOOP; the reverse-time
//                                    recursion over the periods inside, each period the VJP above with gU = [ubar; 0]
//                                    ("Closed-loop adjoint").
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mpcqp.h"
#include "mpcqp_internal.h"
#include "mpcqp_lane.h"
#include "mpcqp_adjoint_common.h"
#include "mpcqp_model_small.h"

namespace mpcqp {

namespace {

__device__ inline const double *tangent_of(const void *p, int64_t stride, int64_t b, int t, int64_t len)
{
    return p ? (const double *)p + b * stride + (int64_t)t * len : nullptr;
}

// ------------------------------------------------------------------------------------------------ small models
// (the LDS image, the workgroup shape, SmallKkt and the grid: mpcqp_model_small.h)
// Sixteen lanes per problem: lane l of a row is variable l (t, w~, r, dU), active slot l (its row of S, nu, mu), state
// component l (costate, rollout, the nx-wide outputs) and inequality rows l and l + 16. A problem that is not solved, or
// a row past the end of the batch, takes every wavefront-wide step with zeros: there is no return before the last one.
template <bool kJvp>
__global__ void __launch_bounds__(kSmallThreads) mpcqp_model_diff_small_kernel(const ModelDiffLaunch a)
{
    extern __shared__ double lds_image[];
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, nT = N * nx, R = (N + 1) * nx;
    const ModelLayout ml = make_model_layout(nx, N, n, m);
    const SmallImage im = make_small_image(nx, N, m);
    {
        const int tid = threadIdx.x;
        for (int i = tid; i < m * 16; i += kSmallThreads) lds_image[im.M + i] = a.model[ml.off_M + i];
        for (int i = tid; i < 256; i += kSmallThreads) lds_image[im.Lt + i] = a.model[ml.off_LinvT + i];
        for (int i = tid; i < 16 * nx; i += kSmallThreads) {
            lds_image[im.Wx + i] = a.model[ml.off_Wx + i];
            lds_image[im.Wg + i] = a.model[ml.off_Wg + i];
        }
        for (int i = tid; i < 16 * nT; i += kSmallThreads) lds_image[im.Wt + i] = a.model[ml.off_Wt + i];
        for (int i = tid; i < m * nx; i += kSmallThreads) lds_image[im.Hx + i] = a.model[ml.off_Hx + i];
    }
    const bool model_bad = a.model[ml.total] != 0.0;
    __syncthreads();
    const double *Mm = lds_image + im.M, *Lt = lds_image + im.Lt, *Wx = lds_image + im.Wx, *Wg = lds_image + im.Wg;
    const double *Wt = lds_image + im.Wt, *Hx = lds_image + im.Hx;
    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
    const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15;
    const int slot = (threadIdx.x >> 6) * 4 + g;  // this row's problem within the round

    for (int64_t base = (int64_t)blockIdx.x * kSmallPerBlock; base < a.batch; base += (int64_t)gridDim.x * kSmallPerBlock) {
        const int64_t b = base + slot;
        const bool valid = b < a.batch;
        int verdict = valid ? (model_bad ? MPCQP_NOT_PD : a.status[b]) : -1;
        const bool live = verdict == 0;
        // active rows: ids ascending, slot i takes the i-th set bit
        const double *lam = a.lam ? a.lam + b * (int64_t)m : nullptr;
        const bool a0 = live && l < m && lam[l] > 0.0, a1 = live && l + 16 < m && lam[l + 16] > 0.0;
        const unsigned long long m0 = __ballot(a0), m1 = __ballot(a1);
        const unsigned act = (unsigned)((m0 >> (16 * g)) & 0xffffull) | ((unsigned)((m1 >> (16 * g)) & 0xffffull) << 16);
        int k = __popc(act);
        if (live && k > n) verdict = MPCQP_NOT_PD;  // more active rows than variables: not a vertex's multipliers
        const bool run = verdict == 0;
        if (!run) k = 0;
        int id = 0;  // this slot's row (0 past the k-th: its products are masked)
        {
            unsigned x = act;
            for (int s = 0; s < 15; ++s)
                if (s < l) x &= x - 1;
            if (l < k) id = __builtin_ctz(x);
        }
        const int kmax = max(max(lane_get(k, 0), lane_get(k, 16)), max(lane_get(k, 32), lane_get(k, 48)));
        // this slot's row of M_A
        double ma[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) ma[c] = l < k ? Mm[id * 16 + c] : 0.0;
        // S = M_A M_A', row `l` on this lane
        double S[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            S[c] = 0.0;
            if (c < kmax) {
                const int idc = __shfl(id, c, 16);
                const double *mc = Mm + idc * 16;
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 16; ++j) acc += ma[j] * mc[j];
                S[c] = (c < k) ? acc : 0.0;
            }
        }
        // in-place lower Cholesky, the pivot test of chol_lower<BS, true> (mpcqp_adjoint_common.h): lane j holds pivot j and
        // passes it on only where it exceeds the floor times its row's squared norm, the diagonal before elimination
        bool bad = false;
        double dinv = 0.0, dg = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) dg += ma[c] * ma[c];
        dg *= gram_pivot_floor(16, 16);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < kmax) {
                const double d = __shfl(S[j] > dg ? S[j] : 0.0, j, 16);
                const bool in = j < k;
                if (in && !(d > 0.0)) bad = true;
                const bool ok = in && !bad;
                const double sd = ok ? sqrt(d) : 1.0, inv = ok ? 1.0 / sd : 0.0;
                if (l == j) dinv = inv;
                const double lij = (l == j) ? sd : S[j] * inv;
                S[j] = lij;
#pragma unroll
                for (int c = j + 1; c < 16; ++c) {
                    if (c < kmax) {
                        const double lcj = __shfl(lij, c, 16);
                        S[c] -= lij * lcj;
                    }
                }
            }
        }
        if (run && bad) verdict = MPCQP_NOT_PD;
        const bool good = verdict == 0;
        // x <- S^-1 x for the slot-distributed x
        auto solve = [&](double x) {
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j < kmax) {
                    if (l == j) x *= dinv;
                    const double xj = __shfl(x, j, 16);
                    if (l > j) x -= S[j] * xj;
                }
            }
#pragma unroll
            for (int j = 15; j >= 0; --j) {
                if (j < kmax) {
                    const double s = row_sum_dpp((l > j && l < k) ? S[j] * x : 0.0);
                    if (l == j) x = (x - s) * dinv;
                }
            }
            return (l < k) ? x : 0.0;
        };
        // y_l = sum_i M[id_i][l] x_i for the slot-distributed x
        auto rows_t = [&](double x) {
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (i < kmax) {
                    const int idi = __shfl(id, i, 16);
                    const double xi = __shfl(x, i, 16);
                    acc += Mm[idi * 16 + l] * xi;
                }
            }
            return acc;
        };
        // sum_c ma[c] v_c for the variable-distributed v
        auto rows = [&](double v) {
            double acc = 0.0;
#pragma unroll
            for (int c = 0; c < 16; ++c) acc += ma[c] * __shfl(v, c, 16);
            return acc;
        };

        if constexpr (!kJvp) {
            // u = gU + Psi' gX by the costate recursion; p ends as p_0
            double u = (good && l < n) ? a.gU[b * (int64_t)n + l] : 0.0, p = 0.0;
            if (a.gX) {
                const double *gX = a.gX + b * (int64_t)R;
                const double *Ab = (const double *)a.A.ptr + b * a.A.batch_stride;
                const double *Bb = (const double *)a.B.ptr + b * a.B.batch_stride;
                p = (good && l < nx) ? gX[N * nx + l] : 0.0;
                for (int kk = N - 1; kk >= 0; --kk) {
                    const double *Ak = Ab + kk * a.A.step_stride, *Bk = Bb + kk * a.B.step_stride;
                    double accA = 0.0, accB = 0.0;
                    for (int c = 0; c < nx; ++c) {
                        const double pc = __shfl(p, c, 16);
                        if (good && l < nx) accA += Ak[c * nx + l] * pc;
                        if (good && l < nu) accB += Bk[c * nu + l] * pc;
                    }
                    const double v = __shfl(accB, (l - kk * nu) & 15, 16);
                    if (l >= kk * nu && l < (kk + 1) * nu) u += v;
                    p = ((good && l < nx) ? gX[kk * nx + l] : 0.0) + accA;
                }
            }
            // t = L^-1 u
            double t = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double uj = __shfl(u, j, 16);
                if (j <= l) t += Lt[j * 16 + l] * uj;
            }
            if (l >= n) t = 0.0;
            const double nuv = solve(rows(t));
            const double w = (l < n) ? t - rows_t(nuv) : 0.0;
            // the products with the maps
            double gx = p, gg = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double wj = __shfl(w, j, 16);
                if (l < nx) {
                    gx -= Wx[j * nx + l] * wj;
                    if (qt) gg += Wg[j * nx + l] * wj;
                }
                if (j < kmax) {
                    const double nj = __shfl(nuv, j, 16);
                    const int idj = __shfl(id, j, 16);
                    if (l < nx) gx -= Hx[idj * nx + l] * nj;
                }
            }
            if (valid && l < nx) {
                a.g_x0[b * nx + l] = good ? gx : 0.0;
                if (a.g_goal) a.g_goal[b * nx + l] = good ? gg : 0.0;
            }
            if (a.g_e) {  // nu of row r sits in slot popc(act below r); zero off the active set
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int r = l + 16 * h;
                    const int pos = __popc(act & ((1u << r) - 1u)) & 15;
                    const double v = __shfl(nuv, pos, 16);
                    if (valid && r < m) a.g_e[b * (int64_t)m + r] = (good && ((act >> r) & 1u)) ? v : 0.0;
                }
            }
            if (a.g_targets) {
                for (int c0 = 0; c0 < nT; c0 += 16) {
                    const int c = c0 + l;
                    double acc = 0.0;
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const double wj = __shfl(w, j, 16);
                        if (qs && c < nT) acc += Wt[j * nT + c] * wj;
                    }
                    if (valid && c < nT) a.g_targets[b * (int64_t)nT + c] = good ? acc : 0.0;
                }
            }
        } else {
            const double *Ab = a.A.ptr ? (const double *)a.A.ptr + b * a.A.batch_stride : nullptr;
            const double *Bb = a.B.ptr ? (const double *)a.B.ptr + b * a.B.batch_stride : nullptr;
            for (int tt = 0; tt < a.ntan; ++tt) {
                const double *dx0 = good ? tangent_of(a.tan.dx0, a.tan.dx0_stride, b, tt, nx) : nullptr;
                const double *dgl = (good && qt) ? tangent_of(a.tan.dgoal, a.tan.dgoal_stride, b, tt, nx) : nullptr;
                const double *dtg = (good && qs) ? tangent_of(a.tan.dtargets, a.tan.dtargets_stride, b, tt, nT) : nullptr;
                const double *de = good ? tangent_of(a.tan.de, a.tan.de_stride, b, tt, m) : nullptr;
                double r = 0.0, dh = de ? (l < k ? de[id] : 0.0) : 0.0;
                for (int c = 0; c < nx; ++c) {
                    const double x = dx0 ? dx0[c] : 0.0, gl = dgl ? dgl[c] : 0.0;
                    r -= Wx[l * nx + c] * x - Wg[l * nx + c] * gl;
                    if (l < k) dh -= Hx[id * nx + c] * x;
                }
                if (dtg)
                    for (int c = 0; c < nT; ++c) r += Wt[l * nT + c] * dtg[c];
                if (!good || l >= n) r = 0.0;
                const double mu = solve(rows(r) - (l < k ? dh : 0.0));
                const double x = (l < n) ? r - rows_t(mu) : 0.0;
                double du = 0.0;  // dU = L^-T x
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const double xj = __shfl(x, j, 16);
                    if (j >= l) du += Lt[l * 16 + j] * xj;
                }
                if (!good) du = 0.0;
                if (valid && l < n) a.dU[(b * a.ntan + tt) * (int64_t)n + l] = du;
                if (a.dX) {
                    double *dXo = a.dX + (b * a.ntan + tt) * (int64_t)R;
                    double xs = (dx0 && l < nx) ? dx0[l] : 0.0;
                    if (valid && l < nx) dXo[l] = xs;
                    for (int kk = 0; kk < N; ++kk) {
                        const double *Ak = Ab + kk * a.A.step_stride, *Bk = Bb + kk * a.B.step_stride;
                        double acc = 0.0;
                        for (int c = 0; c < nx; ++c) {
                            const double xc = __shfl(xs, c, 16);
                            if (good && l < nx) acc += Ak[l * nx + c] * xc;
                        }
                        for (int j = 0; j < nu; ++j) {
                            const double uj = __shfl(du, kk * nu + j, 16);
                            if (good && l < nx) acc += Bk[l * nu + j] * uj;
                        }
                        xs = acc;
                        if (valid && l < nx) dXo[(kk + 1) * nx + l] = xs;
                    }
                }
            }
        }
        if (valid && l == 0 && a.out_status) a.out_status[b] = verdict;
    }
}

// ------------------------------------------------------------------------------------------------ closed loops
// (SmallKkt, the KKT block of one problem on its sixteen lanes: mpcqp_model_small.h)
// mpcqp_model_periods_vjp_batch: the layout of the kernel above -- sixteen lanes per LOOP, four loops per wavefront, the LDS
// image staged once per workgroup, workgroups striding over the batch -- with the period loop running backwards inside. Lane
// l of a row carries component l of the costate `cs`, row l of g_A and g_B, component l of the period-summed g_goal and
// components l, l + 16, ... of the period-summed g_targets, all in registers. A period without a plan, a loop past the end of
// the batch or a failed model takes every wavefront-wide step with zeros: no lane leaves before the last one.
__global__ void __launch_bounds__(kSmallThreads) mpcqp_loop_adjoint_small_kernel(const LoopAdjointLaunch a)
{
    extern __shared__ double lds_image[];
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, nT = N * nx, P = a.nperiods;
    const ModelLayout ml = make_model_layout(nx, N, n, m);
    const SmallImage im = make_small_image(nx, N, m);
    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
    {
        const int tid = threadIdx.x;
        for (int i = tid; i < m * 16; i += kSmallThreads) lds_image[im.M + i] = a.model[ml.off_M + i];
        for (int i = tid; i < 256; i += kSmallThreads) lds_image[im.Lt + i] = a.model[ml.off_LinvT + i];
        for (int i = tid; i < 16 * nx; i += kSmallThreads) {
            lds_image[im.Wx + i] = a.model[ml.off_Wx + i];
            if (qt) lds_image[im.Wg + i] = a.model[ml.off_Wg + i];
        }
        if (qs)
            for (int i = tid; i < 16 * nT; i += kSmallThreads) lds_image[im.Wt + i] = a.model[ml.off_Wt + i];
        for (int i = tid; i < m * nx; i += kSmallThreads) lds_image[im.Hx + i] = a.model[ml.off_Hx + i];
    }
    const bool model_bad = a.model[ml.total] != 0.0;
    __syncthreads();
    const double *Mm = lds_image + im.M, *Lt = lds_image + im.Lt, *Wx = lds_image + im.Wx, *Wg = lds_image + im.Wg;
    const double *Wt = lds_image + im.Wt, *Hx = lds_image + im.Hx;
    const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15;
    const int slot = (threadIdx.x >> 6) * 4 + g;  // this row's loop within the round
    double *const gg_out = (double *)a.g_goal.ptr, *const gt_out = (double *)a.g_targets.ptr;
    const bool gg_sum = a.g_goal.period_stride == 0, gt_sum = a.g_targets.period_stride == 0;

    for (int64_t base = (int64_t)blockIdx.x * kSmallPerBlock; base < a.batch; base += (int64_t)gridDim.x * kSmallPerBlock) {
        const bool valid = base + slot < a.batch;
        const int64_t b = valid ? base + slot : 0;  // (a row past the end of the batch addresses loop 0 and touches nothing)
        const bool on = valid && !model_bad;
        const double *Ab = (const double *)a.A.ptr + b * a.A.batch_stride;
        const double *Bb = (const double *)a.B.ptr + b * a.B.batch_stride;
        const double *gXb = a.gX ? a.gX + b * (P + 1) * nx : nullptr;
        double cs = (on && gXb && l < nx) ? gXb[P * nx + l] : 0.0;  // the costate a_P
        if (a.g_states && valid && l < nx) a.g_states[(b * (P + 1) + P) * nx + l] = cs;
        double gA[16], gB[16], gt[16], ggs = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) gA[c] = gB[c] = gt[c] = 0.0;
        int fails = 0;

        for (int t = P - 1; t >= 0; --t) {
            const int64_t bt = b * P + t;
            // the plant: g_A += a x_t', g_B += a u0_t', ubar = gU0_t + B' a, a_new = gX_t + A' a
            if (a.g_A) {
                const double xt = (on && l < nx) ? a.X[(b * (P + 1) + t) * nx + l] : 0.0;
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < nx) gA[c] += cs * __shfl(xt, c, 16);
            }
            if (a.g_B) {
                const double ut = (on && l < nu) ? a.U0[bt * nu + l] : 0.0;
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < nu) gB[c] += cs * __shfl(ut, c, 16);
            }
            double accA = 0.0, accB = 0.0;
            for (int c = 0; c < nx; ++c) {
                const double pc = __shfl(cs, c, 16);
                if (on && l < nx) accA += Ab[c * nx + l] * pc;
                if (on && l < nu) accB += Bb[c * nu + l] * pc;
            }
            const double u = ((on && a.gU0 && l < nu) ? a.gU0[bt * nu + l] : 0.0) + accB;  // (zero from lane nu on)
            double an = ((on && gXb && l < nx) ? gXb[t * nx + l] : 0.0) + accA;
            // the period's plan on its active set
            const bool live = on && a.status[bt] == 0;
            SmallKkt q;
            const bool fits = q.build(Mm, a.lam + bt * m, live, l, g, n, m);
            const bool pd = q.factor(l);
            const bool good = live && fits && pd;
            if (live && !good) ++fails;
            // tt = L^-1 [ubar; 0]
            double tt = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                if (j < nu) {
                    const double uj = __shfl(u, j, 16);
                    if (j <= l) tt += Lt[j * 16 + l] * uj;
                }
            }
            if (l >= n || !good) tt = 0.0;
            const double nuv = q.solve(q.rows(tt), l);
            const double w = (l < n) ? tt - q.rows_t(Mm, nuv, l) : 0.0;
            // a_new -= Wx' w + Hx_A' nu, g_goal_t = Wg' w
            double gx = an, gg = 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const double wj = __shfl(w, j, 16);
                if (l < nx) {
                    gx -= Wx[j * nx + l] * wj;
                    if (qt) gg += Wg[j * nx + l] * wj;
                }
                if (j < q.kmax) {
                    const double nj = __shfl(nuv, j, 16);
                    const int idj = __shfl(q.id, j, 16);
                    if (l < nx) gx -= Hx[idj * nx + l] * nj;
                }
            }
            if (good) an = gx;
            if (!good) gg = 0.0;
            if (gg_out) {
                if (gg_sum)
                    ggs += gg;
                else if (valid && l < nx)
                    gg_out[b * a.g_goal.batch_stride + t * a.g_goal.period_stride + l] = gg;
            }
            if (gt_out) {  // g_targets_t = Wt' w, sixteen components a pass
#pragma unroll
                for (int ci = 0; ci < 16; ++ci) {
                    if (ci * 16 < nT) {
                        const int c = ci * 16 + l;
                        double acc = 0.0;
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const double wj = __shfl(w, j, 16);
                            if (qs && c < nT) acc += Wt[j * nT + c] * wj;
                        }
                        if (!good) acc = 0.0;
                        if (gt_sum)
                            gt[ci] += acc;
                        else if (valid && c < nT)
                            gt_out[b * a.g_targets.batch_stride + t * a.g_targets.period_stride + c] = acc;
                    }
                }
            }
            cs = an;
            if (a.g_states && valid && l < nx) a.g_states[(b * (P + 1) + t) * nx + l] = cs;
        }

        if (valid && l < nx) {
            a.g_x0[b * nx + l] = cs;
            if (gg_out && gg_sum) gg_out[b * a.g_goal.batch_stride + l] = ggs;
            if (a.g_A) {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < nx) a.g_A[(b * nx + l) * nx + c] = gA[c];
            }
            if (a.g_B) {
#pragma unroll
                for (int c = 0; c < 16; ++c)
                    if (c < nu) a.g_B[(b * nx + l) * nu + c] = gB[c];
            }
        }
        if (gt_out && gt_sum) {
#pragma unroll
            for (int ci = 0; ci < 16; ++ci) {
                const int c = ci * 16 + l;
                if (valid && c < nT) gt_out[b * a.g_targets.batch_stride + c] = gt[ci];
            }
        }
        if (valid && l == 0 && a.out_status) a.out_status[b] = model_bad ? P : fails;
    }
}

// ------------------------------------------------------------------------------------------------ general models
// LDS carve of the general kernel, in doubles: S (n x ld), the vectors, two state vectors that roll along the horizon,
// then the active rows' ids
struct GeneralCarve {
    int ld, S, t, nu, w, u, p, idx, total;
};
__host__ __device__ inline GeneralCarve make_general_carve(int n, int nx)
{
    GeneralCarve c{};
    c.ld = n | 1;
    c.S = 0;
    c.t = c.S + n * c.ld;
    c.nu = c.t + n;
    c.w = c.nu + n;
    c.u = c.w + n;
    c.p = c.u + n;
    c.idx = c.p + 2 * nx;
    c.total = c.idx + (n + 2) / 2;
    return c;
}

constexpr int kGeneralThreads = 256;

template <bool kJvp>
__global__ void __launch_bounds__(kGeneralThreads) mpcqp_model_diff_general_kernel(const ModelDiffLaunch a)
{
    constexpr int BS = kGeneralThreads;
    extern __shared__ double lds_carve[];
    __shared__ int s_k;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, nT = N * nx, R = (N + 1) * nx;
    const ModelLayout ml = make_model_layout(nx, N, n, m);
    const int nc = ml.nc;
    const GeneralCarve cv = make_general_carve(n, nx);
    const int ld = cv.ld;
    double *S = lds_carve + cv.S, *t = lds_carve + cv.t, *nuv = lds_carve + cv.nu, *w = lds_carve + cv.w;
    double *u = lds_carve + cv.u, *p = lds_carve + cv.p;
    int *idx = (int *)(lds_carve + cv.idx);
    const double *Mm = a.model + ml.off_M, *Lt = a.model + ml.off_LinvT, *Hx = a.model + ml.off_Hx;
    const double *Wx = a.model + ml.off_Wx, *Wg = a.model + ml.off_Wg, *Wt = a.model + ml.off_Wt;
    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
    const double *Ab = a.A.ptr ? (const double *)a.A.ptr + b * a.A.batch_stride : nullptr;
    const double *Bb = a.B.ptr ? (const double *)a.B.ptr + b * a.B.batch_stride : nullptr;

    int verdict = a.model[ml.total] != 0.0 ? MPCQP_NOT_PD : a.status[b];
    int k = 0;
    if (verdict == 0) {
        k = active_rows(a.lam ? a.lam + b * (int64_t)m : nullptr, m, n, idx, &s_k);
        if (k > n) verdict = MPCQP_NOT_PD;
    }
    if (verdict == 0) {
        // lower triangle of S = M_A M_A' from the model's rows
        for (int e = tid; e < k * k; e += BS) {
            const int i = e / k, j = e % k;
            if (j <= i) {
                const double *mi = Mm + (size_t)idx[i] * nc, *mj = Mm + (size_t)idx[j] * nc;
                double acc = 0.0;
                for (int c = 0; c < n; ++c) acc += mi[c] * mj[c];
                S[i * ld + j] = acc;
            }
        }
        if (!chol_lower<BS, true>(S, k, ld, tid, gram_pivot_floor(n, k))) verdict = MPCQP_NOT_PD;
    }
    // nu <- S^-1 (M_A v - sub) for v (n) in LDS; then out = v - M_A' nu. Called by the whole workgroup.
    auto kkt = [&](const double *v, const double *sub, double *out) {
        for (int i = tid; i < k; i += BS) {
            const double *mi = Mm + (size_t)idx[i] * nc;
            double acc = sub ? -sub[i] : 0.0;
            for (int c = 0; c < n; ++c) acc += mi[c] * v[c];
            nuv[i] = acc;
        }
        __syncthreads();
        solve_lower<BS>(S, k, ld, nuv, tid);
        solve_lower_t<BS>(S, k, ld, nuv, tid);
        for (int j = tid; j < n; j += BS) {
            double acc = v[j];
            for (int r = 0; r < k; ++r) acc -= Mm[(size_t)idx[r] * nc + j] * nuv[r];
            out[j] = acc;
        }
        __syncthreads();
    };

    if constexpr (!kJvp) {
        double *gx0 = a.g_x0 + b * nx;
        double *ggoal = out_at(a.g_goal, b * nx), *gtgt = out_at(a.g_targets, b * (int64_t)nT);
        double *ge = out_at(a.g_e, b * (int64_t)m);
        if (verdict == 0) {
            const double *gU = a.gU + b * (int64_t)n;
            for (int i = tid; i < n; i += BS) u[i] = gU[i];
            double *pc = p, *pn = p + nx;
            for (int i = tid; i < nx; i += BS) pc[i] = a.gX ? a.gX[b * (int64_t)R + N * nx + i] : 0.0;
            __syncthreads();
            if (a.gX) {  // u += Psi' gX, p_0 by the costate recursion
                const double *gX = a.gX + b * (int64_t)R;
                for (int kk = N - 1; kk >= 0; --kk) {
                    const double *Ak = Ab + kk * a.A.step_stride, *Bk = Bb + kk * a.B.step_stride;
                    for (int e = tid; e < nx + nu; e += BS) {
                        double acc = 0.0;
                        if (e < nx) {
                            for (int j = 0; j < nx; ++j) acc += Ak[j * nx + e] * pc[j];
                            pn[e] = gX[kk * nx + e] + acc;
                        } else {
                            const int j = e - nx;
                            for (int c = 0; c < nx; ++c) acc += Bk[c * nu + j] * pc[c];
                            u[kk * nu + j] += acc;
                        }
                    }
                    __syncthreads();
                    double *sw = pc;
                    pc = pn;
                    pn = sw;
                }
            }
            for (int i = tid; i < n; i += BS) {  // t = L^-1 u
                double acc = 0.0;
                for (int j = 0; j <= i; ++j) acc += Lt[(size_t)j * nc + i] * u[j];
                t[i] = acc;
            }
            __syncthreads();
            kkt(t, nullptr, w);
            for (int c = tid; c < nx; c += BS) {
                double acc = pc[c], gg = 0.0;
                for (int j = 0; j < n; ++j) {
                    acc -= Wx[(size_t)j * nx + c] * w[j];
                    if (qt) gg += Wg[(size_t)j * nx + c] * w[j];
                }
                for (int r = 0; r < k; ++r) acc -= Hx[(size_t)idx[r] * nx + c] * nuv[r];
                gx0[c] = acc;
                if (ggoal) ggoal[c] = gg;
            }
            if (gtgt)
                for (int c = tid; c < nT; c += BS) {
                    double acc = 0.0;
                    if (qs)
                        for (int j = 0; j < n; ++j) acc += Wt[(size_t)j * nT + c] * w[j];
                    gtgt[c] = acc;
                }
            if (ge)
                for (int i = tid; i < m; i += BS) {
                    const int lo = lower_bound(idx, k, i);
                    ge[i] = (lo < k && idx[lo] == i) ? nuv[lo] : 0.0;
                }
        } else {
            zero_outputs<BS>(tid, gx0, nx, ggoal, nx, gtgt, (int64_t)nT, ge, m);
        }
    } else {
        double *dU = a.dU + b * a.ntan * (int64_t)n;
        double *dX = out_at(a.dX, b * a.ntan * (int64_t)R);
        if (verdict == 0) {
            for (int tt = 0; tt < a.ntan; ++tt) {
                const double *dx0 = tangent_of(a.tan.dx0, a.tan.dx0_stride, b, tt, nx);
                const double *dgl = qt ? tangent_of(a.tan.dgoal, a.tan.dgoal_stride, b, tt, nx) : nullptr;
                const double *dtg = qs ? tangent_of(a.tan.dtargets, a.tan.dtargets_stride, b, tt, nT) : nullptr;
                const double *de = tangent_of(a.tan.de, a.tan.de_stride, b, tt, m);
                for (int j = tid; j < n; j += BS) {  // r = -dd
                    double acc = 0.0;
                    for (int c = 0; c < nx; ++c) {
                        if (dx0) acc -= Wx[(size_t)j * nx + c] * dx0[c];
                        if (dgl) acc += Wg[(size_t)j * nx + c] * dgl[c];
                    }
                    if (dtg)
                        for (int c = 0; c < nT; ++c) acc += Wt[(size_t)j * nT + c] * dtg[c];
                    t[j] = acc;
                }
                for (int i = tid; i < k; i += BS) {  // dh on the active rows
                    double acc = de ? de[idx[i]] : 0.0;
                    if (dx0)
                        for (int c = 0; c < nx; ++c) acc -= Hx[(size_t)idx[i] * nx + c] * dx0[c];
                    u[i] = acc;
                }
                __syncthreads();
                kkt(t, u, w);
                for (int i = tid; i < n; i += BS) {  // dU = L^-T x
                    double acc = 0.0;
                    for (int j = i; j < n; ++j) acc += Lt[(size_t)i * nc + j] * w[j];
                    u[i] = acc;
                    dU[tt * (int64_t)n + i] = acc;
                }
                double *pc = p, *pn = p + nx;
                if (dX)
                    for (int i = tid; i < nx; i += BS) dX[tt * (int64_t)R + i] = pc[i] = dx0 ? dx0[i] : 0.0;
                __syncthreads();
                if (dX) {
                    for (int kk = 0; kk < N; ++kk) {
                        const double *Ak = Ab + kk * a.A.step_stride, *Bk = Bb + kk * a.B.step_stride;
                        for (int i = tid; i < nx; i += BS) {
                            double acc = 0.0;
                            for (int c = 0; c < nx; ++c) acc += Ak[i * nx + c] * pc[c];
                            for (int j = 0; j < nu; ++j) acc += Bk[i * nu + j] * u[kk * nu + j];
                            pn[i] = acc;
                            dX[tt * (int64_t)R + (kk + 1) * nx + i] = acc;
                        }
                        __syncthreads();
                        double *sw = pc;
                        pc = pn;
                        pn = sw;
                    }
                }
            }
        } else {
            zero_outputs<BS>(tid, dU, a.ntan * (int64_t)n, dX, a.ntan * (int64_t)R);
        }
    }
    if (a.out_status && tid == 0) a.out_status[b] = verdict;
}

}  // namespace

bool model_diff_small_applies(int nx, int n, int m) { return n <= 16 && m <= 32 && nx <= 16; }

int launch_model_diff_small(const ModelDiffLaunch &l, hipStream_t st)
{
    const size_t lds = (size_t)make_small_image(l.nx, l.N, l.m).total * sizeof(double);
    // (at most 47,104 bytes inside the envelope, at nx = 16, N = 16, m = 32: below the 48 KiB a launch gets unasked)
    auto kern = l.ntan > 0 ? mpcqp_model_diff_small_kernel<true> : mpcqp_model_diff_small_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)model_diff_small_grid(l.batch)), dim3(kSmallThreads), lds, st, l);
    return (int)hipGetLastError();
}

int launch_loop_adjoint_small(const LoopAdjointLaunch &l, hipStream_t st)
{
    const size_t lds = (size_t)make_small_image(l.nx, l.N, l.m).total * sizeof(double);  // (the image of the kernel above)
    hipLaunchKernelGGL(mpcqp_loop_adjoint_small_kernel, dim3((unsigned)model_diff_small_grid(l.batch)), dim3(kSmallThreads),
                       lds, st, l);
    return (int)hipGetLastError();
}

size_t model_diff_general_lds_bytes(int nx, int n) { return (size_t)make_general_carve(n, nx).total * sizeof(double); }

int launch_model_diff_general(const ModelDiffLaunch &l, hipStream_t st)
{
    const size_t lds = model_diff_general_lds_bytes(l.nx, l.n);
    auto kern = l.ntan > 0 ? mpcqp_model_diff_general_kernel<true> : mpcqp_model_diff_general_kernel<false>;
    return launch_per_problem(kern, l, kGeneralThreads, lds, l.batch, st);
}

}  // namespace mpcqp
