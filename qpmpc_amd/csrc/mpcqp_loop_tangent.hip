// mpcqp_loop_tangent.hip -- forward sensitivities of closed loops of a factored shared model:
// mpcqp_model_periods_jvp_batch (include/mpcqp.h; DESIGN.md section 9, "Closed-loop forward sensitivities").
//
// The loop of mpcqp_model_periods_batch -- u0_t the plan's first input, zero without a plan, x_{t+1} = A x_t + B u0_t + d_t --
// linearised along its records: dx_0 = dx0, and for t = 0 .. P-1, on the active set A_t = {i : lam_i > 0} of the period's
// plan, S = M_A M_A' (the whitened maps of mpcqp_model_adjoint.hip),
//     r = -(Wx dx_t - Wg dgoal_t - Wt dtargets_t),  mu = S^-1 (M_A r + Hx_A dx_t),  du0_t = [L^-T (r - M_A' mu)]_{0 .. nu-1}
//     dx_{t+1} = A dx_t + B du0_t + dd_t + dA x_t + dB u0_t
// and du0_t = 0 for a period without a plan, with more active rows than variables or whose S fails the pivot test.
//   mpcqp_loop_tangent_small_kernel  the layout of mpcqp_loop_adjoint_small_kernel: sixteen lanes per LOOP, four loops per
//                                    wavefront, the LDS image staged once per workgroup, workgroups striding over the batch,
//                                    the period loop running FORWARDS inside. S does not depend on the tangent: a period's
//                                    active rows are gathered and S is factored ONCE and every tangent of the pass reuses
//                                    the factor. A pass holds up to sixteen tangents, lane l carrying component l of dx of
//                                    each in registers; more tangents take the period loop again per chunk of sixteen.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mpcqp.h"
#include "mpcqp_internal.h"
#include "mpcqp_lane.h"
#include "mpcqp_model_small.h"

namespace mpcqp {

namespace {

constexpr int kPassTangents = 16;

// The carried tangents of a pass as a queue in registers, every index a constant: the tangent in turn is v[0]; its successor
// goes to the end of the queue of `nt`, the others move up. After nt turns the queue is in order again.
__device__ __forceinline__ void rotate(double (&v)[kPassTangents], int nt, double x)
{
#pragma unroll
    for (int i = 0; i + 1 < kPassTangents; ++i) v[i] = (i == nt - 1) ? x : v[i + 1];
    v[kPassTangents - 1] = (nt == kPassTangents) ? x : 0.0;
}

__device__ __forceinline__ const double *period_tangent(const MpcqpPeriodTangent &p, int64_t b)
{
    return p.ptr ? (const double *)p.ptr + b * p.batch_stride : nullptr;
}

// Lane l of a row is variable l (r, y), active slot l (its row of S, mu), state component l (dx, the records, the rows of the
// plant and of dA / dB) and inequality rows l and l + 16. A period without a plan, a loop past the end of the batch or a
// failed model takes every wavefront-wide step with zeros and differs only in what it stores: no lane leaves before the last.
__global__ void __launch_bounds__(kSmallThreads) mpcqp_loop_tangent_small_kernel(const LoopTangentLaunch a)
{
    extern __shared__ double lds_image[];
    const int nx = a.nx, nu = a.nu, N = a.N, n = a.n, m = a.m, nT = N * nx, P = a.nperiods, ntan = a.ntan;
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

    for (int64_t base = (int64_t)blockIdx.x * kSmallPerBlock; base < a.batch; base += (int64_t)gridDim.x * kSmallPerBlock) {
        const bool valid = base + slot < a.batch;
        const int64_t b = valid ? base + slot : 0;  // (a row past the end of the batch addresses loop 0 and touches nothing)
        const bool on = valid && !model_bad, xrow = on && l < nx;
        const double *Bb = (const double *)a.B.ptr + b * a.B.batch_stride;
        const double *dx0 = a.tan.dx0 ? (const double *)a.tan.dx0 + b * a.tan.dx0_stride : nullptr;
        const double *dgl = qt ? period_tangent(a.tan.dgoal, b) : nullptr;
        const double *dtg = qs ? period_tangent(a.tan.dtargets, b) : nullptr;
        const double *ddp = period_tangent(a.tan.dd, b);
        const double *dAp = a.tan.dA ? (const double *)a.tan.dA + b * a.tan.dA_stride : nullptr;
        const double *dBp = a.tan.dB ? (const double *)a.tan.dB + b * a.tan.dB_stride : nullptr;
        double Arow[16];  // this component's row of the plant's A
        {
            const double *Ab = (const double *)a.A.ptr + b * a.A.batch_stride;
#pragma unroll
            for (int c = 0; c < 16; ++c) Arow[c] = (xrow && c < nx) ? Ab[l * nx + c] : 0.0;
        }
        int fails = 0;

        for (int j0 = 0; j0 < ntan; j0 += kPassTangents) {
            const int nt = min(kPassTangents, ntan - j0);
            double dx[kPassTangents];  // component l of dx_t of the pass's tangents
#pragma unroll
            for (int j = 0; j < kPassTangents; ++j) {
                dx[j] = 0.0;
                if (j < nt) {
                    const int64_t jj = j0 + j;
                    if (dx0 && xrow) dx[j] = dx0[jj * nx + l];
                    if (valid && l < nx) a.dX[(b * ntan + jj) * (P + 1) * nx + l] = dx[j];
                }
            }

            for (int t = 0; t < P; ++t) {
                const int64_t bt = b * P + t;
                // the period's plan on its active set, once for every tangent of the pass
                const bool live = on && a.status[bt] == 0;
                SmallKkt q;
                const bool fits = q.build(Mm, a.lam + bt * m, live, l, g, n, m);
                const bool pd = q.factor(l);
                const bool good = live && fits && pd;
                if (j0 == 0 && live && !good) ++fails;
                const double xt = (dAp && xrow) ? a.X[(b * (P + 1) + t) * nx + l] : 0.0;
                const double ut = (dBp && on && l < nu) ? a.U0[bt * nu + l] : 0.0;

                for (int j = 0; j < nt; ++j) {
                    const int64_t jj = j0 + j;
                    const double x = dx[0];  // the tangent in turn (zero from lane nx on)
                    // r = -(Wx dx - Wg dgoal - Wt dtargets) on lane l; Hx_A dx on slot l
                    double r = 0.0, hx = 0.0;
                    for (int c = 0; c < nx; ++c) {
                        const double xc = __shfl(x, c, 16);
                        r -= Wx[l * nx + c] * xc;
                        hx += Hx[q.id * nx + c] * xc;
                    }
                    if (dgl) {
                        const double v = xrow ? dgl[jj * a.tan.dgoal.tangent_stride + t * a.tan.dgoal.period_stride + l] : 0.0;
                        for (int c = 0; c < nx; ++c) r += Wg[l * nx + c] * __shfl(v, c, 16);
                    }
                    if (dtg) {  // sixteen components a pass
                        const double *dt = dtg + jj * a.tan.dtargets.tangent_stride + t * a.tan.dtargets.period_stride;
                        for (int c0 = 0; c0 < nT; c0 += 16) {
                            const double v = (on && c0 + l < nT) ? dt[c0 + l] : 0.0;
                            const int w = min(16, nT - c0);
                            for (int c = 0; c < w; ++c) r += Wt[l * nT + c0 + c] * __shfl(v, c, 16);
                        }
                    }
                    if (!good || l >= n) r = 0.0;
                    const double mu = q.solve(q.rows(r) + ((good && l < q.k) ? hx : 0.0), l);
                    const double y = (l < n) ? r - q.rows_t(Mm, mu, l) : 0.0;
                    // du0 = the first nu entries of L^-T y: entry i on lane i
                    double du = 0.0;
                    for (int i = 0; i < nu; ++i) {
                        const double s = row_sum_dpp(l >= i ? Lt[i * 16 + l] * y : 0.0);
                        if (l == i) du = s;
                    }
                    if (!good) du = 0.0;
                    if (a.dU0 && valid && l < nu) a.dU0[((b * ntan + jj) * P + t) * nu + l] = du;
                    // the plant: dx+ = A dx + B du0 + dd + dA x_t + dB u0_t
                    double acc = (ddp && xrow) ? ddp[jj * a.tan.dd.tangent_stride + t * a.tan.dd.period_stride + l] : 0.0;
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (c < nx) acc += Arow[c] * __shfl(x, c, 16);
                    for (int i = 0; i < nu; ++i) {
                        const double ui = __shfl(du, i, 16);
                        if (xrow) acc += Bb[l * nu + i] * ui;
                    }
                    if (dAp) {
                        const double *dA = dAp + jj * nx * nx;
                        for (int c = 0; c < nx; ++c) {
                            const double xc = __shfl(xt, c, 16);
                            if (xrow) acc += dA[l * nx + c] * xc;
                        }
                    }
                    if (dBp) {
                        const double *dB = dBp + jj * nx * nu;
                        for (int i = 0; i < nu; ++i) {
                            const double ui = __shfl(ut, i, 16);
                            if (xrow) acc += dB[l * nu + i] * ui;
                        }
                    }
                    if (!xrow) acc = 0.0;
                    if (valid && l < nx) a.dX[((b * ntan + jj) * (P + 1) + t + 1) * nx + l] = acc;
                    rotate(dx, nt, acc);
                }
            }
        }
        if (valid && l == 0 && a.out_status) a.out_status[b] = model_bad ? P : fails;
    }
}

}  // namespace

int launch_loop_tangent_small(const LoopTangentLaunch &l, hipStream_t st)
{
    const size_t lds = (size_t)make_small_image(l.nx, l.N, l.m).total * sizeof(double);  // (at most 47,104 bytes)
    hipLaunchKernelGGL(mpcqp_loop_tangent_small_kernel, dim3((unsigned)model_diff_small_grid(l.batch)), dim3(kSmallThreads),
                       lds, st, l);
    return (int)hipGetLastError();
}

}  // namespace mpcqp
