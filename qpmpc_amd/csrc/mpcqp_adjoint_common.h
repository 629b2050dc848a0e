// Device code shared by the adjoint kernels: mpcqp_adjoint.hip (the condensed adjoint and the tangent kernel) and
// mpcqp_adjoint_stagewise.hip. One problem per workgroup of BS threads; every helper is called by the whole workgroup with
// uniform arguments.
#ifndef MPCQP_ADJOINT_COMMON_H_
#define MPCQP_ADJOINT_COMMON_H_

#include <hip/hip_runtime.h>

#include "mpcqp.h"
#include "mpcqp_internal.h"

namespace mpcqp {

__device__ inline const double *op_step(const MpcqpOperand &o, int64_t b, int k)
{
    return o.ptr ? (const double *)o.ptr + b * o.batch_stride + (int64_t)k * o.step_stride : nullptr;
}

// problem b's part of a nullable output packed per problem
__device__ inline double *out_at(void *p, int64_t off) { return p ? (double *)p + off : nullptr; }

// The pivot test of the Gram matrix S = M_A M_A' of k whitened active rows of n entries: pivot j, the squared distance of
// row j from the span of the rows before it, must exceed gram_pivot_floor(n, k) times S_jj as it was before elimination.
// Where row j is a multiple f of an earlier row i the exact pivot is 0 and the computed one is rounding: the factor computed
// is the exact factor of S + dS with |dS_ij| <= gamma_{k+1} sqrt(S_ii S_jj) (Higham, Accuracy and Stability, theorem 10.3),
// on top of the gamma_n sqrt(S_ii S_jj) of the n-term sums that formed S (Cauchy-Schwarz), and the pivot moves by
// dS_jj - 2 f dS_ji + f^2 dS_ii. With S_jj = f^2 S_ii the three terms are at most gamma S_jj, 2 |f| gamma sqrt(S_ii S_jj) =
// 2 gamma S_jj and f^2 gamma S_ii = gamma S_jj: 4 (gamma_n + gamma_{k+1}) S_jj <= 4 (n + k + 1) 2^-53 S_jj for EVERY f, whichever
// of the two rows comes first. So a row that is a multiple of ONE earlier active row (a row stated twice, a row and its
// multiple, both halves of an equality) is MPCQP_NOT_PD whatever the sign of the rounding. A row that is a combination
// sum_i x_i row_i of SEVERAL earlier rows is not covered by this bound: its pivot moves by up to
// (sqrt(S_jj) + sum_i |x_i| sqrt(S_ii))^2 gamma, which grows with the conditioning of those rows, so there the verdict can
// still depend on rounding. Rows that pass are at an angle of more than 1e-7 or so to the span of their predecessors. A
// zero row (S_jj = 0) fails as before.
__host__ __device__ inline double gram_pivot_floor(int n, int k) { return 4.0 * (double)(n + k + 1) * 0x1p-53; }

// In-place lower Cholesky of the nn x nn matrix a (stride ld; only the lower triangle is read or written).
// Uniform result: every thread reads the same pivot after a barrier. kGram: the pivot test above, with rel =
// gram_pivot_floor(n, k); the diagonal before elimination is kept in row 0 of the (otherwise unused) strict upper triangle.
template <int BS, bool kGram = false>
__device__ inline bool chol_lower(double *a, int nn, int ld, int tid, double rel = 0.0)
{
    if (kGram) {
        __syncthreads();  // (the callers form S without a barrier behind it)
        for (int j = 1 + tid; j < nn; j += BS) a[j] = a[j * ld + j];
    }
    for (int j = 0; j < nn; ++j) {
        __syncthreads();
        const double d = a[j * ld + j];
        if (!(d > (kGram ? rel * a[j] : 0.0))) return false;  // (j = 0: a[0] is d itself)
        const double sd = sqrt(d), inv = 1.0 / sd;
        __syncthreads();
        if (tid == 0) a[j * ld + j] = sd;
        for (int i = j + 1 + tid; i < nn; i += BS) a[i * ld + j] *= inv;
        __syncthreads();
        const int w = nn - j - 1;
        for (int e = tid; e < w * w; e += BS) {
            const int i = j + 1 + e / w, c = j + 1 + e % w;
            if (c <= i) a[i * ld + c] -= a[i * ld + j] * a[c * ld + j];
        }
    }
    __syncthreads();
    return true;
}

// x <- R^-1 x, then (transposed) x <- R^-T x for one vector and the lower factor R (stride ld)
template <int BS>
__device__ inline void solve_lower(const double *R, int nn, int ld, double *x, int tid)
{
    for (int j = 0; j < nn; ++j) {
        if (tid == 0) x[j] /= R[j * ld + j];
        __syncthreads();
        for (int i = j + 1 + tid; i < nn; i += BS) x[i] -= R[i * ld + j] * x[j];
        __syncthreads();
    }
}
template <int BS>
__device__ inline void solve_lower_t(const double *R, int nn, int ld, double *x, int tid)
{
    for (int j = nn - 1; j >= 0; --j) {
        if (tid == 0) x[j] /= R[j * ld + j];
        __syncthreads();
        for (int i = tid; i < j; i += BS) x[i] -= R[j * ld + i] * x[j];
        __syncthreads();
    }
}

// The same solves for nr right-hand sides stored as rows (rows[r * ld + j], the stride of L), column by column:
// rows <- rows L^-T (each row x <- L^-1 x), and the transposed sweep rows <- rows L^-1 (each row x <- L^-T x)
template <int BS>
__device__ inline void sweep_lower(const double *L, int nn, int ld, double *rows, int nr, int tid)
{
    for (int j = 0; j < nn; ++j) {
        const double inv = 1.0 / L[j * ld + j];
        for (int r = tid; r < nr; r += BS) rows[r * ld + j] *= inv;
        __syncthreads();
        const int w = nn - j - 1;
        for (int e = tid; e < nr * w; e += BS) {
            const int r = e / w, i = j + 1 + e % w;
            rows[r * ld + i] -= L[i * ld + j] * rows[r * ld + j];
        }
        __syncthreads();
    }
}
template <int BS>
__device__ inline void sweep_lower_t(const double *L, int nn, int ld, double *rows, int nr, int tid)
{
    for (int j = nn - 1; j >= 0; --j) {
        const double inv = 1.0 / L[j * ld + j];
        for (int r = tid; r < nr; r += BS) rows[r * ld + j] *= inv;
        __syncthreads();
        for (int e = tid; e < nr * j; e += BS) {
            const int r = e / j, i = e % j;
            rows[r * ld + i] -= L[j * ld + i] * rows[r * ld + j];
        }
        __syncthreads();
    }
}

// Lower triangle of S = M M' (stride ld) for the k rows of M, rows r0 .. r0 + k - 1 of Z (n wide, stride ld)
template <int BS>
__device__ inline void gram_lower(const double *Z, int r0, int k, int n, int ld, double *S, int tid)
{
    for (int e = tid; e < k * k; e += BS) {
        const int i = e / k, j = e % k;
        if (j <= i) {
            const double *zi = Z + (r0 + i) * ld, *zj = Z + (r0 + j) * ld;
            double acc = 0.0;
            for (int c = 0; c < n; ++c) acc += zi[c] * zj[c];
            S[i * ld + j] = acc;
        }
    }
}

// The active rows {i < m : lam_i > 0}, ascending, compacted by wave 0 with a ballot and a prefix count per 64 rows; the
// first `cap` ids go to idx. Returns their count (which may exceed cap), the same in every thread.
__device__ inline int active_rows(const double *lam, int m, int cap, int *idx, int *s_k)
{
    const int tid = threadIdx.x;
    if (tid < 64) {
        int count = 0;
        for (int i0 = 0; i0 < m; i0 += 64) {
            const int i = i0 + tid;
            const bool act = i < m && lam[i] > 0.0;
            const unsigned long long mask = __ballot(act);
            const int pre = __popcll(mask & ((1ull << tid) - 1ull));
            if (act && count + pre < cap) idx[count + pre] = i;
            count += __popcll(mask);
        }
        if (tid == 0) *s_k = count;
    }
    __syncthreads();
    return *s_k;
}

// first position of the ascending ids idx[0 .. k) that is >= key
__device__ inline int lower_bound(const int *idx, int k, int key)
{
    int lo = 0, hi = k;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idx[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// zeros into the non-null outputs (pointer, length) of a problem that is not solved
template <int BS>
__device__ inline void zero_outputs(int tid, double *p, int64_t len)
{
    if (p)
        for (int64_t j = tid; j < len; j += BS) p[j] = 0.0;
}
template <int BS, typename... More>
__device__ inline void zero_outputs(int tid, double *p, int64_t len, More... more)
{
    zero_outputs<BS>(tid, p, len);
    zero_outputs<BS>(tid, more...);
}
// ... the model outputs g_A .. g_w of problem b
template <int BS>
__device__ inline void zero_model_outputs(const MpcqpVjpModelOut &o, int nx, int nu, int N, int m, int64_t b, int tid)
{
    const int64_t NA = (int64_t)N * nx * nx, NB = (int64_t)N * nx * nu, NC = (int64_t)m * nx, ND = (int64_t)m * nu;
    zero_outputs<BS>(tid, out_at(o.g_A, b * NA), NA, out_at(o.g_B, b * NB), NB, out_at(o.g_C, b * NC), NC,
                     out_at(o.g_D, b * ND), ND, out_at(o.g_w, b * 3), 3);
}

// acc - Y x: acc + y x where y holds -Y, acc - y x where it holds Y (the expression each kernel evaluated before)
template <bool kNegY>
__device__ inline double sub_y(double acc, double y, double x) { return kNegY ? acc + y * x : acc - y * x; }

// The vectors of model_epilogue, in the calling kernel's carve (problem b's)
struct ModelVecs {
    const double *lam, *U, *w, *y, *goal, *tgt;  // y: -Y (kNegY) or Y; goal / tgt: null where the q term is off
    const double *nua;                            // dL/dh on the k active rows idx (ascending)
    const int *idx;
    int k;
    double *p, *X, *Zf, *pz, *sc, *nuf, *wred;  // p: a = v (kWithP: recursed here), wred: 3 BS
};

// The model and cost gradients once X = rollout(x0, U), Zf = rollout(0, U), w, Y and the costate p's right-hand side (or
// p itself) are in place ("Model and cost gradients"): dL/dh over every row, the right-hand sides of
// pz and s with the partial sums of Y'E, the recursions x_k += A_k' x_{k+1} (of p too when kWithP), the outer products
// g_A .. g_D and g_w = (-Y_N'E_N, -sum_{k<N} Y_k'E_k, -w'U) by one tree reduction. kNegY: y holds -Y (the condensed
// adjoint) rather than Y (the stage-wise one). D: the kernel's dimensions (nx, nu, N, mk, n, m, flags, wt, wx).
template <int BS, bool kNegY, bool kWithP, class D>
__device__ void model_epilogue(const D &d, const MpcqpOperand &A, const MpcqpOperand &C, const MpcqpVjpModelOut &o,
                               int64_t b, const ModelVecs &v)
{
    const int tid = threadIdx.x;
    const int n = d.n, m = d.m, nx = d.nx, nu = d.nu, N = d.N, mk = d.mk;
    const int R = (N + 1) * nx;
    const bool pt = (d.flags & MPCQP_P_TERMINAL) != 0, ps = (d.flags & MPCQP_P_STAGE) != 0;
    const bool qt = (d.flags & MPCQP_Q_TERMINAL) != 0, qs = (d.flags & MPCQP_Q_STAGE) != 0;
    const double *lam = v.lam, *U = v.U, *w = v.w, *y = v.y, *X = v.X, *Zf = v.Zf;
    double *p = v.p, *pz = v.pz, *sc = v.sc, *nuf = v.nuf, *wred = v.wred;
    const double *Ab = (const double *)A.ptr + b * A.batch_stride;
    const double *Cb = C.ptr ? (const double *)C.ptr + b * C.batch_stride : nullptr;

    for (int i = tid; i < m; i += BS) nuf[i] = 0.0;
    __syncthreads();
    for (int r = tid; r < v.k; r += BS) nuf[v.idx[r]] = v.nua[r];
    double tw = 0.0, sw = 0.0;
    for (int e = tid; e < R; e += BS) {
        const int kk = e / nx, i = e % nx;
        double az = 0.0, bb = 0.0;
        if (kk < N) {
            if (ps) {
                const double E = qs ? X[e] - v.tgt[e] : Zf[e];
                bb -= d.wx * E;
                sw = sub_y<kNegY>(sw, y[e], E);
                if (!qs) az = sub_y<kNegY>(az, d.wx, y[e]);
            }
            if (Cb) {
                const double *Ck = Cb + kk * C.step_stride;
                for (int r = 0; r < mk; ++r) bb -= Ck[r * nx + i] * lam[kk * mk + r];
            }
        } else if (pt) {
            const double E = qt ? X[e] - v.goal[i] : Zf[e];
            bb -= d.wt * E;
            tw = sub_y<kNegY>(tw, y[e], E);
            if (!qt) az = sub_y<kNegY>(az, d.wt, y[e]);
        }
        pz[e] = az;
        sc[e] = bb;
    }
    __syncthreads();
    // x_k += A_k' x_{k+1} for k = N - 1 .. 0, the costates side by side
    constexpr int first = kWithP ? 0 : 1;
    for (int kk = N - 1; kk >= 0; --kk) {
        const double *Ak = Ab + kk * A.step_stride;
        for (int e = tid; e < (3 - first) * nx; e += BS) {
            const int which = e / nx + first, i = e % nx;
            double *x = which == 0 ? p : (which == 1 ? pz : sc);
            const double *xn = x + (kk + 1) * nx;
            double acc = 0.0;
            for (int j = 0; j < nx; ++j) acc += Ak[j * nx + i] * xn[j];
            x[kk * nx + i] += acc;
        }
        __syncthreads();
    }
    // outer products, packed per problem
    if (o.g_A) {
        const int64_t NA = (int64_t)N * nx * nx;
        double *gA = (double *)o.g_A + b * NA;
        for (int64_t e = tid; e < NA; e += BS) {
            const int kk = (int)(e / (nx * nx)), r = (int)(e % (nx * nx)), i = r / nx, j = r % nx;
            const int oo = (kk + 1) * nx + i, c = kk * nx + j;
            gA[e] = sub_y<!kNegY>(p[oo] * X[c] + pz[oo] * Zf[c], sc[oo], y[c]);
        }
    }
    if (o.g_B) {
        const int64_t NB = (int64_t)N * nx * nu;
        double *gB = (double *)o.g_B + b * NB;
        for (int64_t e = tid; e < NB; e += BS) {
            const int kk = (int)(e / (nx * nu)), r = (int)(e % (nx * nu)), i = r / nu, j = r % nu;
            const int oo = (kk + 1) * nx + i, c = kk * nu + j;
            gB[e] = (p[oo] + pz[oo]) * U[c] + sc[oo] * w[c];
        }
    }
    if (o.g_C) {
        const int64_t NC = (int64_t)m * nx;
        double *gC = (double *)o.g_C + b * NC;
        for (int64_t e = tid; e < NC; e += BS) {
            const int row = (int)(e / nx), i = (int)(e % nx), c = (row / mk) * nx + i;
            gC[e] = kNegY ? lam[row] * y[c] - nuf[row] * X[c] : -(lam[row] * y[c] + nuf[row] * X[c]);
        }
    }
    if (o.g_D) {
        const int64_t ND = (int64_t)m * nu;
        double *gD = (double *)o.g_D + b * ND;
        for (int64_t e = tid; e < ND; e += BS) {
            const int row = (int)(e / nu), j = (int)(e % nu), c = (row / mk) * nu + j;
            gD[e] = -(lam[row] * w[c] + nuf[row] * U[c]);
        }
    }
    if (o.g_w) {
        double uw = 0.0;
        for (int c = tid; c < n; c += BS) uw += w[c] * U[c];
        wred[tid] = tw;
        wred[BS + tid] = sw;
        wred[2 * BS + tid] = uw;
        __syncthreads();
        for (int st = BS / 2; st > 0; st >>= 1) {
            if (tid < st)
                for (int q = 0; q < 3; ++q) wred[q * BS + tid] += wred[q * BS + tid + st];
            __syncthreads();
        }
        if (tid < 3) ((double *)o.g_w)[b * 3 + tid] = tid < 2 ? wred[tid * BS] : -wred[2 * BS];
    }
}

// ---- model and weight tangents ("Model and weight tangents"): what the kModel instantiations of
// mpcqp_tangent_kernel and mpcqp_tangent_stagewise_kernel share. With U and lam held fixed a tangent of A, B, C, D and the
// weights adds a forcing term to the rollout xs (and zs), terms to the cost tangent's per-state vector c, the per-input
// vector g (dq = Psi' c + g) and two terms to dh; all read the trajectories X = rollout(x0, U), Zf = rollout(0, U) and the
// costate pi of the stationarity condition.

// Problem b's model tangents (null = zero; tangent t at t N nx nx, t N nx nu, t N mk nx, t N mk nu, 3 t) and the vectors
// their terms read, in the calling kernel's carve
struct ModelTanVecs {
    const double *dA, *dB, *dC, *dD, *dw;
    const double *X, *Zf, *pi, *U, *lam, *goal, *tgt;  // goal / tgt: null where the q term is off
};

__device__ inline const double *tan_at(const void *p, int64_t stride, int64_t b)
{
    return p ? (const double *)p + b * stride : nullptr;
}

// a P-only term (flagged P, not Q) reads the tangent zs of the forced response
__host__ __device__ inline bool tangent_needs_zs(int flags)
{
    return ((flags & MPCQP_P_STAGE) && !(flags & MPCQP_Q_STAGE)) || ((flags & MPCQP_P_TERMINAL) && !(flags & MPCQP_Q_TERMINAL));
}

// pi = the costate of the stationarity condition, (N + 1) nx: s_k = w_x E_k + C_k' lam_k (k < N), s_N = w_t E_N, then
// pi_k = s_k + A_k' pi_{k+1}, serial over k on nx lanes. E_k = X_k - r_k where the q term is flagged, Zf_k where only the P
// term is, 0 where neither. v.X, v.Zf must be in place (a barrier behind them); ends with a barrier.
template <int BS, class D>
__device__ inline void stationarity_costate(const D &d, const MpcqpOperand &A, const MpcqpOperand &C, int64_t b,
                                            const ModelTanVecs &v, double *pi)
{
    const int tid = threadIdx.x, nx = d.nx, N = d.N, mk = d.mk, R = (N + 1) * nx;
    const bool pt = (d.flags & MPCQP_P_TERMINAL) != 0, ps = (d.flags & MPCQP_P_STAGE) != 0;
    for (int e = tid; e < R; e += BS) {
        const int kk = e / nx, i = e % nx;
        double acc = 0.0;
        if (kk < N) {
            if (ps) acc = d.wx * (v.tgt ? v.X[e] - v.tgt[e] : v.Zf[e]);
            if (const double *Ck = op_step(C, b, kk))
                for (int r = 0; r < mk; ++r) acc += Ck[r * nx + i] * v.lam[kk * mk + r];
        } else if (pt) {
            acc = d.wt * (v.goal ? v.X[e] - v.goal[i] : v.Zf[e]);
        }
        pi[e] = acc;
    }
    __syncthreads();
    for (int kk = N - 1; kk >= 0; --kk) {
        const double *Ak = op_step(A, b, kk);
        for (int i = tid; i < nx; i += BS) {
            double acc = 0.0;
            for (int j = 0; j < nx; ++j) acc += Ak[j * nx + i] * pi[(kk + 1) * nx + j];
            pi[kk * nx + i] += acc;
        }
        __syncthreads();
    }
}

// component i of the forcing term dA_k traj_k + dB_k u_k of tangent t's rollout (traj: X for xs, Zf for zs)
template <class D>
__device__ inline double tangent_forcing(const D &d, const ModelTanVecs &v, const double *traj, int t, int kk, int i)
{
    const int nx = d.nx, nu = d.nu;
    const int64_t tk = (int64_t)t * d.N + kk;
    double acc = 0.0;
    if (v.dA) {
        const double *row = v.dA + (tk * nx + i) * nx;
        for (int l = 0; l < nx; ++l) acc += row[l] * traj[kk * nx + l];
    }
    if (v.dB) {
        const double *row = v.dB + (tk * nx + i) * nu;
        for (int c = 0; c < nu; ++c) acc += row[c] * v.U[kk * nu + c];
    }
    return acc;
}

// c of tangent t at state entry e = kk nx + i: [P] dw E + w dE + dC_k' lam_k + dA_k' pi_{k+1}; xs, zs: the tangent's
// rollouts at e; dtgt, dgoal: the tangent's dtargets / dgoal (null = zero)
template <class D>
__device__ inline double tangent_c(const D &d, const ModelTanVecs &v, int t, int e, double xs, double zs,
                                   const double *dtgt, const double *dgoal)
{
    const int nx = d.nx, N = d.N, mk = d.mk, kk = e / nx, i = e % nx;
    const bool pt = (d.flags & MPCQP_P_TERMINAL) != 0, ps = (d.flags & MPCQP_P_STAGE) != 0;
    const bool qt = (d.flags & MPCQP_Q_TERMINAL) != 0, qs = (d.flags & MPCQP_Q_STAGE) != 0;
    const double *dw = v.dw ? v.dw + 3 * (int64_t)t : nullptr;
    double acc = 0.0;
    if (kk < N) {
        const int64_t tk = (int64_t)t * N + kk;
        if (qs) acc = d.wx * (xs - (dtgt ? dtgt[e] : 0.0));
        else if (ps) acc = d.wx * zs;
        if (ps && dw) acc += dw[1] * (qs ? v.X[e] - v.tgt[e] : v.Zf[e]);
        if (v.dC) {
            const double *dCk = v.dC + tk * mk * nx;
            for (int r = 0; r < mk; ++r) acc += dCk[r * nx + i] * v.lam[kk * mk + r];
        }
        if (v.dA) {
            const double *dAk = v.dA + tk * nx * nx;
            for (int j = 0; j < nx; ++j) acc += dAk[j * nx + i] * v.pi[(kk + 1) * nx + j];
        }
    } else {
        if (qt) acc = d.wt * (xs - (dgoal ? dgoal[i] : 0.0));
        else if (pt) acc = d.wt * zs;
        if (pt && dw) acc += dw[0] * (qt ? v.X[e] - v.goal[i] : v.Zf[e]);
    }
    return acc;
}

// g of tangent t at input entry col = kk nu + j: dw_u u + dB_k' pi_{k+1} + dD_k' lam_k
template <class D>
__device__ inline double tangent_g(const D &d, const ModelTanVecs &v, int t, int col)
{
    const int nx = d.nx, nu = d.nu, mk = d.mk, kk = col / nu, j = col % nu;
    const int64_t tk = (int64_t)t * d.N + kk;
    double acc = v.dw ? v.dw[3 * (int64_t)t + 2] * v.U[col] : 0.0;
    if (v.dB) {
        const double *dBk = v.dB + tk * nx * nu;
        for (int i = 0; i < nx; ++i) acc += dBk[i * nu + j] * v.pi[(kk + 1) * nx + i];
    }
    if (v.dD) {
        const double *dDk = v.dD + tk * mk * nu;
        for (int r = 0; r < mk; ++r) acc += dDk[r * nu + j] * v.lam[kk * mk + r];
    }
    return acc;
}

// what the model tangent takes from dh at `row`: dC_k X_k + dD_k u_k (dh = de - C xs - this)
template <class D>
__device__ inline double tangent_dh(const D &d, const ModelTanVecs &v, int t, int row)
{
    const int nx = d.nx, nu = d.nu, mk = d.mk, kk = row / mk;
    const int64_t tr = (int64_t)t * d.N * mk + row;
    double acc = 0.0;
    if (v.dC)
        for (int i = 0; i < nx; ++i) acc += v.dC[tr * nx + i] * v.X[kk * nx + i];
    if (v.dD)
        for (int j = 0; j < nu; ++j) acc += v.dD[tr * nu + j] * v.U[kk * nu + j];
    return acc;
}

// One workgroup of bs threads per problem, lds_bytes of dynamic LDS (the kernel's limit raised past 48 KiB)
template <class Args>
int launch_per_problem(void (*kern)(Args), const Args &a, int bs, size_t lds_bytes, int64_t batch, hipStream_t st)
{
    if (lds_bytes > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(bs), lds_bytes, st, a);
    return (int)hipGetLastError();
}

}  // namespace mpcqp
#endif
