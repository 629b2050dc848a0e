// mpcqp_adjoint.hip -- vector-Jacobian product of a batch of solved MPC plans (mpcqp_plan_vjp_batch).
//
// One problem per workgroup, float64. The condensed matrices P, G, Phi, Psi come from mpcqp_condense_batch (the C ABI
// runs it into the workspace first); the active set comes from the forward solve's multipliers (lam_i > 0). Per problem:
//   1. gU += Psi' gX                                  (state gradients folded into the input gradient)
//   2. P = L L' (Cholesky), t = L^-1 gU
//   3. A = {i : lam_i > 0}, compacted with a ballot and prefix count (k = |A| <= n, else MPCQP_NOT_PD)
//   4. M_A' = L^-1 G_A'                              (the k active rows solved together with t: one forward sweep)
//   5. S = M_A M_A' = R R', nu = S^-1 M_A t, w = L^-T (t - M_A' nu)
//   6. dL/dq = -w, dL/dh_A = nu; then back through the condensing:
//      y = Psi dL/dq;  g_goal = -w_t y_N;  g_targets_k = -w_x y_k;  g_e = dL/dh;
//      g_x0 = sum_k Phi_k' v_k,  v_k = gX_k + w_x y_k [k < N] + w_t y_N [k = N] - C_k' dL/dh_k
// The carve (L, the k + 1 right-hand sides, the k x k Gram, the vectors) is sized from the actual n, rows at an odd
// stride (as in mpcqp_lds.hip); it lives in LDS when it fits a CU (about n <= 78: 8.3 KB at n = 16, 19 workgroups per CU), else in the workspace.
//
// kModel (mpcqp_plan_vjp_model_batch) appends, after phase 6, the gradients with respect to A, B, C, D and the three cost
// weights ("model and cost gradients"; Y = -y, w, nu and the plan U are held fixed):
//   7. Z = Psi U (forced response), X = Phi x0 + Z; E = X - r_k / X_N - goal where the q term is flagged, else Z
//   8. costates, serial over k and parallel over nx lanes: p from a = v (phase 6's v), pz from the P-only weighted Y
//      terms, s from b = -(w_x E_k + w_t E_N + C_k' lam_k); x_k = a_k + A_k' x_{k+1}
//   9. g_A_k = p_{k+1} X_k' + pz_{k+1} Z_k' + s_{k+1} Y_k',  g_B_k = (p + pz)_{k+1} u_k' + s_{k+1} w_k',
//      g_C_k = -(lam_k Y_k' + nu_k X_k'),  g_D_k = -(lam_k w_k' + nu_k u_k')     (coalesced over (k, i, j))
//  10. g_w = (-Y_N'E_N, -sum_{k<N} Y_k'E_k, -w'U), one block reduction
// The carve grows by X, Z, pz, s ((N + 1) nx each), nu scattered over all m rows and the reduction's 3 x threads.
//
// mpcqp_tangent_kernel (mpcqp_plan_jvp_batch) is the forward-mode counterpart: the same KKT system on the same active set,
// with T tangents (dx0, dgoal, dtargets, de) as right-hand sides ("Forward sensitivities"):
//   1. dq_t = w_t psi_N'(phi_N dx0 - dgoal) + w_x Psi'(Phi dx0 - dtargets) (terms as flagged), dh_t = de - C Phi dx0
//   2. P = L L'; one forward sweep L^-1 over the T + k right-hand sides (-dq_t, then the active rows of G)
//   3. S = M_A M_A' = R R', mu_t = S^-1 (M_A r_t - dh_A,t)        (forward and backward substitution, over tangents)
//   4. dU_t = L^-T (r_t - M_A' mu_t)                               (one backward sweep, over tangents); dX_t = Phi dx0 + Psi dU_t
// Its carve: L (n ld), the T + n right-hand sides ((T + n) ld), S (n ld), mu (T ld), Phi dx0_t (T (N + 1) nx; step 1
// reads it for dq and dh, and dX reuses it), the active row ids.
#include <hip/hip_runtime.h>

#include "mpcqp.h"
#include "mpcqp_internal.h"

namespace mpcqp {
namespace {

struct AdjArgs {
    int nx, nu, N, mk, n, m, flags;
    double wt, wx;
    const double *P, *G, *Phi, *Psi;  // condensed (packed per problem, mpcqp_condense_batch)
    MpcqpOperand C;                   // ineq_state_matrix of the problem (nullable)
    const double *lam, *gU, *gX;      // gX nullable
    const int32_t *status;
    double *g_x0, *g_goal, *g_targets, *g_e;  // all but g_x0 nullable
    int32_t *vjp_status;                       // nullable
    double *carve_ws;                          // per-problem carves when they do not fit LDS (else null)
    int64_t carve;                             // doubles per problem
    // kModel only
    MpcqpOperand A, x0, goal, targets;
    const double *U;                           // the forward plan [batch * n]
    double *g_A, *g_B, *g_C, *g_D, *g_w;       // nullable, packed per problem
};

struct Carve {
    int ld;  // odd row stride of the n-wide matrices
    int64_t L, Z, S, nu, s, y, v, red, idx, total;
    int64_t X, Zf, pz, sc, nuf, wred;  // model: appended after idx (total includes them only when model)
};

__host__ __device__ inline Carve make_carve(int n, int N, int nx, int threads, int m = 0, bool model = false)
{
    Carve c;
    c.ld = n | 1;
    const int64_t mat = (int64_t)n * c.ld;
    c.L = 0;
    c.Z = c.L + mat;                      // row 0: t; rows 1 .. k: the active rows of M_A (n + 1 rows)
    c.S = c.Z + mat + c.ld;               // k x k Gram, stride ld
    c.nu = c.S + mat;                     // n
    c.s = c.nu + n;                       // n: t - M_A' nu, then w in place
    c.y = c.s + n;                        // (N + 1) nx: Psi dL/dq
    c.v = c.y + (int64_t)(N + 1) * nx;    // (N + 1) nx
    c.red = c.v + (int64_t)(N + 1) * nx;  // threads: partial sums of g_x0
    c.idx = c.red + threads;              // n + 1 int32 (active row ids)
    c.total = c.idx + (n + 2) / 2;
    const int64_t R = (int64_t)(N + 1) * nx;
    c.X = c.total;           // (N + 1) nx: Phi x0 + Psi U
    c.Zf = c.X + R;          // (N + 1) nx: Psi U
    c.pz = c.Zf + R;         // (N + 1) nx: costate of Z (p lives in v)
    c.sc = c.pz + R;         // (N + 1) nx: costate of Y
    c.nuf = c.sc + R;        // m: dL/dh over every row
    c.wred = c.nuf + m;      // 3 x threads: partial sums of g_w
    if (model) c.total = c.wred + 3 * threads;
    return c;
}

// In-place lower Cholesky of the nn x nn matrix a (stride ld; only the lower triangle is read or written).
// Uniform result: every thread reads the same pivot after a barrier.
template <int BS>
__device__ bool chol_lower(double *a, int nn, int ld, int tid)
{
    for (int j = 0; j < nn; ++j) {
        __syncthreads();
        const double d = a[j * ld + j];
        if (!(d > 0.0)) return false;
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
__device__ void solve_lower(const double *R, int nn, int ld, double *x, int tid)
{
    for (int j = 0; j < nn; ++j) {
        if (tid == 0) x[j] /= R[j * ld + j];
        __syncthreads();
        for (int i = j + 1 + tid; i < nn; i += BS) x[i] -= R[i * ld + j] * x[j];
        __syncthreads();
    }
}
template <int BS>
__device__ void solve_lower_t(const double *R, int nn, int ld, double *x, int tid)
{
    for (int j = nn - 1; j >= 0; --j) {
        if (tid == 0) x[j] /= R[j * ld + j];
        __syncthreads();
        for (int i = tid; i < j; i += BS) x[i] -= R[j * ld + i] * x[j];
        __syncthreads();
    }
}

// 7 .. 10 of the header, after phase 6 of a solved problem (uniform: every thread of the block gets here). On entry the
// carve holds w (s), the k active entries of dL/dh (nu, rows idx), y = -Y and v = a; g_x0 is written.
template <int BS>
__device__ void model_phase(const AdjArgs &a, const Carve &cv, double *base, const double *Phi, const double *Psi,
                            const double *lam, int k, int64_t b)
{
    const int tid = threadIdx.x;
    const int n = a.n, m = a.m, nx = a.nx, nu = a.nu, N = a.N, mk = a.mk;
    const int R = (N + 1) * nx;
    const double *w = base + cv.s, *nu_a = base + cv.nu, *y = base + cv.y;
    const int *idx = (const int *)(base + cv.idx);
    double *p = base + cv.v, *X = base + cv.X, *Zf = base + cv.Zf, *pz = base + cv.pz, *sc = base + cv.sc;
    double *nuf = base + cv.nuf, *wred = base + cv.wred;
    const double *U = a.U + b * (int64_t)n;
    const bool pt = (a.flags & MPCQP_P_TERMINAL) != 0, ps = (a.flags & MPCQP_P_STAGE) != 0;
    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
    const double *x0 = (const double *)a.x0.ptr + b * a.x0.batch_stride;
    const double *goal = qt ? (const double *)a.goal.ptr + b * a.goal.batch_stride : nullptr;
    const double *tgt = qs ? (const double *)a.targets.ptr + b * a.targets.batch_stride : nullptr;
    const double *Cb = a.C.ptr ? (const double *)a.C.ptr + b * a.C.batch_stride : nullptr;
    const double *Ab = (const double *)a.A.ptr + b * a.A.batch_stride;

    // 7. Z = Psi U, X = Phi x0 + Z; nu over every row (zero off the active set)
    for (int r = tid; r < R; r += BS) {
        const double *pr = Psi + (int64_t)r * n, *fr = Phi + (int64_t)r * nx;
        double z = 0.0, f = 0.0;
        for (int c = 0; c < n; ++c) z += pr[c] * U[c];
        for (int c = 0; c < nx; ++c) f += fr[c] * x0[c];
        Zf[r] = z;
        X[r] = f + z;
    }
    for (int i = tid; i < m; i += BS) nuf[i] = 0.0;
    __syncthreads();
    for (int r = tid; r < k; r += BS) nuf[idx[r]] = nu_a[r];
    // 8. right-hand sides of pz and s (p starts as v), with the partial sums of Y'E for g_w
    double tw = 0.0, sw = 0.0;
    for (int e = tid; e < R; e += BS) {
        const int kk = e / nx, i = e % nx;
        double az = 0.0, bb = 0.0;
        if (kk < N) {
            if (ps) {
                const double E = qs ? X[e] - tgt[e] : Zf[e];
                bb -= a.wx * E;
                sw += y[e] * E;
                if (!qs) az += a.wx * y[e];
            }
            if (Cb) {
                const double *Ck = Cb + kk * a.C.step_stride;
                for (int r = 0; r < mk; ++r) bb -= Ck[r * nx + i] * lam[kk * mk + r];
            }
        } else if (pt) {
            const double E = qt ? X[e] - goal[i] : Zf[e];
            bb -= a.wt * E;
            tw += y[e] * E;
            if (!qt) az += a.wt * y[e];
        }
        pz[e] = az;
        sc[e] = bb;
    }
    __syncthreads();
    // ... then x_k += A_k' x_{k+1} for k = N - 1 .. 0, the three costates side by side
    for (int kk = N - 1; kk >= 0; --kk) {
        const double *Ak = Ab + kk * a.A.step_stride;
        for (int e = tid; e < 3 * nx; e += BS) {
            const int which = e / nx, i = e % nx;
            double *x = which == 0 ? p : (which == 1 ? pz : sc);
            const double *xn = x + (kk + 1) * nx;
            double acc = 0.0;
            for (int j = 0; j < nx; ++j) acc += Ak[j * nx + i] * xn[j];
            x[kk * nx + i] += acc;
        }
        __syncthreads();
    }
    // 9. outer products, packed per problem
    if (a.g_A) {
        const int64_t NA = (int64_t)N * nx * nx;
        double *gA = a.g_A + b * NA;
        for (int64_t e = tid; e < NA; e += BS) {
            const int kk = (int)(e / (nx * nx)), r = (int)(e % (nx * nx)), i = r / nx, j = r % nx;
            const int o = (kk + 1) * nx + i, c = kk * nx + j;
            gA[e] = p[o] * X[c] + pz[o] * Zf[c] - sc[o] * y[c];
        }
    }
    if (a.g_B) {
        const int64_t NB = (int64_t)N * nx * nu;
        double *gB = a.g_B + b * NB;
        for (int64_t e = tid; e < NB; e += BS) {
            const int kk = (int)(e / (nx * nu)), r = (int)(e % (nx * nu)), i = r / nu, j = r % nu;
            const int o = (kk + 1) * nx + i, c = kk * nu + j;
            gB[e] = (p[o] + pz[o]) * U[c] + sc[o] * w[c];
        }
    }
    if (a.g_C) {
        const int64_t NC = (int64_t)m * nx;
        double *gC = a.g_C + b * NC;
        for (int64_t e = tid; e < NC; e += BS) {
            const int row = (int)(e / nx), i = (int)(e % nx), c = (row / mk) * nx + i;
            gC[e] = lam[row] * y[c] - nuf[row] * X[c];
        }
    }
    if (a.g_D) {
        const int64_t ND = (int64_t)m * nu;
        double *gD = a.g_D + b * ND;
        for (int64_t e = tid; e < ND; e += BS) {
            const int row = (int)(e / nu), j = (int)(e % nu), c = (row / mk) * nu + j;
            gD[e] = -(lam[row] * w[c] + nuf[row] * U[c]);
        }
    }
    // 10. g_w = (-Y_N'E_N, -sum Y_k'E_k, -w'U) with Y = -y: one tree reduction of the three partial sums
    if (a.g_w) {
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
        if (tid < 3) a.g_w[b * 3 + tid] = tid < 2 ? wred[tid * BS] : -wred[2 * BS];
    }
}

template <int BS, bool kLds, bool kModel>
__global__ void __launch_bounds__(BS) mpcqp_adjoint_kernel(const AdjArgs a)
{
    extern __shared__ double lds_carve[];
    __shared__ int s_k;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int n = a.n, m = a.m, nx = a.nx, N = a.N, mk = a.mk;
    const int R = (N + 1) * nx;  // rows of Phi / Psi (blocks 0 .. N)
    const Carve cv = make_carve(n, N, nx, BS, m, kModel);
    const int ld = cv.ld;
    double *base = kLds ? lds_carve : a.carve_ws + b * a.carve;
    double *L = base + cv.L, *Z = base + cv.Z, *S = base + cv.S, *nu = base + cv.nu, *s = base + cv.s;
    double *y = base + cv.y, *v = base + cv.v, *red = base + cv.red;
    int *idx = (int *)(base + cv.idx);

    double *gx0 = a.g_x0 + b * nx;
    double *ggoal = a.g_goal ? a.g_goal + b * nx : nullptr;
    double *gtgt = a.g_targets ? a.g_targets + b * (int64_t)N * nx : nullptr;
    double *ge = a.g_e ? a.g_e + b * (int64_t)m : nullptr;
    const double *P = a.P + b * (int64_t)n * n;
    const double *G = a.G ? a.G + b * (int64_t)m * n : nullptr;
    const double *Phi = a.Phi + b * (int64_t)R * nx;
    const double *Psi = a.Psi + b * (int64_t)R * n;
    const double *lam = a.lam + b * (int64_t)m;
    const double *gU = a.gU + b * (int64_t)n;
    const double *gX = a.gX ? a.gX + b * (int64_t)R : nullptr;

    int verdict = a.status[b];
    if (verdict == 0) {
        // 1. lower triangle of P; Z row 0 = gU + Psi' gX; 3. active rows (wave 0: ballot + prefix count, ids ascending)
        for (int e = tid; e < n * n; e += BS) {
            const int i = e / n, j = e % n;
            if (j <= i) L[i * ld + j] = P[e];
        }
        for (int i = tid; i < n; i += BS) {
            double acc = gU[i];
            if (gX)
                for (int r = 0; r < R; ++r) acc += Psi[(int64_t)r * n + i] * gX[r];
            Z[i] = acc;
        }
        if (tid < 64) {
            int count = 0;
            for (int i0 = 0; i0 < m; i0 += 64) {
                const int i = i0 + tid;
                const bool act = i < m && lam[i] > 0.0;
                const unsigned long long mask = __ballot(act);
                const int pre = __popcll(mask & ((1ull << tid) - 1ull));
                if (act && count + pre < n) idx[count + pre] = i;
                count += __popcll(mask);
            }
            if (tid == 0) s_k = count;
        }
        __syncthreads();
        const int k = s_k;
        if (k > n) {
            verdict = MPCQP_NOT_PD;  // more active rows than variables: the forward's multipliers are not a vertex's
        } else {
            // 4. G_A rows into Z rows 1 .. k, then one forward sweep L^-1 over all k + 1 right-hand sides
            for (int e = tid; e < k * n; e += BS) {
                const int r = e / n, j = e % n;
                Z[(r + 1) * ld + j] = G[(int64_t)idx[r] * n + j];
            }
            if (!chol_lower<BS>(L, n, ld, tid)) {
                verdict = MPCQP_NOT_PD;
            } else {
                const int nr = k + 1;
                for (int j = 0; j < n; ++j) {
                    const double inv = 1.0 / L[j * ld + j];
                    for (int r = tid; r < nr; r += BS) Z[r * ld + j] *= inv;
                    __syncthreads();
                    const int w = n - j - 1;
                    for (int e = tid; e < nr * w; e += BS) {
                        const int r = e / w, i = j + 1 + e % w;
                        Z[r * ld + i] -= L[i * ld + j] * Z[r * ld + j];
                    }
                    __syncthreads();
                }
                // 5. Gram S = M_A M_A' (lower) and nu = M_A t
                for (int e = tid; e < k * k; e += BS) {
                    const int i = e / k, j = e % k;
                    if (j <= i) {
                        const double *zi = Z + (i + 1) * ld, *zj = Z + (j + 1) * ld;
                        double acc = 0.0;
                        for (int c = 0; c < n; ++c) acc += zi[c] * zj[c];
                        S[i * ld + j] = acc;
                    }
                }
                for (int i = tid; i < k; i += BS) {
                    const double *zi = Z + (i + 1) * ld;
                    double acc = 0.0;
                    for (int c = 0; c < n; ++c) acc += zi[c] * Z[c];
                    nu[i] = acc;
                }
                if (!chol_lower<BS>(S, k, ld, tid)) {
                    verdict = MPCQP_NOT_PD;
                } else {
                    solve_lower<BS>(S, k, ld, nu, tid);
                    solve_lower_t<BS>(S, k, ld, nu, tid);
                    // w = L^-T (t - M_A' nu)
                    for (int j = tid; j < n; j += BS) {
                        double acc = Z[j];
                        for (int r = 0; r < k; ++r) acc -= Z[(r + 1) * ld + j] * nu[r];
                        s[j] = acc;
                    }
                    __syncthreads();
                    solve_lower_t<BS>(L, n, ld, s, tid);
                    // 6. y = Psi dL/dq = -Psi w
                    for (int r = tid; r < R; r += BS) {
                        const double *pr = Psi + (int64_t)r * n;
                        double acc = 0.0;
                        for (int c = 0; c < n; ++c) acc += pr[c] * s[c];
                        y[r] = -acc;
                    }
                    __syncthreads();
                    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
                    const double *Cb = a.C.ptr ? (const double *)a.C.ptr + b * a.C.batch_stride : nullptr;
                    for (int e = tid; e < R; e += BS) {
                        const int kk = e / nx, j = e % nx;
                        double acc = gX ? gX[e] : 0.0;
                        if (qs && kk < N) acc += a.wx * y[e];
                        if (qt && kk == N) acc += a.wt * y[e];
                        if (Cb && kk < N) {
                            const double *Ck = Cb + kk * a.C.step_stride;
                            for (int r = 0; r < k; ++r) {
                                const int row = idx[r];
                                if (row / mk == kk) acc -= Ck[(row % mk) * nx + j] * nu[r];
                            }
                        }
                        v[e] = acc;
                        if (ggoal && kk == N) ggoal[j] = qt ? -a.wt * y[e] : 0.0;
                        if (gtgt && kk < N) gtgt[e] = qs ? -a.wx * y[e] : 0.0;
                    }
                    if (ge) {
                        for (int i = tid; i < m; i += BS) {
                            // idx is ascending: binary search for row i among the k active ones
                            int lo = 0, hi = k;
                            while (lo < hi) {
                                const int mid = (lo + hi) >> 1;
                                if (idx[mid] < i) lo = mid + 1; else hi = mid;
                            }
                            ge[i] = (lo < k && idx[lo] == i) ? nu[lo] : 0.0;
                        }
                    }
                    __syncthreads();
                    // g_x0 = sum_k Phi_k' v_k: lanes split the (N + 1) nx rows, one partial per lane, then a column sum
                    if (nx <= BS) {
                        const int nsl = BS / nx;
                        if (tid < nsl * nx) {
                            const int c = tid % nx, sl = tid / nx;
                            double acc = 0.0;
                            for (int r = sl; r < R; r += nsl) acc += Phi[(int64_t)r * nx + c] * v[r];
                            red[tid] = acc;
                        }
                        __syncthreads();
                        if (tid < nx) {
                            double acc = 0.0;
                            for (int sl = 0; sl < nsl; ++sl) acc += red[sl * nx + tid];
                            gx0[tid] = acc;
                        }
                    } else {
                        for (int c = tid; c < nx; c += BS) {
                            double acc = 0.0;
                            for (int r = 0; r < R; ++r) acc += Phi[(int64_t)r * nx + c] * v[r];
                            gx0[c] = acc;
                        }
                    }
                    if constexpr (kModel) model_phase<BS>(a, cv, base, Phi, Psi, lam, k, b);
                }
            }
        }
    }
    if (verdict != 0) {  // (uniform: every thread took the same branches) unsolved or degenerate: all-zero gradients
        for (int j = tid; j < nx; j += BS) gx0[j] = 0.0;
        if (ggoal)
            for (int j = tid; j < nx; j += BS) ggoal[j] = 0.0;
        if (gtgt)
            for (int j = tid; j < N * nx; j += BS) gtgt[j] = 0.0;
        if (ge)
            for (int j = tid; j < m; j += BS) ge[j] = 0.0;
        if constexpr (kModel) {
            const int64_t NA = (int64_t)N * nx * nx, NB = (int64_t)N * nx * a.nu, NC = (int64_t)m * nx,
                          ND = (int64_t)m * a.nu;
            if (a.g_A)
                for (int64_t j = tid; j < NA; j += BS) a.g_A[b * NA + j] = 0.0;
            if (a.g_B)
                for (int64_t j = tid; j < NB; j += BS) a.g_B[b * NB + j] = 0.0;
            if (a.g_C)
                for (int64_t j = tid; j < NC; j += BS) a.g_C[b * NC + j] = 0.0;
            if (a.g_D)
                for (int64_t j = tid; j < ND; j += BS) a.g_D[b * ND + j] = 0.0;
            if (a.g_w && tid < 3) a.g_w[b * 3 + tid] = 0.0;
        }
    }
    if (a.vjp_status && tid == 0) a.vjp_status[b] = verdict;
}

// 64 lanes for n <= 32 (config 2: n = 16, several workgroups per CU); 256 above
inline int adjoint_threads(int n) { return n <= 32 ? 64 : 256; }

template <int BS, bool kModel>
int launch_bs(const AdjArgs &a, bool lds, size_t lds_bytes, int64_t batch, hipStream_t st)
{
    if (lds) {
        auto kern = mpcqp_adjoint_kernel<BS, true, kModel>;
        if (lds_bytes > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(BS), lds_bytes, st, a);
    } else {
        hipLaunchKernelGGL((mpcqp_adjoint_kernel<BS, false, kModel>), dim3((unsigned)batch), dim3(BS), 0, st, a);
    }
    return (int)hipGetLastError();
}

struct TanArgs {
    int nx, nu, N, mk, n, m, flags, T;
    double wt, wx;
    const double *P, *G, *Phi, *Psi;  // condensed (packed per problem, mpcqp_condense_batch)
    MpcqpOperand C;                   // ineq_state_matrix of the problem (nullable)
    const double *lam;                // nullable when m = 0
    const int32_t *status;
    const double *dx0, *dgoal, *dtgt, *de;  // nullable (a zero tangent); tangent t of a problem at t nx / t nx / t N nx / t m
    int64_t sx0, sgoal, stgt, se;           // elements between problems (0: shared)
    double *dU, *dX;                        // [batch][T][n], [batch][T][(N + 1) nx] (dX nullable)
    int32_t *jvp_status;                    // nullable
    double *carve_ws;                       // per-problem carves when they do not fit LDS (else null)
    int64_t carve;                          // doubles per problem
};

struct TanCarve {
    int ld;
    int64_t L, Z, S, mu, x, idx, total;
};

__host__ __device__ inline TanCarve make_tan_carve(int n, int T, int R)
{
    TanCarve c;
    c.ld = n | 1;
    c.L = 0;
    c.Z = c.L + (int64_t)n * c.ld;        // rows 0 .. T-1: the tangents' right-hand sides; T .. T+k-1: the active rows
    c.S = c.Z + (int64_t)(T + n) * c.ld;  // k x k Gram, stride ld
    c.mu = c.S + (int64_t)n * c.ld;       // T rows of k: dh_A, then mu
    c.x = c.mu + (int64_t)T * c.ld;       // T rows of R = (N + 1) nx: Phi dx0_t
    c.idx = c.x + (int64_t)T * R;         // n + 1 int32 (active row ids)
    c.total = c.idx + (n + 2) / 2;
    return c;
}

template <int BS, bool kLds>
__global__ void __launch_bounds__(BS) mpcqp_tangent_kernel(const TanArgs a)
{
    extern __shared__ double lds_carve[];
    __shared__ int s_k;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int n = a.n, m = a.m, nx = a.nx, N = a.N, mk = a.mk, T = a.T;
    const int R = (N + 1) * nx;
    const TanCarve cv = make_tan_carve(n, T, R);
    const int ld = cv.ld;
    double *base = kLds ? lds_carve : a.carve_ws + b * a.carve;
    double *L = base + cv.L, *Z = base + cv.Z, *S = base + cv.S, *mu = base + cv.mu, *xs = base + cv.x;
    int *idx = (int *)(base + cv.idx);

    const double *P = a.P + b * (int64_t)n * n;
    const double *G = a.G ? a.G + b * (int64_t)m * n : nullptr;
    const double *Phi = a.Phi + b * (int64_t)R * nx;
    const double *Psi = a.Psi + b * (int64_t)R * n;
    const double *lam = a.lam ? a.lam + b * (int64_t)m : nullptr;
    const double *dx0 = a.dx0 ? a.dx0 + b * a.sx0 : nullptr;
    const double *dgoal = a.dgoal ? a.dgoal + b * a.sgoal : nullptr;
    const double *dtgt = a.dtgt ? a.dtgt + b * a.stgt : nullptr;
    const double *de = a.de ? a.de + b * a.se : nullptr;
    double *dU = a.dU + b * (int64_t)T * n;
    double *dX = a.dX ? a.dX + b * (int64_t)T * R : nullptr;
    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
    const double *Cb = a.C.ptr ? (const double *)a.C.ptr + b * a.C.batch_stride : nullptr;

    int verdict = a.status[b];
    if (verdict == 0) {
        // lower triangle of P; active rows (wave 0: ballot + prefix count, ids ascending), as mpcqp_adjoint_kernel
        for (int e = tid; e < n * n; e += BS) {
            const int i = e / n, j = e % n;
            if (j <= i) L[i * ld + j] = P[e];
        }
        if (tid < 64) {
            int count = 0;
            for (int i0 = 0; i0 < m; i0 += 64) {
                const int i = i0 + tid;
                const bool act = i < m && lam[i] > 0.0;
                const unsigned long long mask = __ballot(act);
                const int pre = __popcll(mask & ((1ull << tid) - 1ull));
                if (act && count + pre < n) idx[count + pre] = i;
                count += __popcll(mask);
            }
            if (tid == 0) s_k = count;
        }
        __syncthreads();
        const int k = s_k;
        if (k > n) {
            verdict = MPCQP_NOT_PD;
        } else {
            // 1. xs_t = Phi dx0_t; Z rows 0 .. T-1 = -dq_t; rows T .. T+k-1 = G_A; mu rows = dh_A,t
            if (dx0) {
                for (int e = tid; e < T * R; e += BS) {
                    const int t = e / R, r = e % R;
                    const double *fr = Phi + (int64_t)r * nx, *x0t = dx0 + (int64_t)t * nx;
                    double acc = 0.0;
                    for (int j = 0; j < nx; ++j) acc += fr[j] * x0t[j];
                    xs[e] = acc;
                }
                __syncthreads();
            }
            for (int e = tid; e < T * n; e += BS) {
                const int t = e / n, c = e % n;
                const double *xt = dx0 ? xs + (int64_t)t * R : nullptr;
                double acc = 0.0;
                if (qs && (xt || dtgt)) {
                    const double *tg = dtgt ? dtgt + (int64_t)t * N * nx : nullptr;
                    double s = 0.0;
                    for (int r = 0; r < N * nx; ++r)
                        s += Psi[(int64_t)r * n + c] * ((xt ? xt[r] : 0.0) - (tg ? tg[r] : 0.0));
                    acc += a.wx * s;
                }
                if (qt && (xt || dgoal)) {
                    const double *gl = dgoal ? dgoal + (int64_t)t * nx : nullptr;
                    double s = 0.0;
                    for (int i = 0; i < nx; ++i) {
                        const int r = N * nx + i;
                        s += Psi[(int64_t)r * n + c] * ((xt ? xt[r] : 0.0) - (gl ? gl[i] : 0.0));
                    }
                    acc += a.wt * s;
                }
                Z[t * ld + c] = -acc;
            }
            for (int e = tid; e < k * n; e += BS) {
                const int r = e / n, j = e % n;
                Z[(T + r) * ld + j] = G[(int64_t)idx[r] * n + j];
            }
            for (int e = tid; e < T * k; e += BS) {
                const int t = e / k, r = e % k, row = idx[r], kk = row / mk;
                double h = de ? de[(int64_t)t * m + row] : 0.0;
                if (Cb && dx0) {
                    const double *Ci = Cb + kk * a.C.step_stride + (row % mk) * nx, *xk = xs + (int64_t)t * R + kk * nx;
                    for (int i = 0; i < nx; ++i) h -= Ci[i] * xk[i];
                }
                mu[t * ld + r] = h;
            }
            // 2. P = L L', then one forward sweep L^-1 over all T + k right-hand sides
            if (!chol_lower<BS>(L, n, ld, tid)) {
                verdict = MPCQP_NOT_PD;
            } else {
                const int nr = T + k;
                for (int j = 0; j < n; ++j) {
                    const double inv = 1.0 / L[j * ld + j];
                    for (int r = tid; r < nr; r += BS) Z[r * ld + j] *= inv;
                    __syncthreads();
                    const int w = n - j - 1;
                    for (int e = tid; e < nr * w; e += BS) {
                        const int r = e / w, i = j + 1 + e % w;
                        Z[r * ld + i] -= L[i * ld + j] * Z[r * ld + j];
                    }
                    __syncthreads();
                }
                // 3. Gram S = M_A M_A' (lower); mu_t = M_A r_t - dh_A,t
                for (int e = tid; e < k * k; e += BS) {
                    const int i = e / k, j = e % k;
                    if (j <= i) {
                        const double *zi = Z + (T + i) * ld, *zj = Z + (T + j) * ld;
                        double acc = 0.0;
                        for (int c = 0; c < n; ++c) acc += zi[c] * zj[c];
                        S[i * ld + j] = acc;
                    }
                }
                for (int e = tid; e < T * k; e += BS) {
                    const int t = e / k, i = e % k;
                    const double *zi = Z + (T + i) * ld, *zt = Z + t * ld;
                    double acc = 0.0;
                    for (int c = 0; c < n; ++c) acc += zi[c] * zt[c];
                    mu[t * ld + i] = acc - mu[t * ld + i];
                }
                if (!chol_lower<BS>(S, k, ld, tid)) {
                    verdict = MPCQP_NOT_PD;
                } else {
                    // mu_t = R^-T R^-1 (...), every tangent at once
                    for (int j = 0; j < k; ++j) {
                        const double inv = 1.0 / S[j * ld + j];
                        for (int t = tid; t < T; t += BS) mu[t * ld + j] *= inv;
                        __syncthreads();
                        const int w = k - j - 1;
                        for (int e = tid; e < T * w; e += BS) {
                            const int t = e / w, i = j + 1 + e % w;
                            mu[t * ld + i] -= S[i * ld + j] * mu[t * ld + j];
                        }
                        __syncthreads();
                    }
                    for (int j = k - 1; j >= 0; --j) {
                        const double inv = 1.0 / S[j * ld + j];
                        for (int t = tid; t < T; t += BS) mu[t * ld + j] *= inv;
                        __syncthreads();
                        for (int e = tid; e < T * j; e += BS) {
                            const int t = e / j, i = e % j;
                            mu[t * ld + i] -= S[j * ld + i] * mu[t * ld + j];
                        }
                        __syncthreads();
                    }
                    // 4. r_t - M_A' mu_t in place, then dU_t = L^-T (...), every tangent at once
                    for (int e = tid; e < T * n; e += BS) {
                        const int t = e / n, c = e % n;
                        double acc = Z[t * ld + c];
                        for (int r = 0; r < k; ++r) acc -= Z[(T + r) * ld + c] * mu[t * ld + r];
                        Z[t * ld + c] = acc;
                    }
                    __syncthreads();
                    for (int j = n - 1; j >= 0; --j) {
                        const double inv = 1.0 / L[j * ld + j];
                        for (int t = tid; t < T; t += BS) Z[t * ld + j] *= inv;
                        __syncthreads();
                        for (int e = tid; e < T * j; e += BS) {
                            const int t = e / j, i = e % j;
                            Z[t * ld + i] -= L[j * ld + i] * Z[t * ld + j];
                        }
                        __syncthreads();
                    }
                    for (int e = tid; e < T * n; e += BS) dU[e] = Z[(e / n) * ld + e % n];
                    if (dX) {
                        for (int64_t e = tid; e < (int64_t)T * R; e += BS) {
                            const int t = (int)(e / R), r = (int)(e % R);
                            const double *pr = Psi + (int64_t)r * n, *zt = Z + t * ld;
                            double acc = dx0 ? xs[e] : 0.0;
                            for (int c = 0; c < n; ++c) acc += pr[c] * zt[c];
                            dX[e] = acc;
                        }
                    }
                }
            }
        }
    }
    if (verdict != 0) {  // (uniform) unsolved or degenerate: all-zero tangents
        for (int e = tid; e < T * n; e += BS) dU[e] = 0.0;
        if (dX)
            for (int64_t e = tid; e < (int64_t)T * R; e += BS) dX[e] = 0.0;
    }
    if (a.jvp_status && tid == 0) a.jvp_status[b] = verdict;
}

template <int BS>
int launch_tangent_bs(const TanArgs &a, bool lds, size_t lds_bytes, int64_t batch, hipStream_t st)
{
    if (lds) {
        auto kern = mpcqp_tangent_kernel<BS, true>;
        if (lds_bytes > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
            if (e != hipSuccess) return (int)e;
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(BS), lds_bytes, st, a);
    } else {
        hipLaunchKernelGGL((mpcqp_tangent_kernel<BS, false>), dim3((unsigned)batch), dim3(BS), 0, st, a);
    }
    return (int)hipGetLastError();
}

}  // namespace

size_t adjoint_carve_bytes(int n, int N, int nx, int m, bool model)
{
    return (size_t)make_carve(n, N, nx, adjoint_threads(n), m, model).total * sizeof(double);
}

// (the 64 bytes spare leave room for the kernel's static s_k)
bool adjoint_carve_in_lds(int n, int N, int nx, int m, bool model)
{
    return adjoint_carve_bytes(n, N, nx, m, model) + 64 <= kLdsBytesPerCU;
}

int launch_adjoint(const AdjointLaunch &l, int64_t batch, hipStream_t st)
{
    AdjArgs a;
    a.nx = l.nx;
    a.nu = l.nu;
    a.N = l.N;
    a.mk = l.mk;
    a.n = l.N * l.nu;
    a.m = l.N * l.mk;
    a.flags = l.flags;
    a.wt = l.wt;
    a.wx = l.wx;
    a.P = (const double *)l.P;
    a.G = (const double *)l.G;
    a.Phi = (const double *)l.Phi;
    a.Psi = (const double *)l.Psi;
    a.C = l.C;
    a.lam = (const double *)l.lam;
    a.gU = (const double *)l.gU;
    a.gX = (const double *)l.gX;
    a.status = l.status;
    a.g_x0 = (double *)l.g_x0;
    a.g_goal = (double *)l.g_goal;
    a.g_targets = (double *)l.g_targets;
    a.g_e = (double *)l.g_e;
    a.vjp_status = l.vjp_status;
    a.A = l.A;
    a.x0 = l.x0;
    a.goal = l.goal;
    a.targets = l.targets;
    a.U = (const double *)l.U;
    a.g_A = (double *)l.g_A;
    a.g_B = (double *)l.g_B;
    a.g_C = (double *)l.g_C;
    a.g_D = (double *)l.g_D;
    a.g_w = (double *)l.g_w;
    const bool lds = adjoint_carve_in_lds(a.n, a.N, a.nx, a.m, l.model);
    const size_t bytes = adjoint_carve_bytes(a.n, a.N, a.nx, a.m, l.model);
    a.carve_ws = lds ? nullptr : (double *)l.carve_ws;
    a.carve = (int64_t)(bytes / sizeof(double));
    if (!lds && !a.carve_ws) return MPCQP_EWORKSPACE;
    if (l.model && (!a.U || !a.A.ptr || !a.x0.ptr)) return MPCQP_EINVAL;
    if (adjoint_threads(a.n) == 64)
        return l.model ? launch_bs<64, true>(a, lds, bytes, batch, st) : launch_bs<64, false>(a, lds, bytes, batch, st);
    return l.model ? launch_bs<256, true>(a, lds, bytes, batch, st) : launch_bs<256, false>(a, lds, bytes, batch, st);
}

size_t tangent_carve_bytes(int n, int N, int nx, int ntan)
{
    return (size_t)make_tan_carve(n, ntan, (N + 1) * nx).total * sizeof(double);
}

// (the 64 bytes spare leave room for the kernel's static s_k, as adjoint_carve_in_lds)
bool tangent_carve_in_lds(int n, int N, int nx, int ntan)
{
    return tangent_carve_bytes(n, N, nx, ntan) + 64 <= kLdsBytesPerCU;
}

int launch_tangent(const TangentLaunch &l, int64_t batch, hipStream_t st)
{
    TanArgs a;
    a.nx = l.nx;
    a.nu = l.nu;
    a.N = l.N;
    a.mk = l.mk;
    a.n = l.N * l.nu;
    a.m = l.N * l.mk;
    a.flags = l.flags;
    a.T = l.ntan;
    a.wt = l.wt;
    a.wx = l.wx;
    a.P = (const double *)l.P;
    a.G = (const double *)l.G;
    a.Phi = (const double *)l.Phi;
    a.Psi = (const double *)l.Psi;
    a.C = l.C;
    a.lam = (const double *)l.lam;
    a.status = l.status;
    a.dx0 = (const double *)l.tan.dx0;
    a.dgoal = (const double *)l.tan.dgoal;
    a.dtgt = (const double *)l.tan.dtargets;
    a.de = a.m > 0 ? (const double *)l.tan.de : nullptr;
    a.sx0 = l.tan.dx0_stride;
    a.sgoal = l.tan.dgoal_stride;
    a.stgt = l.tan.dtargets_stride;
    a.se = l.tan.de_stride;
    a.dU = (double *)l.dU;
    a.dX = (double *)l.dX;
    a.jvp_status = l.jvp_status;
    const bool lds = tangent_carve_in_lds(a.n, a.N, a.nx, a.T);
    const size_t bytes = tangent_carve_bytes(a.n, a.N, a.nx, a.T);
    a.carve_ws = lds ? nullptr : (double *)l.carve_ws;
    a.carve = (int64_t)(bytes / sizeof(double));
    if (!lds && !a.carve_ws) return MPCQP_EWORKSPACE;
    if (adjoint_threads(a.n) == 64) return launch_tangent_bs<64>(a, lds, bytes, batch, st);
    return launch_tangent_bs<256>(a, lds, bytes, batch, st);
}

}  // namespace mpcqp
