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
// 8 .. 10 are model_epilogue of mpcqp_adjoint_common.h, which the stage-wise adjoint shares (as the factorisations, sweeps,
// active-row compaction and zero-fill the kernels here are built from).
//
// mpcqp_tangent_kernel (mpcqp_plan_jvp_batch) is the forward-mode counterpart: the same KKT system on the same active set,
// with T tangents (dx0, dgoal, dtargets, de) as right-hand sides ("Forward sensitivities"):
//   1. dq_t = w_t psi_N'(phi_N dx0 - dgoal) + w_x Psi'(Phi dx0 - dtargets) (terms as flagged), dh_t = de - C Phi dx0
//   2. P = L L'; one forward sweep L^-1 over the T + k right-hand sides (-dq_t, then the active rows of G)
//   3. S = M_A M_A' = R R', mu_t = S^-1 (M_A r_t - dh_A,t)        (forward and backward substitution, over tangents)
//   4. dU_t = L^-T (r_t - M_A' mu_t)                               (one backward sweep, over tangents); dX_t = Phi dx0 + Psi dU_t
// Its carve: L (n ld), the T + n right-hand sides ((T + n) ld), S (n ld), mu (T ld), Phi dx0_t (T (N + 1) nx; step 1
// reads it for dq and dh, and dX reuses it), the active row ids.
//
// Its kModel instantiation (mpcqp_plan_jvp_model_batch) takes tangents of A, B, C, D and the weights as well: see the comment
// above the kernel. Its carve grows by X, Z, pi ((N + 1) nx each) and T (N + 1) nx for zs (then c).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mpcqp.h"
#include "mpcqp_adjoint_common.h"

namespace mpcqp {
namespace {

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

template <int BS, bool kLds, bool kModel>
__global__ void __launch_bounds__(BS) mpcqp_adjoint_kernel(const AdjointLaunch a)
{
    extern __shared__ double lds_carve[];
    __shared__ int s_k;
    const CondensedKkt &d = a.kkt;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int n = d.n, m = d.m, nx = d.nx, N = d.N, mk = d.mk;
    const int R = (N + 1) * nx;  // rows of Phi / Psi (blocks 0 .. N)
    const Carve cv = make_carve(n, N, nx, BS, m, kModel);
    const int ld = cv.ld;
    double *base = kLds ? lds_carve : d.carve_ws + b * cv.total;
    double *L = base + cv.L, *Z = base + cv.Z, *S = base + cv.S, *nu = base + cv.nu, *s = base + cv.s;
    double *y = base + cv.y, *v = base + cv.v, *red = base + cv.red;
    int *idx = (int *)(base + cv.idx);

    double *gx0 = (double *)a.out.g_x0 + b * nx;
    double *ggoal = out_at(a.out.g_goal, b * nx);
    double *gtgt = out_at(a.out.g_targets, b * (int64_t)N * nx);
    double *ge = out_at(a.out.g_e, b * (int64_t)m);
    const double *P = d.P + b * (int64_t)n * n;
    const double *G = d.G ? d.G + b * (int64_t)m * n : nullptr;
    const double *Phi = d.Phi + b * (int64_t)R * nx;
    const double *Psi = d.Psi + b * (int64_t)R * n;
    const double *lam = d.lam + b * (int64_t)m;
    const double *gU = a.gU + b * (int64_t)n;
    const double *gX = a.gX ? a.gX + b * (int64_t)R : nullptr;

    int verdict = d.status[b];
    if (verdict == 0) {
        // 1. lower triangle of P; Z row 0 = gU + Psi' gX; 3. active rows (ids ascending)
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
        const int k = active_rows(lam, m, n, idx, &s_k);
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
                sweep_lower<BS>(L, n, ld, Z, k + 1, tid);
                // 5. Gram S = M_A M_A' (lower) and nu = M_A t
                gram_lower<BS>(Z, 1, k, n, ld, S, tid);
                for (int i = tid; i < k; i += BS) {
                    const double *zi = Z + (i + 1) * ld;
                    double acc = 0.0;
                    for (int c = 0; c < n; ++c) acc += zi[c] * Z[c];
                    nu[i] = acc;
                }
                if (!chol_lower<BS, true>(S, k, ld, tid, gram_pivot_floor(n, k))) {
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
                    const bool qt = (d.flags & MPCQP_Q_TERMINAL) != 0, qs = (d.flags & MPCQP_Q_STAGE) != 0;
                    const double *Cb = d.C.ptr ? (const double *)d.C.ptr + b * d.C.batch_stride : nullptr;
                    for (int e = tid; e < R; e += BS) {
                        const int kk = e / nx, j = e % nx;
                        double acc = gX ? gX[e] : 0.0;
                        if (qs && kk < N) acc += d.wx * y[e];
                        if (qt && kk == N) acc += d.wt * y[e];
                        if (Cb && kk < N) {
                            const double *Ck = Cb + kk * d.C.step_stride;
                            for (int r = 0; r < k; ++r) {
                                const int row = idx[r];
                                if (row / mk == kk) acc -= Ck[(row % mk) * nx + j] * nu[r];
                            }
                        }
                        v[e] = acc;
                        if (ggoal && kk == N) ggoal[j] = qt ? -d.wt * y[e] : 0.0;
                        if (gtgt && kk < N) gtgt[e] = qs ? -d.wx * y[e] : 0.0;
                    }
                    if (ge) {
                        for (int i = tid; i < m; i += BS) {
                            const int lo = lower_bound(idx, k, i);
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
                    if constexpr (kModel) {
                        // 7. Z = Psi U, X = Phi x0 + Z; then 8 .. 10 with y = -Y and p starting as v
                        const double *U = a.U + b * (int64_t)n;
                        const double *x0 = (const double *)a.x0.ptr + b * a.x0.batch_stride;
                        double *X = base + cv.X, *Zf = base + cv.Zf;
                        for (int r = tid; r < R; r += BS) {
                            const double *pr = Psi + (int64_t)r * n, *fr = Phi + (int64_t)r * nx;
                            double z = 0.0, f = 0.0;
                            for (int c = 0; c < n; ++c) z += pr[c] * U[c];
                            for (int c = 0; c < nx; ++c) f += fr[c] * x0[c];
                            Zf[r] = z;
                            X[r] = f + z;
                        }
                        const ModelVecs mv{lam, U, s, y,
                                           qt ? (const double *)a.goal.ptr + b * a.goal.batch_stride : nullptr,
                                           qs ? (const double *)a.targets.ptr + b * a.targets.batch_stride : nullptr,
                                           nu, idx, k, v, X, Zf, base + cv.pz, base + cv.sc, base + cv.nuf, base + cv.wred};
                        model_epilogue<BS, true, true>(d, a.A, d.C, a.out, b, mv);
                    }
                }
            }
        }
    }
    if (verdict != 0) {  // (uniform: every thread took the same branches) unsolved or degenerate: all-zero gradients
        zero_outputs<BS>(tid, gx0, nx, ggoal, nx, gtgt, (int64_t)N * nx, ge, m);
        if constexpr (kModel) zero_model_outputs<BS>(a.out, nx, d.nu, N, m, b, tid);
    }
    if (a.vjp_status && tid == 0) a.vjp_status[b] = verdict;
}

// 64 lanes for n <= 32 (config 2: n = 16, several workgroups per CU); 256 above
inline int adjoint_threads(int n) { return n <= 32 ? 64 : 256; }

template <int BS, bool kModel>
int launch_adjoint_bs(const AdjointLaunch &a, bool lds, size_t lds_bytes, int64_t batch, hipStream_t st)
{
    if (lds) return launch_per_problem(mpcqp_adjoint_kernel<BS, true, kModel>, a, BS, lds_bytes, batch, st);
    return launch_per_problem(mpcqp_adjoint_kernel<BS, false, kModel>, a, BS, 0, batch, st);
}

struct TanCarve {
    int ld;
    int64_t L, Z, S, mu, x, idx, total;
    int64_t X, Zf, pi, zs;  // model: appended after idx (total includes them only when model)
};

__host__ __device__ inline TanCarve make_tan_carve(int n, int T, int R, bool model = false)
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
    c.X = c.total;      // R: Phi x0 + Psi U
    c.Zf = c.X + R;     // R: Psi U
    c.pi = c.Zf + R;    // R: the costate of the stationarity condition
    c.zs = c.pi + R;    // T rows of R: the tangents zs of Zf, then c in place
    if (model) c.total = c.zs + (int64_t)T * R;
    return c;
}

// kModel (mpcqp_plan_jvp_model_batch; DESIGN.md section 9, "Model and weight tangents"): tangents of A, B, C, D and the
// weights as well. Before step 1: Z = Psi U and X = Phi x0 + Z in one pass, the costate pi (stationarity_costate), then xs
// (and zs where a P-only term reads it) of all tangents side by side by the recursion with its forcing term, one barrier
// per step, in place of the Phi dx0 pass; c overwrites zs entry by entry. Step 1 then has Z rows -(Psi' c + g) and the two
// more terms of dh (tangent_c, tangent_g, tangent_dh of mpcqp_adjoint_common.h); the rest is the kernel as it was.
template <int BS, bool kLds, bool kModel>
__global__ void __launch_bounds__(BS)
mpcqp_tangent_kernel(const typename std::conditional<kModel, TangentModelLaunch, TangentLaunch>::type a)
{
    extern __shared__ double lds_carve[];
    __shared__ int s_k;
    const CondensedKkt &d = a.kkt;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int n = d.n, m = d.m, nx = d.nx, N = d.N, mk = d.mk, T = a.ntan;
    const int R = (N + 1) * nx;
    const TanCarve cv = make_tan_carve(n, T, R, kModel);
    const int ld = cv.ld;
    double *base = kLds ? lds_carve : d.carve_ws + b * cv.total;
    double *L = base + cv.L, *Z = base + cv.Z, *S = base + cv.S, *mu = base + cv.mu, *xs = base + cv.x;
    ModelTanVecs mv{};
    int *idx = (int *)(base + cv.idx);

    const double *P = d.P + b * (int64_t)n * n;
    const double *G = d.G ? d.G + b * (int64_t)m * n : nullptr;
    const double *Phi = d.Phi + b * (int64_t)R * nx;
    const double *Psi = d.Psi + b * (int64_t)R * n;
    const double *lam = d.lam ? d.lam + b * (int64_t)m : nullptr;
    // tangent t of a problem at t nx / t nx / t N nx / t m; a null one is zero, a zero stride shares it
    const double *dx0 = a.tan.dx0 ? (const double *)a.tan.dx0 + b * a.tan.dx0_stride : nullptr;
    const double *dgoal = a.tan.dgoal ? (const double *)a.tan.dgoal + b * a.tan.dgoal_stride : nullptr;
    const double *dtgt = a.tan.dtargets ? (const double *)a.tan.dtargets + b * a.tan.dtargets_stride : nullptr;
    const double *de = a.tan.de ? (const double *)a.tan.de + b * a.tan.de_stride : nullptr;
    double *dU = a.dU + b * (int64_t)T * n;
    double *dX = a.dX ? a.dX + b * (int64_t)T * R : nullptr;
    const bool qt = (d.flags & MPCQP_Q_TERMINAL) != 0, qs = (d.flags & MPCQP_Q_STAGE) != 0;
    const double *Cb = d.C.ptr ? (const double *)d.C.ptr + b * d.C.batch_stride : nullptr;

    int verdict = d.status[b];
    if (verdict == 0) {
        // lower triangle of P; active rows (ids ascending), as mpcqp_adjoint_kernel
        for (int e = tid; e < n * n; e += BS) {
            const int i = e / n, j = e % n;
            if (j <= i) L[i * ld + j] = P[e];
        }
        const int k = active_rows(lam, m, n, idx, &s_k);
        if (k > n) {
            verdict = MPCQP_NOT_PD;
        } else {
            // 1. xs_t = Phi dx0_t; Z rows 0 .. T-1 = -dq_t; rows T .. T+k-1 = G_A; mu rows = dh_A,t
            if constexpr (kModel) {
                const double *U = a.U + b * (int64_t)n;
                const double *x0 = (const double *)a.x0.ptr + b * a.x0.batch_stride;
                double *X = base + cv.X, *Zf = base + cv.Zf, *pi = base + cv.pi, *zs = base + cv.zs;
                for (int r = tid; r < R; r += BS) {
                    const double *pr = Psi + (int64_t)r * n, *fr = Phi + (int64_t)r * nx;
                    double z = 0.0, f = 0.0;
                    for (int c = 0; c < n; ++c) z += pr[c] * U[c];
                    for (int c = 0; c < nx; ++c) f += fr[c] * x0[c];
                    Zf[r] = z;
                    X[r] = f + z;
                }
                mv = ModelTanVecs{tan_at(a.mtan.dA, a.mtan.dA_stride, b), tan_at(a.mtan.dB, a.mtan.dB_stride, b),
                                  tan_at(a.mtan.dC, a.mtan.dC_stride, b), tan_at(a.mtan.dD, a.mtan.dD_stride, b),
                                  tan_at(a.mtan.dw, a.mtan.dw_stride, b), X, Zf, pi, U, lam,
                                  qt ? (const double *)a.goal.ptr + b * a.goal.batch_stride : nullptr,
                                  qs ? (const double *)a.targets.ptr + b * a.targets.batch_stride : nullptr};
                __syncthreads();
                stationarity_costate<BS>(d, a.A, d.C, b, mv, pi);
                // xs (which = 0) and zs (which = 1) of every tangent, one barrier per step
                const int nw = tangent_needs_zs(d.flags) ? 2 : 1;
                for (int e = tid; e < nw * T * nx; e += BS) {
                    const int which = e / (T * nx), t = (e / nx) % T, i = e % nx;
                    (which ? zs : xs)[(int64_t)t * R + i] = (!which && dx0) ? dx0[(int64_t)t * nx + i] : 0.0;
                }
                __syncthreads();
                for (int kk = 0; kk < N; ++kk) {
                    const double *Ak = op_step(a.A, b, kk);
                    for (int e = tid; e < nw * T * nx; e += BS) {
                        const int which = e / (T * nx), t = (e / nx) % T, i = e % nx;
                        double *x = (which ? zs : xs) + (int64_t)t * R;
                        double acc = tangent_forcing(d, mv, which ? Zf : X, t, kk, i);
                        for (int l = 0; l < nx; ++l) acc += Ak[i * nx + l] * x[kk * nx + l];
                        x[(kk + 1) * nx + i] = acc;
                    }
                    __syncthreads();
                }
                for (int e = tid; e < T * R; e += BS) {
                    const int t = e / R, r = e % R;
                    zs[e] = tangent_c(d, mv, t, r, xs[e], nw == 2 ? zs[e] : 0.0, dtgt ? dtgt + (int64_t)t * N * nx : nullptr,
                                      dgoal ? dgoal + (int64_t)t * nx : nullptr);
                }
                __syncthreads();
                for (int e = tid; e < T * n; e += BS) {
                    const int t = e / n, c = e % n;
                    const double *ct = zs + (int64_t)t * R;
                    double acc = tangent_g(d, mv, t, c);
                    for (int r = 0; r < R; ++r) acc += Psi[(int64_t)r * n + c] * ct[r];
                    Z[t * ld + c] = -acc;
                }
            } else {
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
                        acc += d.wx * s;
                    }
                    if (qt && (xt || dgoal)) {
                        const double *gl = dgoal ? dgoal + (int64_t)t * nx : nullptr;
                        double s = 0.0;
                        for (int i = 0; i < nx; ++i) {
                            const int r = N * nx + i;
                            s += Psi[(int64_t)r * n + c] * ((xt ? xt[r] : 0.0) - (gl ? gl[i] : 0.0));
                        }
                        acc += d.wt * s;
                    }
                    Z[t * ld + c] = -acc;
                }
            }
            for (int e = tid; e < k * n; e += BS) {
                const int r = e / n, j = e % n;
                Z[(T + r) * ld + j] = G[(int64_t)idx[r] * n + j];
            }
            for (int e = tid; e < T * k; e += BS) {
                const int t = e / k, r = e % k, row = idx[r], kk = row / mk;
                double h = de ? de[(int64_t)t * m + row] : 0.0;
                if (Cb && (kModel || dx0)) {
                    const double *Ci = Cb + kk * d.C.step_stride + (row % mk) * nx, *xk = xs + (int64_t)t * R + kk * nx;
                    for (int i = 0; i < nx; ++i) h -= Ci[i] * xk[i];
                }
                if constexpr (kModel) h -= tangent_dh(d, mv, t, row);
                mu[t * ld + r] = h;
            }
            // 2. P = L L', then one forward sweep L^-1 over all T + k right-hand sides
            if (!chol_lower<BS>(L, n, ld, tid)) {
                verdict = MPCQP_NOT_PD;
            } else {
                sweep_lower<BS>(L, n, ld, Z, T + k, tid);
                // 3. Gram S = M_A M_A' (lower); mu_t = M_A r_t - dh_A,t
                gram_lower<BS>(Z, T, k, n, ld, S, tid);
                for (int e = tid; e < T * k; e += BS) {
                    const int t = e / k, i = e % k;
                    const double *zi = Z + (T + i) * ld, *zt = Z + t * ld;
                    double acc = 0.0;
                    for (int c = 0; c < n; ++c) acc += zi[c] * zt[c];
                    mu[t * ld + i] = acc - mu[t * ld + i];
                }
                if (!chol_lower<BS, true>(S, k, ld, tid, gram_pivot_floor(n, k))) {
                    verdict = MPCQP_NOT_PD;
                } else {
                    // mu_t = R^-T R^-1 (...), every tangent at once
                    sweep_lower<BS>(S, k, ld, mu, T, tid);
                    sweep_lower_t<BS>(S, k, ld, mu, T, tid);
                    // 4. r_t - M_A' mu_t in place, then dU_t = L^-T (...), every tangent at once
                    for (int e = tid; e < T * n; e += BS) {
                        const int t = e / n, c = e % n;
                        double acc = Z[t * ld + c];
                        for (int r = 0; r < k; ++r) acc -= Z[(T + r) * ld + c] * mu[t * ld + r];
                        Z[t * ld + c] = acc;
                    }
                    __syncthreads();
                    sweep_lower_t<BS>(L, n, ld, Z, T, tid);
                    for (int e = tid; e < T * n; e += BS) dU[e] = Z[(e / n) * ld + e % n];
                    if (dX) {
                        for (int64_t e = tid; e < (int64_t)T * R; e += BS) {
                            const int t = (int)(e / R), r = (int)(e % R);
                            const double *pr = Psi + (int64_t)r * n, *zt = Z + t * ld;
                            double acc = (kModel || dx0) ? xs[e] : 0.0;
                            for (int c = 0; c < n; ++c) acc += pr[c] * zt[c];
                            dX[e] = acc;
                        }
                    }
                }
            }
        }
    }
    if (verdict != 0)  // (uniform) unsolved or degenerate: all-zero tangents
        zero_outputs<BS>(tid, dU, (int64_t)T * n, dX, (int64_t)T * R);
    if (a.jvp_status && tid == 0) a.jvp_status[b] = verdict;
}

template <int BS>
int launch_tangent_bs(const TangentLaunch &a, bool lds, size_t lds_bytes, int64_t batch, hipStream_t st)
{
    if (lds) return launch_per_problem(mpcqp_tangent_kernel<BS, true, false>, a, BS, lds_bytes, batch, st);
    return launch_per_problem(mpcqp_tangent_kernel<BS, false, false>, a, BS, 0, batch, st);
}
template <int BS>
int launch_tangent_model_bs(const TangentModelLaunch &a, bool lds, size_t lds_bytes, int64_t batch, hipStream_t st)
{
    if (lds) return launch_per_problem(mpcqp_tangent_kernel<BS, true, true>, a, BS, lds_bytes, batch, st);
    return launch_per_problem(mpcqp_tangent_kernel<BS, false, true>, a, BS, 0, batch, st);
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
    const CondensedKkt &d = l.kkt;
    const bool lds = adjoint_carve_in_lds(d.n, d.N, d.nx, d.m, l.model);
    const size_t bytes = adjoint_carve_bytes(d.n, d.N, d.nx, d.m, l.model);
    if (!lds && !d.carve_ws) return MPCQP_EWORKSPACE;
    if (l.model && (!l.U || !l.A.ptr || !l.x0.ptr)) return MPCQP_EINVAL;
    if (adjoint_threads(d.n) == 64)
        return l.model ? launch_adjoint_bs<64, true>(l, lds, bytes, batch, st) : launch_adjoint_bs<64, false>(l, lds, bytes, batch, st);
    return l.model ? launch_adjoint_bs<256, true>(l, lds, bytes, batch, st) : launch_adjoint_bs<256, false>(l, lds, bytes, batch, st);
}

size_t tangent_carve_bytes(int n, int N, int nx, int ntan, bool model)
{
    return (size_t)make_tan_carve(n, ntan, (N + 1) * nx, model).total * sizeof(double);
}

// (the 64 bytes spare leave room for the kernel's static s_k, as adjoint_carve_in_lds)
bool tangent_carve_in_lds(int n, int N, int nx, int ntan, bool model)
{
    return tangent_carve_bytes(n, N, nx, ntan, model) + 64 <= kLdsBytesPerCU;
}

int launch_tangent(const TangentLaunch &l, int64_t batch, hipStream_t st)
{
    const CondensedKkt &d = l.kkt;
    const bool lds = tangent_carve_in_lds(d.n, d.N, d.nx, l.ntan);
    const size_t bytes = tangent_carve_bytes(d.n, d.N, d.nx, l.ntan);
    if (!lds && !d.carve_ws) return MPCQP_EWORKSPACE;
    if (adjoint_threads(d.n) == 64) return launch_tangent_bs<64>(l, lds, bytes, batch, st);
    return launch_tangent_bs<256>(l, lds, bytes, batch, st);
}

int launch_tangent_model(const TangentModelLaunch &l, int64_t batch, hipStream_t st)
{
    const CondensedKkt &d = l.kkt;
    const bool lds = tangent_carve_in_lds(d.n, d.N, d.nx, l.ntan, true);
    const size_t bytes = tangent_carve_bytes(d.n, d.N, d.nx, l.ntan, true);
    if (!lds && !d.carve_ws) return MPCQP_EWORKSPACE;
    if (!l.U || !l.A.ptr || !l.x0.ptr) return MPCQP_EINVAL;
    if (adjoint_threads(d.n) == 64) return launch_tangent_model_bs<64>(l, lds, bytes, batch, st);
    return launch_tangent_model_bs<256>(l, lds, bytes, batch, st);
}

}  // namespace mpcqp
