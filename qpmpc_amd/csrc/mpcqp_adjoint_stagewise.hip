// mpcqp_adjoint_stagewise.hip -- the stage-wise adjoint (mpcqp_plan_vjp_stagewise_batch): the vector-Jacobian product of
// a batch of solved plans at any horizon, without condensing.
//
// One workgroup of 256 threads per problem, float64; nx <= 32, nu <= 8, any N. It solves the KKT adjoint of
// mpcqp_adjoint.hip,  [P G_A'; G_A 0][a; b] = [gU + Psi' gX; 0]  on A = {i : lam_i > 0}, with P = L L' the block Cholesky
// factorisation that the Riccati recursion is in whitened coordinates (oracle/stagewise_qr_np.py, WhitenedRiccati;
// DESIGN.md section 9, "Stage-wise adjoint"). Per problem:
//   1. Riccati, k = N-1 .. 0 (block-wide, P_{k+1} in LDS): S_k = w_u I + B_k' P B_k = Ls Ls' (MPCQP_NOT_PD if not PD),
//      Li = Ls^-1, K = S_k^-1 B_k' P A_k, Acl = A_k - B_k K; the record [Acl, K, Fn = Li B_k', Bw = B_k Li', Li] of the
//      step goes to the workspace; P_k = Q_k + sym(A_k' P Acl)
//   2. t = L^-1 (gU + Psi' gX): one backward sweep  y_k = Fn p + Li r_k,  p <- q_k + Acl' p - K' r_k  (q = gX, r = gU)
//   3. the active rows (ballot + prefix count, ascending; more than n: MPCQP_NOT_PD, more than max_active: MPCQP_SLOTS_FULL),
//      each one backward sweep started at its step j: y_j = Li D_row, p = C_row - K' D_row, then y_k = Fn p, p <- Acl' p.
//      The sweeps are independent: 256 / max(nx, nu) of them run side by side, lanes over state components
//   4. S = Y_A Y_A' (S_ab is a dot product over min(j_a, j_b) + 1 steps; one wavefront per row of S), rhs Y_A t,
//      S = R R' (LDS while max_active <= 63, else the workspace), b = S^-1 Y_A t
//   5. a = L^-T (t - Y_A' b): one forward sweep from x0 = 0, u_k = -K x + Li' s_k, x <- Acl x + Bw s_k, giving w = a and
//      Y = Psi a; then v_k = gX_k - w_x Y_k [k < N] - w_t Y_N [k = N] - C_k' b_k (terms gated by MPCQP_Q_STAGE / _TERMINAL),
//      g_goal = w_t Y_N, g_targets_k = w_x Y_k, g_e = b on the active rows, g_x0 = p_0 of p_k = v_k + A_k' p_{k+1}
//   6. (any of g_A .. g_w requested) X = rollout(x0, U), Z = rollout(0, U), then model_epilogue of
//      mpcqp_adjoint_common.h as in mpcqp_adjoint.hip: the costates pz and s, the outer products and the g_w reduction
//      (Y from phase 5 in place of -Psi w)
// The per-problem region of the workspace (doubles): the N records, the max_active whitened rows of n, S when it does not
// fit LDS, then t, s, w, Y, v, b, the row ids and, for phase 6, X, Z, pz, s, b over every row and the g_w partial sums.
#include <hip/hip_runtime.h>

#include "mpcqp.h"
#include "mpcqp_adjoint_common.h"

namespace mpcqp {
namespace {

constexpr int BS = 256;
constexpr int kMaxNx = 32, kMaxNu = 8;
constexpr int kSmDoubles = 3 * kMaxNx * kMaxNx + 3 * kMaxNx * kMaxNu + 2 * kMaxNu * kMaxNu;  // Riccati scratch
constexpr int kSLdsMax = 63;  // max_active whose S (stride max_active | 1) stays in LDS: 63 * 63 * 8 = 31 KB

struct SwCarve {
    int rs, ldS;                                    // doubles per record; stride of S
    int64_t rec, Y, S, t, s, w, Ys, v, bv, idx;     // idx: int32 row ids
    int64_t X, Zf, pz, sc, nuf, wred, total;
};

__host__ __device__ inline bool s_in_lds(int ka) { return ka <= kSLdsMax; }

// (phase 6 included: one size whichever outputs a launch asks for)
__host__ __device__ inline SwCarve make_carve(int nx, int nu, int N, int mk, int ka)
{
    SwCarve c;
    const int64_t n = (int64_t)N * nu, R = (int64_t)(N + 1) * nx, m = (int64_t)N * mk;
    c.rs = nx * nx + 2 * nu * nx + nx * nu + nu * nu;
    c.ldS = ka | 1;
    c.rec = 0;
    c.Y = c.rec + (int64_t)N * c.rs;
    c.S = c.Y + (int64_t)ka * n;
    c.t = c.S + (s_in_lds(ka) ? 0 : (int64_t)ka * c.ldS);
    c.s = c.t + n;
    c.w = c.s + n;
    c.Ys = c.w + n;
    c.v = c.Ys + R;
    c.bv = c.v + R;
    c.idx = c.bv + ka + 1;
    c.X = c.idx + (ka + 2) / 2;
    c.Zf = c.X + R;
    c.pz = c.Zf + R;
    c.sc = c.pz + R;
    c.nuf = c.sc + R;
    c.wred = c.nuf + m;
    c.total = c.wred + 3 * BS;
    return c;
}

// record of step k: Acl [nx x nx], K [nu x nx], Fn [nu x nx], Bw [nx x nu], Li [nu x nu] (lower)
struct Rec {
    const double *Acl, *K, *Fn, *Bw, *Li;
};
__device__ inline Rec rec_at(const double *rec, int k, int rs, int nx, int nu)
{
    const double *r = rec + (int64_t)k * rs;
    return Rec{r, r + nx * nx, r + nx * nx + nu * nx, r + nx * nx + 2 * nu * nx, r + nx * nx + 3 * nu * nx};
}

// 1. Riccati recursion into the records; false (uniform) where a stage Hessian is not positive definite
__device__ bool riccati(const StagewiseAdjointLaunch &a, int64_t b, double *rec, int rs, double *sm, int *s_flag)
{
    const int tid = threadIdx.x, nx = a.nx, nu = a.nu;
    double *P = sm, *PA = P + kMaxNx * kMaxNx, *Ac = PA + kMaxNx * kMaxNx, *PB = Ac + kMaxNx * kMaxNx;
    double *H = PB + kMaxNx * kMaxNu, *T = H + kMaxNx * kMaxNu, *Sm = T + kMaxNx * kMaxNu, *Li = Sm + kMaxNu * kMaxNu;
    const double qt = (a.flags & MPCQP_P_TERMINAL) ? a.wt : 0.0, qs = (a.flags & MPCQP_P_STAGE) ? a.wx : 0.0;
    for (int e = tid; e < nx * nx; e += BS) P[e] = (e / nx == e % nx) ? qt : 0.0;
    if (tid == 0) *s_flag = 0;
    __syncthreads();
    for (int k = a.N - 1; k >= 0; --k) {
        const double *Ak = op_step(a.problem.A, b, k), *Bk = op_step(a.problem.B, b, k);
        double *r = rec + (int64_t)k * rs;
        double *rAcl = r, *rK = r + nx * nx, *rFn = rK + nu * nx, *rBw = rFn + nu * nx, *rLi = rBw + nx * nu;
        for (int e = tid; e < nx * nx; e += BS) {  // PA = P A_k
            const int i = e / nx, j = e % nx;
            double acc = 0.0;
            for (int l = 0; l < nx; ++l) acc += P[i * nx + l] * Ak[l * nx + j];
            PA[e] = acc;
        }
        for (int e = tid; e < nx * nu; e += BS) {  // PB = P B_k
            const int i = e / nu, j = e % nu;
            double acc = 0.0;
            for (int l = 0; l < nx; ++l) acc += P[i * nx + l] * Bk[l * nu + j];
            PB[e] = acc;
        }
        __syncthreads();
        for (int e = tid; e < nu * nu; e += BS) {  // S = w_u I + B' P B
            const int i = e / nu, j = e % nu;
            double acc = i == j ? a.wu : 0.0;
            for (int l = 0; l < nx; ++l) acc += Bk[l * nu + i] * PB[l * nu + j];
            Sm[e] = acc;
        }
        for (int e = tid; e < nu * nx; e += BS) {  // H = B' P A
            const int i = e / nx, j = e % nx;
            double acc = 0.0;
            for (int l = 0; l < nx; ++l) acc += Bk[l * nu + i] * PA[l * nx + j];
            H[e] = acc;
        }
        __syncthreads();
        if (tid == 0) {  // S = Ls Ls', Li = Ls^-1 (nu <= 8: one lane)
            bool ok = true;
            for (int j = 0; j < nu && ok; ++j) {
                double d = Sm[j * nu + j];
                for (int l = 0; l < j; ++l) d -= Sm[j * nu + l] * Sm[j * nu + l];
                if (!(d > 0.0)) { ok = false; break; }
                const double sd = sqrt(d);
                Sm[j * nu + j] = sd;
                for (int i = j + 1; i < nu; ++i) {
                    double x = Sm[i * nu + j];
                    for (int l = 0; l < j; ++l) x -= Sm[i * nu + l] * Sm[j * nu + l];
                    Sm[i * nu + j] = x / sd;
                }
            }
            if (ok) {
                for (int c = 0; c < nu; ++c)
                    for (int i = 0; i < nu; ++i) {
                        double x = i == c ? 1.0 : 0.0;
                        for (int l = c; l < i; ++l) x -= Sm[i * nu + l] * Li[l * nu + c];
                        Li[i * nu + c] = i < c ? 0.0 : x / Sm[i * nu + i];
                    }
            } else {
                *s_flag = 1;
            }
        }
        __syncthreads();
        if (*s_flag) return false;
        for (int e = tid; e < nu * nx; e += BS) {  // T = Li H; Fn = Li B'
            const int i = e / nx, j = e % nx;
            double t = 0.0, f = 0.0;
            for (int l = 0; l <= i; ++l) {
                t += Li[i * nu + l] * H[l * nx + j];
                f += Li[i * nu + l] * Bk[j * nu + l];
            }
            T[e] = t;
            rFn[e] = f;
        }
        for (int e = tid; e < nx * nu; e += BS) {  // Bw = B Li'
            const int i = e / nu, j = e % nu;
            double acc = 0.0;
            for (int l = 0; l <= j; ++l) acc += Bk[i * nu + l] * Li[j * nu + l];
            rBw[e] = acc;
        }
        for (int e = tid; e < nu * nu; e += BS) rLi[e] = Li[e];
        __syncthreads();
        for (int e = tid; e < nu * nx; e += BS) {  // K = Li' T
            const int i = e / nx, j = e % nx;
            double acc = 0.0;
            for (int l = i; l < nu; ++l) acc += Li[l * nu + i] * T[l * nx + j];
            H[e] = acc;
            rK[e] = acc;
        }
        __syncthreads();
        for (int e = tid; e < nx * nx; e += BS) {  // Acl = A - B K
            const int i = e / nx, j = e % nx;
            double acc = Ak[e];
            for (int c = 0; c < nu; ++c) acc -= Bk[i * nu + c] * H[c * nx + j];
            Ac[e] = acc;
            rAcl[e] = acc;
        }
        __syncthreads();
        const double qk = k >= 1 ? qs : 0.0;
        for (int e = tid; e < nx * nx; e += BS) {  // P = Q_k + sym(A' P Acl), A' P = (P A)'
            const int i = e / nx, j = e % nx;
            double x = 0.0, y = 0.0;
            for (int l = 0; l < nx; ++l) {
                x += PA[l * nx + i] * Ac[l * nx + j];
                y += PA[l * nx + j] * Ac[l * nx + i];
            }
            P[e] = 0.5 * (x + y) + (i == j ? qk : 0.0);
        }
        __syncthreads();
    }
    return true;
}

template <bool kSLds>
__global__ void __launch_bounds__(BS) mpcqp_adjoint_stagewise_kernel(const StagewiseAdjointLaunch a)
{
    extern __shared__ double s_dyn[];
    __shared__ double sm[kSmDoubles];
    __shared__ int s_int[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const int nx = a.nx, nu = a.nu, N = a.N, mk = a.mk, n = a.n, m = a.m;
    const int R = (N + 1) * nx;
    const SwCarve cv = make_carve(nx, nu, N, mk, a.ka);
    double *base = a.workspace + b * cv.total;
    double *rec = base + cv.rec, *Y = base + cv.Y, *S = kSLds ? s_dyn : base + cv.S;
    double *t = base + cv.t, *s = base + cv.s, *w = base + cv.w, *Ys = base + cv.Ys, *v = base + cv.v;
    double *bv = base + cv.bv;
    int *idx = (int *)(base + cv.idx);
    const double *lam = a.lam ? a.lam + b * (int64_t)m : nullptr;
    const double *gU = a.gU + b * (int64_t)n;
    const double *gX = a.gX ? a.gX + b * (int64_t)R : nullptr;
    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
    const int Wd = nx > nu ? nx : nu;

    int verdict = a.status[b];
    int k = 0;
    if (verdict == 0 && !riccati(a, b, rec, cv.rs, sm, &s_int[1])) verdict = MPCQP_NOT_PD;
    if (verdict == 0) {
        // 3a. active rows, ascending; only the first max_active ids are kept
        k = active_rows(lam, m, a.ka, idx, &s_int[0]);
        if (k > n) verdict = MPCQP_NOT_PD;  // more active rows than variables: not a vertex's multipliers
        else if (k > a.ka) verdict = MPCQP_SLOTS_FULL;
    }
    if (verdict == 0) {
        // 2. t = L^-1 (gU + Psi' gX): one backward sweep, lanes over components, p double-buffered in LDS
        double *pv = sm;  // (the Riccati scratch is free now) 2 x 32
        if (tid < nx) pv[tid] = gX ? gX[N * nx + tid] : 0.0;
        __syncthreads();
        for (int kk = N - 1; kk >= 0; --kk) {
            const double *cur = pv + ((N - 1 - kk) & 1) * kMaxNx;
            double *nxt = pv + ((N - kk) & 1) * kMaxNx;
            const Rec rk = rec_at(rec, kk, cv.rs, nx, nu);
            const double *r = gU + kk * nu;
            if (tid < nu) {
                double acc = 0.0;
                for (int l = 0; l < nx; ++l) acc += rk.Fn[tid * nx + l] * cur[l];
                for (int l = 0; l <= tid; ++l) acc += rk.Li[tid * nu + l] * r[l];
                t[kk * nu + tid] = acc;
            }
            if (tid < nx) {
                double acc = gX ? gX[kk * nx + tid] : 0.0;
                for (int l = 0; l < nx; ++l) acc += rk.Acl[l * nx + tid] * cur[l];
                for (int c = 0; c < nu; ++c) acc -= rk.K[c * nx + tid] * r[c];
                nxt[tid] = acc;
            }
            __syncthreads();
        }
        // 3b. whitened active rows: BS / Wd sweeps side by side, each from its own step down to 0
        const int slots = BS / Wd, sl = tid / Wd, i = tid % Wd;
        double *pb = sm + 2 * kMaxNx;  // 2 x BS
        for (int r0 = 0; r0 < k; r0 += slots) {
            const int ra = r0 + sl;
            const bool on = sl < slots && ra < k;
            const int row = on ? idx[ra] : 0, ja = row / (mk > 0 ? mk : 1), rr = row - ja * mk;
            const int last = (r0 + slots < k ? r0 + slots : k) - 1;
            const int jmax = idx[last] / mk;
            double *yrow = Y + (int64_t)ra * n;
            for (int kk = jmax; kk >= 0; --kk) {
                const double *cur = pb + ((jmax - kk) & 1) * BS + sl * Wd;
                double *nxt = pb + ((jmax - kk + 1) & 1) * BS + sl * Wd;
                if (on && kk <= ja) {
                    const Rec rk = rec_at(rec, kk, cv.rs, nx, nu);
                    if (kk == ja) {
                        const double *Cr = op_step(a.problem.C, b, kk), *Dr = op_step(a.problem.D, b, kk);
                        if (Cr) Cr += rr * nx;
                        if (Dr) Dr += rr * nu;
                        if (i < nu) {
                            double acc = 0.0;
                            if (Dr)
                                for (int l = 0; l <= i; ++l) acc += rk.Li[i * nu + l] * Dr[l];
                            yrow[kk * nu + i] = acc;
                        }
                        if (i < nx) {
                            double acc = Cr ? Cr[i] : 0.0;
                            if (Dr)
                                for (int c = 0; c < nu; ++c) acc -= rk.K[c * nx + i] * Dr[c];
                            nxt[i] = acc;
                        }
                    } else {
                        if (i < nu) {
                            double acc = 0.0;
                            for (int l = 0; l < nx; ++l) acc += rk.Fn[i * nx + l] * cur[l];
                            yrow[kk * nu + i] = acc;
                        }
                        if (i < nx) {
                            double acc = 0.0;
                            for (int l = 0; l < nx; ++l) acc += rk.Acl[l * nx + i] * cur[l];
                            nxt[i] = acc;
                        }
                    }
                }
                __syncthreads();
            }
        }
        __syncthreads();
        // 4. S = Y_A Y_A' (lower) and Y_A t: one wavefront per row of S, lanes along the rows' common support
        for (int ra = wave; ra < k; ra += BS / 64) {
            const int ja = idx[ra] / mk;
            const double *ya = Y + (int64_t)ra * n;
            for (int rb = 0; rb <= ra + 1; ++rb) {
                const bool rhs = rb == ra + 1;
                const int jb = rhs ? ja : idx[rb] / mk;
                const int len = ((ja < jb ? ja : jb) + 1) * nu;
                const double *yb = rhs ? t : Y + (int64_t)rb * n;
                double acc = 0.0;
                for (int c = lane; c < len; c += 64) acc += ya[c] * yb[c];
                for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
                if (lane == 0) {
                    if (rhs) bv[ra] = acc;
                    else S[ra * cv.ldS + rb] = acc;
                }
            }
        }
        __syncthreads();
        if (!chol_lower<BS>(S, k, cv.ldS, tid)) verdict = MPCQP_NOT_PD;
    }
    if (verdict == 0) {
        solve_lower<BS>(S, k, cv.ldS, bv, tid);
        solve_lower_t<BS>(S, k, cv.ldS, bv, tid);
        // 5. s = t - Y_A' b (row a reaches column c when its step is >= c's), then a = L^-T s from x0 = 0
        for (int c = tid; c < n; c += BS) {
            double acc = t[c];
            for (int ra = lower_bound(idx, k, (c / nu) * mk); ra < k; ++ra) acc -= Y[(int64_t)ra * n + c] * bv[ra];
            s[c] = acc;
        }
        double *xv = sm;  // 2 x 32
        if (tid < nx) {
            xv[tid] = 0.0;
            Ys[tid] = 0.0;
        }
        __syncthreads();
        for (int kk = 0; kk < N; ++kk) {
            const double *cur = xv + (kk & 1) * kMaxNx;
            double *nxt = xv + ((kk + 1) & 1) * kMaxNx;
            const Rec rk = rec_at(rec, kk, cv.rs, nx, nu);
            const double *sk = s + kk * nu;
            if (tid < nu) {
                double acc = 0.0;
                for (int l = 0; l < nx; ++l) acc -= rk.K[tid * nx + l] * cur[l];
                for (int l = tid; l < nu; ++l) acc += rk.Li[l * nu + tid] * sk[l];
                w[kk * nu + tid] = acc;
            }
            if (tid < nx) {
                double acc = 0.0;
                for (int l = 0; l < nx; ++l) acc += rk.Acl[tid * nx + l] * cur[l];
                for (int c = 0; c < nu; ++c) acc += rk.Bw[tid * nu + c] * sk[c];
                nxt[tid] = acc;
                Ys[(kk + 1) * nx + tid] = acc;
            }
            __syncthreads();
        }
        // v, g_goal, g_targets, g_e
        double *ggoal = out_at(a.out.g_goal, b * nx);
        double *gtgt = out_at(a.out.g_targets, b * (int64_t)N * nx);
        double *ge = out_at(a.out.g_e, b * (int64_t)m);
        for (int e = tid; e < R; e += BS) {
            const int kk = e / nx, j = e % nx;
            double acc = gX ? gX[e] : 0.0;
            if (qs && kk < N) acc -= a.wx * Ys[e];
            if (qt && kk == N) acc -= a.wt * Ys[e];
            if (kk < N && a.problem.C.ptr) {
                const double *Ck = op_step(a.problem.C, b, kk);
                for (int ra = lower_bound(idx, k, kk * mk); ra < k && idx[ra] < (kk + 1) * mk; ++ra)
                    acc -= Ck[(idx[ra] - kk * mk) * nx + j] * bv[ra];
            }
            v[e] = acc;
            if (ggoal && kk == N) ggoal[j] = qt ? a.wt * Ys[e] : 0.0;
            if (gtgt && kk < N) gtgt[e] = qs ? a.wx * Ys[e] : 0.0;
        }
        if (ge)
            for (int i = tid; i < m; i += BS) {
                const int lo = lower_bound(idx, k, i);
                ge[i] = (lo < k && idx[lo] == i) ? bv[lo] : 0.0;
            }
        __syncthreads();
        // g_x0 = p_0: p_N = v_N, p_k = v_k + A_k' p_{k+1} (in place on v)
        for (int kk = N - 1; kk >= 0; --kk) {
            const double *Ak = op_step(a.problem.A, b, kk);
            if (tid < nx) {
                double acc = 0.0;
                for (int j = 0; j < nx; ++j) acc += Ak[j * nx + tid] * v[(kk + 1) * nx + j];
                v[kk * nx + tid] += acc;
            }
            __syncthreads();
        }
        if (a.out.g_x0 && tid < nx) ((double *)a.out.g_x0)[b * nx + tid] = v[tid];
        if (a.model) {
            // 6. X = rollout(x0, U), Z = rollout(0, U), then the model epilogue with Y (p is v, recursed above)
            double *X = base + cv.X, *Zf = base + cv.Zf;
            const double *U = a.U + b * (int64_t)n;
            const double *x0 = (const double *)a.problem.x0.ptr + b * a.problem.x0.batch_stride;
            if (tid < nx) {
                X[tid] = x0[tid];
                Zf[tid] = 0.0;
            }
            __syncthreads();
            for (int kk = 0; kk < N; ++kk) {
                const double *Ak = op_step(a.problem.A, b, kk), *Bk = op_step(a.problem.B, b, kk);
                if (tid < 2 * nx) {
                    double *x = tid < nx ? X : Zf;
                    const int i = tid % nx;
                    double acc = 0.0;
                    for (int l = 0; l < nx; ++l) acc += Ak[i * nx + l] * x[kk * nx + l];
                    for (int c = 0; c < nu; ++c) acc += Bk[i * nu + c] * U[kk * nu + c];
                    x[(kk + 1) * nx + i] = acc;
                }
                __syncthreads();
            }
            const ModelVecs mv{lam, U, w, Ys,
                               qt ? (const double *)a.problem.goal.ptr + b * a.problem.goal.batch_stride : nullptr,
                               qs ? (const double *)a.problem.targets.ptr + b * a.problem.targets.batch_stride : nullptr,
                               bv, idx, k, v, X, Zf, base + cv.pz, base + cv.sc, base + cv.nuf, base + cv.wred};
            model_epilogue<BS, false, false>(a, a.problem.A, a.problem.C, a.out, b, mv);
        }
    }
    if (verdict != 0) {  // (uniform) unsolved, not positive definite or slots full: all-zero gradients
        zero_outputs<BS>(tid, out_at(a.out.g_x0, b * nx), nx, out_at(a.out.g_goal, b * nx), nx,
                         out_at(a.out.g_targets, b * (int64_t)N * nx), (int64_t)N * nx, out_at(a.out.g_e, b * (int64_t)m), m);
        zero_model_outputs<BS>(a.out, nx, nu, N, m, b, tid);
    }
    if (a.vjp_status && tid == 0) a.vjp_status[b] = verdict;
}

}  // namespace

bool stagewise_adjoint_applies(int nx, int nu) { return nx <= kMaxNx && nu <= kMaxNu; }

// per problem, phase 6 included (one size whichever outputs a launch asks for)
size_t stagewise_adjoint_bytes(int nx, int nu, int N, int mk, int max_active)
{
    return (size_t)make_carve(nx, nu, N, mk, max_active > 0 ? max_active : 1).total * sizeof(double);
}

int launch_adjoint_stagewise(const StagewiseAdjointLaunch &l, int64_t batch, hipStream_t st)
{
    if (!l.workspace) return MPCQP_EWORKSPACE;
    if (l.model && !l.U) return MPCQP_EINVAL;
    if (s_in_lds(l.ka))
        return launch_per_problem(mpcqp_adjoint_stagewise_kernel<true>, l, BS, (size_t)l.ka * (l.ka | 1) * sizeof(double), batch, st);
    return launch_per_problem(mpcqp_adjoint_stagewise_kernel<false>, l, BS, 0, batch, st);
}

}  // namespace mpcqp
