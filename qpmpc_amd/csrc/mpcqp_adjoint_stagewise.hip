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
//
// The stage-wise tangent (mpcqp_plan_jvp_stagewise_batch, mpcqp_tangent_stagewise_kernel below) is the forward-mode
// counterpart on the same factorisation: phases 1, 3 and 4 are device functions that both kernels call.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "mpcqp.h"
#include "mpcqp_adjoint_common.h"
#include "mpcqp_lane.h"

namespace mpcqp {
namespace {

constexpr int BS = 256;
constexpr int kMaxNx = 32, kMaxNu = 8;
constexpr int kSmDoubles = 3 * kMaxNx * kMaxNx + 3 * kMaxNx * kMaxNu + 2 * kMaxNu * kMaxNu;  // Riccati scratch
constexpr int kPassLds = 2 * BS;  // one buffer of a pass of tangents: BS / max(nx, nu) slots of nx + nu <= 2 max(nx, nu)
constexpr int kSLdsMax = 63;  // max_active whose S (stride max_active | 1) stays in LDS: 63 * 63 * 8 = 31 KB

// the part of a problem's region that both kernels lay out alike: the N records, the max_active whitened rows of n, S when
// it does not fit LDS; `end` is where the kernel's own vectors start
struct SwBase {
    int rs, ldS;  // doubles per record; stride of S
    int64_t rec, Y, S, end;
};

__host__ __device__ inline bool s_in_lds(int ka) { return ka <= kSLdsMax; }

__host__ __device__ inline SwBase make_base(int nx, int nu, int N, int ka)
{
    SwBase c;
    c.rs = nx * nx + 2 * nu * nx + nx * nu + nu * nu;
    c.ldS = ka | 1;
    c.rec = 0;
    c.Y = c.rec + (int64_t)N * c.rs;
    c.S = c.Y + (int64_t)ka * N * nu;
    c.end = c.S + (s_in_lds(ka) ? 0 : (int64_t)ka * c.ldS);
    return c;
}

struct SwCarve : SwBase {
    int64_t t, s, w, Ys, v, bv, idx;  // idx: int32 row ids
    int64_t X, Zf, pz, sc, nuf, wred, total;
};

// (phase 6 included: one size whichever outputs a launch asks for)
__host__ __device__ inline SwCarve make_carve(int nx, int nu, int N, int mk, int ka)
{
    SwCarve c;
    static_cast<SwBase &>(c) = make_base(nx, nu, N, ka);
    const int64_t n = (int64_t)N * nu, R = (int64_t)(N + 1) * nx, m = (int64_t)N * mk;
    c.t = c.end;
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

// The stage-wise tangent kernel's region: the base, the row ids, then the scratch of ONE pass of tangents (tg = min(ntan,
// tangent_slots): the passes reuse it): xs = rollout(dx0, 0) [tg x (N + 1) nx] and dh_A, then mu [tg x ldS]. r, s and dU
// share the caller's dU.
struct SwTanCarve : SwBase {
    int tg;
    int64_t idx, xs, mu, total;
    int64_t X, Zf, pi, zs;  // model: appended after mu (total includes them only when model); zs: the pass's second slot
};

__host__ __device__ inline int tangent_slots(int nx, int nu) { return BS / (nx > nu ? nx : nu); }

__host__ __device__ inline SwTanCarve make_tan_carve(int nx, int nu, int N, int ka, int ntan, bool model = false)
{
    SwTanCarve c;
    static_cast<SwBase &>(c) = make_base(nx, nu, N, ka);
    const int slots = tangent_slots(nx, nu);
    c.tg = ntan < slots ? ntan : slots;
    c.idx = c.end;
    c.xs = c.idx + (ka + 2) / 2;
    c.mu = c.xs + (int64_t)c.tg * (N + 1) * nx;
    c.total = c.mu + (int64_t)c.tg * c.ldS;
    const int64_t R = (int64_t)(N + 1) * nx;
    c.X = c.total;
    c.Zf = c.X + R;
    c.pi = c.Zf + R;
    c.zs = c.pi + R;
    if (model) c.total = c.zs + c.tg * R;
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
// (D: the kernel's launch structure -- nx, nu, N, flags, wt, wx, wu, problem)
template <class D>
__device__ bool riccati(const D &a, int64_t b, double *rec, int rs, double *sm, int *s_flag)
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

// 3b. The whitened active rows Y [k x n] (ids idx, ascending): BS / max(nx, nu) backward sweeps side by side, lanes over
// state components, each from its own step down to 0; one barrier per step for the whole group. pb: 2 x BS doubles of LDS.
__device__ void whiten_rows(const MpcqpProblem &problem, int64_t b, const double *rec, int rs, int nx, int nu, int mk, int n,
                            const int *idx, int k, double *Y, double *pb)
{
    const int tid = threadIdx.x, Wd = nx > nu ? nx : nu;
    const int slots = BS / Wd, sl = tid / Wd, i = tid % Wd;
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
                const Rec rk = rec_at(rec, kk, rs, nx, nu);
                if (kk == ja) {
                    const double *Cr = op_step(problem.C, b, kk), *Dr = op_step(problem.D, b, kk);
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
}

// 4. S = Y_A Y_A' (lower, stride ldS) and, when `rhs` is given, bv = Y_A rhs: S_ab is a dot product over min(j_a, j_b) + 1
// steps; one wavefront per row of S, lanes along the rows' common support
__device__ void gram_rows(const double *Y, const int *idx, int k, int mk, int nu, int n, double *S, int ldS, const double *rhs,
                          double *bv)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int ra = wave; ra < k; ra += BS / 64) {
        const int ja = idx[ra] / mk;
        const double *ya = Y + (int64_t)ra * n;
        for (int rb = 0; rb <= ra + (rhs ? 1 : 0); ++rb) {
            const bool last = rb == ra + 1;
            const int jb = last ? ja : idx[rb] / mk;
            const int len = ((ja < jb ? ja : jb) + 1) * nu;
            const double *yb = last ? rhs : Y + (int64_t)rb * n;
            double acc = 0.0;
            for (int c = lane; c < len; c += 64) acc += ya[c] * yb[c];
            acc = wave_sum_shfl(acc);
            if (lane == 0) {
                if (last) bv[ra] = acc;
                else S[ra * ldS + rb] = acc;
            }
        }
    }
    __syncthreads();
}

template <bool kSLds>
__global__ void __launch_bounds__(BS) mpcqp_adjoint_stagewise_kernel(const StagewiseAdjointLaunch a)
{
    extern __shared__ double s_dyn[];
    __shared__ double sm[kSmDoubles];
    __shared__ int s_int[2];
    const int tid = threadIdx.x;
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
        // 3b. the whitened active rows, 4. their Gram matrix and Y_A t
        whiten_rows(a.problem, b, rec, cv.rs, nx, nu, mk, n, idx, k, Y, sm + 2 * kMaxNx);
        gram_rows(Y, idx, k, mk, nu, n, S, cv.ldS, t, bv);
        if (!chol_lower<BS, true>(S, k, cv.ldS, tid, gram_pivot_floor(n, k))) verdict = MPCQP_NOT_PD;
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

// mpcqp_tangent_stagewise_kernel (mpcqp_plan_jvp_stagewise_batch): the forward-mode counterpart at any horizon, T tangents
// (dx0, dgoal, dtargets, de) per problem on ONE factorisation ("Stage-wise forward sensitivities").
// Phases 1, 3 and 4 above run once (no right-hand side in phase 4); then, per pass of BS / max(nx, nu) tangents side by
// side (lanes over state components, one barrier per step for the whole group, as the row sweeps of phase 3b):
//   a. xs = rollout(dx0, 0) with A_k                                         (skipped when dx0 is NULL: xs = 0)
//   b. r = -L^-1 Psi' c: phase 2's backward sweep with gU = 0, gX = -c,  c_k = w_x (xs_k - dtargets_k) [k < N],
//      c_N = w_t (xs_N - dgoal) (terms gated by MPCQP_Q_STAGE / _TERMINAL); r goes to the tangent's dU
//   c. mu = S^-1 (Y_A r - dh_A), dh_A = de_A - (C xs)_A: one wavefront per (row, tangent), then the two substitutions with
//      S = R R' for the whole pass (sweep_lower / sweep_lower_t)
//   d. s = r - Y_A' mu in place, then phase 5's forward sweep from x = 0 in place: dU = L^-T s, dX = xs + (the state)
// A tangent's arithmetic does not depend on its slot, its pass or T.
//
// kModel (mpcqp_plan_jvp_model_stagewise_batch; DESIGN.md section 9, "Model and weight tangents"): tangents of A, B, C, D
// and the weights as well. Once per problem X = rollout(x0, U), Z = rollout(0, U) (as phase 6 above) and the costate pi
// (stationarity_costate); per pass the rollout of a. has its forcing term and carries zs in a second slot where a P-only
// term reads it, the sweep of b. starts from gX = -c, gU = -g (the step's g staged in LDS one step ahead, as d. stages
// s_k), and dh has its two more terms (tangent_c, tangent_g, tangent_dh of mpcqp_adjoint_common.h).
template <bool kSLds, bool kModel>
__global__ void __launch_bounds__(BS)
mpcqp_tangent_stagewise_kernel(const typename std::conditional<kModel, StagewiseTangentModelLaunch, StagewiseTangentLaunch>::type a)
{
    extern __shared__ double s_dyn[];
    __shared__ double sm[kSmDoubles];
    __shared__ int s_int[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t b = blockIdx.x;
    const int nx = a.nx, nu = a.nu, N = a.N, mk = a.mk, n = a.n, m = a.m, T = a.ntan;
    const int R = (N + 1) * nx;
    const SwTanCarve cv = make_tan_carve(nx, nu, N, a.ka, T, kModel);
    double *base = a.workspace + b * cv.total;
    double *rec = base + cv.rec, *Y = base + cv.Y, *S = kSLds ? s_dyn : base + cv.S;
    double *xs = base + cv.xs, *mu = base + cv.mu;
    int *idx = (int *)(base + cv.idx);
    const double *lam = a.lam ? a.lam + b * (int64_t)m : nullptr;
    // tangent t of a problem at t nx / t nx / t N nx / t m; a null one is zero, a zero stride shares it
    const double *dx0 = a.tan.dx0 ? (const double *)a.tan.dx0 + b * a.tan.dx0_stride : nullptr;
    const double *dgoal = a.tan.dgoal ? (const double *)a.tan.dgoal + b * a.tan.dgoal_stride : nullptr;
    const double *dtgt = a.tan.dtargets ? (const double *)a.tan.dtargets + b * a.tan.dtargets_stride : nullptr;
    const double *de = a.tan.de ? (const double *)a.tan.de + b * a.tan.de_stride : nullptr;
    double *dU = a.dU + b * (int64_t)T * n;
    double *dX = a.dX ? a.dX + b * (int64_t)T * R : nullptr;
    const bool qt = (a.flags & MPCQP_Q_TERMINAL) != 0, qs = (a.flags & MPCQP_Q_STAGE) != 0;
    const bool has_xs = kModel || dx0;  // xs holds the tangents' rollouts (else they are zero)
    ModelTanVecs mv{};

    int verdict = a.status[b];
    int k = 0;
    if (verdict == 0 && !riccati(a, b, rec, cv.rs, sm, &s_int[1])) verdict = MPCQP_NOT_PD;
    if (verdict == 0) {
        k = active_rows(lam, m, a.ka, idx, &s_int[0]);
        if (k > n) verdict = MPCQP_NOT_PD;
        else if (k > a.ka) verdict = MPCQP_SLOTS_FULL;
    }
    if (verdict == 0 && k > 0) {
        whiten_rows(a.problem, b, rec, cv.rs, nx, nu, mk, n, idx, k, Y, sm);
        gram_rows(Y, idx, k, mk, nu, n, S, cv.ldS, nullptr, nullptr);
        if (!chol_lower<BS, true>(S, k, cv.ldS, tid, gram_pivot_floor(n, k))) verdict = MPCQP_NOT_PD;
    }
    if constexpr (kModel) {
        if (verdict == 0) {
            // X = rollout(x0, U), Z = rollout(0, U), then the costate pi
            double *X = base + cv.X, *Zf = base + cv.Zf, *pi = base + cv.pi;
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
            mv = ModelTanVecs{tan_at(a.mtan.dA, a.mtan.dA_stride, b), tan_at(a.mtan.dB, a.mtan.dB_stride, b),
                              tan_at(a.mtan.dC, a.mtan.dC_stride, b), tan_at(a.mtan.dD, a.mtan.dD_stride, b),
                              tan_at(a.mtan.dw, a.mtan.dw_stride, b), X, Zf, pi, U, lam,
                              qt ? (const double *)a.problem.goal.ptr + b * a.problem.goal.batch_stride : nullptr,
                              qs ? (const double *)a.problem.targets.ptr + b * a.problem.targets.batch_stride : nullptr};
            stationarity_costate<BS>(a, a.problem.A, a.problem.C, b, mv, pi);
        }
    }
    if (verdict == 0) {
        const int Wd = nx > nu ? nx : nu, slots = BS / Wd, sl = tid / Wd, i = tid % Wd;
        const int ls = nx + nu;  // a slot's LDS: the carried state, then the step's s_k (phase d) or g_k (phase b, kModel)
        double *buf = sm;        // 2 x kPassLds (the Riccati scratch is free now)
        double *zbuf = sm + 2 * kPassLds;  // kModel: 2 x kPassLds more, the carried zs
        const bool with_zs = kModel && tangent_needs_zs(a.flags);
        for (int t0 = 0; t0 < T; t0 += slots) {
            const int tg = T - t0 < slots ? T - t0 : slots;
            const bool on = sl < tg;
            const int64_t tt = t0 + (on ? sl : 0);
            double *xst = xs + (int64_t)(on ? sl : 0) * R, *dUt = dU + tt * n, *dXt = dX ? dX + tt * R : nullptr;
            const double *x0t = dx0 ? dx0 + tt * nx : nullptr, *glt = dgoal ? dgoal + tt * nx : nullptr;
            const double *tgt = dtgt ? dtgt + tt * N * nx : nullptr;
            double *zst = base + cv.zs + (int64_t)(on ? sl : 0) * R;  // (kModel)
            // a. xs = rollout(dx0, 0)
            if constexpr (kModel) {
                // ... with the forcing term dA_k X_k + dB_k u_k, and zs the same from 0 with Z_k
                if (on && i < nx) {
                    const double x = x0t ? x0t[i] : 0.0;
                    buf[sl * ls + i] = x;
                    xst[i] = x;
                    if (with_zs) {
                        zbuf[sl * ls + i] = 0.0;
                        zst[i] = 0.0;
                    }
                }
                __syncthreads();
                for (int kk = 0; kk < N; ++kk) {
                    const int cb = (kk & 1) * kPassLds + sl * ls, nb = ((kk + 1) & 1) * kPassLds + sl * ls;
                    if (on && i < nx) {
                        const double *Ak = op_step(a.problem.A, b, kk);
                        double acc = tangent_forcing(a, mv, mv.X, (int)tt, kk, i);
                        for (int l = 0; l < nx; ++l) acc += Ak[i * nx + l] * buf[cb + l];
                        buf[nb + i] = acc;
                        xst[(kk + 1) * nx + i] = acc;
                        if (with_zs) {
                            double az = tangent_forcing(a, mv, mv.Zf, (int)tt, kk, i);
                            for (int l = 0; l < nx; ++l) az += Ak[i * nx + l] * zbuf[cb + l];
                            zbuf[nb + i] = az;
                            zst[(kk + 1) * nx + i] = az;
                        }
                    }
                    __syncthreads();
                }
            } else if (dx0) {
                if (on && i < nx) {
                    const double x = x0t[i];
                    buf[sl * ls + i] = x;
                    xst[i] = x;
                }
                __syncthreads();
                for (int kk = 0; kk < N; ++kk) {
                    const double *cur = buf + (kk & 1) * kPassLds + sl * ls;
                    double *nxt = buf + ((kk + 1) & 1) * kPassLds + sl * ls;
                    if (on && i < nx) {
                        const double *Ak = op_step(a.problem.A, b, kk);
                        double acc = 0.0;
                        for (int l = 0; l < nx; ++l) acc += Ak[i * nx + l] * cur[l];
                        nxt[i] = acc;
                        xst[(kk + 1) * nx + i] = acc;
                    }
                    __syncthreads();
                }
            }
            // b. r = -L^-1 Psi' c into dU (lane i reads back the xs components it wrote itself)
            if constexpr (kModel) {
                // ... r = -L^-1 (Psi' c + g): phase 2's sweep with gX = -c, gU = -g
                if (on) {
                    if (i < nx) {
                        const int e = N * nx + i;
                        buf[sl * ls + i] = -tangent_c(a, mv, (int)tt, e, xst[e], with_zs ? zst[e] : 0.0, tgt, glt);
                    }
                    if (i < nu) buf[sl * ls + nx + i] = -tangent_g(a, mv, (int)tt, (N - 1) * nu + i);
                }
                __syncthreads();
                for (int kk = N - 1; kk >= 0; --kk) {
                    const double *cur = buf + ((N - 1 - kk) & 1) * kPassLds + sl * ls, *rk_ = cur + nx;
                    double *nxt = buf + ((N - kk) & 1) * kPassLds + sl * ls;
                    if (on) {
                        const Rec rk = rec_at(rec, kk, cv.rs, nx, nu);
                        if (i < nu) {
                            double acc = 0.0;
                            for (int l = 0; l < nx; ++l) acc += rk.Fn[i * nx + l] * cur[l];
                            for (int l = 0; l <= i; ++l) acc += rk.Li[i * nu + l] * rk_[l];
                            dUt[kk * nu + i] = acc;
                            if (kk > 0) nxt[nx + i] = -tangent_g(a, mv, (int)tt, (kk - 1) * nu + i);
                        }
                        if (i < nx) {
                            const int e = kk * nx + i;
                            double acc = -tangent_c(a, mv, (int)tt, e, xst[e], with_zs ? zst[e] : 0.0, tgt, glt);
                            for (int l = 0; l < nx; ++l) acc += rk.Acl[l * nx + i] * cur[l];
                            for (int c = 0; c < nu; ++c) acc -= rk.K[c * nx + i] * rk_[c];
                            nxt[i] = acc;
                        }
                    }
                    __syncthreads();
                }
            } else {
                if (on && i < nx) {
                    double c = 0.0;
                    if (qt) c = a.wt * ((dx0 ? xst[N * nx + i] : 0.0) - (glt ? glt[i] : 0.0));
                    buf[sl * ls + i] = -c;
                }
                __syncthreads();
                for (int kk = N - 1; kk >= 0; --kk) {
                    const double *cur = buf + ((N - 1 - kk) & 1) * kPassLds + sl * ls;
                    double *nxt = buf + ((N - kk) & 1) * kPassLds + sl * ls;
                    if (on) {
                        const Rec rk = rec_at(rec, kk, cv.rs, nx, nu);
                        if (i < nu) {
                            double acc = 0.0;
                            for (int l = 0; l < nx; ++l) acc += rk.Fn[i * nx + l] * cur[l];
                            dUt[kk * nu + i] = acc;
                        }
                        if (i < nx) {
                            double acc = 0.0;
                            if (qs) acc = -a.wx * ((dx0 ? xst[kk * nx + i] : 0.0) - (tgt ? tgt[kk * nx + i] : 0.0));
                            for (int l = 0; l < nx; ++l) acc += rk.Acl[l * nx + i] * cur[l];
                            nxt[i] = acc;
                        }
                    }
                    __syncthreads();
                }
            }
            if (k > 0) {
                // c. mu = Y_A r - dh_A = Y_A r + (C xs)_A - de_A: one wavefront per (row, tangent), lanes along the row's
                // support (the first nx lanes add the C xs terms); then mu <- S^-1 mu for the pass
                for (int e = wave; e < k * tg; e += BS / 64) {
                    const int ra = e / tg, g = e % tg;
                    const int row = idx[ra], ja = row / mk;
                    const double *ya = Y + (int64_t)ra * n, *rt = dU + (int64_t)(t0 + g) * n;
                    const int len = (ja + 1) * nu;
                    double acc = 0.0;
                    for (int c = lane; c < len; c += 64) acc += ya[c] * rt[c];
                    if (has_xs && a.problem.C.ptr && lane < nx)
                        acc += op_step(a.problem.C, b, ja)[(row - ja * mk) * nx + lane] * xs[(int64_t)g * R + ja * nx + lane];
                    acc = wave_sum_shfl(acc);
                    if constexpr (kModel) {
                        if (lane == 0) acc += tangent_dh(a, mv, t0 + g, row);
                    }
                    if (lane == 0) mu[g * cv.ldS + ra] = acc - (de ? de[(int64_t)(t0 + g) * m + row] : 0.0);
                }
                __syncthreads();
                sweep_lower<BS>(S, k, cv.ldS, mu, tg, tid);
                sweep_lower_t<BS>(S, k, cv.ldS, mu, tg, tid);
                // d. s = r - Y_A' mu in place (row a reaches column c when its step is >= c's)
                for (int e = tid; e < tg * n; e += BS) {
                    const int g = e / n, c = e % n;
                    double *sc = dU + (int64_t)(t0 + g) * n + c;
                    const double *mg = mu + g * cv.ldS;
                    double acc = *sc;
                    for (int ra = lower_bound(idx, k, (c / nu) * mk); ra < k; ++ra) acc -= Y[(int64_t)ra * n + c] * mg[ra];
                    *sc = acc;
                }
                __syncthreads();
            }
            // d (second half). dU = L^-T s in place, from x = 0: the step's s_k is staged in LDS one step ahead of the u_k that replaces it
            if (on) {
                if (i < nx) {
                    buf[sl * ls + i] = 0.0;
                    if (dXt) dXt[i] = dx0 ? x0t[i] : 0.0;
                }
                if (i < nu) buf[sl * ls + nx + i] = dUt[i];
            }
            __syncthreads();
            for (int kk = 0; kk < N; ++kk) {
                const double *cur = buf + (kk & 1) * kPassLds + sl * ls, *sk = cur + nx;
                double *nxt = buf + ((kk + 1) & 1) * kPassLds + sl * ls;
                if (on) {
                    const Rec rk = rec_at(rec, kk, cv.rs, nx, nu);
                    if (i < nu) {
                        double acc = 0.0;
                        for (int l = 0; l < nx; ++l) acc -= rk.K[i * nx + l] * cur[l];
                        for (int l = i; l < nu; ++l) acc += rk.Li[l * nu + i] * sk[l];
                        dUt[kk * nu + i] = acc;
                        if (kk + 1 < N) nxt[nx + i] = dUt[(kk + 1) * nu + i];
                    }
                    if (i < nx) {
                        double acc = 0.0;
                        for (int l = 0; l < nx; ++l) acc += rk.Acl[i * nx + l] * cur[l];
                        for (int c = 0; c < nu; ++c) acc += rk.Bw[i * nu + c] * sk[c];
                        nxt[i] = acc;
                        if (dXt) dXt[(kk + 1) * nx + i] = (has_xs ? xst[(kk + 1) * nx + i] : 0.0) + acc;
                    }
                }
                __syncthreads();
            }
        }
    }
    if (verdict != 0)  // (uniform) unsolved, not positive definite or slots full: all-zero tangents
        zero_outputs<BS>(tid, dU, (int64_t)T * n, dX, (int64_t)T * R);
    if (a.jvp_status && tid == 0) a.jvp_status[b] = verdict;
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

// per problem: the records, the whitened rows, S beyond LDS, the row ids and one pass of tangents' scratch
size_t stagewise_tangent_bytes(int nx, int nu, int N, int max_active, int ntan, bool model)
{
    return (size_t)make_tan_carve(nx, nu, N, max_active > 0 ? max_active : 1, ntan, model).total * sizeof(double);
}

int launch_tangent_stagewise(const StagewiseTangentLaunch &l, int64_t batch, hipStream_t st)
{
    if (!l.workspace) return MPCQP_EWORKSPACE;
    if (s_in_lds(l.ka))
        return launch_per_problem(mpcqp_tangent_stagewise_kernel<true, false>, l, BS, (size_t)l.ka * (l.ka | 1) * sizeof(double), batch, st);
    return launch_per_problem(mpcqp_tangent_stagewise_kernel<false, false>, l, BS, 0, batch, st);
}

int launch_tangent_model_stagewise(const StagewiseTangentModelLaunch &l, int64_t batch, hipStream_t st)
{
    if (!l.workspace) return MPCQP_EWORKSPACE;
    if (!l.U) return MPCQP_EINVAL;
    if (s_in_lds(l.ka))
        return launch_per_problem(mpcqp_tangent_stagewise_kernel<true, true>, l, BS, (size_t)l.ka * (l.ka | 1) * sizeof(double), batch, st);
    return launch_per_problem(mpcqp_tangent_stagewise_kernel<false, true>, l, BS, 0, batch, st);
}

}  // namespace mpcqp
