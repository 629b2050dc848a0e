// mpcqp_duo.hip -- gfx950 kernel for problems of 17 .. 32 variables (m <= 64 inequality rows, at most four rows per step,
// nx in {2, 3, 4}, float64): TWO PROBLEMS PER WAVEFRONT, everything on chip, no workspace (MPCQP_OPT_ON_CHIP_32).
//
// Replaces the same reference code as its siblings (qpmpc/mpc_qp.py:53-149 for the build, qpsolvers.solve_problem at
// qpmpc/solve_mpc.py:43 for the solve) for the cold fused build+solve one step behind the four-per-wavefront kernels' sixteen
// variables, where the launch otherwise falls to the stage-wise kernels.
//
// A problem owns the 32 lanes of half a wavefront (mpcqp_pair.hip's split), and lane l of a half holds, in registers,
//   RT   row l of T = N* (active-set slot l; its multiplier and constraint id)      32 doubles
//   RH   row l of the projector H = I - M_A' T (symmetric)                         32 doubles
//   RM0  row l of M = G L^-T (constraint l), RM1 row 32 + l, and their slacks      64 doubles
// and component l of every 32-vector (y, z, u). One wavefront per SIMD (a 512-register budget; see profiles/onchip32.md for
// the figures), at most 40 KB of LDS per wavefront, so four wavefronts -- eight problems -- per compute unit.
// Nothing is exchanged by hand-written DPP arithmetic: a vector every lane of a problem needs (row p of M, z, the leaving
// row of T) is written to LDS by its owner and read back as broadcast ds_read_b128 (the mpcqp_w64.hip idiom); reductions are
// the DPP row rotations of mpcqp_lane.h plus one v_permlane16_swap; a value of one lane comes through ds_bpermute.
// The two halves take their own branches of the iteration through predication: every per-problem scalar is a per-lane value
// that is uniform inside a half, and no value ever crosses from one half to the other, so a problem's arithmetic does not
// depend on its neighbour or on the batch size.
//
// Solver: the dual active-set method of mpcqp_w64.hip (Goldfarb-Idnani 1983 with the explicit operator T = N*; derivation
// there), with H kept explicitly as in mpcqp_pair.hip and the constraint rows NOT kept projected (the K-less trip):
//   row p selected: farthest violated row in the P^-1 metric, s_i / |M_i|
//   r_a = T_a . M_p ; z = -H M_p ; d2 = |z|^2 from z itself ; M_i . z from the rows of M
//   t = min(t1 = min lam_a / r_a, t2 = -s_p / d2) ; s_i -= t M_i . z ; lam_a -= t r_a
//   full step:    T_a += (r_a/d2) z, T_new = -z/d2, H -= z z'/d2
//   partial step: slot l leaves, T_a -= (T_a.T_l / T_l.T_l) T_l, H += T_l T_l'/T_l.T_l, then the same p again
// M_p depends on the active rows when d2 / |M_p|^2 <= 1e-14; no step possible (no blocking multiplier either) = infeasible.
// The final multipliers get one step of iterative refinement, and the slacks are evaluated from scratch at the refined point
// before the plan is accepted; a point that fails goes back into the loop (four times at most).
//
// Build: lane a carries column a of Psi_k and -- every lane for itself -- the free response Phi_k x0; the rows of G go through
// a 32-row LDS image to the lanes that own them; the Gram matrix is accumulated by rows (v_b broadcast from LDS). Cholesky
// and the rows of L^-T come out of ONE right-looking elimination: column j of the trailing matrix is broadcast through LDS and
// both rows a lane holds (P_l, e_l) take the same update; M = G L^-T is then a triangular product against the broadcast rows
// of L^-T.
//
// Shared model (MODEL = true; mpcqp_solve_model_bounds_batch, and mpcqp_solve_model_batch with MPCQP_OPT_ON_CHIP_32): the
// reference's build-once usage (mpc_qp.py:129-163, update_cost_vector / update_constraint_vector). Build, elimination and
// triangular product are replaced by loads from what mpcqp_factor_model wrote and a few short products with its linear maps
// (h = e - Hx x0, w = Wx x0 - Wg goal - Wt targets); nx and the number of rows per step are run-time numbers there (NX is not
// read), and the bounds e come per problem or from the model. From `int status = MPCQP_MAX_ITER` on both modes run the same
// statements.
//
// QP given (NX = 0, MODEL = false; mpcqp_solve_batch with MPCQP_OPT_ON_CHIP_32): the dense strictly convex QPs that replace
// qpsolvers.solve_problem at qpmpc/solve_mpc.py:43, 1 <= n <= 32 and 1 <= m <= 64, packed per problem. The build is replaced by
// loads: P, then the rows of G, come through the 32-row image to the lanes that own them, padded as the fused build pads
// (identity rows and columns of P beyond n, zero rows and columns of G); elimination, triangular product and everything after
// them are the fused mode's statements. P is read in full and taken as symmetric. Figures: profiles/onchip32_qp.md.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mpcqp.h"
#include "mpcqp_internal.h"
#include "mpcqp_lane.h"

namespace mpcqp {

namespace duo {

constexpr int NV = 32;    // padded number of variables / slots = lanes per problem
constexpr int MMAX = 64;  // constraints a half can hold (two per lane)
constexpr int LDG = 34;   // row stride of the G and L^-T images (272 B: every row starts 16-byte aligned)
constexpr int LDW = 33;   // row stride of the column-sum scratch (odd: columns are read without bank conflicts)
constexpr double DEP = 1e-14;  // |z|^2 / |M_p|^2 below this: M_p depends on the active rows

struct Lay {      // LDS carve of ONE problem in doubles (host-computed, passed by value)
    int off_X;    // build: G image 32 x LDG | from the factorisation on: rows of L^-T 32 x LDG
    int off_W;    // build: staged operands, then the Gram exchange NX x 32 | main: column-sum scratch 32 x LDW
    int off_v;    // hv (64), y0v, zv, kAv, rv (32 each), mpv (32 + 4)
    int nA, nB, nC, nD;
    int per;      // doubles per problem (the second half's carve starts here)
};

// all-reduce (min) over the 32 lanes of each half
__device__ __forceinline__ unsigned half_min(unsigned v)
{
    v = min(v, dpp<ROR8>(v));
    v = min(v, dpp<ROR4>(v));
    v = min(v, dpp<ROR2>(v));
    v = min(v, dpp<ROR1>(v));
    // rows 1 and 3 of the first operand are exchanged with rows 0 and 2 of the second
    const auto sw = __builtin_amdgcn_permlane16_swap(v, v, false, false);
    return min((unsigned)sw[0], (unsigned)sw[1]);
}
// value of lane `idx` (0..31; may differ from lane to lane) of the caller's own half
__device__ __forceinline__ int half_get(int x, int hb, int idx) { return __builtin_amdgcn_ds_bpermute((hb + idx) << 2, x); }
__device__ __forceinline__ double half_get(double x, int hb, int idx)
{
    const int a = (hb + idx) << 2;
    const int lo = __builtin_amdgcn_ds_bpermute(a, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(a, __double2hiint(x));
    return __hiloint2double(hi, lo);
}
// per-constraint value of row `row` (0..63): x0 of lane row for the first 32 rows, x1 of lane row - 32 beyond
__device__ __forceinline__ double row_get(double x0, double x1, int hb, int row)
{
    const double a = half_get(x0, hb, row & 31), b = half_get(x1, hb, row & 31);
    return row < 32 ? a : b;
}
// true in every lane of a half iff `pred` holds in one of its lanes
__device__ __forceinline__ bool half_any(bool pred, int hb) { return ((unsigned)(__ballot(pred) >> hb)) != 0u; }

__device__ __forceinline__ void ld32(double (&d)[NV], const double *src)
{
    const double2 *p = reinterpret_cast<const double2 *>(src);
#pragma unroll
    for (int i = 0; i < NV / 2; ++i) {
        const double2 t = p[i];
        d[2 * i] = t.x;
        d[2 * i + 1] = t.y;
    }
}
__device__ __forceinline__ void st32(double *dst, const double (&s)[NV])
{
    double2 *p = reinterpret_cast<double2 *>(dst);
#pragma unroll
    for (int i = 0; i < NV / 2; ++i) p[i] = double2{s[2 * i], s[2 * i + 1]};
}
__device__ __forceinline__ double dot32(const double (&a)[NV], const double (&b)[NV])
{
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll
    for (int k = 0; k < NV; k += 4) {
        acc0 += a[k] * b[k];
        acc1 += a[k + 1] * b[k + 1];
        acc2 += a[k + 2] * b[k + 2];
        acc3 += a[k + 3] * b[k + 3];
    }
    return (acc0 + acc1) + (acc2 + acc3);
}
// sum over the lanes l of the caller's half of x_l[k], returned in lane k: the vectors go through the scratch image by rows
// and come back by columns (a fixed order of summation)
__device__ __forceinline__ double half_colsum(const double (&x)[NV], double *W, int hl)
{
    wave_sync();
#pragma unroll
    for (int k = 0; k < NV; ++k) W[hl * LDW + k] = x[k];
    wave_sync();
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int l = 0; l < NV; l += 4) {
        a0 += W[l * LDW + hl];
        a1 += W[(l + 1) * LDW + hl];
        a2 += W[(l + 2) * LDW + hl];
        a3 += W[(l + 3) * LDW + hl];
    }
    return (a0 + a1) + (a2 + a3);
}

}  // namespace duo

using namespace duo;

template <int NX, bool MODEL>
__global__ void __launch_bounds__(64, 1)
    mpcqp_duo_kernel(const double *__restrict__ gA, const double *__restrict__ gB, const double *__restrict__ gC,
                     const double *__restrict__ gD, const double *__restrict__ ge, const double *__restrict__ gx0,
                     const double *__restrict__ ggoal, const double *__restrict__ gtgt, double *__restrict__ oU,
                     double *__restrict__ olam, int32_t *__restrict__ ostatus, int32_t *__restrict__ oiters,
                     const KernelArgs ka, const Lay L, const int64_t batch)
{
    using T = double;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int hb = lane & 32;  // first lane of this half
    const int hl = lane & 31;  // lane inside the half
    int64_t prob = 2 * (int64_t)blockIdx.x + (hb >> 5);
    const bool valid = prob < batch;  // an odd batch leaves the last half idle: it repeats the last problem, stores nothing
    prob = valid ? prob : batch - 1;
    T *sm = (T *)smem_raw + (hb ? L.per : 0);
    const int n = ka.n, m = ka.m;
    const bool isc0 = hl < m, isc1 = hl + 32 < m;  // this lane's two constraints
    const T INF = HUGE_VAL;
    T *Gimg = sm + L.off_X, *LTimg = sm + L.off_X;
    T *Wimg = sm + L.off_W;
    T *hv = sm + L.off_v, *y0v = hv + MMAX, *zv = y0v + NV, *kAv = zv + NV, *rv = kAv + NV, *mpv = rv + NV;
    T *cb = zv;  // the factorisation's two column buffers (zv and kAv, adjacent, are not in use yet)

    T RM0[NV], RM1[NV];
    T Pr[NV];  // row hl of P
    T qa = T(0);
    T h0, h1;
    bool notpd = false;
    T y0m = T(0);  // MODEL: y0 = -w of this lane
    constexpr bool QP = !MODEL && NX == 0;  // the QP is given: P, q, G, h in the first four operand slots
    // ---------------------------------------------------------------- shared model (mpc_qp.py:129-163 on a factored model)
    // What mpcqp_factor_model wrote replaces the build, the elimination and the triangular product: the rows of M and of L^-T
    // are loaded (row stride n, which may be odd: no 16-byte loads), h = e - Hx x0 and w = Wx x0 - Wg goal - Wt targets come from
    // the model's linear maps against the problem's x0, goal and targets, staged once per half in the scratch image.
    if constexpr (MODEL) {
        const T *model = gA;
        const int nxr = ka.nx, nT = ka.N * ka.nx, mk = ka.mk;
        const ModelLayout ml = make_model_layout(nxr, ka.N, n, m);
        const T *x0 = gx0 + prob * ka.x0.batch_stride;
        const T *goal = ggoal ? ggoal + prob * ka.goal.batch_stride : nullptr;
        const T *tgt = gtgt ? gtgt + prob * ka.targets.batch_stride : nullptr;
        const bool termQ = (ka.flags & MPCQP_Q_TERMINAL) && goal, stageQ = (ka.flags & MPCQP_Q_STAGE) && tgt;
        notpd = model[ml.total] != T(0);
        auto al4 = [](int c) { return (c + 3) & ~3; };  // as make_lay
        T *xs = Wimg, *gs = xs + al4(nxr), *ts = gs + al4(nxr);
        for (int i = hl; i < nxr; i += NV) {
            xs[i] = x0[i];
            gs[i] = termQ ? goal[i] : T(0);
        }
        if (stageQ)
            for (int i = hl; i < nT; i += NV) ts[i] = tgt[i];
        const bool col = hl < n;
        const int c1 = hl + 32;
        // rows hl and 32 + hl of M: a lane without a row reads row 0 and keeps zeros, a column beyond n repeats column n - 1
        // and keeps a zero (no load leaves the model, no branch on the lane)
        {
            const T *p0 = model + ml.off_M + (size_t)(isc0 ? hl : 0) * n;
            const T *p1 = model + ml.off_M + (size_t)(isc1 ? c1 : 0) * n;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int kc = k < n ? k : n - 1;
                const T a = p0[kc], b = p1[kc];
                RM0[k] = (isc0 && k < n) ? a : T(0);
                RM1[k] = (isc1 && k < n) ? b : T(0);
            }
        }
        // row hl of L^-T into its image; rows and columns beyond n are the identity (a lane without a variable keeps u = 0)
        {
            const T *pl = model + ml.off_LinvT + (size_t)(col ? hl : 0) * n;
            T lt[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int kc = k < n ? k : n - 1;
                const T a = pl[kc];
                lt[k] = (col && k < n) ? a : ((hl == k) ? T(1) : T(0));
            }
            st32(LTimg + hl * LDG, lt);
        }
        const T e0 = !isc0 ? INF : ge ? ge[prob * ka.e.batch_stride + (hl / mk) * ka.e.step_stride + (hl % mk)] : model[ml.off_e + hl];
        const T e1 = !isc1 ? INF : ge ? ge[prob * ka.e.batch_stride + (c1 / mk) * ka.e.step_stride + (c1 % mk)] : model[ml.off_e + c1];
        wave_sync();  // (x0, goal and targets are staged)
        // h_i = e_i - Hx_i . x0
        {
            const T *hx0 = model + ml.off_Hx + (size_t)(isc0 ? hl : 0) * nxr;
            const T *hx1 = model + ml.off_Hx + (size_t)(isc1 ? c1 : 0) * nxr;
            T a0 = T(0), a1 = T(0);
            for (int c = 0; c < nxr; ++c) {
                const T xc = xs[c];
                a0 += hx0[c] * xc;
                a1 += hx1[c] * xc;
            }
            h0 = isc0 ? e0 - a0 : INF;
            h1 = isc1 ? e1 - a1 : INF;
        }
        // w_k = Wx_k . x0 - Wg_k . goal - Wt_k . targets, lane k walking its own rows (the staged vectors are broadcast reads);
        // the long product over the targets runs in four chains
        {
            const size_t row = col ? hl : 0;
            const T *wx = model + ml.off_Wx + row * nxr, *wg = model + ml.off_Wg + row * nxr, *wt = model + ml.off_Wt + row * nT;
            T wk = T(0);
            for (int c = 0; c < nxr; ++c) wk += wx[c] * xs[c];
            if (termQ)
                for (int c = 0; c < nxr; ++c) wk -= wg[c] * gs[c];
            if (stageQ) {
                T t0 = T(0), t1 = T(0), t2 = T(0), t3 = T(0);
                int j = 0;
                for (; j + 4 <= nT; j += 4) {
                    t0 += wt[j] * ts[j];
                    t1 += wt[j + 1] * ts[j + 1];
                    t2 += wt[j + 2] * ts[j + 2];
                    t3 += wt[j + 3] * ts[j + 3];
                }
                for (; j < nT; ++j) t0 += wt[j] * ts[j];
                wk -= (t0 + t1) + (t2 + t3);
            }
            y0m = col ? -wk : T(0);  // y0 = -w
        }
        wave_sync();  // (the staged vectors are read: the scratch image is free again; the L^-T image is written)
    }
    // ---------------------------------------------------------------- QP given (the call at solve_mpc.py:43)
    // Packed P [n n], q [n], G [m n], h [m] of this problem. The 32 lanes of the half read 32 consecutive elements of a row
    // (n may be odd: 8-byte loads), row after row with no index to divide, into the 32-row image; then every lane takes its own
    // row from there: P, G rows 0 .. 31, G rows 32 .. 63 (the fused build's flush). A lane without a column repeats column n - 1, a
    // row beyond the last one repeats the last one, and both keep the padding value: no load leaves the problem's arrays.
    if constexpr (QP) {
        const T *Pg = gA + prob * (int64_t)(n * n), *qg = gB + prob * (int64_t)n;
        const T *Gg = gC + prob * (int64_t)(m * n), *hg = gD + prob * (int64_t)m;
        const bool col = hl < n;
        const int cc = col ? hl : n - 1;
        const int c1 = hl + 32;
        // (all the loads of a stage are issued before its first store to the image)
        auto stage = [&](const T *src, int rows, int first, bool ident) {
            T t[NV];
#pragma unroll
            for (int r = 0; r < NV; ++r) {
                const int rr = first + r < rows ? first + r : rows - 1;
                t[r] = src[(size_t)rr * n + cc];
            }
#pragma unroll
            for (int r = 0; r < NV; ++r) {
                const T pad = (ident && hl == r) ? T(1) : T(0);
                Gimg[r * LDG + hl] = (col && first + r < rows) ? t[r] : pad;
            }
        };
        auto take = [&](T (&dst)[NV]) {
            wave_sync();
            ld32(dst, Gimg + hl * LDG);
            wave_sync();
        };
        stage(Pg, n, 0, true);
        const T qv = qg[cc];
        const T hv0 = hg[isc0 ? hl : m - 1], hv1 = hg[isc1 ? c1 : m - 1];
        take(Pr);
        stage(Gg, m, 0, false);
        take(RM0);
        if (m > 32) {
            stage(Gg, m, 32, false);
            take(RM1);
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) RM1[k] = T(0);
        }
        qa = col ? qv : T(0);
        h0 = isc0 ? hv0 : INF;
        h1 = isc1 ? hv1 : INF;
    }
    // ---------------------------------------------------------------- build (mpc_qp.py:53-114)
    if constexpr (!MODEL && !QP) {
        constexpr int nx = NX;
        const int nu = ka.nu, N = ka.N, mk = ka.mk;
        const T *A = gA + prob * ka.A.batch_stride;
        const T *B = gB + prob * ka.B.batch_stride;
        const T *Cm = gC ? gC + prob * ka.C.batch_stride : nullptr;
        const T *Dm = gD ? gD + prob * ka.D.batch_stride : nullptr;
        const T *x0 = gx0 + prob * ka.x0.batch_stride;
        const T *goal = ggoal ? ggoal + prob * ka.goal.batch_stride : nullptr;
        const T *tgt = gtgt ? gtgt + prob * ka.targets.batch_stride : nullptr;
        const int sA = ka.A.step_stride ? nx * nx : 0, sB = ka.B.step_stride ? nx * nu : 0;
        const int sC = ka.C.step_stride ? mk * nx : 0, sD = ka.D.step_stride ? mk * nu : 0;
        const bool stageP = ka.flags & MPCQP_P_STAGE, stageQ = (ka.flags & MPCQP_Q_STAGE) && tgt;
        const bool termP = ka.flags & MPCQP_P_TERMINAL, termQ = (ka.flags & MPCQP_Q_TERMINAL) && goal;
        auto al4 = [](int c) { return (c + 3) & ~3; };  // as make_lay: every staged array starts 16-byte aligned
        T *As = Wimg, *Bs = As + al4(L.nA), *Cs = Bs + al4(L.nB), *Ds = Cs + al4(L.nC), *ex = Ds + al4(L.nD);
        // the problem's operands are staged in LDS by the 32 lanes of its half: one coalesced pass, a single HBM latency
        for (int i = hl; i < L.nA; i += NV) As[i] = A[i];
        for (int i = hl; i < L.nB; i += NV) Bs[i] = B[i];
        for (int i = hl; i < L.nC; i += NV) Cs[i] = Cm[i];
        for (int i = hl; i < L.nD; i += NV) Ds[i] = Dm[i];
        const bool col = hl < n;
        const int j = col ? hl / nu : -1, ii = col ? hl - j * nu : 0;
        const int c1 = hl + 32;
        const T e0 = isc0 ? ge[prob * ka.e.batch_stride + (hl / mk) * ka.e.step_stride + (hl % mk)] : INF;
        const T e1 = isc1 ? ge[prob * ka.e.batch_stride + (c1 / mk) * ka.e.step_stride + (c1 % mk)] : INF;
        T v[NX], vx[NX], gref[NX];  // column hl of Psi_k ; Phi_k x0 (the same in every lane) ; the goal
#pragma unroll
        for (int s = 0; s < NX; ++s) {
            v[s] = T(0);
            vx[s] = x0[s];
            gref[s] = termQ ? goal[s] : T(0);
        }
        const T wu = (T)ka.wu;
#pragma unroll
        for (int b = 0; b < NV; ++b) {
            Pr[b] = (hl == b) ? (col ? wu : T(1)) : T(0);
            RM0[b] = T(0);
        }
#pragma unroll
        for (int k = 0; k < LDG / 2; ++k) reinterpret_cast<double2 *>(Gimg + hl * LDG)[k] = double2{0.0, 0.0};  // (see flush)
        wave_sync();
        T bcol[NX];  // this lane's column of B_j (enters the chain at step j)
#pragma unroll
        for (int r = 0; r < NX; ++r) bcol[r] = col ? Bs[j * sB + r * nu + ii] : T(0);

        // Gram accumulation of one block: Pr[b] += w v_a . v_b, qa += w v_a . (Phi_k x0 - ref)
        auto gram = [&](T w, bool useP, bool useQ, const T (&ref)[NX]) {
            if (!useP && !useQ) return;
            if (useP) {
                wave_sync();
#pragma unroll
                for (int s = 0; s < NX; ++s) ex[s * NV + hl] = v[s];
                wave_sync();
            }
#pragma unroll
            for (int s = 0; s < NX; ++s) {
                const T t = w * v[s];
                if (useP) {
                    T vb[NV];
                    ld32(vb, ex + s * NV);
#pragma unroll
                    for (int b = 0; b < NV; ++b) Pr[b] += t * vb[b];
                }
                if (useQ) qa += t * (vx[s] - ref[s]);
            }
        };
        // The G image holds 32 rows. flush(): its rows go to the lanes that own them, and the image is cleared again, so that a
        // row nobody writes is zero (a lane without a constraint then holds a zero row: no selects on the register rows, which
        // the compiler would carry through the elimination below).
        auto clear_image = [&]() {
#pragma unroll
            for (int k = 0; k < LDG / 2; ++k) reinterpret_cast<double2 *>(Gimg + hl * LDG)[k] = double2{0.0, 0.0};
        };
        auto flush = [&](T (&dst)[NV]) {
            wave_sync();
            ld32(dst, Gimg + hl * LDG);
            wave_sync();
            clear_image();
            wave_sync();
        };
        // G rows of step k from v = Psi_k[:, hl]: lane hl fills column hl of the image, lane 0 the C_k Phi_k x0 part of h
        // (mpc_qp.py:62-78). The image holds 32 rows: when row 32 arrives the first 32 go to their lanes.
        auto g_rows = [&](int k) {
            const bool here = (j == k);
            for (int i2 = 0; i2 < mk; ++i2) {
                const int row = k * mk + i2;
                T acc = T(0), accx = T(0);
                if (L.nC) {
                    const T *Ci = Cs + k * sC + i2 * nx;  // broadcast LDS reads
#pragma unroll
                    for (int s = 0; s < NX; ++s) {
                        acc += Ci[s] * v[s];
                        accx += Ci[s] * vx[s];
                    }
                }
                if (L.nD) {
                    const T dv = Ds[k * sD + i2 * nu + ii];
                    acc += here ? dv : T(0);
                }
                if (row == 32) flush(RM0);
                Gimg[(row & 31) * LDG + hl] = acc;
                if (hl == 0) hv[row] = accx;
            }
        };
        // Psi_{k+1} = A_k Psi_k, then column block k <- B_k (mpc_qp.py:88-90); Phi_{k+1} x0 = A_k Phi_k x0
        auto advance = [&](int k) {
            const T *Ak = As + k * sA;
            const bool here = (j == k);
            T w[NX], wx2[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                T acc = T(0), accx = T(0);
#pragma unroll
                for (int s = 0; s < NX; ++s) {
                    acc += Ak[r * nx + s] * v[s];
                    accx += Ak[r * nx + s] * vx[s];
                }
                w[r] = acc;
                wx2[r] = accx;
            }
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                v[r] = here ? bcol[r] : w[r];
                vx[r] = wx2[r];
            }
        };
        for (int k = 0; k < N; ++k) {
            g_rows(k);
            if (k >= 1 && (stageP || stageQ)) {
                T tref[NX];
#pragma unroll
                for (int s = 0; s < NX; ++s) tref[s] = stageQ ? tgt[k * nx + s] : T(0);
                gram((T)ka.wx, stageP, stageQ, tref);
            }
            advance(k);
        }
        gram((T)ka.wt, termP, termQ, gref);  // v = Psi_N
        if (m <= 32) flush(RM0);
        flush(RM1);  // (the rows behind the first 32, or a cleared image)
        h0 = isc0 ? e0 - hv[hl] : INF;  // h_i = e_i - C_k Phi_k x0
        h1 = isc1 ? e1 - hv[c1] : INF;
        qa = col ? qa : T(0);
        wave_sync();
    }

    // ------------------------------------------------------------ factorise, rows of L^-T, M = G L^-T
    // Right-looking: in step j, column j of the trailing matrix (lane k: P[k][j] = L[k][j] L[j][j]) is broadcast through a
    // double-buffered LDS vector, and a row x becomes x_j / L[j][j], x_k -= (x_j / piv) P[k][j] for k > j -- the Cholesky
    // update for the rows of P, the forward substitution x L^-T for the rows of the identity.
    if constexpr (!MODEL) {
        T LT[NV];  // row hl of the identity -> of L^-T
#pragma unroll
        for (int k = 0; k < NV; ++k) LT[k] = (hl == k) ? T(1) : T(0);
        T pmin = T(1);  // QP: the smallest pivot so far, -1 behind one that is not positive
        cb[hl] = Pr[0];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            wave_sync();
            const T *cbj = cb + (j & 1) * NV;
            T cv[NV];
#pragma unroll
            for (int g = j / 2; g < NV / 2; ++g) {
                const double2 t = reinterpret_cast<const double2 *>(cbj)[g];
                cv[2 * g] = t.x;
                cv[2 * g + 1] = t.y;
            }
            const T piv = cv[j];
            if constexpr (QP)  // (one running minimum instead of 32 pivots kept for 32 comparisons behind the triangular product)
                pmin = fmin(pmin, piv > T(0) ? piv : T(-1));
            else if (!(piv > T(0)))
                notpd = true;
            const T rinv = rsqrt(piv);
            const T ri2 = rinv * rinv;
            const T tP = Pr[j] * ri2, tL = LT[j] * ri2;
            if (j + 1 < NV) {
                Pr[j + 1] -= tP * cv[j + 1];
                (cb + ((j + 1) & 1) * NV)[hl] = Pr[j + 1];
            }
#pragma unroll
            for (int k = j + 1; k < NV; ++k) {
                if (k > j + 1) Pr[k] -= tP * cv[k];
                LT[k] -= tL * cv[k];
            }
            // (element j of the row of L^-T is final: it leaves for the image here, so that every step's updates are used inside
            // the loop)
            LTimg[hl * LDG + j] = LT[j] * rinv;
            __builtin_amdgcn_sched_barrier(0);  // (a step's updates finish before the next column arrives: register pressure)
        }
        if constexpr (QP) notpd = !(pmin > T(0));
    }
    wave_sync();
    // M_i = G_i L^-T: row l of L^-T (zero before column l) is broadcast from its image, once for both rows of a lane
    if constexpr (!MODEL) {
        T g0[NV], g1[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            g0[k] = RM0[k];
            g1[k] = RM1[k];
            RM0[k] = T(0);
            RM1[k] = T(0);
        }
#pragma unroll
        for (int l = 0; l < NV; ++l) {
            T row[NV];
#pragma unroll
            for (int g = l / 2; g < NV / 2; ++g) {
                const double2 t = reinterpret_cast<const double2 *>(LTimg + l * LDG)[g];
                row[2 * g] = t.x;
                row[2 * g + 1] = t.y;
            }
#pragma unroll
            for (int k = l; k < NV; ++k) {
                RM0[k] += g0[l] * row[k];
                RM1[k] += g1[l] * row[k];
            }
            if ((l & 3) == 3) __builtin_amdgcn_sched_barrier(0);
        }
    }
    // |M_i|^2 at once, and into LDS: a store keeps both products in this block -- left to itself the compiler sinks the second
    // row's below the first use of the first one's and spills every broadcast row of L^-T on the way (4 KB of scratch)
    const T nn0 = dot32(RM0, RM0), nn1 = dot32(RM1, RM1);
    mpv[hl] = nn0 + nn1;
    rv[hl] = qa;
    wave_sync();
    // y0 = -w, w = L^-1 q: w_k = sum_l q_l (L^-T)[l][k]
    T y0k;
    if constexpr (MODEL) {
        y0k = y0m;
    } else {
        T qq[NV];
        ld32(qq, rv);
        T a0 = T(0), a1 = T(0);
#pragma unroll
        for (int l = 0; l < NV; l += 2) {
            a0 += qq[l] * LTimg[l * LDG + hl];
            a1 += qq[l + 1] * LTimg[(l + 1) * LDG + hl];
        }
        y0k = -(a0 + a1);
    }
    y0v[hl] = y0k;
    kAv[hl] = T(0);
    zv[hl] = T(0);
    wave_sync();

    int status = MPCQP_MAX_ITER, iters = 0;
    T xsol = T(0), lam0_out = T(0), lam1_out = T(0);
    bool done = notpd;      // this half has left the active-set loop
    bool finished = notpd;  // ... and needs no refinement any more (failed, or accepted)
    if (notpd) status = MPCQP_NOT_PD;

    T RT[NV], RH[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        RT[k] = T(0);                       // T = N* starts empty
        RH[k] = (hl == k) ? T(1) : T(0);    // H = I
    }
    T s0, s1;
    {
        T y0[NV];
        ld32(y0, y0v);
        s0 = isc0 ? h0 - dot32(RM0, y0) : INF;
        s1 = isc1 ? h1 - dot32(RM1, y0) : INF;
    }
    // Selection rule (the classic Goldfarb-Idnani one): among the rows violated beyond the tolerance, the one FARTHEST from
    // its hyperplane in the P^-1 metric, s_i / |M_i|.
    T invn0, invn1;
    invn0 = (nn0 > T(0)) ? rsqrt(nn0) : T(1);
    invn1 = (nn1 > T(0)) ? rsqrt(nn1) : T(1);
    const bool sel0 = isc0 && (h0 < T(1e29)), sel1 = isc1 && (h1 < T(1e29));
    const T tol = (T)ka.tol;
    const T tolh0 = tol + tol * fabs(h0), tolh1 = tol + tol * fabs(h1);  // row i is violated when s_i < -tol (1 + |h_i|)
    const int max_iter = ka.max_iter;

    T lam = T(0);       // slot hl: its multiplier
    int myact = 0;      // slot hl: the constraint it holds
    bool occ = false;   // slot hl: occupied
    int pos0 = -1, pos1 = -1;  // constraints hl, 32 + hl: their slot, or -1
    // half-uniform state
    int nq = 0, p = 0, ldrop = 0, fails = 0;
    unsigned mask = 0;  // occupied slots
    bool needp = true, dropping = false;
    T up = T(0);

    for (;;) {
        // ===================================================== active-set loop
        for (;;) {
            // ---- selection, for the halves that start a new constraint
            {
                // a violated row's scaled slack is negative: the order of the magnitudes is the order of the high words, so
                // the most violated row has the smallest complement
                const bool want = needp & !done;
                const unsigned hi0 = ~(unsigned)__double2hiint(s0 * invn0), hi1 = ~(unsigned)__double2hiint(s1 * invn1);
                const bool v0 = want & sel0 & (pos0 < 0) & (s0 < -tolh0), v1 = want & sel1 & (pos1 < 0) & (s1 < -tolh1);
                const unsigned k0 = v0 ? ((hi0 & ~63u) | (unsigned)hl) : 0xffffffffu;
                const unsigned k1 = v1 ? ((hi1 & ~63u) | (unsigned)(hl + 32)) : 0xffffffffu;
                const unsigned mkey = half_min(min(k0, k1));
                const bool none = want & (mkey == 0xffffffffu);
                const bool got = want & !none;
                done = done | none;
                status = none ? (int)MPCQP_SOLVED : status;
                p = got ? (int)(mkey & 63u) : p;
                up = got ? T(0) : up;
                needp = needp & !got;
            }
            if (__ballot(!done) == 0ull) break;
            bool stepping = !done && !dropping;
            const bool drp = !done && dropping;
            if (stepping && iters >= max_iter) {
                done = finished = true;
                status = MPCQP_MAX_ITER;
                stepping = false;
            }
            iters += stepping ? 1 : 0;
            // ---- row p of M, its slack and 1 / |M_p| from the lane that owns it
            wave_sync();
            if (stepping && hl == (p & 31)) {
                const bool lo = p < 32;
                T row[NV];
#pragma unroll
                for (int k = 0; k < NV; ++k) row[k] = lo ? RM0[k] : RM1[k];
                st32(mpv, row);
                mpv[NV] = lo ? s0 : s1;
                mpv[NV + 1] = lo ? invn0 : invn1;
            }
            wave_sync();
            T rd, zl;
            {
                T mp[NV];
                ld32(mp, mpv);
                rd = dot32(RT, mp);    // r_a = T_a . M_p
                zl = -dot32(RH, mp);   // z = -H M_p
            }
            const T sp = mpv[NV], ip = mpv[NV + 1];
            if (stepping) zv[hl] = zl;
            wave_sync();
            // ---- the vector of this trip's pass over the register rows: z, or the leaving row T_l (left in kAv)
            T vv[NV];
            ld32(vv, drp ? kAv : zv);
            const T dd = dot32(vv, vv);  // |z|^2 from z itself ; |T_l|^2
            const T mz0 = dot32(RM0, vv), mz1 = dot32(RM1, vv);
            // ---- step length
            const bool can_move = (nq < n) & (dd * ip * ip > T(DEP)) & (dd > T(0));
            const T inv = (stepping & can_move) ? fast_rcp(dd) : T(0);
            const T t2 = can_move ? -sp * inv : INF;
            const int sl = (int)__builtin_ctz(~mask);  // lowest free slot (nq < n <= 32 whenever it is used)
            const T r = (occ && stepping) ? rd : T(0);
            const bool cand = occ && (r > T(0));
            // a blocking multiplier exists iff lam_a / r_a < t2 for some slot
            const bool blocked = half_any(stepping && cand && (lam < t2 * r), hb);
            T t1 = INF;
            int l = 0;
            if (__ballot(blocked) != 0ull) {  // ratio test on the multipliers
                const T ratio = cand ? lam * fast_rcp(r) : INF;
                unsigned hi, lo;
                ordered(ratio, hi, lo);
                hi = cand ? hi : 0xffffffffu;
                const unsigned mhi = half_min(hi);
                const unsigned k2 = (cand && hi == mhi) ? ((lo & ~31u) | (unsigned)hl) : 0xffffffffu;
                const unsigned ml = half_min(k2);
                l = (int)(ml & 31u);
                const T tl1 = half_get(ratio, hb, l);
                t1 = (blocked && mhi != 0xffffffffu) ? tl1 : INF;
            }
            T t = t1 < t2 ? t1 : t2;
            if (stepping && !(t < INF)) {  // no step possible: the constraints are inconsistent
                done = finished = true;
                status = MPCQP_INFEASIBLE;
                stepping = false;
            }
            t = stepping ? t : T(0);
            const bool full = stepping && (t2 <= t1);
            // ---- coefficients of the pass: a full step's rank-one update by z, or the removal of slot ldrop
            T cT = T(0), cH = T(0);
            if (full) {
                cT = (hl == sl) ? -inv : r * inv;  // T_a += (r_a/d2) z, T_new = -z/d2 (an empty slot's row is zero, so is r_a)
                cH = -zl * inv;                    // H_k -= (z_k/d2) z
            }
            if (__ballot(drp) != 0ull) {
                // With W = T T' implicit, T_a -= (T_a . T_l / T_l . T_l) T_l (row l: -1, it becomes exactly zero); the null
                // space of the active rows gains the direction T_l: H += T_l T_l' / T_l . T_l.
                const T tl = dot32(RT, vv);
                const T itl = fast_rcp(dd);
                if (drp) {
                    cT = (hl == ldrop) ? T(-1) : (occ ? -tl * itl : T(0));
                    cH = kAv[hl] * itl;
                }
            }
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                RT[k] += cT * vv[k];
                RH[k] += cH * vv[k];
            }
            // ---- bookkeeping
            if (stepping) {
                // the implied primal point moved by t z: s_i -= t M_i . z
                if (isc0) s0 = (pos0 >= 0) ? T(0) : s0 - t * mz0;
                if (isc1) s1 = (pos1 >= 0) ? T(0) : s1 - t * mz1;
                lam -= t * r;
                lam = (occ && lam < T(0)) ? T(0) : lam;
                up += t;
            }
            if (full) {  // p takes slot sl
                if (hl == sl) {
                    lam = up;
                    myact = p;
                    occ = true;
                }
                if (hl == p) {
                    pos0 = sl;
                    s0 = T(0);
                }
                if (hl + 32 == p) {
                    pos1 = sl;
                    s1 = T(0);
                }
                mask |= 1u << sl;
                ++nq;
                needp = true;
            }
            const bool partial = stepping && !full;
            if (drp) {
                if (hl == ldrop) {
                    lam = T(0);
                    occ = false;
                }
                mask &= ~(1u << ldrop);
                --nq;
                dropping = false;
            }
            if (__ballot(partial) != 0ull) {
                // partial step: the next trip removes slot l from T (this trip's pass left the rows as they were)
                const int cl = half_get(myact, hb, l);
                wave_sync();
                if (partial && hl == l) st32(kAv, RT);
                if (partial) {
                    if (hl == cl) pos0 = -1;
                    if (hl + 32 == cl) pos1 = -1;
                    dropping = true;
                    ldrop = l;
                }
            }
            wave_sync();
        }
        if (__ballot(!finished) == 0ull) break;
        // ================================== multipliers by refinement, slacks re-evaluated
        // (halves that are already finished compute along and change nothing)
        const bool act = !finished;  // (half-uniform; done holds for every half here)
        T yy[NV];
        T fresh0, fresh1;
        auto slacks = [&](T yk) {
            wave_sync();
            zv[hl] = yk;
            wave_sync();
            ld32(yy, zv);
            fresh0 = isc0 ? h0 - dot32(RM0, yy) : INF;
            fresh1 = isc1 ? h1 - dot32(RM1, yy) : INF;
        };
        // y = y0 - M_A' lam, summed over the constraint lanes' rows
        T y;
        {
            const T lc0 = half_get(lam, hb, pos0 < 0 ? 0 : pos0), lc1 = half_get(lam, hb, pos1 < 0 ? 0 : pos1);
            const T a0 = pos0 >= 0 ? lc0 : T(0), a1 = pos1 >= 0 ? lc1 : T(0);
            T x[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) x[k] = a0 * RM0[k] + a1 * RM1[k];
            y = y0k - half_colsum(x, Wimg, hl);
        }
        slacks(y);
        // active residuals rho_a = h_a - M_a y should vanish: dlam = -W rho_A = -T (T' rho_A), one step
        {
            T rho = row_get(fresh0, fresh1, hb, myact);
            rho = occ ? rho : T(0);
            T x[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) x[k] = rho * RT[k];
            const T uk = half_colsum(x, Wimg, hl);  // (T' rho)_k
            wave_sync();
            rv[hl] = uk;
            wave_sync();
            T uu[NV];
            ld32(uu, rv);
            T dl = -dot32(RT, uu);
            dl = occ ? dl : T(0);
            if (act && nq > 0) {
                const T lraw = lam + dl;
                lam = (occ && lraw < T(0)) ? T(0) : lraw;
                // y - M_A' dl = y + M_A' T (T' rho) = y + T' rho, because T' rho lies in the range of M_A' where M_A' T = I - H
                // is the identity
                y += uk;
            }
        }
        slacks(y);
        // ---- acceptance: no inactive row violated, every active row on its bound, no negative multiplier -- with
        //      stationarity by construction these are the KKT conditions of the strictly convex QP
        bool dirty = half_any((sel0 && pos0 < 0 && !(fresh0 >= -T(4) * tolh0)) || (sel1 && pos1 < 0 && !(fresh1 >= -T(4) * tolh1)), hb);
        {
            const T ra = row_get(fresh0, fresh1, hb, myact);
            const T ta = row_get(tolh0, tolh1, hb, myact);
            const bool off = half_any(occ && !(fabs(ra) <= T(1e3) * ta), hb);
            const bool neg = half_any(occ && !(lam >= T(0)), hb);
            dirty = dirty || off || neg;
        }
        if (act) {
            if (!dirty || ++fails >= 4) {
                // u = L^-T y (yy holds y; the rows of L^-T come back from their image)
                T lt[NV];
                ld32(lt, LTimg + hl * LDG);
                xsol = dot32(lt, yy);
                status = dirty ? MPCQP_MAX_ITER : MPCQP_SOLVED;
                finished = true;
            } else {
                // continue the active-set loop from the re-evaluated slacks
                s0 = (pos0 >= 0) ? T(0) : fresh0;
                s1 = (pos1 >= 0) ? T(0) : fresh1;
                status = MPCQP_MAX_ITER;
                done = false;
                needp = true;
            }
        }
        if (__ballot(!finished) == 0ull) break;
    }
    if (olam) {
        const T l0 = half_get(lam, hb, pos0 < 0 ? 0 : pos0), l1 = half_get(lam, hb, pos1 < 0 ? 0 : pos1);
        lam0_out = (pos0 >= 0) ? l0 : T(0);
        lam1_out = (pos1 >= 0) ? l1 : T(0);
    }

    const bool ok = (status == MPCQP_SOLVED);
    if (valid) {
        if (hl < n) oU[prob * (int64_t)n + hl] = ok ? xsol : T(0);
        if (olam && isc0) olam[prob * (int64_t)m + hl] = ok ? lam0_out : T(0);
        if (olam && isc1) olam[prob * (int64_t)m + hl + 32] = ok ? lam1_out : T(0);
        if (hl == 0) {
            if (ostatus) ostatus[prob] = status;
            if (oiters) oiters[prob] = iters;
        }
    }
}

// ------------------------------------------------------------ host side
// model: the carve of a shared-model launch -- no staged operands; x0, goal and the targets (N nx of them) share the scratch image
// qp: the carve of a QP-given launch -- nothing is staged beside the image: the image, the column-sum scratch, the vectors
static Lay make_lay(const KernelArgs &ka, bool model = false, bool qp = false)
{
    Lay L{};
    auto al = [](int c) { return (c + 3) & ~3; };
    L.off_X = 0;
    L.off_W = NV * LDG;
    if (!model && !qp) {
        L.nA = (ka.A.step_stride ? ka.N : 1) * ka.nx * ka.nx;
        L.nB = (ka.B.step_stride ? ka.N : 1) * ka.nx * ka.nu;
        L.nC = ka.C.ptr ? (ka.C.step_stride ? ka.N : 1) * ka.mk * ka.nx : 0;
        L.nD = ka.D.ptr ? (ka.D.step_stride ? ka.N : 1) * ka.mk * ka.nu : 0;
    }
    const int w_build = qp ? 0 : model ? 2 * al(ka.nx) + al(ka.N * ka.nx) : al(L.nA) + al(L.nB) + al(L.nC) + al(L.nD) + ka.nx * NV;
    const int w_main = NV * LDW;
    L.off_v = L.off_W + al(w_build > w_main ? w_build : w_main);
    L.per = al(L.off_v + MMAX + 4 * NV + NV + 4);
    return L;
}

// the envelope of MPCQP_OPT_ON_CHIP_32 (include/mpcqp.h)
bool duo_applies(const KernelArgs &ka)
{
    return ka.n >= 17 && ka.n <= NV && ka.m >= 1 && ka.m <= MMAX && ka.mk >= 1 && ka.mk <= 4 && ka.nx >= 2 && ka.nx <= 4;
}
// ... and of its shared-model mode: the operands' layout no longer matters (any nx, any number of rows per step)
bool duo_model_applies(const KernelArgs &ka) { return ka.n >= 17 && ka.n <= NV && ka.m >= 1 && ka.m <= MMAX && ka.mk >= 1; }
// ... and of its QP-given mode: dense QPs from one variable up (below seventeen they are padded like the last lanes of n = 17)
bool duo_qp_applies(const KernelArgs &ka) { return ka.n >= 1 && ka.n <= NV && ka.m >= 1 && ka.m <= MMAX; }

template <int NX> static int launch_duo_t(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    const Lay L = make_lay(ka);
    const size_t bytes = (size_t)L.per * 2 * sizeof(double);
    const int64_t waves = (batch + 1) / 2;  // one wavefront per workgroup, whatever the batch: they share nothing
    hipLaunchKernelGGL((mpcqp_duo_kernel<NX, false>), dim3((unsigned)waves), dim3(64), bytes, st, (const double *)ka.A.ptr,
                       (const double *)ka.B.ptr, (const double *)ka.C.ptr, (const double *)ka.D.ptr, (const double *)ka.e.ptr,
                       (const double *)ka.x0.ptr, (const double *)ka.goal.ptr, (const double *)ka.targets.ptr, (double *)ka.U,
                       (double *)ka.lam, ka.status, ka.iters, ka, L, batch);
    return (int)hipGetLastError();
}

int launch_duo(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    switch (ka.nx) {
    case 2: return launch_duo_t<2>(ka, batch, st);
    case 3: return launch_duo_t<3>(ka, batch, st);
    default: return launch_duo_t<4>(ka, batch, st);
    }
}

// shared model (ka.model, in the first argument as in the pair and quad kernels; ka.e.ptr: bounds per problem, or null)
int launch_duo_model(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    const Lay L = make_lay(ka, true);
    const size_t bytes = (size_t)L.per * 2 * sizeof(double);  // (38 KB until N nx exceeds 1000: then the targets set the carve)
    if (bytes > kLdsBytesPerCU) return MPCQP_ETOOLARGE;
    auto kern = mpcqp_duo_kernel<0, true>;
    if (bytes > 48 * 1024) (void)hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    const int64_t waves = (batch + 1) / 2;
    hipLaunchKernelGGL(kern, dim3((unsigned)waves), dim3(64), bytes, st, (const double *)ka.model, (const double *)nullptr,
                       (const double *)nullptr, (const double *)nullptr, (const double *)ka.e.ptr, (const double *)ka.x0.ptr,
                       (const double *)ka.goal.ptr, (const double *)ka.targets.ptr, (double *)ka.U, (double *)ka.lam, ka.status,
                       ka.iters, ka, L, batch);
    return (int)hipGetLastError();
}

// QP given (ka.P, ka.q, ka.G, ka.h, packed per problem, in the first four arguments). The carve is the shared-model one without
// its staged vectors (37.1 KB per wavefront): below the 48 KB a launch may ask for without setting a function attribute.
int launch_duo_qp(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    const Lay L = make_lay(ka, false, true);
    const size_t bytes = (size_t)L.per * 2 * sizeof(double);
    static_assert((size_t)(NV * LDG + NV * LDW + MMAX + 5 * NV + 4 + 3) * 2 * sizeof(double) <= 48 * 1024, "the QP carve needs no attribute");
    const int64_t waves = (batch + 1) / 2;
    hipLaunchKernelGGL((mpcqp_duo_kernel<0, false>), dim3((unsigned)waves), dim3(64), bytes, st, (const double *)ka.P,
                       (const double *)ka.q, (const double *)ka.G, (const double *)ka.h, (const double *)nullptr,
                       (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, (double *)ka.U, (double *)ka.lam,
                       ka.status, ka.iters, ka, L, batch);
    return (int)hipGetLastError();
}

}  // namespace mpcqp
