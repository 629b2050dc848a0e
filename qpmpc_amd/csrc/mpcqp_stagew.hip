// mpcqp_stagew.hip -- the stage-wise (uncondensed) formulation for WIDER systems: 2 <= nx <= 16, 1 <= nu <= 4,
// float64 and float32 (BASELINE config 5's dimensions nx = 12, nu = 4 among them).
//
// Same problem, same method and same per-problem data as mpcqp_stage.hip (see there: Goldfarb-Idnani in the metric of
// the condensed Hessian P with P never formed; a product with P^-1 is one LQR solve; qpmpc/mpc_qp.py:39,108-109 and
// qpmpc/solve_mpc.py:31-32 are what it replaces). What differs is how one wavefront handles nx x nx matrices that no
// longer fit a lane's registers:
//   * RICCATI RECURSION: the step's matrices (P, A_k, A_k', P A, A_cl, ...) live in LDS as 16 x 16 tiles and every
//     product runs on the matrix cores (one 16x16x4 MFMA per chunk of 4 of the inner dimension).
//   * SWEEPS of the LQR solve: serial over the horizon and latency-bound, so a step is nothing but a short chain of
//     MFMAs: the costate / state is a 16-vector held the way the matrix cores take a B operand (component 4 q + g in
//     register q of the lanes of row group g), the step's matrix comes from a per-step record the factor wrote in
//     A-operand order (64 consecutive values per MFMA), with its rows permuted so that the product lands in B-operand
//     order again -- no shuffles, no LDS, no barrier between the steps. The matrices are stacked so that one product
//     gives everything a step needs: backward [A_cl' ; -S^-1 B'] p -> (p_k, ff_k); forward [[A_cl, B], [-K, I]] (x, ff)
//     -> (x_{k+1}, u_k). Records are requested D steps ahead into a register ring. The 16 columns of the operand are
//     independent right-hand sides: a sweep pair carries the candidate row AND the R - 1 next most violated ones
//     (V_a = P^-1 g_a' does not depend on the active set, so a later candidate found among them costs no sweep).
//   * S = w_u I + B'PB (nu <= 4) is factored L D L' in registers; lane (., c) solves for column c of K and of -S^-1 B'.
//   * ACTIVE SET: every active row a keeps V_a = P^-1 g_a' (inputs only) and h_a = G V_a (all m rows), so an iteration
//     after the candidate's two sweeps is m-long AXPYs over coalesced arrays: c_a = h_p[row a], slack update
//     s += t (h_p - sum r_a h_a). Slots are addressed through a permutation, nothing is copied when rows enter or leave.
// One wavefront per problem and ~11 KB (f32) of LDS: 12 problems per CU are in flight (168 VGPRs), against ONE for the
// dense large-problem solver (its packed L^-1 fills the LDS). DESIGN.md 3.8 has the measurements.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "mpcqp.h"
#include "mpcqp_internal.h"
#include "mpcqp_lane.h"

namespace mpcqp {

// (build-time knobs of the developer's A/B runs: tools/ab_stagew.sh builds variants of this unit with -D...)
#ifndef STAGEW_D
#define STAGEW_D 4
#endif
#ifndef STAGEW_VTRIG32
#define STAGEW_VTRIG32 8
#endif
#ifndef STAGEW_VACC32
#define STAGEW_VACC32 16
#endif
#ifndef STAGEW_VNOISE32
#define STAGEW_VNOISE32 16
#endif
#ifndef STAGEW_VPASS32
#define STAGEW_VPASS32 3
#endif
#ifndef STAGEW_PDD
#define STAGEW_PDD 2 /* steps ahead of the recursion at which the default instantiations request a step's operands */
#endif
#ifndef STAGEW_QFD
// active rows up to which an iteration of the default float32 instantiations runs on its "small" path (one four-vector of Q per lane and row)
#define STAGEW_QFD 4
#endif
#ifndef STAGEW_MSUMD
#define STAGEW_MSUMD 0
#endif
#ifndef STAGEW_YCU_LATE
#define STAGEW_YCU_LATE 0
#endif
#ifndef STAGEW_WPE32
#define STAGEW_WPE32 3
#endif
#ifndef STAGEW_DBG
#define STAGEW_DBG 0 /* timing experiments only (wrong results): 1 no rows' products in the forward sweep, 2 no record loads in its loop, 4 no group work */
#endif
#ifndef STAGEW_DLOW
#define STAGEW_DLOW 12
#endif
#ifndef STAGEW_RLOW
#define STAGEW_RLOW 12
#endif
#ifndef STAGEW_LDS_PAD
#define STAGEW_LDS_PAD 0
#endif
#ifndef STAGEW_RF
#define STAGEW_RF 7 /* (round 4, with the lazy slacks: 7 -> 1.183 ms, 6 -> 1.198, 8 -> 1.215, 10 -> 1.238, 16 -> 1.309 per 8192 config-5 problems) */
#endif

namespace stagew {

constexpr int NU = 4;   // capacity of the input dimension (register arrays, LDS tiles); nu is a run-time value
constexpr int LD = 17;  // row stride of the 16 x 16 LDS tiles (odd: the MFMA operand reads are conflict-free)
// right-hand sides per BACKWARD sweep (columns of the MFMA B operand): the candidate + R - 1 speculated rows. The matrix cores
// compute all 16 columns whatever their number; a column costs its share of the selection that picks the rows, and the sweep
// starts at the latest of its rows' steps. (The forward sweeps carry ONE vector since round 6: the projected one.)
constexpr int R_PLAIN = 8, R_FUSE = STAGEW_RF;
// LOW (float32, FUSE layout): the instantiation for batches that do not fill the SIMDs -- a launch of at most one wavefront per
// SIMD (the 8-GPU share of config 5: 1024 problems) is bounded by the LATENCY of its longest problem, and the registers of
// the empty wavefront slots buy some of it back: one wavefront per SIMD (512 VGPRs), twelve right-hand sides per backward
// sweep, a six-step request ring.
constexpr int R_FUSE_LOW = STAGEW_RLOW, D_LOW = STAGEW_DLOW;

struct Ws {  // per-problem workspace carve, in elements of T (host-computed, passed by value; 32-bit: scalar registers are short)
    int Mb, Mf, ff, Zs, Gp, s0, s, invn, thr, vpt, ust, junk, Q, W;
    int maxq, mg;
    int64_t total;
};

// a lane's group of L record values (L < 4: packed, so that a step's record has no padding -- 12-byte loads for L = 3)
template <typename T, int L> struct __attribute__((packed, aligned(sizeof(T)))) RecN {
    T v[L];
};
// floats of one step's record with `nv` values per lane: groups of four, or ONE group of nv when nv < 4
inline int64_t rec_elems(int nv) { return nv < 4 ? 64 * nv : (int64_t)((nv + 3) / 4) * 256; }

// FUSE: the constraint matrices C, D do not change along the horizon and have at most 16 rows per step (a multiple of
// four): h = G (x_k, u_k) of a forward sweep is then formed by the sweep itself, on the matrix cores, with [C | D] as a
// constant operand held in registers, and the sweep's own lanes own the rows (slack update, selection): no trajectory is
// written and no pass over the m rows reads it back.
inline bool fuse_ok(int mk, bool ginv) { return ginv && mk <= 16 && (mk & 3) == 0; }

// nxc: nx rounded up to a multiple of 4 (the kernel's compile-time row length)
inline int nxc_of(int nx) { return (nx + 3) & ~3; }

// ginv: C and D do not change along the horizon (their packed copy holds mk rows instead of N mk)
inline Ws make_ws(int nx, int nu, int N, int mk, int maxq, bool ginv, size_t esz, bool low = false)
{
    (void)esz;
    (void)nu;
    Ws w{};
    int64_t o = 0;
    auto take = [&](int64_t cnt) {
        const int64_t at = o;
        o += (cnt + 3) & ~(int64_t)3;
        return (int)at;
    };
    const int nxc = nxc_of(nx);
    const int64_t m = (int64_t)N * mk;
    // per-step records of the sweeps, in MFMA A-operand order: nq (backward) and nq + 1 (forward) chunks of 64 values
    // for each of the na row blocks of the stacked matrix (one when nxc + 4 <= 16)
    // (lane-major, in groups of four values per lane: 256 values per group)
    const int nq = nxc / 4, na = nxc <= 12 ? 1 : 2;
    w.Mb = take((int64_t)N * rec_elems(na * nq));
    w.Mf = take((int64_t)N * rec_elems(na * (nq + 1)));
    const bool fuse = fuse_ok(mk, ginv);
    const int R = fuse ? (low ? R_FUSE_LOW : R_FUSE) : R_PLAIN;
    (void)R;
    w.ff = take((int64_t)16 * N * 4);          // whitened vectors y_a of the latest backward sweep's rows, per column of the operand
    w.Zs = take(fuse ? 0 : (int64_t)N * (nxc + 4));  // (x_k, u_k) of the latest forward sweep, in B-operand order
    w.mg = ginv ? mk : (int)m;
    w.Gp = take(fuse ? 0 : (int64_t)(nxc + 4) * w.mg);  // [C | D] in the order of Zs's rows, as four-vectors: Gp[j][row], j <= nxc / 4
    w.s0 = take(m);    // rows of the latest evaluation of the point (the active rows' residuals)
    w.s = take(m);
    w.invn = take(m);
    w.thr = take(m);
    w.vpt = take((int64_t)N * 4);                   // the point in whitened coordinates
    w.ust = take((int64_t)N * 4);                   // its inputs, as the latest forward sweep left them (rows of 4)
    w.junk = take(64);                              // a cell per lane for the stores of lanes without a row
    w.Q = take((int64_t)(maxq + 1) * N * 4);        // Q by vectors (vector nq: the candidate's projection)
    w.W = take((int64_t)maxq * maxq);               // R by columns, once it has outgrown its LDS tile
    o = (o + 127) & ~(int64_t)127;  // odd multiple of 512 B / 1 KB between problems (memory channels)
    if (((o >> 7) & 1) == 0) o += 128;
    w.total = o;
    w.maxq = maxq;
    return w;
}

template <typename T> struct Tol;
template <> struct Tol<double> { static constexpr double dep = 1e-13; };
template <> struct Tol<float> { static constexpr float dep = 1e-6f; };
// 16 x 16 (+)= 16 x 4 times 4 x 16 on the matrix cores; operands A[lane % 16][lane / 16], B[lane / 16][lane % 16];
// result register t of a lane: column lane % 16, row 4 (lane / 16) + t in float32, (lane / 16) + 4 t in float64
// (checked on MI355X, tools/ note in DESIGN.md).
template <typename T> struct Mfma;
template <> struct Mfma<float> {
    using V = __attribute__((ext_vector_type(4))) float;
    static __device__ __forceinline__ V run(float a, float b, V c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int pg, int t) { return 4 * pg + t; }
    // the row of the stacked matrix an A-operand row must hold for the product to come out in B-operand order
    static __device__ __forceinline__ int rowmap(int i) { return 4 * (i & 3) + (i >> 2); }
};
template <> struct Mfma<double> {
    using V = __attribute__((ext_vector_type(4))) double;
    static __device__ __forceinline__ V run(double a, double b, V c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    static __device__ __forceinline__ int row(int pg, int t) { return pg + 4 * t; }
    static __device__ __forceinline__ int rowmap(int i) { return i; }
};

// sum_c a[c] (x) b[c] (+ init): a chain of products accumulating into one another, or (STAGEW_CHAIN 0) INDEPENDENT products summed
// on the vector pipe. Round 6 measured a sweep step's bare chain of four float32 16x16x4 products at 358 cycles for a lone
// wavefront and tried the independent form: slower everywhere (the sums' twelve vector instructions and the registers cost more
// than the chain's waits).
#ifndef STAGEW_CHAIN
#define STAGEW_CHAIN 1 /* 0: independent products summed on the vector pipe -- measured SLOWER (config 5: 6.35 against 6.61 M/s, Riccati 183 k against 167 k cycles), kept for A/B runs */
#endif
template <typename T, int NCH> __device__ __forceinline__ typename Mfma<T>::V mfma_sum(const T (&a)[NCH], const T (&b)[NCH], typename Mfma<T>::V init)
{
    using MV = typename Mfma<T>::V;
    if constexpr (STAGEW_CHAIN || NCH == 1) {
        MV acc = init;
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc = Mfma<T>::run(a[c], b[c], acc);
        return acc;
    } else {
        const MV zero = {T(0), T(0), T(0), T(0)};
        MV m[NCH];
        m[0] = Mfma<T>::run(a[0], b[0], init);
#pragma unroll
        for (int c = 1; c < NCH; ++c) m[c] = Mfma<T>::run(a[c], b[c], zero);
#pragma unroll
        for (int st = 1; st < NCH; st *= 2)
#pragma unroll
            for (int c = 0; c + st < NCH; c += 2 * st) m[c] += m[c + st];
        return m[0];
    }
}

// C[r][c] = alpha sum_k A[r][k] B[k][c] (+ beta Add[r][c]) on the matrix cores: one MFMA per chunk of 4 along k,
// operands read from LDS tiles with compile-time strides. Tiles are 16 or 4 rows / columns (NR, NC) and ZERO outside
// their valid part, so the products run over the full tile and the padding of the result is zero again; reads past a
// 4-row / 4-column operand land in the neighbouring tiles and only feed results that are not stored.
template <typename T, int LDA, int LDB, int LDC, int NR, int NC, int NK, bool SUB>
__device__ __forceinline__ void mm_t(T *C, const T *A, const T *B, const T *Add, int pg, int c16)
{
    // SUB: C = Add - A B (Add has C's layout), else C = A B
    typename Mfma<T>::V acc = {T(0), T(0), T(0), T(0)};
#pragma unroll
    for (int k = 0; k < NK; k += 4) acc = Mfma<T>::run(A[c16 * LDA + k + pg], B[(k + pg) * LDB + c16], acc);
    if (NC < 16 && c16 >= NC) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int r = Mfma<T>::row(pg, t);
        if (NR == 16 || r < NR) C[r * LDC + c16] = SUB ? Add[r * LDC + c16] - acc[t] : acc[t];
    }
}

// reciprocal square root: hardware estimate + Newton steps
__device__ __forceinline__ float frsq(float x)
{
    const float r = __builtin_amdgcn_rsqf(x);
    return r * fmaf(-0.5f * x * r, r, 1.5f);
}
__device__ __forceinline__ double frsq(double x)
{
    double r = __builtin_amdgcn_rsq(x);
    r = r * fma(-0.5 * x * r, r, 1.5);
    return r * fma(-0.5 * x * r, r, 1.5);
}
// S = L D L' of a symmetric positive definite 4 x 4 (unit lower L): id[i] = 1 / d_i, l = (l10, l20, l30, l21, l31, l32)
template <typename T> struct Ldl4 {
    T id[4], l[6], sd[4];  // (sd[i] = 1 / sqrt(d_i): the whitening scale, S = Ls Ls' with Ls = L D^1/2)
    // returns false when a pivot is not positive (or not a number): S, hence the condensed Hessian, is not positive definite
    __device__ __forceinline__ bool factor(const T (&s)[10])  // s = (s00, s10, s11, s20, s21, s22, s30, s31, s32, s33)
    {
        const T d0 = s[0];
        id[0] = fast_rcp_e_first(d0);
        l[0] = s[1] * id[0];
        l[1] = s[3] * id[0];
        l[2] = s[6] * id[0];
        const T d1 = s[2] - l[0] * s[1];
        id[1] = fast_rcp_e_first(d1);
        const T t21 = s[4] - l[1] * s[1], t31 = s[7] - l[2] * s[1];
        l[3] = t21 * id[1];
        l[4] = t31 * id[1];
        const T d2 = s[5] - l[1] * s[3] - l[3] * t21;
        id[2] = fast_rcp_e_first(d2);
        const T t32 = s[8] - l[2] * s[3] - l[4] * t21;
        l[5] = t32 * id[2];
        const T d3 = s[9] - l[2] * s[6] - l[4] * t31 - l[5] * t32;
        id[3] = fast_rcp_e_first(d3);
        sd[0] = frsq(d0);
        sd[1] = frsq(d1);
        sd[2] = frsq(d2);
        sd[3] = frsq(d3);
        return (d0 > T(0)) & (d1 > T(0)) & (d2 > T(0)) & (d3 > T(0));
    }
    // b <- Ls^-1 b with S = Ls Ls', Ls = L D^1/2 (sid[i] = 1 / sqrt(d_i)): the WHITENING of a stage's input-sized vector
    __device__ __forceinline__ void wsolve(T (&b)[4], const T (&sid)[4]) const
    {
        b[1] -= l[0] * b[0];
        b[2] -= l[1] * b[0] + l[3] * b[1];
        b[3] -= l[2] * b[0] + l[4] * b[1] + l[5] * b[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] *= sid[i];
    }
    __device__ __forceinline__ void solve(T (&b)[4]) const  // b <- S^-1 b
    {
        b[1] -= l[0] * b[0];
        b[2] -= l[1] * b[0] + l[3] * b[1];
        b[3] -= l[2] * b[0] + l[4] * b[1] + l[5] * b[2];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] *= id[i];
        b[2] -= l[5] * b[3];
        b[1] -= l[3] * b[2] + l[4] * b[3];
        b[0] -= l[0] * b[1] + l[1] * b[2] + l[2] * b[3];
    }
};

// The sums over the wavefront of SIXTEEN per-lane values at once: lane l ends with the total of value l % 16. A wave_sum per value is
// a chain of eight dependent cross-lane steps (~200 cycles for a lone wavefront) and an iteration of the wide kernel's active-set loop
// needs ~20 of them; here every exchange step HALVES the number of live values -- a lane keeps the half whose index has its own bit
// and hands the other half to its partner -- so sixteen sums cost 15 exchanges + 6 row / half steps instead of 128.
template <int MASK> __device__ __forceinline__ float lane_xor(float v)
{
    if constexpr (MASK == 1) return dpp_mov<0xb1>(v);
    else if constexpr (MASK == 2) return dpp_mov<0x4e>(v);
    else if constexpr (MASK == 32) return __shfl_xor(v, 32);
    else return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), (MASK << 10) | 0x1f));  // (bit-mask mode: xor inside 32 lanes)
}
template <int MASK> __device__ __forceinline__ double lane_xor(double v)
{
    if constexpr (MASK == 1) return dpp_mov<0xb1>(v);
    else if constexpr (MASK == 2) return dpp_mov<0x4e>(v);
    else if constexpr (MASK == 32) return __shfl_xor(v, 32);
    else {
        const int lo = __builtin_amdgcn_ds_swizzle(__double2loint(v), (MASK << 10) | 0x1f);
        const int hi = __builtin_amdgcn_ds_swizzle(__double2hiint(v), (MASK << 10) | 0x1f);
        return __hiloint2double(hi, lo);
    }
}
// K = 4, 8 or 16 values: lane l ends with the total of value l % K
template <typename T, int K> __device__ __forceinline__ T multi_sum(const T (&p)[K], int lane)
{
    static_assert(K == 4 || K == 8 || K == 16, "multi_sum: 4, 8 or 16 values");
    T a[K / 2];
    const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
#pragma unroll
    for (int i = 0; i < K / 2; ++i) a[i] = (b0 ? p[2 * i + 1] : p[2 * i]) + lane_xor<1>(b0 ? p[2 * i] : p[2 * i + 1]);
    T b[K / 4];
#pragma unroll
    for (int i = 0; i < K / 4; ++i) b[i] = (b1 ? a[2 * i + 1] : a[2 * i]) + lane_xor<2>(b1 ? a[2 * i] : a[2 * i + 1]);
    T d;
    if constexpr (K == 4) {
        d = b[0];
        d += lane_xor<4>(d);
        d += lane_xor<8>(d);
    } else {
        T c[K / 8];
#pragma unroll
        for (int i = 0; i < K / 8; ++i) c[i] = (b2 ? b[2 * i + 1] : b[2 * i]) + lane_xor<4>(b2 ? b[2 * i] : b[2 * i + 1]);
        if constexpr (K == 8) {
            d = c[0];
            d += lane_xor<8>(d);
        } else {
            d = (b3 ? c[1] : c[0]) + lane_xor<8>(b3 ? c[0] : c[1]);
        }
    }
    d += lane_xor<16>(d);
    d += lane_xor<32>(d);
    return d;
}

}  // namespace stagew

using namespace stagew;

template <typename T, int NXC, bool FUSE, bool LOW = false>
// (float32: three wavefronts per SIMD, 168 VGPRs -- except the instantiations that do not fit them without spilling: nx = 16, and
// the general constraint layout at nx = 12, take two)
__global__ void __launch_bounds__(64)
    __attribute__((amdgpu_waves_per_eu(LOW ? 1 : (sizeof(T) == 4 && NXC < 16 && (FUSE || NXC < 12)) ? STAGEW_WPE32 : 2)))
    mpcqp_stagew_kernel(const KernelArgs ka, const Ws wl, T *__restrict__ wsbase, const int64_t batch)
{
    using V4 = __attribute__((ext_vector_type(4))) T;
    using MV = typename Mfma<T>::V;
    constexpr int D = sizeof(T) == 4 ? (LOW ? D_LOW : STAGEW_D) : 4;  // the sweeps request their records this many steps ahead
    // passes of the final verification: every pass but the last one triggers a refinement step of the multipliers when an
    // active row is off its bound by more than 10 tol (1 + |e|) (float64; see below) / STAGEW_VTRIG32 tol (1 + |e|) (float32: 8, was 64
    // -- a stress run in float32 left rows 6e-4 off their bounds and plans 1.5e-3 off the oracle's). Round 4: float32 makes
    // up to two refinement steps and then ACCEPTS only at STAGEW_VACC32 = 16 tol (1 + |e|) plus the rounding noise of the
    // evaluation itself (it was 1000 tol: plans 3e-3 from the float64 one came back SOLVED when W had drifted; such a
    // problem is now MPCQP_MAX_ITER and the host side retries it through the other formulations: tools/stress_f32.py)
    // Round 5, float64: an active row 1e-6 (1 + |e|) off its bound used to be accepted -- the oracle's own rule, but the oracle's
    // rows sit 1e-12 off theirs -- and on a nearly fully active problem that is a plan 6e-6 from the minimiser reported SOLVED
    // (tools/stress_tight.py wide, STRESS_TIGHT=0.3, seed 11). Now 10 tol (1 + |e|) triggers a refinement step, up to two of them,
    // and 100 tol (1 + |e|) = 1e-7 is what is accepted; what still fails is MPCQP_MAX_ITER and the host side re-solves it through
    // the other formulations (the general stage-wise kernel last).
    constexpr int VPASS = sizeof(T) == 4 ? STAGEW_VPASS32 : 3;
    extern __shared__ __attribute__((aligned(16))) unsigned char stagew_smem[];
    const int lane = threadIdx.x, pg = lane >> 4, c16 = lane & 15;
    const int64_t prob = blockIdx.x;
    const int nx = ka.nx, nu = ka.nu, N = ka.N, mk = ka.mk, maxq = wl.maxq;
    const int M = N * mk, nvar = N * nu, nv4 = N * 4;
    constexpr int NQ = NXC / 4;             // quarters of the state
    constexpr bool STACK = NXC <= 12;       // the input-sized rows fit under the state-sized ones in one 16-row block
    constexpr int NA = STACK ? 1 : 2;       // row blocks of the stacked matrices
    constexpr int NB = NA * NQ, NF = NA * (NQ + 1);  // record values per lane and step, backward / forward
    // a step's record is stored lane-major in groups of LB (LF) <= 4 values (one load per lane and group: the sweeps are
    // bound by the ISSUE of their loads, not by latency -- measured): value e of lane l sits at (e / L) 64 L + L l + e % L.
    // Fewer than four values per lane form ONE group of that many (round 3: the records are the kernel's HBM traffic, and
    // config 5's backward record -- three values -- was padded to four).
    constexpr int LB = NB < 4 ? NB : 4, LF = NF < 4 ? NF : 4;
    constexpr int GB = (NB + LB - 1) / LB, GF = (NF + LF - 1) / LF;
    constexpr int SB = GB * 64 * LB, SF = GF * 64 * LF;  // elements per step
    using RecB = RecN<T, LB>;
    using RecF = RecN<T, LF>;
    constexpr int R = FUSE ? (LOW ? R_FUSE_LOW : R_FUSE) : R_PLAIN;  // right-hand sides per sweep pair
    constexpr int ZL = NXC + 4;             // a row of Zp: position g (NQ + 1) + q holds x[4 q + g] (q < NQ), u[g] (q = NQ)
    const bool col0 = c16 == 0;             // the lanes of right-hand side 0
    const bool colr = c16 < R;              // the lanes of the right-hand sides in use
    const int cn = colr ? c16 : 0;          // this lane's right-hand side
    const T INF = (T)HUGE_VAL;
    const T DEPTOL = Tol<T>::dep;
    // ---- LDS: matrix tiles of the Riccati step, the sweeps' running vectors, the vectors shared by the lanes
    // (the stacked instantiations, nx <= 12, run the recursion in registers and carve no tiles: kTileElems below)
    T *Pm = (T *)stagew_smem, *PAm = Pm + 16 * LD, *Mm = PAm + 16 * LD, *Am = Mm + 16 * LD, *Atm = Am + 16 * LD;
    T *Acm = Atm + 16 * LD, *PBm = Acm + 16 * LD, *Bm = PBm + 16 * 4, *Btm = Bm + 16 * 4, *BPAm = Btm + 4 * LD;
    T *Km = BPAm + 4 * LD, *Fm = Km + 4 * LD, *Sm = Fm + 4 * LD, *Lim = Sm + 16;  // (Lim: Ls^-1 of the step, 4 x 4)
    T *cst = STACK ? (T *)stagew_smem : Sm + 32;  // cst: 0, 1, spare cells
    // (the active set's LDS -- d, r, multipliers, row ids, the tile of R -- is carved behind cst + 8 where the loop starts)
    // ---- workspace
    T *ws = wsbase + prob * wl.total;
    T *Mb = ws + wl.Mb, *Mf = ws + wl.Mf, *ffv = ws + wl.ff;
    T *Zs = ws + wl.Zs, *s0 = ws + wl.s0, *sl = ws + wl.s, *invn = ws + wl.invn, *thr = ws + wl.thr;
    V4 *Gp = (V4 *)(ws + wl.Gp);
    const int Mg = wl.mg;
    const bool ginv = Mg != M;
    // ---- operands
    const T *gA = (const T *)ka.A.ptr + prob * ka.A.batch_stride;
    const T *gB = (const T *)ka.B.ptr + prob * ka.B.batch_stride;
    const T *gC = ka.C.ptr ? (const T *)ka.C.ptr + prob * ka.C.batch_stride : nullptr;
    const T *gD = ka.D.ptr ? (const T *)ka.D.ptr + prob * ka.D.batch_stride : nullptr;
    const T *ge = (const T *)ka.e.ptr + prob * ka.e.batch_stride;
    const T *gx0 = (const T *)ka.x0.ptr + prob * ka.x0.batch_stride;
    const T *ggoal = ka.goal.ptr ? (const T *)ka.goal.ptr + prob * ka.goal.batch_stride : nullptr;
    const T *gtgt = ka.targets.ptr ? (const T *)ka.targets.ptr + prob * ka.targets.batch_stride : nullptr;
    const int64_t sA = ka.A.step_stride, sB = ka.B.step_stride, sC = ka.C.step_stride, sD = ka.D.step_stride, sE = ka.e.step_stride;
    const bool stageP = ka.flags & MPCQP_P_STAGE, termP = ka.flags & MPCQP_P_TERMINAL;
    const bool stageQ = (ka.flags & MPCQP_Q_STAGE) && gtgt, termQ = (ka.flags & MPCQP_Q_TERMINAL) && ggoal;
    const T wu = (T)ka.wu, wx = stageP ? (T)ka.wx : T(0), wt = termP ? (T)ka.wt : T(0);

    if (ka.opt_flags & kOptSecondOpinion) {  // (behind the narrow kernel: only what it left unsolved, mpcqp_internal.h)
        const int st0 = ka.status[prob];
        if (st0 != MPCQP_MAX_ITER && st0 != MPCQP_INFEASIBLE) return;
    }
    long long *stamp = ka.probe ? (long long *)ka.probe + prob * 16 : nullptr;
    auto tick = [&](int slot) {
        if (stamp && lane == 0) stamp[slot] = (long long)__builtin_readcyclecounter();
    };
    tick(0);
    // (developer probe) slots 8..15 accumulate the time spent in the parts of the active-set loop
    long long tlast = 0;
    auto tacc = [&](int slot) {
        if (stamp) {
            const long long now = (long long)__builtin_readcyclecounter();
            if (lane == 0 && slot >= 0) stamp[slot] += now - tlast;
            tlast = now;
        }
    };
    if (stamp && lane == 0)
        for (int i = 8; i < 16; ++i) stamp[i] = 0;

    // ================================================================= factor: Riccati recursion
    bool notpd = false;  // a pivot of S_k = w_u I + B_k' P_{k+1} B_k was not positive: the condensed Hessian is not positive definite
    if constexpr (STACK) {
        // ---- nx <= 12: the whole recursion in REGISTERS on the matrix cores, no LDS, no barrier.
        // Every matrix is a 16 x 16 tile in the accumulator layout of the 16x16x4 MFMA ("D layout": register t of lane
        // (pg, c16) holds physical row Mfma::row(pg, t), column c16). Feeding register t of two such tiles X, Y as the A
        // and B operand of ONE instruction contracts them over the rows of that register: sum_t mfma(X[t], Y[t]) = X' Y,
        // again in D layout -- so products chain register to register. Logical indices: row 4 t + pg, column
        // rowmap(c16) (the same permutation on both sides; identity in float64); states 0..NXC-1 are registers t < NQ,
        // the inputs NXC..NXC+3 are register NQ, and a contraction over states / inputs only is NQ / one instruction.
        //   W = [A B],  Z = P W,  H = W' Z = [[A'PA, A'PB], [B'PA, B'PB]],  S = w_u I + H_uu = L D L' (every lane, from
        //   ten v_readlane), K = S^-1 H_ux and S^-1 through ONE product with S^-1 spread over the input block,
        //   E = [A 0] - [B; I] [K, S^-1] = [[Acl, F'], [-K, -S^-1]] (F = -S^-1 B': rows t < NQ are the backward record),
        //   P_k = Q_k + H_xx - H_ux' K (symmetrised by a product with the identity), [Acl', -K'] = [A' 0] - K' [B', I]
        //   (the forward record). 13 instructions on the matrix cores and ~100 on the vector pipe per step (nx = 12)
        //   against ~20 + 370 and seven LDS round trips for the tiled version below.
        constexpr int TI = NQ;  // the register (contraction chunk) of the input rows
        const int lcol = Mfma<T>::rowmap(c16);
        const bool scol = lcol < NXC, ucol = lcol >= NXC && lcol < NXC + 4;
        const int ic = lcol - NXC;  // input index of an input column
        // this lane's entries of the step's operands: W[t] = [A B][4 t + pg][lcol], WA[t] = A'[4 t + pg][lcol],
        // mB = -[B', I][pg][lcol]; element offsets inside the step's block (clamped) and validity
        unsigned offW[NQ], offAt[NQ], offBt;
        bool okW[NQ], okAt[NQ];
#pragma unroll
        for (int t = 0; t < NQ; ++t) {
            const int lr = 4 * t + pg;
            okW[t] = scol ? (lr < nx && lcol < nx) : (ucol && ic < nu && lr < nx);
            offW[t] = okW[t] ? (unsigned)(scol ? lr * nx + lcol : lr * nu + ic) : 0u;
            okAt[t] = scol && lr < nx && lcol < nx;
            offAt[t] = okAt[t] ? (unsigned)(lcol * nx + lr) : 0u;
        }
        const bool okBt = scol && lcol < nx && pg < nu;
        offBt = okBt ? (unsigned)(lcol * nu + pg) : 0u;
        const T cBt = (ucol && ic == pg) ? T(-1) : T(0);
        const T *baseW = scol ? gA : gB;
        const int64_t stW = scol ? sA : sB;
        MV P, Id;  // P_{k+1} (state block; zero elsewhere) and the identity, both in D layout
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int lr = 4 * t + pg;
            Id[t] = (t < NQ && lr == lcol) ? T(1) : T(0);
            P[t] = (t < NQ && lr == lcol && lr < nx) ? wt : T(0);
        }
        // The backward sweep of the UNCONSTRAINED minimiser rides along: its costate p_k = Acl_k' p_{k+1} - w_x xref_k and
        // feed-forward term ff_k = F_k p_{k+1} need exactly the record this step produces ([Acl, F'] = rows t < NQ of E),
        // run in the same direction, and their three products fill gaps of the recursion's dependent chain: the
        // separate sweep (64 serial steps, ~7 % of a config-5 problem) is gone. Column 0 of the operand, as in the sweeps.
        const bool tgtq = stageQ;
        const T wxq = (T)ka.wx;
        MV pst = {T(0), T(0), T(0), T(0)};
        if (termQ && col0) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (4 * q + pg < nx) pst[q] = -(T)ka.wt * ggoal[4 * q + pg];
        }
        const T *tp0 = stageQ ? gtgt : gA;  // (a readable address when there are no targets)
        constexpr int PD = LOW ? 4 : STAGEW_PDD;  // operands are requested this many steps ahead (a lone wavefront: deeper)
        T pw[PD][NQ], pa[PD][NQ], pb[PD], ptg[PD][NQ];
        auto request = [&](int d, int k) {
            const T *w = baseW + k * stW, *a = gA + k * sA, *b = gB + k * sB;
#pragma unroll
            for (int t = 0; t < NQ; ++t) {
                pw[d][t] = w[offW[t]];
                pa[d][t] = a[offAt[t]];
                ptg[d][t] = tp0[(int64_t)(tgtq ? k : 0) * nx + (4 * t + pg < nx ? 4 * t + pg : nx - 1)];
            }
            pb[d] = b[offBt];
        };
#pragma unroll
        for (int d = 0; d < PD; ++d) {
            request(d, N - 1 - d >= 0 ? N - 1 - d : 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        const MV zero4 = {T(0), T(0), T(0), T(0)};
        auto rstep = [&](int d, int k) {
            MV W = zero4, Wz = zero4, WA = zero4;
            T tgk[NQ];
#pragma unroll
            for (int t = 0; t < NQ; ++t) {
                W[t] = okW[t] ? pw[d][t] : T(0);
                Wz[t] = scol ? W[t] : T(0);
                WA[t] = okAt[t] ? pa[d][t] : T(0);
                tgk[t] = ptg[d][t];
            }
            const T mB = okBt ? -pb[d] : cBt;
            request(d, k - PD >= 0 ? k - PD : 0);
            MV Z, H;
            {   // Z = P W, H = W' P W
                T pa_[NQ], wa_[NQ], za_[NQ];
#pragma unroll
                for (int t = 0; t < NQ; ++t) {
                    pa_[t] = P[t];
                    wa_[t] = W[t];
                }
                Z = mfma_sum<T, NQ>(pa_, wa_, zero4);
#pragma unroll
                for (int t = 0; t < NQ; ++t) za_[t] = Z[t];
                H = mfma_sum<T, NQ>(wa_, za_, zero4);
            }
            // S = w_u I + H_uu (identity on the padding), the same in every lane
            Ldl4<T> ldl;
            {
                T sv[10];
#pragma unroll
                for (int i = 0, e = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j, ++e)
                        sv[e] = lane_get_halves(H[TI], 16 * i + Mfma<T>::rowmap(NXC + j)) + ((i == j) ? (i < nu ? wu : T(1)) : T(0));
                notpd |= !ldl.factor(sv);
            }
            // S^-1 spread over the input block: lane (pg, input column b) holds S^-1[pg][b]
            T sfull;
            {
                T eb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) eb[i] = (ic == i) ? T(1) : T(0);
                ldl.solve(eb);
                const T v = pg == 0 ? eb[0] : pg == 1 ? eb[1] : pg == 2 ? eb[2] : eb[3];
                sfull = ucol ? v : T(0);
            }
            // Ls^-T spread over the input block the same way: lane (pg, input column b) holds Ls^-T[pg][b] = Ls^-1[b][pg]
            // (S = Ls Ls', Ls = L D^1/2). The records are kept in WHITENED coordinates (round 6): the backward sweep then yields
            // y_k = Ls_k' ff_k directly and g_a P^-1 g_b' = y_a . y_b (the Riccati recursion is a block Cholesky factorisation of
            // the condensed Hessian), the forward sweep takes y_k as its input.
            T sid[4], swh;
            {
#pragma unroll
                for (int i = 0; i < 4; ++i) sid[i] = ldl.sd[i];
                T eb[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) eb[i] = (pg == i) ? T(1) : T(0);
                ldl.wsolve(eb, sid);
                const T v = ic == 0 ? eb[0] : ic == 1 ? eb[1] : ic == 2 ? eb[2] : eb[3];
                swh = ucol ? v : T(0);
            }
            const MV K3 = Mfma<T>::run(sfull, H[TI], zero4);  // rows of the inputs: S^-1 [H_ux, H_uu]
            const T kfull = scol ? K3[TI] : T(0);              // K = S^-1 H_ux
            const T ks3 = scol ? K3[TI] : swh;                 // [K, Ls^-T]
            const MV E = Mfma<T>::run(mB, ks3, Wz);            // [[Acl, -B Ls^-T], [-K, -Ls^-T]]
            const MV RW = Mfma<T>::run(swh, -mB, zero4);       // rows of the inputs: Ls^-1 [B', I]
            MV Hq = H;
#pragma unroll
            for (int t = 0; t < NQ; ++t) Hq[t] += (4 * t + pg == lcol && lcol < nx && k >= 1) ? wx : T(0);  // (x_0 is data: Q_0 = 0)
            {  // (p_k, ff_k) = [Acl' ; F] p_{k+1} (+ the tracking cost of step k)
                MV a0 = zero4;
#pragma unroll
                for (int t = 0; t < NQ; ++t) a0[t] = T(0);
                {
                    T ea_[NQ], pp_[NQ];
#pragma unroll
                    for (int t = 0; t < NQ; ++t) {
                        ea_[t] = E[t];
                        pp_[t] = pst[t];
                    }
                    a0 = mfma_sum<T, NQ>(ea_, pp_, zero4);
                }
                ws[col0 ? (unsigned)wl.ff + (unsigned)(k * 4 + pg) : (unsigned)wl.junk + (unsigned)lane] = a0[NQ];  // (column 0 carries the tracking terms; the other lanes aim at their junk cell: no branch, no traffic)
#pragma unroll
                for (int t = 0; t < NQ; ++t)
                    pst[t] = a0[t] - ((tgtq && k >= 1 && col0 && 4 * t + pg < nx) ? wxq * tgk[t] : T(0));
            }
            MV Pk = Mfma<T>::run(H[TI], E[TI], Hq);  // Q_k + H_xx - H_ux' K
#pragma unroll
            for (int t = 0; t < 4; ++t) Pk[t] = (t < NQ && scol) ? Pk[t] : T(0);
            MV PT = zero4;
#pragma unroll
            for (int t = 0; t < NQ; ++t) PT[t] = T(0);  // P_k' = P_k' I
            {
                T pk_[NQ], id_[NQ];
#pragma unroll
                for (int t = 0; t < NQ; ++t) {
                    pk_[t] = Pk[t];
                    id_[t] = Id[t];
                }
                PT = mfma_sum<T, NQ>(pk_, id_, zero4);
            }
            const MV M2 = Mfma<T>::run(kfull, mB, WA);  // [Acl', -K']
            // factors to the workspace: the sweeps' records (one MFMA operand = 64 consecutive values), K' and the factor
            // of S (read at the candidate row's step)
            {
                RecB rb;  // (this branch: NB = NQ <= 3 and NF = NQ + 1 <= 4 values per lane, one group each)
                RecF rf;
#pragma unroll
                for (int e = 0; e < NQ; ++e) {
                    rb.v[e] = E[e];
                    rf.v[e] = M2[e];
                }
                rf.v[NQ] = RW[TI];
                *(RecB *)(Mb + (int64_t)k * SB + lane * LB) = rb;
                *(RecF *)(Mf + (int64_t)k * SF + lane * LF) = rf;
                // (K' and Ls^-1 of the step, which a candidate row's backward sweep starts from, are IN the forward record -- its
                // input columns --: rounds 2-5 stored them a second time, 80 values per step)
            }
#pragma unroll
            for (int t = 0; t < NQ; ++t) P[t] = T(0.5) * (Pk[t] + PT[t]);
        };
        int k = N - 1;
        for (int g = N / PD; g > 0; --g) {
#pragma unroll
            for (int d = 0; d < PD; ++d) rstep(d, k - d);
            k -= PD;
        }
#pragma unroll
        for (int d = 0; d < PD - 1; ++d)
            if (k - d >= 0) rstep(d, k - d);
        if (lane < 8) cst[lane] = lane == 1 ? T(1) : T(0);
        wave_sync_workgroup();
    } else {
        // ---- nx > 12: 16 x 16 tiles in LDS
        for (int i = lane; i < (int)(cst - Pm) + 8; i += 64) Pm[i] = T(0);  // every tile and the constants
        wave_sync_workgroup();
        if (lane < nx) Pm[lane * LD + lane] = wt;
        if (lane == 0) cst[1] = T(1);
        wave_sync_workgroup();
        // where this lane's record values come from (LDS offsets from Pm; fixed along the horizon): entry (blk, kk) of a
        // record is the stacked matrix at row rowmap(lane % 16) of block blk, column 4 kk + lane / 16
        int srcb[NB], srcf[NF];
        T sgnf[NF];
        {
            const int zero = (int)(cst - Pm), mrow = Mfma<T>::rowmap(c16);
#pragma unroll
            for (int blk = 0; blk < NA; ++blk) {
#pragma unroll
                for (int kk = 0; kk <= NQ; ++kk) {
                    const int col = 4 * kk + pg;
                    // the input-sized row this (block, row) is, or -1
                    const int irow = (blk == 0) ? ((STACK && mrow >= NXC && mrow < NXC + 4) ? mrow - NXC : -1) : (mrow < 4 ? mrow : -1);
                    if (kk < NQ) {  // backward: [Acl' ; F], F = -Ls^-1 B'
                        int o = zero;
                        if (blk == 0 && mrow < NXC) o = (int)(Acm - Pm) + col * LD + mrow;
                        if (irow >= 0) o = (int)(Fm - Pm) + irow * LD + col;
                        srcb[blk * NQ + kk] = o;
                    }
                    {  // forward: [[Acl, B Ls^-T], [-K, Ls^-T]]  (B Ls^-T = -F' with F = -Ls^-1 B', whitened records: round 6)
                        int o = zero;
                        T sg = T(1);
                        if (blk == 0 && mrow < NXC) {
                            if (col < NXC) {
                                o = (int)(Acm - Pm) + mrow * LD + col;
                            } else {
                                o = (int)(Fm - Pm) + (col - NXC) * LD + mrow;
                                sg = T(-1);
                            }
                        }
                        if (irow >= 0) {
                            if (col < NXC) {
                                o = (int)(Km - Pm) + irow * LD + col;
                                sg = T(-1);
                            } else {
                                o = (int)(Lim - Pm) + (col - NXC) * 4 + irow;  // Ls^-T[irow][j] = Ls^-1[j][irow]
                            }
                        }
                        srcf[blk * (NQ + 1) + kk] = o;
                        sgnf[blk * (NQ + 1) + kk] = sg;
                    }
                }
            }
        }
        // A_k, B_k are requested one step ahead (<= 4 + 1 entries per lane) and land in the LDS tiles at the top of their step.
        // No branches: lanes without an entry re-read the last one and write it to a spare LDS cell.
        constexpr int NAU = (NXC * NXC + 63) / 64;
        const int junk = (int)(cst - Pm) + 4;
        T pfa[NAU], pfb;
        unsigned idxA[NAU], idxB;
        int offA[NAU], offAt[NAU], offB = junk, offBt = junk + 1, offK = -1;  // LDS offsets (from Pm) of this lane's entries
#pragma unroll
        for (int u = 0; u < NAU; ++u) {
            const int i = lane + 64 * u, r = i / nx, c = i - r * nx;
            const bool in = i < nx * nx;
            idxA[u] = (unsigned)(in ? i : nx * nx - 1);
            offA[u] = in ? (int)(Am - Pm) + r * LD + c : junk;
            offAt[u] = in ? (int)(Atm - Pm) + c * LD + r : junk + 1;
        }
        idxB = (unsigned)(lane < nx * nu ? lane : nx * nu - 1);
        if (lane < nx * nu) {
            const int r = lane / nu, c = lane - r * nu;
            offB = (int)(Bm - Pm) + r * 4 + c;
            offBt = (int)(Btm - Pm) + c * LD + r;
            offK = c * LD + r;  // Kt[r][c] = K[c][r]
        }
        auto request = [&](int k) {
            const T *a = gA + k * sA, *bb = gB + k * sB;
#pragma unroll
            for (int u = 0; u < NAU; ++u) pfa[u] = a[idxA[u]];
            pfb = bb[idxB];
        };
        request(N - 1);
        for (int k = N - 1; k >= 0; --k) {
            // stage A_k, A_k', B_k, B_k'
#pragma unroll
            for (int u = 0; u < NAU; ++u) {
                Pm[offA[u]] = pfa[u];
                Pm[offAt[u]] = pfa[u];
            }
            Pm[offB] = pfb;
            Pm[offBt] = pfb;
            wave_sync_workgroup();
            request(k > 0 ? k - 1 : 0);
            mm_t<T, LD, LD, LD, 16, 16, NXC, false>(PAm, Pm, Am, nullptr, pg, c16);    // PA = P A
            mm_t<T, LD, 4, 4, 16, 4, NXC, false>(PBm, Pm, Bm, nullptr, pg, c16);      // PB = P B
            wave_sync_workgroup();
            mm_t<T, LD, 4, 4, 4, 4, NXC, false>(Sm, Btm, PBm, nullptr, pg, c16);     // B' P B
            mm_t<T, LD, LD, LD, 4, 16, NXC, false>(BPAm, Btm, PAm, nullptr, pg, c16); // B' P A
            wave_sync_workgroup();
            // S = w_u I + B'PB (nu <= 4, identity on the padding) is factored L D L' in registers, every lane the same; lane
            // (., c) then solves for column c of K = S^-1 B'PA and of F = -S^-1 B' (row group i writes row i)
            Ldl4<T> ldl;
            {
                T sv[10];
#pragma unroll
                for (int i = 0, e = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j <= i; ++j, ++e) sv[e] = Sm[i * 4 + j] + ((i == j) ? (i < nu ? wu : T(1)) : T(0));
                notpd |= !ldl.factor(sv);
                T kc[4], fc[4], ec[4], sid[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    kc[i] = BPAm[i * LD + c16];
                    fc[i] = Bm[c16 * 4 + i];
                    ec[i] = (c16 == i) ? T(1) : T(0);
                    sid[i] = ldl.sd[i];
                }
                ldl.solve(kc);
                ldl.wsolve(fc, sid);  // Ls^-1 B' (column c16): the WHITENED feed-forward row block
                ldl.wsolve(ec, sid);  // Ls^-1 (column c16 < 4)
                const T kv = pg == 0 ? kc[0] : pg == 1 ? kc[1] : pg == 2 ? kc[2] : kc[3];
                const T fv = pg == 0 ? fc[0] : pg == 1 ? fc[1] : pg == 2 ? fc[2] : fc[3];
                const T lv = pg == 0 ? ec[0] : pg == 1 ? ec[1] : pg == 2 ? ec[2] : ec[3];
                Km[pg * LD + c16] = kv;
                Fm[pg * LD + c16] = -fv;
                if (c16 < 4) Lim[pg * 4 + c16] = lv;
#pragma unroll
                for (int i = 0; i < 4; ++i) ldl.id[i] = sid[i];  // (what the workspace keeps: 1 / sqrt(d_i))
            }
            wave_sync_workgroup();
            mm_t<T, 4, LD, LD, 16, 16, 4, true>(Acm, Bm, Km, Am, pg, c16);           // Acl = A - B K
            mm_t<T, 4, LD, LD, 16, 16, 4, true>(Mm, PBm, Km, PAm, pg, c16);          // M = P Acl = PA - PB K
            wave_sync_workgroup();
            mm_t<T, LD, LD, LD, 16, 16, NXC, false>(PAm, Atm, Mm, nullptr, pg, c16);   // A' P Acl (into the PA tile)
            // factors to the workspace: the sweeps' records (A-operand order, 64 consecutive values per MFMA), and K', S^-1
            // (read at the candidate row's step)
            {
                T *mb = Mb + (int64_t)k * SB + lane * LB, *mf = Mf + (int64_t)k * SF + lane * LF;
#pragma unroll
                for (int g = 0; g < GB; ++g) {
                    RecB v;
#pragma unroll
                    for (int j = 0; j < LB; ++j) v.v[j] = (LB * g + j < NB) ? Pm[srcb[LB * g + j < NB ? LB * g + j : 0]] : T(0);
                    *(RecB *)(mb + g * 64 * LB) = v;
                }
#pragma unroll
                for (int g = 0; g < GF; ++g) {
                    RecF v;
#pragma unroll
                    for (int j = 0; j < LF; ++j)
                        v.v[j] = (LF * g + j < NF) ? sgnf[LF * g + j < NF ? LF * g + j : 0] * Pm[srcf[LF * g + j < NF ? LF * g + j : 0]] : T(0);
                    *(RecF *)(mf + g * 64 * LF) = v;
                }
            }
            wave_sync_workgroup();
            // P_k = Q_k + sym(A' P Acl)   (x_0 is data: Q_0 = 0)
            {
                const T qk = (k >= 1) ? wx : T(0);
                T pn[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int r = pg + 4 * t;
                    pn[t] = T(0.5) * (PAm[r * LD + c16] + PAm[c16 * LD + r]) + ((r == c16 && r < nx) ? qk : T(0));  // (zero padding)
                }
                wave_sync_workgroup();
#pragma unroll
                for (int t = 0; t < 4; ++t) Pm[(pg + 4 * t) * LD + c16] = pn[t];
            }
            wave_sync_workgroup();
        }
    }
    tick(1);
    if (__ballot(notpd) != 0ull) {
        // mpc_problem.py:104-107 only guarantees w_u > 0; a negative state weight can still make the Hessian indefinite.
        // The pivots S_k of the recursion are the Schur complements of the condensed Hessian in the order u_{N-1}, ...,
        // u_0, so P is positive definite iff every S_k is: report what the condensed kernels' Cholesky reports.
        T *ou = (T *)ka.U + prob * (int64_t)nvar;
        for (int i = lane; i < nvar; i += 64) ou[i] = T(0);
        if (ka.lam) {
            T *ol = (T *)ka.lam + prob * (int64_t)M;
            for (int i = lane; i < M; i += 64) ol[i] = T(0);
        }
        if (lane == 0) {
            if (ka.status) ka.status[prob] = MPCQP_NOT_PD;
            if (ka.iters) ka.iters[prob] = 0;
        }
        return;
    }

    // ================================================================= the LQR solve: two serial sweeps
    // The running vector is an MFMA B operand: register q of the lanes of row group g = lane / 16 holds component
    // 4 q + g (columns: right-hand sides; column 0 = lanes with lane % 16 == 0 is the one in use).
    const T *tp = stageQ ? gtgt : Mb;  // (a readable address when there are no targets)
    // backward: (p_k, ff_k) = [Acl_k' ; F_k] p_{k+1} (+ the step's linear cost). With `track` the tracking costs from p_N;
    // else the costate of one row of G, which is zero after its step kq: `start` is (p_kq, ff_kq) and the sweep runs
    // over k < kq.
    // Several rows at once: column n of the operand is row n's costate; it is injected at its own step (mykq, per
    // lane; `start` = (p_kq, ff_kq)) and the sweep starts at the latest of them (kq).
    auto backward = [&](auto trackc, int kq, MV start, T ffstart, int mykq) {
        constexpr bool track = decltype(trackc)::value;
        const bool tgt = track && stageQ;
        const T wxq = (T)ka.wx;
        const unsigned ffo = (unsigned)(c16 * N * 4 + pg);  // this lane's entries of the array of whitened vectors (sixteen columns)
        MV st = start;
        const int kstart = track ? N - 1 : kq - 1;
        if (!track) {
            const bool now = colr && mykq == kq;
#pragma unroll
            for (int q = 0; q < 4; ++q) st[q] = now ? start[q] : T(0);
            if (now) ffv[ffo + (unsigned)(kq * 4)] = ffstart;
        }
        T rec[D][NB], tg[D][NQ];
#pragma unroll
        for (int d = 0; d < D; ++d) {
#pragma unroll
            for (int e = 0; e < NB; ++e) rec[d][e] = T(0);
#pragma unroll
            for (int q = 0; q < NQ; ++q) tg[d][q] = T(0);
        }
        auto req = [&](int d, int k) {
            const T *mb = Mb + (int64_t)k * SB + lane * LB;
#pragma unroll
            for (int g = 0; g < GB; ++g) {
                const RecB v = *(const RecB *)(mb + g * 64 * LB);
#pragma unroll
                for (int j = 0; j < LB; ++j)
                    if (LB * g + j < NB) rec[d][LB * g + j] = v.v[j];
            }
            if (track) {
#pragma unroll
                for (int q = 0; q < NQ; ++q) tg[d][q] = tp[(int64_t)k * nx + (4 * q + pg < nx ? 4 * q + pg : nx - 1)];
            }
        };
        // (requests are unconditional -- clamped at the end of the sweep -- so that every path carries the same number
        // of loads in flight and the compiler can wait for exactly the oldest)
#pragma unroll
        for (int d = 0; d < D; ++d) {
            req(d, kstart - d >= 0 ? kstart - d : 0);
            __builtin_amdgcn_sched_barrier(0);  // oldest first: the loop waits for them in this order
        }
        auto step = [&](int d, int k, bool again) {
            MV a0 = {T(0), T(0), T(0), T(0)}, a1 = {T(0), T(0), T(0), T(0)};
            {
                T ra_[NQ], rb_[NQ], sb_[NQ];
#pragma unroll
                for (int kk = 0; kk < NQ; ++kk) {
                    ra_[kk] = rec[d][kk];
                    rb_[kk] = rec[d][NA == 2 ? NQ + kk : kk];
                    sb_[kk] = st[kk];
                }
                a0 = mfma_sum<T, NQ>(ra_, sb_, a0);
                if (NA == 2) a1 = mfma_sum<T, NQ>(rb_, sb_, a1);
            }
            if (tgt && k >= 1 && col0) {
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (4 * q + pg < nx) a0[q] -= wxq * tg[d][q];
            }
            T ffk = STACK ? a0[NQ] : a1[0];
            if (!track && k == mykq) {  // this column's row enters here (its costate above is zero)
                a0 = start;
                ffk = ffstart;
            }
            ws[colr ? (unsigned)wl.ff + ffo + (unsigned)(k * 4) : (unsigned)wl.junk + (unsigned)lane] = ffk;  // (no branch: a store behind one shortens the request ring, see the forward sweep; the lanes of unused columns aim at their junk cell)
            st = a0;
            if (again) req(d, k - D >= 0 ? k - D : 0);
        };
        // full groups of D steps (every step re-requests: same loads in flight on every path), then the remainder
        int k = kstart;
        for (int g = (kstart + 1) / D; g > 0; --g) {
#pragma unroll
            for (int d = 0; d < D; ++d) step(d, k - d, true);
            k -= D;
        }
#pragma unroll
        for (int d = 0; d < D - 1; ++d)
            if (k - d >= 0) step(d, k - d, false);
    };
    // forward: (x_{k+1}, u_k) = [[Acl_k, B_k Ls_k^-T], [-K_k, Ls_k^-T]] (x_k, y_k) from x_0 = xs, y = the WHITENED feed-forward
    // terms yin[k][0..3] (what the backward sweep left, or a projected vector of the active set).
    // FUSE: [C | D]' as a constant MFMA operand: chunk q of lane (c16, pg) is G[r][4 q + pg] of the row r that lane c16 stands
    // for (chosen so that row group pg' of the RESULT holds rows 4 pg' .. 4 pg' + 3 in both precisions); the last chunk is D
    constexpr int NG = NQ + 1;
    T gT[NG];
    if constexpr (FUSE) {
        const int r = sizeof(T) == 4 ? c16 : 4 * (c16 & 3) + (c16 >> 2);
#pragma unroll
        for (int q = 0; q < NQ; ++q) gT[q] = (gC && r < mk && 4 * q + pg < nx) ? gC[r * nx + 4 * q + pg] : T(0);
        gT[NQ] = (gD && r < mk && pg < nu) ? gD[r * nu + pg] : T(0);
    }
    // chunks of [C | D] that are zero in every lane cost no product (box constraints touch few states): one bit per chunk
    unsigned gnz = 0u;
#pragma unroll
    for (int q = 0; q < NG; ++q) gnz |= (FUSE && __ballot(gT[q] != T(0)) != 0ull) ? (1u << q) : 0u;
    const int mksh = (mk & (mk - 1)) == 0 ? __builtin_ctz(mk) : -1;
    auto stepof = [&](int i) { return mksh >= 0 ? i >> mksh : i / mk; };
    const T tol = ka.tol;
    // ---- LDS of the active set (described where the loop starts)
    constexpr int WL = 32, WLD = 33;
    T *cv = cst + 8, *rv = cv + maxq, *lamv = rv + maxq, *ev = lamv + maxq;
    int *actrow = (int *)(ev + maxq), *colp = actrow + maxq, *crow = colp + maxq;
    T *Rl = (T *)(((uintptr_t)(crow + R) + 15) & ~(uintptr_t)15);
    T *cg = (T *)(Rl + WL * WLD);  // what the cached rows' slacks gain per unit step (y_c . z): the general path's hand-over (the rows'
                                   // state itself -- slack, threshold, metric, active or not -- lives in registers, one row per lane)
    T *invr_l = (T *)(((uintptr_t)(cg + R) + 15) & ~(uintptr_t)15);  // FUSE: 1 / |g_r| of the sixteen rows of a step
    T *Wl_end = invr_l + 16;                                            // (small-batch instantiation: copies of vectors behind this)

    // ---- what happens to a row of G once h_i = g_i . (x_k, u_k) of a forward sweep is known (round 6: the sweeps own the rows).
    // INIT: the sweep of the unconstrained minimiser -- slack, threshold, selection metric; EVAL: the point from scratch
    // (s = e - G (x, u); active rows -- infinite threshold -- checked against their bounds, inactive ones against feasibility).
    // Both also look for the most violated inactive row (sel*). There is no incremental slack update: between two evaluations the
    // iterations only track the rows whose whitened vectors are cached (s_c += t y_c . z, a dot product).
    enum { FW_INIT = 0, FW_EVAL = 2, FW_EVALR = 3 };  // (EVALR: an evaluation that also leaves every row's residual in s0, for a polish step)
    T selb = INF, selv = T(0);
    int seli = 0x7fffffff;
    bool offa = false;
    auto rowlogic = [&](int mode, int i, T hs, T hsa, T ra, T rb, T iv, T fac) {
        const T v = ra - hs;
        T th;
        bool act = false;
        if (mode == FW_INIT) {
            th = tol + tol * (T)fabs((double)ra);
            thr[i] = th;
            invn[i] = iv;
            sl[i] = v;
        } else {
            th = rb;
            act = th == INF;
            if (mode == FW_EVALR) s0[i] = v;
            sl[i] = act ? T(0) : v;
            // (float32: plus what the evaluation itself cannot resolve -- STAGEW_VNOISE32 ulps of the terms' magnitudes)
            const T lim = fac * (tol + tol * (T)fabs((double)ra)) +
                          (sizeof(T) == 4 ? T(STAGEW_VNOISE32) * T(6e-8) * ((T)fabs((double)ra) + hsa) : T(0));
            offa |= act && !((T)fabs((double)v) <= lim);
        }
        const T sc = v * iv;
        if (!act && v < -th && sc < selb) {  // (ties: a lane meets its rows in ascending order; across lanes wave_argmin)
            selb = sc;
            seli = i;
            selv = v;
        }
    };
    // the lane that owns row i in the sweeps (FUSE) / the m-row passes
    auto owner = [&](int i) {
        if constexpr (FUSE) {  // (row r of step k: row group r / 4, column 4 (k % 4) + r % 4)
            const int k = stepof(i), r = i - k * mk;
            return 16 * (r >> 2) + 4 * (k & 3) + (r & 3);
        } else {
            return i & 63;
        }
    };
    auto sel_reduce = [&]() {
        wave_argmin_dpp(selb, seli);
        selv = __shfl(selv, owner(seli < M ? seli : 0));
    };
    T myinvn = T(1);  // FUSE: 1 / |g_r| of the row this lane owns in the sweeps (r = 4 pg + c16, c16 < 4)
    if constexpr (FUSE) {
        T nnv = T(0);  // |g_r|^2 of the row this lane's column stands for in gT (summed over the four row groups)
#pragma unroll
        for (int q = 0; q <= NQ; ++q) nnv += gT[q] * gT[q];
        nnv += __shfl_xor(nnv, 16);
        nnv += __shfl_xor(nnv, 32);
        const int r = (4 * pg + (c16 & 3)) & 15;
        const T nn = __shfl(nnv, sizeof(T) == 4 ? r : 4 * (r & 3) + (r >> 2));
        myinvn = nn > T(0) ? (T)rsqrt((double)nn) : T(1);
    }
    T myl1 = T(0);    // FUSE, float32: sum_j |g_rj| of that row (bounds the magnitude of the row's terms: the evaluation's noise allowance)
    if constexpr (FUSE && sizeof(T) == 4) {
        T l1 = T(0);
#pragma unroll
        for (int q = 0; q <= NQ; ++q) l1 += (T)fabs((double)gT[q]);
        l1 += __shfl_xor(l1, 16);
        l1 += __shfl_xor(l1, 32);
        const int r = (4 * pg + (c16 & 3)) & 15;
        myl1 = __shfl(l1, r);
    }
    unsigned sE32;  // (an independent scalar register: the 64-bit stride sits in a 16-register tuple of the kernel arguments that was reloaded whole)
    asm volatile("s_mov_b32 %0, %1" : "=s"(sE32) : "s"((unsigned)sE));
    T xmax = T(0);  // max |x_k|, |u_k| over the latest forward sweep's trajectory (float32: the noise allowance of the NEXT evaluation)
    T *ou = (T *)ka.U + prob * (int64_t)nvar;
    // What bounds a sweep step (round 6, measured): (i) instruction ISSUE -- a lone wavefront spent ~1000 cycles per step on ~130
    // instructions, a third of them reloads of spilled scalar registers (base pointers, masks, 64-bit strides): every array of the
    // workspace is now addressed from ONE base with 32-bit per-lane offsets, the mode is a compile-time constant, zero chunks of
    // [C | D] are multiplied like the others; (ii) the memory counter: a store inside a lane-divergent `if` sits behind a branch, the
    // compiler must assume the path WITHOUT it when it counts the operations issued since a load (vmcnt is in order), and a ring
    // of D requests degenerates to a wait for the step before. So NO memory operation of the loop is conditional: the vector rides
    // in all sixteen columns, a lane owns the row 4 pg + (c16 & 3) of ONE step in four (phase c16 >> 2), keeps that step's h and u
    // in a register and does its row's work -- bound, threshold, slack, selection, stores -- once per group of four steps, with all
    // 64 lanes busy; lanes without a row (mk < 16, the horizon's last partial group) aim at a junk cell of their own. The vector's
    // entries and the rows' operands are requested per group, D / 4 groups ahead, and a step takes its entry from the lane of its
    // phase by a row broadcast (DPP).
    constexpr int DG = D / 4;  // the groups' request ring
    static_assert(D % 4 == 0, "the forward sweep works in groups of four steps");
    auto forward = [&](auto modec, const T *xs, unsigned yoff, T fac) {
        constexpr int mode = decltype(modec)::value;
        const int ph = c16 >> 2;
        const unsigned r = (unsigned)(4 * pg + (c16 & 3));
        const bool valid = FUSE && r < (unsigned)mk;
        T z[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) z[q] = (xs && 4 * q + pg < nx) ? xs[4 * q + pg] : T(0);
        const unsigned lo_rec = (unsigned)wl.Mf + (unsigned)(lane * LF), lo_z = (unsigned)wl.Zs + (unsigned)(pg * (NQ + 1));
        const unsigned junk = (unsigned)wl.junk + (unsigned)lane;
        const unsigned mku = (unsigned)mk;
        const T c_noise = T(STAGEW_VNOISE32) * T(6e-8), xprev = xmax;
        const int NGall = (N + 3) >> 2;
        T xm = T(0), hacc = T(0), uacc = T(0);
        T rec[D][NF], yv[DG], ev[DG], thv[DG];
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int e = 0; e < NF; ++e) rec[d][e] = T(0);
#pragma unroll
        for (int g = 0; g < DG; ++g) yv[g] = ev[g] = thv[g] = T(0);
        auto req = [&](int d, int k) {
            const unsigned ku = (unsigned)k;
#pragma unroll
            for (int g = 0; g < GF; ++g) {
                const RecF v = *(const RecF *)(ws + (lo_rec + ku * (unsigned)SF + (unsigned)(g * 64 * LF)));
#pragma unroll
                for (int j = 0; j < LF; ++j)
                    if (LF * g + j < NF) rec[d][LF * g + j] = v.v[j];
            }
        };
        // a group's operands: this lane's entry of the vector at ITS step of the group, its row's bound (and threshold)
        auto greq = [&](int gs, int gi) {
            const int st0 = 4 * gi + ph;
            const unsigned stp = (unsigned)(st0 < N ? st0 : N - 1);
            yv[gs] = ws[yoff + 4u * stp + (unsigned)pg];
            if constexpr (FUSE && !(STAGEW_DBG & 16)) {
                ev[gs] = ge[valid ? stp * sE32 + r : 0u];
                if (mode != FW_INIT) thv[gs] = ws[valid ? (unsigned)wl.thr + stp * mku + r : junk];
            }
        };
#pragma unroll
        for (int d = 0; d < D; ++d) {
            req(d, d < N ? d : N - 1);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int g = 0; g < DG; ++g) greq(g, g < NGall ? g : NGall - 1);
        auto step = [&](int d, int gs, int k, auto sc_, bool again) {
            constexpr int sph = decltype(sc_)::value;  // the step's phase in its group
            const unsigned ku = (unsigned)k;
            const T ffd = dpp_mov<0x150 + 4 * sph>(yv[gs]);  // (row_newbcast: the entry held by the lane of phase sph of this row)
            MV a0 = {T(0), T(0), T(0), T(0)}, a1 = {T(0), T(0), T(0), T(0)};
            {
                T ra_[NQ + 1], rb_[NQ + 1], zb_[NQ + 1];
#pragma unroll
                for (int kk = 0; kk <= NQ; ++kk) {
                    ra_[kk] = rec[d][kk];
                    rb_[kk] = rec[d][NA == 2 ? NQ + 1 + kk : kk];
                    zb_[kk] = kk < NQ ? z[kk < NQ ? kk : 0] : ffd;
                }
                a0 = mfma_sum<T, NQ + 1>(ra_, zb_, a0);
                if (NA == 2) a1 = mfma_sum<T, NQ + 1>(rb_, zb_, a1);
            }
            const T u = STACK ? a0[NQ] : a1[0];
            const bool mine = ph == sph;
            uacc = mine ? u : uacc;
            if constexpr (FUSE && !(STAGEW_DBG & 1)) {
                MV hk = {T(0), T(0), T(0), T(0)};
#pragma unroll
                for (int q = 0; q < NQ; ++q)
                    if (gnz & (1u << q)) hk = Mfma<T>::run(gT[q], z[q], hk);
                if (gnz & (1u << NQ)) hk = Mfma<T>::run(gT[NQ], u, hk);
                if constexpr (sizeof(T) == 4) {
#pragma unroll
                    for (int q = 0; q < NQ; ++q) xm = fmaxf(xm, fabsf(z[q]));
                    xm = fmaxf(xm, fabsf(u));
                }
                T hs = hk[0];
                hs = (c16 & 3) == 1 ? hk[1] : hs;
                hs = (c16 & 3) == 2 ? hk[2] : hs;
                hs = (c16 & 3) == 3 ? hk[3] : hs;
                hacc = mine ? hs : hacc;
            } else if constexpr (!FUSE) {
                const unsigned zr = lo_z + ku * (unsigned)ZL;  // (every column writes the same values)
#pragma unroll
                for (int q = 0; q < NQ; ++q) ws[zr + q] = z[q];
                ws[zr + NQ] = u;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) z[q] = a0[q];
            if (again && !(STAGEW_DBG & 2)) req(d, k + D < N ? k + D : N - 1);
        };
        // the end of group gi: every lane's row of ITS step of the group
        auto gend = [&](int gs, int gi) {
            const int st0 = 4 * gi + ph;
            const bool liveu = st0 < N;
            const unsigned stp = (unsigned)(liveu ? st0 : N - 1);
            if (!(STAGEW_DBG & 8)) ws[liveu ? (unsigned)wl.ust + 4u * stp + (unsigned)pg : junk] = uacc;  // (the point itself; the columns of a phase write the same value)
            if constexpr (FUSE) {
                const bool live = valid && liveu;
                const unsigned irow = stp * mku + r;
                const T e_ = ev[gs], v = e_ - hacc;
                const T th0 = tol + tol * (T)fabs((double)e_);  // tol (1 + |e|)
                T th = th0;
                bool act = false;
                if constexpr (mode != FW_INIT) {
                    th = thv[gs];
                    act = th == INF;
                    // (float32: plus what the evaluation itself cannot resolve -- STAGEW_VNOISE32 ulps of the magnitude of the
                    // row's terms, bounded by |e| + |g_r|_1 max |x|)
                    const T lim = fac * th0 + (sizeof(T) == 4 ? c_noise * ((T)fabs((double)e_) + myl1 * xprev) : T(0));
                    offa |= live && act && !((T)fabs((double)v) <= lim);
                }
                const T sc = v * myinvn;
                const bool take = live && !act && v < -th && sc < selb;  // (a lane meets its rows in ascending order; across lanes wave_argmin)
                selb = take ? sc : selb;
                selv = take ? v : selv;
                seli = take ? (int)irow : seli;
                if constexpr (STAGEW_DBG & 8) {
                    selv += th0 * T(1e-30);
                } else if constexpr (mode == FW_INIT) {  // (the selection metric 1 / |g_r| depends on the row of the step only: invr[], no array)
                    ws[live ? (unsigned)wl.thr + irow : junk] = th0;
                    ws[live ? (unsigned)wl.s + irow : junk] = v;
                } else {
                    if constexpr (mode == FW_EVALR) ws[live ? (unsigned)wl.s0 + irow : junk] = v;
                    ws[live ? (unsigned)wl.s + irow : junk] = act ? T(0) : v;
                }
            }
        };
        using P0 = std::integral_constant<int, 0>;
        using P1 = std::integral_constant<int, 1>;
        using P2 = std::integral_constant<int, 2>;
        using P3 = std::integral_constant<int, 3>;
        int k = 0;
        for (int it = N / D; it > 0; --it) {
#pragma unroll
            for (int gs = 0; gs < DG; ++gs) {
                const int kg = k + 4 * gs, gi = kg >> 2;
                step(4 * gs + 0, gs, kg + 0, P0{}, true);
                step(4 * gs + 1, gs, kg + 1, P1{}, true);
                step(4 * gs + 2, gs, kg + 2, P2{}, true);
                step(4 * gs + 3, gs, kg + 3, P3{}, true);
                if (!(STAGEW_DBG & 4)) {
                    gend(gs, gi);
                    greq(gs, gi + DG < NGall ? gi + DG : NGall - 1);
                }
            }
            k += D;
        }
#pragma unroll
        for (int gs = 0; gs < DG; ++gs) {  // the remainder: up to D - 1 steps, the last group possibly partial
            const int kg = k + 4 * gs;
            if (kg < N) {
                step(4 * gs + 0, gs, kg + 0, P0{}, false);
                if (kg + 1 < N) step(4 * gs + 1, gs, kg + 1, P1{}, false);
                if (kg + 2 < N) step(4 * gs + 2, gs, kg + 2, P2{}, false);
                if (kg + 3 < N) step(4 * gs + 3, gs, kg + 3, P3{}, false);
                gend(gs, kg >> 2);
            }
        }
        if constexpr (FUSE && sizeof(T) == 4) {
            int dummy = 0;
            T neg = -xm;
            wave_argmin_dpp(neg, dummy);
            xmax = -neg;
        }
    };
    // ---- the general constraint layout: [C | D] packed once -- row i (or r, when they do not change along the horizon) in the
    // order of Zs's rows, as NQ + 1 four-vectors, zero-padded, vector-major so that the lanes of a pass read side by side -- and
    // ONE pass over the m rows behind every forward sweep: lane <-> row i = k mk + r, GU rows per lane in flight
    constexpr int GU = sizeof(T) == 4 ? 2 : 1;
    for (int i = lane; i < (FUSE ? 0 : Mg); i += 64) {
        const int k = stepof(i), r = i - k * mk;
        V4 g[NQ + 1];
#pragma unroll
        for (int pos = 0; pos < ZL; ++pos) {
            const int gq = pos / (NQ + 1), q = pos - gq * (NQ + 1);  // position g (NQ + 1) + q
            T v = T(0);
            if (q < NQ) {
                if (gC && 4 * q + gq < nx) v = gC[k * sC + r * nx + 4 * q + gq];
            } else if (gD && gq < nu) {
                v = gD[k * sD + r * nu + gq];
            }
            g[pos / 4][pos % 4] = v;
        }
#pragma unroll
        for (int q = 0; q <= NQ; ++q) Gp[(int64_t)q * Mg + i] = g[q];
    }
    auto rowpass = [&](int mode, T fac) {
        for (int i0 = lane; i0 < M; i0 += 64 * GU) {
            V4 g[GU][NQ + 1], zq[GU][NQ + 1];
            T ra[GU], rb[GU], rc[GU];
#pragma unroll
            for (int u = 0; u < GU; ++u) {
                const int i = i0 + 64 * u < M ? i0 + 64 * u : M - 1;
                const int k = stepof(i);
                const int gi = ginv ? i - k * mk : i;
                const V4 *zr = (const V4 *)(Zs + (unsigned)(k * ZL));
#pragma unroll
                for (int q = 0; q <= NQ; ++q) {
                    g[u][q] = Gp[(unsigned)(q * Mg + gi)];
                    zq[u][q] = zr[q];
                }
                ra[u] = ge[k * sE + (i - k * mk)];
                rb[u] = mode == FW_INIT ? T(0) : thr[i];
                rc[u] = mode == FW_INIT ? T(0) : invn[i];
            }
#pragma unroll
            for (int u = 0; u < GU; ++u)
                if (i0 + 64 * u < M) {
                    T hs = T(0), hsa = T(0), nn = T(0);
#pragma unroll
                    for (int q = 0; q <= NQ; ++q)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            hs += g[u][q][j] * zq[u][q][j];
                            if (sizeof(T) == 4) hsa += (T)fabs((double)(g[u][q][j] * zq[u][q][j]));
                            nn += g[u][q][j] * g[u][q][j];
                        }
                    const T iv = mode == FW_INIT ? (nn > T(0) ? (T)rsqrt((double)nn) : T(1)) : rc[u];
                    rowlogic(mode, i0 + 64 * u, hs, hsa, ra[u], rb[u], iv, fac);
                }
        }
    };
    // a forward sweep and what follows it: the rows, the reduction of the selection
    auto fsweep = [&](auto modec, const T *xs, unsigned yoff, T fac) {
        constexpr int mode = decltype(modec)::value;
        selb = INF;
        seli = 0x7fffffff;
        selv = T(0);
        offa = false;
        forward(modec, xs, yoff, fac);
        if constexpr (!FUSE) {
            wave_sync_workgroup();  // (the trajectory is read by other lanes)
            rowpass(mode, fac);
        }
        sel_reduce();
        offa = __ballot(offa) != 0ull;
    };
    using FwInit = std::integral_constant<int, FW_INIT>;
    using FwEval = std::integral_constant<int, FW_EVAL>;
    using FwEvalR = std::integral_constant<int, FW_EVALR>;

    // the right-hand sides of a backward sweep: column 0 carries the candidate row bi, columns 1 .. R - 1 the rows NEXT IN LINE -- the
    // inactive rows of smallest scaled slack, violated or not yet: a row close to its bound is the likeliest to be asked for by the
    // steps to come, and a cached row costs a dot product per step where a row that is not costs a backward sweep and an evaluation --
    // (the whitened vector y_a of a row does not depend on the active set: a row found among them later costs no sweep; which
    // rows ride along has no influence on the iterates). Per lane: its column's row, the row's step, (p_kq, y_kq) to inject there;
    // kmax = the latest of the steps.
    // warm-state record (MpcqpSolveOpts.warm_state): int32 count, then the rows that were active when the last solve ended
    int *wrec = ka.warm_state ? (int *)((char *)ka.warm_state + prob * (int64_t)stagew_warm_bytes(maxq)) : nullptr;
    int wcnt = 0, wpos = 0;
    if (wrec && ka.warm_start == MPCQP_WARM_ACTIVE_SET) {
        wcnt = __builtin_amdgcn_readfirstlane(wrec[0]);  // (wave-uniform: scalar registers)
        wcnt = (wcnt < 0 || wcnt > maxq) ? 0 : wcnt;     // (a record that is not one: no warm rows)
    }
    constexpr int TU = sizeof(T) == 4 ? 8 : 4;  // rows per lane requested together
    auto candidates = [&](int bi, int &myrow, int &mykq, int &kmax, MV &st, T &ffs) {
        // rows[0] = the candidate; then the next most violated rows (per-lane top two, R - 1 wave minima)
        int rows[R];
        rows[0] = bi;
        int jstart = 1;  // rows[1 .. jstart - 1] come from the warm list
        if (wpos < wcnt) {
            // MPCQP_WARM_ACTIVE_SET: the rows that were active at the end of the previous solve (moved with the horizon) ride
            // along FIRST -- y_a does not depend on the active set, so when the iterations ask for one of them
            // its sweep is already done. Sixteen ids are examined per call (one round trip): in range, not the candidate,
            // not active now.
            const int t = lane & 15;
            const int id = wpos + t < wcnt ? wrec[1 + wpos + t] - ka.warm_shift : -1;
            bool okr = id >= 0 && id < M && id != bi && lane < 16;
            if (okr) okr = !(thr[id] == INF);
            unsigned okm = (unsigned)__ballot(okr) & 0xffffu;
            int last = -1;
#pragma unroll
            for (int j = 1; j < R; ++j) {
                if (okm) {
                    const int b = (int)__builtin_ctz(okm);
                    okm &= okm - 1;
                    rows[j] = __shfl(id, b);
                    last = b;
                    jstart = j + 1;
                } else {
                    rows[j] = -1;
                }
            }
            wpos += (okm != 0u) ? last + 1 : 16;  // (ids left over are examined again by the next call)
        }
        {
            T b1 = INF, b2 = INF;
            int i1 = 0x7fffffff, i2 = 0x7fffffff;
            for (int i0 = lane; i0 < M; i0 += 64 * TU) {
                T sv[TU], iv[TU], th[TU];
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    const unsigned i = (unsigned)(i0 + 64 * u < M ? i0 + 64 * u : M - 1);
                    sv[u] = sl[i];
                    iv[u] = FUSE ? invr_l[(i - stepof((int)i) * mk) & 15] : invn[i];
                    th[u] = thr[i];
                }
#pragma unroll
                for (int u = 0; u < TU; ++u) {
                    const int i = i0 + 64 * u;
                    const T sc = sv[u] * iv[u];
                    bool dup = false;  // a warm row that is violated as well must not take a second sweep slot
                    if (jstart > 1) {  // (wave-uniform; only the launch's first selections carry warm rows)
#pragma unroll
                        for (int j = 1; j < R; ++j) dup = dup || (j < jstart && rows[j] == i);
                    }
                    if (i < M && th[u] < INF && sv[u] < T(1e29) && i != bi && !dup) {  // (not active -- an active row's threshold is infinite --, a real bound)
                        if (sc < b1) {
                            b2 = b1;
                            i2 = i1;
                            b1 = sc;
                            i1 = i;
                        } else if (sc < b2) {
                            b2 = sc;
                            i2 = i;
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 1; j < R; ++j) {
                if (j < jstart) continue;  // (wave-uniform)
                T v = b1;
                int ix = i1;
                wave_argmin_dpp(v, ix);
                rows[j] = (v < INF) ? ix : -1;
                if (v < INF && ix == i1) {
                    b1 = b2;
                    i1 = i2;
                    b2 = INF;
                    i2 = 0x7fffffff;
                }
            }
        }
        myrow = -1;
#pragma unroll
        for (int j = 0; j < R; ++j)
            if (c16 == j) myrow = rows[j];
        // (p_kq, y_kq) of this lane's row (kq, rq): p = -C' + K' D', y = Ls^-1 D'  (r = -D'; the costate above kq is zero)
        st = MV{T(0), T(0), T(0), T(0)};
        ffs = T(0);
        mykq = -1;
        if (myrow >= 0) {
            const int kq = stepof(myrow), rq = myrow - kq * mk;
            mykq = kq;
            // K' and Ls^-1 of step kq are read out of the step's FORWARD record [[Acl, B Ls^-T], [-K, Ls^-T]]: entry e of lane L sits at
            // (e / LF) 64 LF + L LF + e % LF; K'[c][i] = K[i][c] and Ls^-1[a][j] live in the lanes of row group c % 4 / a whose column
            // maps to input i / j (stacked layout: columns NXC + i, entries q = c / 4 and NQ; two-block layout: rows i of the second
            // block, entries NQ + 1 + q and 2 NQ + 1)
            const T *mf = Mf + (unsigned)(kq * SF);
            auto unmap = [](int lc) { return sizeof(T) == 4 ? 4 * (lc & 3) + (lc >> 2) : lc; };  // (the inverse of Mfma::rowmap)
            auto recf = [&](int L, int e) { return mf[(e / LF) * 64 * LF + L * LF + e % LF]; };
            T dd[NU], cq[NQ], kq4[NQ][NU], li[NU];  // every load first, then the arithmetic
#pragma unroll
            for (int i = 0; i < NU; ++i) {
                dd[i] = (gD && i < nu) ? gD[kq * sD + rq * nu + i] : T(0);
                const int L = 16 * pg + unmap(STACK ? NXC + i : i);
                li[i] = recf(L, STACK ? NQ : 2 * NQ + 1);  // Ls^-1[pg][i]
#pragma unroll
                for (int q = 0; q < NQ; ++q) kq4[q][i] = -recf(L, STACK ? q : NQ + 1 + q);  // K'[4 q + pg][i]
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                const int c = 4 * q + pg;
                cq[q] = (gC && c < nx) ? gC[kq * sC + rq * nx + c] : T(0);
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                T v = -cq[q];
#pragma unroll
                for (int i = 0; i < NU; ++i) v += kq4[q][i] * dd[i];
                st[q] = (4 * q + pg < nx) ? v : T(0);
            }
            ffs = T(0);
#pragma unroll
            for (int i = 0; i < NU; ++i) ffs += li[i] * dd[i];  // (Ls^-1 D')[pg]
        }
        kmax = -1;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int kj = rows[j] >= 0 ? stepof(rows[j]) : -1;
            kmax = kj > kmax ? kj : kmax;
        }
        kmax = __builtin_amdgcn_readfirstlane(kmax);  // (wave-uniform, but it came out of vector registers: the sweep's loop control and
                                                      // its records' addresses belong on the scalar unit)
    };

    // ================================================================= unconstrained minimiser, slacks, first selection
    tick(2);
    {
        MV pN = {T(0), T(0), T(0), T(0)};
        if (termQ && col0) {
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (4 * q + pg < nx) pN[q] = -(T)ka.wt * ggoal[4 * q + pg];
        }
        if constexpr (!STACK) backward(std::true_type{}, -1, pN, T(0), -1);  // (nx <= 12: done inside the recursion)
    }
    wave_sync_workgroup();
    tick(3);
    // ---- LDS of the active set (round 6): the thin QR factorisation Y_A = Q R of the active rows' whitened vectors. R (upper
    // triangular, by COLUMNS through a permutation: nothing is copied when a row leaves) sits in a WL x WL tile of LDS and
    // moves to the workspace when the 33rd row arrives; Q (vectors of nv4 entries) lives in the workspace, every pass over it
    // with the same lane <-> step mapping: no exchange through memory between its passes. d = Q' y (cv), r = R^-1 d (rv), the
    // multipliers, the rows' ids, a scratch vector (ev: re-orthogonalisation, rotations), the rows cached by the backward sweeps.
    T *vpt = ws + wl.vpt, *Qs = ws + wl.Q, *Wm = ws + wl.W;
    for (int a = lane; a < maxq; a += 64) colp[a] = a;
    if (lane < R) crow[lane] = -1;
    if constexpr (FUSE) {
        if (c16 < 4) invr_l[(4 * pg + c16) & 15] = myinvn;
    }
    // the point in whitened coordinates: v = y0 (the sweeps' lane <-> step mapping of the vector passes: lane k % 64 owns step k)
    for (int k = lane; k < N; k += 64) ((V4 *)vpt)[k] = ((const V4 *)ffv)[k];
    lsync();
    fsweep(FwInit{}, gx0, (unsigned)wl.ff, T(0));
    tick(4);
    if constexpr (STAGEW_DBG != 0) {  // (timing experiments: the state is garbage from here on -- stop)
        if (lane == 0) {
            if (stamp)
                for (int i2 = 5; i2 < 8; ++i2) stamp[i2] = stamp[4];
            if (ka.status) ka.status[prob] = MPCQP_MAX_ITER;
            if (ka.iters) ka.iters[prob] = 0;
        }
        return;
    }
    tick(5);

    int nq = 0, iters = 0, status = MPCQP_MAX_ITER;
    const int max_iter = ka.max_iter;
    bool fail = false, slotsfull = false, wglob = false;
    const T DEP = sizeof(T) == 4 ? T(1e-10) : T(1e-26);  // |z|^2 <= DEP |y|^2: the row depends on the active ones
    auto dot4 = [](V4 a, V4 b) { return (a[0] * b[0] + a[1] * b[1]) + (a[2] * b[2] + a[3] * b[3]); };
    auto Q4 = [&](int a) { return (V4 *)(Qs + (int64_t)a * nv4); };
    // d = Q' y into cv, z = y - Q d into zq; when that cancelled (|z|^2 < |y|^2 / 4) once more on z, the second pass's coefficients
    // added to d (classical Gram-Schmidt with re-orthogonalisation on demand); returns |z|^2 as the SUM of z's squares.
    // y: a cached row's vector, zero behind its step kq (the array holds stale values there).
    auto ortho = [&](const T *yp, int kq, T *zq, T &yy) -> T {
        T zz = T(0);
        for (int pass = 0; pass < 2; ++pass) {
            const V4 *src = (const V4 *)(pass == 0 ? yp : zq);
            const int klim = pass == 0 ? kq : N - 1;
            T *co = pass == 0 ? cv : ev;
            const V4 zero4v = {T(0), T(0), T(0), T(0)};
            for (int a0 = 0; a0 < nq; a0 += 4) {  // four vectors per round: their loads overlap
                T p0 = T(0), p1 = T(0), p2 = T(0), p3 = T(0);
                const V4 *q0 = Q4(a0), *q1 = Q4(a0 + 1 < nq ? a0 + 1 : a0), *q2 = Q4(a0 + 2 < nq ? a0 + 2 : a0), *q3 = Q4(a0 + 3 < nq ? a0 + 3 : a0);
                for (int k = lane; k < N; k += 64) {
                    const V4 sv = k <= klim ? src[k] : zero4v;
                    const V4 v0 = q0[k], v1 = q1[k], v2 = q2[k], v3 = q3[k];
                    p0 += dot4(v0, sv);
                    p1 += dot4(v1, sv);
                    p2 += dot4(v2, sv);
                    p3 += dot4(v3, sv);
                }
                p0 = wave_sum_dpp(p0);
                p1 = wave_sum_dpp(p1);
                p2 = wave_sum_dpp(p2);
                p3 = wave_sum_dpp(p3);
                if (lane == 0) {
                    co[a0] = p0;
                    if (a0 + 1 < nq) co[a0 + 1] = p1;
                    if (a0 + 2 < nq) co[a0 + 2] = p2;
                    if (a0 + 3 < nq) co[a0 + 3] = p3;
                }
            }
            lsync();
            T part = T(0), ypart = T(0);
            for (int k = lane; k < N; k += 64) {
                V4 acc = k <= klim ? src[k] : zero4v;
                ypart += dot4(acc, acc);
                int a = 0;
                for (; a + 4 <= nq; a += 4) {
                    const V4 v0 = Q4(a)[k], v1 = Q4(a + 1)[k], v2 = Q4(a + 2)[k], v3 = Q4(a + 3)[k];
                    const T c0 = co[a], c1 = co[a + 1], c2 = co[a + 2], c3 = co[a + 3];
                    acc -= c0 * v0 + c1 * v1;
                    acc -= c2 * v2 + c3 * v3;
                }
                for (; a < nq; ++a) acc -= co[a] * Q4(a)[k];
                ((V4 *)zq)[k] = acc;
                part += dot4(acc, acc);
            }
            const T prev = pass == 0 ? wave_sum_dpp(ypart) : zz;
            if (pass == 0) yy = prev;
            zz = wave_sum_dpp(part);
            if (pass == 1) {
                for (int a = lane; a < nq; a += 64) cv[a] += ev[a];
                lsync();
            }
            if (pass == 0 && (nq == 0 || zz >= T(0.25) * prev)) break;  // no cancellation: Q' z is at rounding level already
        }
        return zz;
    };
    // g_c = y_c . z of the cached rows (what their slacks gain per unit step along z) into cg[]
    auto cached_dots = [&](const T *zq) {
        for (int j0 = 0; j0 < R; j0 += 4) {
            T p[4] = {T(0), T(0), T(0), T(0)};
            int kj[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) kj[u] = (j0 + u < R && crow[j0 + u < R ? j0 + u : 0] >= 0) ? stepof(crow[j0 + u]) : -1;
            for (int k = lane; k < N; k += 64) {
                const V4 zv = ((const V4 *)zq)[k];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const V4 yv = ((const V4 *)(ffv + (int64_t)(j0 + u < R ? j0 + u : 0) * nv4))[k];
                    if (k <= kj[u]) p[u] += dot4(yv, zv);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const T g = wave_sum_dpp(p[u]);
                if (lane == 0 && j0 + u < R) cg[j0 + u] = g;
            }
        }
        lsync();
    };
    // The same for horizons of at most 64 steps with at most QF active rows (a lane holds ONE four-vector of every vector): every
    // load of the iteration -- the candidate's vector, Q, the cached rows' vectors -- is issued up front (one round trip), Q is
    // read once. Leaves d in cv, z in zq, g_c in cg[]; returns |z|^2.
    // (registers: the default instantiations run three / two wavefronts per SIMD, and float64 four-vectors are eight registers)
    constexpr int QF = (LOW && sizeof(T) == 4) ? 8 : (sizeof(T) == 4 ? STAGEW_QFD : 4);
    // Small-batch instantiation (one wavefront per SIMD: what an iteration costs is its round trips): copies of the cached rows'
    // vectors and of the first QF vectors of Q in LDS (written behind the backward sweep / by the step that appends a vector; a
    // leaving row invalidates the copies from its slot on, which are read again from the workspace).
    constexpr bool VLDS = LOW;
    T *yl = Wl_end, *ql = yl + (VLDS ? R * 256 : 0);  // (horizons of at most 64 steps: a vector is 256 entries)
    int qvalid = 0;  // vectors of Q valid in ql
    auto stage_cached = [&]() {  // (behind a backward sweep) the cached rows' vectors into LDS, zero behind their steps
        if constexpr (VLDS) {
            if (N <= 64) {
                const V4 zero4v = {T(0), T(0), T(0), T(0)};
                const int k = lane < N ? lane : N - 1;
                V4 v[R];
#pragma unroll
                for (int j = 0; j < R; ++j) v[j] = ((const V4 *)(ffv + (int64_t)j * nv4))[k];
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const int rj = crow[j];
                    ((V4 *)(yl + j * 256))[lane] = (lane < N && rj >= 0 && k <= stepof(rj)) ? v[j] : zero4v;
                }
            }
        }
    };
    V4 zlast = {T(0), T(0), T(0), T(0)};  // z of the latest ortho_small (this lane's four-vector)
    V4 vreg = {T(0), T(0), T(0), T(0)};   // the point v (this lane's four-vector) while the loop stays on the small path
    bool vreg_ok = false;
    // The whole vector work of an iteration for horizons of at most 64 steps with at most QF active rows (a lane holds ONE four-vector
    // of every vector): Q is read once, and the ~20 sums over the wavefront -- d = Q' y, |y|^2, |z|^2, the cached rows' y_c . z -- are
    // a few multi-reductions (multi_sum). Leaves d in cv, z in zq and zlast, g_c in cg[]; returns |z|^2.
    constexpr int K1 = QF == 8 ? 16 : 8;            // first batch: d_0 .. d_{QF-1}, |y|^2
    constexpr int RB = (LOW && sizeof(T) == 4) ? 16 : 4;  // the cached rows' dots per batch (|z|^2 rides in the first one's last cell)
    auto ortho_small = [&](const T *yp, int hit, int kq, T *zq, T &yy, T &dmine, T &cgmine) -> T {
        const V4 zero4v = {T(0), T(0), T(0), T(0)};
        const int k = lane < N ? lane : N - 1;
        const bool kin = lane < N;
        V4 qv[QF], yv, ycu[LOW ? 1 : R];  // (ycu: the cached rows' vectors of the default instantiations, requested up front)
        auto cached = [&](int j) -> V4 {  // the cached row's vector (this lane's four-vector), zero behind the row's step
            if constexpr (VLDS) {
                return ((const V4 *)(yl + j * 256))[lane];
            } else {
                const V4 v = ((const V4 *)(ffv + (int64_t)j * nv4))[k];
                const int rj = crow[j];
                return (kin && rj >= 0 && k <= stepof(rj)) ? v : zero4v;
            }
        };
        if constexpr (VLDS) {
            for (int u = qvalid; u < nq; ++u) ((V4 *)(ql + u * 256))[lane] = kin ? Q4(u)[k] : zero4v;  // (rare: behind a leaving row)
            qvalid = nq;
            lsync();
            yv = ((const V4 *)(yl + hit * 256))[lane];
#pragma unroll
            for (int u = 0; u < QF; ++u) qv[u] = ((const V4 *)(ql + (u < nq ? u : 0) * 256))[lane];
        } else {
            const V4 yv0 = ((const V4 *)yp)[k];
#pragma unroll
            for (int u = 0; u < QF; ++u) qv[u] = Q4(u < nq ? u : 0)[k];
            if constexpr (!LOW && !STAGEW_YCU_LATE) {
#pragma unroll
                for (int j = 0; j < R; ++j) ycu[j] = cached(j);
            }
            yv = (kin && k <= kq) ? yv0 : zero4v;
        }
        T p1[K1], dd[QF];
#pragma unroll
        for (int u = 0; u < K1; ++u) p1[u] = T(0);
#pragma unroll
        for (int u = 0; u < QF; ++u) {
            if (!kin || u >= nq) qv[u] = zero4v;
            p1[u] = dot4(qv[u], yv);
        }
        p1[QF] = dot4(yv, yv);
        if constexpr (LOW || (STAGEW_MSUMD && sizeof(T) == 4)) {
            const T r1 = multi_sum<T, K1>(p1, lane);
#pragma unroll
            for (int u = 0; u < QF; ++u) dd[u] = lane_get(r1, u);
            yy = lane_get(r1, QF);
        } else {  // (three / two wavefronts per SIMD hide a wave_sum's chain, and the multi-reduction's registers spill there)
#pragma unroll
            for (int u = 0; u < QF; ++u) dd[u] = u < nq ? wave_sum_dpp(p1[u]) : T(0);
            yy = wave_sum_dpp(p1[QF]);
        }
        V4 zv = yv;
#pragma unroll
        for (int u = 0; u < QF; ++u) zv -= dd[u] * qv[u];
        if constexpr (!LOW && STAGEW_YCU_LATE) {  // (requested behind Q's use: a second round trip, fewer live registers)
#pragma unroll
            for (int j = 0; j < R; ++j) ycu[j] = cached(j);
        }
        T zz = T(0);
        bool redo = false;
        for (int pass = 0; pass < 2; ++pass) {
            if constexpr (RB == 16) {  // every cached row and |z|^2 in one reduction
                T p2[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) p2[u] = T(0);
#pragma unroll
                for (int j = 0; j < R; ++j) p2[j] = dot4(cached(j), zv);
                p2[15] = dot4(zv, zv);
                const T r2 = multi_sum<T, 16>(p2, lane);
                zz = lane_get(r2, 15);
                cgmine = r2;  // (lane j: y_j . z)
            } else if constexpr (LOW) {  // groups of three cached rows; |z|^2 in cell 3 of the first group
                for (int j0 = 0; j0 < R; j0 += 3) {
                    T p2[4];
#pragma unroll
                    for (int u = 0; u < 3; ++u) p2[u] = j0 + u < R ? dot4(cached(j0 + u < R ? j0 + u : R - 1), zv) : T(0);
                    p2[3] = dot4(zv, zv);
                    const T r2 = multi_sum<T, 4>(p2, lane);
                    zz = lane_get(r2, 3);
#pragma unroll
                    for (int u = 0; u < 3; ++u) cgmine = lane == j0 + u ? lane_get(r2, u) : cgmine;
                }
            } else if constexpr (STAGEW_MSUMD && sizeof(T) == 4 && R <= 7) {  // the cached rows and |z|^2 in one reduction of eight
                T p2[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) p2[u] = T(0);
#pragma unroll
                for (int j = 0; j < R; ++j) p2[j] = dot4(ycu[j], zv);
                p2[7] = dot4(zv, zv);
                const T r2 = multi_sum<T, 8>(p2, lane);
                zz = lane_get(r2, 7);
                cgmine = r2;  // (lane j < R: y_j . z)
            } else {  // a wave_sum per cached row (their vectors were requested with Q's: one round trip for the iteration)
                zz = wave_sum_dpp(dot4(zv, zv));
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const T g = wave_sum_dpp(dot4(ycu[j], zv));
                    cgmine = lane == j ? g : cgmine;
                }
            }
            redo = pass == 0 && nq > 0 && zz < T(0.25) * yy;
            if (!redo) break;
            // cancellation (rare): once more on z
#pragma unroll
            for (int u = 0; u < QF; ++u) {
                const T e2 = u < nq ? wave_sum_dpp(dot4(qv[u], zv)) : T(0);
                dd[u] += e2;
                zv -= e2 * qv[u];
            }
        }
        if (kin) ((V4 *)zq)[k] = zv;
        if constexpr (LOW) zlast = zv;
        dmine = T(0);
#pragma unroll
        for (int u = 0; u < QF; ++u) dmine = lane == u ? dd[u] : dmine;  // (lane a: d_a)
        return zz;
    };
    // r = R^-1 d (d in cv) into rv: back substitution, column b of R read by the lanes of the rows above it
    auto rsolve = [&](const T *Rp, int ld) {
        for (int a = lane; a < nq; a += 64) rv[a] = cv[a];
        lsync();
        for (int b = nq - 1; b >= 0; --b) {
            const T *col = Rp + (int64_t)colp[b] * ld;
            const T rb = rv[b] / col[b];
            for (int j = lane; j < b; j += 64) rv[j] -= col[j] * rb;
            if (lane == 0) rv[b] = rb;
            lsync();
        }
    };
    // ... the same for at most QF active rows whose factor sits in the LDS tile: lane j < nq takes row j of R into registers (one
    // round trip for all entries), the substitution runs on lane reads -- no LDS hand-over per step; d arrives and r leaves in a
    // register (lane a: d_a, r_a).
    auto rsolve_small = [&](T dmine) -> T {
        const int cp = colp[lane < maxq ? lane : 0];  // (lane b holds the physical column of slot b)
        T acc = lane < nq ? dmine : T(0);
        T row[QF], dg = T(1);
#pragma unroll
        for (int b = 0; b < QF; ++b) {
            const int cb = __builtin_amdgcn_readlane(cp, b);
            const T e_ = Rl[cb * WLD + (lane < QF ? lane : 0)];  // R[lane][b]
            row[b] = (b < nq && lane < b) ? e_ : T(0);
            dg = (lane == b && b < nq) ? e_ : dg;
        }
        const T idg = T(1) / dg;
#pragma unroll
        for (int b = QF - 1; b >= 0; --b) {
            if (b < nq) {  // (wave-uniform)
                const T rb = lane_get(acc * idg, b);
                acc = lane == b ? rb : acc - row[b] * rb;
            }
        }
        return lane < nq ? acc : T(0);
    };
    // w = R^-T rho (rho in cv) into ev: forward substitution, a dot product along column b per step
    auto rtsolve = [&](const T *Rp, int ld) {
        for (int b = 0; b < nq; ++b) {
            const T *col = Rp + (int64_t)colp[b] * ld;
            T part = T(0);
            for (int j = lane; j < b; j += 64) part += col[j] * ev[j];
            const T wb = (cv[b] - wave_sum_dpp(part)) / col[b];
            if (lane == 0) ev[b] = wb;
            lsync();
        }
    };
    // the candidate becomes basis vector nq: Q gains z / |z|, R the column [d; |z|]
    auto append = [&](T *Rp, int ld, T *zq, T zz, T up, int bi, bool small, T dmine) {
        const T zn = (T)sqrt((double)zz), izn = T(1) / zn;
        if (LOW && small) {  // (z is in a register: no load; the small-batch instantiation's copy of Q takes the vector as well)
            const V4 qn = zlast * izn;
            if (lane < N) ((V4 *)zq)[lane] = qn;
            if constexpr (VLDS) {
                if (qvalid == nq && nq < QF) {
                    ((V4 *)(ql + nq * 256))[lane] = lane < N ? qn : V4{T(0), T(0), T(0), T(0)};
                    qvalid = nq + 1;
                }
            }
        } else {
            for (int k = lane; k < N; k += 64) ((V4 *)zq)[k] *= izn;
        }
        T *col = Rp + (int64_t)colp[nq] * ld;
        if (small) {
            if (lane < nq) col[lane] = dmine;
        } else {
            for (int a = lane; a < nq; a += 64) col[a] = cv[a];
        }
        if (lane == 0) {
            col[nq] = zn;
            lamv[nq] = up;
            actrow[nq] = bi;
        }
    };
    // slot l leaves: its column of R goes (the permutation closes the gap, the small per-slot arrays move down by one), and one
    // Givens rotation per column behind it -- on two rows of R and two vectors of Q -- restores the triangle. Lane b carries
    // column b's entry of the MOVING row in cv[b]; what a step reads of R no earlier step of this drop has written.
    auto drop = [&](int l, T *Rp, int ld) {
        const int k = nq - 1, rowl = actrow[l], saved = colp[l];
        for (int a0 = l; a0 < k; a0 += 64) {  // (chunks ascending: a chunk reads before any lane writes it)
            const int a = a0 + lane;
            int c = 0, ar = 0;
            T lv = T(0);
            if (a < k) {
                c = colp[a + 1];
                ar = actrow[a + 1];
                lv = lamv[a + 1];
            }
            lsync();
            if (a < k) {
                colp[a] = c;
                actrow[a] = ar;
                lamv[a] = lv;
            }
            lsync();
        }
        if (lane == 0) colp[k] = saved;
        lsync();
        for (int b = l + lane; b < k; b += 64) cv[b] = Rp[(int64_t)colp[b] * ld + l];
        lsync();
        for (int j = l; j < k; ++j) {  // zero R[j + 1][j] against R[j][j]
            const T aj = cv[j], bj = Rp[(int64_t)colp[j] * ld + j + 1];
            const T hh = (T)sqrt((double)(aj * aj + bj * bj));
            const T cc = hh > T(0) ? aj / hh : T(1), ss = hh > T(0) ? bj / hh : T(0);
            for (int b = j + lane; b < k; b += 64) {
                T *cb = Rp + (int64_t)colp[b] * ld;
                const T u = cb[j + 1], mv = cv[b];
                cb[j] = cc * mv + ss * u;
                cv[b] = cc * u - ss * mv;
            }
            if (lane == 0) {
                rv[j] = cc;
                ev[j] = ss;
            }
            lsync();
        }
        for (int kk = lane; kk < N; kk += 64) {  // Q takes the rotations in one pass (lane <-> steps: no exchange)
            V4 t1 = Q4(l)[kk];
            V4 un = l < k ? Q4(l + 1)[kk] : t1;
            for (int j = l; j < k; ++j) {
                const V4 u2 = un;
                if (j + 1 < k) un = Q4(j + 2)[kk];
                const T cc = rv[j], ss = ev[j];
                Q4(j)[kk] = cc * t1 + ss * u2;
                t1 = cc * u2 - ss * t1;
            }
        }
        if (lane == owner(rowl)) {  // (the row's owner) the row can be selected again
            const int kr = stepof(rowl), r = rowl - kr * mk;
            thr[rowl] = tol + tol * (T)fabs((double)ge[kr * sE + r]);
        }
    };

    // ================================================================= active-set loop (Goldfarb-Idnani; oracle/stagewise_qr_np.py)
    // Between two evaluations of the point the loop works on the rows whose whitened vectors the latest backward sweep cached
    // (the most violated row and the R - 1 next ones): a row's slack moves by t y_c . z with a step -- a dot product, no sweep --,
    // the most violated CACHED row is taken next (any violated row is a valid Goldfarb-Idnani choice: the dual objective grows
    // with every full step), and when none of them is violated the point is evaluated from scratch: ONE forward sweep of v from
    // x0 gives every row's slack, the inputs, the check of the active rows and the most violated row of all, with which the
    // next backward sweep starts. No slack is ever updated incrementally across evaluations.
    T best = selb, sp = selv;
    int bi = seli;
    int polish = 0;
    // the cached rows' state, one row per lane (lane j < R): row id, slack, threshold, selection metric, whether it is active now --
    // registers, so that the selection among them and their slacks' updates touch no memory (crow[] also sits in LDS for the
    // passes that look a row up by its column)
    int c_row = -1;
    T c_s = T(0), c_th = INF, c_iv = T(1);
    bool c_act = false;
    for (;;) {
        tacc(-1);
        if (!(best < INF)) {
            status = MPCQP_SOLVED;
            break;
        }
        {   // ---- the next R rows: the most violated one and the rows next in line; their whitened vectors (one backward sweep)
            int myrow, mykq, kmax;
            MV st;
            T ffs;
            wave_sync_workgroup();  // (the sweeps' rows are read by other lanes)
            if (stamp && lane == 0) stamp[15] += 1;
            candidates(bi, myrow, mykq, kmax, st, ffs);
            backward(std::false_type{}, kmax, st, ffs, mykq);
            const int rj = __shfl(myrow, lane & 15);  // (column j's row sits in the lanes with c16 == j)
            c_row = lane < R ? rj : -1;
            {
                const unsigned ri = (unsigned)(c_row >= 0 ? c_row : 0);
                c_s = sl[ri];
                c_th = thr[ri];
                c_iv = FUSE ? invr_l[((int)ri - stepof((int)ri) * mk) & 15] : invn[ri];
                c_act = false;
            }
            if (lane < R) crow[lane] = c_row;
            wave_sync_workgroup();
            stage_cached();
            lsync();
        }
        tacc(9);
        for (;;) {
            // ---- the most violated cached row
            int hit = lane;
            T sc = (c_row >= 0 && !c_act && c_s < -c_th) ? c_s * c_iv : INF;
            wave_argmin_dpp(sc, hit);
            if (!(sc < INF)) break;  // none: the point is evaluated from scratch
            tacc(8);
            bi = lane_get(c_row, hit);
            sp = lane_get(c_s, hit);
            const T *yp = ffv + (int64_t)hit * nv4;
            const int kq = stepof(bi);
            T up = T(0);
            bool added = false;
            while (!added) {
                if (iters >= max_iter) {
                    fail = true;
                    break;
                }
                ++iters;
                T *zq = Qs + (int64_t)nq * nv4;
                T yy, zz;
                // small: the whole iteration on registers -- d, r, the multipliers and the cached rows' gains one per lane
                const bool small = N <= 64 && nq <= QF && !wglob;
                T dmine = T(0), cgmine = T(0), rmine = T(0), lam_mine = T(0);
                T t1 = INF;
                int l = 0x7fffffff;
                if (small) {
                    lam_mine = lamv[lane < maxq ? lane : 0];  // (requested first: needed last)
                    zz = ortho_small(yp, hit, kq, zq, yy, dmine, cgmine);
                    tacc(10);
                    rmine = rsolve_small(dmine);
                    if (lane < nq && rmine > T(0)) {  // ---- ratio test on the multipliers
                        t1 = lam_mine / rmine;
                        l = lane;
                    }
                } else {
                    zz = ortho(yp, kq, zq, yy);
                    cached_dots(zq);
                    cgmine = cg[lane < R ? lane : 0];
                    tacc(10);
                    if (wglob)
                        rsolve(Wm, maxq);
                    else
                        rsolve(Rl, WLD);
                    for (int a = lane; a < nq; a += 64) {
                        const T ra = rv[a];
                        if (ra > T(0)) {
                            const T q = lamv[a] / ra;
                            if (q < t1) {
                                t1 = q;
                                l = a;
                            }
                        }
                    }
                }
                const bool can_move = (nq < nvar) && (zz > DEP * yy) && (zz > T(0));
                wave_argmin_dpp(t1, l);
                const T t2 = can_move ? -sp / zz : INF;
                const T t = t1 < t2 ? t1 : t2;
                if (!(t < INF)) {
                    status = MPCQP_INFEASIBLE;
                    fail = true;
                    break;
                }
                const bool full = (t2 <= t1);
                if (full && nq >= maxq) {  // every slot is taken (max_active < min(n, m)) -> MPCQP_SLOTS_FULL
                    fail = true;
                    slotsfull = true;
                    break;
                }
                tacc(11);
                if (can_move) {
                    // the step: the point moves against z (v -= t z), the slack of a cached row c gains t y_c . z (active rows stay on
                    // their bounds, the candidate's own gain is t |z|^2: it lands on its bound exactly with a full step)
                    if (LOW && small) {  // (the point's four-vector stays in a register while the loop stays on this path: no load)
                        if (!vreg_ok) vreg = ((const V4 *)vpt)[lane < N ? lane : N - 1];
                        vreg_ok = true;
                        vreg -= t * zlast;
                        if (lane < N) ((V4 *)vpt)[lane] = vreg;
                    } else {
                        for (int k = lane; k < N; k += 64) ((V4 *)vpt)[k] -= t * ((const V4 *)zq)[k];
                        vreg_ok = false;
                    }
                    c_s = c_act ? c_s : c_s + t * cgmine;
                    sp += t * zz;
                }
                tacc(12);
                // ---- multipliers
                if (small) {
                    if (lane < nq) {
                        const T v = lam_mine - t * rmine;
                        lamv[lane] = v < T(0) ? T(0) : v;
                    }
                } else {
                    for (int a = lane; a < nq; a += 64) {
                        const T v = lamv[a] - t * rv[a];
                        lamv[a] = v < T(0) ? T(0) : v;
                    }
                }
                up += t;
                if (full) {
                    if (!wglob && nq >= WL) {  // R outgrows its LDS tile: it moves to the workspace
                        for (int b = 0; b < WL; ++b)
                            for (int a = lane; a < WL; a += 64) Wm[(int64_t)b * maxq + a] = Rl[b * WLD + a];
                        wglob = true;
                    }
                    if (wglob)
                        append(Wm, maxq, zq, zz, up, bi, small, dmine);
                    else
                        append(Rl, WLD, zq, zz, up, bi, small, dmine);
                    ++nq;
                    added = true;
                    if (lane == owner(bi)) thr[bi] = INF;  // (the row's owner) active: infinite threshold
                    if (lane == hit) {
                        c_act = true;
                        c_s = T(0);
                    }
                } else {
                    const int rowl = actrow[l];
                    if (wglob)
                        drop(l, Wm, maxq);
                    else
                        drop(l, Rl, WLD);
                    --nq;
                    qvalid = qvalid < l ? qvalid : l;  // (the vectors from slot l on were rotated)
                    if (c_row == rowl) {  // (a cached row that leaves is tracked again, from its bound)
                        c_act = false;
                        c_s = T(0);
                    }
                }
                if (wglob)
                    wave_sync_workgroup();
                else
                    lsync();
                tacc(13);
            }
            if (fail) break;
        }
        if (fail) break;
        tacc(-1);
        // ================================================================= the point from scratch
        // One forward sweep of the whitened point v from x0 gives the inputs that are returned and every row (closed loop: stable
        // whatever the spectrum of A). The most violated inactive row, if there is one, starts the next round of the loop. If there
        // is none the point is the answer -- once its ACTIVE rows sit on their bounds: beyond the trigger a polish step
        // (S dlam = rho with S = R' R, the point moves along Q R^-T rho) and the evaluation again; a point that still fails the
        // acceptance bound is not reported solved.
        for (;;) {
            const T fac = polish < VPASS - 1 ? T(sizeof(T) == 4 ? STAGEW_VTRIG32 : 10)
                                             : (sizeof(T) == 4 ? T(STAGEW_VACC32) : (T(100) > T(1e-7) / tol ? T(100) : T(1e-7) / tol));
            wave_sync_workgroup();  // (v is read by the sweep's lanes)
            fsweep(FwEval{}, gx0, (unsigned)wl.vpt, fac);
            if (stamp && lane == 0) stamp[15] += 256;
            if (selb < INF || !offa) break;
            if (stamp && lane == 0) stamp[15] += 65536;
            if (++polish >= VPASS) {
                fail = true;
                break;
            }
            wave_sync_workgroup();
            fsweep(FwEvalR{}, gx0, (unsigned)wl.vpt, fac);  // (rare: the same evaluation once more, leaving every row's residual in s0)
            wave_sync_workgroup();  // (the rows' residuals are read by other lanes)
            for (int a = lane; a < nq; a += 64) cv[a] = s0[actrow[a]];
            lsync();
            if (wglob) {
                rtsolve(Wm, maxq);
            } else {
                rtsolve(Rl, WLD);
            }
            vreg_ok = false;
            for (int k = lane; k < N; k += 64) {  // v += Q w
                V4 acc = ((const V4 *)vpt)[k];
                for (int a = 0; a < nq; ++a) acc += ev[a] * Q4(a)[k];
                ((V4 *)vpt)[k] = acc;
            }
            for (int a = lane; a < nq; a += 64) cv[a] = ev[a];
            lsync();
            if (wglob)
                rsolve(Wm, maxq);
            else
                rsolve(Rl, WLD);
            for (int a = lane; a < nq; a += 64) {
                const T v = lamv[a] - rv[a];
                lamv[a] = v < T(0) ? T(0) : v;
            }
            lsync();
        }
        if (fail) break;
        tacc(14);
        best = selb;
        bi = seli;
        sp = selv;
    }
    tick(6);
    tick(7);
    if (fail && status == MPCQP_SOLVED) status = MPCQP_MAX_ITER;
    if (slotsfull) status = MPCQP_SLOTS_FULL;
    const bool ok = status == MPCQP_SOLVED;
    wave_sync_workgroup();
    {   // the inputs of the latest evaluation (rows of 4), or zeros when there is no plan
        const T *ust = ws + wl.ust;
        for (int i = lane; i < nv4; i += 64)
            if ((i & 3) < nu) ou[(i >> 2) * nu + (i & 3)] = ok ? ust[i] : T(0);
    }
    if (ka.lam) {
        T *ol = (T *)ka.lam + prob * (int64_t)M;
        for (int i = lane; i < M; i += 64) ol[i] = T(0);
        wave_sync_workgroup();
        if (ok)
            for (int a = lane; a < nq; a += 64) ol[actrow[a]] = lamv[a];
    }
    if (wrec) {  // the rows that are active now: the next solve's warm rows (MPCQP_WARM_ACTIVE_SET)
        if (lane == 0) wrec[0] = ok ? nq : 0;
        for (int a = lane; ok && a < nq; a += 64) wrec[1 + a] = actrow[a];
    }
    if (lane == 0) {
        if (ka.status) ka.status[prob] = status;
        if (ka.iters) ka.iters[prob] = iters;
    }
}

// ------------------------------------------------------------ host side
static bool g_invariant(const KernelArgs &ka)
{
    // (a size query carries no operands: it gets the larger, per-step layout)
    return (ka.C.ptr || ka.D.ptr) && (!ka.C.ptr || ka.C.step_stride == 0) && (!ka.D.ptr || ka.D.step_stride == 0);
}

bool stagew_supported(const KernelArgs &ka, int dtype)
{
    return (dtype == MPCQP_F64 || dtype == MPCQP_F32) && ka.nx >= 2 && ka.nx <= 16 && ka.nu >= 1 && ka.nu <= NU && ka.mk >= 1;
}

size_t stagew_ws_elems(const KernelArgs &ka, int maxq, int dtype)
{
    // (a size query carries no operands and does not know which layout the launch will take: the larger of the two)
    const size_t esz = dtype == MPCQP_F64 ? 8 : 4;
    // (... and not whether the small-batch instantiation, with its larger carve, will serve it: a workspace sized for one batch may
    // be used for a smaller one)
    size_t best = 0;
    for (int low = 0; low < 2; ++low) {
        const size_t a = (size_t)make_ws(ka.nx, ka.nu, ka.N, ka.mk, maxq, g_invariant(ka), esz, low != 0).total;
        const size_t b = ka.A.ptr ? 0 : (size_t)make_ws(ka.nx, ka.nu, ka.N, ka.mk, maxq, true, esz, low != 0).total;
        best = a > best ? a : best;
        best = b > best ? b : best;
    }
    return best;
}

// SIMDs of the current device (the small-batch instantiation serves launches of at most one wavefront per SIMD)
static int64_t device_simds()
{
    const int s = device_simds_now();
    return s > 0 ? s : 1024;
}

template <typename T, int NXC, bool FUSE, bool LOW = false>
static int launch_stagew_t(const KernelArgs &ka, int maxq, int64_t batch, void *ws, hipStream_t st)
{
    if constexpr (std::is_same<T, float>::value && FUSE && !LOW) {
        if (batch <= device_simds()) return launch_stagew_t<T, NXC, FUSE, true>(ka, maxq, batch, ws, st);
    }
    constexpr int RR = FUSE ? (LOW ? R_FUSE_LOW : R_FUSE) : R_PLAIN;
    const Ws wl = make_ws(ka.nx, ka.nu, ka.N, ka.mk, maxq, g_invariant(ka), sizeof(T), LOW);
    if (wl.total >= ((int64_t)1 << 31)) return MPCQP_ETOOLARGE;  // (the kernel addresses a problem's arrays with 32-bit offsets)
    // the matrix tiles of the LDS Riccati recursion only exist for nx > 12; then 8 constant / spare cells
    const size_t tiles = (size_t)((NXC <= 12 ? 0 : 6 * 16 * LD + 2 * 16 * 4 + 4 * 4 * LD + 16 + 16) + 8);
    // + d, r, multipliers, a scratch vector; active rows, column permutation of R, the backward sweeps' rows; the 32 x 33 tile of R
    const size_t lds = tiles * sizeof(T) + (size_t)maxq * (4 * sizeof(T) + 2 * sizeof(int)) + (size_t)RR * sizeof(int) + 16 +
                       (size_t)32 * 33 * sizeof(T) + (size_t)RR * sizeof(T) + 16 + 16 * sizeof(T) +
                       (LOW ? (size_t)(RR + 8) * 256 * sizeof(T) : 0);  // (LOW: copies of the cached rows' vectors and of up to eight vectors of Q)
    auto kern = mpcqp_stagew_kernel<T, NXC, FUSE, LOW>;
    // (developer knob: -DSTAGEW_LDS_PAD=<bytes> of unused LDS per wavefront lowers the number of resident wavefronts)
    const size_t lds_req = lds + (size_t)STAGEW_LDS_PAD;
    if (lds_req > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_req);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)batch), dim3(64), lds_req, st, ka, wl, (T *)ws, batch);
    return (int)hipGetLastError();
}

template <typename T, bool FUSE> static int launch_stagew_f(const KernelArgs &ka, int maxq, int64_t batch, void *ws, hipStream_t st)
{
    switch (nxc_of(ka.nx)) {
    case 4: return launch_stagew_t<T, 4, FUSE>(ka, maxq, batch, ws, st);
    case 8: return launch_stagew_t<T, 8, FUSE>(ka, maxq, batch, ws, st);
    case 12: return launch_stagew_t<T, 12, FUSE>(ka, maxq, batch, ws, st);
    default: return launch_stagew_t<T, 16, FUSE>(ka, maxq, batch, ws, st);
    }
}

template <typename T> static int launch_stagew_d(const KernelArgs &ka, int maxq, int64_t batch, void *ws, hipStream_t st)
{
    return fuse_ok(ka.mk, g_invariant(ka)) ? launch_stagew_f<T, true>(ka, maxq, batch, ws, st)
                                           : launch_stagew_f<T, false>(ka, maxq, batch, ws, st);
}

int launch_stagew(const KernelArgs &ka, int dtype, int maxq, int64_t batch, void *ws, hipStream_t st)
{
    return dtype == MPCQP_F64 ? launch_stagew_d<double>(ka, maxq, batch, ws, st) : launch_stagew_d<float>(ka, maxq, batch, ws, st);
}

}  // namespace mpcqp
