// mpcqp_quad_common.h -- what the four-problems-per-wavefront kernels share: the lean / shared-model kernel of mpcqp_quad.hip and the
// general kernel of mpcqp_quadg.hip (two or four constraint rows per lane). Device helpers of a problem that owns ONE 16-lane DPP row
// (reductions and broadcasts inside the row, the hand-written v_fmac_f64_dpp and the pin that gives it its wait states, 16-wide
// loads, stores and dot products, the fast reciprocals) and the LDS carve of one problem.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "mpcqp_internal.h"

namespace mpcqp {

namespace quad {

constexpr int NV = 16;  // padded number of variables / slots = lanes per problem

template <int CTRL> __device__ __forceinline__ unsigned dpp_u(unsigned x)
{
    return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}
constexpr int ROR8 = 0x128, ROR4 = 0x124, ROR2 = 0x122, ROR1 = 0x121;  // rotate within a row of 16

// all-reduce (min) over the 16 lanes of each row
__device__ __forceinline__ unsigned row_min(unsigned v)
{
    v = min(v, dpp_u<ROR8>(v));
    v = min(v, dpp_u<ROR4>(v));
    v = min(v, dpp_u<ROR2>(v));
    v = min(v, dpp_u<ROR1>(v));
    return v;
}
// value of lane `idx` (0..15; per lane, usually uniform inside a row) of the caller's own row
__device__ __forceinline__ int row_get(int x, int rb, int idx) { return __builtin_amdgcn_ds_bpermute((rb + idx) << 2, x); }
__device__ __forceinline__ double row_get(double x, int rb, int idx)
{
    const int a = (rb + idx) << 2;
    const int lo = __builtin_amdgcn_ds_bpermute(a, __double2loint(x));
    const int hi = __builtin_amdgcn_ds_bpermute(a, __double2hiint(x));
    return __hiloint2double(hi, lo);
}
// true in every lane of a row iff `pred` holds in one of its lanes
__device__ __forceinline__ bool row_any(bool pred, int rb)
{
    const unsigned long long b = __ballot(pred);
    return ((unsigned)(b >> rb) & 0xffffu) != 0u;
}
// order-preserving map of a double onto two unsigned words
__device__ __forceinline__ void ordered(double x, unsigned &hi, unsigned &lo)
{
    const unsigned h = (unsigned)__double2hiint(x), l = (unsigned)__double2loint(x);
    const bool neg = h & 0x80000000u;
    hi = neg ? ~h : (h | 0x80000000u);
    lo = neg ? ~l : l;
}
__device__ __forceinline__ void ld16(double (&d)[NV], const double *src)
{
    const double2 *p = reinterpret_cast<const double2 *>(src);
#pragma unroll
    for (int i = 0; i < NV / 2; ++i) {
        const double2 t = p[i];
        d[2 * i] = t.x;
        d[2 * i + 1] = t.y;
    }
}
__device__ __forceinline__ void st16(double *dst, const double (&s)[NV])
{
    double2 *p = reinterpret_cast<double2 *>(dst);
#pragma unroll
    for (int i = 0; i < NV / 2; ++i) {
        double2 t;
        t.x = s[2 * i];
        t.y = s[2 * i + 1];
        p[i] = t;
    }
}
__device__ __forceinline__ double dot16(const double (&a)[NV], const double (&b)[NV])
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
// two dot products with one vector, two chains each (a lone wavefront issues a dependent FMA every 8.5 cycles and an
// independent one every 5.1: four chains in flight are enough, and accumulators are registers the loop does not have)
__device__ __forceinline__ void dot16x2(const double (&a)[NV], const double (&b)[NV], const double (&x)[NV], double &ra, double &rb)
{
    double a0 = a[0] * x[0], a1 = a[1] * x[1], b0 = b[0] * x[0], b1 = b[1] * x[1];
#pragma unroll
    for (int k = 2; k < NV; k += 2) {
        a0 = fma(a[k], x[k], a0);
        b0 = fma(b[k], x[k], b0);
        a1 = fma(a[k + 1], x[k + 1], a1);
        b1 = fma(b[k + 1], x[k + 1], b1);
    }
    ra = a0 + a1;
    rb = b0 + b1;
}
__device__ __forceinline__ void pin(double &x) { asm volatile("" : "+v"(x)); }

// The value held by lane N of the caller's 16-lane row, in every lane of that row (v_mov_b64_dpp row_newbcast:N).
template <int N> __device__ __forceinline__ double row_bcast(double x) { return __builtin_amdgcn_mov_dpp(x, 0x150 + N, 0xf, 0xf, true); }
// acc += (x of lane N of the caller's row) * m in ONE instruction (v_fmac_f64_dpp). The compiler cannot see inside the asm:
// a register written by a VALU instruction needs two wait states before a DPP read, so every batch of these is preceded by
// dpp_ready(x) on its broadcast source (tools/check_dpp_hazards.py verifies that on the assembly).
template <int N> __device__ __forceinline__ void fmac_bcast(double &acc, double x, double m)
{
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(m), "n"(N));
}
__device__ __forceinline__ void dpp_ready(double &x) { asm volatile("s_nop 1" : "+v"(x)); }
// Compile-time loop: f(integral_constant<int, I>) for I = B .. E-1. The DPP lane select is an immediate, so the loops over lanes
// are unrolled by the front end (a `switch` on an unrolled loop's counter is only folded AFTER the unroller has priced the
// body with all sixteen cases in it -- the fused factorisation then exceeds the unroller's budget and stays a loop of jump tables).
template <int I> using ic = std::integral_constant<int, I>;
template <int B, int E, typename F> __device__ __forceinline__ void static_for(F &&f)
{
    if constexpr (B < E) {
        f(ic<B>{});
        static_for<B + 1, E>(f);
    }
}
// sum_k (x_k of lane k of the caller's row) * m[k]: a dot product with a vector spread over the row's lanes, two chains
__device__ __forceinline__ double dot_bcast(double x, const double (&m)[NV], double init)
{
    double a0 = init, a1 = 0.0;
    dpp_ready(x);
    static_for<0, NV / 2>([&](auto kk) {
        constexpr int k = 2 * decltype(kk)::value;
        fmac_bcast<k>(a0, x, m[k]);
        fmac_bcast<k + 1>(a1, x, m[k + 1]);
    });
    return a0 + a1;
}

// 1/x from the hardware estimate plus two Newton steps (operands are never subnormal or zero when the result is used)
__device__ __forceinline__ double fast_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}
// 1/sqrt(x) from the hardware estimate, one Newton step and one third-order step (x is a positive, normal number wherever the
// result is used: a pivot of a positive definite matrix, a squared row norm; the library's rsqrt spends two thirds of its
// instructions on subnormals and infinities)
__device__ __forceinline__ double fast_rsqrt(double x)
{
    double y = __builtin_amdgcn_rsq(x);
    double e = fma(-x * y, y, 1.0);
    y = fma(0.5 * y, e, y);
    e = fma(-x * y, y, 1.0);
    return fma(y * e, fma(0.375, e, 0.5), y);
}
// The wavefronts of a workgroup share nothing and a wavefront's LDS operations complete in order: only the COMPILER has
// to keep the order of an exchange (no s_barrier, no queue drain).
__device__ __forceinline__ void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// LDS carve of ONE problem, in doubles, for ROWS constraint rows per lane (the M image holds 16 ROWS rows). Two of each:
//  ROWS = 2 (up to 32 rows)
//  * ROOMY (launches of one round: at most one wavefront per SIMD, so LDS is free): M image 32 x 18 (row stride 18 = 144 B: rows start
//    in distinct 16-B slots, conflict-free stores), the full L^-T image, a T image for the rare refinement, the leaving slot's row, the
//    slots' constraint ids: 1112 doubles = 35.6 KB per wavefront, four on a CU.
//  * SLIM (launches of several rounds): 640 doubles = 5120 B, 20 KB per wavefront -- EIGHT wavefronts on a CU's 160 KB, two per SIMD
//    (256-register budget), which is what those launches live on: 65,536 config-4 problems 231 us against 324 us roomy and 305 us
//    for the two-per-wavefront kernel (tools/ab_quad_c4.py). Kept in LDS: M (32 x 16: its stores conflict, +2.6 k cycles once)
//    and the strict upper triangle of L^-T, packed (the diagonal stays in a register). Gone: the T image (T' rho by row sums over
//    the lanes), the leaving slot's row (fetched from its lane by ds_bpermute in the rare drop trip), the slots' ids (DPP). On a
//    one-round launch the slim carve costs 3.8 us (its prologue and epilogue are longer): hence both.
//  ROWS = 4 (up to 64 rows), ONE wavefront per SIMD in both (the kernel holds 334 / 373 registers)
//  * ROOMY (up to three wavefronts per CU): M image 64 x 16 (with 18 only two wavefronts fit a CU), otherwise as above: 1560 doubles =
//    12.2 KB per problem, 49.9 KB per wavefront, three on a CU's 160 KB.
//  * SLIM (launches beyond three wavefronts per CU: 3073 problems and more on an MI355X): 1152 doubles, 36.9 KB per wavefront, FOUR on
//    a CU. 4096 problems with m = 64: 119 us roomy (two rounds of three per CU), 81 us slim (one round).
template <bool SLIM, int ROWS = 2> struct Carve {
    static constexpr int MMAX = NV * ROWS;  // constraints a problem can hold
    static constexpr int GS = MMAX + 1;     // the build's G image is stored by COLUMN with an odd stride
    static constexpr int LDM = (SLIM || ROWS == 4) ? 16 : 18;
    static constexpr int OFF_M = 0;  // build: G image by column, 16 x GS (slim: over the start of the region behind it, which is not
                                     // alive yet) | main: M image, MMAX x LDM
    static constexpr int OFF_LT = MMAX * LDM;  // roomy: rows of L^-T, 16 x 16 | slim: strict upper triangle by rows, packed: row l at
                                               // l (31 - l) / 2, 15 - l entries
    static constexpr int NLT = SLIM ? NV * (NV - 1) / 2 + 8 : NV * NV;  // (slim: eight spare doubles keep the G image inside the carve)
    static constexpr int OFF_T = OFF_LT + NLT;                    // roomy only from here on: T by rows (refinement)
    static constexpr int OFF_KA = OFF_T + NV * NV;                // the row of a leaving slot
    static constexpr int OFF_ACT = OFF_KA + NV;                   // 16 int32: constraint held by each slot
    static constexpr int PER = SLIM ? OFF_LT + NLT : OFF_ACT + NV / 2;  // doubles per problem: 640 | 1112 (ROWS = 2), 1152 | 1560 (ROWS = 4)
    static_assert(ROWS == 2 || ROWS == 4, "two or four constraint rows per lane");
    static_assert(NV * GS <= PER, "the G image must fit the problem's carve");
    static_assert(PER % 2 == 0 && (!SLIM || PER * 4 * 8 <= 10 * ROWS * 1024), "16-byte alignment; slim: 20 / 40 KB per wavefront");
};

constexpr double DEP = 1e-14;      // |z|^2 / |M_p|^2 below this: M_p depends on the active rows
constexpr double DEP_FAST = 1e-6;  // K_p . M_p is trusted as |z|^2 only above this (mpcqp_pair.hip); |K_p|^2 otherwise

// a[i] for an index i = 0 .. R-1 that is uniform inside a row (straight-line selects), R = 2 or 4
template <typename X, int R> __device__ __forceinline__ X pick(const X (&a)[R], int i)
{
    if constexpr (R == 2)
        return i == 0 ? a[0] : a[1];
    else
        return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3]));
}

}  // namespace quad

}  // namespace mpcqp
