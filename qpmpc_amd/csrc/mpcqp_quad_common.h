// mpcqp_quad_common.h -- what the four-problems-per-wavefront kernels share: the lean / shared-model kernel of mpcqp_quad.hip and the
// general kernel of mpcqp_quadg.hip (two or four constraint rows per lane). Device helpers of a problem that owns ONE 16-lane DPP row
// beyond the lane primitives of mpcqp_lane.h (a lane's value and a predicate inside the row, the two-vector and the broadcast dot
// products, the compile-time loop, the fast reciprocal square root) and the LDS carve of one problem.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "mpcqp_internal.h"
#include "mpcqp_lane.h"

namespace mpcqp {

namespace quad {

constexpr int NV = kRowLanes;  // padded number of variables / slots = lanes per problem

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
