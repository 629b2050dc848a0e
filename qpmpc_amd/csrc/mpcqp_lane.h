// mpcqp_lane.h -- what the lanes of ONE wavefront do with each other or with the hardware estimate units, each defined once for
// every kernel file: DPP moves and reductions, lane reads, the row broadcast and the hand-written v_fmac_f64_dpp with its hazard
// contract, 16-wide register / LDS helpers, the fast reciprocals, the shuffle reductions and the exchange fences. Device code
// only; the host-side contract between the kernels and the C API is mpcqp_internal.h.
#pragma once

#include <hip/hip_runtime.h>

namespace mpcqp {

constexpr int kRowLanes = 16;  // lanes of a DPP row: the width of every 16-vector below

// ------------------------------------------------------------ DPP moves and lane reads
// x of the lane that CTRL selects, bound_ctrl OFF (v_mov_b32_dpp; a lane without a source keeps 0 -- the row rotations
// below give every lane one).
template <int CTRL> __device__ __forceinline__ int dpp(int x) { return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xf, 0xf, false); }
template <int CTRL> __device__ __forceinline__ unsigned dpp(unsigned x) { return (unsigned)dpp<CTRL>((int)x); }
template <int CTRL> __device__ __forceinline__ float dpp(float x) { return __int_as_float(dpp<CTRL>(__float_as_int(x))); }
template <int CTRL> __device__ __forceinline__ double dpp(double x)
{
    return __hiloint2double(dpp<CTRL>(__double2hiint(x)), dpp<CTRL>(__double2loint(x)));
}
constexpr int ROR8 = 0x128, ROR4 = 0x124, ROR2 = 0x122, ROR1 = 0x121;  // rotate within a row of 16
// ... with bound_ctrl ON: another instruction encoding, hence another name (the all-reductions further down)
template <int CTRL, typename T> __device__ __forceinline__ T dpp_mov(T x)
{
    if constexpr (sizeof(T) == 8) {
        const long long b = __builtin_bit_cast(long long, x);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)b, CTRL, 0xf, 0xf, true);
        const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, true);
        return __builtin_bit_cast(T, ((long long)hi << 32) | (unsigned)lo);
    } else {
        return __builtin_bit_cast(T, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, 0xf, 0xf, true));
    }
}
// x of lane l, in every lane (v_readlane; l must be wavefront-uniform): int, float, double
template <typename T> __device__ __forceinline__ T lane_get(T x, int l)
{
    if constexpr (sizeof(T) == 8) {
        const long long b = __builtin_bit_cast(long long, x);
        const int lo = __builtin_amdgcn_readlane((int)b, l), hi = __builtin_amdgcn_readlane((int)(b >> 32), l);
        return __builtin_bit_cast(T, ((long long)hi << 32) | (unsigned)lo);
    } else {
        return __builtin_bit_cast(T, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), l));
    }
}
// The same value with the double taken apart by __double2loint / __double2hiint instead of the 64-bit cast above. Only the
// stage-wise kernels' own lane reads use it: with the cast their instructions change (the wide kernel's register allocation,
// the sense of sixteen branches in the narrow one), and those kernels stay the instructions they were measured as. (float: one
// word, nothing to take apart -- for the call sites that are generic over the element type.)
__device__ __forceinline__ double lane_get_halves(double x, int l)
{
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float lane_get_halves(float x, int l) { return lane_get(x, l); }

// ------------------------------------------------------------ reductions over a 16-lane row, by rotation
// all-reduce inside each row of 16 by four row rotations (NOT row_sum_dpp below: other partners, another summation order)
template <typename T> __device__ __forceinline__ T row_sum_ror(T v)
{
    v += dpp<ROR8>(v);
    v += dpp<ROR4>(v);
    v += dpp<ROR2>(v);
    v += dpp<ROR1>(v);
    return v;
}
__device__ __forceinline__ unsigned row_min(unsigned v)
{
    v = min(v, dpp<ROR8>(v));
    v = min(v, dpp<ROR4>(v));
    v = min(v, dpp<ROR2>(v));
    v = min(v, dpp<ROR1>(v));
    return v;
}
// One step of row_min, hand-written (N = 8, 4, 2, 1 in this order make the reduction): for a caller that places the steps between its
// own hand-written instructions, where the compiler would pad each of its own DPP steps (it counts no wait states for inline asm).
// HAZARD CONTRACT as fmac_bcast's: v is the DPP operand, written by a VALU instruction at least two wait states earlier.
template <int N> __device__ __forceinline__ void min_ror(unsigned &v)
{
    asm volatile("v_min_u32_dpp %0, %0, %0 row_ror:%1 row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(v) : "n"(N));
}
// order-preserving map of a floating-point value onto unsigned words (the key of the arg-mins built on row_min)
__device__ __forceinline__ void ordered(double x, unsigned &hi, unsigned &lo)
{
    const unsigned h = (unsigned)__double2hiint(x), l = (unsigned)__double2loint(x);
    const bool neg = h & 0x80000000u;
    hi = neg ? ~h : (h | 0x80000000u);
    lo = neg ? ~l : l;
}
__device__ __forceinline__ void ordered(float x, unsigned &hi, unsigned &lo)
{
    const unsigned h = __float_as_uint(x);
    hi = (h & 0x80000000u) ? ~h : (h | 0x80000000u);
    lo = 0;
}

// ------------------------------------------------------------ wavefront all-reductions on the vector pipe
// (the stage-wise kernels; __shfl_xor is a ds_bpermute per dword and step: 18 dependent LDS round trips for one (double, int)
// arg-min). Four DPP steps reduce every 16-lane row in all of its lanes (xor 1, xor 2 inside the quads, row_half_mirror,
// row_mirror: every step pairs each lane with a lane of the other half of its group, and the operations are commutative, so the
// lanes of a row end with the same bits); the four row results meet through v_readlane. Call with all 64 lanes active.
// the sum over each 16-lane row, in every lane of the row
template <typename T> __device__ __forceinline__ T row_sum_dpp(T v)
{
    v += dpp_mov<0xb1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov<0x4e>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);  // row_half_mirror
    v += dpp_mov<0x140>(v);  // row_mirror
    return v;
}
template <typename T> __device__ __forceinline__ T wave_sum_dpp(T v)
{
    v = row_sum_dpp(v);
    return (lane_get(v, 0) + lane_get(v, 16)) + (lane_get(v, 32) + lane_get(v, 48));
}
// (value, index) arg-min; ties -> lowest index (a total order: any reduction tree gives the same pair); every lane gets it
template <typename T> __device__ __forceinline__ void wave_argmin_dpp(T &v, int &idx)
{
    auto merge = [&](T ov, int oi) {
        const bool take = (ov < v) || (ov == v && oi < idx);
        v = take ? ov : v;
        idx = take ? oi : idx;
    };
    merge(dpp_mov<0xb1>(v), dpp_mov<0xb1>(idx));
    merge(dpp_mov<0x4e>(v), dpp_mov<0x4e>(idx));
    merge(dpp_mov<0x141>(v), dpp_mov<0x141>(idx));
    merge(dpp_mov<0x140>(v), dpp_mov<0x140>(idx));
    const T v1 = lane_get(v, 16), v2 = lane_get(v, 32), v3 = lane_get(v, 48);
    const int i1 = lane_get(idx, 16), i2 = lane_get(idx, 32), i3 = lane_get(idx, 48);
    v = lane_get(v, 0);
    idx = lane_get(idx, 0);
    merge(v1, i1);
    merge(v2, i2);
    merge(v3, i3);
}

// ------------------------------------------------------------ ... and the same two over __shfl_xor (ds_bpermute)
// (the kernels with several wavefronts per problem, whose block reductions finish them through LDS)
template <typename T> __device__ __forceinline__ T wave_sum_shfl(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
template <typename T> __device__ __forceinline__ void wave_argmin_shfl(T &v, int &i)  // ties -> lowest index
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const T ov = __shfl_xor(v, off);
        const int oi = __shfl_xor(i, off);
        if (ov < v || (ov == v && oi < i)) {
            v = ov;
            i = oi;
        }
    }
}

// ------------------------------------------------------------ 16-vectors: registers <-> LDS in 16-byte pieces
template <typename T> struct Vec;
template <> struct Vec<double> {
    using type = double2;
    static constexpr int W = 2;
};
template <> struct Vec<float> {
    using type = float4;
    static constexpr int W = 4;
};
template <typename T> __device__ __forceinline__ void ld16(T (&d)[kRowLanes], const T *src)
{
    using V = typename Vec<T>::type;
    const V *p = reinterpret_cast<const V *>(src);
#pragma unroll
    for (int i = 0; i < kRowLanes / Vec<T>::W; ++i) {
        const V t = p[i];
        if constexpr (Vec<T>::W == 2) {
            d[2 * i] = t.x;
            d[2 * i + 1] = t.y;
        } else {
            d[4 * i] = t.x;
            d[4 * i + 1] = t.y;
            d[4 * i + 2] = t.z;
            d[4 * i + 3] = t.w;
        }
    }
}
template <typename T> __device__ __forceinline__ void st16(T *dst, const T (&s)[kRowLanes])
{
    using V = typename Vec<T>::type;
    V *p = reinterpret_cast<V *>(dst);
#pragma unroll
    for (int i = 0; i < kRowLanes / Vec<T>::W; ++i) {
        V t;
        if constexpr (Vec<T>::W == 2) {
            t.x = s[2 * i];
            t.y = s[2 * i + 1];
        } else {
            t.x = s[4 * i];
            t.y = s[4 * i + 1];
            t.z = s[4 * i + 2];
            t.w = s[4 * i + 3];
        }
        p[i] = t;
    }
}
__device__ __forceinline__ double dot16(const double (&a)[kRowLanes], const double (&b)[kRowLanes])
{
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
#pragma unroll
    for (int k = 0; k < kRowLanes; k += 4) {
        acc0 += a[k] * b[k];
        acc1 += a[k + 1] * b[k + 1];
        acc2 += a[k + 2] * b[k + 2];
        acc3 += a[k + 3] * b[k + 3];
    }
    return (acc0 + acc1) + (acc2 + acc3);
}
// Make a value opaque at this point: the compiler can neither sink the computation that produced it below here nor keep its
// operands alive instead (without this the trailing updates of a factorisation are deferred and every exchanged column stays
// live -> hundreds of bytes of scratch).
template <typename T> __device__ __forceinline__ void pin(T &x) { asm volatile("" : "+v"(x)); }

// ------------------------------------------------------------ DPP row broadcast
// The value held by lane N of the caller's 16-lane row, in every lane of that row: a 64-bit DPP move
// (v_mov_b64_dpp row_newbcast:N) -- a register-to-register broadcast on the vector pipe, no LDS round trip.
template <int N> __device__ __forceinline__ double row_bcast(double x) { return __builtin_amdgcn_mov_dpp(x, 0x150 + N, 0xf, 0xf, true); }
// acc += (x of lane N of the caller's row) * m in ONE instruction (v_fmac_f64_dpp); the compiler does not fold the DPP move into
// the FMA by itself.
// HAZARD CONTRACT: a VGPR written by a VALU instruction needs TWO wait states before a DPP instruction reads it as its DPP
// operand (src0, here x). The compiler keeps that for the DPP instructions it emits, but it cannot see inside the asm: the
// caller puts dpp_ready(x) -- an s_nop 1 tied to x, so that x is written before it and read after it -- in front of every
// batch of fmac_bcast on one broadcast source. tools/check_dpp_hazards.py checks it on the assembly of every unit. The scan follows
// branches (the worst predecessor of every basic block, back edges included), holds a VALU write of EXEC to its five wait states in
// front of a DPP instruction too, and tests/test_gpu_dpp_instantiations.py launches every instantiation that carries the instruction.
template <int N> __device__ __forceinline__ void fmac_bcast(double &acc, double x, double m)
{
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(m), "n"(N));
}
__device__ __forceinline__ void dpp_ready(double &x) { asm volatile("s_nop 1" : "+v"(x)); }

// ------------------------------------------------------------ reciprocal
// 1/x from the hardware estimate plus Newton steps, two in float64 and one in float32 (a full IEEE division costs ~3x the
// instructions; the operands are never subnormal or zero when the result is used)
__device__ __forceinline__ double fast_rcp(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    double e = fma(-x, y, 1.0);
    y = fma(y, e, y);
    e = fma(-x, y, 1.0);
    return fma(y, e, y);
}
__device__ __forceinline__ float fast_rcp(float x)
{
    float y = __builtin_amdgcn_rcpf(x);
    const float e = fmaf(-x, y, 1.0f);
    return fmaf(y, e, y);
}
// The same values with the correction e as the FIRST factor of the Newton FMAs, fma(e, y, y): the compiler keeps the source's
// operand order in v_fmac (src0 and src1 exchanged), and the stage-wise kernels stay the instructions they were measured as.
__device__ __forceinline__ double fast_rcp_e_first(double x)
{
    double y = __builtin_amdgcn_rcp(x);
    y = fma(fma(-x, y, 1.0), y, y);
    return fma(fma(-x, y, 1.0), y, y);
}
__device__ __forceinline__ float fast_rcp_e_first(float x)
{
    const float y = __builtin_amdgcn_rcpf(x);
    return fmaf(fmaf(-x, y, 1.0f), y, y);
}

// ------------------------------------------------------------ exchanges between the lanes of one wavefront
// Every one of these orders the accesses of ONE wavefront; none is a workgroup barrier. They differ in what the fence makes
// the hardware wait for, so they differ in name: a line moved between kernel families keeps its meaning or does not compile.
//
// Compiler-only ordering at wavefront scope: no instruction is issued.
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
// Exchange through LDS between the lanes of a wavefront that shares its data with no other wavefront (one wavefront per
// workgroup, or wavefronts of a workgroup that share nothing). LDS operations of a wavefront complete in order, so what one
// lane wrote is what another lane reads next without any wait. Only the COMPILER has to keep the order (wavefront-scope
// fence); __syncthreads() would also drain the LDS queue (s_waitcnt lgkmcnt(0)) at every exchange, six times per active-set
// iteration.
__device__ __forceinline__ void wave_sync()
{
    wave_fence();
    __builtin_amdgcn_wave_barrier();
}
// Exchange through the workspace in GLOBAL memory (the stage-wise kernels): stores of one lane become visible to the other
// lanes of the wavefront (same CU, same L1) -- the workgroup-scope fence waits for the outstanding memory operations, which
// the wavefront-scope one above does not.
__device__ __forceinline__ void wave_sync_workgroup()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}
// Hand-over through LDS inside ONE wavefront without a fence: its LDS operations execute in order, so nothing has to be waited
// for -- only the compiler must not move the accesses across this point.
__device__ __forceinline__ void lsync()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_wave_barrier();
}

}  // namespace mpcqp
