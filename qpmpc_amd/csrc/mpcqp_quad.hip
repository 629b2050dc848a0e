// mpcqp_quad.hip -- gfx950 kernel for SMALL problems (n <= 16 variables, m <= 32 inequality rows, nx <= 16,
// float64, one to four rows per step): FOUR PROBLEMS PER WAVEFRONT, one per 16-lane DPP row.
//
// Replaces the same reference code as mpcqp_pair.hip (qpmpc/mpc_qp.py:53-149 for the build, qpsolvers.solve_problem at
// qpmpc/solve_mpc.py:43 for the solve) for cold fused build+solve launches: BASELINE configs 1, 2 and 4 (nx = 3, nu = 1,
// N = 16 -> n = 16, m = 32; terminal cost only, two state rows per step: the lean build) and, since round 6, every other
// cost / constraint layout of these sizes (input rows, stage cost with per-step targets, mk = 1 .. 4, nx = 2, 5 .. 16: the general
// build, template parameter GEN -- the reference's examples/wheeled_inverted_pendulum.py:90-94 is of that kind). Warm
// starts and seed steps stay on mpcqp_pair.hip, which is also this kernel's cross-check (MPCQP_OPT_TWO_PER_WAVE).
// More than 32 rows: mpcqp_quadg.hip, this kernel's general build as a template over the rows a lane holds; the device helpers and the
// LDS carve both files use are in mpcqp_quad_common.h.
//
// Why four per wavefront (round-4 counters on the pair kernel, profiles/r04_pair_m_rocprof_summary.txt): 8.17 M vector
// instructions per 4096-problem launch of which 4.22 M are float64 arithmetic -- 48 % of vector issue is masks, selects,
// lane moves and reductions that serve TWO problems per instruction, and half of every lane-crossing step exists only
// because a problem straddles two DPP rows (v_permlane16_swap in every reduction, the copy of the factor into the second
// row, the high row's -z copied over the low one). Here a problem owns ONE 16-lane row and each lane owns FOUR 16-register
// rows, so the same overhead stream serves four problems and every lane-crossing step is a row-only DPP operation:
//   lane l of a row (l = 0..15):
//     RT  row l of T = N* (active-set slot l, its multiplier, its constraint id)
//     RH  row l of the projector H = I - M_A' T
//     K0  K_l = H M_l (constraint l, slack s0)        K1  K_{l+16} = H M_{l+16} (constraint l + 16, slack s1)
//   build: lane l owns column l of Psi and row l of P -> L; EVERY lane carries the free response Phi_k x0 (there is no
//   17th lane; the 15 extra FMAs per step are issue slots a lone wavefront leaves idle anyway), so h and q need no exchange.
// 1024 wavefronts for the 4096 problems of config 2 -> one wavefront per SIMD; 254 registers and 20 KB of LDS each, so that launches
// of several rounds keep two on every SIMD.
//
// Solver: the dual active-set method (Goldfarb-Idnani 1983) in the explicit-operator form of mpcqp_pair.hip, same pivots,
// same tolerances; see that file for the derivation. What differs:
//   * Cholesky and forward substitution are ONE right-looking pass: step j scales column j of L and immediately applies it
//     to the trailing columns of P, of the two rows of G, of the identity row (-> L^-T) -- four independent FMA streams on
//     the same DPP broadcasts -- and to q (-> w = L^-1 q, component k in lane k).
//   * Plain trips (nearly all) run in a steady loop of one basic block (mpcqp_quad_steady.h) in front of the general loop, which serves
//     every kind of trip. A trip that is not plain is made ONCE: the steady loop leaves with what it computed of it, the general loop
//     finishes it. A partial step removes its blocking slot in the same trip (the removal is that trip's rank-one update), and the
//     wavefront is back in the steady loop as soon as none of its live rows holds a constraint it still has to add.
//     The update vector (z, or T_l of a leaving slot: component k in lane k) is applied by DPP row broadcasts at the
//     top of the next trip; the rare parts (|K_p|^2 near dependence, ratio test, drop) sit behind wavefront-uniform ballots.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <type_traits>

#include "mpcqp.h"
#include "mpcqp_internal.h"
#include "mpcqp_quad_common.h"

namespace mpcqp {

namespace quad {

constexpr int MMAX = 32;  // constraints a problem can hold (two per lane)
constexpr int MK = 2;     // inequality rows per step
// Placement of the steady loop (profiles/quad_prologue.md, quad_trip_slots.md: its speed follows the header's offset): padding in the probe's
#ifndef QUAD_STEADY_PAD  // tick(4) block of the headline instantiation, which a launch without probe skips. Six: the best of eight
#define QUAD_STEADY_PAD "s_nop 0\ns_nop 0\ns_nop 0\ns_nop 0\ns_nop 0\ns_nop 0"
#endif
#ifndef QUAD_PROBE_REFINE  // 1: slot 14 of the probe also marks a pass through the refinement arm (tools/gen_golden_quad_prologue.py);
#define QUAD_PROBE_REFINE 0  // not in the shipped build: the mark costs the slim instantiations 8 B of scratch
#endif

}  // namespace quad

using namespace quad;

// ORD: the launch carries a pairing order (MpcqpSolveOpts.order): row i of the launch takes problem order[i].
// WPB: wavefronts per workgroup (they share nothing).
// MODEL: the launch shares one factored model (mpcqp_factor_model: gA points at it); the per-problem vectors are x0, goal, targets and,
//        optionally, the bounds e. No build, no factorisation: M, L^-T and the linear maps of h and w are read from the model.
// GEN:   the build serves every cost and constraint layout of one to four rows per step (round 6): input rows D_k next to / instead of
//        the state rows C_k, a stage cost w_x sum |x_k - xref_k|^2 (the Gram matrix accumulated over every Psi_k of the chain, as
//        mpcqp_pair.hip's generic build does) -- the reference's own wheeled-inverted-pendulum example
//        (examples/wheeled_inverted_pendulum.py:90-94: input box, stage + terminal cost) is of this kind.
template <int NX, bool ORD, int WPB, bool SLIM, bool MODEL = false, bool GEN = false>
__global__ void __launch_bounds__(64 * WPB, SLIM ? 2 : 1)
    mpcqp_quad_kernel(const double *__restrict__ gA, const double *__restrict__ gB, const double *__restrict__ gC,
                      const double *__restrict__ ge, const double *__restrict__ gx0, const double *__restrict__ ggoal,
                      const double *__restrict__ gtgt, double *__restrict__ oU, double *__restrict__ olam, int32_t *__restrict__ ostatus,
                      int32_t *__restrict__ oiters, const KernelArgs ka, const int64_t batch)
{
    using T = double;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    {  // every kernel argument the operand addresses need, requested in ONE batch of scalar loads at the top (mpcqp_pair.hip)
        const int64_t b0 = ka.A.batch_stride, b1 = ka.B.batch_stride, b2 = ka.C.batch_stride, b3 = ka.e.batch_stride,
                      b4 = ka.x0.batch_stride, b5 = ka.goal.batch_stride;
        const int64_t s0 = ka.A.step_stride, s1 = ka.B.step_stride, s2 = ka.C.step_stride, s3 = ka.e.step_stride;
        asm volatile("" ::"s"(b0), "s"(b1), "s"(b2), "s"(b3), "s"(b4), "s"(b5), "s"(s0), "s"(s1), "s"(s2), "s"(s3), "s"(ka.N), "s"(ka.nu),
                     "s"(ka.flags), "s"(ka.probe), "s"(gA), "s"(gB), "s"(gC), "s"(ge), "s"(gx0), "s"(ggoal), "s"(ka.n), "s"(ka.m),
                     "s"(batch));
    }
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int rb = lane & 48;  // first lane of this row
    const int l = lane & 15;   // lane inside the row
    int64_t prob = 4 * ((int64_t)blockIdx.x * WPB + wv) + (rb >> 4);
    const bool valid = prob < batch;  // a batch that is no multiple of four leaves rows idle: they repeat the last problem, store nothing
    prob = valid ? prob : batch - 1;
    if constexpr (ORD) {  // (an index outside the batch is clamped: a bad order costs wrong pairings, never an access out of bounds)
        const int64_t o = ka.order[prob];
        prob = o < 0 ? 0 : (o >= batch ? batch - 1 : o);
    }
    using CV = Carve<SLIM>;
    constexpr int LDM = CV::LDM, PER = CV::PER;
    T *sm = (T *)smem_raw + (4 * wv + (rb >> 4)) * PER;
    const int n = ka.n, m = ka.m;
    const int row0 = l, row1 = l + NV;                // the two constraints of this lane
    const bool isc0 = row0 < m, isc1 = row1 < m;
    const T INF = HUGE_VAL;
    constexpr int GS = 33;  // the G image is stored by COLUMN with an odd stride
    T *Gimg = sm + CV::OFF_M, *Ml = sm + CV::OFF_M;
    T *LTp = sm + CV::OFF_LT + (l * (31 - l)) / 2 - (l + 1);  // slim: LTp[k] = entry (l, k) of L^-T, k > l
    T *LTimg = sm + CV::OFF_LT, *Timg = sm + CV::OFF_T;  // roomy (OFF_KA, the row of a leaving slot, is no longer used by this kernel)
    int *actv = reinterpret_cast<int *>(sm + CV::OFF_ACT);

    // optional phase timestamps (developer probe, MpcqpSolveOpts.probe): long long[16] per problem, slots as mpcqp_pair.hip
    long long *stamp = ka.probe ? (long long *)ka.probe + prob * 16 : nullptr;
    auto tick = [&](int slot) {
        if (stamp && l == 0 && valid) {
            stamp[slot] = (long long)__builtin_readcyclecounter();
            if (slot == 0 || slot == 6) stamp[slot ? 13 : 12] = (long long)__builtin_amdgcn_s_memrealtime();
            if (slot == 4 && NX == 3 && !ORD && !SLIM && !MODEL && !GEN) asm volatile(QUAD_STEADY_PAD);
        }
    };
    tick(0);

    T hval0, hval1;
    bool notpd = false;
    T RM0[NV], RM1[NV], RLt[NV];
    T wv_ = T(0);  // w = L^-1 q, component l
    if constexpr (MODEL) {
        // rows of M and of L^-T straight from the model (4 KB, read by every wavefront of the launch: L1/L2), h = e - Hx x0 and
        // w = L^-1 q = Wx x0 - Wg goal - Wt targets from the model's linear maps (mpcqp_pair.hip's model mode, four to a wavefront)
        const T *model = gA;
        const ModelLayout ml = make_model_layout(ka.nx, ka.N, n, m);
        const int nxr = ka.nx, nT = ka.N * ka.nx;
        const T *x0 = gx0 + prob * ka.x0.batch_stride;
        const T *goal = ggoal ? ggoal + prob * ka.goal.batch_stride : nullptr;
        const T *tgt = gtgt ? gtgt + prob * ka.targets.batch_stride : nullptr;
        notpd = model[ml.total] != T(0);
        {
            T r0[NV], r1[NV];
            ld16(r0, model + ml.off_M + (size_t)(isc0 ? row0 : 0) * NV);
            ld16(r1, model + ml.off_M + (size_t)(isc1 ? row1 : 0) * NV);
            ld16(RLt, model + ml.off_LinvT + (size_t)l * NV);
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                RM0[k] = isc0 ? r0[k] : T(0);
                RM1[k] = isc1 ? r1[k] : T(0);
            }
        }
        // the bounds come with the model, or per problem (mpcqp_solve_model_bounds_batch: matrices shared, e moving)
        auto bound = [&](int row, bool isc) {
            if (!isc) return INF;
            const int mkr = ka.mk, kq = mkr == 2 ? row >> 1 : row / mkr;
            T hh = ge ? ge[prob * ka.e.batch_stride + kq * ka.e.step_stride + (row - kq * mkr)] : model[ml.off_e + row];
            for (int c = 0; c < nxr; ++c) hh -= model[ml.off_Hx + (size_t)row * nxr + c] * x0[c];
            return hh;
        };
        hval0 = bound(row0, isc0);
        hval1 = bound(row1, isc1);
        for (int c = 0; c < nxr; ++c) wv_ += model[ml.off_Wx + (size_t)l * nxr + c] * x0[c];
        if ((ka.flags & MPCQP_Q_TERMINAL) && goal)
            for (int c = 0; c < nxr; ++c) wv_ -= model[ml.off_Wg + (size_t)l * nxr + c] * goal[c];
        if ((ka.flags & MPCQP_Q_STAGE) && tgt)
            for (int j2 = 0; j2 < nT; ++j2) wv_ -= model[ml.off_Wt + (size_t)l * nT + j2] * tgt[j2];
        tick(1);
    } else {
    // ---------------------------------------------------------------- build (mpc_qp.py:53-114)
    T Pr[NV];  // row l of P, then of L
    T qa;
    T g15a = T(0), g15b = T(0);
    {
        // WIDE (round 6, NX = 8 / 12 / 16 as padded sizes for nx = 7 .. 16): the operands of a step do not fit registers for the whole
        // horizon -- they are streamed, two steps ahead of the chain, and the chain is a loop over the steps (see below)
        constexpr bool WIDE = GEN && NX > 6;
        const int nx = WIDE ? ka.nx : NX;
        const int nu = ka.nu, N = ka.N;
        // rows per step: two in the lean build; one to four in the general one (a run-time number: the chain's loops over the rows of
        // a step are unrolled four wide behind wavefront-uniform tests)
        constexpr int MKG = GEN ? 4 : MK;
        const int mk = GEN ? ka.mk : MK;
        auto stepof = [&](int row) { return mk == 2 ? row >> 1 : (mk == 1 ? row : (mk == 4 ? row >> 2 : row / 3)); };
        const T *A = gA + prob * ka.A.batch_stride;
        const bool hasC = !GEN || gC != nullptr;
        const T *Cm = hasC ? gC + prob * ka.C.batch_stride : A;  // (no state rows: the lanes load valid addresses, the products are dropped)
        const int sA = ka.A.step_stride ? nx * nx : 0, sB = ka.B.step_stride ? nx * nu : 0, sC = (hasC && ka.C.step_stride) ? mk * nx : 0;
        constexpr int NAe = NX * NX, NEe = NAe + MKG * NX;  // elements of [A_k | C_k]
        const int NEr = hasC ? NAe + mk * NX : NAe;          // ... that exist
        constexpr int NOP = WIDE ? 1 : (NEe + 15) / 16;  // operand registers per step: two up to nx = 4, three / four for nx = 5 / 6
        T op[NOP][NV];
#include "mpcqp_quad_operands.h"  // (a fragment of this body) the sixteen [A_k | C_k] loads, requested in front of everything else
        const T *B = gB + prob * ka.B.batch_stride;
        const T *x0 = gx0 + prob * ka.x0.batch_stride;
        const T *goal = ggoal ? ggoal + prob * ka.goal.batch_stride : nullptr;
        const bool termP = ka.flags & MPCQP_P_TERMINAL, termQ = (ka.flags & MPCQP_Q_TERMINAL) && goal;
        // (GEN) input rows and the stage cost
        const T *Dm = (GEN && ka.D.ptr) ? (const T *)ka.D.ptr + prob * ka.D.batch_stride : nullptr;
        const T *tgt = (GEN && gtgt) ? gtgt + prob * ka.targets.batch_stride : nullptr;
        const int sD = (GEN && ka.D.step_stride) ? mk * nu : 0;
        const bool stageP = GEN && (ka.flags & MPCQP_P_STAGE), stageQ = GEN && (ka.flags & MPCQP_Q_STAGE) && tgt;
        const bool col = (l < n);
        const int j = col ? (nu == 1 ? l : l / nu) : -1, ii = col ? l - j * nu : 0;  // (nu == 1: no division before the loads)
        // every load is issued before the first use: the whole build costs ONE HBM latency. A lane without an element loads a valid
        // address of its problem and drops the value: no load sits behind an exec-mask branch
        const int64_t eb = prob * ka.e.batch_stride;
        const int kq0 = stepof(row0), kq1 = stepof(row1);
        const T elo0 = ge[eb + (isc0 ? kq0 * ka.e.step_stride + (row0 - kq0 * mk) : 0)];
        const T elo1 = ge[eb + (isc1 ? kq1 * ka.e.step_stride + (row1 - kq1 * mk) : 0)];
        const T eval0 = isc0 ? elo0 : INF, eval1 = isc1 ? elo1 : INF;
        // The free response Phi_k x0 rides in LANE 15 of the row: that lane's own column belongs to the horizon's last step (or to
        // no variable at all), so it is zero in every G_k and enters Psi_N only as B's column itself -- its registers are idle for the
        // whole chain. The lane starts from x0 instead of zero, the chain's FMAs propagate it with everyone else's columns, and a row's
        // C_k Phi_k x0 is a row broadcast of what lane 15 computes as "its G entry" (round 5; before: a second chain of 15 FMAs per step
        // in every lane).
        const bool xl15 = (l == NV - 1);
        T v[NX], gref[NX], bcol[NX];
        const T *gsrc = termQ ? goal : x0;  // (every lane of the row loads x0 and the goal from the address lane 15 uses, and selects)
#pragma unroll
        for (int s = 0; s < NX; ++s) {
            const T xs = x0[s < nx ? s : 0], gs = gsrc[s < nx ? s : 0];
            v[s] = (xl15 && s < nx) ? xs : T(0);
            gref[s] = (termQ && s < nx) ? gs : T(0);
        }
        const int jB = col ? j * sB + ii : 0;
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            const T bs = B[jB + (r < nx ? r : 0) * nu];
            bcol[r] = (col && r < nx) ? bs : T(0);
        }
        // (GEN) this lane's column of D_j: the G entries of its variable, rows (j, 0) and (j, 1). Lane 15's cells of the image carry
        // the free response through the chain: when it owns a variable (n = 16: an input of the LAST step) the two rows of that step
        // fetch its entries of D straight from memory, behind the chain. Targets: lane e keeps xref element e, e + 16, e + 32, e + 48
        // (N nx <= 64), the chain fetches them as row broadcasts.
        T dcol[MKG], d15a = T(0), d15b = T(0), tg[NX];  // (targets: N nx <= 16 nx values, one per lane and register)
#pragma unroll
        for (int u = 0; u < NX; ++u) tg[u] = T(0);
#pragma unroll
        for (int i2 = 0; i2 < MKG; ++i2) dcol[i2] = T(0);
        if constexpr (GEN) {
            if (Dm) {
#pragma unroll
                for (int i2 = 0; i2 < MKG; ++i2) dcol[i2] = (col && !xl15 && i2 < mk) ? Dm[j * sD + i2 * nu + ii] : T(0);
                if (n == NV) {
                    const int j15 = nu == 1 ? NV - 1 : (NV - 1) / nu, i15 = NV - 1 - j15 * nu;
                    d15a = (isc0 && kq0 == j15) ? Dm[j15 * sD + (row0 - kq0 * mk) * nu + i15] : T(0);
                    d15b = (isc1 && kq1 == j15) ? Dm[j15 * sD + (row1 - kq1 * mk) * nu + i15] : T(0);
                }
            }
            if (stageQ && !WIDE) {
#pragma unroll
                for (int u = 0; u < NX; ++u) tg[u] = (l + 16 * u < N * NX) ? tgt[l + 16 * u] : T(0);
            }
        }
        if constexpr (!WIDE) {
        tick(8);
        const T wu = (T)ka.wu;
        qa = T(0);
#pragma unroll
        for (int b = 0; b < NV; ++b) Pr[b] = (l == b) ? (col ? wu : T(1)) : T(0);
        tick(9);
        // acc += (element IDX of [A_k | C_k]) * xx
        auto mac = [&](auto idx, auto kc_, T &acc, T xx) {
            constexpr int IDX = decltype(idx)::value, K = decltype(kc_)::value;
            fmac_bcast<IDX % 16>(acc, op[IDX / 16][K], xx);
        };
        // [G_k; Psi_{k+1}] = [C_k; A_k] Psi_k (column l in lane l; lane 15: [C_k Phi_k x0; Phi_{k+1} x0])
        static_for<0, NV>([&](auto kk) {
            constexpr int k = decltype(kk)::value;
            if (k < N) {
                if constexpr (GEN && k >= 1) {
                    // stage cost on x_k: P += w_x Psi_k' Psi_k, q += w_x Psi_k' (Phi_k x0 - xref_k)  (mpc_qp.py:99-105, 129-149; lane 15's
                    // own column is zero in every Psi_k of the chain, its registers hold the free response)
                    if (stageP || stageQ) {
                        const T wxs = (T)ka.wx;
                        static_for<0, NX>([&](auto sc) {
                            constexpr int s2 = decltype(sc)::value;
                            constexpr int te = k * NX + s2;
                            T src = xl15 ? T(0) : v[s2];
                            const T t = wxs * src;
                            if (stageQ) qa += t * (row_bcast<NV - 1>(v[s2]) - row_bcast<te % 16>(tg[te / 16]));
                            if (stageP) {
                                dpp_ready(src);
                                static_for<0, NV>([&](auto bc) { fmac_bcast<decltype(bc)::value>(Pr[decltype(bc)::value], src, t); });
                            }
                        });
                    }
                }
                // A step has mk + NX independent sums of NX products; fmac_bcast is asm volatile, so the source order is the issue order. The
                // loop over the products is the OUTER one and the sums take their turn inside it; each keeps its start value and the order of its
                // terms: the same bits. Lane 15 stores C_k Phi_k x0 into column 15 of the image (zero in G); B_j's column starts lane j's sums.
                const T hk = (j == k && !xl15) ? T(1) : T(0);
                T g[MKG], w[NX];
#pragma unroll
                for (int i2 = 0; i2 < MKG; ++i2) g[i2] = T(0);
#pragma unroll
                for (int r = 0; r < NX; ++r) w[r] = hk * bcol[r];
                if constexpr (!GEN) {
                    static_for<0, NX>([&](auto sc) {
                        constexpr int s2 = decltype(sc)::value;
                        static_for<0, MK>([&](auto i2c) { mac(ic<NAe + decltype(i2c)::value * NX + s2>{}, kk, g[decltype(i2c)::value], v[s2]); });
                        static_for<0, NX>([&](auto rc) { mac(ic<decltype(rc)::value * NX + s2>{}, kk, w[decltype(rc)::value], v[s2]); });
                    });
#pragma unroll
                    for (int i2 = 0; i2 < MK; ++i2) Gimg[l * GS + k * MK + i2] = g[i2];
                } else {
                    // (one to four rows per step, wavefront-uniform tests. nx = 6: the G rows first, as a group: ten sums do not fit 256 registers)
                    auto psi = [&](auto sc) {
                        constexpr int s2 = decltype(sc)::value;
                        static_for<0, NX>([&](auto rc) { mac(ic<decltype(rc)::value * NX + s2>{}, kk, w[decltype(rc)::value], v[s2]); });
                    };
                    auto grows = [&](auto sc) {
                        constexpr int s2 = decltype(sc)::value;
                        if (!hasC) return;
                        mac(ic<NAe + s2>{}, kk, g[0], v[s2]);
                        if (mk > 1) mac(ic<NAe + NX + s2>{}, kk, g[1], v[s2]);
                        if (mk > 2) mac(ic<NAe + 2 * NX + s2>{}, kk, g[2], v[s2]);
                        if (mk > 3) mac(ic<NAe + 3 * NX + s2>{}, kk, g[3], v[s2]);
                    };
                    if constexpr (NX > 5) static_for<0, NX>(grows);
                    else static_for<0, NX>([&](auto sc) { psi(sc); grows(sc); });
                    static_for<0, MKG>([&](auto i2c) {
                        constexpr int i2 = decltype(i2c)::value;
                        if (i2 < mk) {  // (wavefront-uniform)
                            g[i2] += (j == k) ? dcol[i2] : T(0);
                            Gimg[l * GS + k * mk + i2] = g[i2];
                        }
                    });
                    if constexpr (NX > 5) static_for<0, NX>(psi);
                }
#pragma unroll
                for (int r = 0; r < NX; ++r) v[r] = w[r];
            }
        });
        } else {
        tick(8);
        const T wu = (T)ka.wu;
        qa = T(0);
#pragma unroll
        for (int b = 0; b < NV; ++b) Pr[b] = (l == b) ? (col ? wu : T(1)) : T(0);
        tick(9);
        // ---- streamed operands. Element e of a step's [A_k (NX x NX) | C_k (4 x NX) | xref_k (NX)] -- padded to NX, entries beyond nx /
        // mk read as zero -- sits in lane e % 16 of register e / 16; every register holds one kind of element (NX^2 and 4 NX are
        // multiples of 16). Two steps' registers are alive: step k + 2 is requested when step k has been consumed.
        constexpr int NAw = NX * NX, NCw = 4 * NX, NEw = NAw + NCw + NX, NOPW = (NEw + 15) / 16;
        T opw[2][NOPW];
        auto fetch = [&](auto dc, int k) {
            constexpr int d = decltype(dc)::value;
            const int kc = k < N ? k : N - 1;
            static_for<0, NOPW>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                constexpr int e0 = 16 * r;
                const int e = e0 + l;
                T val;
                if constexpr (e0 < NAw) {
                    const int rr = e / NX, ss = e - rr * NX;
                    const bool ok = rr < nx && ss < nx;
                    val = A[kc * sA + (ok ? rr * nx + ss : 0)];
                    val = ok ? val : T(0);
                } else if constexpr (e0 < NAw + NCw) {
                    const int e2 = e - NAw, i2 = e2 / NX, ss = e2 - i2 * NX;
                    const bool ok = hasC && i2 < mk && ss < nx;
                    val = Cm[ok ? kc * sC + i2 * nx + ss : 0];
                    val = ok ? val : T(0);
                } else {
                    const int ss = e - NAw - NCw;
                    const bool ok = stageQ && ss < nx;
                    val = ok ? tgt[kc * nx + ss] : T(0);
                }
                opw[d][r] = val;
            });
        };
        fetch(ic<0>{}, 0);
        fetch(ic<1>{}, 1);
        const T wxs = (T)ka.wx;
        auto cstep = [&](auto dc, int k) {
            constexpr int d = decltype(dc)::value;
            // (the step's operand registers are DPP sources of hand-written instructions: pinned in vector registers two wait states
            // ahead -- an instantiation that runs on more than 256 registers may otherwise fetch one from an accumulation register
            // right in front of its first use)
            static_for<0, NOPW>([&](auto rc) { dpp_ready(opw[d][decltype(rc)::value]); });
            // G rows of step k from Psi_k (lane 15: C_k Phi_k x0)
            static_for<0, 4>([&](auto i2c) {
                constexpr int i2 = decltype(i2c)::value;
                if (i2 < mk) {  // (wavefront-uniform)
                    T acc = T(0);
                    if (hasC) {
                        static_for<0, NX>([&](auto sc) {
                            constexpr int s2 = decltype(sc)::value, E = NAw + i2 * NX + s2;
                            fmac_bcast<E % 16>(acc, opw[d][E / 16], v[s2]);
                        });
                    }
                    acc += (j == k) ? dcol[i2] : T(0);
                    Gimg[l * GS + k * mk + i2] = acc;
                }
            });
            // stage cost on x_k (k >= 1)
            if (k >= 1 && (stageP || stageQ)) {
                static_for<0, NX>([&](auto sc) {
                    constexpr int s2 = decltype(sc)::value, E = NAw + NCw + s2;
                    T src = xl15 ? T(0) : v[s2];
                    const T t = wxs * src;
                    if (stageQ) qa += t * (row_bcast<NV - 1>(v[s2]) - row_bcast<E % 16>(opw[d][E / 16]));
                    if (stageP) {
                        dpp_ready(src);
                        static_for<0, NV>([&](auto bc) { fmac_bcast<decltype(bc)::value>(Pr[decltype(bc)::value], src, t); });
                    }
                });
            }
            // Psi_{k+1} = A_k Psi_k, B_k's column entering at step j
            const T hk = (j == k && !xl15) ? T(1) : T(0);
            T w[NX];
            static_for<0, NX>([&](auto rc) {
                constexpr int r = decltype(rc)::value;
                T acc = hk * bcol[r];
                static_for<0, NX>([&](auto sc) {
                    constexpr int s2 = decltype(sc)::value, E = r * NX + s2;
                    fmac_bcast<E % 16>(acc, opw[d][E / 16], v[s2]);
                });
                w[r] = acc;
            });
#pragma unroll
            for (int r = 0; r < NX; ++r) v[r] = w[r];
            fetch(dc, k + 2);
        };
        for (int k = 0; k < N; k += 2) {
            cstep(ic<0>{}, k);
            if (k + 1 < N) cstep(ic<1>{}, k + 1);
        }
        }
        tick(10);
        // P = wu I + wt psi_N' psi_N ; q = wt psi_N' (Phi_N x0 - goal)   (mpc_qp.py:99-105, 129-149)
        const T wt = (T)ka.wt;
        // Phi_N x0 from lane 15, whose own column of Psi_N is B's column of the last step (or nothing)
        T x[NX];
#pragma unroll
        for (int s = 0; s < NX; ++s) {
            x[s] = row_bcast<NV - 1>(v[s]);
            v[s] = xl15 ? bcol[s] : v[s];
        }
#pragma unroll
        for (int s = 0; s < NX; ++s) {
            const T t = wt * v[s];
            if (termQ) qa += t * (x[s] - gref[s]);
            if (termP) {
                T src = v[s];
                dpp_ready(src);
                static_for<0, NV>([&](auto bc) { fmac_bcast<decltype(bc)::value>(Pr[decltype(bc)::value], src, t); });
            }
        }
        qa = col ? qa : T(0);
        tick(11);
        wave_sync();  // the G image is complete
        hval0 = isc0 ? eval0 - Gimg[(NV - 1) * GS + row0] : INF;  // h_i = e_i - C_k Phi_k x0 (column 15 of the image)
        hval1 = isc1 ? eval1 - Gimg[(NV - 1) * GS + row1] : INF;
        if constexpr (GEN) {  // (column 15 of G: the last step's input rows)
            g15a = d15a;
            g15b = d15b;
        }
    }
    tick(1);
    // ------------------------------------------------------------ factorise + forward substitution, one pass
    // Right-looking Cholesky; step j scales column j of L and applies it at once to everything that waits for it:
    //   P[:, k] -= L[:, j] L[k][j]                       (trailing columns of P)
    //   x[k]    -= (x[j] / L_jj) L[k][j], x[j] /= L_jj   for the rows x = G_l, G_{l+16}, e_l: -> M_l, M_{l+16}, (L^-T)_l
    //   q_k     -= L[k][j] w_j, w_j = q_j / L_jj         (q_k in lane k: L[k][j] is local, w_j the broadcast)
    // L[k][j] of lane k is a DPP row broadcast; the four FMA streams are independent of each other.
    {
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            // (column 15 of G is zero: the column of the horizon's last step, or of no variable -- its cells hold the free response)
            RM0[k] = (isc0 && k < NV - 1) ? Gimg[k * GS + row0] : (GEN && k == NV - 1 ? g15a : T(0));
            RM1[k] = (isc1 && k < NV - 1) ? Gimg[k * GS + row1] : (GEN && k == NV - 1 ? g15b : T(0));
            RLt[k] = (l == k) ? T(1) : T(0);
        }
        static_for<0, NV>([&](auto jc) {
            constexpr int j = decltype(jc)::value;
            const T pij = Pr[j];                 // P[l][j] of this lane's row, before scaling
            const T piv = row_bcast<j>(pij);     // P[j][j]
            if (!(piv > T(0))) notpd = true;
            const T rinv = fast_rsqrt(piv);
            const T nt2 = -(pij * rinv * rinv);  // -P[l][j] / piv
            T nl = -(pij * rinv);                // -L[l][j] (column j of L is never read after this step: not kept)
            RM0[j] *= rinv;
            RM1[j] *= rinv;
            RLt[j] *= rinv;
            const T wj = qa * rinv;              // lane j: w_j
            wv_ = (l == j) ? wj : wv_;
            {
                T src = pij, wsrc = wj;
                asm volatile("s_nop 1" : "+v"(src), "+v"(nl), "+v"(wsrc) : "v"(RM0[j]), "v"(RM1[j]), "v"(RLt[j]));  // (the DPP wait states)
                fmac_bcast<j>(qa, wsrc, nl);  // q_k -= L[k][j] w_j (lanes k <= j hold values nobody reads again)
                static_for<j + 1, NV>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    fmac_bcast<k>(Pr[k], src, nt2);     // P[k][j] from lane k
                    fmac_bcast<k>(RM0[k], nl, RM0[j]);  // -L[k][j] from lane k
                    fmac_bcast<k>(RM1[k], nl, RM1[j]);
                    fmac_bcast<k>(RLt[k], nl, RLt[j]);
                });
            }
        });
        wave_sync();  // the M image below reuses the G image
    }
    }  // (!MODEL)
    tick(2);
    tick(3);
    int status = MPCQP_MAX_ITER, iters = 0;
    T xsol = T(0);
    bool done = notpd;      // this row has left the active-set loop
    bool finished = notpd;  // ... and needs no refinement any more (failed, or accepted)
    if (notpd) status = MPCQP_NOT_PD;

    if (isc0) st16(Ml + row0 * LDM, RM0);  // image of M: row-p broadcasts, the active rows in the refinement
    if (isc1) st16(Ml + row1 * LDM, RM1);
    // the rows of L^-T leave the registers. Slim: L^-T is upper triangular (the identity pushed through a forward substitution with a
    // lower triangular factor): the strict upper part packed in LDS, the diagonal in a register
    T ltd = T(0);
    if constexpr (SLIM) {
        static_for<0, NV>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            ltd = (l == k) ? RLt[k] : ltd;
            if (k > l) LTp[k] = RLt[k];
        });
    } else {
        st16(LTimg + l * NV, RLt);
    }
    const T y0 = -wv_;          // y0 = -L^-1 q, component l
    T s0, s1, invn0, invn1;
    {
        // (computed by EVERY lane: a DPP read from a lane that a branch has switched off returns zero)
        const T d0 = dot_bcast(wv_, RM0, hval0), d1 = dot_bcast(wv_, RM1, hval1);  // h - M y0 = h + M w
        s0 = isc0 ? d0 : INF;
        s1 = isc1 ? d1 : INF;
        const T nn0 = dot16(RM0, RM0), nn1 = dot16(RM1, RM1);
        invn0 = (nn0 > T(0)) ? fast_rsqrt(nn0) : T(1);
        invn1 = (nn1 > T(0)) ? fast_rsqrt(nn1) : T(1);
    }
    // Selection rule (the classic Goldfarb-Idnani one): among the rows violated beyond the tolerance, the one FARTHEST
    // from its hyperplane in the P^-1 metric, s_i / |M_i|.
    const bool sel0 = isc0 && (hval0 < T(1e29)), sel1 = isc1 && (hval1 < T(1e29));
    const T tol = (T)ka.tol;
    const T tolh0 = tol + tol * fabs(hval0), tolh1 = tol + tol * fabs(hval1);  // row i is violated when s_i < -tol (1 + |h_i|)
    const int max_iter = ka.max_iter;
    T RT[NV], RH[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        RT[k] = T(0);                      // T = N* starts empty
        RH[k] = (l == k) ? T(1) : T(0);    // H = I
    }
    T lam = T(0);      // multiplier of slot l
    int myact = 0;     // constraint held by slot l
    bool occ = false;  // slot l occupied
    bool e0 = sel0, e1 = sel1;  // this lane's constraints may be selected: they have a bound and are not active (the slack of an
                                // active row is never read: it stays whatever the steps make of it, zero up to rounding)
    // row-uniform state
    int nq = 0, p = 0;
    unsigned mask = 0;  // occupied slots
    bool needp = true;
    T up = T(0);
    int fails = 0;
    // ---- selection, for the rows that start a new constraint (straight-line selects: no divergent branches), and the
    //      fetch of row p of M (a broadcast read inside the row). Called between the two halves of the (deferred) rank-one
    //      update: the update's first FMAs cover the reduction's dependent chain, its last ones the LDS round trip.
    T mp[NV];
    auto select = [&]() {
        // a violated row's scaled slack is negative: the order of the magnitudes is the order of the high words, so
        // the most violated row has the smallest complement
        const bool want = needp & !done;
        const unsigned h0 = ~(unsigned)__double2hiint(s0 * invn0), h1 = ~(unsigned)__double2hiint(s1 * invn1);
        const bool v0 = want & e0 & (s0 < -tolh0), v1 = want & e1 & (s1 < -tolh1);
        const unsigned k0 = v0 ? ((h0 & ~31u) | (unsigned)row0) : 0xffffffffu;
        const unsigned k1 = v1 ? ((h1 & ~31u) | (unsigned)row1) : 0xffffffffu;
        const unsigned mkey = row_min(min(k0, k1));
        const bool none = want & (mkey == 0xffffffffu);
        const bool got = want & !none;
        done = done | none;
        status = none ? (int)MPCQP_SOLVED : status;
        p = got ? (int)(mkey & 31u) : p;
        up = got ? T(0) : up;
        needp = needp & !got;
    };
    // R += c v for the two maintained register rows, v spread over the row (component k in lane k), columns B .. E-1
    auto update = [&](auto bc, auto ec, T zn, T cT, T cH) {
        static_for<decltype(bc)::value, decltype(ec)::value>([&](auto kc) {
            constexpr int k = decltype(kc)::value;
            fmac_bcast<k>(RT[k], zn, cT);
            fmac_bcast<k>(RH[k], zn, cH);
        });
    };
#ifndef QUAD_USPLIT
#define QUAD_USPLIT 8
#endif
    constexpr int USPLIT = QUAD_USPLIT;  // columns of the update issued before the selection's row fetch
    // pending rank-one update R += c v, applied at the top of the next trip -- the ONE site that writes the register rows,
    // selects and fetches
    T zn = T(0), cT = T(0), cH = T(0);
    T hd, kd0, kd1, inv, t2, rd;  // the general loop's trip in flight (-z_l, -M_i . z, 1/|z|^2, t2, r_a): handed over by the steady loop
    wave_sync();
    tick(4);
    for (;;) {
#include "mpcqp_quad_steady.h"  // (a fragment of this body) the steady loop: plain trips in one basic block; defines `general`
        // (the two loops alternate inside one pass of this outer loop: `resume` sends the wavefront back to the steady loop's entry;
        // the refinement and the acceptance test below are reached only when every row is done)
        bool resume = false;
        if (general) for (;;) {  // ===== general loop: every kind of trip. Entered, and re-entered from its own tail, with a trip that is
            //                         updated, selected and measured: hd = -z_l, kd = -M_i . z, inv = 1/|z|^2, t2, rd = r_a
            const bool st = !done;     // this row steps
            const bool phi = p >= NV;  // (row-uniform)
            const int pl = p & 15;
            if (__ballot(st & !(inv > T(0))) != 0ull) {  // rare: |z|^2 as a sum of squares, robust near dependence
                T z2 = hd * hd;
                z2 += dpp_mov<ROR8>(z2);
                z2 += dpp_mov<ROR4>(z2);
                z2 += dpp_mov<ROR2>(z2);
                z2 += dpp_mov<ROR1>(z2);
                z2 = row_bcast<0>(z2);  // (the rotations sum in another order in every lane)
                const T sq = row_get(phi ? s1 : s0, rb, pl), iq = row_get(phi ? invn1 : invn0, rb, pl);
                const bool ok2 = (z2 * iq * iq > T(DEP)) & (z2 > T(0));
                const T iv2 = fast_rcp(z2);
                const bool nearp = !(inv > T(0));
                t2 = nearp ? -sq * iv2 : t2;
                inv = nearp ? (ok2 ? iv2 : T(0)) : inv;
            }
            const bool can_move = (nq < n) & (inv > T(0));
            inv = (can_move & st) ? inv : T(0);
            t2 = can_move ? t2 : INF;
            const int sl = (int)__builtin_ctz(~mask);  // lowest free slot
            const T r = (occ & st) ? rd : T(0);
            // a blocking multiplier exists iff lam_a / r_a < t2 for some slot
            const bool blk = (r > T(0)) & (lam < t2 * r);
            if (__ballot(st & (!can_move | (iters >= max_iter) | blk)) == 0ull) {
                // ---- PLAIN TRIP: every row still in the loop takes a full step. Coefficients of the (deferred) update with
                //      -z: slot sl takes -z/d2, the occupied slots r_a/d2, H row l -z_l/d2
                const T tt = st ? t2 : T(0);
                const bool isnew = st & (l == sl), isp = st & (l == pl);
                iters += st ? 1 : 0;
                zn = hd;
                cT = (l == sl) ? inv : -(r * inv);
                cH = -(hd * inv);
                s0 = fma(tt, kd0, s0);  // s_i -= t M_i . z
                s1 = fma(tt, kd1, s1);
                T ln = fma(-tt, r, lam);
                ln = (occ & (ln < T(0))) ? T(0) : ln;
                lam = isnew ? up + tt : ln;
                myact = isnew ? p : myact;
                occ = occ | isnew;
                e0 = e0 & !(isp & !phi);
                e1 = e1 & !(isp & phi);
                mask |= st ? (1u << sl) : 0u;
                nq += st ? 1 : 0;
                needp = needp | st;
            } else {
                // ---- GENERAL TRIP: limits, partial steps, drops
                bool stepping = st;
                {
                    const bool lim = stepping & (iters >= max_iter);
                    done = done | lim;
                    finished = finished | lim;
                    status = lim ? (int)MPCQP_MAX_ITER : status;
                    stepping = stepping & !lim;
                }
                iters += stepping ? 1 : 0;
                const bool cand = occ & stepping & (r > T(0));
                T t1 = INF;
                int lq = 0;
                const unsigned long long bl = __ballot(stepping & blk);
                if (bl != 0ull) {  // ratio test on the multipliers
                    const T ratio = cand ? lam * fast_rcp(r) : INF;
                    unsigned hi, lo;
                    ordered(ratio, hi, lo);
                    hi = cand ? hi : 0xffffffffu;
                    const unsigned mhi = row_min(hi);
                    const unsigned k2 = (cand && hi == mhi) ? ((lo & ~31u) | (unsigned)l) : 0xffffffffu;
                    const unsigned ml = row_min(k2);
                    lq = (int)(ml & 15u);
                    const T tl1 = row_get(ratio, rb, lq);
                    // (only for the rows that are blocked: a row's result must not depend on what its wavefront's other rows need)
                    const bool blocked = ((unsigned)(bl >> rb) & 0xffffu) != 0u;
                    t1 = (blocked && mhi != 0xffffffffu) ? tl1 : INF;
                }
                T t = t1 < t2 ? t1 : t2;
                {
                    const bool inf = stepping & !(t < INF);  // no step possible: the constraints are inconsistent
                    done = done | inf;
                    finished = finished | inf;
                    status = inf ? (int)MPCQP_INFEASIBLE : status;
                    stepping = stepping & !inf;
                }
                t = stepping ? t : T(0);
                const bool full = stepping & (t2 <= t1);
                zn = hd;
                cT = full ? ((l == sl) ? inv : -(r * inv)) : T(0);
                cH = full ? -(hd * inv) : T(0);
                // ---- bookkeeping: the implied primal point moved by t z: s_i -= t M_i . z
                if (stepping) {
                    s0 = fma(t, kd0, s0);
                    s1 = fma(t, kd1, s1);
                    lam -= t * r;
                    lam = (occ && lam < T(0)) ? T(0) : lam;
                    up += t;
                }
                if (full) {  // p takes slot sl
                    if (l == sl) {
                        lam = up;
                        myact = p;
                        occ = true;
                    }
                    if (l == pl) {
                        e0 = e0 & phi;
                        e1 = e1 & !phi;
                    }
                    mask |= 1u << sl;
                    ++nq;
                    needp = true;
                }
                const bool partial = stepping & !full;
                if (__ballot(partial) != 0ull) {
                    // partial step: slot lq leaves in this very trip. Its row T_l sits in lane lq and is current -- a row that takes a
                    // partial step has no update pending, and none of its own: the slot's removal IS this trip's update. With W = T T'
                    // implicit, T_a -= (T_a . T_l / T_l . T_l) T_l (row l becomes exactly zero); the null space of the active rows
                    // gains the direction T_l: H += T_l T_l' / T_l . T_l. The row keeps its p and steps again in the next trip.
                    const int cl = row_get(myact, rb, lq);
                    // T_a . T_l as dot16 sums it (four chains, column k in chain k % 4), four columns of T_l at a time, each fetched from
                    // lane lq: the row is never held as a whole -- 32 registers this loop does not have (nor an image of it in LDS: the
                    // masked stores of lane lq cost the roomy instantiations their budget of 256 registers)
                    T vl = T(0), ac[4] = {T(0), T(0), T(0), T(0)};
                    static_for<0, NV / 4>([&](auto cc) {
                        constexpr int k = 4 * decltype(cc)::value;
                        T v[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            v[j] = row_get(RT[k + j], rb, lq);
                            vl = (l == k + j) ? v[j] : vl;
                        }
#pragma unroll
                        for (int j = 0; j < 4; ++j) ac[j] = fma(RT[k + j], v[j], ac[j]);
                        pin(ac[3]);
                    });
                    const T tl = (ac[0] + ac[1]) + (ac[2] + ac[3]);
                    const T tld = row_get(tl, rb, lq);
                    const T itl = fast_rcp(tld);
                    if (partial && l == (cl & 15)) {  // the row that leaves may be selected again
                        e0 = (cl < NV) ? sel0 : e0;
                        e1 = (cl < NV) ? e1 : sel1;
                    }
                    zn = partial ? vl : zn;
                    cT = partial ? ((l == lq) ? T(-1) : (occ ? -tl * itl : T(0))) : cT;
                    cH = partial ? vl * itl : cH;
                    lam = (partial & (l == lq)) ? T(0) : lam;
                    occ = occ & !(partial & (l == lq));
                    mask &= partial ? ~(1u << lq) : ~0u;
                    nq -= partial ? 1 : 0;
                }
            }
            // ---- back to the steady loop when no live row holds a p (its entry state; its first update applies zn, cT, cH) -- also
            //      when every row is done: it ends at once and skips this loop
            if (__ballot(!done & !needp) == 0ull) {
                resume = true;
                break;
            }
            // ---- the next trip. The rank-one update  T_a += (r_a/d2) z, T_new = -z/d2 ; H -= z z'/d2  (or the same with a leaving
            //      slot's T_l), wrapped around the selection and row fetch, which only read the slacks
            dpp_ready(zn);
            update(ic<0>{}, ic<USPLIT>{}, zn, cT, cH);
            select();
            ld16(mp, Ml + p * LDM);
            update(ic<USPLIT>{}, ic<NV>{}, zn, cT, cH);
            cT = cH = T(0);
            // ---- r_a = T_a . M_p ; -z_l = H_l . M_p ; then -M_i . z = sum_k M_i[k] (-z_k) for this lane's two rows, with -z
            //      spread over the row: the projected rows K_i = H M_i of mpcqp_pair.hip are NOT maintained (32 FMAs of update
            //      and 32 of dot products per trip against the 32 of these two)
            hd = dot16(RH, mp);
            kd0 = dot_bcast(hd, RM0, T(0)), kd1 = dot_bcast(hd, RM1, T(0));
            // ---- step length, by lane p from its own row: |z|^2 = -M_p . z (trusted well away from dependence, DEP_FAST),
            //      1/|z|^2, t2 = -s_p/|z|^2; the two results go to the row (inv = -1: too close to dependence)
            {
                const bool hi = p >= NV;
                const T kp = hi ? kd1 : kd0, sq = hi ? s1 : s0, iq = hi ? invn1 : invn0;
                const bool okf = kp * iq * iq > T(DEP_FAST);
                const T iv = fast_rcp(kp);
                inv = row_get(okf ? iv : T(-1), rb, p & 15);
                t2 = row_get(-sq * iv, rb, p & 15);
            }
            rd = dot16(RT, mp);  // (while the exchange is in flight)
            pin(rd);
        }
        if (resume) continue;
        tick(5);
        if (__ballot(!finished) == 0ull) break;
        // ================================== multipliers by refinement, slacks re-evaluated
        // (rows that are already finished compute along and change nothing)
        int aa[NV];  // constraint held by each slot (an empty one: row 0 with a zero coefficient)
        if constexpr (SLIM) {
            const int mine = occ ? myact : 0;
            static_for<0, NV>([&](auto ac) { aa[decltype(ac)::value] = __builtin_amdgcn_update_dpp(0, mine, 0x150 + decltype(ac)::value, 0xf, 0xf, false); });
        } else {
            actv[l] = occ ? myact : 0;
            wave_sync();
            const int4 *ap = reinterpret_cast<const int4 *>(actv);
#pragma unroll
            for (int q = 0; q < NV / 4; ++q) {
                const int4 t4 = ap[q];
                aa[4 * q] = t4.x;
                aa[4 * q + 1] = t4.y;
                aa[4 * q + 2] = t4.z;
                aa[4 * q + 3] = t4.w;
            }
        }
        // (M_A' cf)_l, cf_a in lane a (an empty slot carries a zero coefficient)
        auto ma_dot = [&](T cf) {
            T ma[NV];
#pragma unroll
            for (int a = 0; a < NV; ++a) ma[a] = Ml[aa[a] * LDM + l];
            return dot_bcast(cf, ma, T(0));
        };
        // slacks of this lane's two rows at the point y (component k in lane k)
        T fresh0, fresh1;
        auto slacks = [&](T yv) {
            const T f0 = dot_bcast(yv, RM0, T(0)), f1 = dot_bcast(yv, RM1, T(0));
            fresh0 = isc0 ? hval0 - f0 : INF;
            fresh1 = isc1 ? hval1 - f1 : INF;
        };
        // value of this slot's own constraint row (x0 of rows 0..15, x1 of rows 16..31)
        auto of_act = [&](T x0v, T x1v) {
            const T a = row_get(x0v, rb, myact & 15), b = row_get(x1v, rb, myact & 15);
            return (myact < NV) ? a : b;
        };
        T y = y0 - ma_dot(occ ? lam : T(0));  // y = y0 - M_A' lam
        slacks(y);
        // active residuals rho_a = h_a - M_a y should vanish. When they already do to REFTOL (1 + |h_a|) in every row --
        // the usual case: a dozen rank-one updates of T in float64 -- the refinement step below would move y by less than
        // that and is skipped.
        T rho = of_act(fresh0, fresh1);  // (fetched by EVERY lane: an exchange only sees the lanes that take part in it)
        rho = occ ? rho : T(0);
        constexpr double REFTOL = 1e-11;
        const T hact = of_act(hval0, hval1);
        const bool needref = occ & !finished & !(fabs(rho) <= T(REFTOL) * (T(1) + fabs(hact)));
        const unsigned long long nr = __ballot(needref);
        if (nr != 0ull) {
            rho = (((unsigned)(nr >> rb) & 0xffffu) != 0u) ? rho : T(0);  // (rows that need none take a zero step: see the ratio test)
            // dlam = -W rho_A = -T (T' rho_A). (T' rho)_k = sum_a T_a[k] rho_a: lane a holds row a of T, so the sum runs over the
            // lanes -- slim: sixteen row reductions, lane k keeps the k-th (a rare path); roomy: through an image of T in LDS
            T uk = T(0);
            if constexpr (SLIM) {
                static_for<0, NV>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    T v = RT[k] * rho;
                    v += dpp_mov<ROR8>(v);
                    v += dpp_mov<ROR4>(v);
                    v += dpp_mov<ROR2>(v);
                    v += dpp_mov<ROR1>(v);
                    uk = (l == k) ? v : uk;
                });
            } else {
                st16(Timg + l * NV, RT);
                wave_sync();
                T tc[NV];
#pragma unroll
                for (int a = 0; a < NV; ++a) tc[a] = Timg[a * NV + l];
                uk = dot_bcast(rho, tc, T(0));  // (T' rho)_l
            }
            T dl = -dot_bcast(uk, RT, T(0));
            dl = occ ? dl : T(0);
            if (!finished) {
                const T lraw = lam + dl;
                lam = (occ && lraw < T(0)) ? T(0) : lraw;
            }
            // with dl as it is (not clamped) y moves exactly onto the active hyperplanes: y - M_A' dl = y + M_A' T (T' rho)
            // = y + T' rho, because T' rho lies in the range of M_A' where M_A' T = I - H is the identity
            y += uk;
            wave_sync();
            slacks(y);
        }
        // ---- acceptance: no inactive row violated, every active row on its bound, lam >= 0 -- with stationarity by
        //      construction these are the KKT conditions of the strictly convex QP
        bool dirty = row_any((e0 && !(fresh0 >= -T(4) * tolh0)) || (e1 && !(fresh1 >= -T(4) * tolh1)), rb);
        {
            const T ra = of_act(fresh0, fresh1);
            const T ta = of_act(tolh0, tolh1);
            const bool off = row_any(occ && !(fabs(ra) <= T(1e3) * ta), rb);
            const bool neg = row_any(occ && !(lam >= T(0)), rb);
            if (stamp && l == 0 && valid && !finished && done) {  // developer probe: why the last acceptance test failed
                stamp[14] = (long long)(dirty ? 1 : 0) | (off ? 2 : 0) | (neg ? 4 : 0) | ((long long)fails << 8) | ((long long)nq << 16);
                if (QUAD_PROBE_REFINE && ((unsigned)(nr >> rb) & 0xffffu) != 0u) stamp[14] |= 1ll << 24;  // (this pass refined)
            }
            dirty = dirty || off || neg;
        }
        // u = L^-T y (component l). Slim: the diagonal from its register, the strict upper triangle from its packed image
        auto primal = [&]() {
            T lt[NV];
            if constexpr (SLIM) {
                static_for<0, NV>([&](auto kc) {
                    constexpr int k = decltype(kc)::value;
                    lt[k] = (k > l) ? LTp[k > l ? k : l + 1] : ((k == l) ? ltd : T(0));
                });
            } else {
                ld16(lt, LTimg + l * NV);
            }
            return dot_bcast(y, lt, T(0));
        };
        if (!finished && done) {
            if (!dirty) {
                xsol = primal();
                status = MPCQP_SOLVED;
                finished = true;
            } else if (++fails < 4) {
                // continue the active-set loop from the re-evaluated slacks
                s0 = fresh0;
                s1 = fresh1;
                status = MPCQP_MAX_ITER;
                done = false;
                needp = true;
            } else {
                xsol = primal();
                status = MPCQP_MAX_ITER;
                finished = true;
            }
        }
        wave_sync();
        if (__ballot(!finished) == 0ull) break;
    }
    tick(6);
    const bool ok = (status == MPCQP_SOLVED);
    T lo0 = T(0), lo1 = T(0);
    if (olam) {  // multipliers by constraint: every occupied slot drops its multiplier at its row's place
        T *lamv = Ml;  // (the M image is dead: every row has finished; 32 doubles)
        lamv[row0] = T(0);
        lamv[row1] = T(0);
        wave_sync();
        if (occ) lamv[myact] = lam;
        wave_sync();
        lo0 = ok ? lamv[row0] : T(0);
        lo1 = ok ? lamv[row1] : T(0);
    }
    if (valid) {
        if (l < n) oU[prob * (int64_t)n + l] = ok ? xsol : T(0);
        if (olam) {
            if (isc0) olam[prob * (int64_t)m + row0] = lo0;
            if (isc1) olam[prob * (int64_t)m + row1] = lo1;
        }
        if (l == 0) {
            if (ostatus) ostatus[prob] = status;
            if (oiters) oiters[prob] = iters;
        }
    }
}

// ------------------------------------------------------------ host side
// true when four problems per wavefront beat two (tools/ab_quad.py, tools/ab_quad_c4.py on an MI355X, 1024 SIMDs): from MORE THAN TWO
// problems per SIMD up -- up to there a lone two-problem wavefront per SIMD is shorter (2048 problems: 18.2 against 19.3 us), one
// problem more and some SIMD runs two of them (2304: 23.5 against 19.1 us; the rule read 2.25 per SIMD until that was measured). One
// round (up to four problems per SIMD) runs the roomy carve: config 2 at 4096: 22.4 against 24.8 us; anything larger the slim one,
// two wavefronts per SIMD: config 2 at 8192 / 16,384: 37.8 / 65.0 against 47.3 / 85.6 us; config 4 at 8192 / 16,384 / 65,536:
// 45.5 / 74.0 / 231 against 56.9 / 90.9 / 305 us.
[[maybe_unused]] static bool quad_pays(int64_t batch, SimdCount &simds) { return batch > 2 * (int64_t)simds.get(); }

// the lean build (terminal cost only, state rows only: BASELINE configs 1, 2, 4) or the general one (GEN: input rows, stage cost)
static bool quad_general(const KernelArgs &ka)
{
    return ka.nx > 4 || ka.mk != MK || !ka.C.ptr || ka.D.ptr || (ka.flags & (MPCQP_P_STAGE | MPCQP_Q_STAGE));
}

// (this file is compiled twice: as itself -- nx = 2 .. 4 and the shared-model mode -- and, with MPCQP_QUAD_WIDE_UNIT defined, through
// mpcqp_quadw.hip -- the general build's instantiations for nx = 5 .. 16 --: two units of two minutes instead of one of four)
#ifndef MPCQP_QUAD_WIDE_UNIT
bool quad_applies(const KernelArgs &ka)
{
    // the register-pipelined chain: one to four rows per step (state rows, input rows or both), nx = 2 .. 16 (from nx = 7 with the
    // operands streamed per step); cold launches
    if (ka.n > NV || ka.m > MMAX || ka.m < 1 || ka.nx < 2 || ka.nx > 16) return false;
    if (ka.mk < 1 || ka.mk > 4 || (!ka.C.ptr && !ka.D.ptr)) return false;
    if (ka.N * ka.mk != ka.m || ka.N > NV) return false;
    if (ka.warm_state || (ka.opt_flags & MPCQP_OPT_SEED_VIOLATED)) return false;
    if (quad_general(ka) && ka.order) return false;  // (the general build has no instantiation with a pairing order)
    return true;
}

bool quad_eligible(const KernelArgs &ka, int64_t batch, SimdCount &simds)
{
    if (!quad_applies(ka) || (ka.opt_flags & MPCQP_OPT_TWO_PER_WAVE)) return false;
    // (the general build at every batch size: the two-per-wavefront kernel's generic build stages its operands in LDS and is the slower
    // one from a single wavefront up -- the reference's WIP example, N = 12: 256 problems 13.2 against 19.3 us, 2048: 14.2 / 21.8,
    // 4096: 15.1 / 25.8; a random family with C + D rows and a stage cost, 12 iterations: 32.5 / 40.3, 39.5 / 49.7, 45.3 / 61.6;
    // tools/ab_quad_general.py)
    return (ka.opt_flags & MPCQP_OPT_FOUR_PER_WAVE) || quad_general(ka) || quad_pays(batch, simds);
}

#endif

template <int NX> static int launch_quad_t(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    const int64_t waves = (batch + 3) / 4;
    auto go = [&](auto kern, size_t per) {
        const size_t bytes = per * 4 * sizeof(double);
        hipLaunchKernelGGL(kern, dim3((unsigned)waves), dim3(64), bytes, st, (const double *)ka.A.ptr, (const double *)ka.B.ptr,
                           (const double *)ka.C.ptr, (const double *)ka.e.ptr, (const double *)ka.x0.ptr,
                           (const double *)ka.goal.ptr, (const double *)nullptr, (double *)ka.U, (double *)ka.lam, ka.status, ka.iters,
                           ka, batch);
    };
    // one round (at most one wavefront per SIMD): the roomy carve; several rounds: the slim one, two wavefronts per SIMD
    const bool slim = waves > device_simds_now();
    if (NX > 4 || quad_general(ka)) {  // (nx = 5, 6: the general build only -- three / four operand registers per step)
        auto gen = [&](auto kern, size_t per) {
            hipLaunchKernelGGL(kern, dim3((unsigned)waves), dim3(64), per * 4 * sizeof(double), st, (const double *)ka.A.ptr,
                               (const double *)ka.B.ptr, (const double *)ka.C.ptr, (const double *)ka.e.ptr, (const double *)ka.x0.ptr,
                               (const double *)ka.goal.ptr, (const double *)ka.targets.ptr, (double *)ka.U, (double *)ka.lam, ka.status,
                               ka.iters, ka, batch);
        };
        if (slim)
            gen(mpcqp_quad_kernel<NX, false, 1, true, false, true>, Carve<true>::PER);
        else
            gen(mpcqp_quad_kernel<NX, false, 1, false, false, true>, Carve<false>::PER);
    } else if constexpr (NX <= 4) {
        if (ka.order) {
            if (slim)
                go(mpcqp_quad_kernel<NX, true, 1, true>, Carve<true>::PER);
            else
                go(mpcqp_quad_kernel<NX, true, 1, false>, Carve<false>::PER);
        } else if (slim) {
            go(mpcqp_quad_kernel<NX, false, 1, true>, Carve<true>::PER);
        } else {
            go(mpcqp_quad_kernel<NX, false, 1, false>, Carve<false>::PER);
        }
    }
    return (int)hipGetLastError();
}

#ifdef MPCQP_QUAD_WIDE_UNIT
int launch_quad_wide(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    if (ka.nx == 5) return launch_quad_t<5>(ka, batch, st);
    if (ka.nx == 6) return launch_quad_t<6>(ka, batch, st);
    // nx = 7 .. 16: the streamed build, compiled for the padded sizes 8, 12, 16
    return ka.nx <= 8 ? launch_quad_t<8>(ka, batch, st) : ka.nx <= 12 ? launch_quad_t<12>(ka, batch, st) : launch_quad_t<16>(ka, batch, st);
}
#else
int launch_quad_wide(const KernelArgs &ka, int64_t batch, hipStream_t st);  // (mpcqp_quadw.hip)

int launch_quad(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    switch (ka.nx) {
    case 2: return launch_quad_t<2>(ka, batch, st);
    case 3: return launch_quad_t<3>(ka, batch, st);
    case 4: return launch_quad_t<4>(ka, batch, st);
    default: return launch_quad_wide(ka, batch, st);
    }
}

// Shared-model launches (mpcqp_solve_model_batch / _bounds_batch): any cost and constraint layout the model was factored from, as
// long as the condensed problem fits the rows (the caller has checked pair_eligible(ka, MODE_MODEL)).
bool quad_model_eligible(const KernelArgs &ka, int64_t batch, SimdCount &simds)
{
    if (ka.n > NV || ka.m > MMAX || ka.m < 1 || ka.warm_state || (ka.opt_flags & (MPCQP_OPT_TWO_PER_WAVE | MPCQP_OPT_SEED_VIOLATED)))
        return false;
    return (ka.opt_flags & MPCQP_OPT_FOUR_PER_WAVE) || quad_pays(batch, simds);
}

int launch_quad_model(const KernelArgs &ka, int64_t batch, hipStream_t st)
{
    const int64_t waves = (batch + 3) / 4;
    auto go = [&](auto kern, size_t per) {
        const size_t bytes = per * 4 * sizeof(double);
        hipLaunchKernelGGL(kern, dim3((unsigned)waves), dim3(64), bytes, st, (const double *)ka.model, (const double *)nullptr,
                           (const double *)nullptr, (const double *)ka.e.ptr, (const double *)ka.x0.ptr, (const double *)ka.goal.ptr,
                           (const double *)ka.targets.ptr, (double *)ka.U, (double *)ka.lam, ka.status, ka.iters, ka, batch);
    };
    const bool slim = waves > device_simds_now();
    if (ka.order) {
        if (slim)
            go(mpcqp_quad_kernel<3, true, 1, true, true>, Carve<true>::PER);
        else
            go(mpcqp_quad_kernel<3, true, 1, false, true>, Carve<false>::PER);
    } else if (slim) {
        go(mpcqp_quad_kernel<3, false, 1, true, true>, Carve<true>::PER);
    } else {
        go(mpcqp_quad_kernel<3, false, 1, false, true>, Carve<false>::PER);
    }
    return (int)hipGetLastError();
}

#endif  // MPCQP_QUAD_WIDE_UNIT

}  // namespace mpcqp
