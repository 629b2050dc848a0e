// mpcqp_model_small.h -- what the sixteen-lanes-per-problem kernels of a factored shared model share (n <= 16, m <= 32,
// nx <= 16): the LDS image of the model's matrices, the workgroup shape, the per-problem KKT block and the grid.
// Included by mpcqp_model_adjoint.hip (mpcqp_model_diff_small_kernel, mpcqp_loop_adjoint_small_kernel) and
// mpcqp_loop_tangent.hip (mpcqp_loop_tangent_small_kernel); DESIGN.md section 9.
#ifndef MPCQP_MODEL_SMALL_H
#define MPCQP_MODEL_SMALL_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mpcqp_internal.h"
#include "mpcqp_lane.h"

namespace mpcqp {

namespace {

// LDS image of the shared matrices, in doubles: M [m][16], L^-T [16][16], Wx [16][nx], Wg [16][nx], Wt [16][N nx],
// Hx [m][nx]
struct SmallImage {
    int M, Lt, Wx, Wg, Wt, Hx, total;
};
__host__ __device__ inline SmallImage make_small_image(int nx, int N, int m)
{
    SmallImage s{};
    s.M = 0;
    s.Lt = s.M + m * 16;
    s.Wx = s.Lt + 256;
    s.Wg = s.Wx + 16 * nx;
    s.Wt = s.Wg + 16 * nx;
    s.Hx = s.Wt + 16 * N * nx;
    s.total = s.Hx + m * nx;
    return s;
}

constexpr int kSmallThreads = 256;                       // four wavefronts,
constexpr int kSmallPerBlock = kSmallThreads / 16;       // sixteen problems per round of a workgroup

// The KKT block of one problem on its sixteen lanes, as mpcqp_model_diff_small_kernel has it inline, in a struct: the
// active rows' ids (slot i takes the i-th set bit of lam > 0, two ballots), this slot's row `ma` of M_A, S = M_A M_A' with
// row `l` on lane l, its in-place lower Cholesky factor, and the products and solves with them. `l` is the lane within the
// row of sixteen, `g` the row within the wavefront; every loop over slots stops at kmax, the largest k of the wavefront's
// four problems, so every member is called by the whole wavefront. (mpcqp_model_diff_small_kernel keeps its own text: built
// on this struct it compiled to 202 / 168 VGPRs, not the 204 / 169 of profiles/model_diff_kernel_resources.txt; DESIGN.md
// section 9, "Closed-loop adjoint".)
struct SmallKkt {
    unsigned act;     // bit r: row r is active
    int k, kmax, id;  // active rows; this slot's row (0 past the k-th: its products are masked)
    double dinv;
    double ma[16], S[16];

    // -> false when more rows are active than there are variables (not a vertex's multipliers): k is then 0
    __device__ __forceinline__ bool build(const double *Mm, const double *lam, bool live, int l, int g, int n, int m)
    {
        const bool a0 = live && l < m && lam[l] > 0.0, a1 = live && l + 16 < m && lam[l + 16] > 0.0;
        const unsigned long long m0 = __ballot(a0), m1 = __ballot(a1);
        act = (unsigned)((m0 >> (16 * g)) & 0xffffull) | ((unsigned)((m1 >> (16 * g)) & 0xffffull) << 16);
        k = __popc(act);
        const bool fits = k <= n;
        if (!fits) k = 0;
        id = 0;
        {
            unsigned x = act;
            for (int s = 0; s < 15; ++s)
                if (s < l) x &= x - 1;
            if (l < k) id = __builtin_ctz(x);
        }
        kmax = max(max(lane_get(k, 0), lane_get(k, 16)), max(lane_get(k, 32), lane_get(k, 48)));
#pragma unroll
        for (int c = 0; c < 16; ++c) ma[c] = l < k ? Mm[id * 16 + c] : 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) {
            S[c] = 0.0;
            if (c < kmax) {
                const int idc = __shfl(id, c, 16);
                const double *mc = Mm + idc * 16;
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 16; ++j) acc += ma[j] * mc[j];
                S[c] = (c < k) ? acc : 0.0;
            }
        }
        return fits;
    }

    // in-place lower Cholesky, the pivot test of chol_lower (mpcqp_adjoint_common.h) -> false when a pivot fails
    __device__ __forceinline__ bool factor(int l)
    {
        bool bad = false;
        dinv = 0.0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < kmax) {
                const double d = __shfl(S[j], j, 16);
                const bool in = j < k;
                if (in && !(d > 0.0)) bad = true;
                const bool ok = in && !bad;
                const double sd = ok ? sqrt(d) : 1.0, inv = ok ? 1.0 / sd : 0.0;
                if (l == j) dinv = inv;
                const double lij = (l == j) ? sd : S[j] * inv;
                S[j] = lij;
#pragma unroll
                for (int c = j + 1; c < 16; ++c) {
                    if (c < kmax) {
                        const double lcj = __shfl(lij, c, 16);
                        S[c] -= lij * lcj;
                    }
                }
            }
        }
        return !bad;
    }

    // x <- S^-1 x for the slot-distributed x
    __device__ __forceinline__ double solve(double x, int l) const
    {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            if (j < kmax) {
                if (l == j) x *= dinv;
                const double xj = __shfl(x, j, 16);
                if (l > j) x -= S[j] * xj;
            }
        }
#pragma unroll
        for (int j = 15; j >= 0; --j) {
            if (j < kmax) {
                const double s = row_sum_dpp((l > j && l < k) ? S[j] * x : 0.0);
                if (l == j) x = (x - s) * dinv;
            }
        }
        return (l < k) ? x : 0.0;
    }

    // y_l = sum_i M[id_i][l] x_i for the slot-distributed x
    __device__ __forceinline__ double rows_t(const double *Mm, double x, int l) const
    {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < kmax) {
                const int idi = __shfl(id, i, 16);
                const double xi = __shfl(x, i, 16);
                acc += Mm[idi * 16 + l] * xi;
            }
        }
        return acc;
    }

    // sum_c ma[c] v_c for the variable-distributed v
    __device__ __forceinline__ double rows(double v) const
    {
        double acc = 0.0;
#pragma unroll
        for (int c = 0; c < 16; ++c) acc += ma[c] * __shfl(v, c, 16);
        return acc;
    }
};

// workgroups of sixteen problems a round, at most kModelDiffMaxGrid of them: larger batches take further rounds
inline int model_diff_small_grid(int64_t batch)
{
    const int64_t blocks = (batch + kSmallPerBlock - 1) / kSmallPerBlock;
    return (int)(blocks < kModelDiffMaxGrid ? blocks : kModelDiffMaxGrid);
}

}  // namespace

}  // namespace mpcqp
#endif
