// mpcqp_quad_operands.h -- the OPERAND LOADS of mpcqp_quad_kernel's build (mpcqp_quad.hip): a fragment of that kernel's body, included
// once, right behind the two base pointers it needs (A, Cm) and in front of every other load of the build. It is no header in the
// usual sense: it reads the kernel's locals (l, N, A, Cm, sA, sC, NAe, NEr) and fills op[][]. It was split out while a test named lines
// of the kernel file; none does now, so nothing but history keeps it in a file of its own.
//
// Lane e of the row keeps element e (and e + 16, ...) of [A_k | C_k] for every step k, straight from HBM; the chain fetches an operand
// as a DPP row broadcast (lanes without an element load a valid address and are never read). The chain's first step waits for the first
// of these loads, so they come first: one per-lane base and one per-lane BYTE STRIDE (that of A or that of C: with nx = 3 the lanes of
// both kinds share a register, so the step offset cannot be an immediate of the instruction; zero for an operand that is time-invariant:
// every step reads one address), and per load one multiply-add on them. That holds for the full horizon, N = 16, behind ONE
// wavefront-uniform test; any other N clamps the step, as before: a load never reaches past step N - 1 of its problem.
if constexpr (!WIDE) {
    static_for<0, NOP>([&](auto rc) {
        constexpr int r = decltype(rc)::value;
        const int e = l + 16 * r;
        const bool ok = e < NEr;
        const T *p = (e < NAe) ? A + e : Cm + (ok ? e - NAe : 0);
        const int st = (e < NAe) ? sA : sC;
        if (N == NV) {
            const uint32_t stb = (uint32_t)st * (uint32_t)sizeof(T);
#pragma unroll
            for (int k = 0; k < NV; ++k) op[r][k] = *reinterpret_cast<const T *>(reinterpret_cast<const char *>(p) + (uint64_t)k * stb);
        } else {
#pragma unroll
            for (int k = 0; k < NV; ++k) {
                const int kc = (k < N) ? k : N - 1;
                op[r][k] = p[kc * st];
            }
        }
    });
}
