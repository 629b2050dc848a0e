// mpcqp_quad_steady.h -- the STEADY LOOP of mpcqp_quad_kernel (mpcqp_quad.hip): a fragment of that kernel's body, included once at the
// top of its outer loop, in front of the general active-set loop. It is no header in the usual sense: it reads and writes the kernel's
// local state (RT, RH, RM0, RM1, s0, s1, lam, myact, occ, e0, e1, mask, nq, iters, zn, cT, cH, done, status, p, up, needp; hd, kd0, kd1,
// inv, t2, rd of the trip it leaves with) and defines `general`, false when every row finished here and the general loop has nothing to
// do. It sits in a file of its own so that the kernel file keeps its line numbers (tests/dpp_instantiations.py names the launch lines
// of every instantiation).
//
// Nearly every trip is a plain one -- every row still in the loop selects a constraint and takes the full step, no multiplier
// blocks (config 2: 10.75 iterations per problem, 10.75 rows active at the optimum). Those trips run here, in a loop of one
// basic block that carries only what a plain trip changes; the flags stay lane masks. Here every row that is not done needs a new
// constraint (true at the kernel's start, after a failed acceptance and whenever the general loop hands back; kept by every plain trip).
// The first trip that is not plain -- near dependence, a step that cannot be taken, the iteration limit, a blocking multiplier --
// leaves WITHOUT its bookkeeping: the general loop behind this one FINISHES that trip from hd, kd0, kd1, inv, t2, rd, which are what it
// would compute itself, and comes back here as soon as no live row holds a p. Same operations in the same order as its plain arm.
bool general = true;
{
    const int iters_in = iters;
    // the lane flags travel as the wavefront's lane masks (every lane is active here): no 0/1 bytes in vector registers
    auto maskof = [](bool b) { return (unsigned long long)__builtin_amdgcn_ballot_w64(b); };
    auto lanes = [](unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); };
    unsigned long long donem = maskof(done), occm = maskof(occ), e0m = maskof(e0), e1m = maskof(e1);
    for (;;) {
        dpp_ready(zn);
        update(ic<0>{}, ic<USPLIT>{}, zn, cT, cH);
        {  // select() of a row that needs a constraint and is not dropping
            const bool want = !lanes(donem), e0 = lanes(e0m), e1 = lanes(e1m);
            const unsigned h0 = ~(unsigned)__double2hiint(s0 * invn0), h1 = ~(unsigned)__double2hiint(s1 * invn1);
            const bool v0 = want & e0 & (s0 < -tolh0), v1 = want & e1 & (s1 < -tolh1);
            const unsigned k0 = v0 ? ((h0 & ~31u) | (unsigned)row0) : 0xffffffffu;
            const unsigned k1 = v1 ? ((h1 & ~31u) | (unsigned)row1) : 0xffffffffu;
            const unsigned mkey = row_min(min(k0, k1));
            const bool none = want & (mkey == 0xffffffffu);
            donem |= maskof(none);
            status = none ? (int)MPCQP_SOLVED : status;
            p = (want & !none) ? (int)(mkey & 31u) : p;
        }
        ld16(mp, Ml + p * LDM);
        update(ic<USPLIT>{}, ic<NV>{}, zn, cT, cH);
        const bool st = !lanes(donem), occ = lanes(occm);  // st: this row steps
        if (donem == ~0ull) {  // every row is done: no general trip either
            general = false;
            break;
        }
        const bool phi = p >= NV;  // (row-uniform)
        const int pl = p & 15;
        hd = dot16(RH, mp);
        {  // dot_bcast(hd, RM0, 0), dot_bcast(hd, RM1, 0) on ONE pinned copy of hd: each sum's chains in their own order
            T a0 = T(0), a1 = T(0), b0 = T(0), b1 = T(0);
            dpp_ready(hd);
            static_for<0, NV / 2>([&](auto kk) {
                constexpr int k = 2 * decltype(kk)::value;
                fmac_bcast<k>(a0, hd, RM0[k]);
                fmac_bcast<k + 1>(a1, hd, RM0[k + 1]);
                fmac_bcast<k>(b0, hd, RM1[k]);
                fmac_bcast<k + 1>(b1, hd, RM1[k + 1]);
            });
            kd0 = a0 + a1;
            kd1 = b0 + b1;
        }
        {
            const T kp = phi ? kd1 : kd0, sq = phi ? s1 : s0, iq = phi ? invn1 : invn0;
            const bool okf = kp * iq * iq > T(DEP_FAST);
            const T iv = fast_rcp(kp);
            inv = row_get(okf ? iv : T(-1), rb, pl);
            t2 = row_get(-sq * iv, rb, pl);
        }
        rd = dot16(RT, mp);  // (while the exchange is in flight)
        pin(rd);
        const bool can_move = (nq < n) & (inv > T(0));  // (inv <= 0: near dependence, the general loop's sum of squares)
        const int sl = (int)__builtin_ctz(~mask);  // lowest free slot
        const T r = (occ & st) ? rd : T(0);
        const bool blk = (r > T(0)) & (lam < t2 * r);
        if (maskof(st & (!can_move | (iters >= max_iter) | blk)) != 0ull) break;  // not plain: the general loop finishes THIS trip
        // ---- the plain trip's bookkeeping (a row that is done: zero coefficients, nothing changes)
        inv = st ? inv : T(0);
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
        lam = isnew ? tt : ln;  // (up + tt with up = 0 since the selection; tt > 0)
        myact = isnew ? p : myact;
        occm |= maskof(isnew);
        e0m &= ~maskof(isp & !phi);
        e1m &= ~maskof(isp & phi);
        mask |= st ? (1u << sl) : 0u;
        nq += st ? 1 : 0;
    }
    done = lanes(donem);
    occ = lanes(occm);
    e0 = lanes(e0m);
    e1 = lanes(e1m);
    // what select() and the plain trips leave in the state this loop does not carry: a row that selected has up = 0; one that
    // still steps holds its p (needp false), one that stepped and is done asks for a new one (never read before it is reset)
    const bool went = iters != iters_in;
    up = (went | !done) ? T(0) : up;
    needp = done ? (needp | went) : false;
    cT = cH = T(0);  // (the update of the trip that left has been applied)
}
