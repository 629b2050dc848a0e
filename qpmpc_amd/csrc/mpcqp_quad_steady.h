// mpcqp_quad_steady.h -- the STEADY LOOP of mpcqp_quad_kernel (mpcqp_quad.hip): a fragment of that kernel's body, included once at the
// top of its outer loop, in front of the general active-set loop. It is no header in the usual sense: it reads and writes the kernel's
// local state (RT, RH, RM0, RM1, s0, s1, lam, myact, occ, e0, e1, mask, nq, iters, zn, cT, cH, done, status, p, up, needp; hd, kd0, kd1,
// inv, t2, rd of the trip it leaves with) and defines `general`, false when every row finished here and the general loop has nothing to
// do. It was split out while a test named lines of the kernel file; none does now (tests/dpp_instantiations.py names the launcher
// functions), so nothing but history keeps it in a file of its own.
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
    const int iters_in = iters, nq_in = nq;
    // the lane flags travel as the wavefront's lane masks (every lane is active here): no 0/1 bytes in vector registers. A new mask is
    // the ballot of ONE compare, combined with the carried masks by scalar logic: the ballot of a combined predicate goes through a 0/1
    // register and a second compare
    auto maskof = [](bool b) { return (unsigned long long)__builtin_amdgcn_ballot_w64(b); };
    auto lanes = [](unsigned long long m) { return __builtin_amdgcn_inverse_ballot_w64(m); };
    unsigned long long donem = maskof(done), occm = maskof(occ), e0m = maskof(e0), e1m = maskof(e1);
    const unsigned long long done_in = donem;
    // iters and nq both grow by one per trip a row steps: ONE counter of those trips, against the nearer of the two limits (the
    // iteration limit, nq = n); both are rebuilt behind the loop, where a row that finished here gets its status too
    int ks = 0;
    const int klim = min(max_iter - iters_in, n - nq_in);
    static_assert(USPLIT % 4 == 0, "the four steps of the row minimum stand between the quarters of the update's first half");
    dpp_ready(zn);  // (on the entry edge only: inside the loop zn is written in a trip's bookkeeping, many instructions in front of the
    for (;;) {      // next trip's first FMA -- tools/check_dpp_hazards.py follows the back edge)
        {  // select() of a row that needs a constraint and is not dropping. The four steps of its row minimum are hand-written (min_ror)
            // and stand between the hand-written FMAs of the update's first half, four FMAs apart: the compiler pads its own DPP steps
            // there with s_nop 1 each, because it counts no wait states for inline asm
            const unsigned h0 = ~(unsigned)__double2hiint(s0 * invn0), h1 = ~(unsigned)__double2hiint(s1 * invn1);
            const bool v0 = lanes(~donem & e0m & maskof(s0 < -tolh0)), v1 = lanes(~donem & e1m & maskof(s1 < -tolh1));
            const unsigned k0 = v0 ? ((h0 & ~31u) | (unsigned)row0) : 0xffffffffu;
            const unsigned k1 = v1 ? ((h1 & ~31u) | (unsigned)row1) : 0xffffffffu;
            unsigned mkey = min(k0, k1);
            pin(mkey);  // (written here: four FMAs in front of its first DPP read)
            update(ic<0>{}, ic<USPLIT / 4>{}, zn, cT, cH);
            min_ror<8>(mkey);
            update(ic<USPLIT / 4>{}, ic<USPLIT / 2>{}, zn, cT, cH);
            min_ror<4>(mkey);
            update(ic<USPLIT / 2>{}, ic<3 * USPLIT / 4>{}, zn, cT, cH);
            min_ror<2>(mkey);
            update(ic<3 * USPLIT / 4>{}, ic<USPLIT>{}, zn, cT, cH);
            min_ror<1>(mkey);
            donem |= maskof(mkey == 0xffffffffu);  // no violated row: solved (a row that is done has no key either)
            p = lanes(donem) ? p : (int)(mkey & 31u);
        }
        ld16(mp, Ml + p * LDM);
        update(ic<USPLIT>{}, ic<NV>{}, zn, cT, cH);
        if (donem == ~0ull) {  // every row is done: no general trip either
            general = false;
            break;
        }
        const unsigned long long stm = ~donem, phim = maskof(p >= NV);  // stm: this row steps; phim (row-uniform)
        const bool st = lanes(stm), phi = lanes(phim);
        const int pl = p & 15;
        {  // hd = dot16(RH, mp), its sums and their order, with TWO waits for row p: each half of the row is pinned as a whole in front of
            // the eight FMAs that read it (the compiler waits once per pin; left alone, it waits once per 16-byte read, eight times)
            asm volatile("" : "+v"(mp[0]), "+v"(mp[1]), "+v"(mp[2]), "+v"(mp[3]), "+v"(mp[4]), "+v"(mp[5]), "+v"(mp[6]), "+v"(mp[7]));
            T c0 = T(0), c1 = T(0), c2 = T(0), c3 = T(0);
            static_for<0, 2>([&](auto qc) {
                constexpr int k = 4 * decltype(qc)::value;
                c0 += RH[k] * mp[k], c1 += RH[k + 1] * mp[k + 1], c2 += RH[k + 2] * mp[k + 2], c3 += RH[k + 3] * mp[k + 3];
            });
            asm volatile("" : "+v"(mp[8]), "+v"(mp[9]), "+v"(mp[10]), "+v"(mp[11]), "+v"(mp[12]), "+v"(mp[13]), "+v"(mp[14]), "+v"(mp[15]),
                         "+v"(c0), "+v"(c1), "+v"(c2), "+v"(c3));
            static_for<2, 4>([&](auto qc) {
                constexpr int k = 4 * decltype(qc)::value;
                c0 += RH[k] * mp[k], c1 += RH[k + 1] * mp[k + 1], c2 += RH[k + 2] * mp[k + 2], c3 += RH[k + 3] * mp[k + 3];
            });
            hd = (c0 + c1) + (c2 + c3);
        }
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
        const int sl = (int)__builtin_ctz(~mask);  // lowest free slot
        const T r = lanes(occm & stm) ? rd : T(0);
        // not plain -- inv <= 0 (near dependence, the general loop's sum of squares), a limit, a blocking multiplier --: the general
        // loop finishes THIS trip
        if ((stm & (maskof(!(inv > T(0))) | maskof(ks >= klim) | (maskof(r > T(0)) & maskof(lam < t2 * r)))) != 0ull) break;
        // ---- the plain trip's bookkeeping (a row that is done: zero coefficients, nothing changes)
        inv = st ? inv : T(0);
        const T tt = st ? t2 : T(0);
        const unsigned long long slm = maskof(l == sl), isnewm = slm & stm, ispm = maskof(l == pl) & stm;
        const bool isnew = lanes(isnewm);
        ks += st ? 1 : 0;
        zn = hd;
        cT = lanes(slm) ? inv : -(r * inv);
        cH = -(hd * inv);
        s0 = fma(tt, kd0, s0);  // s_i -= t M_i . z
        s1 = fma(tt, kd1, s1);
        T ln = fma(-tt, r, lam);
        ln = lanes(occm & maskof(ln < T(0))) ? T(0) : ln;
        lam = isnew ? tt : ln;  // (up + tt with up = 0 since the selection; tt > 0)
        myact = isnew ? p : myact;
        occm |= isnewm;
        e0m &= ~(ispm & ~phim);
        e1m &= ~(ispm & phim);
        mask |= st ? (1u << sl) : 0u;
    }
    done = lanes(donem);
    occ = lanes(occm);
    e0 = lanes(e0m);
    e1 = lanes(e1m);
    status = lanes(donem & ~done_in) ? (int)MPCQP_SOLVED : status;  // (the one way a row finishes in this loop)
    iters = iters_in + ks;
    nq = nq_in + ks;
    // what select() and the plain trips leave in the state this loop does not carry: a row that selected has up = 0; one that
    // still steps holds its p (needp false), one that stepped and is done asks for a new one (never read before it is reset)
    const bool went = ks != 0;
    up = (went | !done) ? T(0) : up;
    needp = done ? (needp | went) : false;
    cT = cH = T(0);  // (the update of the trip that left has been applied)
}
