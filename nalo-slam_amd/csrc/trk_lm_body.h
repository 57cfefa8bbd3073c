// The body of both persistent LM kernels of kernels_trk_lm.hip, included once into each (function-body text: no include guard, nothing else includes it).
// The including kernel provides: TrkLmParams P; constexpr bool kTries; and, read only where kTries is true, TrkLmTries Q, LmTriesState* Xp, double* list (LDS).
// kTries = false is nalo_trk_track's launch: one descent, described by P alone. kTries = true adds the outer level: when a descent ends, wave 0 runs
// lm_try_finished and the loop goes on with the next hypothesis; the per-evaluation code is the same text. Sharing the text through an include and not
// through a template keeps trk_lm_kernel's instructions what they were before the second kernel existed (an inlined template body got another schedule).
    __shared__ float rows[(kLmThreads / 4) * kLmStride];
    __shared__ double sums[64];
    __shared__ double part[kLmThreads / 64][64];
    __shared__ LmState S;
    __shared__ int bar_ok;
    const int tid = threadIdx.x, blk = blockIdx.x, NB = gridDim.x;
    const float lambdaExtrapolationLimit = 0.001f;
    int timed_out = 0;
    if (tid == 0) bar_ok = 1;
    float c_id = 0.f, c_x = 0.f, c_y = 0.f, c_rc = 0.f;   // this lane's point of level cached_lvl (levels that fit one round of the grid)
    int cached_lvl = -1;

    // every block keeps its own copy of the LM state and advances it with the same inputs (the summed partials): the control flow is
    // replicated, not broadcast, which saves a second grid barrier per evaluation
    if (tid == 0) {
        for (int i = 0; i < 12; ++i) S.T[i] = P.T0[i];
        S.aff[0] = P.aff0[0]; S.aff[1] = P.aff0[1];
        for (int i = 0; i < 5; ++i) S.lastRes[i] = NAN;
        S.flow[0] = S.flow[1] = S.flow[2] = 1000;
        S.lvl = P.coarsest; S.it = 0; S.phase = 0; S.next_lvl = -1; S.haveRepeated = P.have_repeated_in; S.good = 1; S.evals = 0; S.done = 0; S.break_pending = 0;
        S.levelCutoffRepeat = 1; S.lambda = 0.01f;
        for (int i = 0; i < NALO_MAX_LEVELS; ++i) S.evals_lvl[i] = 0;
        double T0[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) T0[i] = P.T0[i];
        lm_prepare_eval(S, P, P.coarsest, 1.f, T0, P.aff0[0], P.aff0[1], true);
        if constexpr (kTries) {
            LmTriesState& X = *Xp;
            for (int i = 0; i < 5; ++i) X.ach[i] = NAN;
            for (int i = 0; i < 12; ++i) X.T[i] = P.T0[i];
            X.aff[0] = P.aff0[0]; X.aff[1] = P.aff0[1];
            X.flow[0] = X.flow[1] = X.flow[2] = 0;
            X.cur = 0; X.have = 0; X.winner = -1; X.par = 0; X.tag0 = (Q.launch0 & 0xFFFFFu) << 12;
            for (int i = 0; i < NALO_MAX_LEVELS; ++i) X.evals_lvl[i] = 0;
        }
    }
    if constexpr (kTries) for (int i = tid; i < Q.n_tries * 12; i += kLmThreads) list[i] = Q.list[i];
    __syncthreads();
    int my_try = 0;                                         // kTries: the try this lane's guard counts for

    // phase 0: first evaluation of a level at the accepted estimate (with the cutoff-repeat loop, :1104-1115)
    // phase 1: evaluation of an LM candidate (:1184)
    for (int guard = 0; guard < 4096; ++guard) {
        if (S.done) break;
        if constexpr (kTries) { if (Xp->cur != my_try) { my_try = Xp->cur; guard = 0; } }      // the bound is per try, like its evaluation numbers
        // ------------------------------------------------------------- fused calcRes + calcGS over this level's points
        const TrkLevel& L = P.lv[S.lvl];
        float acc[kTrkVals];
#pragma unroll
        for (int k = 0; k < kTrkVals; ++k) acc[k] = 0.f;
        {
            const float wlm3 = (float)(L.wl - 3), hlm3 = (float)(L.hl - 3);
            const float affa = S.affa, affb = S.affb, b0 = S.b0, cutoff = S.cutoff, maxEnergy = S.maxEnergy;
            const int lvl = S.lvl;
            float RK[9], Kq[9], tt[3];
#pragma unroll
            for (int q = 0; q < 9; ++q) { RK[q] = S.RKi[q]; Kq[q] = S.Ki[q]; }
            tt[0] = S.t[0]; tt[1] = S.t[1]; tt[2] = S.t[2];
            // G = 1 point per lane per round in flight (point loads, then the texel gathers, then the arithmetic); the rounds stride over the grid. Two
            // points per lane measured within +-2 %. The [G] arrays and one-trip g loops stay: written with scalars, the same
            // evaluation compiles to a different instruction schedule
            constexpr int G = 1;
            const int gthreads = NB * kLmThreads;
            // A level whose points fit ONE round of the grid (<= 64 x 512 points) gives each lane one point for all the ~5 evaluations of the level: it is
            // loaded once and stays in four registers, which takes one of the two dependent memory round trips (point -> texels) out of every later
            // evaluation. Not every level of a KITTI-sized cloud does: the headline cloud (8750 inputs) has 41 711 and 36 103 points on levels 0 and 1, two
            // rounds each, the second ragged (18 and 7 of the 64 workgroups); its levels 2 and 3 (21 381 and 6 249 points) fit one round.
            const bool one_round = L.n <= gthreads;
            if (one_round && cached_lvl != lvl) {
                const int i = blk * kLmThreads + tid, ii = i < L.n ? i : 0;
                c_id = L.id[ii]; c_x = L.u[ii]; c_y = L.v[ii]; c_rc = L.col[ii];
                cached_lvl = lvl;
            }
            for (int base = blk * kLmThreads + tid; base < L.n; base += G * gthreads) {
                float id[G], x[G], y[G], rc[G], Ku[G], Kv[G], uu[G], vv[G], nid[G];
                bool inb[G], ok[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int i = base + g * gthreads;
                    inb[g] = i < L.n;
                    const int ii = inb[g] ? i : 0;
                    if (one_round) { id[g] = c_id; x[g] = c_x; y[g] = c_y; rc[g] = c_rc; }
                    else { id[g] = L.id[ii]; x[g] = L.u[ii]; y[g] = L.v[ii]; rc[g] = L.col[ii]; }
                }
                float4 p00[G], p10[G], p01[G], p11[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    trk_project(RK, tt, L, x[g], y[g], id[g], uu[g], vv[g], Ku[g], Kv[g], nid[g]);
                    ok[g] = inb[g] && (Ku[g] > 2.f && Kv[g] > 2.f && Ku[g] < wlm3 && Kv[g] < hlm3 && nid[g] > 0.f);        // :981
                    const int ix = ok[g] ? (int)Ku[g] : 2, iy = ok[g] ? (int)Kv[g] : 2;
                    const float4* bp = L.dI + ix + iy * L.wl;
                    p00[g] = bp[0]; p10[g] = bp[1]; p01[g] = bp[L.wl]; p11[g] = bp[1 + L.wl];
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int i = base + g * gthreads;
                    if (inb[g] && lvl == 0 && (i & 31) == 0) trk_flow(acc, RK, Kq, tt, L, x[g], y[g], id[g], Ku[g], Kv[g]);
                    if (!ok[g]) continue;
                    const float3 hit = trk_interp(Ku[g], Kv[g], p00[g], p10[g], p01[g], p11[g]);
                    if (!isfinite(hit.x)) continue;
                    float hw; const float residual = trk_residual(hit.x, rc[g], affa, affb, hw);
                    acc[kTrkNE] += 1.f;
                    if (fabsf(residual) > cutoff) { acc[kTrkE] += maxEnergy; acc[kTrkNSat] += 1.f; }
                    else {
                        acc[kTrkE] += hw * residual * residual * (2.f - hw);
                        acc[kTrkNWarped] += 1.f;
                        float J[9];
                        trk_jacobian(J, hit, rc[g], uu[g], vv[g], nid[g], L.fx, L.fy, affa, b0, residual);
#pragma unroll
                        for (int r = 0; r < 9; ++r) {
                            const float Jw = J[r] * hw;
#pragma unroll
                            for (int c2 = r; c2 < 9; ++c2) acc[trk_ut(r, c2)] += Jw * J[c2];
                        }
                    }
                }
            }
        }
        // ------------------------------------------------------------- block reduction (same scheme as reduce.h), then the grid sum
        const int nbl = min(NB, (L.n + kLmThreads - 1) / kLmThreads);          // blocks that own points of this level
        if (blk < nbl) {
#pragma unroll
            for (int k = 0; k < kTrkVals; ++k) acc[k] = dpp_quad_sum(acc[k]);
            if ((tid & 3) == 0) {
                float* row = rows + (tid >> 2) * kLmStride;
#pragma unroll
                for (int k = 0; k < kTrkVals; ++k) row[k] = acc[k];
            }
            __syncthreads();
            {                                                // fp64 column sums over the quad rows: (T/64) lane groups x 16 rows, fixed order
                const int j = tid & 63, g = tid >> 6;
                double s = 0;
                if (j < kTrkVals) for (int r = g * 16; r < g * 16 + 16; ++r) s += (double)rows[r * kLmStride + j];
                part[g][j] = s;
            }
            __syncthreads();
            if (tid < kTrkVals) {
                double s = 0; for (int g = 0; g < kLmThreads / 64; ++g) s += part[g][tid];
                if (NB == 1) sums[tid] = s;
                else __hip_atomic_store(&P.partial[((size_t)(kTries ? Xp->par : (S.evals & 1)) * NB + blk) * 64 + tid], lm_pack((float)s, (kTries ? Xp->tag0 : P.tag0) + (unsigned)S.evals), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (NB > 1) {                                        // block partials -> every block sums them in the same fixed order
            // the wave's group as a scalar, made here in every evaluation (the empty asm keeps what derives from it - block indices, guards - from being hoisted
            // out of the evaluation loop, where it would be live across the gather, the kernel's register peak)
            const int j = tid & 63;
            int g = __builtin_amdgcn_readfirstlane(tid >> 6);
            asm volatile("" : "+s"(g));
            const unsigned long long* pp = P.partial + (size_t)(kTries ? Xp->par : (S.evals & 1)) * NB * 64;
            const unsigned want = (kTries ? Xp->tag0 : P.tag0) + (unsigned)S.evals;
            double s = 0;
            bool pending = j < kTrkVals;
            // a pass loads all words of this lane's blocks back to back and waits once (lm_exchange_pass: 8 words on a grid of <= kLmMaxBlocks workgroups, 16
            // on the double grid); a pass that finds a tag missing is repeated whole until every tag matches
            constexpr int kWords = kLmMaxBlocks / (kLmThreads / 64);
            for (unsigned spins = 0; pending; ++spins) {
                pending = NB <= kLmMaxBlocks ? lm_exchange_pass<kWords>(pp, g, j, nbl, want, s) : lm_exchange_pass<2 * kWords>(pp, g, j, nbl, want, s);
                if (pending) { if (spins > (1u << 21)) { bar_ok = 0; break; } __builtin_amdgcn_s_sleep(1); }
            }
            part[g][j] = s;
            __syncthreads();
            if (!bar_ok) { timed_out = 1; break; }
            if (tid < kTrkVals) { double t2 = 0; for (int g2 = 0; g2 < kLmThreads / 64; ++g2) t2 += part[g2][tid]; sums[tid] = t2; }
        }
        __syncthreads();
        // ------------------------------------------------------------- wave 0 = the host of the reference
        // Scalars of the control flow are computed by every lane of the wave (uniform); the 8x8 solve puts one row per lane; lane 0 writes
        // the state back. Nothing here waits on memory other than a handful of LDS broadcasts.
        if (tid < 64) {
            const int lane = tid;
            int phase = S.phase, it = S.it, lvl = S.lvl, brk = S.break_pending, haveRep = S.haveRepeated, good = S.good, done = 0, next_lvl = S.next_lvl;
            float lambda = S.lambda, lcr = S.levelCutoffRepeat;
            const int evals = S.evals + 1;
            if (lane == 0) S.evals_lvl[S.lvl] += 1;
            // sums (52 doubles) -> stats6 and this lane's entry of the scaled H / b (CoarseTracker.cpp:1040-1046, 869-884)
            const double E = sums[kTrkE], nE = sums[kTrkNE], nSat = sums[kTrkNSat], nW = sums[kTrkNWarped], sT = sums[kTrkST], sRT = sums[kTrkSRT], sN = sums[kTrkSN];
            // (round 4: the three fp64 divisions an evaluation does not need are off wave 0's path - the two flow indicators are divided when a level ends, from the
            // sums kept meanwhile; the accepted estimate's E / nE is kept as a quotient instead of being divided again at every later test; same operands, same bits)
            const double st[6] = {E, nE, sT, sN, sRT, E / nE};
            const double inv = 1.0 / (double)(((long)nW + 3) & ~3L);
            const int hr = lane >> 3, hc = lane & 7, lo = hr < hc ? hr : hc, hi = hr < hc ? hc : hr;
            // trk_ut(lo, hi) and trk_ut(bl, 8) written out: through the function the same index compiles to a different instruction schedule
            const double Hval = sums[lo * 9 - lo * (lo - 1) / 2 + (hi - lo)] * inv * lm_scale(hr) * lm_scale(hc);
            const int bl = lane & 7;
            const double bval = sums[bl * 9 - bl * (bl - 1) / 2 + (8 - bl)] * inv * lm_scale(bl);
            double ro[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) ro[i] = S.resOld[i];
            int next_action;                                 // 0 = evaluate again at the accepted estimate, 1 = propose, 2 = finish level
            bool store_H = false, take_T = false;
            if (phase == 0) {
                store_H = true;
                if ((double)((float)nSat / (float)nE) > 0.6 && lcr < 50) { lcr *= 2; next_action = 0; }   // :1106-1113
                else { lambda = 0.01f; it = 0; brk = 0; next_action = 1; }
            } else {
                const bool accept = st[5] < ro[5];                                               // :1186 (resNew[0] / resNew[1]) < (resOld[0] / resOld[1])
                if (accept) { store_H = true; take_T = true; lambda *= 0.5f; }                   // :1202-1209
                else { lambda *= 4; if (lambda < lambdaExtrapolationLimit) lambda = lambdaExtrapolationLimit; }
                it++;
                next_action = brk ? 2 : 1;                                                       // `if(!(inc.norm() > 1e-3)) break;` (:1216-1221)
            }
            if (store_H) {
                S.H[lane] = Hval;
                if (lane < 8) S.b[lane] = bval;
#pragma unroll
                for (int i = 0; i < 6; ++i) ro[i] = st[i];
            }
            if (take_T) { if (lane < 12) S.T[lane] = S.Tn[lane]; else if (lane < 14) S.aff[lane - 12] = S.affn[lane - 12]; }
            lm_wave_sync();
            double T[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = S.T[i];
            const double aff0 = S.aff[0], aff1 = S.aff[1];
            if (next_action == 1) {
                if (it < lm_max_iterations(lvl)) {                                               // :1133-1184
                    double U[36], rhs[8], iv[8], is[8];
                    const float opl = 1 + lambda;
#pragma unroll
                    for (int r = 0; r < 8; ++r) {                // wave-uniform LDS reads (broadcast): every lane holds the whole system
#pragma unroll
                        for (int cc = r; cc < 8; ++cc) U[lm_ut(r, cc)] = S.H[r * 8 + cc];
                        U[lm_ut(r, r)] *= opl;
                        rhs[r] = -S.b[r];
                    }
                    lm_ldlt8_uniform(U, rhs, iv);
                    float extrapFac = 1;
                    if (lambda < lambdaExtrapolationLimit) extrapFac = sqrtf(sqrtf(lambdaExtrapolationLimit / lambda));
                    // labels swapped vs tangent order in the reference (:1172-1173): entries 0-2 scale with SCALE_XI_ROT, 3-5 with SCALE_XI_TRANS
#pragma unroll
                    for (int i = 0; i < 8; ++i) { iv[i] *= extrapFac; is[i] = iv[i] * (i < 3 ? (double)kScaleXiRot : i < 6 ? (double)kScaleXiTrans : i == 6 ? (double)kScaleA : (double)kScaleB); }
                    double ssum = 0, nrm = 0;
#pragma unroll
                    for (int i = 0; i < 8; ++i) { ssum += is[i]; nrm += iv[i] * iv[i]; }
                    if (!isfinite(ssum)) {
#pragma unroll
                        for (int i = 0; i < 8; ++i) is[i] = 0;
                    }
                    double E12[12], Tn[12];
                    lm_se3_exp(is, E12);
                    lm_se3_mul(E12, T, Tn);
                    const double affn0 = aff0 + is[6], affn1 = aff1 + is[7];
                    brk = !(sqrt(nrm) > 1e-3);
                    if (lane == 0) {
#pragma unroll
                        for (int i = 0; i < 12; ++i) S.Tn[i] = Tn[i];
                        S.affn[0] = affn0; S.affn[1] = affn1;
                    }
                    lm_prepare_eval(S, P, lvl, lcr, Tn, affn0, affn1, lane == 0);
                    phase = 1;
                } else next_action = 2;
            }
            if (next_action == 0) lm_prepare_eval(S, P, lvl, lcr, T, aff0, aff1, lane == 0);
            if (next_action == 2) {                                                              // level finished (:1225-1235)
                const double lr = (double)sqrtf((float)ro[5]);
                if (lane == 0) { S.lastRes[lvl] = lr; S.flow[0] = ro[2] / (ro[3] + 0.1); S.flow[1] = 0; S.flow[2] = ro[4] / (ro[3] + 0.1); }
                if (kTries ? lr > 1.5 * Xp->ach[lvl] : (P.has_minres && lr > 1.5 * P.minRes[lvl])) { good = 0; done = 1; }      // :1227; a list's bound is its achievedRes
                else {
                    int next = lvl - 1;
                    if (lcr > 1 && !haveRep) { next = lvl; haveRep = 1; }                        // repeat this level once
                    if (next < P.stop_lvl) { done = 1; next_lvl = next; }
                    else { lvl = next; lcr = 1; phase = 0; lm_prepare_eval(S, P, lvl, lcr, T, aff0, aff1, lane == 0); }
                }
            }
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 6; ++i) S.resOld[i] = ro[i];
                S.phase = phase; S.it = it; S.lvl = lvl; S.break_pending = brk; S.haveRepeated = haveRep; S.good = good; S.next_lvl = next_lvl;
                S.lambda = lambda; S.levelCutoffRepeat = lcr; S.evals = evals; S.done = done;
            }
            if constexpr (kTries) {
                if (lane == 0) Xp->par ^= 1;
                if (done) { lm_wave_sync(); lm_try_finished(S, *Xp, P, Q, list, lane, blk == 0); }
            }
        }
        __syncthreads();
    }
    if constexpr (kTries) {
        if (blk == 0 && tid == 0) {                          // the summary; the records went out as their tries ended (same lane, program order, before the release below)
            const LmTriesState& X = *Xp;
            double* o = Q.out;
            for (int i = 0; i < 12; ++i) o[i] = X.T[i];
            o[12] = X.aff[0]; o[13] = X.aff[1];
            for (int i = 0; i < 5; ++i) o[14 + i] = X.ach[i];
            for (int i = 0; i < 3; ++i) o[19 + i] = X.flow[i];
            o[22] = (timed_out || !S.done) ? -1.0 : 1.0;     // -1: a partial never arrived (or a try outran its guard): the host redoes the whole list
            o[23] = (double)X.have; o[24] = (double)X.cur; o[25] = (double)X.winner;
            for (int i = 0; i < 5; ++i) o[26 + i] = (double)X.evals_lvl[i];
            __threadfence_system();
            __hip_atomic_store(&o[31], P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    } else
    if (blk == 0 && tid == 0) {
        double* o = P.out;
        int ok = S.good;
        for (int i = 0; i < 12; ++i) o[i] = S.T[i];
        o[12] = S.aff[0]; o[13] = S.aff[1];
        for (int i = 0; i < 5; ++i) o[14 + i] = S.lastRes[i];
        for (int i = 0; i < 3; ++i) o[19 + i] = S.flow[i];
        if (ok && (fabsf((float)S.aff[0]) > 1.2f || fabsf((float)S.aff[1]) > 200.f)) ok = 2;   // :1243-1245: pose is still written, return false
        if (timed_out) ok = -1;
        for (int i = 0; i < 5; ++i) o[26 + i] = (double)S.evals_lvl[i];
        o[22] = (double)ok; o[23] = (double)S.evals; o[24] = (double)S.next_lvl; o[25] = (double)S.haveRepeated;
        __threadfence_system();
        __hip_atomic_store(&o[31], P.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
