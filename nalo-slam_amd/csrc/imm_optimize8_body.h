// The body of imm_optimize8_kernel (kernels_imm.hip), included once per kernel: NALO_IMM_OPT_COUNT is the number of points, a kernel argument for the staged and
// indexed calls and a word in device memory for nalo_imm_resident_activate. It is a textual include, not an inline function, so that the first kernel's
// machine code does not depend on the second's existence. ImmOptParams P is in scope.
    __shared__ double en_s[(NALO_MAX_WINDOW - 1) * kImmGroups], nen_s[(NALO_MAX_WINDOW - 1) * kImmGroups];
    const int l = threadIdx.x & 7, tid = threadIdx.x >> 3;                     // tid = group (point) inside the block
    const int p = blockIdx.x * kImmGroups + tid;
    if (p >= NALO_IMM_OPT_COUNT) return;
    double* en = en_s + tid; double* nen = nen_s + tid;
    const int q = P.sel ? P.sel[p] : p;                                        // where the point's inputs are; the outputs are indexed by p
    const int W = P.W, hf = P.host[q], nres = W - 1;
    const float color_l = P.color[(size_t)q * 8 + l], weight_l = P.weights[(size_t)q * 8 + l];
    const float u = P.u[q], v = P.v[q], energyTH = P.energyTH[q];
    unsigned st = 0, nst = 0;                                                  // state = IN (0) for every residual; newState = OUTLIER
    for (int i = 0; i < nres; ++i) { en[i * kImmGroups] = 0; nen[i * kImmGroups] = 0; nst |= (unsigned)IRS_OUTLIER << (2 * i); }
    if (l == 0) for (int t = 0; t < W; ++t) P.res_in[(size_t)p * W + t] = 0;
    if (l == 0) P.idepth_out[p] = NAN;
    auto tgt = [&](int i) { return i < hf ? i : i + 1; };                      // residual i <-> the i-th frame that is not the host
    float lastEnergy = 0, lastHdd = 0, lastbd = 0;
    float currentIdepth = (P.idmax[q] + P.idmin[q]) * 0.5f;
    for (int i = 0; i < nres; ++i) {
        // `float += double`: formed in double, rounded once (FullSystemOptPoint.cpp:79)
        lastEnergy = (float)((double)lastEnergy + imm_linearize8(P, hf, tgt(i), u, v, color_l, weight_l, l, energyTH, 1000.f, st, nst, en, nen, i, lastHdd, lastbd, currentIdepth));
        st = (st & ~(3u << (2 * i))) | (((nst >> (2 * i)) & 3u) << (2 * i));
        en[i * kImmGroups] = nen[i * kImmGroups];
    }
    if (!isfinite(lastEnergy) || lastHdd < kImmMinIdepthHAct) { if (l == 0) P.result[p] = 0; return; }
    float lambda = 0.1f;
    for (int it = 0; it < kImmGNItsActivation; ++it) {
        float H = lastHdd; H *= 1 + lambda;
        const float step = (float)((1.0 / (double)H) * (double)lastbd);        // `(1.0/H) * lastbd` is a double expression, :99
        const float newIdepth = currentIdepth - step;
        float newHdd = 0, newbd = 0, newEnergy = 0;
        for (int i = 0; i < nres; ++i)
            newEnergy = (float)((double)newEnergy + imm_linearize8(P, hf, tgt(i), u, v, color_l, weight_l, l, energyTH, 1.f, st, nst, en, nen, i, newHdd, newbd, newIdepth));
        if (!isfinite(lastEnergy) || newHdd < kImmMinIdepthHAct) { if (l == 0) P.result[p] = 0; return; }
        if (newEnergy < lastEnergy) {
            currentIdepth = newIdepth; lastHdd = newHdd; lastbd = newbd; lastEnergy = newEnergy;
            st = nst;
            for (int i = 0; i < nres; ++i) en[i * kImmGroups] = nen[i * kImmGroups];
            lambda *= 0.5f;
        } else lambda *= 5;
        if ((double)fabsf(step) < 0.0001 * (double)currentIdepth) break;
    }
    if (!isfinite(currentIdepth)) { if (l == 0) P.result[p] = -1; return; }
    int numGood = 0;
    for (int i = 0; i < nres; ++i) if (((st >> (2 * i)) & 3u) == IRS_IN) numGood++;
    if (numGood < P.minObs) { if (l == 0) P.result[p] = -1; return; }
    if (!isfinite(energyTH)) { if (l == 0) P.result[p] = -1; return; }                     // PointHessian inherits energyTH, :158
    if (l == 0) for (int i = 0; i < nres; ++i) if (((st >> (2 * i)) & 3u) == IRS_IN) P.res_in[(size_t)p * W + tgt(i)] = 1;
    if (l == 0) P.idepth_out[p] = currentIdepth;
    if (l == 0) P.result[p] = 1;
