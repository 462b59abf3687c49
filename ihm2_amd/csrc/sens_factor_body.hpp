// sens_factor_body.hpp -- the factorisation both sensitivities differentiate (formulas: top of kernels_sens.hip): the row gradients of the
// track rows and the a_lat row at xbar, rcoef, the row weights over the slot table (side_sigma), htilde, the backward Riccati sweep on Ht.
// A code fragment, not a header (no include guard, no namespace, no function of its own): sens_body (sens_body.hpp) and k_adj
// (kernels_adj.hip) #include it behind their LDS carve-up and early return, so that the compiler reads the same statements in both --
// as functions the pieces changed the register allocation of both kernels (NOTES.md R5.6).
//   Expects in scope: a (const SensArgs &), b, bs, lane, N, NS and the LDS pointers w, hc, ha, Kl, P, Al, Bl, Ht, PA, PB, Q.
//   Leaves in scope: linb, ra, rbv (both kernels' later sweeps), xo, uo (k_adj's weight gradients) and every other local, the lambdas
//   included: include it once per function body.
//   SENS_FACTOR_KEEP_QUU_INV(k, m, j, i0, i1): the includer's statement on the lanes < 16 of stage k, (i0, i1) = row m of Quu_k^-1.
#ifndef SENS_FACTOR_KEEP_QUU_INV
#error "define SENS_FACTOR_KEEP_QUU_INV (sens_body: empty, k_adj: the store of Quu_k^-1) before including sens_factor_body.hpp"
#endif
    const double *xb = a.xbar + bs * NS * 8, *ubb = a.ubar + bs * N * 2;
    const double *xo = a.x + bs * NS * 8, *uo = a.u + bs * N * 2;
    const double *lamb = a.lam + bs * NS * 28, *slkb = a.slk + bs * NS * 28;
    const double *lamab = a.lam_a + bs * NS * 2, *slkab = a.slk_a + bs * NS * 2;
    const double *linb = a.lin + bs * N * LIN_REC;
    const double *Hs0 = a.Hs + bs * a.hs_bs, *HsT = Hs0 + a.hs_te;
    const double *slb = a.slot_lb + bs * a.sl_bs, *sub = a.slot_ub + bs * a.sl_bs;

    // ---- row gradients of the nonlinear rows at xbar, zero weights ----
    double w_R = 0.0, w_L = 0.0;
    if (a.path) {
        const int trk = a.track_id[b];
        w_R = a.widths[trk * 2 + 0]; w_L = a.widths[trk * 2 + 1];
    }
    for (int k = lane; k < NS; k += 64) {
        // the track rows as the QP forms them (kernels_qp.hip: qp_wave_body), stages 1..N
        const double psi = xb[k * 8 + 2], sgn = (psi > 0.0) - (psi < 0.0);
        const double dfoot = -0.5 * a.car_L * cos(fabs(psi)) * sgn, dlat = -0.5 * a.car_W * sin(psi);
        hc[k * 2 + 0] = (a.path && k >= 1) ? dfoot + dlat : 0.0;
        hc[k * 2 + 1] = (a.path && k >= 1) ? -dfoot + dlat : 0.0;
        double g4[4] = {0.0, 0.0, 0.0, 0.0};
        if (a.alat && k >= 1 && k < N) ihm2::alat_eval(xb[k * 8 + 3], xb[k * 8 + 4], xb[k * 8 + 6], xb[k * 8 + 7], g4);
#pragma unroll
        for (int q = 0; q < 4; q++) ha[k * 4 + q] = g4[q];
    }
    for (int e = lane; e < NS * SENS_NR; e += 64) w[e] = 0.0;
    SSYNC();

    // coefficient of row c of stage k on the variable j of z_k = (dx_k, du_k)
    auto rcoef = [&](int k, int c, int j) -> double {
        if (c < 10) return (j == c) ? 1.0 : 0.0;
        if (c < 12) return a.CD[((size_t)k * 2 + (c - 10)) * 10 + j];
        if (c < 14) return (j == 1) ? ((c == 12) ? 1.0 : -1.0) : (j == 2) ? hc[k * 2 + (c - 12)] : 0.0;
        return (j == 3) ? ha[k * 4] : (j == 4) ? ha[k * 4 + 1] : (j == 6) ? ha[k * 4 + 2] : (j == 7) ? ha[k * 4 + 3] : 0.0;
    };

    // ---- row weights: every entry of the slot table on the lane that owns it in the QP (a split row's halves share a lane: no race) ----
    for (int s = lane; s < a.nslots; s += 64) {
        const int kc = a.slot_kc[s];
        if (kc < 0) continue;
        const int k = kc >> 4, c = kc & 15;
        // row value at xbar (as the QP forms it) and the row times the step
        double cz, rdz = 0.0;
        if (c < 8) cz = xb[k * 8 + c];
        else if (c < 10) cz = ubb[k * 2 + c - 8];
        else if (c == 14) {
            double g4[4];
            cz = ihm2::alat_eval(xb[k * 8 + 3], xb[k * 8 + 4], xb[k * 8 + 6], xb[k * 8 + 7], g4);
        } else if (c >= 12) {
            const double n = xb[k * 8 + 1], psi = xb[k * 8 + 2];
            const double foot = -0.5 * a.car_L * sin(fabs(psi)), lat = 0.5 * a.car_W * cos(psi);
            cz = (c == 12) ? n + foot + lat - w_R : -n - foot + lat - w_L;
        } else {
            cz = 0.0;
            for (int j = 0; j < 8; j++) cz = fma(a.CD[((size_t)k * 2 + (c - 10)) * 10 + j], xb[k * 8 + j], cz);
            cz = fma(a.CD[((size_t)k * 2 + (c - 10)) * 10 + 8], ubb[k * 2 + 0], cz);
            cz = fma(a.CD[((size_t)k * 2 + (c - 10)) * 10 + 9], ubb[k * 2 + 1], cz);
        }
        for (int j = 0; j < 10; j++) {
            const double dzj = (j < 8) ? xo[k * 8 + j] - xb[k * 8 + j] : (k < N) ? uo[k * 2 + j - 8] - ubb[k * 2 + j - 8] : 0.0;
            rdz = fma(rcoef(k, c, j), dzj, rdz);
        }
        const double lb = slb[s], ub = sub[s], zw = a.slot_zw[s], Zw = a.slot_Zw[s];
        const bool soft = Zw >= 0.0;
        double sig = 0.0;
        if (sfin(lb)) {
            const double lm = (c == 14) ? lamab[k * 2] : lamb[k * 28 + c];
            const double sl = soft ? ((c == 14) ? slkab[k * 2] : slkb[k * 28 + c]) : 0.0;
            sig += side_sigma(lm, rdz - (lb - cz) + sl, sl, zw, Zw, a.tau);
        }
        if (sfin(ub)) {
            const double lm = (c == 14) ? lamab[k * 2 + 1] : lamb[k * 28 + 14 + c];
            const double sl = soft ? ((c == 14) ? slkab[k * 2 + 1] : slkb[k * 28 + 14 + c]) : 0.0;
            sig += side_sigma(lm, (ub - cz) - rdz + sl, sl, zw, Zw, a.tau);
        }
        w[k * SENS_NR + c] += sig;
    }
    SSYNC();

    // entry (i, j) of Ht_k = H_k + sum_c w_c r_c r_c'
    auto htilde = [&](int k, int i, int j) -> double {
        const double *Hk = (k == N) ? HsT : Hs0 + (size_t)k * a.hs_ks;
        double v = Hk[i * 10 + j];
        const int cmax = (k == N) ? 8 : 10;       // terminal stage: no input rows; general rows only for k < N
        if (i == j && i < cmax) v += w[k * SENS_NR + i];
        if (k < N)
            for (int c = 10; c < 12; c++) v = fma(w[k * SENS_NR + c] * rcoef(k, c, i), rcoef(k, c, j), v);
        for (int c = 12; c < SENS_NR; c++) {
            const double wc = w[k * SENS_NR + c];
            if (wc != 0.0) v = fma(wc * rcoef(k, c, i), rcoef(k, c, j), v);
        }
        return v;
    };

    // ---- backward Riccati sweep on Ht: P_N = Ht_N[x,x]; K_k = -Quu^-1 Qux, P_k = Qxx + Qux' K_k ----
    {
        const int i = lane >> 3, j = lane & 7;
        P[lane] = htilde(N, i, j);
    }
    // the record of stage k is fetched one stage ahead, into registers
    double ra = linb[(size_t)(N - 1) * LIN_REC + lane], rbv = (lane < 16) ? linb[(size_t)(N - 1) * LIN_REC + 64 + lane] : 0.0;
    for (int k = N - 1; k >= 0; k--) {
        Al[lane] = ra;
        if (lane < 16) Bl[lane] = rbv;
        if (k > 0) {
            ra = linb[(size_t)(k - 1) * LIN_REC + lane];
            if (lane < 16) rbv = linb[(size_t)(k - 1) * LIN_REC + 64 + lane];
        }
        for (int e = lane; e < 100; e += 64) Ht[e] = htilde(k, e / 10, e % 10);
        SSYNC();
        {
            const int i = lane >> 3, j = lane & 7;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < 8; l++) acc = fma(P[i * 8 + l], Al[l * 8 + j], acc);
            PA[lane] = acc;
            if (lane < 16) {
                const int ii = lane >> 1, m = lane & 1;
                double accb = 0.0;
#pragma unroll
                for (int l = 0; l < 8; l++) accb = fma(P[ii * 8 + l], Bl[l * 2 + m], accb);
                PB[lane] = accb;
            }
        }
        SSYNC();
        {
            const int i = lane >> 3, j = lane & 7;
            double acc = Ht[i * 10 + j];
#pragma unroll
            for (int l = 0; l < 8; l++) acc = fma(Al[l * 8 + i], PA[l * 8 + j], acc);
            Q[lane] = acc;
            if (lane < 16) {        // Qux (m, j)
                const int m = lane >> 3, jj = lane & 7;
                double q = Ht[(8 + m) * 10 + jj];
#pragma unroll
                for (int l = 0; l < 8; l++) q = fma(Bl[l * 2 + m], PA[l * 8 + jj], q);
                Q[64 + lane] = q;
            } else if (lane < 20) {  // Quu (m, n)
                const int m = (lane - 16) >> 1, n = (lane - 16) & 1;
                double q = Ht[(8 + m) * 10 + 8 + n];
#pragma unroll
                for (int l = 0; l < 8; l++) q = fma(Bl[l * 2 + m], PB[l * 2 + n], q);
                Q[80 + (lane - 16)] = q;
            }
        }
        SSYNC();
        if (lane < 16) {
            const int m = lane >> 3, j = lane & 7;
            const double q00 = Q[80], q01 = 0.5 * (Q[81] + Q[82]), q11 = Q[83];
            const double idet = 1.0 / (q00 * q11 - q01 * q01);
            const double i0 = (m == 0) ? q11 * idet : -q01 * idet, i1 = (m == 0) ? -q01 * idet : q00 * idet;
            Kl[k * 16 + lane] = -(i0 * Q[64 + j] + i1 * Q[72 + j]);
            SENS_FACTOR_KEEP_QUU_INV(k, m, j, i0, i1);
        }
        SSYNC();
        {
            const int i = lane >> 3, j = lane & 7;
            const double *K = Kl + k * 16;
            const double pij = Q[i * 8 + j] + Q[64 + i] * K[j] + Q[72 + i] * K[8 + j];
            const double pji = Q[j * 8 + i] + Q[64 + j] * K[i] + Q[72 + j] * K[8 + i];
            P[lane] = 0.5 * (pij + pji);
        }
        SSYNC();
    }
