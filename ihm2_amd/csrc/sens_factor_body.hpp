// sens_factor_body.hpp -- the factorisation both sensitivities differentiate (formulas: top of kernels_sens.hip): the row weights over the
// slot table (side_sigma) on the constraint rows at xbar, htilde, the backward Riccati sweep on Ht.  The rows themselves -- their gradients
// at xbar, rcoef, the walk over the slot table -- are the fragment sens_rows_body.hpp, included here with the hooks that form the weights.
// A code fragment, not a header (no include guard, no namespace, no function of its own): sens_body (sens_body.hpp) and k_adj
// (kernels_adj.hip) #include it behind their LDS carve-up and early return, so that the compiler reads the same statements in both --
// as functions the pieces changed the register allocation of both kernels (NOTES.md R5.6).
//   Expects in scope: a (const SensArgs &), b, bs, lane, N, NS and the LDS pointers w, hc, ha, Kl, P, Al, Bl, Ht, PA, PB, Q.
//   Leaves in scope: linb, ra, rbv (both kernels' later sweeps), xo, uo (k_adj's weight gradients) and every other local, the lambdas
//   and what sens_rows_body.hpp leaves included: include it once per function body.
//   SENS_FACTOR_KEEP_QUU_INV(k, m, j, i0, i1): the includer's statement on the lanes < 16 of stage k, (i0, i1) = row m of Quu_k^-1.
#ifndef SENS_FACTOR_KEEP_QUU_INV
#error "define SENS_FACTOR_KEEP_QUU_INV (sens_body: empty, k_adj: the store of Quu_k^-1) before including sens_factor_body.hpp"
#endif
    const double *linb = a.lin + bs * N * LIN_REC;
    const double *Hs0 = a.Hs + bs * a.hs_bs, *HsT = Hs0 + a.hs_te;

    // ---- row weights w = sigma_lower + sigma_upper of every row: a hard side (Zw < 0) has no slack, and its slk is not read ----
#define SENS_ROWS_CLEAR for (int e = lane; e < NS * SENS_NR; e += 64) w[e] = 0.0;
#define SENS_ROWS_SLOT_OPEN(s)
#define SENS_ROWS_SLOT_BEGIN(s)                            \
        const double zw = SENS_ROWS_ZW(s), Zw = SENS_ROWS_ZZ(s); \
        const bool soft = Zw >= 0.0;                       \
        double sig = 0.0;
#define SENS_ROWS_SIDE(k, c, up, LM, GAP, SL)              \
            const double lm = LM;                          \
            const double sl = soft ? (SL) : 0.0;           \
            sig += side_sigma(lm, GAP + sl, sl, zw, Zw, a.tau);
#define SENS_ROWS_SLOT_END(k, c) w[k * SENS_NR + c] += sig;
#include "sens_rows_body.hpp"
#undef SENS_ROWS_CLEAR
#undef SENS_ROWS_SLOT_OPEN
#undef SENS_ROWS_SLOT_BEGIN
#undef SENS_ROWS_SIDE
#undef SENS_ROWS_SLOT_END

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
