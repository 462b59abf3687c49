// sens_body.hpp -- the body of the x0-sensitivity kernel (kernels_sens.hip: k_sens, one launch after the QP), shared with the persistent
// loop (kernels_qp.hip: k_steps<..., SENS = 1>, after every step's QP).  The formulas and the mapping are described at the top of
// kernels_sens.hip; the argument block SensArgs is declared in ihm2mpc_internal.h.
#pragma once

#include <cmath>

#include "ihm2mpc_internal.h"
#include "model.hpp"

namespace {

#define SENS_INF 1e20
#define SENS_NR 15      // rows per stage: 8 state boxes, 2 input boxes, 2 general rows, 2 track rows, the lateral-acceleration row

// one wavefront: a hand-off through LDS needs a compiler fence, no s_barrier (kernels_qp.hip: WSYNC)
#define SSYNC()                                                  \
    do {                                                         \
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   \
        __builtin_amdgcn_wave_barrier();                         \
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   \
    } while (0)

__device__ __forceinline__ bool sfin(double v) { return fabs(v) < SENS_INF; }

// sigma of one side: lm its multiplier, gap its primal gap (slack included), sl the slack, zw / Zw its penalties (Zw < 0: hard)
__device__ __forceinline__ double side_sigma(double lm, double gap, double sl, double zw, double Zw, double tau)
{
    if (!(lm > 0.0)) return 0.0;
    const double t = fmax(gap, tau);
    if (Zw < 0.0) return lm / t;
    const double nu = fmax(zw + Zw * sl - lm, 0.0);
    const double rho = Zw + nu / fmax(sl, tau);
    return lm * rho / (t * rho + lm);          // 1 / (t / lm + 1 / rho), finite for rho = 0
}

// The body of k_sens for instance b on the calling wavefront (lane = threadIdx.x), sm the block's dynamic LDS (written before it is
// read).  step: the control step of the persistent loop (k_sens: 0) -- the row of a.hist it writes, and the forward sweep of mode 2 runs
// on a.sweep_step only.  Not inlined: k_sens and k_steps<..., SENS = 1> run the same code, whatever their translation units contract.
__device__ __noinline__ void sens_body(const SensArgs &a, const int b, double *sm, const int step)
{
    const int lane = threadIdx.x;
    const int N = a.N, NS = N + 1;
    // ---- LDS carve-up (doubles) ----
    double *w = sm;                  // NS*15  row weights sigma_lower + sigma_upper
    double *hc = w + NS * SENS_NR;   // NS*2   d h_R / d psi, d h_L / d psi of the track rows at xbar
    double *ha = hc + NS * 2;        // NS*4   d a_lat / d (v_x, v_y, T, delta) at xbar
    double *Kl = ha + NS * 4;        // N*16   gains K_k (du = K_k dx)
    double *P = Kl + N * 16;         // 64
    double *Al = P + 64;             // 64
    double *Bl = Al + 64;            // 16
    double *Ht = Bl + 16;            // 100
    double *PA = Ht + 100;           // 64
    double *PB = PA + 64;            // 16
    double *Q = PB + 16;             // 84: Qxx (64) | Qux (16) | Quu (4)
    double *X = Q + 84;              // 64  forward sweep: dX_k
    double *U = X + 64;              // 16  forward sweep: dU_k

    const size_t bs = (size_t)b;
    const int st = a.status[b];
    const bool sweep = a.mode == 2 && step == a.sweep_step;
    double *krow = a.hist ? a.hist + ((size_t)step * a.B + bs) * 16 : nullptr;
    if (st != 0 && st != 2) {        // no solution to differentiate (wave-uniform)
        if (lane < 16) {
            a.sens_u0[bs * 16 + lane] = NAN;
            if (krow) krow[lane] = NAN;
        }
        if (sweep) {
            for (int e = lane; e < NS * 64; e += 64) a.sens_x[bs * NS * 64 + e] = NAN;
            for (int e = lane; e < N * 16; e += 64) a.sens_u[bs * N * 16 + e] = NAN;
        }
        return;
    }
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
    if (lane < 16) {
        a.sens_u0[bs * 16 + lane] = Kl[lane];
        if (krow) krow[lane] = Kl[lane];
    }
    if (!sweep) return;

    // ---- forward sweep: dX_0 = I, dU_k = K_k dX_k, dX_{k+1} = A_k dX_k + B_k dU_k ----
    double *sx = a.sens_x + bs * NS * 64, *su = a.sens_u + bs * N * 16;
    {
        const int i = lane >> 3, j = lane & 7;
        X[lane] = (i == j) ? 1.0 : 0.0;
        sx[lane] = X[lane];
    }
    ra = linb[lane]; rbv = (lane < 16) ? linb[64 + lane] : 0.0;
    for (int k = 0; k < N; k++) {
        Al[lane] = ra;
        if (lane < 16) Bl[lane] = rbv;
        if (k + 1 < N) {
            ra = linb[(size_t)(k + 1) * LIN_REC + lane];
            if (lane < 16) rbv = linb[(size_t)(k + 1) * LIN_REC + 64 + lane];
        }
        if (lane < 16) {
            const int m = lane >> 3, j = lane & 7;
            const double *K = Kl + k * 16;
            double acc = 0.0;
#pragma unroll
            for (int l = 0; l < 8; l++) acc = fma(K[m * 8 + l], X[l * 8 + j], acc);
            U[lane] = acc;
            su[k * 16 + lane] = acc;
        }
        SSYNC();
        const int i = lane >> 3, j = lane & 7;
        double acc = 0.0;
#pragma unroll
        for (int l = 0; l < 8; l++) acc = fma(Al[i * 8 + l], X[l * 8 + j], acc);
        acc = fma(Bl[i * 2 + 0], U[j], acc);
        acc = fma(Bl[i * 2 + 1], U[8 + j], acc);
        SSYNC();
        X[lane] = acc;
        sx[(k + 1) * 64 + lane] = acc;
        SSYNC();
    }
}

}  // namespace
