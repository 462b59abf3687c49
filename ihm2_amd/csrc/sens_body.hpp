// sens_body.hpp -- the body of the x0-sensitivity kernel (kernels_sens.hip: k_sens, one launch after the QP), shared with the persistent
// loop (kernels_qp.hip: k_steps<..., SENS = 1>, after every step's QP).  The formulas and the mapping are described at the top of
// kernels_sens.hip; the argument block SensArgs is declared in ihm2mpc_internal.h.
#pragma once

#include <cmath>

#include "ihm2mpc_internal.h"
#include "model.hpp"
#include "qp_lds.hpp"
#include "wave_sync.hpp"

namespace {

#define SENS_INF 1e20
#define SENS_NR 15      // rows per stage: 8 state boxes, 2 input boxes, 2 general rows, 2 track rows, the lateral-acceleration row
// the LDS of the factorisation and of the whole body in doubles: qp_lds.hpp, where the launches' sizes are chosen
static_assert(SENS_NR == ihm2::SENS_ROWS, "sens_factor_lds_doubles counts other rows than the carve-up");
using ihm2::sens_factor_lds_doubles;

#define SSYNC() WSYNC()      // (the name the 14 hand-offs of sens_body, sens_factor_body.hpp and kernels_adj.hip were written with)

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

// t and rho of one soft side (arguments as side_sigma's, Zw >= 0, lm > 0), as side_sigma forms them
__device__ __forceinline__ void side_slack_terms(double lm, double gap, double sl, double zw, double Zw, double tau, double &t, double &rho)
{
    t = fmax(gap, tau);
    const double nu = fmax(zw + Zw * sl - lm, 0.0);
    rho = Zw + nu / fmax(sl, tau);
}

// gamma of one soft side (arguments as side_sigma's, Zw >= 0): the share sigma / rho of a move of the row that its slack takes, which is what
// carries a seed on the slack onto the stage variables (kernels_slackseed.hip)
__device__ __forceinline__ double side_slack_share(double lm, double gap, double sl, double zw, double Zw, double tau)
{
    if (!(lm > 0.0)) return 0.0;
    double t, rho;
    side_slack_terms(lm, gap, sl, zw, Zw, tau, t, rho);
    return lm / (t * rho + lm);                // finite for rho = 0, where it is 1
}

// The sides of one stage as the tables of k_slack_fold and k_penalty_grad hold them (kernels_slackseed.hip, kernels_penaltygrad.hip):
// the layout of lam / slk -- the lower sides of the rows 0..13, then their upper sides -- and behind it the lower and the upper side of
// the lateral-acceleration row (lam_a / slk_a).
#define SENS_SIDES 30
__device__ __forceinline__ int sens_side(int c, bool upper) { return upper ? ((c == 14) ? 29 : 14 + c) : ((c == 14) ? 28 : c); }
// ... and back: the row of side o, and whether o is its upper side
__device__ __forceinline__ int sens_side_row(int o) { return (o >= 28) ? 14 : (o < 14) ? o : o - 14; }
__device__ __forceinline__ bool sens_side_upper(int o) { return (o >= 28) ? o == 29 : o >= 14; }

// The body of k_sens for instance b on the calling wavefront (lane = threadIdx.x), sm the block's dynamic LDS (written before it is
// read).  step: the control step of the persistent loop (k_sens: 0) -- the row of a.hist it writes, and the forward sweep of mode 2 runs
// on a.sweep_step only.  Not inlined: k_sens and k_steps<..., SENS = 1> run the same code, whatever their translation units contract.
__device__ __noinline__ void sens_body(const SensArgs &a, const int b, double *sm, const int step)
{
    const int lane = threadIdx.x;
    const int N = a.N, NS = N + 1;
    // ---- LDS carve-up (doubles): w .. Q as in k_adj (kernels_adj.hip), sens_factor_lds_doubles of them ----
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
#define SENS_FACTOR_KEEP_QUU_INV(k, m, j, i0, i1)
#include "sens_factor_body.hpp"
#undef SENS_FACTOR_KEEP_QUU_INV
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
