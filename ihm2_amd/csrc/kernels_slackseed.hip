// kernels_slackseed.hip -- adjoint seeds on the soft slacks: a seed c_i = dL/ds_i on the slack of a soft side is carried onto the stage
// variables before k_adj runs (ihm2mpc_eval_adjoint_sensitivities_s, ihm2mpc_eval_cost_gradient_soft; DESIGN.md §4 "seeds on the slacks").
//
// k_sens and k_adj (kernels_sens.hip, kernels_adj.hip) differentiate the system in which every soft slack is eliminated in series
// (sens_body.hpp: side_sigma).  With the slack kept as a variable its row reads (lam_i / t_i) (s + sgn_i r_i z) + rho_i s = c_i; eliminating
// it leaves Ht as k_sens forms it and moves the right-hand side:
//   seed_z,k  <-  seed_z,k - sum over the soft sides i of stage k with lam_i > 0 of  c_i gamma_i sgn_i r_i,
//   gamma_i = lam_i / (t_i rho_i + lam_i)  (sens_body.hpp: side_slack_share),  sgn_i = +1 on a lower and -1 on an upper side
// -- gamma_i = sigma_i / rho_i is the share of a row move that the slack takes (1 for rho_i = 0, 0 for lam_i = 0).  Everything behind
// the fold is k_adj, unchanged.  For the cost (COST) c_i = dJ_slack / ds_i = z_i + Z_i s_i, from the penalties and slacks themselves.
//
// Mapping: one wavefront per instance.  Phase 1 runs over the slot table exactly as the row-weight phase of sens_factor_body.hpp does
// (s = lane, lane + 64, ..: a split row's halves are on one lane) and writes gamma_i of every soft side into one LDS table (NS, 30):
// 14 lower sides, 14 upper sides, the two sides of the lateral-acceleration row.  The row gradients at xbar (hc, ha), rcoef and the row
// evaluation of a slot mirror that fragment statement by statement; the fragment itself is not included, since it carries the Riccati
// sweep.  Phase 2, per seed: the lane owns the entries (k, j) of seed_z with k * 10 + j = lane, lane + 64, .. and subtracts
// sum_c rcoef(k, c, j) (c_lower gamma_lower - c_upper gamma_upper) in ascending c -- one read-modify-write per entry, no atomics, the
// same bits whatever the batch.  Instances whose status is neither 0 nor 2 are skipped (k_adj writes NaN gradients for them).  fp64.
#include <cmath>

#include "ihm2mpc_internal.h"
#include "sens_body.hpp"

namespace {

#define FOLD_SIDES 30   // per stage: lower sides of the rows 0..13, their upper sides, the lower and the upper side of the a_lat row

struct FoldArgs {
    SensArgs s;                         // k_sens' block (sens_u0, sens_x, sens_u, hist unused)
    int n_seeds;                        // 1..8 (COST: 1)
    const double *seed_s, *seed_sa;     // (B,n_seeds,N+1,28), (B,n_seeds,N+1,2) dL/ds; nullptr = zero (COST: not read)
    double *seed_x, *seed_u;            // (B,n_seeds,N+1,8), (B,n_seeds,N,2) dL/dz, folded in place
};

// LDS of one instance (doubles): hc (NS*2) | ha (NS*4) | gamma (NS*30) | COST: c (NS*30)
__host__ __device__ constexpr size_t fold_lds_doubles(size_t N, bool cost) { return (N + 1) * (6 + FOLD_SIDES * (cost ? 2 : 1)); }
static_assert(fold_lds_doubles(40, false) * sizeof(double) == 11808 && fold_lds_doubles(40, true) * sizeof(double) == 21648,
              "k_slack_fold: launch LDS at N = 40");

// COST: the coefficients are dJ_slack/ds_i = z_i + Z_i s_i (one seed) instead of seed_s / seed_sa
template <bool COST>
__global__ __launch_bounds__(64) void k_slack_fold(FoldArgs fa)
{
    extern __shared__ double sm[];
    const SensArgs &a = fa.s;
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int st = a.status[b];
    if (st != 0 && st != 2) return;     // no solution to differentiate (wave-uniform): the seeds stay as they came
    const int lane = threadIdx.x;
    const int N = a.N, NS = N + 1, S = COST ? 1 : fa.n_seeds;
    double *hc = sm;                    // NS*2   d h_R / d psi, d h_L / d psi of the track rows at xbar
    double *ha = hc + NS * 2;           // NS*4   d a_lat / d (v_x, v_y, T, delta) at xbar
    double *gam = ha + NS * 4;          // NS*30  gamma_i of the soft sides, 0 elsewhere
    double *cof = gam + NS * FOLD_SIDES;    // NS*30  COST: c_i of the same sides

    const size_t bs = (size_t)b;
    const double *xb = a.xbar + bs * NS * 8, *ubb = a.ubar + bs * N * 2;
    const double *xo = a.x + bs * NS * 8, *uo = a.u + bs * N * 2;
    const double *lamb = a.lam + bs * NS * 28, *slkb = a.slk + bs * NS * 28;
    const double *lamab = a.lam_a + bs * NS * 2, *slkab = a.slk_a + bs * NS * 2;
    const double *slb = a.slot_lb + bs * a.sl_bs, *sub = a.slot_ub + bs * a.sl_bs;

    // ---- row gradients of the nonlinear rows at xbar (sens_factor_body.hpp), the table zeroed ----
    double w_R = 0.0, w_L = 0.0;
    if (a.path) {
        const int trk = a.track_id[b];
        w_R = a.widths[trk * 2 + 0]; w_L = a.widths[trk * 2 + 1];
    }
    for (int k = lane; k < NS; k += 64) {
        const double psi = xb[k * 8 + 2], sgn = (psi > 0.0) - (psi < 0.0);
        const double dfoot = -0.5 * a.car_L * cos(fabs(psi)) * sgn, dlat = -0.5 * a.car_W * sin(psi);
        hc[k * 2 + 0] = (a.path && k >= 1) ? dfoot + dlat : 0.0;
        hc[k * 2 + 1] = (a.path && k >= 1) ? -dfoot + dlat : 0.0;
        double g4[4] = {0.0, 0.0, 0.0, 0.0};
        if (a.alat && k >= 1 && k < N) ihm2::alat_eval(xb[k * 8 + 3], xb[k * 8 + 4], xb[k * 8 + 6], xb[k * 8 + 7], g4);
#pragma unroll
        for (int q = 0; q < 4; q++) ha[k * 4 + q] = g4[q];
    }
    for (int e = lane; e < NS * FOLD_SIDES; e += 64) gam[e] = 0.0;
    WSYNC();

    // coefficient of row c of stage k on the variable j of z_k = (dx_k, du_k)
    auto rcoef = [&](int k, int c, int j) -> double {
        if (c < 10) return (j == c) ? 1.0 : 0.0;
        if (c < 12) return a.CD[((size_t)k * 2 + (c - 10)) * 10 + j];
        if (c < 14) return (j == 1) ? ((c == 12) ? 1.0 : -1.0) : (j == 2) ? hc[k * 2 + (c - 12)] : 0.0;
        return (j == 3) ? ha[k * 4] : (j == 4) ? ha[k * 4 + 1] : (j == 6) ? ha[k * 4 + 2] : (j == 7) ? ha[k * 4 + 3] : 0.0;
    };

    // ======== phase 1: gamma of every soft side, each entry of the slot table on the lane that owns it in the QP ========
    for (int s = lane; s < a.nslots; s += 64) {
        const int kc = a.slot_kc[s];
        if (kc < 0) continue;
        const double zw = a.slot_zw[s], Zw = a.slot_Zw[s];
        if (!(Zw >= 0.0)) continue;         // a hard slot: no slack
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
        const double lb = slb[s], ub = sub[s];
        if (sfin(lb)) {
            const double lm = (c == 14) ? lamab[k * 2] : lamb[k * 28 + c];
            const double sl = (c == 14) ? slkab[k * 2] : slkb[k * 28 + c];
            const int e = k * FOLD_SIDES + ((c == 14) ? 28 : c);
            gam[e] = side_slack_share(lm, rdz - (lb - cz) + sl, sl, zw, Zw, a.tau);
            if (COST) cof[e] = fma(Zw, sl, zw);
        }
        if (sfin(ub)) {
            const double lm = (c == 14) ? lamab[k * 2 + 1] : lamb[k * 28 + 14 + c];
            const double sl = (c == 14) ? slkab[k * 2 + 1] : slkb[k * 28 + 14 + c];
            const int e = k * FOLD_SIDES + ((c == 14) ? 29 : 14 + c);
            gam[e] = side_slack_share(lm, (ub - cz) - rdz + sl, sl, zw, Zw, a.tau);
            if (COST) cof[e] = fma(Zw, sl, zw);
        }
    }
    WSYNC();

    // ======== phase 2: the fold, one read-modify-write per entry of seed_z and per seed ========
    for (int q = 0; q < S; q++) {
        double *sx = fa.seed_x + (bs * S + q) * NS * 8, *su = fa.seed_u + (bs * S + q) * N * 2;
        const double *ss = (!COST && fa.seed_s) ? fa.seed_s + (bs * S + q) * NS * 28 : nullptr;
        const double *sa = (!COST && fa.seed_sa) ? fa.seed_sa + (bs * S + q) * NS * 2 : nullptr;
        // sum over the two sides of row c of sgn c gamma, lower before upper; a side without a slack (gamma = 0) is not read
        auto share = [&](int k, int c) -> double {
            const int lo = k * FOLD_SIDES + ((c == 14) ? 28 : c), up = k * FOLD_SIDES + ((c == 14) ? 29 : 14 + c);
            const double gl = gam[lo], gu = gam[up];
            double t = 0.0;
            if (gl != 0.0) {
                const double cl = COST ? cof[lo] : (c == 14) ? (sa ? sa[k * 2] : 0.0) : (ss ? ss[k * 28 + c] : 0.0);
                t = cl * gl;
            }
            if (gu != 0.0) {
                const double cu = COST ? cof[up] : (c == 14) ? (sa ? sa[k * 2 + 1] : 0.0) : (ss ? ss[k * 28 + 14 + c] : 0.0);
                t = fma(-cu, gu, t);
            }
            return t;
        };
        for (int e = lane; e < N * 10 + 8; e += 64) {
            const int k = e / 10, j = e - k * 10;
            double acc = 0.0;
            for (int c = 0; c < SENS_NR; c++) {
                if (c < 10 && c != j) continue;             // a box acts on its own variable
                if (c >= 10 && c < 12 && k >= N) continue;  // general rows: stages k < N
                const double r = rcoef(k, c, j);
                if (r == 0.0) continue;
                acc = fma(r, share(k, c), acc);
            }
            double *p = (j < 8) ? sx + k * 8 + j : su + k * 2 + (j - 8);
            *p = *p - acc;
        }
    }
}

}  // namespace

// The fold of the handle on h->stream: seed_x (B,n_seeds,NS,8), seed_u (B,n_seeds,N,2) in device memory are folded in place.  cost: the
// coefficients of the cost's slack terms (n_seeds = 1, seed_s / seed_sa not read); otherwise seed_s (B,n_seeds,NS,28) and seed_sa
// (B,n_seeds,NS,2) in device memory, either may be nullptr = zero.
void ihm2_launch_slack_fold(ihm2mpc_handle *h, int cost, int n_seeds, const double *seed_s, const double *seed_sa, double *seed_x, double *seed_u)
{
    FoldArgs a;
    ihm2_sens_args(h, &a.s);
    a.n_seeds = cost ? 1 : n_seeds;
    a.seed_s = seed_s; a.seed_sa = seed_sa; a.seed_x = seed_x; a.seed_u = seed_u;
    const size_t lds = sizeof(double) * fold_lds_doubles((size_t)h->N, cost != 0);
    if (cost) {
        (void)hipFuncSetAttribute((const void *)k_slack_fold<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_slack_fold<true>, dim3(h->B), dim3(64), lds, h->stream, a);
    } else {
        (void)hipFuncSetAttribute((const void *)k_slack_fold<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_slack_fold<false>, dim3(h->B), dim3(64), lds, h->stream, a);
    }
}
