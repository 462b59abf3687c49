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
// Mapping: one wavefront per instance.  Phase 1 is the fragment sens_rows_body.hpp, the text k_sens and k_adj take their rows from: the row
// gradients at xbar (hc, ha), rcoef and the walk over the slot table (s = lane, lane + 64, ..: a split row's halves are on one lane), with
// hooks that skip the hard slots and write gamma_i of every soft side into one LDS table (NS, SENS_SIDES) (sens_body.hpp: sens_side).
// Phase 2, per seed: the lane owns the entries (k, j) of seed_z with k * 10 + j = lane, lane + 64, .. and subtracts
// sum_c rcoef(k, c, j) (c_lower gamma_lower - c_upper gamma_upper) in ascending c -- one read-modify-write per entry, no atomics, the
// same bits whatever the batch.  Instances whose status is neither 0 nor 2 are skipped (k_adj writes NaN gradients for them).  fp64.
#include <cmath>

#include "ihm2mpc_internal.h"
#include "sens_body.hpp"

namespace {

struct FoldArgs {
    SensArgs s;                         // k_sens' block (sens_u0, sens_x, sens_u, hist unused)
    int n_seeds;                        // 1..8 (COST: 1)
    const double *seed_s, *seed_sa;     // (B,n_seeds,N+1,28), (B,n_seeds,N+1,2) dL/ds; nullptr = zero (COST: not read)
    double *seed_x, *seed_u;            // (B,n_seeds,N+1,8), (B,n_seeds,N,2) dL/dz, folded in place
};

// LDS of one instance (doubles): hc (NS*2) | ha (NS*4) | gamma (NS*30) | COST: c (NS*30)
__host__ __device__ constexpr size_t fold_lds_doubles(size_t N, bool cost) { return (N + 1) * (6 + SENS_SIDES * (cost ? 2 : 1)); }
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
    double *cof = gam + NS * SENS_SIDES;    // NS*30  COST: c_i of the same sides

    const size_t bs = (size_t)b;

    // ======== phase 1: the rows at xbar (sens_rows_body.hpp); gamma of every soft side, 0 elsewhere ========
#define SENS_ROWS_CLEAR for (int e = lane; e < NS * SENS_SIDES; e += 64) gam[e] = 0.0;
#define SENS_ROWS_SLOT_OPEN(s)                             \
        const double zw = SENS_ROWS_ZW(s), Zw = SENS_ROWS_ZZ(s); \
        if (!(Zw >= 0.0)) continue;         // a hard slot: no slack
#define SENS_ROWS_SLOT_BEGIN(s)
#define SENS_ROWS_SIDE(k, c, up, LM, GAP, SL)              \
            const double lm = LM;                          \
            const double sl = SL;                          \
            const int e = k * SENS_SIDES + sens_side(c, up); \
            gam[e] = side_slack_share(lm, GAP + sl, sl, zw, Zw, a.tau); \
            if (COST) cof[e] = fma(Zw, sl, zw);
#define SENS_ROWS_SLOT_END(k, c)
#include "sens_rows_body.hpp"
#undef SENS_ROWS_CLEAR
#undef SENS_ROWS_SLOT_OPEN
#undef SENS_ROWS_SLOT_BEGIN
#undef SENS_ROWS_SIDE
#undef SENS_ROWS_SLOT_END

    // ======== phase 2: the fold, one read-modify-write per entry of seed_z and per seed ========
    for (int q = 0; q < S; q++) {
        double *sx = fa.seed_x + (bs * S + q) * NS * 8, *su = fa.seed_u + (bs * S + q) * N * 2;
        const double *ss = (!COST && fa.seed_s) ? fa.seed_s + (bs * S + q) * NS * 28 : nullptr;
        const double *sa = (!COST && fa.seed_sa) ? fa.seed_sa + (bs * S + q) * NS * 2 : nullptr;
        // sum over the two sides of row c of sgn c gamma, lower before upper; a side without a slack (gamma = 0) is not read
        auto share = [&](int k, int c) -> double {
            const int lo = k * SENS_SIDES + sens_side(c, false), up = k * SENS_SIDES + sens_side(c, true);
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
