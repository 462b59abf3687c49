// kernels_penaltygrad.hip -- adjoint gradients in the slack penalties z_i, Z_i of the soft sides (ihm2mpc_set_soft and the two pairs of the
// lateral-acceleration row): ihm2mpc_eval_adjoint_sensitivities_p, ihm2mpc_eval_cost_gradient_penalties; DESIGN.md §4 "gradients in the
// soft penalties".
//
// With the slack of a soft side i of row r_i at stage k kept as a variable, its row of the differentiated system reads
//   w_i (s + sgn_i r_i z) + rho_i s = c_i,   w_i = lam_i / t_i,  t_i = max(gap_i, tau),  nu_i = max(z_i + Z_i s_i - lam_i, 0),
//   rho_i = Z_i + nu_i / max(s_i, tau),  sgn_i = +1 on a lower and -1 on an upper side,  c_i = dL/ds_i
// (kernels_slackseed.hip).  It linearises the slack's stationarity z_i + Z_i s_i - lam_i - nu_i = 0, which a change of the penalties moves
// by dz_i + s_i dZ_i; with [zeta_z; zeta_s; nu] = M^-1 [seed_z; c; 0] and dL = -zeta' dg
//   zeta_s,i = (c_i - w_i sgn_i r_i zeta_k) / (w_i + rho_i) = (c_i t_i - lam_i sgn_i r_i zeta_k) / (t_i rho_i + lam_i),
//   dL/dz_i = -zeta_s,i,   dL/dZ_i = -s_i zeta_s,i.
// The second form is evaluated: its denominator is side_slack_share's (sens_body.hpp) and w_i, up to 1e13, never appears.  zeta_k is the
// adjoint solution of stage k on the folded seeds, which k_adj<true, true> (kernels_adj.hip) stores.  A side with !(lam_i > 0) is
// dropped as side_sigma and side_slack_share drop it: both gradients 0 (there rho_i >= nu_i / tau, so the dropped zeta_s is at most
// |c_i| tau / z_i).  A side without a slack -- hard, or no finite bound -- has the gradients 0 as well.  COST: c_i = z_i + Z_i s_i and the
// explicit partials of J are added on every slack, dJ/dz_i = s_i - zeta_s,i, dJ/dZ_i = s_i^2 / 2 - s_i zeta_s,i (one seed).
//
// Mapping: one wavefront per instance.  Phase 1 is the fragment sens_rows_body.hpp, the text k_sens, k_adj and k_slack_fold take their rows
// from: the row gradients at xbar, rcoef and the walk over the slot table (s = lane, lane + 64, ..), with hooks that skip the hard slots and
// keep t_i, lam_i, rho_i (sens_body.hpp: side_slack_terms) and s_i of every soft side in LDS tables (NS, SENS_SIDES) (sens_body.hpp:
// sens_side), with lam_i = 0 for "no slack here".
// Phase 2, per seed: zeta of the seed is staged in LDS, and the lane owns the sides e = lane, lane + 64, .. of the table: r_i zeta_k in
// ascending j (over the entries of the row that rcoef does not have zero), zeta_s,i, one plain store per output entry -- no atomics, the same bits whatever the batch.  Instances whose status is
// neither 0 nor 2 get NaN.  fp64.
#include <cmath>

#include "ihm2mpc_internal.h"
#include "sens_body.hpp"

namespace {

struct PenaltyGradArgs {
    SensArgs s;                         // k_sens' block (sens_u0, sens_x, sens_u, hist unused)
    int n_seeds;                        // 1..8 (COST: 1)
    const double *seed_s, *seed_sa;     // (B,n_seeds,N+1,28), (B,n_seeds,N+1,2) dL/ds; nullptr = zero (COST: not read)
    const double *zeta;                 // (B,n_seeds,N+1,10) of k_adj<true, true>
    double *grad_z, *grad_Z;            // (B,n_seeds,N+1,28)
    double *grad_za, *grad_Za;          // (B,n_seeds,N+1,2)
};

// LDS of one instance (doubles): hc (NS*2) | ha (NS*4) | t, lam, rho, s (NS*30 each) | zeta of one seed (NS*10) | COST: c (NS*30)
__host__ __device__ constexpr size_t penalty_grad_lds_doubles(size_t N, bool cost) { return (N + 1) * (6 + 10 + SENS_SIDES * (cost ? 5 : 4)); }
static_assert(penalty_grad_lds_doubles(40, false) * sizeof(double) == 44608 && penalty_grad_lds_doubles(40, true) * sizeof(double) == 54448,
              "k_penalty_grad: launch LDS at N = 40");

// COST: the slack seeds are dJ_slack/ds_i = z_i + Z_i s_i and the explicit partials of J are added (one seed)
template <bool COST>
__global__ __launch_bounds__(64) void k_penalty_grad(PenaltyGradArgs pa)
{
    extern __shared__ double sm[];
    const SensArgs &a = pa.s;
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int lane = threadIdx.x;
    const int N = a.N, NS = N + 1, S = COST ? 1 : pa.n_seeds;
    const size_t bs = (size_t)b;
    double *gz = pa.grad_z + bs * S * NS * 28, *gZ = pa.grad_Z + bs * S * NS * 28;
    double *gza = pa.grad_za + bs * S * NS * 2, *gZa = pa.grad_Za + bs * S * NS * 2;
    const int st = a.status[b];
    if (st != 0 && st != 2) {           // no solution to differentiate (wave-uniform)
        for (int e = lane; e < S * NS * 28; e += 64) { gz[e] = NAN; gZ[e] = NAN; }
        for (int e = lane; e < S * NS * 2; e += 64) { gza[e] = NAN; gZa[e] = NAN; }
        return;
    }
    double *hc = sm;                    // NS*2   d h_R / d psi, d h_L / d psi of the track rows at xbar
    double *ha = hc + NS * 2;           // NS*4   d a_lat / d (v_x, v_y, T, delta) at xbar
    double *tt = ha + NS * 4;           // NS*30  t_i of the soft sides
    double *lmt = tt + NS * SENS_SIDES; // NS*30  lam_i, 0 = no slack here (or a dropped side)
    double *rho = lmt + NS * SENS_SIDES;    // NS*30  rho_i
    double *slt = rho + NS * SENS_SIDES;    // NS*30  s_i
    double *zl = slt + NS * SENS_SIDES; // NS*10  zeta of the seed at hand
    double *cof = zl + NS * 10;         // NS*30  COST: c_i

    // t, lam, rho, s of one soft side into entry e of the tables
    auto keep_side = [&](int e, double lm, double gap, double sl, double zw, double Zw) {
        slt[e] = sl;
        if (!(lm > 0.0)) return;        // a dropped side: the marker stays 0
        side_slack_terms(lm, gap, sl, zw, Zw, a.tau, tt[e], rho[e]);
        lmt[e] = lm;
        if (COST) cof[e] = fma(Zw, sl, zw);
    };

    // ======== phase 1: the rows at xbar (sens_rows_body.hpp); the terms of every soft side, the marker table zeroed ========
#define SENS_ROWS_CLEAR                                    \
    for (int e = lane; e < NS * SENS_SIDES; e += 64) {     \
        lmt[e] = 0.0;                                      \
        if (COST) slt[e] = 0.0;         /* the explicit partials are taken on every side: 0 where there is no slack */ \
    }
#define SENS_ROWS_SLOT_OPEN(s)                             \
        const double zw = SENS_ROWS_ZW(s), Zw = SENS_ROWS_ZZ(s); \
        if (!(Zw >= 0.0)) continue;         // a hard slot: no slack
#define SENS_ROWS_SLOT_BEGIN(s)
#define SENS_ROWS_SIDE(k, c, up, LM, GAP, SL)              \
            const double lm = LM;                          \
            const double sl = SL;                          \
            keep_side(k * SENS_SIDES + sens_side(c, up), lm, GAP + sl, sl, zw, Zw);
#define SENS_ROWS_SLOT_END(k, c)
#include "sens_rows_body.hpp"
#undef SENS_ROWS_CLEAR
#undef SENS_ROWS_SLOT_OPEN
#undef SENS_ROWS_SLOT_BEGIN
#undef SENS_ROWS_SIDE
#undef SENS_ROWS_SLOT_END

    // ======== phase 2: per seed, zeta_s of the sides this lane owns and the two gradients, one store per output entry ========
    for (int q = 0; q < S; q++) {
        const double *zq = pa.zeta + (bs * S + q) * NS * 10;
        const double *ss = (!COST && pa.seed_s) ? pa.seed_s + (bs * S + q) * NS * 28 : nullptr;
        const double *sa = (!COST && pa.seed_sa) ? pa.seed_sa + (bs * S + q) * NS * 2 : nullptr;
        if (q > 0) WSYNC();             // every lane is done with the last seed's zeta
        for (int e = lane; e < NS * 10; e += 64) zl[e] = zq[e];
        WSYNC();
        for (int e = lane; e < NS * SENS_SIDES; e += 64) {
            const int k = e / SENS_SIDES, o = e - k * SENS_SIDES;
            const bool al = o >= 28;                        // a side of the a_lat row: its outputs are grad_za / grad_Za [o - 28]
            const int c = sens_side_row(o);
            const double sgn = sens_side_upper(o) ? -1.0 : 1.0;
            const double lm = lmt[e];
            double dz = 0.0, dZ = 0.0;
            if (lm != 0.0) {            // a side without a slack is not read
                // r_i zeta_k in ascending j, over the entries rcoef can have: one of a box, n and psi of a track row, four of the a_lat row
                const double *zk = zl + k * 10;
                double rz;
                if (c < 10) rz = zk[c];
                else if (c < 12) {
                    rz = 0.0;
                    for (int j = 0; j < 10; j++) rz = fma(a.CD[((size_t)k * 2 + (c - 10)) * 10 + j], zk[j], rz);
                } else if (c < 14) rz = fma(hc[k * 2 + (c - 12)], zk[2], (c == 12) ? zk[1] : -zk[1]);
                else rz = fma(ha[k * 4 + 3], zk[7], fma(ha[k * 4 + 2], zk[6], fma(ha[k * 4 + 1], zk[4], ha[k * 4] * zk[3])));
                const double t = tt[e];
                const double ci = COST ? cof[e] : al ? (sa ? sa[k * 2 + (o - 28)] : 0.0) : (ss ? ss[k * 28 + o] : 0.0);
                const double zs = fma(ci, t, -(sgn * lm) * rz) / fma(t, rho[e], lm);
                dz = -zs;
                dZ = -__dmul_rn(slt[e], zs);
            }
            if (COST) {                 // the explicit partials of J_slack = z s + Z s^2 / 2 of every slack, one rounded addition each
                const double sl = slt[e];
                dz = __dadd_rn(sl, dz);
                dZ = __dadd_rn(__dmul_rn(0.5 * sl, sl), dZ);
            }
            if (al) {
                gza[(q * NS + k) * 2 + (o - 28)] = dz;
                gZa[(q * NS + k) * 2 + (o - 28)] = dZ;
            } else {
                gz[(q * NS + k) * 28 + o] = dz;
                gZ[(q * NS + k) * 28 + o] = dZ;
            }
        }
    }
}

}  // namespace

// The penalty gradients of the handle on h->stream, behind ihm2_launch_adj with the same zeta (all arrays in device memory): grad_z,
// grad_Z (B,n_seeds,NS,28), grad_za, grad_Za (B,n_seeds,NS,2).  cost: the slack seeds are the cost's own and the explicit partials are
// added (n_seeds = 1, seed_s / seed_sa not read); otherwise seed_s (B,n_seeds,NS,28), seed_sa (B,n_seeds,NS,2), either may be nullptr = zero.
void ihm2_launch_penalty_grad(ihm2mpc_handle *h, int cost, int n_seeds, const double *seed_s, const double *seed_sa, const double *zeta,
                              double *grad_z, double *grad_Z, double *grad_za, double *grad_Za)
{
    PenaltyGradArgs a;
    ihm2_sens_args(h, &a.s);
    a.n_seeds = cost ? 1 : n_seeds;
    a.seed_s = seed_s; a.seed_sa = seed_sa; a.zeta = zeta;
    a.grad_z = grad_z; a.grad_Z = grad_Z; a.grad_za = grad_za; a.grad_Za = grad_Za;
    const size_t lds = sizeof(double) * penalty_grad_lds_doubles((size_t)h->N, cost != 0);
    if (cost) {
        (void)hipFuncSetAttribute((const void *)k_penalty_grad<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_penalty_grad<true>, dim3(h->B), dim3(64), lds, h->stream, a);
    } else {
        (void)hipFuncSetAttribute((const void *)k_penalty_grad<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_penalty_grad<false>, dim3(h->B), dim3(64), lds, h->stream, a);
    }
}
