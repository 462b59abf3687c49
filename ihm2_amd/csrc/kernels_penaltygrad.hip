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
// Mapping: one wavefront per instance.  Phase 1 runs over the slot table as phase 1 of k_slack_fold does (s = lane, lane + 64, ..; the
// row gradients at xbar, rcoef and the row evaluation restated from that file) and keeps t_i, lam_i, rho_i, s_i of every soft side in LDS
// tables (NS, 30) -- 14 lower sides, 14 upper sides, the two sides of the lateral-acceleration row -- with lam_i = 0 for "no slack here".
// Phase 2, per seed: zeta of the seed is staged in LDS, and the lane owns the sides e = lane, lane + 64, .. of the table: r_i zeta_k in
// ascending j (over the entries of the row that rcoef does not have zero), zeta_s,i, one plain store per output entry -- no atomics, the same bits whatever the batch.  Instances whose status is
// neither 0 nor 2 get NaN.  fp64.
#include <cmath>

#include "ihm2mpc_internal.h"
#include "sens_body.hpp"

namespace {

#define PG_SIDES 30     // per stage: lower sides of the rows 0..13, their upper sides, the lower and the upper side of the a_lat row

struct PenaltyGradArgs {
    SensArgs s;                         // k_sens' block (sens_u0, sens_x, sens_u, hist unused)
    int n_seeds;                        // 1..8 (COST: 1)
    const double *seed_s, *seed_sa;     // (B,n_seeds,N+1,28), (B,n_seeds,N+1,2) dL/ds; nullptr = zero (COST: not read)
    const double *zeta;                 // (B,n_seeds,N+1,10) of k_adj<true, true>
    double *grad_z, *grad_Z;            // (B,n_seeds,N+1,28)
    double *grad_za, *grad_Za;          // (B,n_seeds,N+1,2)
};

// LDS of one instance (doubles): hc (NS*2) | ha (NS*4) | t, lam, rho, s (NS*30 each) | zeta of one seed (NS*10) | COST: c (NS*30)
__host__ __device__ constexpr size_t penalty_grad_lds_doubles(size_t N, bool cost) { return (N + 1) * (6 + 10 + PG_SIDES * (cost ? 5 : 4)); }
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
    double *lmt = tt + NS * PG_SIDES;   // NS*30  lam_i, 0 = no slack here (or a dropped side)
    double *rho = lmt + NS * PG_SIDES;  // NS*30  rho_i
    double *slt = rho + NS * PG_SIDES;  // NS*30  s_i
    double *zl = slt + NS * PG_SIDES;   // NS*10  zeta of the seed at hand
    double *cof = zl + NS * 10;         // NS*30  COST: c_i

    const double *xb = a.xbar + bs * NS * 8, *ubb = a.ubar + bs * N * 2;
    const double *xo = a.x + bs * NS * 8, *uo = a.u + bs * N * 2;
    const double *lamb = a.lam + bs * NS * 28, *slkb = a.slk + bs * NS * 28;
    const double *lamab = a.lam_a + bs * NS * 2, *slkab = a.slk_a + bs * NS * 2;
    const double *slb = a.slot_lb + bs * a.sl_bs, *sub = a.slot_ub + bs * a.sl_bs;

    // ---- row gradients of the nonlinear rows at xbar (kernels_slackseed.hip), the marker table zeroed ----
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
    for (int e = lane; e < NS * PG_SIDES; e += 64) {
        lmt[e] = 0.0;
        if (COST) slt[e] = 0.0;         // the explicit partials are taken on every side: 0 where there is no slack
    }
    WSYNC();

    // coefficient of row c of stage k on the variable j of z_k = (dx_k, du_k)
    auto rcoef = [&](int k, int c, int j) -> double {
        if (c < 10) return (j == c) ? 1.0 : 0.0;
        if (c < 12) return a.CD[((size_t)k * 2 + (c - 10)) * 10 + j];
        if (c < 14) return (j == 1) ? ((c == 12) ? 1.0 : -1.0) : (j == 2) ? hc[k * 2 + (c - 12)] : 0.0;
        return (j == 3) ? ha[k * 4] : (j == 4) ? ha[k * 4 + 1] : (j == 6) ? ha[k * 4 + 2] : (j == 7) ? ha[k * 4 + 3] : 0.0;
    };
    // t, lam, rho, s of one soft side into entry e of the tables: t, nu and rho as side_slack_share forms them (sens_body.hpp)
    auto keep_side = [&](int e, double lm, double gap, double sl, double zw, double Zw) {
        slt[e] = sl;
        if (!(lm > 0.0)) return;        // a dropped side: the marker stays 0
        const double nu = fmax(zw + Zw * sl - lm, 0.0);
        tt[e] = fmax(gap, a.tau);
        lmt[e] = lm;
        rho[e] = Zw + nu / fmax(sl, a.tau);
        if (COST) cof[e] = fma(Zw, sl, zw);
    };

    // ======== phase 1: the terms of every soft side, each entry of the slot table on the lane that owns it in the QP ========
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
            keep_side(k * PG_SIDES + ((c == 14) ? 28 : c), lm, rdz - (lb - cz) + sl, sl, zw, Zw);
        }
        if (sfin(ub)) {
            const double lm = (c == 14) ? lamab[k * 2 + 1] : lamb[k * 28 + 14 + c];
            const double sl = (c == 14) ? slkab[k * 2 + 1] : slkb[k * 28 + 14 + c];
            keep_side(k * PG_SIDES + ((c == 14) ? 29 : 14 + c), lm, (ub - cz) - rdz + sl, sl, zw, Zw);
        }
    }
    WSYNC();

    // ======== phase 2: per seed, zeta_s of the sides this lane owns and the two gradients, one store per output entry ========
    for (int q = 0; q < S; q++) {
        const double *zq = pa.zeta + (bs * S + q) * NS * 10;
        const double *ss = (!COST && pa.seed_s) ? pa.seed_s + (bs * S + q) * NS * 28 : nullptr;
        const double *sa = (!COST && pa.seed_sa) ? pa.seed_sa + (bs * S + q) * NS * 2 : nullptr;
        if (q > 0) WSYNC();             // every lane is done with the last seed's zeta
        for (int e = lane; e < NS * 10; e += 64) zl[e] = zq[e];
        WSYNC();
        for (int e = lane; e < NS * PG_SIDES; e += 64) {
            const int k = e / PG_SIDES, o = e - k * PG_SIDES;
            const bool al = o >= 28;                        // a side of the a_lat row
            const int c = al ? 14 : (o < 14) ? o : o - 14;
            const double sgn = (al ? o == 28 : o < 14) ? 1.0 : -1.0;
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
