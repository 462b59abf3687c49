// kernels_adj.hip -- adjoint sensitivities of the last RTI QP's solution: the gradient of a scalar function of the solution with respect
// to the initial state and the reference (acados: eval_adjoint_solution_sensitivity(seed_x, seed_u)).
//
// The differentiated system is k_sens' (kernels_sens.hip, DESIGN.md §4 "x0 sensitivities"): M = [[Ht, E'], [E, 0]] with
// Ht_k = H_k + sum_i sigma_i r_i r_i' and E the rows x_0 = . , x_{k+1} - A_k x_k - B_k u_k = . .  A change of the stage gradients and of the
// initial state moves the solution by M [dz; dpi] = [-dg; (dx0, 0, ..)].  For seeds s_k = dL/dz_k let [zeta; nu] = M^-1 [s; 0] (M is
// symmetric); then dL = -zeta' dg + nu_0' dx0, and with g_k = H_k z_k - Gy_k yref_k (kernels_qp.hip)
//   dL/dx0 = nu_0,   dL/dyref_k = Gy_k' zeta_k  (k < N),   dL/dyref_e = GyT' zeta_N[0:8].
// [zeta; nu] is the solution of the affine LQ problem with the linear terms q_k = -s_k from zeta_x,0 = 0:
//   backward  l_x = q_x + A_k' p_{k+1},  l_u = q_u + B_k' p_{k+1},  kappa_k = -Quu_k^-1 l_u,  p_k = l_x + K_k' l_u,  p_N = q_x,N
//   forward   zeta_u,k = K_k zeta_x,k + kappa_k,  zeta_x,k+1 = A_k zeta_x,k + B_k zeta_u,k;   nu_0 = -p_0
// on the gains K_k and the Quu_k of the backward Riccati sweep on Ht.
//
// Mapping: one wavefront per instance.  Phase 1 is k_sens' factorisation -- the row weights over the slot table, the Riccati sweep, one
// output entry per lane -- from the text sens_body includes too (sens_factor_body.hpp), with a hook that also keeps Quu_k^-1; its
// helpers (side_sigma, SSYNC) and its argument block are sens_body.hpp's.  Phases 2 and 3 carry vectors of 8 / 10 entries, so the lane
// (seed = lane >> 3, row = lane & 7) runs up to eight seeds through both sweeps at the cost of one; p and zeta_x change hands through
// LDS (two buffers: a stage reads one and writes the other), kappa_k of all stages and seeds waits in LDS for the forward sweep.  fp64.
//
// The gradients in the cost weights (k_adj<true>: ihm2mpc_eval_adjoint_sensitivities_w).  The stationarity row of stage k reads
// H_k dz_k + g_k = c_s V' W_k (V z+_k - yref_k) with z+ the returned solution, so a change dW of the weights moves it by c_s V' dW e_k,
// e_k = V z+_k - yref_k (terminal: dW_e (x+_N - yref_e)), and on the symmetric matrices
//   dL/dW = -c_s sum_{k<N} sym((V zeta_k) e_k'),   dL/dW_e = -sym(zeta_N[0:8] (x+_N - yref_e)'),   sym(X) = (X + X') / 2.
// The forward sweep holds all of V zeta_k in every lane of a seed's group (zeta_x,k in LDS, zeta_u,k in registers); e_k does not depend on
// the seed and is formed once per stage by 12 lanes.  The lane (seed, row) keeps row `row` of the 12 x 12 sum and six entries of row
// 8 + (row >> 1) in registers -- 18 of the seed's 144 -- and the sums are symmetrised through LDS when they are written.
#include <cmath>

#include "ihm2mpc_internal.h"
#include "sens_body.hpp"

namespace {

struct AdjArgs {
    SensArgs s;         // k_sens' block (sens_u0, sens_x, sens_u, hist unused)
    // dg_k / dyref_k = -Gy_k: instance base stride, offset of the terminal block, stride between stages -- as hs_bs, hs_te, hs_ks
    const double *Gy;
    int gy_bs, gy_te, gy_ks;
    int n_seeds;        // 1..8
    int unit_u0;        // the two unit seeds on u_0 (n_seeds = 2) instead of seed_x / seed_u
    const double *seed_x, *seed_u;      // (B,n_seeds,N+1,8), (B,n_seeds,N,2); nullptr = zero
    double *grad_x0, *grad_yref, *grad_yref_e;      // (B,n_seeds,8), (B,n_seeds,N,12), (B,n_seeds,8)
    // k_adj<true> only
    const double *yref, *yref_e;        // (B,N,12), (B,8) as the solve read them
    double cs;                          // cost_scale_stage
    double *grad_W, *grad_W_e;          // (B,n_seeds,12,12), (B,n_seeds,8,8)
    // k_adj<true, true> only
    double *zeta;                       // (B,n_seeds,N+1,10) the adjoint solution zeta_k = (zeta_x,k, zeta_u,k), zeros on the input part of row N
};

// LDS of one instance (doubles) behind the factorisation's arrays: see the carve-up in k_adj
__host__ __device__ constexpr size_t adj_lds_doubles(size_t N)
{
    return sens_factor_lds_doubles(N) + N * 4 + N * 16 + 128 + 128;
}
// k_adj<true>: e_k (16) behind those, and at least the 8 x 144 doubles the sums of the eight seeds are symmetrised through
__host__ __device__ constexpr size_t adjw_lds_doubles(size_t N)
{
    return adj_lds_doubles(N) + 16 > 8 * 144 ? adj_lds_doubles(N) + 16 : 8 * 144;
}
static_assert(adj_lds_doubles(40) == 2965 && adj_lds_doubles(1) == 742, "k_adj<false>: launch LDS at N = 40 and N = 1");
static_assert(adjw_lds_doubles(40) == 2981 && adjw_lds_doubles(1) == 8 * 144, "k_adj<true>: likewise; N = 1 sits on the floor of 8 x 144");

// WG: also the gradients in the cost weights (grad_W, grad_W_e); the three other outputs are computed by the same instructions either way.
// ZETA: the forward sweep also stores zeta itself (kernels_penaltygrad.hip reads it); every gradient keeps its instructions
template <bool WG, bool ZETA = false>
__global__ __launch_bounds__(64) void k_adj(AdjArgs aa)
{
    extern __shared__ double sm[];
    const SensArgs &a = aa.s;
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int lane = threadIdx.x;
    const int N = a.N, NS = N + 1, S = aa.n_seeds;
    // ---- LDS carve-up (doubles): w .. Q as in sens_body (sens_body.hpp), sens_factor_lds_doubles of them ----
    double *w = sm;                  // NS*15  row weights sigma_lower + sigma_upper
    double *hc = w + NS * SENS_NR;   // NS*2   d h_R / d psi, d h_L / d psi of the track rows at xbar
    double *ha = hc + NS * 2;        // NS*4   d a_lat / d (v_x, v_y, T, delta) at xbar
    double *Kl = ha + NS * 4;        // N*16   gains K_k
    double *P = Kl + N * 16;         // 64
    double *Al = P + 64;             // 64
    double *Bl = Al + 64;            // 16
    double *Ht = Bl + 16;            // 100
    double *PA = Ht + 100;           // 64
    double *PB = PA + 64;            // 16
    double *Q = PB + 16;             // 84: Qxx (64) | Qux (16) | Quu (4)
    double *Qi = Q + 84;             // N*4    Quu_k^-1 (row-major)
    double *kap = Qi + N * 4;        // N*16   kappa_k of seed j at (k * 8 + j) * 2
    double *pv = kap + N * 16;       // 2*64   p_k of the eight seeds, two buffers
    double *zx = pv + 128;           // 2*64   zeta_x,k of the eight seeds, two buffers
    double *ek = zx + 128;           // 16     e_k = V z+_k - yref_k (WG only)

    const size_t bs = (size_t)b;
    const int sd = lane >> 3, row = lane & 7;       // phases 2 and 3: this lane's seed and row
    const bool live = sd < S;
    double *gx0 = aa.grad_x0 + (bs * S + sd) * 8, *gyr = aa.grad_yref + (bs * S + sd) * N * 12, *gye = aa.grad_yref_e + (bs * S + sd) * 8;
    const int st = a.status[b];
    if (st != 0 && st != 2) {        // no solution to differentiate (wave-uniform)
        if (live) {
            gx0[row] = NAN;
            gye[row] = NAN;
            for (int e = row; e < N * 12; e += 8) gyr[e] = NAN;
            if (WG) {
                double *gW = aa.grad_W + (bs * S + sd) * 144, *gWe = aa.grad_W_e + (bs * S + sd) * 64;
                for (int e = row; e < 144; e += 8) gW[e] = NAN;
                for (int e = row; e < 64; e += 8) gWe[e] = NAN;
            }
            if constexpr (ZETA) {
                double *zt = aa.zeta + (bs * S + sd) * NS * 10;
                for (int e = row; e < NS * 10; e += 8) zt[e] = NAN;
            }
        }
        return;
    }

    // ======== phase 1: the factorisation of sens_body (sens_factor_body.hpp), keeping Quu_k^-1 (row m on the lane j = 0) ========
#define SENS_FACTOR_KEEP_QUU_INV(k, m, j, i0, i1) if (j == 0) { Qi[k * 4 + m * 2] = i0; Qi[k * 4 + m * 2 + 1] = i1; }
#include "sens_factor_body.hpp"
#undef SENS_FACTOR_KEEP_QUU_INV

    // ======== phase 2: the backward vector sweep, eight seeds at once ========
    const double *sxp = (live && aa.seed_x && !aa.unit_u0) ? aa.seed_x + (bs * S + sd) * NS * 8 + row : nullptr;
    const double *sup = (live && aa.seed_u && !aa.unit_u0) ? aa.seed_u + (bs * S + sd) * N * 2 : nullptr;
    auto seed_of_x = [&](int k) -> double { return sxp ? sxp[k * 8] : 0.0; };
    auto seed_of_u = [&](int k, int m) -> double {
        if (aa.unit_u0) return (live && k == 0 && m == sd) ? 1.0 : 0.0;
        return sup ? sup[k * 2 + m] : 0.0;
    };
    int cur = 0;
    double pk = -seed_of_x(N);
    pv[lane] = pk;
    // the record and the seeds of stage k are fetched one stage ahead, into registers
    ra = linb[(size_t)(N - 1) * LIN_REC + lane]; rbv = (lane < 16) ? linb[(size_t)(N - 1) * LIN_REC + 64 + lane] : 0.0;
    double qx = seed_of_x(N - 1), qu0 = seed_of_u(N - 1, 0), qu1 = seed_of_u(N - 1, 1);
    for (int k = N - 1; k >= 0; k--) {
        Al[lane] = ra;
        if (lane < 16) Bl[lane] = rbv;
        double lx = -qx, lu0 = -qu0, lu1 = -qu1;
        if (k > 0) {
            ra = linb[(size_t)(k - 1) * LIN_REC + lane];
            if (lane < 16) rbv = linb[(size_t)(k - 1) * LIN_REC + 64 + lane];
            qx = seed_of_x(k - 1); qu0 = seed_of_u(k - 1, 0); qu1 = seed_of_u(k - 1, 1);
        }
        SSYNC();
        const double *p = pv + cur * 64 + sd * 8;
#pragma unroll
        for (int l = 0; l < 8; l++) {
            const double pl = p[l];
            lx = fma(Al[l * 8 + row], pl, lx);
            lu0 = fma(Bl[l * 2 + 0], pl, lu0);
            lu1 = fma(Bl[l * 2 + 1], pl, lu1);
        }
        const double *K = Kl + k * 16, *qi = Qi + k * 4;
        if (row < 2) kap[(k * 8 + sd) * 2 + row] = -(qi[row * 2] * lu0 + qi[row * 2 + 1] * lu1);
        pk = lx + K[row] * lu0 + K[8 + row] * lu1;
        cur ^= 1;
        pv[cur * 64 + lane] = pk;
        SSYNC();
    }
    if (live) gx0[row] = -pk;        // nu_0 = -p_0

    // ======== phase 3: the forward sweep and the products with Gy ========
    const double *Gy0 = aa.Gy + bs * aa.gy_bs, *GyT = Gy0 + aa.gy_te;
    cur = 0;
    zx[lane] = 0.0;
    ra = linb[lane]; rbv = (lane < 16) ? linb[64 + lane] : 0.0;
    // WG: row `row` of sum_k (V zeta_k) e_k' and the columns hc0 .. hc0 + 5 of its row 8 + (row >> 1)
    double wr[12], wh[6];
    const int hr = row >> 1, hc0 = (row & 1) * 6;
    const double *yrb = WG ? aa.yref + bs * N * 12 : nullptr;
    double *zt = nullptr;
    if constexpr (ZETA) zt = aa.zeta + (bs * S + sd) * NS * 10;
    if (WG) {
#pragma unroll
        for (int j = 0; j < 12; j++) wr[j] = 0.0;
#pragma unroll
        for (int j = 0; j < 6; j++) wh[j] = 0.0;
    }
    for (int k = 0; k < N; k++) {
        Al[lane] = ra;
        if (lane < 16) Bl[lane] = rbv;
        if (WG && lane < 12) {       // e_k: y = (x, u, x[6:8] - u) of the returned solution minus yref_k
            const double y = (lane < 8) ? xo[k * 8 + lane] : (lane < 10) ? uo[k * 2 + lane - 8] : xo[k * 8 + lane - 4] - uo[k * 2 + lane - 10];
            ek[lane] = y - yrb[k * 12 + lane];
        }
        if (k + 1 < N) {
            ra = linb[(size_t)(k + 1) * LIN_REC + lane];
            if (lane < 16) rbv = linb[(size_t)(k + 1) * LIN_REC + 64 + lane];
        }
        SSYNC();
        const double *zk = zx + cur * 64 + sd * 8, *K = Kl + k * 16, *G = Gy0 + (size_t)k * aa.gy_ks;
        double u0 = kap[(k * 8 + sd) * 2], u1 = kap[(k * 8 + sd) * 2 + 1];
        double xn = 0.0, g0 = 0.0, g1 = 0.0;
#pragma unroll
        for (int l = 0; l < 8; l++) {
            const double zl = zk[l];
            u0 = fma(K[l], zl, u0);
            u1 = fma(K[8 + l], zl, u1);
            xn = fma(Al[row * 8 + l], zl, xn);
            g0 = fma(G[l * 12 + row], zl, g0);
            if (row < 4) g1 = fma(G[l * 12 + 8 + row], zl, g1);
        }
        xn = fma(Bl[row * 2 + 0], u0, xn);
        xn = fma(Bl[row * 2 + 1], u1, xn);
        g0 = fma(G[8 * 12 + row], u0, g0);
        g0 = fma(G[9 * 12 + row], u1, g0);
        if (live) gyr[k * 12 + row] = g0;          // columns row and (row < 4) 8 + row of Gy_k' zeta_k
        if constexpr (ZETA) {
            if (live) {
                zt[k * 10 + row] = zk[row];
                if (row < 2) zt[k * 10 + 8 + row] = row ? u1 : u0;
            }
        }
        if (row < 4) {
            g1 = fma(G[8 * 12 + 8 + row], u0, g1);
            g1 = fma(G[9 * 12 + 8 + row], u1, g1);
            if (live) gyr[k * 12 + 8 + row] = g1;
        }
        if (WG) {
            // V zeta_k: zeta_x,k (8), zeta_u,k (2), zeta_x,k[6:8] - zeta_u,k
            const double ar = zk[row], ah = (hr == 0) ? u0 : (hr == 1) ? u1 : (hr == 2) ? zk[6] - u0 : zk[7] - u1;
#pragma unroll
            for (int j = 0; j < 12; j++) wr[j] = fma(ar, ek[j], wr[j]);
#pragma unroll
            for (int j = 0; j < 6; j++) wh[j] = fma(ah, ek[hc0 + j], wh[j]);
        }
        cur ^= 1;
        zx[cur * 64 + lane] = xn;
        SSYNC();
    }
    {
        const double *zk = zx + cur * 64 + sd * 8;
        double ge = 0.0;
#pragma unroll
        for (int l = 0; l < 8; l++) ge = fma(GyT[l * 12 + row], zk[l], ge);
        if (live) gye[row] = ge;
        if constexpr (ZETA) {
            if (live) {
                zt[N * 10 + row] = zk[row];
                if (row < 2) zt[N * 10 + 8 + row] = 0.0;
            }
        }
        if (WG) {
            // the terminal outer product: both products rounded before they are added, so that entry (i, j) and entry (j, i) get the same bits
            double *gWe = aa.grad_W_e + (bs * S + sd) * 64;
            const double *xN = xo + N * 8, *yre = aa.yref_e + bs * 8;
            const double zi = zk[row], ei = xN[row] - yre[row];
            double oe[8];
#pragma unroll
            for (int j = 0; j < 8; j++) oe[j] = -0.5 * (__dmul_rn(zi, xN[j] - yre[j]) + __dmul_rn(zk[j], ei));
            SSYNC();                    // every lane has read zeta_N: the LDS is free for the staging of the stage sums
            double *X = sm + sd * 144;
#pragma unroll
            for (int j = 0; j < 12; j++) X[row * 12 + j] = wr[j];
#pragma unroll
            for (int j = 0; j < 6; j++) X[(8 + hr) * 12 + hc0 + j] = wh[j];
            SSYNC();
            if (live) {
                double *gW = aa.grad_W + (bs * S + sd) * 144;
                const double f = -0.5 * aa.cs;
                for (int e = row; e < 144; e += 8) {
                    const int i = e / 12, j = e - i * 12;
                    gW[e] = f * (X[i * 12 + j] + X[j * 12 + i]);
                }
#pragma unroll
                for (int j = 0; j < 8; j++) gWe[row * 8 + j] = oe[j];
            }
        }
    }
}

}  // namespace

// The handle's adjoint evaluation on h->stream: seeds from h->adj_sx / h->adj_su (nullptr = zero; unit_u0: the two unit seeds on u_0),
// gradients into h->adj_gx0, h->adj_gy, h->adj_gye and (weights) h->adj_gW, h->adj_gWe.  zeta (device, (B,n_seeds,N+1,10)) or nullptr: with
// weights, k_adj<true, true> also stores the adjoint solution there.
void ihm2_launch_adj(ihm2mpc_handle *h, int n_seeds, const double *seed_x, const double *seed_u, int unit_u0, int weights, double *zeta)
{
    AdjArgs a;
    ihm2_sens_args(h, &a.s);
    a.Gy = h->Gy; a.gy_bs = 0; a.gy_te = h->N * 120; a.gy_ks = 120;
    if (h->inst_w) { a.Gy = h->iGy; a.gy_bs = 240; a.gy_te = 120; a.gy_ks = 0; }
    a.n_seeds = n_seeds; a.unit_u0 = unit_u0;
    a.seed_x = seed_x; a.seed_u = seed_u;
    a.grad_x0 = h->adj_gx0; a.grad_yref = h->adj_gy; a.grad_yref_e = h->adj_gye;
    a.yref = h->yref; a.yref_e = h->yref_e; a.cs = h->cfg.cost_scale_stage;
    a.grad_W = h->adj_gW; a.grad_W_e = h->adj_gWe;
    a.zeta = zeta;
    if (weights) {
        const size_t lds = sizeof(double) * adjw_lds_doubles((size_t)h->N);
        if (zeta) {
            (void)hipFuncSetAttribute((const void *)k_adj<true, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL((k_adj<true, true>), dim3(h->B), dim3(64), lds, h->stream, a);
            return;
        }
        (void)hipFuncSetAttribute((const void *)k_adj<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_adj<true>, dim3(h->B), dim3(64), lds, h->stream, a);
        return;
    }
    const size_t lds = sizeof(double) * adj_lds_doubles((size_t)h->N);
    (void)hipFuncSetAttribute((const void *)k_adj<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_adj<false>, dim3(h->B), dim3(64), lds, h->stream, a);
}
