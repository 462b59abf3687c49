// kernels_cost.hip -- the objective of the OCP at the handle's iterate, and the pieces of its total gradient in x0, yref and the weights
// (ihm2mpc_eval_cost, ihm2mpc_eval_cost_gradient; DESIGN.md §4 "cost and its gradient").
//
//   J = sum_{k<N} (c_s / 2) e_k' W_k e_k + 1/2 e_N' W_e e_N + J_slack,   e_k = V z_k - yref_k,  e_N = x_N - yref_e,
//   J_slack = sum over the soft sides of z_i s_i + 1/2 Z_i s_i^2
// with V the 12 x 10 selector y = (x, u, x[6:8] - u), c_s = cost_scale_stage, W_k from Wd (iWd with per-instance weights), s_i from slk
// (slk_a for the lateral-acceleration row), z_i / Z_i from st_sz / st_sZ: what the merit function of the SQP mode sums at the full
// step (sqp_body.hpp: merit), evaluated here at (x, u) as they are.
//
// k_cost<GRAD>: one wavefront per instance, the lane over the stages k = lane, lane + 64, ..; every sum in a fixed index order, the
// horizon's sum by the butterfly of the QP (wave_sum), so the value does not depend on the batch or the launch.  W waits in LDS when it
// is the same for every stage.  GRAD also writes, with t_k = W_k e_k,
//   the seeds dJ/dz_k of the adjoint entries (n_seeds = 1):  seed_z,k = c_s V' t_k,  seed_x,N = W_e e_N,
//   the explicit partials:  dJ/dyref_k = -c_s t_k,  dJ/dyref_e = -W_e e_N,  dJ/dW = (c_s / 2) sum_k e_k e_k',  dJ/dW_e = 1/2 e_N e_N'
// -- the two outer-product sums with entry (i, j), i <= j, owned by one lane, summed over k in stage order and mirrored: symmetric to the
// bit.  k_cost_epilogue adds the explicit partials to k_adj<true>'s gradients of those seeds (one rounded addition per element).
#include <algorithm>
#include <cmath>

#include "ihm2mpc_internal.h"
#include "wave_sync.hpp"

namespace {

struct CostArgs {
    int B, N;
    double cs;
    // W (.., 12, 12) of the stages and W_e (8, 8): instance base stride, stride between stages, offset of W_e -- as sqp_body.hpp: LsArgs;
    // w_same: one W for every stage k < N (kept in LDS)
    const double *W;
    int w_bs, w_ks, w_te, w_same;
    const double *st_lb, *st_ub;        // (NS,14) bounds per (stage, row), -+inf = absent; st_bs doubles per instance (0: batch-shared)
    int st_bs;
    const double *st_sz, *st_sZ;        // (NS,28) slack penalties per side, sZ < 0 = hard; sp_bs doubles per instance (0: batch-shared)
    int sp_bs;
    // the lateral-acceleration row (stages 1 .. N-1): its finite sides, lower / upper, and their penalties -- device memory, al_bs
    // doubles per instance (per-instance penalties: (B,2), al_bs = 2), or nullptr: the batch-shared pair below
    int alat_on, alat_fin[2];
    const double *alat_pz, *alat_pZ;
    int al_bs;
    double alat_sz[2], alat_sZ[2];
    const double *x, *u, *yref, *yref_e, *slk, *slk_a;
    const int32_t *status;
    double *cost, *stage_cost, *slack_cost;     // (B), (B,NS), (B); each may be nullptr
    // GRAD
    double *seed_x, *seed_u;                    // (B,NS,8), (B,N,2)
    double *ex_yref, *ex_yref_e, *ex_W, *ex_We; // (B,N,12), (B,8), (B,12,12), (B,8,8)
};

__device__ __forceinline__ double cost_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// LDS of one instance (doubles): W (144) | W_e (64) | GRAD: e_k of the stages 0 .. N (12 each, the terminal one takes 8)
__host__ __device__ constexpr size_t cost_lds_doubles(size_t N, bool grad) { return 208 + (grad ? (N + 1) * 12 : 0); }
static_assert(cost_lds_doubles(40, true) * sizeof(double) == 5600, "k_cost<true>: launch LDS at N = 40");

// entry p = 0 .. n (n + 1) / 2 - 1 of the upper triangle of an n x n matrix, row-major: its row and column
__device__ __forceinline__ void tri_entry(int p, int n, int &i, int &j)
{
    i = 0;
    while (p >= n - i) { p -= n - i; i++; }
    j = i + p;
}

template <bool GRAD>
__global__ __launch_bounds__(64) void k_cost(CostArgs a)
{
    extern __shared__ double sm[];
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int lane = threadIdx.x;
    const int N = a.N, NS = N + 1;
    double *Wl = sm, *Wel = sm + 144, *el = sm + 208;
    const size_t bs = (size_t)b;
    const double *Wb = a.W + bs * a.w_bs;
    const double *xb = a.x + bs * NS * 8, *ub = a.u + bs * N * 2, *yrb = a.yref + bs * N * 12, *yeb = a.yref_e + bs * 8;
    const double *slb = a.slk + bs * NS * 28, *slab = a.slk_a + bs * NS * 2;
    const double *lbb = a.st_lb + bs * a.st_bs, *ubb = a.st_ub + bs * a.st_bs;
    const double *szb = a.st_sz + bs * a.sp_bs, *sZb = a.st_sZ + bs * a.sp_bs;
    double al_z[2], al_Z[2];            // wave-uniform
    for (int m = 0; m < 2; m++) {
        al_z[m] = a.alat_pz ? a.alat_pz[bs * a.al_bs + m] : a.alat_sz[m];
        al_Z[m] = a.alat_pZ ? a.alat_pZ[bs * a.al_bs + m] : a.alat_sZ[m];
    }

    if (a.w_same)
        for (int e = lane; e < 144; e += 64) Wl[e] = Wb[e];
    Wel[lane] = Wb[a.w_te + lane];
    WSYNC();

    const int st = a.status[b];
    const bool solved = st == 0 || st == 2;      // wave-uniform
    double csum = 0.0, ssum = 0.0;
    for (int k = lane; k < NS; k += 64) {
        double track;
        if (k < N) {
            const double *xk = xb + k * 8, *yr = yrb + k * 12;
            const double uT = ub[k * 2], ud = ub[k * 2 + 1];
            double e[12], t[12];
#pragma unroll
            for (int i = 0; i < 8; i++) e[i] = xk[i] - yr[i];
            e[8] = uT - yr[8]; e[9] = ud - yr[9]; e[10] = xk[6] - uT - yr[10]; e[11] = xk[7] - ud - yr[11];
            const double *Wk = a.w_same ? Wl : Wb + (size_t)k * a.w_ks;
            double q = 0.0;
#pragma unroll
            for (int i = 0; i < 12; i++) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 12; j++) acc = fma(Wk[i * 12 + j], e[j], acc);
                t[i] = acc;
                q = fma(e[i], acc, q);
            }
            track = 0.5 * a.cs * q;
            if (GRAD) {
                double *sx = a.seed_x + (bs * NS + k) * 8, *su = a.seed_u + (bs * N + k) * 2, *gy = a.ex_yref + (bs * N + k) * 12;
#pragma unroll
                for (int i = 0; i < 6; i++) sx[i] = a.cs * t[i];
                sx[6] = a.cs * (t[6] + t[10]); sx[7] = a.cs * (t[7] + t[11]);
                su[0] = a.cs * (t[8] - t[10]); su[1] = a.cs * (t[9] - t[11]);
#pragma unroll
                for (int i = 0; i < 12; i++) { gy[i] = solved ? -(a.cs * t[i]) : NAN; el[k * 12 + i] = e[i]; }
            }
        } else {
            const double *xk = xb + N * 8;
            double e[8], q = 0.0;
#pragma unroll
            for (int i = 0; i < 8; i++) e[i] = xk[i] - yeb[i];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 8; j++) acc = fma(Wel[i * 8 + j], e[j], acc);
                q = fma(e[i], acc, q);
                if (GRAD) {
                    a.seed_x[(bs * NS + N) * 8 + i] = acc;
                    a.ex_yref_e[bs * 8 + i] = solved ? -acc : NAN;
                    el[N * 12 + i] = e[i];
                }
            }
            track = 0.5 * q;
        }
        // the soft sides of the stage: a finite side with Z >= 0 carries a slack (sqp_body.hpp: merit)
        double sl = 0.0;
        for (int c = 0; c < 14; c++) {
            if (lbb[k * 14 + c] > -INFINITY && sZb[k * 28 + c] >= 0.0) {
                const double sv = slb[k * 28 + c];
                sl += fma(0.5 * sZb[k * 28 + c] * sv, sv, szb[k * 28 + c] * sv);
            }
            if (ubb[k * 14 + c] < INFINITY && sZb[k * 28 + 14 + c] >= 0.0) {
                const double sv = slb[k * 28 + 14 + c];
                sl += fma(0.5 * sZb[k * 28 + 14 + c] * sv, sv, szb[k * 28 + 14 + c] * sv);
            }
        }
        if (a.alat_on && k >= 1 && k < N)
            for (int m = 0; m < 2; m++)
                if (a.alat_fin[m] && al_Z[m] >= 0.0) {
                    const double sv = slab[k * 2 + m];
                    sl += fma(0.5 * al_Z[m] * sv, sv, al_z[m] * sv);
                }
        const double v = track + sl;
        if (a.stage_cost) a.stage_cost[bs * NS + k] = v;
        csum += v; ssum += sl;
    }
    csum = cost_wave_sum(csum); ssum = cost_wave_sum(ssum);
    if (lane == 0) {
        if (a.cost) a.cost[b] = csum;
        if (a.slack_cost) a.slack_cost[b] = ssum;
    }
    if (GRAD) {
        WSYNC();            // e_k of all stages are in LDS
        double *gW = a.ex_W + bs * 144, *gWe = a.ex_We + bs * 64;
        for (int p = lane; p < 78; p += 64) {
            int i, j;
            tri_entry(p, 12, i, j);
            double acc = 0.0;
            for (int k = 0; k < N; k++) acc = fma(el[k * 12 + i], el[k * 12 + j], acc);
            const double v = solved ? 0.5 * a.cs * acc : NAN;
            gW[i * 12 + j] = v; gW[j * 12 + i] = v;
        }
        if (lane < 36) {
            int i, j;
            tri_entry(lane, 8, i, j);
            const double v = solved ? 0.5 * __dmul_rn(el[N * 12 + i], el[N * 12 + j]) : NAN;
            gWe[i * 8 + j] = v; gWe[j * 8 + i] = v;
        }
    }
}

// dst[e] := src[e] + dst[e] on four arrays, blockIdx.y the array
struct EpiArgs { double *dst[4]; const double *src[4]; size_t n[4]; };

__global__ __launch_bounds__(256) void k_cost_epilogue(EpiArgs a)
{
    const int s = blockIdx.y;
    double *dst = a.dst[s];
    const double *src = a.src[s];
    const size_t n = a.n[s];
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) dst[e] = __dadd_rn(src[e], dst[e]);
}

}  // namespace

// The cost kernel of the handle on h->stream.  cost (B), stage_cost (B,NS), slack_cost (B) may each be nullptr.  grad: also the seeds
// into seed_x (B,NS,8), seed_u (B,N,2) and the explicit partials into ex_yref (B,N,12), ex_yref_e (B,8), ex_W (B,144), ex_We (B,64).
void ihm2_launch_cost(ihm2mpc_handle *h, int grad, double *cost, double *stage_cost, double *slack_cost, double *seed_x, double *seed_u,
                      double *ex_yref, double *ex_yref_e, double *ex_W, double *ex_We)
{
    CostArgs a;
    a.B = h->B; a.N = h->N; a.cs = h->cfg.cost_scale_stage;
    a.W = h->Wd; a.w_bs = 0; a.w_ks = 144; a.w_te = h->N * 144; a.w_same = h->shared_uniform_H ? 1 : 0;
    if (h->inst_w) { a.W = h->iWd; a.w_bs = 208; a.w_ks = 0; a.w_te = 144; a.w_same = 1; }
    a.st_lb = h->st_lb; a.st_ub = h->st_ub; a.st_bs = 0;
    if (h->inst_b || h->inst_p) { a.st_lb = h->i_st_lb; a.st_ub = h->i_st_ub; a.st_bs = h->NS * (NC + NLAM); }
    a.st_sz = a.st_lb + h->NS * NC; a.st_sZ = a.st_ub + h->NS * NC; a.sp_bs = a.st_bs;      // the penalties: the second half of the same table
    a.alat_pz = nullptr; a.alat_pZ = nullptr; a.al_bs = 0;
    if (h->inst_p) { a.alat_pz = h->ip.alat_sz; a.alat_pZ = h->ip.alat_sZ; a.al_bs = 2; }
    a.alat_on = h->rows.alat_on;
    a.alat_fin[0] = std::isfinite(h->rows.alat_lb); a.alat_fin[1] = std::isfinite(h->rows.alat_ub);
    for (int m = 0; m < 2; m++) { a.alat_sz[m] = h->rows.alat_sz[m]; a.alat_sZ[m] = h->rows.alat_sZ[m]; }
    a.x = h->x; a.u = h->u; a.yref = h->yref; a.yref_e = h->yref_e; a.slk = h->slk; a.slk_a = h->slk_a;
    a.status = h->status;
    a.cost = cost; a.stage_cost = stage_cost; a.slack_cost = slack_cost;
    a.seed_x = seed_x; a.seed_u = seed_u; a.ex_yref = ex_yref; a.ex_yref_e = ex_yref_e; a.ex_W = ex_W; a.ex_We = ex_We;
    const size_t lds = sizeof(double) * cost_lds_doubles((size_t)h->N, grad != 0);
    if (grad) {
        (void)hipFuncSetAttribute((const void *)k_cost<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(k_cost<true>, dim3(h->B), dim3(64), lds, h->stream, a);
    } else {
        hipLaunchKernelGGL(k_cost<false>, dim3(h->B), dim3(64), lds, h->stream, a);
    }
}

// ex_* := the adjoint gradients of one seed (h->adj_gy, adj_gye, adj_gW, adj_gWe) + ex_*, on h->stream
void ihm2_launch_cost_epilogue(ihm2mpc_handle *h, double *ex_yref, double *ex_yref_e, double *ex_W, double *ex_We)
{
    const size_t B = h->B;
    EpiArgs a;
    a.dst[0] = ex_yref; a.src[0] = h->adj_gy; a.n[0] = B * h->N * NY;
    a.dst[1] = ex_yref_e; a.src[1] = h->adj_gye; a.n[1] = B * NX;
    a.dst[2] = ex_W; a.src[2] = h->adj_gW; a.n[2] = B * NY * NY;
    a.dst[3] = ex_We; a.src[3] = h->adj_gWe; a.n[3] = B * NX * NX;
    const size_t most = std::max(a.n[0], a.n[2]);
    const unsigned blocks = (unsigned)std::min<size_t>((most + 255) / 256, 4096);
    hipLaunchKernelGGL(k_cost_epilogue, dim3(blocks, 4), dim3(256), 0, h->stream, a);
}
