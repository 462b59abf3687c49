// kernels_weights.hip -- the per-instance weight tables expanded on the device (ihm2mpc_set_instance_weights_device): the twin of
// ihm2::stage_weight_tables and ihm2::terminal_weight_tables (qp_tables.hpp), which ihm2mpc_set_instance_weights runs on the host, plus the
// copy Wd = [W | W_e] that the merit function and the cost read.
//
// Per instance, from W (12,12) and W_e (8,8):
//   Gy stage (10,12) = c_s V'W        Hs stage (10,10) = c_s V'WV        (V the 12x10 output selector y = V z, entries 0 and +-1)
//   Gy terminal: W_e in the first 8x8, 0 elsewhere                       Hs terminal: W_e in the first 8x8, then I(2), 0 elsewhere
// in the layouts the host setter uploads, (B,2,100), (B,2,120), (B,208), every entry written -- the zeros too.
//
// Bit-identity with the host functions: the same products, summed over l = 0..11 in ascending order from acc = 0, c_s applied last.  Every
// product has a factor 0 or +-1 and is exact, so a fused multiply-add gives the bits of a multiply and an add and the contraction of the
// build cannot tell the two apart.  The zero terms are NOT skipped: 0 * inf is NaN and -0.0 + 0.0 is +0.0 on the host, and so here.
//
// Mapping: one wavefront per instance, lane = output entry (e = lane, lane + 64, ..).  W, W_e are staged in LDS; V'W (unscaled) goes from
// the first phase to the second through LDS with WSYNC.  No s_barrier, no atomics, plain vector stores.  fp64.
//
// CHECK: nothing is stored but code[b] (ihm2mpc_internal.h: ihm2_weight_code_*), in the order of the host setter's tests: the first NaN of
// W, the first NaN of W_e, symmetric10 of the stage Hessian, symmetric10 of the terminal Hessian.
#include <cmath>

#include "ihm2mpc_internal.h"
#include "wave_sync.hpp"

namespace {

struct WeightArgs {
    int B;
    double cs;                  // cost_scale_stage
    const double *W, *W_e;      // (B,12,12), (B,8,8)
    double *Hs, *Gy, *Wd;       // (B,2,100), (B,2,120), (B,208)
    int32_t *code;              // (B), CHECK only
};

// qp_tables.hpp: cost_selector, entry [l][i]
__device__ inline double sel_V(int l, int i)
{
    if (l < 10) return (l == i) ? 1.0 : 0.0;
    if (i == l - 4) return 1.0;         // V[10][6], V[11][7]
    if (i == l - 2) return -1.0;        // V[10][8], V[11][9]
    return 0.0;
}

// qp_tables.hpp: symmetric10's test of one pair, as the host evaluates it (a multiply and an add, no contraction)
__device__ inline bool asym_pair(double a, double b)
{
#pragma clang fp contract(off)
    return fabs(a - b) > 1e-12 * (1 + fabs(a));
}

// LDS of one instance (doubles): W (144) | W_e (64) | V'W (120) | CHECK: Hs stage (100)
constexpr int WT_LDS = 144 + 64 + 120 + 100;

template <bool CHECK>
__global__ __launch_bounds__(64) void k_weight_tables(WeightArgs a)
{
    __shared__ double sm[WT_LDS];
    const int b = blockIdx.x;
    if (b >= a.B) return;
    const int lane = threadIdx.x;
    double *Ws = sm, *Wes = Ws + 144, *VtW = Wes + 64, *Hst = VtW + 120;
    const size_t bs = (size_t)b;
    const double *W = a.W + bs * 144, *We = a.W_e + bs * 64;
    double *Hs = a.Hs + bs * 200, *Gy = a.Gy + bs * 240, *Wd = a.Wd + bs * 208;

    int code = ihm2_weight_code_ok;     // wave-uniform
    for (int e = lane; e < 192; e += 64) {          // (every lane takes part in the ballots)
        const double w = (e < 144) ? W[e] : 0.0;
        if (e < 144) {
            Ws[e] = w;
            if (!CHECK) Wd[e] = w;
        }
        if (CHECK) {
            const unsigned long long m = __ballot(w != w);
            if (m && !code) code = ihm2_weight_code_nan_W + (e - lane) + __ffsll((long long)m) - 1;
        }
    }
    {
        const double w = We[lane];
        Wes[lane] = w;
        if (!CHECK) Wd[144 + lane] = w;
        if (CHECK) {
            const unsigned long long m = __ballot(w != w);
            if (m && !code) code = ihm2_weight_code_nan_We + __ffsll((long long)m) - 1;
        }
    }
    WSYNC();

    // ---- stage: V'W and Gy = c_s V'W ----
    for (int e = lane; e < 120; e += 64) {
        const int i = e / 12, j = e - i * 12;
        double acc = 0;
        for (int l = 0; l < NY; l++) acc += sel_V(l, i) * Ws[l * NY + j];
        VtW[e] = acc;
        if (!CHECK) Gy[e] = a.cs * acc;
    }
    WSYNC();
    // ---- stage: Hs = c_s (V'W) V ----
    for (int e = lane; e < 100; e += 64) {
        const int i = e / 10, j = e - i * 10;
        double acc = 0;
        for (int l = 0; l < NY; l++) acc += VtW[i * 12 + l] * sel_V(l, j);
        if (CHECK) Hst[e] = a.cs * acc;
        else Hs[e] = a.cs * acc;
    }
    if (!CHECK) {
        // ---- terminal: W_e padded with I (Hs), W_e in the first 8x8 (Gy) ----
        for (int e = lane; e < 100; e += 64) {
            const int i = e / 10, j = e - i * 10;
            Hs[100 + e] = (i < NX && j < NX) ? Wes[i * NX + j] : (i == j) ? 1.0 : 0.0;
        }
        for (int e = lane; e < 120; e += 64) {
            const int i = e / 12, j = e - i * 12;
            Gy[120 + e] = (i < NX && j < NX) ? Wes[i * NX + j] : 0.0;
        }
        return;
    }
    WSYNC();
    // ---- symmetric10 of both Hessians: the pairs (i, j < i); the terminal one's rows 8, 9 are those of I ----
    bool bad_s = false, bad_t = false;
    for (int e = lane; e < 100; e += 64) {
        const int i = e / 10, j = e - i * 10;
        if (j >= i) continue;
        bad_s = bad_s || asym_pair(Hst[i * 10 + j], Hst[j * 10 + i]);
        if (i < NX) bad_t = bad_t || asym_pair(Wes[i * NX + j], Wes[j * NX + i]);
    }
    const bool any_s = __ballot(bad_s) != 0, any_t = __ballot(bad_t) != 0;
    if (!code && any_s) code = ihm2_weight_code_asym_stage;
    if (!code && any_t) code = ihm2_weight_code_asym_terminal;
    if (lane == 0) a.code[b] = code;
}

}  // namespace

void ihm2_launch_weight_tables(ihm2mpc_handle *h, const double *W, const double *W_e, double *Hs, double *Gy, double *Wd, int32_t *code)
{
    WeightArgs a;
    a.B = h->B; a.cs = h->cfg.cost_scale_stage;
    a.W = W; a.W_e = W_e; a.Hs = Hs; a.Gy = Gy; a.Wd = Wd; a.code = code;
    if (code) hipLaunchKernelGGL(k_weight_tables<true>, dim3(h->B), dim3(64), 0, h->stream, a);
    else hipLaunchKernelGGL(k_weight_tables<false>, dim3(h->B), dim3(64), 0, h->stream, a);
}
