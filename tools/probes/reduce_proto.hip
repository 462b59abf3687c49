// Stand-alone timing + check of the packed wave reductions of ihm2_amd/csrc/qp_reduce.hpp against the one-value butterflies they replace in
// the full slot form of the QP (kernels_qp.hip): one wave, cycle counter stamps around a dependent chain of CHAIN reductions, median over REPS.
//   norms:  four wave_nanmax + one wave_sum (today)      against  wave_max4 + four ballots + the same wave_sum
//   bounds: two wave_min (today)                         against  wave_min2
// The inputs come from memory and every link of the chain feeds its results back into the next one's operands, so nothing folds; both forms
// must return the same bits, also with a NaN in any one value (checked on every repetition, counted in `mismatches`).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -I ihm2_amd/csrc tools/probes/reduce_proto.hip -o reduce_proto
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "riccati_mfma.hpp"
#include "qp_reduce.hpp"
using namespace ihm2;

constexpr int REPS = 4096, CHAIN = 8, NIN = 1 << 14;

// ---- today's reductions, as in kernels_qp.hip ----
template <typename OP>
__device__ __forceinline__ double wave_reduce(double v, OP op)
{
    v = op(v, dpp_mov<0xB1>(v));
    v = op(v, dpp_mov<0x4E>(v));
    v = op(v, dpp_mov<0x141>(v));
    v = op(v, dpp_mov<0x128>(v));
    int lo = __double2loint(v), hi = __double2hiint(v);
    auto a16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    auto b16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    v = op(__hiloint2double(b16[0], a16[0]), __hiloint2double(b16[1], a16[1]));
    lo = __double2loint(v); hi = __double2hiint(v);
    auto a32 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    auto b32 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return op(__hiloint2double(b32[0], a32[0]), __hiloint2double(b32[1], a32[1]));
}
__device__ __forceinline__ double nanmax(double a, double b) { return (a != a || b != b) ? NAN : fmax(a, b); }
__device__ __forceinline__ double wave_min(double v) { return wave_reduce(v, [](double a, double b) { return fmin(a, b); }); }
__device__ __forceinline__ double wave_sum(double v) { return wave_reduce(v, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ double wave_nanmax(double v) { return wave_reduce(v, [](double a, double b) { return nanmax(a, b); }); }

struct Five { double g, b, d, m, mu; };
__device__ __forceinline__ Five norms_old(int, Five v)
{
    v.g = wave_nanmax(v.g); v.b = wave_nanmax(v.b); v.d = wave_nanmax(v.d); v.m = wave_nanmax(v.m); v.mu = wave_sum(v.mu);
    return v;
}
__device__ __forceinline__ Five norms_new(int lane, Five v)
{
    const bool ng = wave_any(v.g != v.g), nb = wave_any(v.b != v.b), nd = wave_any(v.d != v.d), nm = wave_any(v.m != v.m);
    wave_max4(lane, v.g, v.b, v.d, v.m);
    v.mu = wave_sum(v.mu);
    if (ng) v.g = NAN;
    if (nb) v.b = NAN;
    if (nd) v.d = NAN;
    if (nm) v.m = NAN;
    return v;
}
__device__ __forceinline__ Five bounds_old(int, Five v) { v.g = wave_min(v.g); v.b = wave_min(v.b); return v; }
__device__ __forceinline__ Five bounds_new(int lane, Five v) { wave_min2(lane, v.g, v.b); return v; }

__device__ __forceinline__ unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// which: 0 norms_old, 1 norms_new, 2 bounds_old, 3 bounds_new.  cyc[rep]: cycles of CHAIN dependent reductions; out[rep * 5 + i]: bits of the last link.
template <int WHICH>
__global__ __launch_bounds__(64) void k_time(const double *in, long long *cyc, unsigned long long *out)
{
    const int lane = threadIdx.x;
    for (int rep = 0; rep < REPS; rep++) {
        const double *p = in + ((size_t)(rep * 320 + lane * 5) & (NIN - 1));
        Five own = {p[0], p[1], p[2], p[3], p[4]}, v = own;
        asm volatile("" : "+v"(v.g), "+v"(v.b), "+v"(v.d), "+v"(v.m), "+v"(v.mu));
        const long long t0 = __builtin_readcyclecounter();
#pragma unroll
        for (int j = 0; j < CHAIN; j++) {
            if (j > 0) {        // the next link's operands depend on this link's results and on the lane
                v.g = fma(v.g, 1e-3, own.g); v.b = fma(v.b, 1e-3, own.b); v.d = fma(v.d, 1e-3, own.d); v.m = fma(v.m, 1e-3, own.m); v.mu = fma(v.mu, 1e-3, own.mu);
            }
            v = (WHICH == 0) ? norms_old(lane, v) : (WHICH == 1) ? norms_new(lane, v) : (WHICH == 2) ? bounds_old(lane, v) : bounds_new(lane, v);
        }
        asm volatile("" : "+v"(v.g), "+v"(v.b), "+v"(v.d), "+v"(v.m), "+v"(v.mu));
        const long long t1 = __builtin_readcyclecounter();
        if (lane == 0) {
            cyc[rep] = t1 - t0;
            out[rep * 5 + 0] = bits(v.g); out[rep * 5 + 1] = bits(v.b); out[rep * 5 + 2] = bits(v.d); out[rep * 5 + 3] = bits(v.m); out[rep * 5 + 4] = bits(v.mu);
        }
    }
}

// one reduction of each form per case, all lanes' results compared: cases[c * 320 + lane * 5 + i]; bad[0] counts differing (lane, value) pairs
__global__ __launch_bounds__(64) void k_check(const double *cases, int ncases, int *bad)
{
    const int lane = threadIdx.x;
    int n = 0;
    for (int c = 0; c < ncases; c++) {
        const double *p = cases + (size_t)c * 320 + lane * 5;
        const Five v = {p[0], p[1], p[2], p[3], p[4]};
        const Five a = norms_old(lane, v), b = norms_new(lane, v);
        n += (bits(a.g) != bits(b.g)) + (bits(a.b) != bits(b.b)) + (bits(a.d) != bits(b.d)) + (bits(a.m) != bits(b.m)) + (bits(a.mu) != bits(b.mu));
        // the step bounds are in (0, 1] and never NaN
        Five w = v;
        w.g = fmin(1.0, 1.0 / fmax(1.0, fabs(v.g))); w.b = fmin(1.0, 1.0 / fmax(1.0, fabs(v.b)));
        const Five e = bounds_old(lane, w), f = bounds_new(lane, w);
        n += (bits(e.g) != bits(f.g)) + (bits(e.b) != bits(f.b));
    }
    atomicAdd(bad, n);
}

#define HIP_OK(c) do { hipError_t e_ = (c); if (e_ != hipSuccess) { std::printf("%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while (0)

int main()
{
    srand(11);
    auto rnd = [] { return rand() / (double)RAND_MAX; };
    std::vector<double> in(NIN + 8);
    for (auto &v : in) v = exp(20.0 * rnd() - 10.0);           // non-negative, as every reduced value is
    // cases of the check: random ones, zeros / inf / denormals, and a NaN in each value of each of a few lanes
    const int NC = 256 + 4 * 64;
    std::vector<double> cs((size_t)NC * 320);
    for (size_t i = 0; i < cs.size(); i++) {
        const int r = rand() % 16;
        cs[i] = (r == 0) ? 0.0 : (r == 1) ? INFINITY : (r == 2) ? 4.9e-324 * (1 + rand() % 1000) : exp(40.0 * rnd() - 20.0);
    }
    for (int c = 0; c < 32; c++) for (int i = 0; i < 320; i++) if (cs[(size_t)c * 320 + i] == INFINITY) cs[(size_t)c * 320 + i] = 1.0;   // some without inf (the sum stays finite)
    for (int i = 0; i < 4; i++) for (int l = 0; l < 64; l++) cs[(size_t)(256 + i * 64 + l) * 320 + l * 5 + i] = NAN;
    double *din, *dcs; long long *dc; unsigned long long *dout; int *dbad;
    HIP_OK(hipMalloc(&din, (NIN + 8) * 8)); HIP_OK(hipMalloc(&dcs, cs.size() * 8)); HIP_OK(hipMalloc(&dc, REPS * 8)); HIP_OK(hipMalloc(&dout, REPS * 5 * 8)); HIP_OK(hipMalloc(&dbad, 4));
    HIP_OK(hipMemcpy(din, in.data(), (NIN + 8) * 8, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dcs, cs.data(), cs.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(dbad, 0, 4));
    hipLaunchKernelGGL(k_check, dim3(1), dim3(64), 0, 0, dcs, NC, dbad);
    HIP_OK(hipDeviceSynchronize());
    int bad = -1;
    HIP_OK(hipMemcpy(&bad, dbad, 4, hipMemcpyDeviceToHost));
    std::printf("check: %d cases (256 random with 0 / inf / denormals, 256 with one NaN), mismatches %d %s\n", NC, bad, bad == 0 ? "OK" : "FAIL");

    double med[4];
    std::vector<unsigned long long> outs[4];
    const char *names[4] = {"norms today  (4 wave_nanmax + wave_sum)", "norms packed (wave_max4 + 4 ballots + wave_sum)", "bounds today  (2 wave_min)", "bounds packed (wave_min2)"};
    for (int w = 0; w < 4; w++) {
        for (int pass = 0; pass < 2; pass++) {          // the first launch warms the instruction cache
            if (w == 0) hipLaunchKernelGGL(k_time<0>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            if (w == 1) hipLaunchKernelGGL(k_time<1>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            if (w == 2) hipLaunchKernelGGL(k_time<2>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            if (w == 3) hipLaunchKernelGGL(k_time<3>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            HIP_OK(hipDeviceSynchronize());
        }
        std::vector<long long> c(REPS);
        outs[w].resize(REPS * 5);
        HIP_OK(hipMemcpy(c.data(), dc, REPS * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(outs[w].data(), dout, REPS * 5 * 8, hipMemcpyDeviceToHost));
        std::sort(c.begin(), c.end());
        med[w] = c[REPS / 2] / (double)CHAIN;
        std::printf("%-50s median %8.1f cycles per reduction set (p10 %.1f, p90 %.1f; chain of %d, %d repetitions)\n", names[w], med[w],
                    c[REPS / 10] / (double)CHAIN, c[REPS * 9 / 10] / (double)CHAIN, CHAIN, REPS);
    }
    const bool same = outs[0] == outs[1] && outs[2] == outs[3];
    std::printf("timed chains: results of today's and the packed form %s\n", same ? "equal bit for bit" : "DIFFER");
    std::printf("norms: packed / today = %.3f   bounds: packed / today = %.3f\n", med[1] / med[0], med[3] / med[2]);
    return (bad == 0 && same) ? 0 : 1;
}
