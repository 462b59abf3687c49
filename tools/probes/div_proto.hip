// Stand-alone check + timing of div_batch<K> (ihm2_amd/csrc/qp_div.hpp) against the compiler's fp64 `/` on the same operands: one wave.
//   div_proto check   every operand pair through `/` and through div_batch<K> for K = 1, 2, 3, 5, 10, results compared bit for bit:
//                     about 10^6 random sign / exponent / mantissa pairs; 1.0 / x over the whole exponent range (denormal x included);
//                     all pairs of a table of special values (+-0, +-inf, quiet and signalling NaNs with payloads, denormals, the
//                     extremes of the normal range, numbers next to 1); denormal quotients; quotients that overflow.
//                     One line per width, then "all checks passed".
//   div_proto time    cycle-counter stamps round TEN quotients: as `/` in one dependent chain (what a slot loop of the QP kernel looks like when
//                     its quotients come out one behind the other), and as batches of width 2, 3, 5, 10, each batch's numerators fed by the
//                     batch before.  Operands from memory; median of REPS repetitions.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=on -I ihm2_amd/csrc tools/probes/div_proto.hip -o div_proto
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>
#include "qp_div.hpp"
using namespace ihm2;

constexpr int REPS = 4096, NQ = 10, NIN = 1 << 14;
constexpr int GROUP = 64 * 30;      // pairs per round of the wave for every width: 30 = lcm(1, 2, 3, 5, 10)

__device__ __forceinline__ unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }

// The reference: `/` as the compiler emits it, in a kernel of its own.  (In one kernel with div_batch the instruction selector finds the two
// sequences node for node the same, keeps one, and folds the comparison away -- which says that the sequence is the back end's, and leaves
// nothing to run.)
__global__ __launch_bounds__(64) void k_ref(const double *num, const double *den, int n, double *want)
{
    for (int i = threadIdx.x; i < n; i += 64) want[i] = num[i] / den[i];
}

// res[0]: mismatching pairs, res[1]: index of the first one (n if none)
template <int K>
__global__ __launch_bounds__(64) void k_check(const double *num, const double *den, const double *ref, int n, unsigned long long *res)
{
    const int lane = threadIdx.x;
    unsigned long long bad = 0, first = (unsigned long long)n;
    for (int base = 0; base + 64 * K <= n; base += 64 * K) {
        const int at = base + lane * K;
        double a[K], b[K], q[K];
#pragma unroll
        for (int i = 0; i < K; i++) { a[i] = num[at + i]; b[i] = den[at + i]; }
        div_batch<K>(a, b, q);
#pragma unroll
        for (int i = 0; i < K; i++) {
            const double want = ref[at + i];
            if (bits(q[i]) != bits(want)) { bad++; first = min(first, (unsigned long long)(at + i)); }
        }
    }
    atomicAdd(&res[0], bad);
    atomicMin(&res[1], first);
}

// W = 0: `/`, one dependent chain of NQ quotients; W > 0: batches of W (the last one shorter), chained batch to batch
template <int W, int K>
__device__ __forceinline__ void timed_batch(const double *a, const double *b, int at, double &carry)
{
    double n[K], d[K], q[K];
#pragma unroll
    for (int i = 0; i < K; i++) { n[i] = fma(carry, 0x1p-40, a[at + i]); d[i] = b[at + i]; }
    div_batch<K>(n, d, q);
    carry = q[K - 1];
}
template <int W>
__global__ __launch_bounds__(64) void k_time(const double *in, long long *cyc, unsigned long long *out)
{
    const int lane = threadIdx.x;
    for (int rep = 0; rep < REPS; rep++) {
        const double *p = in + ((size_t)(rep * 64 * 2 * NQ + lane * 2 * NQ) & (NIN - 1));
        double a[NQ], b[NQ];
#pragma unroll
        for (int i = 0; i < NQ; i++) { a[i] = p[i]; b[i] = p[NQ + i]; }
        double carry = 0.0;
        const long long t0 = __builtin_readcyclecounter();
        // every operand passes through a statement that has the stamp as an input: no quotient starts ahead of it
        asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]),
                          "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]), "+v"(b[8]), "+v"(b[9]) : "s"(t0));
        static_assert(NQ == 10, "the statement above names the operands one by one");
        if constexpr (W == 0) {
#pragma unroll
            for (int i = 0; i < NQ; i++) carry = fma(carry, 0x1p-40, a[i]) / b[i];
        } else {
#pragma unroll
            for (int at = 0; at + W <= NQ; at += W) timed_batch<W, W>(a, b, at, carry);
            if constexpr (NQ % W != 0) timed_batch<W, NQ % W>(a, b, NQ - NQ % W, carry);
        }
        asm volatile("" : "+v"(carry));
        const long long t1 = __builtin_readcyclecounter();
        if (lane == 0) { cyc[rep] = t1 - t0; out[rep] = bits(carry); }
    }
}

#define HIP_OK(c) do { hipError_t e_ = (c); if (e_ != hipSuccess) { std::printf("%s: %s\n", #c, hipGetErrorString(e_)); return 1; } } while (0)

static double from_bits(uint64_t u) { double v; std::memcpy(&v, &u, 8); return v; }

static void operands(std::vector<double> &num, std::vector<double> &den)
{
    std::mt19937_64 rng(20240621);
    auto mant = [&] { return rng() & ((1ull << 52) - 1); };
    auto make = [&](int sign, int expo, uint64_t m) { return from_bits(((uint64_t)sign << 63) | ((uint64_t)expo << 52) | m); };
    auto push = [&](double a, double b) { num.push_back(a); den.push_back(b); };
    // random sign, exponent (0 = denormal .. 2046) and mantissa
    for (int i = 0; i < 1000000; i++) push(make(rng() & 1, rng() % 2047, mant()), make(rng() & 1, rng() % 2047, mant()));
    // 1.0 / x over the whole exponent range
    for (int e = 0; e < 2047; e++)
        for (int j = 0; j < 8; j++) push(1.0, make(j & 1, e, j < 2 ? 0 : j < 4 ? (1ull << 52) - 1 : mant()));
    // the special values, every pair
    std::vector<double> sp = {0.0, -0.0, INFINITY, -INFINITY, 1.0, -1.0, 2.0, 0.5, 3.0, 1.0 / 3.0, from_bits(0x3ff0000000000001ull), from_bits(0x3fefffffffffffffull),
                              from_bits(0x7ff8000000000000ull), from_bits(0xfff8000000000000ull), from_bits(0x7ff8000000005a5aull), from_bits(0xfff80000deadbeefull),
                              from_bits(0x7ff0000000000001ull), from_bits(0xfff4000000000123ull),           // signalling
                              from_bits(1), from_bits(0x8000000000000001ull), from_bits(0x000fffffffffffffull), from_bits(0x800fffffffffffffull), from_bits(0x0008000000000000ull),
                              from_bits(0x0000000012345678ull), from_bits(0x0010000000000000ull), from_bits(0x8010000000000000ull), from_bits(0x0010000000000001ull),
                              from_bits(0x7fefffffffffffffull), from_bits(0xffefffffffffffffull), from_bits(0x7fe0000000000000ull), 0x1p-1022, 0x1p1023, 0x1p-537, 0x1p537, 0x1p512, 0x1p-512};
    for (double a : sp) for (double b : sp) push(a, b);
    // denormal quotients (and the round to zero / to the smallest normal on either side of them)
    for (int i = 0; i < 60000; i++) {
        const int ea = 1 + rng() % 1000, eb = std::min(2046, ea + 1020 + (int)(rng() % 60));      // biased exponent of the quotient about 3 .. -57
        push(make(rng() & 1, ea, mant()), make(rng() & 1, eb, mant()));
    }
    for (int i = 0; i < 20000; i++) push(make(rng() & 1, 0, mant()), make(rng() & 1, 1000 + rng() % 100, mant()));       // a denormal numerator
    // quotients that overflow, and those just below
    for (int i = 0; i < 60000; i++) {
        const int eb = rng() % 1024, ea = std::min(2046, eb + 1020 + (int)(rng() % 8));
        push(make(rng() & 1, ea, mant()), make(rng() & 1, eb, mant()));
    }
    while (num.size() % GROUP) push(1.0, 3.0);
}

static int check()
{
    std::vector<double> num, den;
    operands(num, den);
    const int n = (int)num.size();
    double *dn, *dd, *dw; unsigned long long *dres;
    HIP_OK(hipMalloc(&dn, (size_t)n * 8)); HIP_OK(hipMalloc(&dd, (size_t)n * 8)); HIP_OK(hipMalloc(&dw, (size_t)n * 8)); HIP_OK(hipMalloc(&dres, 16));
    HIP_OK(hipMemcpy(dn, num.data(), (size_t)n * 8, hipMemcpyHostToDevice)); HIP_OK(hipMemcpy(dd, den.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_ref, dim3(1), dim3(64), 0, 0, dn, dd, n, dw);
    HIP_OK(hipDeviceSynchronize());
    int fails = 0;
    const int widths[5] = {1, 2, 3, 5, 10};
    for (int w : widths) {
        const unsigned long long init[2] = {0, (unsigned long long)n};
        HIP_OK(hipMemcpy(dres, init, 16, hipMemcpyHostToDevice));
        if (w == 1) hipLaunchKernelGGL(k_check<1>, dim3(1), dim3(64), 0, 0, dn, dd, dw, n, dres);
        if (w == 2) hipLaunchKernelGGL(k_check<2>, dim3(1), dim3(64), 0, 0, dn, dd, dw, n, dres);
        if (w == 3) hipLaunchKernelGGL(k_check<3>, dim3(1), dim3(64), 0, 0, dn, dd, dw, n, dres);
        if (w == 5) hipLaunchKernelGGL(k_check<5>, dim3(1), dim3(64), 0, 0, dn, dd, dw, n, dres);
        if (w == 10) hipLaunchKernelGGL(k_check<10>, dim3(1), dim3(64), 0, 0, dn, dd, dw, n, dres);
        HIP_OK(hipDeviceSynchronize());
        unsigned long long res[2];
        HIP_OK(hipMemcpy(res, dres, 16, hipMemcpyDeviceToHost));
        std::printf("width %d: %d pairs, %llu differ from /", w, n, res[0]);
        if (res[0]) { std::printf(" (first: %a / %a)", num[res[1]], den[res[1]]); fails++; }
        std::printf("\n");
    }
    if (fails) return 1;
    std::printf("all checks passed\n");
    return 0;
}

static int time_them()
{
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::vector<double> in(NIN + 64);
    for (auto &v : in) v = std::exp(20.0 * uni(rng) - 10.0);
    double *din; long long *dc; unsigned long long *dout;
    HIP_OK(hipMalloc(&din, in.size() * 8)); HIP_OK(hipMalloc(&dc, REPS * 8)); HIP_OK(hipMalloc(&dout, REPS * 8));
    HIP_OK(hipMemcpy(din, in.data(), in.size() * 8, hipMemcpyHostToDevice));
    const int widths[5] = {0, 2, 3, 5, 10};
    std::vector<unsigned long long> outs[5];
    double med[5];
    for (int w = 0; w < 5; w++) {
        for (int pass = 0; pass < 2; pass++) {          // the first launch warms the instruction cache
            if (w == 0) hipLaunchKernelGGL(k_time<0>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            if (w == 1) hipLaunchKernelGGL(k_time<2>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            if (w == 2) hipLaunchKernelGGL(k_time<3>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            if (w == 3) hipLaunchKernelGGL(k_time<5>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            if (w == 4) hipLaunchKernelGGL(k_time<10>, dim3(1), dim3(64), 0, 0, din, dc, dout);
            HIP_OK(hipDeviceSynchronize());
        }
        std::vector<long long> c(REPS);
        outs[w].resize(REPS);
        HIP_OK(hipMemcpy(c.data(), dc, REPS * 8, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(outs[w].data(), dout, REPS * 8, hipMemcpyDeviceToHost));
        std::sort(c.begin(), c.end());
        med[w] = (double)c[REPS / 2];
        if (w == 0) std::printf("ten quotients as / in one chain      median %7.1f cycles (p10 %lld, p90 %lld; %d repetitions)\n", med[w], c[REPS / 10], c[REPS * 9 / 10], REPS);
        else std::printf("ten quotients in batches of width %2d  median %7.1f cycles (p10 %lld, p90 %lld)  x %.2f\n", widths[w], med[w], c[REPS / 10], c[REPS * 9 / 10], med[w] / med[0]);
    }
    return 0;       // (the forms differ in which quotient feeds which numerator: the bits are `check`'s business)
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc == 2 && !std::strcmp(argv[1], "time")) return time_them();
    std::printf("usage: div_proto check | time\n");
    return 2;
}
