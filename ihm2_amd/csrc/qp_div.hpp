// qp_div.hpp -- K fp64 quotients side by side (the full slot form of the QP, kernels_qp.hip; tools/probes/div_proto.hip checks and times it).
//
// An fp64 `/` is a chain of eleven dependent instructions: v_div_scale of the denominator, v_rcp_f64, two Newton steps on the reciprocal
// (four FMAs), v_div_scale of the numerator, a multiplication, a residual FMA, v_div_fmas, v_div_fixup.  In a kernel whose registers are
// scarce the compiler lays the quotients of a slot loop one behind the other, and a wave with a SIMD to itself waits out every link of every
// chain.  div_batch writes the same sequence out with the builtins and advances the K chains one step at a time, so that a step's K
// instructions are independent and only eleven latencies are waited for per batch.
//
// Each result is num / den bit for bit, for all operands: the same instructions on the same values, in the operand order the back end
// gives them (LLVM, SIISelLowering: LowerFDIV64) -- the first v_div_scale scales the DENOMINATOR, the second the NUMERATOR, and its
// condition code is the one v_div_fmas takes; v_div_fixup gets (quotient, denominator, numerator) and restores zeros, infinities, NaNs
// with their payloads and denormal results.  The multiplications are not contracted into their neighbours: every FMA is written as one.
#pragma once

namespace ihm2 {

// FENCE: a scheduling fence between the steps keeps the K instructions of a step together (without it the scheduler is free to re-serialise
// the chains where registers are short); 0 leaves the order to the compiler.
template <int K, int FENCE = 1>
__device__ __forceinline__ void div_batch(const double (&num)[K], const double (&den)[K], double (&out)[K])
{
#define QP_DIV_STEP(stmt) do { _Pragma("unroll") for (int i = 0; i < K; i++) { stmt; } if (FENCE) __builtin_amdgcn_sched_barrier(0); } while (0)
    double s0[K], s1[K], r[K], e[K], m[K];
    bool cc[K];
    if (FENCE) __builtin_amdgcn_sched_barrier(0);
    QP_DIV_STEP(bool unused; s0[i] = __builtin_amdgcn_div_scale(num[i], den[i], false, &unused));     // the denominator, scaled
    QP_DIV_STEP(r[i] = __builtin_amdgcn_rcp(s0[i]));
    QP_DIV_STEP(e[i] = __builtin_fma(-s0[i], r[i], 1.0));
    QP_DIV_STEP(r[i] = __builtin_fma(r[i], e[i], r[i]));
    QP_DIV_STEP(e[i] = __builtin_fma(-s0[i], r[i], 1.0));
    QP_DIV_STEP(s1[i] = __builtin_amdgcn_div_scale(num[i], den[i], true, &cc[i]));                     // the numerator, scaled; its flag goes to div_fmas
    QP_DIV_STEP(r[i] = __builtin_fma(r[i], e[i], r[i]));
    QP_DIV_STEP(m[i] = __dmul_rn(s1[i], r[i]));
    QP_DIV_STEP(e[i] = __builtin_fma(-s0[i], m[i], s1[i]));
    QP_DIV_STEP(m[i] = __builtin_amdgcn_div_fmas(e[i], r[i], m[i], cc[i]));
    QP_DIV_STEP(out[i] = __builtin_amdgcn_div_fixup(m[i], den[i], num[i]));
#undef QP_DIV_STEP
}

// M quotients in batches of W, the last one shorter: the sets of a slot phase (two sides of every slot of a lane)
template <int W, int M, int FENCE = 1>
__device__ __forceinline__ void div_sets(const double (&num)[M], const double (&den)[M], double (&out)[M])
{
    static_assert(W >= 1 && W <= M, "a batch width between 1 and the size of the set");
#pragma unroll
    for (int at = 0; at + W <= M; at += W) {
        double n[W], d[W], q[W];
#pragma unroll
        for (int i = 0; i < W; i++) { n[i] = num[at + i]; d[i] = den[at + i]; }
        div_batch<W, FENCE>(n, d, q);
#pragma unroll
        for (int i = 0; i < W; i++) out[at + i] = q[i];
    }
    if constexpr (M % W != 0) {
        constexpr int R = M % W, at = M - R;
        double n[R], d[R], q[R];
#pragma unroll
        for (int i = 0; i < R; i++) { n[i] = num[at + i]; d[i] = den[at + i]; }
        div_batch<R, FENCE>(n, d, q);
#pragma unroll
        for (int i = 0; i < R; i++) out[at + i] = q[i];
    }
}

}  // namespace ihm2
