// rk4.hpp -- the classical Runge-Kutta tableau (dpc/main.py:87-97), written once: rk4_a(st, h), rk4_w(st, h) are the stage point's offset
// a_st h and the stage's weight b_st h of stage st = 0..3.  Every RK4 loop of the library takes them from here.
// The stage loops themselves stay with their callers.  A shared rk4_step<NV, UNROLL>(x, h, f) with a stage hook f(st, X, K) was built and
// measured (NOTES.md, R8): a __forceinline__ helper is optimised on its own before it is inlined, so no caller kept its listing -- the hot
// loop's kernels gained registers or scratch, and the three stand-alone kernels that may move (k_sim_cart, k_sim_dyn10, k_init_guess) came
// out 0.2-1.6 % faster, which is outside the parent's run-to-run spread as well: a refactor leaves the speed where it is.
#pragma once

namespace ihm2 {

__host__ __device__ constexpr double rk4_a(int st, double h) { return (st == 0) ? 0.0 : ((st == 3) ? h : 0.5 * h); }
__host__ __device__ constexpr double rk4_w(int st, double h) { return (st == 0 || st == 3) ? h * (1.0 / 6.0) : h * (2.0 / 6.0); }

}  // namespace ihm2
