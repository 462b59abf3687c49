// qp_reduce.hpp -- several order-free reductions over the 64 lanes of a wave in ONE butterfly, for the full slot form of the interior-point
// QP (kernels_qp.hip, FULL = 1): wave_max4 (four maxima), wave_min2 (two minima).  The one-value butterfly (wave_reduce) walks six dependent
// exchange steps per value; the norms of an iteration are four values and the step bounds two, reduced one after the other -- four and two
// chains of six steps where one chain of six does.
//
// The packing.  A step of a butterfly pairs every lane with a partner; both end up with the same number, so half of the lanes do redundant
// work.  With several values a lane KEEPS half of what it holds and SENDS the other half to the partner, who keeps exactly that half:
//   step 0 (xor 1):  a lane with bit 0 clear keeps values {0, 1} and sends {2, 3}; bit 0 set: keeps {2, 3}, sends {0, 1}
//   step 1 (xor 2):  of its two values a lane with bit 1 clear keeps the lower-numbered one, bit 1 set the higher-numbered one
// so from step 1 on the lane CLASS lane & 3 decides the one value a lane reduces: class 0 -> value 0, 1 -> 2, 2 -> 1, 3 -> 3.  The steps 2..5
// must pair lanes of the same class: rotations by 4 and by 8 inside the 16-lane row (row_ror:4, row_ror:8 -- NOT the mirror inside 8 lanes
// of wave_reduce, which maps class c to 3 - c), then the row and half swaps (lane ^ 16, lane ^ 32).  After step 5 every lane of class c holds
// the reduction of its value over all 64 lanes; a quad broadcast (quad_perm of one lane of the quad) hands each of the four to every lane.
// wave_min2 is the same with two values: step 0 splits them by bit 0, the steps 1..5 (xor 2, rotations by 4 and 8, the swaps) keep bit 0.
//
// Why the bits do not move against the one-value butterflies they replace:
//   * max and min over a set WITHOUT NaNs and without zeros of both signs give the same number in any order; every value reduced here is
//     non-negative (an absolute value, a quantity clamped from below by 1, a step bound in (0, 1]), so -0 never meets +0;
//   * the step bounds amax, amax_d cannot be NaN: they are fmin(1, 1 / rmax) with rmax = fmax(1, ...), and fmax / fmin drop NaNs;
//   * the norms can be NaN, and a NaN must surface exactly as before: nanmax returned the constant NAN as soon as one operand was one, so the
//     old result was "NAN if any lane's value is a NaN, else the maximum".  Here: any_nan by one compare v != v and a ballot, the maximum by
//     plain fmax (which drops NaNs: the number it returns when there are some is discarded), and the result any_nan ? NAN : max -- the same
//     value, including the canonical NAN.
//   Sums are NOT packed: their order fixes their bits.  They keep wave_reduce.
//
// The part up to QP_REDUCE_DEVICE is plain C++17 with no HIP header: tools/probes/check_qp_reduce.cpp builds it with g++ and runs the steps on 64
// software lanes.  The device code below takes its exchanges and its selects from the same functions.
#pragma once

#ifdef __HIPCC__
#define QP_REDUCE_FN __host__ __device__ constexpr
#else
#define QP_REDUCE_FN constexpr
#endif

namespace ihm2 {

constexpr int QR_STEPS = 6;
// steps 0..3 are DPP moves (quad_perm(1,0,3,2), quad_perm(2,3,0,1), row_ror:4, row_ror:8), steps 4 and 5 v_permlane16_swap / v_permlane32_swap
QP_REDUCE_FN int qr_dpp_ctrl(int step) { return step == 0 ? 0xB1 : step == 1 ? 0x4E : step == 2 ? 0x124 : step == 3 ? 0x128 : -1; }
// the lane whose value a lane receives in a step
QP_REDUCE_FN int qr_src_lane(int step, int lane)
{
    return step == 0 ? (lane ^ 1) : step == 1 ? (lane ^ 2) : step == 2 ? ((lane & 48) | ((lane - 4) & 15)) : step == 3 ? ((lane & 48) | ((lane - 8) & 15))
         : step == 4 ? (lane ^ 16) : (lane ^ 32);
}
// quad_perm control that gives every lane of a quad the value of the quad's lane c
QP_REDUCE_FN int qr_quad_bcast(int c) { return c * 0x55; }

// ---- four values ----
// does a lane of class cls = lane & 3 hold (a partial reduction of) value v after `done` steps?  done = 0: every lane holds all four.
QP_REDUCE_FN bool qr4_owns(int done, int cls, int v)
{
    if (done <= 0) return true;
    if ((v >> 1) != (cls & 1)) return false;            // step 0: bit 0 of the lane chooses the pair {0, 1} or {2, 3}
    return done == 1 || (v & 1) == (cls >> 1);          // step 1: bit 1 chooses inside the pair; steps 2..5 keep the class
}
// the class whose lanes hold the final result of value v, and the value a class ends up with (the same map: it is its own inverse)
QP_REDUCE_FN int qr4_class_of(int v) { return ((v & 1) << 1) | (v >> 1); }
QP_REDUCE_FN int qr4_value_of(int cls) { return ((cls & 1) << 1) | (cls >> 1); }
// every exchange after step 1 stays inside a class; steps 0 and 1 flip exactly the bit they split on
QP_REDUCE_FN bool qr4_step_fits(int step, int lane)
{
    const int x = (qr_src_lane(step, lane) ^ lane) & 3;
    return step == 0 ? x == 1 : step == 1 ? x == 2 : x == 0;
}

// ---- two values ----
QP_REDUCE_FN bool qr2_owns(int done, int cls, int v) { return done <= 0 || v == (cls & 1); }
QP_REDUCE_FN int qr2_class_of(int v) { return v; }      // (of lane & 1; inside a quad the lanes v and v + 2)
QP_REDUCE_FN bool qr2_step_fits(int step, int lane)
{
    const int x = (qr_src_lane(step, lane) ^ lane) & 1;
    return step == 0 ? x == 1 : x == 0;
}

static_assert(qr4_owns(1, 0, 0) && qr4_owns(1, 0, 1) && !qr4_owns(1, 0, 2) && qr4_owns(1, 3, 2) && qr4_owns(1, 3, 3) && !qr4_owns(1, 3, 1), "step 0 splits the pairs by bit 0");
static_assert(qr4_owns(2, 0, 0) && qr4_owns(2, 1, 2) && qr4_owns(2, 2, 1) && qr4_owns(2, 3, 3) && !qr4_owns(2, 1, 1) && !qr4_owns(6, 2, 2), "one value per class from step 1 on");
static_assert(qr4_value_of(qr4_class_of(0)) == 0 && qr4_value_of(qr4_class_of(1)) == 1 && qr4_value_of(qr4_class_of(2)) == 2 && qr4_value_of(qr4_class_of(3)) == 3, "class <-> value");
static_assert(qr4_step_fits(2, 13) && qr4_step_fits(3, 2) && qr4_step_fits(2, 49) && qr_src_lane(2, 1) == 13 && qr_src_lane(3, 17) == 25, "the rotations keep lane & 3 and the row");

}  // namespace ihm2

#ifdef __HIPCC__
#define QP_REDUCE_DEVICE 1
// (dpp_mov: riccati_mfma.hpp, included before this header by the translation units that use the device part)
namespace ihm2 {

// both results of a row / half swap of a double with itself: mine and the partner's
template <int STEP>
__device__ __forceinline__ void qr_swap(double v, double &mine, double &theirs)
{
    static_assert(STEP == 4 || STEP == 5, "the swaps are the steps 4 and 5");
    const int lo = __double2loint(v), hi = __double2hiint(v);
    if constexpr (STEP == 4) {
        auto a = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        auto b = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        mine = __hiloint2double(b[0], a[0]); theirs = __hiloint2double(b[1], a[1]);
    } else {
        auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        mine = __hiloint2double(b[0], a[0]); theirs = __hiloint2double(b[1], a[1]);
    }
}
// the class-preserving steps 2..5 of one value (OP symmetric: which of the swap's results is whose does not matter)
template <typename OP>
__device__ __forceinline__ double qr_tail(double k, OP op)
{
    k = op(k, dpp_mov<qr_dpp_ctrl(2)>(k));
    k = op(k, dpp_mov<qr_dpp_ctrl(3)>(k));
    double m, t;
    qr_swap<4>(k, m, t); k = op(m, t);
    qr_swap<5>(k, m, t); return op(m, t);
}

// a, b, c, d <- their maxima over the 64 lanes, in every lane.  fmax: NaNs are dropped (see above for how the callers surface them).
__device__ __forceinline__ void wave_max4(int lane, double &a, double &b, double &c, double &d)
{
    const int cls = lane & 3;
    auto op = [](double x, double y) { return fmax(x, y); };
    // step 0: keep one pair, send the other
    const bool p = !qr4_owns(1, cls, 0);                // this lane keeps {2, 3}
    double k0 = p ? c : a, k1 = p ? d : b;
    const double s0 = p ? a : c, s1 = p ? b : d;
    k0 = op(k0, dpp_mov<qr_dpp_ctrl(0)>(s0)); k1 = op(k1, dpp_mov<qr_dpp_ctrl(0)>(s1));
    // step 1: keep one of the pair
    const bool q = !qr4_owns(2, cls, p ? 2 : 0);        // this lane keeps the higher-numbered value of its pair
    double k = q ? k1 : k0;
    const double s = q ? k0 : k1;
    k = op(k, dpp_mov<qr_dpp_ctrl(1)>(s));
    k = qr_tail(k, op);
    a = dpp_mov<qr_quad_bcast(qr4_class_of(0))>(k); b = dpp_mov<qr_quad_bcast(qr4_class_of(1))>(k);
    c = dpp_mov<qr_quad_bcast(qr4_class_of(2))>(k); d = dpp_mov<qr_quad_bcast(qr4_class_of(3))>(k);
}

// a, b <- their minima over the 64 lanes, in every lane
__device__ __forceinline__ void wave_min2(int lane, double &a, double &b)
{
    auto op = [](double x, double y) { return fmin(x, y); };
    const bool p = !qr2_owns(1, lane & 1, 0);           // this lane keeps b
    double k = p ? b : a;
    const double s = p ? a : b;
    k = op(k, dpp_mov<qr_dpp_ctrl(0)>(s));
    k = op(k, dpp_mov<qr_dpp_ctrl(1)>(k));
    k = qr_tail(k, op);
    a = dpp_mov<qr_quad_bcast(qr2_class_of(0))>(k); b = dpp_mov<qr_quad_bcast(qr2_class_of(1))>(k);
}

// is the value of any lane a NaN?  (wave-uniform: one compare, its mask is the ballot)
__device__ __forceinline__ bool wave_any(bool f) { return __ballot(f) != 0ull; }

}  // namespace ihm2
#endif
