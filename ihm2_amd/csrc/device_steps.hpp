// device_steps.hpp -- the per-instance pieces of one control step as device functions, shared by the stand-alone kernels
// (kernels_misc.hip, kernels_linearize.hip) and the persistent per-instance loop (kernels_qp.hip, k_steps): the same source,
// so both paths produce the same bits.
//
//  * dev_prepare / dev_wrap_lap: reference ramp + warm-start shift of IHM2Controller.compute_control (python/main.py:303-322)
//    and the lap wrap; one wavefront per instance.
//  * dev_integrate_sens_fkin6 / _fkin6_lag / _dyn: RK4 x M with forward sensitivities of one shooting interval (HOT LOOP 1), one lane per
//    (instance, interval) -- three functions by what they integrate: fkin6 column-major, fkin6 with the actuator lags in closed form, the
//    dynamic models stage-major with S in LDS.  dev_linearize: the fkin6 pair on interval k of instance b.
//  * dev_sim_step: the plant step (python/main.py:476-502); four lanes per instance.  dev_sim_step_kin: the plain kinematic plant, which is
//    the fkin6 integrator on (x0, u0).
// The tableau is rk4.hpp's.  The stage loops of this file stay written out, the state-only ones too (dev_sim_step, the state stages of the
// fkin6 integrators): through a shared step function their listings move, and with call_sim_step's every k_steps that calls it (NOTES.md, R8).
#pragma once

#include "ihm2mpc_internal.h"
#include "model.hpp"
#include "rk4.hpp"

namespace ihm2 {

// yref_j = [s0 + s_target j/N, 0 x 11], yref_e = [s0 + s_target, 0 x 7];
// x_j <- x_{j+1}, u_j <- u_{j+1} (j < N-1); x_{N-1} <- x_N; u_{N-1} <- 0   (python/main.py:303-322)
// One wavefront per instance; the old rows are read into registers before anything is overwritten.
__device__ __forceinline__ void dev_prepare(int b, int lane, int N, double s_target, int mode, const double *x0,
                                            double *x, double *u, double *yref, double *yref_e)
{
    double *xb = x + (size_t)b * (N + 1) * 8, *ub = u + (size_t)b * N * 2;
    if (mode & 1) {
        const double s0 = x0[(size_t)b * 8];
        double *yb = yref + (size_t)b * N * 12, *ye = yref_e + (size_t)b * 8;
        for (int e = lane; e < N * 12; e += 64) yb[e] = (e % 12 == 0) ? s0 + s_target * (e / 12) / N : 0.0;
        if (lane < 8) ye[lane] = (lane == 0) ? s0 + s_target : 0.0;
    }
    if (!(mode & 2)) return;
    // shift: element e of stage j takes the value of stage j+1 (j < N-1); stage N-1 takes stage N
    const int nx = N * 8;                    // rows 0..N-1 are rewritten, row N stays
    for (int base = 0; base < nx; base += 64) {
        const int e = base + lane;
        const double v = (e < nx) ? xb[e + 8] : 0.0;
        __syncthreads();                     // all reads of this chunk (incl. the overlap) before its writes
        if (e < nx) xb[e] = v;
        __syncthreads();
    }
    const int nu = N * 2;
    for (int base = 0; base < nu; base += 64) {
        const int e = base + lane;
        const double v = (e < nu - 2) ? ub[e + 2] : 0.0;      // u_{N-1} <- 0
        __syncthreads();
        if (e < nu) ub[e] = v;
        __syncthreads();
    }
}

// Lap wrap for closed loops that run longer than the track tables reach (three laps, s in [-L, 2L)): an instance whose car
// has passed s = L is moved back by one lap -- x0 and the s-component of its whole iterate -- which changes nothing physically
// (the tables are periodic) and keeps s inside the table for ever.  L = -s_ref[0] of the instance's track (Track::length).
__device__ __forceinline__ void dev_wrap_lap(int b, int lane, int N, int nknots, const double *__restrict__ s_ref, const int32_t *__restrict__ track_id,
                                             double *x0, double *x)
{
    const double L = -s_ref[(size_t)track_id[b] * nknots];
    if (!(x0[(size_t)b * 8] >= L)) return;            // wave-uniform
    for (int k = lane; k <= N; k += 64) x[((size_t)b * (N + 1) + k) * 8] -= L;
    if (lane == 0) x0[(size_t)b * 8] -= L;
}

// position of entry (column c, row i) among the structurally non-zero sensitivities (column-major, 52 / 55 entries)
__host__ __device__ constexpr int s_pos(int mdl, int c, int i)
{
    int p = 0;
    for (int cc = 0; cc < c; cc++)
        for (int b = 0; b < 8; b++) p += (S_COL_MASK[mdl][cc] >> b) & 1u;
    for (int b = 0; b < i; b++) p += (S_COL_MASK[mdl][c] >> b) & 1u;
    return p;
}
__host__ __device__ constexpr int s_count(int mdl) { return s_pos(mdl, 10, 0); }

// one RK4 stage of sensitivity column COL:  dX = S + ah*dK_prev ; dK = Jx dX + Ju[:,COL] ; Sacc += wh*dK
// SL != nullptr: the sub-step's base sensitivities S live in LDS (entry-major, one word per lane: Sl[pos * 64]) instead of
// registers -- the dynamic model's forward-AD evaluation needs the registers (it spilled 868 B per lane to scratch)
// FACTORED (fkin6 only): J is the factored form of fkin6_eval, whose rows 2 and 5 are applied through rows 0 and 4 of the same stage --
// the rows are taken in ascending order, so dK[0] and dK[4] are already the new values:
//   dK[2] = dX[5] - kappa dK[0] - (kappa' s_dot) dX[0] ;  dK[5] = l_R dK[4] - dbd_dd dX[7] - (COL == 9 ? dbd_du : 0)
// with the terms the column's mask leaves out left out (22 of the 153 products of a stage over the ten columns)
template <int COL>
__device__ __forceinline__ double fkin6_factored_row(int i, const double (&J)[8][10], const double (&dX)[8], const double (&dK)[8])
{
    constexpr unsigned cm = S_COL_MASK[0][COL];
    double acc = 0.0;
    if (i == 2) {
        if ((cm >> 5) & 1u) acc = dX[5];
        acc = fma(-J[FKIN6_F_ROW2][FKIN6_F_DKS], dX[0], acc);
        acc = fma(-J[FKIN6_F_ROW2][FKIN6_F_KAP], dK[0], acc);
    } else {
        if (COL == 9) acc = -J[FKIN6_F_ROW5][FKIN6_F_DBD_DU];
        if ((cm >> 4) & 1u) acc = fma(k_lR, dK[4], acc);
        if ((cm >> 7) & 1u) acc = fma(-J[FKIN6_F_ROW5][FKIN6_F_DBD_DD], dX[7], acc);
    }
    return acc;
}

template <int MODEL, int COL, bool FACTORED = false>
__device__ __forceinline__ void sens_col_stage(const double (&J)[8][10], const double (&S)[8], const double *Sl, double (&Sacc)[8],
                                               double (&dK)[8], double ah, double wh)
{
    static_assert(!FACTORED || MODEL == IHM2MPC_MODEL_FKIN6, "the factored Jacobian is fkin6's");
    constexpr unsigned cm = S_COL_MASK[MODEL ? 1 : 0][COL];
    double dX[8];
#pragma unroll
    for (int l = 0; l < 8; l++)
        if ((cm >> l) & 1u) dX[l] = fma(ah, dK[l], Sl ? Sl[s_pos(MODEL ? 1 : 0, COL, l) * 64] : S[l]);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        if (!((cm >> i) & 1u)) continue;
        if (FACTORED && (i == 2 || i == 5)) { dK[i] = fkin6_factored_row<COL>(i, J, dX, dK); continue; }
        double acc = 0.0;
        if (COL >= 8 && ((JU_MASK[MODEL ? 1 : 0][i] >> (COL - 8)) & 1u)) acc = J[i][COL];
#pragma unroll
        for (int l = 0; l < 8; l++)
            if (((JX_MASK[MODEL ? 1 : 0][i] & cm) >> l) & 1u) acc = fma(J[i][l], dX[l], acc);
        dK[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 8; i++)
        if ((cm >> i) & 1u) Sacc[i] = fma(wh, dK[i], Sacc[i]);
}

template <int MODEL, int COL>
__device__ __forceinline__ void sens_col_copy(const double (&src)[8], double (&dst)[8])
{
    constexpr unsigned cm = S_COL_MASK[MODEL ? 1 : 0][COL];
#pragma unroll
    for (int i = 0; i < 8; i++)
        if ((cm >> i) & 1u) dst[i] = src[i];
}

// IHM2MPC_INTEG_ERK_LAG: one RK4 stage of sensitivity column COL of the six vehicle states.  The actuator rows of the stage point are
// X_a = u + (a - u) E (E: the lag's stage factor, ihm2mpc_lag_stage_factors), so their derivative is E * S_a for a state column and
// E * S_a + (1 - E) for the lag's own input column; dK and Sacc carry the rows 0..5 only (the rows 6, 7 of S follow a+ in closed form)
template <int COL, bool FACTORED = false>
__device__ __forceinline__ void sens_col_stage_lag(const double (&J)[8][10], const double (&S)[8], double (&Sacc)[8], double (&dK)[8], double ah,
                                                   double wh, double E_T, double E_d)
{
    constexpr unsigned cm = S_COL_MASK[0][COL];
    double dX[8];
#pragma unroll
    for (int l = 0; l < 6; l++)
        if ((cm >> l) & 1u) dX[l] = fma(ah, dK[l], S[l]);
    if ((cm >> 6) & 1u) dX[6] = (COL == 8) ? fma(E_T, S[6], 1.0 - E_T) : E_T * S[6];
    if ((cm >> 7) & 1u) dX[7] = (COL == 9) ? fma(E_d, S[7], 1.0 - E_d) : E_d * S[7];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        if (!((cm >> i) & 1u)) continue;
        if (FACTORED && (i == 2 || i == 5)) { dK[i] = fkin6_factored_row<COL>(i, J, dX, dK); continue; }
        double acc = 0.0;
        if (COL >= 8 && ((JU_MASK[0][i] >> (COL - 8)) & 1u)) acc = J[i][COL];
#pragma unroll
        for (int l = 0; l < 8; l++)
            if (((JX_MASK[0][i] & cm) >> l) & 1u) acc = fma(J[i][l], dX[l], acc);
        dK[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < 6; i++)
        if ((cm >> i) & 1u) Sacc[i] = fma(wh, dK[i], Sacc[i]);
}

#define FOR_ALL_COLS(OP) OP(0) OP(1) OP(2) OP(3) OP(4) OP(5) OP(6) OP(7) OP(8) OP(9)

// ---- the three sensitivity integrators: fkin6, fkin6 with closed-form lags, the dynamic models ----
// Arguments of all three: xk (8), uk (2): where to integrate from; tid: the instance's track; x_next (8): the state the defect b is taken
// against; rec: the 88-double record written at the end; xn_out (8) or nullptr (fkin6): Phi(x_k, u_k) itself.
// They share the column stages above and, as text, their first and last lines (so do k_linearize_dyn and the column kernel of
// kernels_linearize.hip).  Macros, not functions: with x, trk and S handed to a helper by reference the loop head's values come in another
// order and the registers move (k_linearize: 2408 instead of 2402 instructions), with a shared record the exit block of k_sim_step_kin
// moves in front of its loop -- and these listings are held fixed (profiles/r7/listing_compare.txt).
// SENS_LOAD_STATE declares x[8], u_T, u_d and the track segment trk (from the caller's s_ref, kappa_ref, nknots); SENS_WRITE_RECORD writes
// [A (8x8 row-major) | B (8x2) | b = Phi(x_k,u_k) - x_{k+1}] from S ([column][row], mask row MDL) and the caller's x
#define SENS_LOAD_STATE(xk, uk, tid)                                                                                     \
    double x[8];                                                                                                         \
    _Pragma("unroll") for (int i = 0; i < 8; i++) x[i] = (xk)[i];                                                        \
    const double u_T = (uk)[0];                                                                                          \
    const double u_d = (uk)[1];                                                                                          \
    TrackSeg trk;                                                                                                        \
    trk.init(s_ref + (size_t)(tid) * nknots, kappa_ref + (size_t)(tid) * nknots, nknots, x[0]);
#define SENS_WRITE_RECORD(rec, S, MDL, x_next)                                                                                          \
    _Pragma("unroll") for (int i = 0; i < 8; i++) {                                                                                     \
        _Pragma("unroll") for (int j = 0; j < 8; j++) (rec)[i * 8 + j] = ((S_COL_MASK[MDL][j] >> i) & 1u) ? S[j][i] : 0.0;              \
        _Pragma("unroll") for (int j = 0; j < 2; j++) (rec)[64 + i * 2 + j] = ((S_COL_MASK[MDL][8 + j] >> i) & 1u) ? S[8 + j][i] : 0.0; \
        (rec)[80 + i] = x[i] - (x_next)[i];                                                                                             \
    }

// fkin6, one lane: interval k of instance b.  The kinematic PLANT is this very function on (x0, u0) with xn_out: it then runs in lockstep with
// the interval lanes of the same wavefront, see k_steps.
// Per sub-step FIRST the four stage evaluations of the state (the stage points depend on the state only), their
// Jacobians kept; THEN every sensitivity column through its four stages with the column's entries in registers throughout.
// Stage-major order (all columns per stage) moved S, Sacc and dK -- 156 values that do not fit the 256 vector registers
// next to the model evaluation -- between the accumulator file and the vector registers once per STAGE: 507 of the 1617
// instructions of a stage were v_accvgpr moves; column-major order touches S once per SUB-STEP.  Same arithmetic per
// column, bit-identical results.
__device__ __forceinline__ void dev_integrate_sens_fkin6(
    const double *xk, const double *__restrict__ uk, const double *x_next, int tid, int M, double dt, int nknots, const double *__restrict__ s_ref,
    const double *__restrict__ kappa_ref, double *__restrict__ rec, double *xn_out)
{
    constexpr int MODEL = IHM2MPC_MODEL_FKIN6;
    SENS_LOAD_STATE(xk, uk, tid)
    double S[10][8];      // [column][row]; only the rows in S_COL_MASK[column] are ever touched
#pragma unroll
    for (int c = 0; c < 10; c++)
#pragma unroll
        for (int i = 0; i < 8; i++) S[c][i] = (c == i) ? 1.0 : 0.0;
    const double h = dt / M;
    for (int m = 0; m < M; m++) {
        double J4[4][8][10];
        double xacc[8], K[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { xacc[i] = x[i]; K[i] = 0.0; }
#pragma unroll
        for (int st = 0; st < 4; st++) {
            const double ah = rk4_a(st, h), wh = rk4_w(st, h);
            double X[8];
#pragma unroll
            for (int i = 0; i < 8; i++) X[i] = fma(ah, K[i], x[i]);
            fkin6_eval<FKIN6_JAC_FACTORED>(X, u_T, u_d, trk, K, J4[st]);
#pragma unroll
            for (int i = 0; i < 8; i++) xacc[i] = fma(wh, K[i], xacc[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = xacc[i];
#define SUBSTEP_COL(c)                                                                                                   \
        {                                                                                                                \
            double Sa[8], dKc[8];                                                                                        \
            _Pragma("unroll") for (int i = 0; i < 8; i++) { Sa[i] = S[c][i]; dKc[i] = 0.0; }                              \
            _Pragma("unroll") for (int st = 0; st < 4; st++)                                                             \
                sens_col_stage<MODEL, c, true>(J4[st], S[c], nullptr, Sa, dKc, rk4_a(st, h), rk4_w(st, h));              \
            sens_col_copy<MODEL, c>(Sa, S[c]);                                                                           \
        }
        FOR_ALL_COLS(SUBSTEP_COL)
#undef SUBSTEP_COL
    }
    SENS_WRITE_RECORD(rec, S, 0, x_next)
    if (xn_out) {
#pragma unroll
        for (int i = 0; i < 8; i++) xn_out[i] = x[i];
    }
}

// fkin6 with IHM2MPC_INTEG_ERK_LAG: the two actuator lags in closed form, classical RK4 on the six vehicle states with the lags' moment-fitted
// stage values (include/ihm2mpc.h); lagf: {E_0, E_1, E_2, e} of the torque lag, then of the steering lag, for h = dt / M.  The order of
// dev_integrate_sens_fkin6: the four stage evaluations of the state first, then every sensitivity column through its stages
__device__ __forceinline__ void dev_integrate_sens_fkin6_lag(
    const double *xk, const double *__restrict__ uk, const double *x_next, int tid, int M, double dt, int nknots, const double *__restrict__ s_ref,
    const double *__restrict__ kappa_ref, double *__restrict__ rec, double *xn_out, const double *lagf)
{
    SENS_LOAD_STATE(xk, uk, tid)
    double S[10][8];      // [column][row]; only the rows in S_COL_MASK[column] are ever touched
#pragma unroll
    for (int c = 0; c < 10; c++)
#pragma unroll
        for (int i = 0; i < 8; i++) S[c][i] = (c == i) ? 1.0 : 0.0;
    const double h = dt / M;
    double ET[4], ED[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { ET[i] = lagf[i]; ED[i] = lagf[4 + i]; }
    for (int m = 0; m < M; m++) {
        double J4[4][8][10];
        const double dT = x[6] - u_T, dD = x[7] - u_d;
        double xacc[8], K[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { xacc[i] = x[i]; K[i] = 0.0; }
#pragma unroll
        for (int st = 0; st < 4; st++) {
            const double ah = rk4_a(st, h), wh = rk4_w(st, h);
            const int sf = (st == 0) ? 0 : ((st == 3) ? 2 : 1);
            double X[8];
#pragma unroll
            for (int i = 0; i < 6; i++) X[i] = fma(ah, K[i], x[i]);
            X[6] = fma(dT, ET[sf], u_T);
            X[7] = fma(dD, ED[sf], u_d);
            fkin6_eval<FKIN6_JAC_FACTORED>(X, u_T, u_d, trk, K, J4[st]);
#pragma unroll
            for (int i = 0; i < 6; i++) xacc[i] = fma(wh, K[i], xacc[i]);
        }
#pragma unroll
        for (int i = 0; i < 6; i++) x[i] = xacc[i];
        x[6] = fma(dT, ET[3], u_T);
        x[7] = fma(dD, ED[3], u_d);
#define SUBSTEP_COL_LAG(c)                                                                                               \
        {                                                                                                                \
            constexpr unsigned cm = S_COL_MASK[0][c];                                                                    \
            double Sa[8], dKc[8];                                                                                        \
            _Pragma("unroll") for (int i = 0; i < 8; i++) { Sa[i] = S[c][i]; dKc[i] = 0.0; }                              \
            _Pragma("unroll") for (int st = 0; st < 4; st++) {                                                           \
                const int sf = (st == 0) ? 0 : ((st == 3) ? 2 : 1);                                                      \
                sens_col_stage_lag<c, true>(J4[st], S[c], Sa, dKc, rk4_a(st, h), rk4_w(st, h), ET[sf], ED[sf]);          \
            }                                                                                                            \
            _Pragma("unroll") for (int i = 0; i < 6; i++)                                                                \
                if ((cm >> i) & 1u) S[c][i] = Sa[i];                                                                     \
            if ((cm >> 6) & 1u) S[c][6] = (c == 8) ? fma(ET[3], S[c][6], 1.0 - ET[3]) : ET[3] * S[c][6];                  \
            if ((cm >> 7) & 1u) S[c][7] = (c == 9) ? fma(ED[3], S[c][7], 1.0 - ED[3]) : ED[3] * S[c][7];                  \
        }
        FOR_ALL_COLS(SUBSTEP_COL_LAG)
#undef SUBSTEP_COL_LAG
    }
    SENS_WRITE_RECORD(rec, S, 0, x_next)
    if (xn_out) {
#pragma unroll
        for (int i = 0; i < 8; i++) xn_out[i] = x[i];
    }
}

// The dynamic models (fdyn6, fdyn6u), one lane: interval k of instance b -- the integrator of the persistent loop (kernels_qp.hip:
// call_integrate_dyn).  Stage-major: the model and its Jacobian are evaluated once per stage and every column goes through that stage.
// The sub-step's base sensitivities live in LDS (Sl: this lane's column of the copy, see sens_col_stage) and the running sums Sacc in registers;
// at the end of a sub-step Sacc is the new base.  k_linearize_dyn (kernels_linearize.hip) is a second text of this function, see there.
template <int MODEL>
__device__ __forceinline__ void dev_integrate_sens_dyn(
    const double *xk, const double *__restrict__ uk, const double *x_next, int tid, int M, double dt, int nknots, const double *__restrict__ s_ref,
    const double *__restrict__ kappa_ref, double *__restrict__ rec, double *__restrict__ Sl)
{
    static_assert(MODEL == IHM2MPC_MODEL_FDYN6 || MODEL == IHM2MPC_MODEL_FDYN6U, "fkin6 has integrators of its own");
    SENS_LOAD_STATE(xk, uk, tid)

    // S, Sacc, dK: [column][row]; only rows in S_COL_MASK[column] are ever touched (S itself stays the identity: the base is read from Sl)
    double S[10][8], Sacc[10][8], dK[10][8];
#pragma unroll
    for (int c = 0; c < 10; c++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            S[c][i] = (c == i) ? 1.0 : 0.0; dK[c][i] = 0.0;
            Sacc[c][i] = S[c][i];
            if ((S_COL_MASK[1][c] >> i) & 1u) Sl[s_pos(1, c, i) * 64] = S[c][i];
        }

    const double h = dt / M;
    for (int m = 0; m < M; m++) {
        double xacc[8], K[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { xacc[i] = x[i]; K[i] = 0.0; }
#pragma unroll 1
        for (int st = 0; st < 4; st++) {
            const double ah = rk4_a(st, h), wh = rk4_w(st, h);
            double X[8], J[8][10];
#pragma unroll
            for (int i = 0; i < 8; i++) X[i] = fma(ah, K[i], x[i]);
            fdyn6_eval<true, MODEL == IHM2MPC_MODEL_FDYN6U>(X, u_T, u_d, trk, K, J);
#pragma unroll
            for (int i = 0; i < 8; i++) xacc[i] = fma(wh, K[i], xacc[i]);
#define STAGE_COL(c) sens_col_stage<MODEL, c>(J, S[c], Sl, Sacc[c], dK[c], ah, wh);
            FOR_ALL_COLS(STAGE_COL)
#undef STAGE_COL
        }
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = xacc[i];
#pragma unroll
        for (int c = 0; c < 10; c++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                if ((S_COL_MASK[1][c] >> i) & 1u) Sl[s_pos(1, c, i) * 64] = Sacc[c][i];
    }

    SENS_WRITE_RECORD(rec, Sacc, 1, x_next)
}

// fkin6, one lane: interval k of instance b
template <int LAG = 0>
__device__ __forceinline__ void dev_linearize(
    int b, int k, int N, int M, double dt, int nknots, const double *__restrict__ s_ref,
    const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id, const double *xs,
    const double *us, double *lin, const double *lagf = nullptr)
{
    const double *xk = xs + ((size_t)b * (N + 1) + k) * 8;
    const double *uk = us + ((size_t)b * N + k) * 2;
    const int tid = track_id[b];
    double *rec = lin + ((size_t)b * N + k) * LIN_REC;
    if constexpr (LAG != 0) dev_integrate_sens_fkin6_lag(xk, uk, xk + 8, tid, M, dt, nknots, s_ref, kappa_ref, rec, nullptr, lagf);
    else dev_integrate_sens_fkin6(xk, uk, xk + 8, tid, M, dt, nknots, s_ref, kappa_ref, rec, nullptr);
}

// plant / rollout step: x_next = RK4 x M over dt; model -1 (-2: with fdyn6u) = kin/dyn switch of
// python/main.py:482-489 (v^2 sin(beta) / l_R <= 3 -> kinematic, else dynamic).
// The plain kinematic plant (model 0, the OCP's own model) is NOT handled here but by dev_sim_step_kin below.
// FOUR lanes: instance b on the lanes q = 0..3 of a quad, all active -- every lane carries the state, the dynamic model's wheels are spread over
// the lanes (fdyn6_eval_quad: bit-identical to the one-lane evaluation), lane q = 0 stores the result
__device__ __forceinline__ void dev_sim_step(int b, int q, int model, int M, double dt, int nknots,
                                             const double *__restrict__ s_ref, const double *__restrict__ kappa_ref,
                                             const int32_t *__restrict__ track_id, const double *xs,
                                             const double *us, double *xn, const int32_t *active)
{
    if (active && !active[b]) {          // a frozen instance keeps its state (closed loops: failed or finished cars)
        if (xn != xs && q == 0) for (int i = 0; i < 8; i++) xn[(size_t)b * 8 + i] = xs[(size_t)b * 8 + i];
        return;
    }
    double x[8];
#pragma unroll
    for (int i = 0; i < 8; i++) x[i] = xs[(size_t)b * 8 + i];
    const double u_T = us[(size_t)b * 2], u_d = us[(size_t)b * 2 + 1];
    const int tid = track_id[b];
    TrackSeg trk;
    trk.init(s_ref + (size_t)tid * nknots, kappa_ref + (size_t)tid * nknots, nknots, x[0]);
    int mdl = model;
    if (model < 0) {
        const double beta = atan(k_rwd * tan(x[7]));
        const double v2 = x[3] * x[3] + x[4] * x[4];
        mdl = (v2 * sin(beta) / k_lR <= 3.0) ? IHM2MPC_MODEL_FKIN6 : (model == -2 ? IHM2MPC_MODEL_FDYN6U : IHM2MPC_MODEL_FDYN6);
    }
    const double h = dt / M;
    double J[8][10];
    for (int m = 0; m < M; m++) {
        double xacc[8], K[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { xacc[i] = x[i]; K[i] = 0.0; }
#pragma unroll 1
        for (int st = 0; st < 4; st++) {
            const double ah = rk4_a(st, h), wh = rk4_w(st, h);
            double X[8];
#pragma unroll
            for (int i = 0; i < 8; i++) X[i] = fma(ah, K[i], x[i]);
            if (mdl == IHM2MPC_MODEL_FKIN6) fkin6_eval<FKIN6_JAC_NONE>(X, u_T, u_d, trk, K, J);
            else if (mdl == IHM2MPC_MODEL_FDYN6U) fdyn6_eval_quad<true>(q, X, u_T, u_d, trk, K);
            else fdyn6_eval_quad<false>(q, X, u_T, u_d, trk, K);
#pragma unroll
            for (int i = 0; i < 8; i++) xacc[i] = fma(wh, K[i], xacc[i]);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = xacc[i];
    }
    if (q == 0)
#pragma unroll
        for (int i = 0; i < 8; i++) xn[(size_t)b * 8 + i] = x[i];
}


// The plain kinematic plant (model 0) is dev_integrate_sens_fkin6 on (x, u): the same arithmetic as a shooting interval, so that the
// persistent loop can run it on the spare lane of the linearisation for free (k_steps); its record goes to spare_rec
// (88 doubles per instance, never read).
template <int LAG = 0>
__device__ __forceinline__ void dev_sim_step_kin(int b, int M, double dt, int nknots, const double *__restrict__ s_ref,
                                                 const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id,
                                                 const double *xs, const double *us, double *xn, const int32_t *active, double *spare_rec,
                                                 const double *lagf = nullptr)
{
    if (active && !active[b]) {
        if (xn != xs) for (int i = 0; i < 8; i++) xn[(size_t)b * 8 + i] = xs[(size_t)b * 8 + i];
        return;
    }
    if constexpr (LAG != 0)
        dev_integrate_sens_fkin6_lag(xs + (size_t)b * 8, us + (size_t)b * 2, xs + (size_t)b * 8, track_id[b], M, dt, nknots, s_ref, kappa_ref,
                                     spare_rec + (size_t)b * LIN_REC, xn + (size_t)b * 8, lagf);
    else
        dev_integrate_sens_fkin6(xs + (size_t)b * 8, us + (size_t)b * 2, xs + (size_t)b * 8, track_id[b], M, dt, nknots, s_ref, kappa_ref,
                                 spare_rec + (size_t)b * LIN_REC, xn + (size_t)b * 8);
}

}  // namespace ihm2
