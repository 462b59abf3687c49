// kernels_linearize.hip -- HOT LOOP 1 of the RTI step: for every (instance b, shooting interval k)
// integrate the model over dt with M classical RK4 sub-steps and propagate the forward sensitivities
// S = d x_m / d (x_k, u_k) through the same stages (exact derivative of the discrete map).
//
// Replaces what acados' ERK integrator does inside AcadosOcpSolver.solve() for the reference
// (python/main.py:325; options old/generate.py:23-25 with sim_method_num_steps = M).
// RK4 tableau as dpc/main.py:87-97 (rk4.hpp).
// Kernels: k_linearize<LAG> (fkin6; LAG = 1, IHM2MPC_INTEG_ERK_LAG: the same tableau on the six vehicle states, the two actuator lags in
// closed form, include/ihm2mpc.h), k_linearize_cols (fkin6, small batches), k_linearize_dyn<MODEL> (fdyn6, fdyn6u); the plants k_sim_step
// and k_sim_step_kin<LAG>.  The integrators themselves are device_steps.hpp's (dev_integrate_sens_fkin6, _fkin6_lag, _dyn), shared with the
// persistent loop; k_linearize_dyn and k_linearize_cols carry their own text, see there.
//
// Mapping: one lane per (b, k) pair, k fastest (instance-major arrays): a wavefront reads 64
// consecutive 64-byte state rows (4 KB contiguous) and writes 64 consecutive 704-byte records.
// Sensitivities are held column-wise in registers; only the structurally non-zero entries of the
// 8x10 matrix are stored (52 for fkin6, 55 for fdyn6) and only the non-zeros of the model Jacobian (31 / 37) are multiplied
// (model.hpp: JX_MASK / S_COL_MASK).  Algorithmic traffic per pair: read 10 + 8 doubles, write 88.
#include "ihm2mpc_internal.h"     // (with qp_select.hpp: select_linearize, select_sim, and note_lin, note_sim for the launch record)
#include "model.hpp"
#include "device_steps.hpp"

using namespace ihm2;

namespace {

// LAG = 1 (IHM2MPC_INTEG_ERK_LAG): the kernel takes the lags' stage factors as one more argument (LF = LagFac); with LAG = 0 the pack is
// empty and the kernel's arguments are what they were
__device__ __forceinline__ const double *lag_ptr() { return nullptr; }
__device__ __forceinline__ const double *lag_ptr(const LagFac &l) { return l.f; }

template <int LAG = 0, typename... LF>
__global__ __launch_bounds__(64) void k_linearize(
    int B, int N, int M, double dt, int nknots, const double *__restrict__ s_ref,
    const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id, const double *__restrict__ xs,
    const double *__restrict__ us, double *__restrict__ lin, LF... lf)
{
    const long t = (long)blockIdx.x * 64 + threadIdx.x;
    const int b = (int)(t / N);
    const int k = (int)(t % N);
    if (b >= B) return;
    dev_linearize<LAG>(b, k, N, M, dt, nknots, s_ref, kappa_ref, track_id, xs, us, lin, lag_ptr(lf...));
}

// ---- small batches (the single real-time controller, B = 1): one sensitivity COLUMN per lane ----
// With few instances the device is empty and the latency of a solve is what counts.  Here wave c of an interval block
// propagates only column c of S (10 waves per 64 intervals); every lane re-evaluates the model and its Jacobian (10x redundant,
// on otherwise idle SIMDs) but carries 8 instead of 52 sensitivity entries: 0.11 ms instead of 0.25 ms per linearisation.
// The formulas per column are those of dev_integrate_sens_fkin6, but the compiler shares different subexpressions when only one
// column is needed, so the records agree with k_linearize's to rounding (1e-15 relative), not bit for bit; it is therefore used
// for up to 128 intervals only (B <= 3 at N = 40), where nothing is compared bit-wise with the batch path.
template <int COL>
__device__ __forceinline__ void dev_integrate_col_fkin6(const double *xk, const double *uk, int tid, int M, double dt, int nknots,
                                                       const double *__restrict__ s_ref, const double *__restrict__ kappa_ref, double *rec)
{
    constexpr int MODEL = IHM2MPC_MODEL_FKIN6;
    SENS_LOAD_STATE(xk, uk, tid)
    double S[8], Sacc[8], dK[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { S[i] = (COL == i) ? 1.0 : 0.0; dK[i] = 0.0; Sacc[i] = 0.0; }
    const double h = dt / M;
    for (int m = 0; m < M; m++) {
        double xacc[8], K[8];
#pragma unroll
        for (int i = 0; i < 8; i++) { xacc[i] = x[i]; K[i] = 0.0; }
        sens_col_copy<MODEL, COL>(S, Sacc);
#pragma unroll 1
        for (int st = 0; st < 4; st++) {
            const double ah = rk4_a(st, h), wh = rk4_w(st, h);
            double X[8], J[8][10];
#pragma unroll
            for (int i = 0; i < 8; i++) X[i] = fma(ah, K[i], x[i]);
            fkin6_eval<FKIN6_JAC_FACTORED>(X, u_T, u_d, trk, K, J);
#pragma unroll
            for (int i = 0; i < 8; i++) xacc[i] = fma(wh, K[i], xacc[i]);
            sens_col_stage<MODEL, COL, true>(J, S, nullptr, Sacc, dK, ah, wh);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = xacc[i];
        sens_col_copy<MODEL, COL>(Sacc, S);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const double v = ((S_COL_MASK[0][COL] >> i) & 1u) ? S[i] : 0.0;
        if (COL < 8) rec[i * 8 + COL] = v; else rec[64 + i * 2 + (COL - 8)] = v;
        if (COL == 0) rec[80 + i] = x[i] - xk[8 + i];
    }
}

__global__ __launch_bounds__(64) void k_linearize_cols(int B, int N, int M, double dt, int nknots, const double *__restrict__ s_ref,
                                                       const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id,
                                                       const double *__restrict__ xs, const double *__restrict__ us, double *__restrict__ lin)
{
    const long t = (long)blockIdx.x * 64 + threadIdx.x;
    const int b = (int)(t / N), k = (int)(t % N);
    if (b >= B) return;
    const double *xk = xs + ((size_t)b * (N + 1) + k) * 8, *uk = us + ((size_t)b * N + k) * 2;
    double *rec = lin + ((size_t)b * N + k) * LIN_REC;
    const int tid = track_id[b];
    switch (blockIdx.y) {       // block-uniform: one column per wavefront
#define COL_CASE(c) case c: dev_integrate_col_fkin6<c>(xk, uk, tid, M, dt, nknots, s_ref, kappa_ref, rec); break;
    FOR_ALL_COLS(COL_CASE)
#undef COL_CASE
    }
}

// columns of the dynamic models' stage derivatives dK parked in LDS between the stages (k_linearize_dyn), and their positions there
#ifndef DK_PARK_FROM
#define DK_PARK_FROM 7
#endif
__host__ __device__ constexpr int dk_pos(int c, int i)
{
    int p = 0;
    for (int cc = DK_PARK_FROM; cc < 10; cc++)
        for (int ii = 0; ii < 8; ii++) {
            if (cc == c && ii == i) return p;
            if ((S_COL_MASK[1][cc] >> ii) & 1u) p++;
        }
    return p;
}
__host__ __device__ constexpr int dk_count() { return dk_pos(10, 0); }

// The dynamic models keep the integrator in the kernel itself: the text of dev_integrate_sens_dyn (device_steps.hpp), extended by the parked dK
// and the fences of fdyn6_eval.  The two must give the same bits (tests/test_gpu_closed_loop.py: the loop against per-step launches).
// Tried twice as one function.  As a plain shared device function the compiler forwarded the LDS-parked base sensitivities through registers
// (+45 spill stores, +14 %).  As one __forceinline__ template dev_integrate_sens_dyn<MODEL, DK_FROM, FENCE> (the loop: DK_FROM = 10, no fences)
// call_integrate_dyn kept its listing and this kernel did not: fdyn6u 3002 -> 3021 instructions and 256 -> 272 B scratch per lane, fdyn6
// 3016 -> 3025 and 272 -> 288 B (256 VGPR + 256 AGPR, one wave per SIMD both ways) -- the loads of x_{k+1}, read here next to x_k, and of the
// track id come in another order; dropping __restrict__ from the function changes nothing.  So: two texts, neither with a dead branch.
// (Both pay for sens_col_stage's run-time test of Sl: as a compile-time choice this kernel is 2654 / 2661 instructions -- a change of the
// dynamic models' speed, left for one that measures it.)
template <int MODEL>
__global__ __launch_bounds__(64) void k_linearize_dyn(
    int B, int N, int M, double dt, int nknots, const double *__restrict__ s_ref,
    const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id, const double *__restrict__ xs,
    const double *__restrict__ us, double *__restrict__ lin)
{
    const long t = (long)blockIdx.x * 64 + threadIdx.x;
    const int b = (int)(t / N);
    const int k = (int)(t % N);
    if (b >= B) return;

    const double *xk = xs + ((size_t)b * (N + 1) + k) * 8;
    SENS_LOAD_STATE(xk, us + ((size_t)b * N + k) * 2, track_id[b])

    // S, Sacc, dK: [column][row]; only rows in S_COL_MASK[column] are ever touched
    extern __shared__ double s_lds[];
    double *Sl = s_lds + threadIdx.x;
    double S[10][8], Sacc[10][8], dK[10][8];
#pragma unroll
    for (int c = 0; c < 10; c++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            S[c][i] = (c == i) ? 1.0 : 0.0; dK[c][i] = 0.0;
            Sacc[c][i] = S[c][i];
            if ((S_COL_MASK[1][c] >> i) & 1u) Sl[s_pos(1, c, i) * 64] = S[c][i];
        }
    // The stage derivatives dK of the last columns (delta_0, u_T, u_delta: 21 entries) wait in LDS as well while the model is evaluated -- what the
    // 160 KB of a CU hold beside S at four waves: (55 + 21) x 512 B = 38 KB per wave.  They are fetched in front of the column's stage and put back
    // behind it: same arithmetic, fewer values alive across the forward-AD evaluation (scratch 400 -> see profiles/r4/kernel_resources.txt).
    double *Dl = Sl + s_count(1) * 64;
#pragma unroll
    for (int c = DK_PARK_FROM; c < 10; c++)
#pragma unroll
        for (int i = 0; i < 8; i++)
            if ((S_COL_MASK[1][c] >> i) & 1u) Dl[dk_pos(c, i) * 64] = 0.0;

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
            fdyn6_eval<true, MODEL == IHM2MPC_MODEL_FDYN6U, false, true>(X, u_T, u_d, trk, K, J);      // (with the scheduling fences between the wheels)
#pragma unroll
            for (int i = 0; i < 8; i++) xacc[i] = fma(wh, K[i], xacc[i]);
#define DYN_STAGE_COL(c)                                                                                                        \
            {                                                                                                                   \
                if (c >= DK_PARK_FROM) {                                                                                        \
                    _Pragma("unroll") for (int i = 0; i < 8; i++)                                                               \
                        if ((S_COL_MASK[1][c] >> i) & 1u) dK[c][i] = Dl[dk_pos(c, i) * 64];                                     \
                }                                                                                                               \
                sens_col_stage<MODEL, c>(J, S[c], Sl, Sacc[c], dK[c], ah, wh);                                                  \
                if (c >= DK_PARK_FROM) {                                                                                        \
                    _Pragma("unroll") for (int i = 0; i < 8; i++)                                                               \
                        if ((S_COL_MASK[1][c] >> i) & 1u) Dl[dk_pos(c, i) * 64] = dK[c][i];                                     \
                }                                                                                                               \
            }
            FOR_ALL_COLS(DYN_STAGE_COL)
#undef DYN_STAGE_COL
        }
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = xacc[i];
#pragma unroll
        for (int c = 0; c < 10; c++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                if ((S_COL_MASK[1][c] >> i) & 1u) Sl[s_pos(1, c, i) * 64] = Sacc[c][i];
    }

    SENS_WRITE_RECORD(lin + ((size_t)b * N + k) * LIN_REC, Sacc, 1, xk + 8)
}


// plant / rollout step: x_next = RK4 x M over dt, no sensitivities; model -1 (-2: with fdyn6u) = kin/dyn switch of
// python/main.py:482-489 (v^2 sin(beta) / l_R <= 3 -> kinematic, else dynamic)
__global__ __launch_bounds__(64) void k_sim_step(int B, int model, int M, double dt, int nknots,
                                                 const double *__restrict__ s_ref, const double *__restrict__ kappa_ref,
                                                 const int32_t *__restrict__ track_id, const double *xs,
                                                 const double *__restrict__ us, double *xn, const int32_t *__restrict__ active)
{
    // four lanes per instance (the wheels of the dynamic model, device_steps.hpp): a quad is either whole inside the batch or whole outside
    const int t = blockIdx.x * 64 + threadIdx.x, b = t >> 2;
    if (b >= B) return;
    dev_sim_step(b, t & 3, model, M, dt, nknots, s_ref, kappa_ref, track_id, xs, us, xn, active);
}

// the plain kinematic plant (model 0): the integrator of the shooting intervals on (x, u), see dev_sim_step_kin
template <int LAG = 0, typename... LF>
__global__ __launch_bounds__(64) void k_sim_step_kin(int B, int M, double dt, int nknots, const double *__restrict__ s_ref,
                                                     const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id, const double *xs,
                                                     const double *__restrict__ us, double *xn, const int32_t *__restrict__ active, double *spare_rec,
                                                     LF... lf)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    dev_sim_step_kin<LAG>(b, M, dt, nknots, s_ref, kappa_ref, track_id, xs, us, xn, active, spare_rec, lag_ptr(lf...));
}

}  // namespace

// The stage factors of both actuator lags for sub-steps of h (include/ihm2mpc.h: ihm2mpc_lag_stage_factors), on the host: no exp on the device
LagFac ihm2_lag_factors(double h)
{
    LagFac l;
    (void)ihm2mpc_lag_stage_factors(h, k_tT, l.f);
    (void)ihm2mpc_lag_stage_factors(h, k_tdelta, l.f + 4);
    return l;
}

// Which kernel: qp_select.hpp: select_linearize.  One lane per (instance, interval) in blocks of 64; the column kernel ten wavefronts per block.
void ihm2_launch_linearize(ihm2mpc_handle *h)
{
    const LinKernel kernel = select_linearize(ihm2_situation(h));
    note_lin(h->launch_rec, kernel);
    const dim3 blocks((unsigned)(((long)h->B * h->N + 63) / 64));
    const size_t dyn_lds = (s_count(1) + dk_count()) * 64 * sizeof(double);
#define LINEARIZE(k, grid, lds, ...)                                                                                                  \
    hipLaunchKernelGGL(k, grid, dim3(64), lds, h->stream, h->B, h->N, h->cfg.M, h->cfg.dt, h->cfg.nknots, h->s_ref, h->kappa_ref,  \
                       h->track_id, h->x, h->u, h->lin, ##__VA_ARGS__)
    switch (kernel) {
    case LIN_K_LINEARIZE_IRK: ihm2_launch_linearize_irk(h); break;
    case LIN_K_LINEARIZE_LAG: LINEARIZE((k_linearize<1, LagFac>), blocks, 0, ihm2_lag_factors(h->cfg.dt / h->cfg.M)); break;
    case LIN_K_LINEARIZE_DYN:
        if (h->cfg.model == IHM2MPC_MODEL_FDYN6U) LINEARIZE(k_linearize_dyn<IHM2MPC_MODEL_FDYN6U>, blocks, dyn_lds);
        else LINEARIZE(k_linearize_dyn<IHM2MPC_MODEL_FDYN6>, blocks, dyn_lds);
        break;
    case LIN_K_LINEARIZE_COLS: LINEARIZE(k_linearize_cols, dim3(blocks.x, 10), 0); break;
    case LIN_K_LINEARIZE: LINEARIZE(k_linearize<>, blocks, 0); break;
    case LIN_KERNEL_NONE: break;
    }
#undef LINEARIZE
}

// Which kernel: qp_select.hpp: select_sim; none (ERK_LAG with another plant than model 0) launches nothing -- api.hip: check_plant has
// refused the call.  k_sim_step_kin leaves its discarded linearisation record behind the handle's B N records.
void ihm2_launch_sim(ihm2mpc_handle *h, int model, int M_sim, const double *x, const double *u, double *xn, hipStream_t stream, const int32_t *active)
{
    const SimKernel kernel = select_sim(ihm2_situation(h), model);
    note_sim(h->launch_rec, kernel);
    const dim3 blocks((h->B + 63) / 64);
    double *spare_rec = h->lin + (size_t)h->B * h->N * LIN_REC;
    switch (kernel) {
    case SIM_K_SIM_IRK: ihm2_launch_sim_irk(h, model, M_sim, x, u, xn, stream, active); break;
    case SIM_K_SIM_STEP_KIN_LAG:
        hipLaunchKernelGGL((k_sim_step_kin<1, LagFac>), blocks, dim3(64), 0, stream, h->B, M_sim, h->cfg.dt, h->cfg.nknots, h->s_ref, h->kappa_ref,
                           h->track_id, x, u, xn, active, spare_rec, ihm2_lag_factors(h->cfg.dt / M_sim));
        break;
    case SIM_K_SIM_STEP_KIN:
        hipLaunchKernelGGL(k_sim_step_kin<>, blocks, dim3(64), 0, stream, h->B, M_sim, h->cfg.dt, h->cfg.nknots, h->s_ref, h->kappa_ref, h->track_id,
                           x, u, xn, active, spare_rec);
        break;
    case SIM_K_SIM_STEP:        // four lanes per instance
        hipLaunchKernelGGL(k_sim_step, dim3((4 * h->B + 63) / 64), dim3(64), 0, stream, h->B, model, M_sim, h->cfg.dt,
                           h->cfg.nknots, h->s_ref, h->kappa_ref, h->track_id, x, u, xn, active);
        break;
    case SIM_K_SIM_SENS: case SIM_KERNEL_NONE: break;
    }
}

