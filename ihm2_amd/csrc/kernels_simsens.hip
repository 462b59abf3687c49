// kernels_simsens.hip -- plant steps with forward sensitivities (ihm2mpc_sim_step_sens): x_next = Phi(x, u) of the handle's PLANT integrator
// (sim_integrator_type, M_sim steps over dt) together with S_x = dPhi/dx (8 x 8) and S_u = dPhi/du (8 x 2), the exact derivative of the
// discrete map.
//
// Replaces AcadosSimSolver.solve() with sens_forw and its get("Sx" | "Su" | "S_forw") (acados computes S_forw by default).
//
// A translation unit of its own: the device code of every other object stays what it was.  The integrators are the device functions of the
// shooting intervals (device_steps.hpp, irk_body.hpp) on the pairs (x_b, u_b):
//   * k_sim_sens_kin<LAG>   one lane per instance: dev_integrate_sens_fkin6 / dev_integrate_sens_fkin6_lag.  The 88-double record those
//                           functions write is a private array here (constant indices: registers), from which the caller's three arrays
//                           are stored -- no record in memory, nothing of the handle is written.
//   * k_sim_sens_dyn<MODEL> one lane per instance: dev_integrate_sens_dyn, the base sensitivities in LDS (55 words per lane, entry-major,
//                           28 KB per wave: the layout of k_linearize_dyn without its parked dK).
//   * k_sim_sens_irk<MODEL> one quad per instance (lane & 3 = collocation stage): irk_step + irk_sens_cols per step as irk_linearize_quad
//                           runs them, and, for M_sim > 1, the chain S <- [A_m | B_m] applied to S with the rows of S spread over the quad.
// The speed-switched plants (model -1 / -2) do NOT inline both families into one kernel: k_sim_sens_switch evaluates the switch of
// dev_sim_step once per instance into model_used, and the kinematic and the dynamic kernel run one after the other under that mask -- an
// instance takes the code, and so the bits, of a call with its model fixed.
#include "ihm2mpc_internal.h"
#include "model.hpp"
#include "device_steps.hpp"
#include "riccati_mfma.hpp"
#include "irk_body.hpp"
#include "qp_select.hpp"

using namespace ihm2;

namespace {

__device__ __forceinline__ const double *lag_ptr() { return nullptr; }
__device__ __forceinline__ const double *lag_ptr(const LagFac &l) { return l.f; }

// the model that integrates instance b: `model` itself, or for model -1 (-2: with fdyn6u) the branch the kin / dyn switch of
// python/main.py:482-489 takes at x_b (the formula of dev_sim_step: v^2 sin(beta) / l_R <= 3 -> kinematic)
__global__ __launch_bounds__(64) void k_sim_sens_switch(int B, int model, const double *__restrict__ xs, int32_t *__restrict__ model_used)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    int mdl = model;
    if (model < 0) {
        double x[8];
#pragma unroll
        for (int i = 0; i < 8; i++) x[i] = xs[(size_t)b * 8 + i];
        const double beta = atan(k_rwd * tan(x[7]));
        const double v2 = x[3] * x[3] + x[4] * x[4];
        mdl = (v2 * sin(beta) / k_lR <= 3.0) ? IHM2MPC_MODEL_FKIN6 : (model == -2 ? IHM2MPC_MODEL_FDYN6U : IHM2MPC_MODEL_FDYN6);
    }
    model_used[b] = mdl;
}

// record [A (8x8 row-major) | B (8x2) | ..] and the new state -> the caller's arrays, each optional
__device__ __forceinline__ void store_outputs(int b, const double (&rec)[88], const double (&xo)[8], double *xn, double *Sx, double *Su)
{
    if (Sx) {
#pragma unroll
        for (int e = 0; e < 64; e++) Sx[(size_t)b * 64 + e] = rec[e];
    }
    if (Su) {
#pragma unroll
        for (int e = 0; e < 16; e++) Su[(size_t)b * 16 + e] = rec[64 + e];
    }
    if (xn) {
#pragma unroll
        for (int i = 0; i < 8; i++) xn[(size_t)b * 8 + i] = xo[i];
    }
}

// fkin6 (mask: only the instances the switch gave to the kinematic model)
template <int LAG = 0, typename... LF>
__global__ __launch_bounds__(64) void k_sim_sens_kin(int B, int M, double dt, int nknots, const double *__restrict__ s_ref,
                                                     const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id,
                                                     const double *xs, const double *us, const int32_t *mask, double *xn, double *Sx, double *Su,
                                                     LF... lf)
{
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    if (mask && mask[b] != IHM2MPC_MODEL_FKIN6) return;
    const double *xk = xs + (size_t)b * 8, *uk = us + (size_t)b * 2;
    double rec[88], xo[8];
    if constexpr (LAG != 0) dev_integrate_sens_fkin6_lag(xk, uk, xk, track_id[b], M, dt, nknots, s_ref, kappa_ref, rec, xo, lag_ptr(lf...));
    else dev_integrate_sens_fkin6(xk, uk, xk, track_id[b], M, dt, nknots, s_ref, kappa_ref, rec, xo);
    store_outputs(b, rec, xo, xn, Sx, Su);
}

// fdyn6 / fdyn6u.  dev_integrate_sens_dyn returns no state but the defect Phi(x, u) - x_next in the record: taken against zero it is
// Phi(x, u) itself, bit for bit
template <int MODEL>
__global__ __launch_bounds__(64) void k_sim_sens_dyn(int B, int M, double dt, int nknots, const double *__restrict__ s_ref,
                                                     const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id,
                                                     const double *xs, const double *us, const int32_t *mask, double *xn, double *Sx, double *Su)
{
    extern __shared__ double s_lds[];
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;                                // (no barrier and no lane exchange below: a lane may leave alone)
    if (mask && mask[b] != MODEL) return;
    const double zero[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double rec[88], xo[8];
    dev_integrate_sens_dyn<MODEL>(xs + (size_t)b * 8, us + (size_t)b * 2, zero, track_id[b], M, dt, nknots, s_ref, kappa_ref, rec,
                                  s_lds + threadIdx.x);
#pragma unroll
    for (int i = 0; i < 8; i++) xo[i] = rec[80 + i];
    store_outputs(b, rec, xo, xn, Sx, Su);
}

// Collocation, one quad per instance.  Lane st keeps the rows 2 st, 2 st + 1 of the accumulated S = [S_x S_u] (8 x 10).  A step's own map
// P = [A_m | B_m] comes from irk_sens_cols started at [I 0], five columns at a time as in irk_linearize_quad; the first step's is S itself
// (so M_sim = 1 is that function's arithmetic), a later step's is applied as S <- A_m S + [0 | B_m] with the rows of the old S fetched
// by quad broadcasts.  The quads past the end repeat the last instance (all lanes of a quad stay active for the DPP exchanges); a quad
// the mask leaves out returns whole.
template <int MODEL>
__global__ __launch_bounds__(64) void k_sim_sens_irk(int B, int M, const IrkTab *__restrict__ tab, int nknots, const double *__restrict__ s_ref,
                                                     const double *__restrict__ kappa_ref, const int32_t *__restrict__ track_id,
                                                     const double *xs, const double *us, const int32_t *mask, double *xn, double *Sx, double *Su)
{
    const int q = blockIdx.x * 16 + (threadIdx.x >> 2);
    const int b = min(q, B - 1), st = threadIdx.x & 3;
    const bool live = q < B;
    if (mask && mask[b] != MODEL) return;
    const IrkRows rows = irk_rows_from(tab, st);
    double x[8];
#pragma unroll
    for (int a = 0; a < 8; a++) x[a] = xs[(size_t)b * 8 + a];
    const double u_T = us[(size_t)b * 2], u_d = us[(size_t)b * 2 + 1];
    const int tid = track_id[b];
    TrackSeg trk;
    trk.init(s_ref + (size_t)tid * nknots, kappa_ref + (size_t)tid * nknots, nknots, x[0]);
    const double hb = rows.hb;
    double S[2][10];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 10; c++) S[r][c] = 0.0;
    for (int m = 0; m < M; m++) {
        double K[8], J[8][10], P[2][10];
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 10; c++) P[r][c] = 0.0;
        irk_step<MODEL, true>(st, rows, x, u_T, u_d, trk, K, J);
        {
            double dK[8][5];
            irk_sens_cols<MODEL, 0, 5>(st, rows, J, dK);
#pragma unroll
            for (int a = 0; a < 8; a++)
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    const double v = ((a == c) ? 1.0 : 0.0) + quad_sum(hb * dK[a][c]);
                    if ((a >> 1) == st) P[a & 1][c] = v;
                }
        }
        {
            double dK[8][5];
            irk_sens_cols<MODEL, 5, 5>(st, rows, J, dK);
#pragma unroll
            for (int a = 0; a < 8; a++)
#pragma unroll
                for (int c = 0; c < 5; c++) {
                    const double v = ((a == 5 + c) ? 1.0 : 0.0) + quad_sum(hb * dK[a][c]);
                    if ((a >> 1) == st) P[a & 1][5 + c] = v;
                }
        }
#pragma unroll
        for (int a = 0; a < 8; a++) x[a] += quad_sum(hb * K[a]);
        if (m == 0) {
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int c = 0; c < 10; c++) S[r][c] = P[r][c];
        } else {
            double Sn[2][10];
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int c = 0; c < 10; c++) Sn[r][c] = (c >= 8) ? P[r][c] : 0.0;
#pragma unroll
            for (int k = 0; k < 8; k++)
#pragma unroll
                for (int c = 0; c < 10; c++) {
                    const double sk = quad_get(S[k & 1][c], k >> 1);      // S[k][c] of the old S
#pragma unroll
                    for (int r = 0; r < 2; r++) Sn[r][c] = fma(P[r][k], sk, Sn[r][c]);
                }
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int c = 0; c < 10; c++) S[r][c] = Sn[r][c];
        }
    }
    if (!live) return;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int a = 2 * st + r;
        if (Sx) {
#pragma unroll
            for (int c = 0; c < 8; c++) Sx[(size_t)b * 64 + a * 8 + c] = S[r][c];
        }
        if (Su) {
#pragma unroll
            for (int c = 0; c < 2; c++) Su[(size_t)b * 16 + a * 2 + c] = S[r][8 + c];
        }
        if (xn) xn[(size_t)b * 8 + a] = r ? x[2 * st + 1] : x[2 * st];
    }
}

}  // namespace

// Launches on `stream`: the switch into model_used (when given; required for model < 0), then the kernel of each model family the call can
// reach.  The callers (api.hip) have run check_plant: model -2 .. 2, ERK_LAG with model 0 only.  Returns 0, or 1 if the plant's collocation
// tableau could not be uploaded.  The launch record's plant kernel becomes SIM_K_SIM_SENS.
int ihm2_launch_sim_sens(ihm2mpc_handle *h, int model, int M_sim, const double *x, const double *u, double *xn, double *Sx, double *Su,
                         int32_t *model_used, hipStream_t stream)
{
    const int B = h->B, integ = h->cfg.sim_integrator_type;
    const int lanes = (B + 63) / 64, quads = (B + 15) / 16;
    note_sim(h->launch_rec, SIM_K_SIM_SENS);
    if (ihm2_is_irk(integ) && ihm2_upload_sim_irk_tab(h, M_sim)) return 1;
    if (model_used) hipLaunchKernelGGL(k_sim_sens_switch, dim3(lanes), dim3(64), 0, stream, B, model, x, model_used);
    const int32_t *mask = model < 0 ? model_used : nullptr;
    const bool kin = model == IHM2MPC_MODEL_FKIN6 || model < 0;
    const int dyn = model == -1 ? IHM2MPC_MODEL_FDYN6 : model == -2 ? IHM2MPC_MODEL_FDYN6U : model;      // 0: none
    const ihm2mpc_config &c = h->cfg;
    if (ihm2_is_irk(integ)) {
        const IrkTab *tab = h->sim_irk_tab;
#define LAUNCH_SS_IRK(MD) hipLaunchKernelGGL(k_sim_sens_irk<MD>, dim3(quads), dim3(64), 0, stream, B, M_sim, tab, c.nknots, h->s_ref.get(), \
                                             h->kappa_ref.get(), h->track_id.get(), x, u, mask, xn, Sx, Su)
        if (kin) LAUNCH_SS_IRK(IHM2MPC_MODEL_FKIN6);
        if (dyn == IHM2MPC_MODEL_FDYN6) LAUNCH_SS_IRK(IHM2MPC_MODEL_FDYN6);
        if (dyn == IHM2MPC_MODEL_FDYN6U) LAUNCH_SS_IRK(IHM2MPC_MODEL_FDYN6U);
#undef LAUNCH_SS_IRK
        return 0;
    }
    if (integ == IHM2MPC_INTEG_ERK_LAG) {
        hipLaunchKernelGGL((k_sim_sens_kin<1, LagFac>), dim3(lanes), dim3(64), 0, stream, B, M_sim, c.dt, c.nknots, h->s_ref.get(), h->kappa_ref.get(),
                           h->track_id.get(), x, u, mask, xn, Sx, Su, ihm2_lag_factors(c.dt / M_sim));
        return 0;
    }
    if (kin)
        hipLaunchKernelGGL(k_sim_sens_kin<>, dim3(lanes), dim3(64), 0, stream, B, M_sim, c.dt, c.nknots, h->s_ref.get(), h->kappa_ref.get(),
                           h->track_id.get(), x, u, mask, xn, Sx, Su);
    const size_t lds = (size_t)s_count(1) * 64 * sizeof(double);
#define LAUNCH_SS_DYN(MD) hipLaunchKernelGGL(k_sim_sens_dyn<MD>, dim3(lanes), dim3(64), lds, stream, B, M_sim, c.dt, c.nknots, h->s_ref.get(), \
                                             h->kappa_ref.get(), h->track_id.get(), x, u, mask, xn, Sx, Su)
    if (dyn == IHM2MPC_MODEL_FDYN6) LAUNCH_SS_DYN(IHM2MPC_MODEL_FDYN6);
    if (dyn == IHM2MPC_MODEL_FDYN6U) LAUNCH_SS_DYN(IHM2MPC_MODEL_FDYN6U);
#undef LAUNCH_SS_DYN
    return 0;
}
