// kernels_sens.hip -- sensitivities of the last RTI QP's solution with respect to the initial state (acados: eval_param_sens(.., "ex")
// followed by get(stage, "sens_x" / "sens_u")).
//
// The last QP of an instance was linearised at (xbar, ubar) -- the snapshot api.hip takes after the linearisation -- and returned
// dz = (x - xbar, u - ubar), the multipliers lam (lam_a) and the soft slacks slk (slk_a).  The interior point's KKT system, linearised at
// that iterate with the primal gaps in place of its own slacks, is an equality-constrained LQ problem ("x0 sensitivities"):
//   every present side i of a row r_i:  gap_i = r_i dz_k - dl_i + s_i (lower) or du_i - r_i dz_k + s_i (upper),  t_i = max(gap_i, tau)
//     hard:  sigma_i = lam_i / t_i
//     soft:  nu_i = max(z_i + Z_i s_i - lam_i, 0),  rho_i = Z_i + nu_i / max(s_i, tau),  sigma_i = 1 / (t_i / lam_i + 1 / rho_i)
//            (the slack eliminated in series; sigma_i = 0 where lam_i = 0)
//   Ht_k = H_k + sum_i sigma_i r_i r_i',   dx_0 = e_j,  dx_{k+1} = A_k dx_k + B_k du_k.
// Its solution for the eight columns j at once: dU_k = K_k dX_k, dX_{k+1} = (A_k + B_k K_k) dX_k, dX_0 = I, with K_k from the backward
// Riccati recursion on Ht.  sens_u0 = K_0 (mode 1: the backward sweep alone), sens_x / sens_u the whole horizon (mode 2).
//
// Mapping: one wavefront per instance; the recursion's 8x8 / 8x10 / 2x2 products one output entry per lane, operands in LDS.  The row
// weights of all stages are formed first, in parallel over the slot table (the QP kernel's table: the same sides, the same bounds, a split
// row's halves on the same lane); the track rows and the lateral-acceleration row are evaluated at xbar as the QP evaluates them.  fp64.
// The body is sens_body.hpp's, which the persistent loop calls after every step's QP as well (kernels_qp.hip: k_steps<..., SENS = 1>).
#include <cmath>

#include "ihm2mpc_internal.h"
#include "sens_body.hpp"

namespace {

__global__ __launch_bounds__(64) void k_sens(SensArgs a)
{
    extern __shared__ double sm[];
    const int b = blockIdx.x;
    if (b >= a.B) return;
    sens_body(a, b, sm, 0);
}

}  // namespace

size_t ihm2_sens_lds_bytes(const ihm2mpc_handle *h)
{
    return sizeof(double) * ihm2::sens_lds_doubles((size_t)h->N);      // (qp_lds.hpp)
}

void ihm2_sens_args(const ihm2mpc_handle *h, void *out)
{
    SensArgs &a = *(SensArgs *)out;
    a.B = h->B; a.N = h->N; a.mode = h->sens_mode; a.nslots = h->slots.per_lane * 64;
    a.path = h->path_on ? 1 : 0; a.alat = h->rows.alat_on ? 1 : 0;
    a.tau = IHM2MPC_SENS_TAU;
    a.Hs = h->Hs; a.hs_bs = 0; a.hs_te = h->N * 100; a.hs_ks = 100;
    if (h->inst_w) { a.Hs = h->iHs; a.hs_bs = 200; a.hs_te = 100; a.hs_ks = 0; }
    a.CD = h->CD;
    a.slot_kc = h->slot_kc; a.slot_lb = h->slot_lb; a.slot_ub = h->slot_ub; a.unused_pad0 = nullptr; a.unused_pad1 = nullptr; a.sl_bs = 0;
    if (h->inst_b || h->inst_p) { a.slot_lb = h->i_slot_lb; a.slot_ub = h->i_slot_ub; a.sl_bs = 2 * h->slots.per_lane * 64; }
    a.track_id = h->track_id; a.widths = h->widths; a.car_L = h->car_L; a.car_W = h->car_W;
    a.lin = h->lin; a.xbar = h->sens_xbar; a.ubar = h->sens_ubar; a.x = h->x; a.u = h->u;
    a.lam = h->lam; a.slk = h->slk; a.lam_a = h->lam_a; a.slk_a = h->slk_a; a.status = h->status;
    a.sens_u0 = h->sens_u0; a.sens_x = h->sens_x; a.sens_u = h->sens_u;
    a.hist = nullptr; a.sweep_step = 0;
}

void ihm2_launch_sens(ihm2mpc_handle *h)
{
    SensArgs a;
    ihm2_sens_args(h, &a);
    const size_t lds = ihm2_sens_lds_bytes(h);
    (void)hipFuncSetAttribute((const void *)k_sens, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_sens, dim3(h->B), dim3(64), lds, h->stream, a);
}
