// api.hip -- the C ABI of libihm2mpc.so (include/ihm2mpc.h): handle lifetime, copy-in setters,
// copy-out getters, and the launch sequence of one RTI iteration on the handle's HIP stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "ihm2mpc_internal.h"
#include "qp_catalogue.hpp"
#include "qp_select.hpp"
#include "sqp_body.hpp"

static thread_local std::string g_err;

// the error string of ihm2mpc_last_error, also set by comm.hip
int ihm2_fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return -1;
}

namespace {

#define fail(...) ihm2_fail(__VA_ARGS__)

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

#define CHECK_H(h)                                        \
    do {                                                  \
        if (!(h)) return fail("null handle");             \
        HIP_TRY(hipSetDevice((h)->cfg.device));           \
    } while (0)

// Allocates a group of buffers, given as (buffer, elements) pairs, all or none: a failure releases what the call allocated and reports
// the HIP error.  (A grower releases the group's old arrays first.)
int alloc_all() { return 0; }

template <typename T, typename... Rest>
int alloc_all(DevBuf<T> &b, size_t n, Rest &&...rest)
{
    HIP_TRY(b.alloc(n));
    if (alloc_all(rest...)) { b.reset(); return -1; }
    return 0;
}

// IHM2MPC_POISON_WORKSPACE (ihm2mpc_internal.h: WorkBuf): the handle's workspace buffers of doubles by member name.  The argument blocks
// ls_args, step_args and sens_args are left out: they hold pointers and counts.  "track_work" names the local work buffers of
// ihm2mpc_build_tracks / ihm2mpc_fit_tracks.
struct Poisonable { const char *name; WorkBuf<double> ihm2mpc_handle::*buf; };
#define PB(m) {#m, &ihm2mpc_handle::m}
const Poisonable POISONABLE[] = {
    PB(lin), PB(q_g), PB(q_rg), PB(q_P), PB(q_M), PB(scratch), PB(res), PB(qp_res), PB(dyn10), PB(ls_phi),
    PB(ls_x), PB(ls_u), PB(ls_pi), PB(ls_lam), PB(ls_slk), PB(ls_wpi), PB(ls_wlam), PB(ls_alpha), PB(ls_merit),
    PB(hist_u0), PB(hist_x0), PB(hist_k),
    PB(sens_xbar), PB(sens_ubar), PB(sens_u0), PB(sens_x), PB(sens_u),
    PB(adj_sx), PB(adj_su), PB(adj_gx0), PB(adj_gy), PB(adj_gye), PB(adj_gW), PB(adj_gWe),
};
#undef PB

// the switch names this buffer: "1" names all, a comma-separated list its entries
bool poisoned(const ihm2mpc_handle *h, const char *name)
{
    const std::string &s = h->poison;
    if (s.empty() || s == "0") return false;
    if (s == "1") return true;
    const size_t n = strlen(name);
    for (size_t i = 0; i < s.size();) {
        const size_t j = std::min(s.find(',', i), s.size());
        if (j - i == n && s.compare(i, n, name) == 0) return true;
        i = j + 1;
    }
    return false;
}

// before the first allocation: the fill of every workspace buffer the switch names
void arm_poison(ihm2mpc_handle *h)
{
    for (const Poisonable &p : POISONABLE) (h->*p.buf).poison(poisoned(h, p.name));
}

// host (B, elems) <-> device (B, elems): same instance-major layout on both sides
int upload(ihm2mpc_handle *h, const double *host, double *dev, int elems)
{
    HIP_TRY(hipMemcpyAsync(dev, host, (size_t)h->B * elems * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the caller's buffer may be reused as soon as we return
    return 0;
}

int download(ihm2mpc_handle *h, const double *dev, double *host, int elems)
{
    HIP_TRY(hipMemcpyAsync(host, dev, (size_t)h->B * elems * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int upload_shared(ihm2mpc_handle *h, const double *host, double *dev, size_t n)
{
    HIP_TRY(hipMemcpyAsync(dev, host, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

const char *row_name(int c)
{
    static const char *names[NC] = {"lbx/ubx[0]", "lbx/ubx[1]", "lbx/ubx[2]", "lbx/ubx[3]", "lbx/ubx[4]", "lbx/ubx[5]", "lbx/ubx[6]", "lbx/ubx[7]",
                                    "lbu/ubu[0]", "lbu/ubu[1]", "lg/ug[0]", "lg/ug[1]", "lh/uh[0]", "lh/uh[1]"};
    return (c >= 0 && c < NC) ? names[c] : "?";
}

// Per-instance bounds take the batch-shared pattern: refuses when the values' finite sides differ from the shared table's (a later shared
// setter may have changed them).
int check_instance_pattern(const ihm2mpc_handle *h, const double *il, const double *iu)
{
    const ihm2::PatternMismatch m = ihm2::find_pattern_mismatch(h->rows, h->B, il, iu);
    if (!m.found) return 0;
    return fail("instance %d, stage %d, row %d (%s): the finite sides (%s, %s) differ from the batch-shared table's (%s, %s)", m.b, m.k, m.c,
                row_name(m.c), m.lower ? "lower" : "-", m.upper ? "upper" : "-", m.shared_lower ? "lower" : "-", m.shared_upper ? "upper" : "-");
}

// Per-instance slack penalties (ihm2mpc_set_instance_soft / _alat_soft): the same for the values z, Z of the soft sides.
const char *side_name(int side)
{
    static const char *names[NLAM + 2] = {
        "lbx[0]", "lbx[1]", "lbx[2]", "lbx[3]", "lbx[4]", "lbx[5]", "lbx[6]", "lbx[7]", "lbu[0]", "lbu[1]", "lg[0]", "lg[1]", "lh[0]", "lh[1]",
        "ubx[0]", "ubx[1]", "ubx[2]", "ubx[3]", "ubx[4]", "ubx[5]", "ubx[6]", "ubx[7]", "ubu[0]", "ubu[1]", "ug[0]", "ug[1]", "uh[0]", "uh[1]",
        "a_lat lower", "a_lat upper"};
    return (side >= 0 && side < NLAM + 2) ? names[side] : "?";
}

// iz, iZ (B,NS,NLAM), az, aZ (B,2); either pair may be nullptr (those rows are batch-shared)
int check_penalty_pattern(const ihm2mpc_handle *h, const double *iz, const double *iZ, const double *az, const double *aZ)
{
    const ihm2::PenaltyMismatch m = ihm2::find_penalty_mismatch(h->rows, h->B, iz, iZ, az, aZ);
    using P = ihm2::PenaltyMismatch;
    switch (m.kind) {
    case P::NONE: return 0;
    case P::NOT_A_NUMBER: return fail("instance %d, stage %d, side %d (%s): slack penalty is NaN", m.b, m.k, m.side, side_name(m.side));
    case P::FLAG:
        return fail("instance %d, stage %d, side %d (%s): the side is %s (soft_Z %s 0) where the batch-shared table holds it %s", m.b, m.k, m.side,
                    side_name(m.side), m.soft ? "soft" : "hard", m.soft ? ">=" : "<", m.shared_soft ? "soft" : "hard");
    case P::NEGATIVE:
        return fail("instance %d, stage %d, side %d (%s): soft_z < 0 (the slack penalty must be non-decreasing)", m.b, m.k, m.side, side_name(m.side));
    default:
        return fail("instance %d, stage %d, side %d (%s): the soft side has neither a linear nor a quadratic penalty", m.b, m.k, m.side, side_name(m.side));
    }
}

// The constraint tables onto the device, and the flags that say what the device holds: the one place for both.  qp_tables.hpp:
// table_images builds every image in the layout the kernels read -- the slot table's lb | zw and ub | Zw, the (stage, row) bounds with the
// (stage, side) penalties behind them, lb | z and ub | Z -- so that one base serves the bounds and the penalties.  The batch-shared images
// always; the per-instance images (B of each, one base per instance) while either per-instance mode (bounds, slack penalties) is on -- a
// mode that is off contributes the batch-shared values -- and released when both are off.  Bounds whose finite sides differ from the shared
// table's are a refusal (-1); penalties that the pattern does not take any more (a later shared setter changed it) are no error of that
// setter: inst_p_ok stays false and ready() reports it before the next solve.  Penalties that came from device memory
// (ihm2mpc_set_instance_soft_device / _alat_soft_device) have no host copy: the stage images' penalty halves and ip are the copy, which the
// uploads below leave in place and from which k_penalty_tables puts the slot images' penalty halves back -- into whatever layout the
// slot table now has, since the kernel reads the pattern from it.  What such values were admitted under is which sides the shared rows
// hold soft (the four rules of penalty_side read nothing else of the shared table): the handle keeps those flags as they were when the
// pair was set, and a pair whose flags a shared setter has changed is marked as not fitting, since nothing here can check its values
// against the new ones.
std::vector<char> soft_flags(const double *sZ, size_t n)
{
    std::vector<char> f(n);
    for (size_t i = 0; i < n; i++) f[i] = sZ[i] >= 0.0;
    return f;
}

int tables_to_device(ihm2mpc_handle *h)
{
    const int B = h->B;
    const bool inst = h->inst_b || h->inst_p;
    const ihm2::SlotTable &t = h->slots;
    h->inst_b_ok = false; h->inst_p_ok = false;
    h->inst_images = false;     // until the per-instance images of h->slots are on the device, every one of them (every early return below leaves it false)
    if (h->dev_sp == 1 && h->dev_sp_flags != soft_flags(h->rows.sZ.data(), h->rows.sZ.size())) h->dev_sp = 2;
    if (h->dev_ap == 1 && h->dev_ap_flags != soft_flags(h->rows.alat_sZ, 2)) h->dev_ap = 2;
    h->slots_full = false;      // until a table and every bound that goes with it are on the device
    ihm2::TableImages m = ihm2::table_images(t, h->rows, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    if (m.entries && (upload_shared(h, m.slot_lo.data(), h->slot_lb, m.slot_lo.size()) || upload_shared(h, m.slot_up.data(), h->slot_ub, m.slot_up.size())))
        return -1;
    if (upload_shared(h, m.stage_lo.data(), h->st_lb, m.stage_lo.size()) || upload_shared(h, m.stage_up.data(), h->st_ub, m.stage_up.size())) return -1;
    if ((!inst && h->i_st_lb) || (!h->inst_p && h->ip.alat_sz)) HIP_TRY(hipStreamSynchronize(h->stream));       // a launch in flight may still read the arrays
    if (!h->inst_p) h->ip.reset();
    if (!inst) { h->i_slot_lb.reset(); h->i_slot_ub.reset(); h->i_st_lb.reset(); h->i_st_ub.reset(); }
    if (inst) {
        if (h->inst_b && check_instance_pattern(h, h->ih_lb.data(), h->ih_ub.data())) return -1;
        const double *il = h->inst_b ? h->ih_lb.data() : nullptr, *iu = h->inst_b ? h->ih_ub.data() : nullptr;
        const double *iz = h->ih_sz.empty() ? nullptr : h->ih_sz.data(), *iZ = h->ih_sZ.empty() ? nullptr : h->ih_sZ.data();
        const double *az = h->ih_az.empty() ? nullptr : h->ih_az.data(), *aZ = h->ih_aZ.empty() ? nullptr : h->ih_aZ.data();
        const bool p_fit = h->inst_p && !ihm2::find_penalty_mismatch(h->rows, B, iz, iZ, az, aZ).found();
        if (!p_fit) iz = iZ = az = aZ = nullptr;       // (the shared values: launches are refused until the penalties are set again or dropped)
        h->host_p_fit = p_fit;
        const bool keep_sp = h->dev_sp == 1 && h->i_st_lb, keep_ap = h->dev_ap == 1 && h->ip.alat_sz;     // device-set pairs that still fit
        m = ihm2::table_images(t, h->rows, B, il, iu, iz, iZ, az, aZ);
        if (m.slot_lo.size() > h->i_slot_lb.size() || !h->i_st_lb) {
            HIP_TRY(hipStreamSynchronize(h->stream));       // a launch in flight may still read the old arrays
            if (m.slot_lo.size() > h->i_slot_lb.size()) {
                h->i_slot_lb.reset(); h->i_slot_ub.reset();
                if (alloc_all(h->i_slot_lb, m.slot_lo.size(), h->i_slot_ub, m.slot_up.size())) return -1;
            }
            if (!h->i_st_lb && alloc_all(h->i_st_lb, m.stage_lo.size(), h->i_st_ub, m.stage_up.size())) return -1;
        }
        if (m.entries && (upload_shared(h, m.slot_lo.data(), h->i_slot_lb, m.slot_lo.size()) || upload_shared(h, m.slot_up.data(), h->i_slot_ub, m.slot_up.size())))
            return -1;
        if (keep_sp) {          // the bounds halves only: the penalty halves are the one copy of the device-set values
            const size_t row = (m.stage_rows + (size_t)h->NS * NLAM) * sizeof(double), half = m.stage_rows * sizeof(double);
            HIP_TRY(hipMemcpy2DAsync(h->i_st_lb, row, m.stage_lo.data(), row, half, B, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpy2DAsync(h->i_st_ub, row, m.stage_up.data(), row, half, B, hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        } else if (upload_shared(h, m.stage_lo.data(), h->i_st_lb, m.stage_lo.size()) || upload_shared(h, m.stage_up.data(), h->i_st_ub, m.stage_up.size()))
            return -1;
        if (h->inst_p) {        // the a_lat row's (B,2) pairs, which the cost reads beside the tables
            if (!h->ip.alat_sz && alloc_all(h->ip.alat_sz, m.alat_z.size(), h->ip.alat_sZ, m.alat_Z.size())) return -1;
            if (!keep_ap && (upload_shared(h, m.alat_z.data(), h->ip.alat_sz, m.alat_z.size()) || upload_shared(h, m.alat_Z.data(), h->ip.alat_sZ, m.alat_Z.size())))
                return -1;
        }
        // the slot images' penalty halves of the device-set pairs, from the device's copy
        if (keep_sp && m.entries) ihm2_launch_penalty_tables(h, 0, h->i_st_lb + m.stage_rows, h->i_st_ub + m.stage_rows, m.stage_rows + (size_t)h->NS * NLAM, 0);
        if (keep_ap && m.entries) ihm2_launch_penalty_tables(h, 1, h->ip.alat_sz, h->ip.alat_sZ, 2, 0);
        if (keep_sp || keep_ap) HIP_TRY(hipGetLastError());
        h->inst_b_ok = h->inst_b; h->inst_p_ok = p_fit && h->dev_sp != 2 && h->dev_ap != 2;
        h->inst_images = true;
    }
    // the full slot form: the table, with the bounds of every instance that the device now holds
    h->slots_full = h->slots_fit && ihm2::slot_table_full(t, ihm2::full_form_nslot()) && ihm2::slot_bounds_full(t, inst ? B : 1, m.slot_lo, m.slot_up);
    return 0;
}

// ---- the instantiations of the QP kernels and the persistent loop: the handle's situation, the chosen instantiation, launch ----
// The catalogue is the eight objects' tables laid end to end, in the order of qp_catalogue.hpp: catalogue_keys(), whose positions
// qp_select.hpp: select_qp / select_steps return.  Built once.
const QpInst *catalogue_inst(int pos)
{
    static const std::vector<const QpInst *> insts = [] {
        std::vector<const QpInst *> v;
#define QP_SET_INSTS(set) { const QpTable t = QP_SET_TABLE(set)(); for (int i = 0; i < t.n; i++) v.push_back(t.inst + i); }
        QP_SETS(QP_SET_INSTS)
#undef QP_SET_INSTS
        return v;
    }();
    return pos < 0 ? nullptr : insts[pos];
}

// the PATH of the instantiations that take the handle's rows: 0 none, 1 the track rows, 2 the track rows and the lateral-acceleration row
int path_class(const ihm2mpc_handle *h) { return h->rows.alat_on ? 2 : h->path_on ? 1 : 0; }

// IHM2MPC_QP_FORM (read once; qp_select.hpp: factor_form says what the values mean)
int qp_form_limit()
{
    static const int limit = [] { const char *e = getenv("IHM2MPC_QP_FORM"); return (e && e[0] == '0') ? 0 : (e && e[0] == '1') ? 1 : (e && e[0] == '2') ? 2 : 3; }();
    return limit;
}

// the switches that are on with the value 1 (read once each)
bool switch_on(const char *name) { const char *e = getenv(name); return e && e[0] == '1'; }

QpArgs qp_args(ihm2mpc_handle *h)
{
    QpArgs a;
    a.B = h->B; a.N = h->N; a.iter_max = h->cfg.ipm_iter_max; a.nslots = h->slots.per_lane * 64; a.m_act = h->slots.m_act;
    a.nslots_can = h->slots.per_lane * 64;
    a.tol = h->cfg.ipm_tol; a.mu0 = h->cfg.ipm_mu0; a.tau0 = h->cfg.ipm_tau0;
    a.Hs = h->Hs; a.Gy = h->Gy; a.CD = h->CD; a.slot_lb = h->slot_lb; a.slot_ub = h->slot_ub; a.slot_kc = h->slot_kc;
    a.hs_bs = 0; a.hs_te = h->N * 100; a.gy_bs = 0; a.gy_te = h->N * 120; a.sl_bs = 0;
    if (h->inst_w) { a.Hs = h->iHs; a.Gy = h->iGy; a.hs_bs = 200; a.hs_te = 100; a.gy_bs = 240; a.gy_te = 120; }
    if (h->inst_b || h->inst_p) { a.sl_bs = 2 * h->slots.per_lane * 64; a.slot_lb = h->i_slot_lb; a.slot_ub = h->i_slot_ub; }    // bounds | penalties per instance
    a.x = h->x; a.u = h->u; a.x0 = h->x0; a.yref = h->yref; a.yref_e = h->yref_e;
    a.pi = h->pi; a.lam = h->lam; a.res = h->res; a.qp_res = h->qp_res; a.u0 = h->u0; a.status = h->status; a.qp_iter = h->qp_iter;
    a.lin = h->lin; a.g = h->q_g; a.rg = h->q_rg; a.P = h->q_P; a.M = h->q_M + (size_t)QM_PAD * 64;
    a.unused_pad0 = nullptr; a.unused_pad1 = nullptr; a.slk = h->slk;
    a.track_id = h->track_id; a.widths = h->widths; a.car_L = h->car_L; a.car_W = h->car_W;
    a.lam_a = h->lam_a; a.slk_a = h->slk_a;
    a.symmetrize = (h->cfg.model == IHM2MPC_MODEL_FDYN6) ? 1 : 0;
    return a;
}

// one block of 64 x NW lanes per instance, `args` the kernel's arguments
void launch_inst(ihm2mpc_handle *h, const QpInst *e, void **args, size_t lds)
{
    (void)hipFuncSetAttribute(e->kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    (void)hipLaunchKernel(e->kernel, dim3(h->B), dim3(e->threads), args, lds, h->stream);
    ihm2::encode_launch(h->launch_rec, e->key);
}

// The per-step QP; non-zero: no instantiation takes the table (ready() has refused the tables without one), or not in the LDS
int launch_qp(ihm2mpc_handle *h)
{
    const ihm2::QpChoice c = ihm2::select_qp(ihm2_situation(h));
    const QpInst *e = catalogue_inst(c.pos);
    if (!e) return 1;
    QpArgs a = qp_args(h);
    if (e->key.kind == QP_BLOCK) { a.slot_kc = h->slot_kc_blk; a.slot_lb = h->slot_lb_blk; a.slot_ub = h->slot_ub_blk; a.nslots = h->slots.per_blk * 256; }
    void *args[] = {&a};
    launch_inst(h, e, args, c.lds);
    return 0;
}

// n_steps control steps in one launch (k_steps) of the instantiation `c` (qp_select.hpp: select_run), histories into h->hist_*.  Returns
// 0 launched, 1 not launched -- no instantiation, or the plant's tableau could not be uploaded (the caller then runs ihm2mpc_step n_steps
// times, which gives the same results).  sens: the loop with x0 sensitivities (k_steps<..., SENS = 1>), their history into h->hist_k;
// its LDS is the larger of the QP's and k_sens' (the body reuses the QP's).
int launch_steps(ihm2mpc_handle *h, const ihm2::QpChoice &c, int model, int M_sim, double s_target, int n_steps, int freeze, double lap_stop, int sens)
{
    const QpInst *e = catalogue_inst(c.pos);
    if (!e) return 1;
    const bool irk_plant = ihm2_is_irk(h->cfg.sim_integrator_type);     // the plants by collocation (python/main.py:395-400: Radau IIA x M_sim)
    if (irk_plant && ihm2_upload_sim_irk_tab(h, M_sim)) return 1;
    const bool sqp = e->key.sqp;
    QpArgs a = qp_args(h);
    StepArgs s;
    s.ocp_model = h->cfg.model;
    s.n_steps = n_steps; s.model = model; s.M_sim = M_sim; s.M = h->cfg.M; s.nknots = h->cfg.nknots; s.lap_wrap = h->lap_wrap ? 1 : 0;
    s.freeze = freeze; s.s_target = s_target; s.dt = h->cfg.dt; s.lap_stop = lap_stop;
    s.sqp_iters = sqp ? (h->cfg.nlp_solver_max_iter > 0 ? h->cfg.nlp_solver_max_iter : 1) : 0;
    s.s_ref = h->s_ref; s.kappa_ref = h->kappa_ref;
    s.x0 = h->x0; s.yref = h->yref; s.yref_e = h->yref_e; s.lin = h->lin;
    s.active = (freeze || h->active_set) ? h->active.get() : nullptr;
    s.hist_u0 = h->hist_u0; s.hist_x0 = h->hist_x0; s.hist_st = h->hist_st; s.hist_it = h->hist_it;
    s.irk_tab = h->irk_tab;
    s.sim_irk_tab = irk_plant ? h->sim_irk_tab.get() : nullptr;
    s.sens = sens ? (const SensArgs *)h->sens_args.get() : nullptr;
    s.sim_lag = h->cfg.sim_integrator_type == IHM2MPC_INTEG_ERK_LAG;
    std::memset(s.lag, 0, sizeof s.lag);
    if (e->key.irk == 2) {
        const LagFac lo = ihm2_lag_factors(h->cfg.dt / h->cfg.M), lp = ihm2_lag_factors(h->cfg.dt / M_sim);
        std::memcpy(s.lag[0], lo.f, sizeof lo.f); std::memcpy(s.lag[1], lp.f, sizeof lp.f);
    }
    // every field of s is set: upload it (and the line search's block in the SQP mode, the x0 sensitivities' block with SENS)
    static_assert(sizeof(StepArgs) <= 48 * sizeof(double), "step_args holds 384 bytes");
    static_assert(sizeof(ihm2::LsArgs) <= 64 * sizeof(double), "ls_args holds 512 bytes");
    static_assert(sizeof(SensArgs) <= 64 * sizeof(double), "sens_args holds 512 bytes");
    // both blocks go through a pinned staging slot (two slots, used alternately) and are uploaded in stream order: the host does
    // not wait for the previous launch (run_steps(wait = false) enqueues in pieces while the host does other work)
    const int slot = (h->args_idx++) & 1;
    if (hipEventSynchronize(h->args_ev[slot]) != hipSuccess) return 1;          // the upload that last used this slot has been issued long ago
    char *stage = (char *)h->args_host[slot];
    std::memcpy(stage, &s, sizeof(StepArgs));
    if (hipMemcpyAsync(h->step_args, stage, sizeof(StepArgs), hipMemcpyHostToDevice, h->stream) != hipSuccess) return 1;
    if (sqp) {
        ihm2::LsArgs ls_host = ihm2::make_ls_args(h);
        if (e->key.irk) ls_host.phase = 3;        // the trial points' collocation rollouts are done in the loop, one step length at a time
        std::memcpy(stage + 512, &ls_host, sizeof(ihm2::LsArgs));
        if (hipMemcpyAsync(h->ls_args, stage + 512, sizeof(ihm2::LsArgs), hipMemcpyHostToDevice, h->stream) != hipSuccess) return 1;
    }
    if (sens) {         // (the RTI mode only: the second half of the slot is free)
        SensArgs sa;
        ihm2_sens_args(h, &sa);
        sa.hist = h->hist_k; sa.sweep_step = n_steps - 1;
        std::memcpy(stage + 512, &sa, sizeof(SensArgs));
        if (hipMemcpyAsync(h->sens_args, stage + 512, sizeof(SensArgs), hipMemcpyHostToDevice, h->stream) != hipSuccess) return 1;
    }
    if (hipEventRecord(h->args_ev[slot], h->stream) != hipSuccess) return 1;
    const StepArgs *sdev = (const StepArgs *)h->step_args.get();
    const ihm2::LsArgs *ls = (const ihm2::LsArgs *)h->ls_args.get();
    void *args[] = {&sdev, &a, &ls};
    launch_inst(h, e, args, c.lds);
    return 0;
}

// x0 sensitivities (kernels_sens.hip): the point the last QP is linearised at, copied after the linearisation ...
int sens_snapshot(ihm2mpc_handle *h)
{
    if (!h->sens_mode || h->sens_quiet) return 0;
    HIP_TRY(hipMemcpyAsync(h->sens_xbar, h->x, (size_t)h->B * h->NS * NX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->sens_ubar, h->u, (size_t)h->B * h->N * NU * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// ... and the kernel after that QP
void sens_after_qp(ihm2mpc_handle *h)
{
    if (!h->sens_mode || h->sens_quiet) return;
    ihm2_launch_sens(h);
    h->sens_state = 1;
}

// readable sensitivities: the mode is on and the last solve / step computed them
int sens_readable(const ihm2mpc_handle *h)
{
    if (!h->sens_mode) return fail("x0 sensitivities are off: ihm2mpc_set_x0_sensitivities(h, 1 or 2) before the solve");
    if (h->sens_state == 2)
        return fail("the last step came from ihm2mpc_run_steps, which computes no x0 sensitivities (the persistent loop is left as it is): "
                    "call ihm2mpc_run_steps_sens, ihm2mpc_solve, ihm2mpc_compute_control or ihm2mpc_step");
    if (h->sens_state != 1) return fail("no solve has run since x0 sensitivities were set to mode %d: nothing to read yet", h->sens_mode);
    return 0;
}

int ready(ihm2mpc_handle *h)
{
    if (!h->tracks_set) return fail("ihm2mpc_set_tracks has not been called");
    if (!h->weights_set) return fail("ihm2mpc_set_weights has not been called");
    if (!h->bounds_set) return fail("ihm2mpc_set_bounds has not been called");
    if (h->inst_w && !h->uniform_CD) return fail("per-instance weights need stage-independent general rows C, D (the QP keeps one copy of them)");
    if (h->inst_b && !h->inst_b_ok) return fail("the per-instance bounds do not fit the batch-shared constraint pattern any more: set them again, or pass NULL");
    if (h->inst_p && !h->inst_p_ok) return fail("the per-instance penalties do not fit the batch-shared constraint pattern any more: set them again, or pass NULL");
    if (!h->slots_fit) {        // the limits of the catalogue's instantiations for these rows
        std::string hard = "none", soft;
        for (const auto &[S, NSL] : ihm2::slot_limits(path_class(h)))
            if (S == 0) hard = std::to_string(NSL);
            else soft += (soft.empty() ? "" : " or ") + std::to_string(NSL) + " of which " + std::to_string(S) + " soft";
        static const char *rows[3] = {"without track rows", "with track rows", "with track rows and the lateral-acceleration row"};
        return fail("the constraint rows fit no QP kernel: %s a lane of 64 takes at most %s slots when all sides are hard; with soft sides, %s "
                    "(a two-sided hard row is one slot, a row with a soft side two; a lane's one-sided slots lead it)", rows[path_class(h)],
                    hard.c_str(), soft.empty() ? "none" : soft.c_str());
    }
    if (h->rows.alat_on) {
        // the row belongs to the kinematic constraint set of old/generate_acaods_interface.py:198-209, which comes with the track rows and SQP_RTI (old/generate.py:21)
        if (h->cfg.model != IHM2MPC_MODEL_FKIN6) return fail("the lateral-acceleration row is a row of the kinematic model (old/generate_acaods_interface.py:206: `[] if is_dynamic else [a_lat]`)");
        if (!h->path_on) return fail("the lateral-acceleration row comes with the track rows: enable ihm2mpc_set_path_constraints first");
        if (h->cfg.nlp_solver_type != IHM2MPC_SQP_RTI) return fail("the lateral-acceleration row is implemented for SQP_RTI (old/generate.py:21)");
        if (!(h->uniform_H && h->uniform_CD)) return fail("the lateral-acceleration row needs stage-independent weights and general rows (the reference's OCP has them)");
    }
    return 0;
}

struct FieldInfo { double *base; int per_stage; int nstages; };

int field_info(ihm2mpc_handle *h, const char *field, FieldInfo *fi)
{
    const std::string f(field ? field : "");
    if (f == "x") *fi = {h->x, NX, h->NS};
    else if (f == "u") *fi = {h->u, NU, h->N};
    else if (f == "yref") *fi = {h->yref, NY, h->N};
    else if (f == "yref_e") *fi = {h->yref_e, NX, 1};
    else if (f == "pi") *fi = {h->pi, NX, h->NS};
    else if (f == "lam") *fi = {h->lam, NLAM, h->NS};
    else if (f == "lbx" || f == "ubx" || f == "x0") *fi = {h->x0, NX, 1};
    else return fail("unknown field '%s'", f.c_str());
    return 0;
}

}  // namespace

// what the selection reads of the handle (qp_select.hpp); IHM2MPC_BLOCK_QP is the handle's from its creation, the other switches are
// read when the process' first situation is filled
ihm2::QpSituation ihm2_situation(const ihm2mpc_handle *h)
{
    static const bool linearize_cols = switch_on("IHM2MPC_LINEARIZE_COLS"), persistent_rounds = switch_on("IHM2MPC_PERSISTENT_ROUNDS");
    ihm2::QpSituation s;
    s.N = h->N; s.B = h->B; s.n_cu = h->n_cu;
    s.model = h->cfg.model; s.integrator_type = h->cfg.integrator_type; s.sim_integrator_type = h->cfg.sim_integrator_type;
    s.nlp_solver_type = h->cfg.nlp_solver_type; s.sqp_globalization = h->sqp_globalization;
    s.per_lane = h->slots.per_lane; s.per_blk = h->slots.per_blk; s.nsoft = h->slots.nsoft; s.m_act = h->slots.m_act;
    s.slots_full = h->slots_full;
    s.path = path_class(h);
    s.uni = h->uniform_H && h->uniform_CD;
    s.inst_b = h->inst_b || h->inst_p; s.block_qp = h->block_qp;     // (either per-instance table: k_qp_block reads the shared one)
    s.qp_form = qp_form_limit();
    s.irk_tab = !!h->irk_tab; s.ls_x = !!h->ls_x; s.ls_phi = !!h->ls_phi;
    s.sens_lds = (int)(ihm2_sens_lds_bytes(h) / sizeof(double));
    s.linearize_cols = linearize_cols; s.persistent_rounds = persistent_rounds;
    return s;
}

// Runs with the handle's device current.  Nothing of the handle's may still run when its streams and buffers go; the buffers release
// themselves after this body.
ihm2mpc_handle::~ihm2mpc_handle()
{
    for (hipStream_t s : {stream, stream2}) if (s) (void)hipStreamSynchronize(s);
    (void)ihm2mpc_comm_free(this);
    for (hipEvent_t e : {ev_fork, ev_join, ev[0], ev[1], ev[2], ev[3], args_ev[0], args_ev[1]}) if (e) (void)hipEventDestroy(e);
    for (void *p : args_host) if (p) (void)hipHostFree(p);
    for (hipStream_t s : {stream, stream2}) if (s) (void)hipStreamDestroy(s);
}

// classical RK4 is stable for |z| < 2.785 on the negative real axis: z = -(dt / M) / t for the first-order actuator lags
static bool rk4_unstable(double dt, int M) { return dt / M / 1e-3 >= 2.78; }
// the sub-steps of a plant step: at least one, and with the RK4 plant integrator few enough per step to be stable on `lags` (the message's words)
static int check_sim_substeps(const ihm2mpc_handle *h, int M_sim, const char *lags)
{
    if (M_sim < 1) return fail("M_sim must be >= 1");
    if (h->cfg.sim_integrator_type == IHM2MPC_INTEG_ERK && rk4_unstable(h->cfg.dt, M_sim))
        return fail("RK4 with M_sim = %d sub-steps of dt = %g is unstable on the %s: use M_sim >= %d", M_sim, h->cfg.dt, lags,
                    (int)ceil(h->cfg.dt / (2.78 * 1e-3)));
    return 0;
}
// the plant arguments of ihm2mpc_sim_step, _sim_advance, _step and the step loops: sub-steps, plant model -2 .. 2, and a kernel for it
// (qp_select.hpp: select_sim has none where sim_integrator_type ERK_LAG meets another plant than the plain kinematic one)
static int check_plant(const ihm2mpc_handle *h, int model, int M_sim)
{
    if (check_sim_substeps(h, M_sim, "actuator lags")) return -1;
    if (model < -2 || model > IHM2MPC_MODEL_FDYN6U) return fail("unknown plant model %d", model);
    if (ihm2::select_sim(ihm2_situation(h), model) != ihm2::SIM_KERNEL_NONE) return 0;
    return fail("the plant integrator ERK_LAG (closed-form actuator lags) is implemented for the kinematic plant (model 0) only, not for plant "
                "model %d: create the handle with another sim_integrator_type", model);
}

extern "C" {

const char *ihm2mpc_last_error(void) { return g_err.c_str(); }
const char *ihm2mpc_version(void) { return "ihm2mpc 0.1 (gfx950)"; }

// E_0, E_1, E_2: the stage values that make Simpson's rule exact for the first three moments of exp(-t / tau) on [0, h].  With r = h / tau:
// p1 = m1 / h^2 = (1 - e (1 + r)) / r^2 and p2 = m2 / h^3 = 2 (1 - e (1 + r + r^2 / 2)) / r^3; below r = 1 the differences lose digits
// (they start at r^2 / 2 and r^3 / 6), so the series  p1 = sum_{k>=2} (-1)^k (k - 1) / k! r^(k-2),  p2 = sum_{k>=3} (-1)^(k+1) (k - 1)(k - 2) / k! r^(k-3)
int ihm2mpc_lag_stage_factors(double h, double tau, double *out4)
{
    if (!out4) return fail("null argument");
    if (!(h > 0.0) || !(tau > 0.0) || !std::isfinite(h) || !std::isfinite(tau)) return fail("h and tau must be positive and finite");
    const double r = h / tau, e = exp(-r);
    double p1, p2;
    if (r < 1.0) {
        p1 = 0.0; p2 = 0.0;
        double t = 0.5;          // r^(k-2) / k!, from k = 2
        for (int k = 2; k < 40; k++) {
            p1 += ((k & 1) ? -1.0 : 1.0) * (k - 1) * t;
            if (k >= 3) p2 += ((k & 1) ? 1.0 : -1.0) * (double)((k - 1) * (k - 2)) * t / r;
            t *= r / (k + 1);
        }
    } else {
        p1 = (1.0 - e * (1.0 + r)) / (r * r);
        p2 = 2.0 * (1.0 - e * (1.0 + r + 0.5 * r * r)) / (r * r * r);
    }
    const double E1 = 6.0 * (p1 - p2), E2 = 12.0 * p2 - 6.0 * p1;
    out4[0] = 6.0 * (-expm1(-r) / r) - 4.0 * E1 - E2;
    out4[1] = E1;
    out4[2] = E2;
    out4[3] = e;
    return 0;
}

int ihm2mpc_create(const ihm2mpc_config *cfg, ihm2mpc_handle **out)
{
    if (!cfg || !out) return fail("null argument");
    if (cfg->batch < 1) return fail("batch must be >= 1");
    if (cfg->N < 2 || cfg->N > IHM2MPC_NMAX) return fail("N must be in [2, %d]", IHM2MPC_NMAX);
    if (cfg->M < 1) return fail("M must be >= 1");
    if (cfg->integrator_type < IHM2MPC_INTEG_ERK || cfg->integrator_type > IHM2MPC_INTEG_ERK_LAG || cfg->sim_integrator_type < IHM2MPC_INTEG_ERK ||
        cfg->sim_integrator_type > IHM2MPC_INTEG_ERK_LAG)
        return fail("unknown integrator type (%d, %d)", cfg->integrator_type, cfg->sim_integrator_type);
    if (cfg->integrator_type == IHM2MPC_INTEG_ERK_LAG && cfg->model != IHM2MPC_MODEL_FKIN6)
        return fail("the integrator ERK_LAG (closed-form actuator lags) is implemented for the kinematic OCP model IHM2MPC_MODEL_FKIN6 only, not for "
                    "the dynamic models (model %d): use ERK or IRK", cfg->model);
    if (cfg->integrator_type == IHM2MPC_INTEG_ERK_LAG && cfg->nlp_solver_type != IHM2MPC_SQP_RTI)
        return fail("the integrator ERK_LAG (closed-form actuator lags) is implemented for IHM2MPC_SQP_RTI only: the SQP mode's line-search "
                    "rollouts have no such integrator; use ERK or IRK");
    if (ihm2_is_irk(cfg->integrator_type) && cfg->M != 1)
        return fail("the IRK integrator of the shooting intervals takes one step per interval (sim_method_num_steps = 1, python/main.py:236); M = %d", cfg->M);
    if (cfg->integrator_type == IHM2MPC_INTEG_ERK && rk4_unstable(cfg->dt, cfg->M))
        return fail("RK4 with %d sub-step(s) of dt = %g is unstable on the actuator lags (t_T = 1e-3 s, t_delta = 0.02 s: |z| = dt / (M t) must stay "
                    "below 2.78): use M >= %d (the reference's sim_method_num_steps = 1 belongs to its IRK integrator, python/main.py:234-236)",
                    cfg->M, cfg->dt, (int)ceil(cfg->dt / (2.78 * 1e-3)));
    if (cfg->model < IHM2MPC_MODEL_FKIN6 || cfg->model > IHM2MPC_MODEL_FDYN6U) return fail("unknown OCP model %d", cfg->model);
    if (cfg->ntracks < 1 || cfg->nknots < 2) return fail("need at least one track table with >= 2 knots");
    if (!(cfg->dt > 0.0)) return fail("dt must be positive");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) return fail("device %d out of range (%d devices)", cfg->device, ndev);
    HIP_TRY(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("libihm2mpc is built for gfx950 (MI355X) only; device %d is %s", cfg->device, prop.gcnArchName);

    auto h = std::make_unique<ihm2mpc_handle>();     // value-initialised (ihm2mpc_internal.h); released on every failure below
    h->cfg = *cfg;
    h->B = cfg->batch;
    h->N = cfg->N;
    h->NS = cfg->N + 1;
    h->n_cu = prop.multiProcessorCount;
    { const char *e = getenv("IHM2MPC_BLOCK_QP"); h->block_qp = !(e && e[0] == '0'); }
    { const char *e = getenv("IHM2MPC_POISON_WORKSPACE"); h->poison = e ? e : ""; arm_poison(h.get()); }
    const size_t B = h->B, N = h->N, NS = h->NS, nt = (size_t)cfg->ntracks * cfg->nknots;
    HIP_TRY(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    HIP_TRY(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
    for (int i = 0; i < 4; i++) HIP_TRY(hipEventCreate(&h->ev[i]));
    for (int i = 0; i < 2; i++) {      // pinned staging of the persistent loop's argument blocks (uploaded without a host wait)
        HIP_TRY(hipHostMalloc(&h->args_host[i], 1024, hipHostMallocDefault));
        HIP_TRY(hipEventCreateWithFlags(&h->args_ev[i], hipEventDisableTiming));
    }
    if (alloc_all(h->s_ref, nt, h->kappa_ref, nt, h->track_id, B, h->Hs, NS * 100, h->Gy, NS * 120, h->lbx, NS * 8, h->ubx, NS * 8,
                  h->lbu, N * 2, h->ubu, N * 2, h->CD, N * 20, h->lg, N * 2, h->ug, N * 2, h->slot_kc_blk, 1024, h->slot_lb_blk, 1024,
                  h->slot_ub_blk, 1024, h->slot_kc, MAX_SLOTS, h->slot_lb, 2 * MAX_SLOTS, h->slot_ub, 2 * MAX_SLOTS,
                  h->slk, B * NS * NLAM, h->widths, (size_t)cfg->ntracks * 2, h->lam_a, B * NS * 2, h->slk_a, B * NS * 2,
                  h->X_ref, nt, h->Y_ref, nt, h->phi_ref, nt, h->xc, B * 8, h->s_guess, B, h->step_args, 48, h->Wd, N * 144 + 64,
                  h->st_lb, NS * (NC + NLAM), h->st_ub, NS * (NC + NLAM), h->x, B * NS * 8, h->u, B * N * 2, h->x0, B * 8,
                  h->yref, B * N * 12, h->yref_e, B * 8, h->pi, B * NS * 8, h->lam, B * NS * NLAM, h->res, B * 4, h->qp_res, B * 4, h->status, B,
                  h->qp_iter, B, h->active, B, h->u0, B * 2,
                  h->lin, (B * N + B) * LIN_REC,      // + one spare record per instance (the kinematic plant's, never read)
                  h->q_g, B * NS * 10, h->q_rg, B * NS * 10, h->q_P, B * NS * 64, h->q_M, (B * N + 2 * QM_PAD) * 64, h->scratch, B * 24))
        return -1;
    h->slots_fit = true;
    h->slots_full = false;
    h->sqp_globalization = 0; h->sqp_use_suff = 0; h->sqp_full_step_dual = 0;
    h->sqp_alpha_min = 0.05; h->sqp_alpha_red = 0.7; h->sqp_eps = 1e-4;
    for (int i = 0; i < 4; i++) h->sqp_tol[i] = cfg->nlp_tol;
    h->rows = ihm2::ConstraintRows((int)NS);      // no row has a finite side yet; the a_lat row is off and hard
    if (ihm2_upload_irk_tab(h.get())) return fail("could not upload the collocation tableau");
    *out = h.release();
    return 0;
}

int ihm2mpc_free(ihm2mpc_handle *h)
{
    if (!h) return 0;
    (void)hipSetDevice(h->cfg.device);
    delete h;
    return 0;
}

int ihm2mpc_synchronize(ihm2mpc_handle *h)
{
    CHECK_H(h);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_get_stream(ihm2mpc_handle *h, void **stream)
{
    CHECK_H(h);
    if (!stream) return fail("null argument");
    *stream = (void *)h->stream;
    return 0;
}

int ihm2mpc_set_tracks(ihm2mpc_handle *h, const double *s_ref, const double *kappa_ref)
{
    CHECK_H(h);
    if (!s_ref || !kappa_ref) return fail("null argument");
    const size_t n = (size_t)h->cfg.ntracks * h->cfg.nknots;
    for (int t = 0; t < h->cfg.ntracks; t++)
        for (int i = 1; i < h->cfg.nknots; i++)
            if (!(s_ref[(size_t)t * h->cfg.nknots + i] > s_ref[(size_t)t * h->cfg.nknots + i - 1]))
                return fail("s_ref of track %d is not strictly increasing at knot %d", t, i);
    if (upload_shared(h, s_ref, h->s_ref, n) || upload_shared(h, kappa_ref, h->kappa_ref, n)) return -1;
    h->tracks_set = true;
    return 0;
}

int ihm2mpc_build_tracks(ihm2mpc_handle *h, int32_t max_seg, const int32_t *nseg, const double *coeffs_X, const double *coeffs_Y)
{
    CHECK_H(h);
    if (!nseg || !coeffs_X || !coeffs_Y) return fail("null argument");
    if (h->cfg.nknots % 3 != 0) return fail("nknots = %d is not three laps of samples", h->cfg.nknots);
    if (max_seg < 2) return fail("max_seg must be >= 2");
    for (int t = 0; t < h->cfg.ntracks; t++)
        if (nseg[t] < 2 || nseg[t] > max_seg) return fail("track %d has %d spline segments (2 .. max_seg = %d)", t, nseg[t], max_seg);
    const size_t nc = (size_t)h->cfg.ntracks * max_seg;
    StateBuf<double> dev;            // the uploaded coefficients
    WorkBuf<double> dwork;           // "track_work": segment lengths, then their running sums
    StateBuf<int32_t> dseg;
    dwork.poison(poisoned(h, "track_work"));
    HIP_TRY(dev.alloc(nc * 8));
    if (dwork.alloc(nc) != hipSuccess || dseg.alloc(h->cfg.ntracks) != hipSuccess) return fail("out of device memory");
    double *cX = dev, *cY = dev + nc * 4, *work = dwork;
    if (hipMemcpyAsync(cX, coeffs_X, nc * 4 * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(cY, coeffs_Y, nc * 4 * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(dseg, nseg, h->cfg.ntracks * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail("upload of the spline coefficients failed");
    ihm2_launch_build_tracks(h, max_seg, dseg, cX, cY, work);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return fail("track-table kernels failed");
    h->tracks_set = true; h->geometry_set = true;
    return 0;
}

int ihm2mpc_fit_tracks(ihm2mpc_handle *h, int32_t max_pts, const int32_t *npts, const double *xy, double curv_weight, double *coeffs_X, double *coeffs_Y)
{
    CHECK_H(h);
    if (!npts || !xy || !coeffs_X || !coeffs_Y) return fail("null argument");
    if (!(curv_weight >= 0.0)) return fail("curv_weight must be >= 0");
    if (max_pts < 3 || 7 * max_pts + 2 > 1280) return fail("max_pts must be in 3 .. 182 (the elimination lists the non-zeros of a row in LDS)");
    const int nt = h->cfg.ntracks;
    for (int t = 0; t < nt; t++)
        if (npts[t] < 3 || npts[t] > max_pts) return fail("track %d has %d centre-line points (3 .. max_pts = %d)", t, npts[t], max_pts);
    const size_t m = 7 * (size_t)max_pts, nwork = (size_t)nt * m * (m + 2), nxy = (size_t)nt * max_pts * 2, nc = (size_t)nt * max_pts * 4;
    StateBuf<double> dev;        // the uploaded points, then cX, cY: the rows past a track's npts are returned as 0 (include/ihm2mpc.h), the fill's value
    WorkBuf<double> dwork;       // "track_work": the augmented KKT matrices (k_track_fit clears the part it uses)
    StateBuf<int32_t> di;
    dwork.poison(poisoned(h, "track_work"));
    HIP_TRY(dev.alloc(nxy + 2 * nc));
    if (dwork.alloc(nwork) != hipSuccess || di.alloc(2 * (size_t)nt) != hipSuccess) return fail("out of device memory");
    double *work = dwork, *dxy = dev, *cX = dxy + nxy, *cY = cX + nc;
    std::vector<int32_t> flags(nt, 1);
    if (hipMemcpyAsync(dxy, xy, nxy * sizeof(double), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemcpyAsync(di, npts, nt * sizeof(int32_t), hipMemcpyHostToDevice, h->stream) != hipSuccess) return fail("upload of the centre lines failed");
    ihm2_launch_track_fit(h, max_pts, di, dxy, curv_weight, work, cX, cY, di + nt);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(coeffs_X, cX, nc * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(coeffs_Y, cY, nc * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipMemcpyAsync(flags.data(), di + nt, nt * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
        hipStreamSynchronize(h->stream) != hipSuccess) return fail("spline-fit kernel failed");
    for (int t = 0; t < nt; t++)
        if (flags[t]) return fail("the spline fit of track %d is singular (coincident centre-line points?)", t);
    return 0;
}

int ihm2mpc_get_tracks(ihm2mpc_handle *h, double *s_ref, double *kappa_ref, double *X_ref, double *Y_ref, double *phi_ref)
{
    CHECK_H(h);
    if (!h->tracks_set) return fail("no track tables yet");
    const size_t n = (size_t)h->cfg.ntracks * h->cfg.nknots * sizeof(double);
    const double *src[5] = {h->s_ref, h->kappa_ref, h->X_ref, h->Y_ref, h->phi_ref};
    double *dst[5] = {s_ref, kappa_ref, X_ref, Y_ref, phi_ref};
    for (int i = 0; i < 5; i++)
        if (dst[i]) {
            if (i >= 2 && !h->geometry_set) return fail("ihm2mpc_set_track_geometry / ihm2mpc_build_tracks has not been called");
            HIP_TRY(hipMemcpyAsync(dst[i], src[i], n, hipMemcpyDeviceToHost, h->stream));
        }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_set_track_id(ihm2mpc_handle *h, const int32_t *track_id)
{
    CHECK_H(h);
    if (!track_id) return fail("null argument");
    for (int b = 0; b < h->B; b++)
        if (track_id[b] < 0 || track_id[b] >= h->cfg.ntracks) return fail("track_id[%d] = %d out of range", b, track_id[b]);
    HIP_TRY(hipMemcpyAsync(h->track_id, track_id, (size_t)h->B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_set_weights(ihm2mpc_handle *h, const double *W, const double *W_e)
{
    CHECK_H(h);
    if (!W || !W_e) return fail("null argument");
    const int N = h->N, NS = h->NS;
    std::vector<double> Hs((size_t)NS * 100, 0.0), Gy((size_t)NS * 120, 0.0);
    const double cs = h->cfg.cost_scale_stage;
    for (int k = 0; k < N; k++) ihm2::stage_weight_tables(W + (size_t)k * NY * NY, cs, &Hs[(size_t)k * 100], &Gy[(size_t)k * 120]);
    ihm2::terminal_weight_tables(W_e, &Hs[(size_t)N * 100], &Gy[(size_t)N * 120]);
    for (int k = 0; k < NS; k++)
        if (!ihm2::symmetric10(&Hs[(size_t)k * 100])) return fail("weight matrix of stage %d is not symmetric", k);
    // "uniform" covers the gradient map as well: the QP kernel keeps one copy of both
    const bool uni = ihm2::stages_equal(Hs.data(), N, 100) && ihm2::stages_equal(Gy.data(), N, 120);
    if (upload_shared(h, Hs.data(), h->Hs, Hs.size()) || upload_shared(h, Gy.data(), h->Gy, Gy.size())) return -1;
    if (upload_shared(h, W, h->Wd, (size_t)N * 144) || upload_shared(h, W_e, h->Wd + (size_t)N * 144, 64)) return -1;
    h->shared_uniform_H = uni;
    h->uniform_H = h->inst_w || uni;       // per-instance weights are stage-independent whatever the shared table holds
    h->weights_set = true;
    return 0;
}

// One weight set per instance: W (B,12,12) for every stage k < N, W_e (B,8,8) -- acados' per-solver
// cost_set(k, "W", W) / cost_set(N, "W", W_e) (python/main.py:248-292).  Expanded by the code of ihm2mpc_set_weights.
int ihm2mpc_set_instance_weights(ihm2mpc_handle *h, const double *W, const double *W_e)
{
    CHECK_H(h);
    if (!W && !W_e) {
        h->iHs.reset(); h->iGy.reset(); h->iWd.reset();
        h->inst_w = false;
        h->uniform_H = h->shared_uniform_H;
        return 0;
    }
    if (!W || !W_e) return fail("W and W_e must both be given, or both be NULL (batch-shared weights again)");
    if (!h->weights_set) return fail("ihm2mpc_set_weights has not been called (the batch-shared weights come first)");
    if (h->bounds_set && !h->uniform_CD) return fail("per-instance weights need stage-independent general rows C, D");
    const int B = h->B;
    std::vector<double> Hs((size_t)B * 200, 0.0), Gy((size_t)B * 240, 0.0), Wd((size_t)B * 208);
    const double cs = h->cfg.cost_scale_stage;
    for (int b = 0; b < B; b++) {
        const double *Wb = W + (size_t)b * 144, *Web = W_e + (size_t)b * 64;
        for (int i = 0; i < 144; i++) if (Wb[i] != Wb[i]) return fail("instance %d: W[%d][%d] is NaN", b, i / 12, i % 12);
        for (int i = 0; i < 64; i++) if (Web[i] != Web[i]) return fail("instance %d: W_e[%d][%d] is NaN", b, i / 8, i % 8);
        double *Hb = &Hs[(size_t)b * 200], *Gb = &Gy[(size_t)b * 240];
        ihm2::stage_weight_tables(Wb, cs, Hb, Gb);
        ihm2::terminal_weight_tables(Web, Hb + 100, Gb + 120);
        if (!ihm2::symmetric10(Hb)) return fail("instance %d: the weight matrix of the stages 0..%d is not symmetric", b, h->N - 1);
        if (!ihm2::symmetric10(Hb + 100)) return fail("instance %d: the weight matrix of stage %d (terminal) is not symmetric", b, h->N);
        std::memcpy(&Wd[(size_t)b * 208], Wb, 144 * sizeof(double));
        std::memcpy(&Wd[(size_t)b * 208 + 144], Web, 64 * sizeof(double));
    }
    if (!h->iHs && alloc_all(h->iHs, (size_t)B * 200, h->iGy, (size_t)B * 240, h->iWd, (size_t)B * 208)) return -1;
    if (upload_shared(h, Hs.data(), h->iHs, Hs.size()) || upload_shared(h, Gy.data(), h->iGy, Gy.size()) ||
        upload_shared(h, Wd.data(), h->iWd, Wd.size()))
        return -1;
    h->inst_w = true;
    h->uniform_H = true;
    return 0;
}

// The same from W (B,12,12), W_e (B,8,8) in device memory: k_weight_tables (kernels_weights.hip) expands on h->stream what the loop above
// expands on the host, bit for bit.  check: the kernel's validating form runs first and its codes are read back (blocking) -- nothing of
// the handle is written before every instance is accepted.
int ihm2mpc_set_instance_weights_device(ihm2mpc_handle *h, const void *W, const void *W_e, int32_t check)
{
    CHECK_H(h);
    if (!W && !W_e) return ihm2mpc_set_instance_weights(h, nullptr, nullptr);
    if (!W || !W_e) return fail("W and W_e must both be given, or both be NULL (batch-shared weights again)");
    if (!h->weights_set) return fail("ihm2mpc_set_weights has not been called (the batch-shared weights come first)");
    if (h->bounds_set && !h->uniform_CD) return fail("per-instance weights need stage-independent general rows C, D");
    const int B = h->B;
    const double *dW = (const double *)W, *dWe = (const double *)W_e;
    if (check) {
        WorkBuf<int32_t> dcode;     // (B) the kernel writes every entry
        if (dcode.alloc(B) != hipSuccess) return fail("out of device memory");
        ihm2_launch_weight_tables(h, dW, dWe, nullptr, nullptr, nullptr, dcode);
        HIP_TRY(hipGetLastError());
        std::vector<int32_t> code(B);
        HIP_TRY(hipMemcpyAsync(code.data(), dcode, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int b = 0; b < B; b++) {
            const int c = code[b];
            if (c == ihm2_weight_code_ok) continue;
            if (c == ihm2_weight_code_asym_terminal)
                return fail("instance %d: the weight matrix of stage %d (terminal) is not symmetric", b, h->N);
            if (c == ihm2_weight_code_asym_stage) return fail("instance %d: the weight matrix of the stages 0..%d is not symmetric", b, h->N - 1);
            if (c >= ihm2_weight_code_nan_We) {
                const int i = c - ihm2_weight_code_nan_We;
                return fail("instance %d: W_e[%d][%d] is NaN", b, i / 8, i % 8);
            }
            const int i = c - ihm2_weight_code_nan_W;
            return fail("instance %d: W[%d][%d] is NaN", b, i / 12, i % 12);
        }
    }
    if (!h->iHs && alloc_all(h->iHs, (size_t)B * 200, h->iGy, (size_t)B * 240, h->iWd, (size_t)B * 208)) return -1;
    ihm2_launch_weight_tables(h, dW, dWe, h->iHs, h->iGy, h->iWd, nullptr);
    HIP_TRY(hipGetLastError());
    h->inst_w = true;
    h->uniform_H = true;
    return 0;
}

int ihm2mpc_get_instance_weight_tables(ihm2mpc_handle *h, double *Hs, double *Gy, double *Wd)
{
    CHECK_H(h);
    if (!h->inst_w) return fail("per-instance weights are off: ihm2mpc_set_instance_weights or ihm2mpc_set_instance_weights_device first");
    const size_t B = h->B;
    if (Hs) HIP_TRY(hipMemcpyAsync(Hs, h->iHs, B * 200 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Gy) HIP_TRY(hipMemcpyAsync(Gy, h->iGy, B * 240 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (Wd) HIP_TRY(hipMemcpyAsync(Wd, h->iWd, B * 208 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

// The constraint-slot table of the QP kernels from the handle's rows (qp_tables.hpp: lay_out_slots, for the instantiations the catalogue
// has for these rows).  A table that fits none leaves the previous one in the handle: ready() reports it, since the setters come one by one
// and a later one may make the rows fit.
static int rebuild_slots(ihm2mpc_handle *h)
{
    ihm2::SlotTable t = ihm2::lay_out_slots(h->rows, ihm2::slot_limits(path_class(h)));
    h->slots_fit = t.fit;
    h->slots_full = false;      // (a table that does not fit: launches are refused)
    if (!t.fit) return 0;
    h->slots = std::move(t);
    h->inst_images = false;     // the per-instance images are the previous table's, in length too, until tables_to_device has succeeded
    const ihm2::SlotTable &s = h->slots;
    if (s.per_blk) {
        HIP_TRY(hipMemcpyAsync(h->slot_kc_blk, s.kc_blk.data(), s.kc_blk.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (upload_shared(h, s.lb_blk.data(), h->slot_lb_blk, s.lb_blk.size()) || upload_shared(h, s.ub_blk.data(), h->slot_ub_blk, s.ub_blk.size())) return -1;
    }
    if (const size_t n = s.entries()) {
        HIP_TRY(hipMemcpyAsync(h->slot_kc, s.kc.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return tables_to_device(h);     // the bounds and penalties of the new table, per instance too (or a refusal: ready() then reports it)
}

int ihm2mpc_set_bounds(ihm2mpc_handle *h, const double *lbx, const double *ubx, const double *lbu, const double *ubu,
                       const double *C, const double *D, const double *lg, const double *ug)
{
    CHECK_H(h);
    if (!lbx || !ubx || !lbu || !ubu || !C || !D || !lg || !ug) return fail("null argument");
    const int N = h->N, NS = h->NS;
    for (int i = 0; i < NS * NX; i++) if (lbx[i] > ubx[i]) return fail("lbx > ubx at flat index %d", i);
    for (int i = 0; i < N * NU; i++) if (lbu[i] > ubu[i]) return fail("lbu > ubu at flat index %d", i);
    for (int i = 0; i < N * NG; i++) if (lg[i] > ug[i]) return fail("lg > ug at flat index %d", i);
    std::vector<double> CD((size_t)N * 20);
    for (int k = 0; k < N; k++)
        for (int r = 0; r < NG; r++) {
            for (int j = 0; j < NX; j++) CD[((size_t)k * 2 + r) * 10 + j] = C[((size_t)k * 2 + r) * NX + j];
            for (int j = 0; j < NU; j++) CD[((size_t)k * 2 + r) * 10 + 8 + j] = D[((size_t)k * 2 + r) * NU + j];
        }
    h->uniform_CD = ihm2::stages_equal(CD.data(), N, 20);
    h->rows.set_box_rows(lbx, ubx, lbu, ubu, lg, ug);
    if (rebuild_slots(h)) return -1;
    if (upload_shared(h, lbx, h->lbx, (size_t)NS * 8) || upload_shared(h, ubx, h->ubx, (size_t)NS * 8) ||
        upload_shared(h, lbu, h->lbu, (size_t)N * 2) || upload_shared(h, ubu, h->ubu, (size_t)N * 2) ||
        upload_shared(h, CD.data(), h->CD, CD.size()) || upload_shared(h, lg, h->lg, (size_t)N * 2) ||
        upload_shared(h, ug, h->ug, (size_t)N * 2))
        return -1;
    h->bounds_set = true;
    return 0;
}

// The bound values per instance: lbx/ubx (B,N+1,8) (stage 0 unused: x_0 is fixed), lbu/ubu (B,N,2), lg/ug (B,N,2) -- acados' per-solver
// constraints_set(k, "lbx" / "ubx" / "lbu" / "ubu" / "lg" / "ug", ...) (python/main.py:248-292).  The finite sides must be those of the
// batch-shared table (|v| >= 1e20: absent); C, D, soft penalties, track rows and the a_lat row stay batch-shared.
int ihm2mpc_set_instance_bounds(ihm2mpc_handle *h, const double *lbx, const double *ubx, const double *lbu, const double *ubu,
                                const double *lg, const double *ug)
{
    CHECK_H(h);
    const bool none = !lbx && !ubx && !lbu && !ubu && !lg && !ug;
    if (none) {
        HIP_TRY(hipStreamSynchronize(h->stream));       // a launch in flight may still read the arrays
        h->i_lbu.reset(); h->i_ubu.reset(); h->i_lg.reset(); h->i_ug.reset();
        h->ih_lb = std::vector<double>(); h->ih_ub = std::vector<double>();
        h->inst_b = false;
        return tables_to_device(h);     // the batch-shared bounds again, beside the per-instance penalties if there are any
    }
    if (!lbx || !ubx || !lbu || !ubu || !lg || !ug) return fail("lbx, ubx, lbu, ubu, lg, ug must all be given, or all be NULL (batch-shared bounds again)");
    if (!h->bounds_set) return fail("ihm2mpc_set_bounds has not been called (the batch-shared table gives the pattern)");
    const int B = h->B, N = h->N, NS = h->NS;
    std::vector<double> il((size_t)B * NS * 12), iu((size_t)B * NS * 12);
    for (int b = 0; b < B; b++) {
        const double *xl = lbx + (size_t)b * NS * 8, *xu = ubx + (size_t)b * NS * 8, *ul = lbu + (size_t)b * N * 2, *uu = ubu + (size_t)b * N * 2;
        const double *gl = lg + (size_t)b * N * 2, *gu = ug + (size_t)b * N * 2;
        for (int k = 0; k < NS; k++)
            for (int c = 0; c < 12; c++) {
                const auto [lb, ub] = ihm2::box_row(N, k, c, xl, xu, ul, uu, gl, gu);
                if (lb != lb || ub != ub) return fail("instance %d, stage %d, row %d (%s): bound is NaN", b, k, c, row_name(c));
                if (lb > ub) return fail("instance %d, stage %d, row %d (%s): lower bound %g > upper bound %g", b, k, c, row_name(c), lb, ub);
            }
        ihm2::box_rows(N, xl, xu, ul, uu, gl, gu, &il[(size_t)b * NS * 12], &iu[(size_t)b * NS * 12], 12);      // as ihm2mpc_set_bounds
    }
    // the pattern check before anything of the handle changes
    if (check_instance_pattern(h, il.data(), iu.data())) return -1;
    const size_t nb = (size_t)B;
    if (!h->i_lbu && alloc_all(h->i_lbu, nb * N * 2, h->i_ubu, nb * N * 2, h->i_lg, nb * N * 2, h->i_ug, nb * N * 2))
        return -1;
    h->ih_lb = std::move(il); h->ih_ub = std::move(iu);
    if (upload_shared(h, lbu, h->i_lbu, (size_t)B * N * 2) || upload_shared(h, ubu, h->i_ubu, (size_t)B * N * 2) ||
        upload_shared(h, lg, h->i_lg, (size_t)B * N * 2) || upload_shared(h, ug, h->i_ug, (size_t)B * N * 2))
        return -1;
    h->inst_b = true;
    return tables_to_device(h);
}

int ihm2mpc_set_soft(ihm2mpc_handle *h, const double *soft_z, const double *soft_Z)
{
    CHECK_H(h);
    const int n = h->NS * NLAM;
    if ((soft_z == nullptr) != (soft_Z == nullptr)) return fail("soft_z and soft_Z must both be given or both be NULL");
    for (int i = 0; i < n; i++) {
        const double Z = soft_Z ? soft_Z[i] : -1.0, z = soft_z ? soft_z[i] : 0.0;
        if (Z >= 0.0 && !(z >= 0.0)) return fail("soft_z < 0 at flat index %d (the slack penalty must be non-decreasing)", i);
        if (Z >= 0.0 && !(Z + z > 0.0)) return fail("soft side %d has neither a linear nor a quadratic penalty", i);
        h->rows.sz[i] = z; h->rows.sZ[i] = Z;
    }
    HIP_TRY(hipMemsetAsync(h->slk, 0, (size_t)h->B * h->NS * NLAM * sizeof(double), h->stream));
    if (h->bounds_set && rebuild_slots(h)) return -1;
    return 0;
}

// The slack penalties per instance: the values of the soft sides, the pattern (which sides are soft) from the batch-shared setters.
// Both entries keep their values on the host and share one mode for the kernels; the mode goes when both are off.
static int instance_penalties_changed(ihm2mpc_handle *h)
{
    h->inst_p = !h->ih_sz.empty() || !h->ih_az.empty() || h->dev_sp || h->dev_ap;
    return tables_to_device(h);
}

// the new values of one entry into the handle (empty vectors: shared again); on a failure the previous ones are put back, on the host and,
// as far as that still succeeds, on the device
// (dev: the pair's device-set mark, which the host's values replace)
static int take_instance_penalties(ihm2mpc_handle *h, std::vector<double> &z, std::vector<double> &Z, int &dev, std::vector<double> nz, std::vector<double> nZ)
{
    const int was = dev;
    z.swap(nz); Z.swap(nZ); dev = 0;
    if (instance_penalties_changed(h) == 0) return 0;
    const std::string why = ihm2mpc_last_error();
    z.swap(nz); Z.swap(nZ);
    dev = was ? 2 : 0;      // (its values may be gone from the images: they count as not fitting)
    (void)instance_penalties_changed(h);
    return fail("%s", why.c_str());
}

int ihm2mpc_set_instance_soft(ihm2mpc_handle *h, const double *soft_z, const double *soft_Z)
{
    CHECK_H(h);
    if (!soft_z && !soft_Z) {
        return take_instance_penalties(h, h->ih_sz, h->ih_sZ, h->dev_sp, {}, {});
    }
    if (!soft_z || !soft_Z) return fail("soft_z and soft_Z must both be given, or both be NULL (batch-shared penalties again)");
    bool any = false;
    for (double Z : h->rows.sZ) any = any || Z >= 0.0;
    if (!any) return fail("ihm2mpc_set_soft has not been called with a soft side (the batch-shared table gives the pattern)");
    // the pattern check before anything of the handle changes (a failure behind it puts the previous values back)
    if (check_penalty_pattern(h, soft_z, soft_Z, nullptr, nullptr)) return -1;
    const size_t n = (size_t)h->B * h->NS * NLAM;
    return take_instance_penalties(h, h->ih_sz, h->ih_sZ, h->dev_sp, std::vector<double>(soft_z, soft_z + n), std::vector<double>(soft_Z, soft_Z + n));
}

int ihm2mpc_set_instance_alat_soft(ihm2mpc_handle *h, const double *soft_z, const double *soft_Z)
{
    CHECK_H(h);
    if (!soft_z && !soft_Z) {
        return take_instance_penalties(h, h->ih_az, h->ih_aZ, h->dev_ap, {}, {});
    }
    if (!soft_z || !soft_Z) return fail("soft_z and soft_Z must both be given, or both be NULL (batch-shared penalties again)");
    if (!h->rows.alat_on || !(h->rows.alat_sZ[0] >= 0.0 || h->rows.alat_sZ[1] >= 0.0))
        return fail("ihm2mpc_set_alat_constraint has not been called with a soft side (the batch-shared a_lat row gives the pattern)");
    if (check_penalty_pattern(h, nullptr, nullptr, soft_z, soft_Z)) return -1;
    const size_t n = (size_t)h->B * 2;
    return take_instance_penalties(h, h->ih_az, h->ih_aZ, h->dev_ap, std::vector<double>(soft_z, soft_z + n), std::vector<double>(soft_Z, soft_Z + n));
}

// The same two setters from device memory.  k_penalty_check stands for check_penalty_pattern (its codes are read back and turned into
// that function's messages before anything of the handle changes), k_penalty_tables for the penalty part of table_images.  The images
// exist before the kernel runs: tables_to_device builds them with the shared penalties when the per-instance tables are not there yet
// or do not hold what the handle believes (a pattern change, a refused host pair), which is the one blocking step of an unchecked call.
static int penalty_refusal(const ihm2mpc_handle *h, int alat, int b, int code, const double *shared_Z)
{
    const int idx = (code - 1) / 4, kind = (code - 1) % 4 + 1;
    const int k = alat ? 0 : idx / NLAM, side = alat ? NLAM + idx : idx % NLAM;
    const bool shared_soft = shared_Z[idx] >= 0.0;
    switch (kind) {
    case ihm2_penalty_nan: return fail("instance %d, stage %d, side %d (%s): slack penalty is NaN", b, k, side, side_name(side));
    case ihm2_penalty_flag:     // (the instance's flag is the opposite of the shared one: that is the offence)
        return fail("instance %d, stage %d, side %d (%s): the side is %s (soft_Z %s 0) where the batch-shared table holds it %s", b, k, side,
                    side_name(side), !shared_soft ? "soft" : "hard", !shared_soft ? ">=" : "<", shared_soft ? "soft" : "hard");
    case ihm2_penalty_negative:
        return fail("instance %d, stage %d, side %d (%s): soft_z < 0 (the slack penalty must be non-decreasing)", b, k, side, side_name(side));
    default:
        return fail("instance %d, stage %d, side %d (%s): the soft side has neither a linear nor a quadratic penalty", b, k, side, side_name(side));
    }
}

static int set_instance_penalties_device(ihm2mpc_handle *h, int alat, const double *z, const double *Z, int32_t check)
{
    if (!h->bounds_set) return fail("ihm2mpc_set_bounds has not been called (the batch-shared table gives the pattern)");
    const int B = h->B;
    if (check) {
        WorkBuf<int32_t> dcode;     // (B) the kernel writes every entry
        if (dcode.alloc(B) != hipSuccess) return fail("out of device memory");
        ihm2_launch_penalty_check(h, alat, z, Z, dcode);
        HIP_TRY(hipGetLastError());
        std::vector<int32_t> code(B);
        HIP_TRY(hipMemcpyAsync(code.data(), dcode, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        for (int b = 0; b < B; b++)
            if (code[b]) return penalty_refusal(h, alat, b, code[b], alat ? h->rows.alat_sZ : h->rows.sZ.data());
    }
    std::vector<double> &hz = alat ? h->ih_az : h->ih_sz, &hZ = alat ? h->ih_aZ : h->ih_sZ;
    int &dev = alat ? h->dev_ap : h->dev_sp;
    // the device's values replace the pair's previous ones, which are kept until the images are there: on a failure they are put back,
    // on the host and, as far as that still succeeds, on the device, as take_instance_penalties does (a device-set pair's values may
    // be gone from the images by then: it counts as not fitting)
    std::vector<double> oz, oZ;
    const int was = dev;
    const bool was_on = h->inst_p;
    hz.swap(oz); hZ.swap(oZ);
    dev = 0;
    // the images are there, with the host-held penalties in place (the other pair's device-set values are wherever they are valid)
    // (inst_images: they are those of h->slots -- a shared setter that was refused half-way leaves the previous table's, of another length)
    const bool images = h->inst_images && h->inst_p && h->i_st_lb && h->ip.alat_sz && h->host_p_fit;
    if (!images) {
        h->inst_p = true;
        if (tables_to_device(h)) {
            const std::string why = ihm2mpc_last_error();
            hz.swap(oz); hZ.swap(oZ);
            dev = was ? 2 : 0;
            h->inst_p = was_on;
            (void)tables_to_device(h);
            return fail("%s", why.c_str());
        }
    }
    ihm2_launch_penalty_tables(h, alat, z, Z, alat ? 2 : (size_t)h->NS * NLAM, 1);
    HIP_TRY(hipGetLastError());
    dev = 1;
    if (alat) h->dev_ap_flags = soft_flags(h->rows.alat_sZ, 2);
    else h->dev_sp_flags = soft_flags(h->rows.sZ.data(), h->rows.sZ.size());
    h->inst_p_ok = h->host_p_fit && h->dev_sp != 2 && h->dev_ap != 2;
    return 0;
}

int ihm2mpc_set_instance_soft_device(ihm2mpc_handle *h, const void *soft_z, const void *soft_Z, int32_t check)
{
    CHECK_H(h);
    if (!soft_z && !soft_Z) return ihm2mpc_set_instance_soft(h, nullptr, nullptr);
    if (!soft_z || !soft_Z) return fail("soft_z and soft_Z must both be given, or both be NULL (batch-shared penalties again)");
    bool any = false;
    for (double Z : h->rows.sZ) any = any || Z >= 0.0;
    if (!any) return fail("ihm2mpc_set_soft has not been called with a soft side (the batch-shared table gives the pattern)");
    return set_instance_penalties_device(h, 0, (const double *)soft_z, (const double *)soft_Z, check);
}

int ihm2mpc_set_instance_alat_soft_device(ihm2mpc_handle *h, const void *soft_z, const void *soft_Z, int32_t check)
{
    CHECK_H(h);
    if (!soft_z && !soft_Z) return ihm2mpc_set_instance_alat_soft(h, nullptr, nullptr);
    if (!soft_z || !soft_Z) return fail("soft_z and soft_Z must both be given, or both be NULL (batch-shared penalties again)");
    if (!h->rows.alat_on || !(h->rows.alat_sZ[0] >= 0.0 || h->rows.alat_sZ[1] >= 0.0))
        return fail("ihm2mpc_set_alat_constraint has not been called with a soft side (the batch-shared a_lat row gives the pattern)");
    return set_instance_penalties_device(h, 1, (const double *)soft_z, (const double *)soft_Z, check);
}

// the penalty halves of the per-instance images, to host arrays: slot_z, slot_Z (B,MAX_SLOTS) -- the table's entries in table order, then
// padding (0, -1) --, stage_z, stage_Z (B,NS,28), alat_z, alat_Z (B,2) (the shared pair while no per-instance penalty is on)
int ihm2mpc_get_instance_penalty_tables(ihm2mpc_handle *h, double *slot_z, double *slot_Z, double *stage_z, double *stage_Z, double *alat_z,
                                        double *alat_Z)
{
    CHECK_H(h);
    if (h->i_st_lb && !h->inst_images)
        return fail("the per-instance constraint tables are not those of the current constraint rows: a setter behind them was refused "
                    "(its message said why); settle that first");
    if (!h->i_st_lb)
        return fail("the per-instance constraint tables do not exist: ihm2mpc_set_instance_soft, ihm2mpc_set_instance_alat_soft, their _device "
                    "forms or ihm2mpc_set_instance_bounds first");
    const size_t B = h->B, n = h->slots.entries(), nb = (size_t)h->NS * NC, np = (size_t)h->NS * NLAM, D = sizeof(double);
    for (size_t b = 0; b < B; b++)
        for (size_t e = n; e < MAX_SLOTS; e++) {
            if (slot_z) slot_z[b * MAX_SLOTS + e] = ihm2::slot_detail::PADDING.zw;
            if (slot_Z) slot_Z[b * MAX_SLOTS + e] = ihm2::slot_detail::PADDING.Zw;
        }
    if (slot_z && n) HIP_TRY(hipMemcpy2DAsync(slot_z, MAX_SLOTS * D, h->i_slot_lb + n, 2 * n * D, n * D, B, hipMemcpyDeviceToHost, h->stream));
    if (slot_Z && n) HIP_TRY(hipMemcpy2DAsync(slot_Z, MAX_SLOTS * D, h->i_slot_ub + n, 2 * n * D, n * D, B, hipMemcpyDeviceToHost, h->stream));
    if (stage_z) HIP_TRY(hipMemcpy2DAsync(stage_z, np * D, h->i_st_lb + nb, (nb + np) * D, np * D, B, hipMemcpyDeviceToHost, h->stream));
    if (stage_Z) HIP_TRY(hipMemcpy2DAsync(stage_Z, np * D, h->i_st_ub + nb, (nb + np) * D, np * D, B, hipMemcpyDeviceToHost, h->stream));
    if (h->ip.alat_sz) {
        if (alat_z) HIP_TRY(hipMemcpyAsync(alat_z, h->ip.alat_sz, B * 2 * D, hipMemcpyDeviceToHost, h->stream));
        if (alat_Z) HIP_TRY(hipMemcpyAsync(alat_Z, h->ip.alat_sZ, B * 2 * D, hipMemcpyDeviceToHost, h->stream));
    } else
        for (size_t i = 0; i < B * 2; i++) {
            if (alat_z) alat_z[i] = h->rows.alat_sz[i & 1];
            if (alat_Z) alat_Z[i] = h->rows.alat_sZ[i & 1];
        }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_set_path_constraints(ihm2mpc_handle *h, int32_t enable, double car_length, double car_width, const double *widths,
                                 const double *lh, const double *uh)
{
    CHECK_H(h);
    if (enable) {
        if (!widths || !lh || !uh) return fail("null argument");
        if (!(car_length >= 0.0) || !(car_width >= 0.0)) return fail("car_length and car_width must be non-negative");
        for (int i = 0; i < NH; i++) if (lh[i] > uh[i]) return fail("lh > uh at row %d", i);
        for (int t = 0; t < h->cfg.ntracks * 2; t++) if (!(widths[t] > 0.0)) return fail("track width %d is not positive", t);
        if (upload_shared(h, widths, h->widths, (size_t)h->cfg.ntracks * 2)) return -1;
        h->car_L = car_length; h->car_W = car_width;
    }
    h->path_on = enable ? 1 : 0;
    h->rows.set_track_rows(enable != 0, lh, uh);
    if (h->bounds_set && rebuild_slots(h)) return -1;
    return 0;
}

int ihm2mpc_set_alat_constraint(ihm2mpc_handle *h, int32_t enable, double a_lat_min, double a_lat_max, const double *soft_z, const double *soft_Z)
{
    CHECK_H(h);
    if (enable) {
        if (a_lat_min != a_lat_min || a_lat_max != a_lat_max) return fail("a_lat bound is not a number");
        if (a_lat_min > a_lat_max) return fail("a_lat_min > a_lat_max");
        for (int i = 0; i < 2; i++) {
            const double z = soft_z ? soft_z[i] : 0.0, Z = soft_Z ? soft_Z[i] : -1.0;
            if (z != z || Z != Z) return fail("soft penalty of the a_lat row is not a number");
            if (Z >= 0.0 && !(z >= 0.0)) return fail("soft_z < 0 on the a_lat row (the slack penalty must be non-decreasing)");
            if (Z >= 0.0 && !(Z + z > 0.0)) return fail("a soft side of the a_lat row has neither a linear nor a quadratic penalty");
            h->rows.alat_sz[i] = z; h->rows.alat_sZ[i] = Z;
        }
        h->rows.alat_lb = ihm2::bound_or(a_lat_min, -INFINITY);
        h->rows.alat_ub = ihm2::bound_or(a_lat_max, INFINITY);
    }
    h->rows.alat_on = enable ? 1 : 0;
    HIP_TRY(hipMemsetAsync(h->lam_a, 0, (size_t)h->B * h->NS * 2 * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(h->slk_a, 0, (size_t)h->B * h->NS * 2 * sizeof(double), h->stream));
    if (h->bounds_set && rebuild_slots(h)) return -1;
    return 0;
}

int ihm2mpc_set_alat_multipliers(ihm2mpc_handle *h, const double *lam, const double *slk)
{
    CHECK_H(h);
    if (lam) { if (upload(h, lam, h->lam_a, h->NS * 2)) return -1; }
    else HIP_TRY(hipMemsetAsync(h->lam_a, 0, (size_t)h->B * h->NS * 2 * sizeof(double), h->stream));
    if (slk) { if (upload(h, slk, h->slk_a, h->NS * 2)) return -1; }
    else HIP_TRY(hipMemsetAsync(h->slk_a, 0, (size_t)h->B * h->NS * 2 * sizeof(double), h->stream));
    return 0;
}

int ihm2mpc_get_alat_multipliers(ihm2mpc_handle *h, double *lam, double *slk)
{
    CHECK_H(h);
    if (lam && download(h, h->lam_a, lam, h->NS * 2)) return -1;
    if (slk && download(h, h->slk_a, slk, h->NS * 2)) return -1;
    return 0;
}

#define SETTER(name, field, elems)                                   \
    int ihm2mpc_set_##name(ihm2mpc_handle *h, const double *v)       \
    {                                                                \
        CHECK_H(h);                                                  \
        if (!v) return fail("null argument");                        \
        return upload(h, v, h->field, (elems));                      \
    }
SETTER(x0, x0, NX)
SETTER(x, x, h->NS * NX)
SETTER(u, u, h->N * NU)
SETTER(yref, yref, h->N * NY)
SETTER(yref_e, yref_e, NX)
#undef SETTER

int ihm2mpc_set_multipliers(ihm2mpc_handle *h, const double *pi, const double *lam)
{
    CHECK_H(h);
    if (pi) { if (upload(h, pi, h->pi, h->NS * NX)) return -1; }
    else HIP_TRY(hipMemsetAsync(h->pi, 0, (size_t)h->B * h->NS * NX * sizeof(double), h->stream));
    if (lam) { if (upload(h, lam, h->lam, h->NS * NLAM)) return -1; }
    else {
        HIP_TRY(hipMemsetAsync(h->lam, 0, (size_t)h->B * h->NS * NLAM * sizeof(double), h->stream));
        HIP_TRY(hipMemsetAsync(h->lam_a, 0, (size_t)h->B * h->NS * 2 * sizeof(double), h->stream));      // "no multipliers" covers row 14 as well
    }
    return 0;
}

int ihm2mpc_set_slacks(ihm2mpc_handle *h, const double *sl)
{
    CHECK_H(h);
    if (sl) return upload(h, sl, h->slk, h->NS * NLAM);
    HIP_TRY(hipMemsetAsync(h->slk, 0, (size_t)h->B * h->NS * NLAM * sizeof(double), h->stream));
    HIP_TRY(hipMemsetAsync(h->slk_a, 0, (size_t)h->B * h->NS * 2 * sizeof(double), h->stream));
    return 0;
}

int ihm2mpc_set_stage(ihm2mpc_handle *h, int32_t instance, int32_t stage, const char *field, const double *value, int32_t n)
{
    CHECK_H(h);
    FieldInfo fi;
    if (field_info(h, field, &fi)) return -1;
    if (!value) return fail("null argument");
    if (instance < 0 || instance >= h->B) return fail("instance %d out of range", instance);
    const std::string f(field);
    if ((f == "lbx" || f == "ubx") && stage != 0)
        return fail("per-instance '%s' exists at stage 0 only (the initial state); stage bounds are shared: ihm2mpc_set_bounds", field);
    if (f == "yref_e") stage = 0;
    if (stage < 0 || stage >= fi.nstages) return fail("stage %d out of range for field '%s'", stage, field);
    if (n != fi.per_stage) return fail("field '%s' has %d entries per stage, got %d", field, fi.per_stage, n);
    double *dst = fi.base + ((size_t)instance * fi.nstages + stage) * fi.per_stage;
    HIP_TRY(hipMemcpyAsync(dst, value, (size_t)n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_get_stage(ihm2mpc_handle *h, int32_t instance, int32_t stage, const char *field, double *value, int32_t n)
{
    CHECK_H(h);
    FieldInfo fi;
    if (field_info(h, field, &fi)) return -1;
    if (!value) return fail("null argument");
    if (instance < 0 || instance >= h->B) return fail("instance %d out of range", instance);
    if (std::string(field) == "yref_e") stage = 0;
    if (stage < 0 || stage >= fi.nstages) return fail("stage %d out of range for field '%s'", stage, field);
    if (n != fi.per_stage) return fail("field '%s' has %d entries per stage, got %d", field, fi.per_stage, n);
    const double *src = fi.base + ((size_t)instance * fi.nstages + stage) * fi.per_stage;
    HIP_TRY(hipMemcpyAsync(value, src, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_init_guess(ihm2mpc_handle *h, double v_ref_scale)
{
    CHECK_H(h);
    if (ready(h)) return -1;
    ihm2_launch_init_guess(h, v_ref_scale, 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ihm2mpc_reinit_failed(ihm2mpc_handle *h, double v_ref_scale)
{
    CHECK_H(h);
    if (ready(h)) return -1;
    ihm2_launch_init_guess(h, v_ref_scale, 1);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ihm2mpc_prepare_step(ihm2mpc_handle *h, double s_target)
{
    CHECK_H(h);
    if (h->lap_wrap) ihm2_launch_wrap_lap(h);
    ihm2_launch_prepare(h, s_target, 3, h->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int ihm2mpc_linearize(ihm2mpc_handle *h)
{
    CHECK_H(h);
    if (ready(h)) return -1;
    ihm2_launch_linearize(h);
    HIP_TRY(hipGetLastError());
    return 0;
}

// SQP mode: buffers of the line search, allocated on first use (36 KB per instance)
static int sqp_buffers(ihm2mpc_handle *h)
{
    if (h->ls_x) return 0;
    const size_t B = h->B, N = h->N, NS = h->NS;
    return alloc_all(h->ls_x, B * NS * 8, h->ls_u, B * N * 2, h->ls_pi, B * NS * 8, h->ls_lam, B * NS * NLAM, h->ls_slk, B * NS * NLAM,
                     h->ls_wpi, B * NS * 8, h->ls_wlam, B * NS * NLAM, h->ls_alpha, B, h->ls_merit, B * 4, h->ls_args, 64, h->ls_done, B, h->ls_status, B,
                     h->ls_iter, B, h->ls_qp_acc, B, h->ls_pending, B);
}

// SQP mode with the collocation integrator: room for the line search's trial-point rollouts (every step length of the ladder,
// qp_select.hpp: ladder_length)
static int sqp_phi_buffer(ihm2mpc_handle *h, int *n_alpha_out)
{
    const size_t B = h->B, N = h->N;
    const int n_alpha = ihm2::ladder_length(h->sqp_alpha_min, h->sqp_alpha_red);
    if (n_alpha > IHM2MPC_LS_MAX_TRIALS) return fail("backtracking ladder longer than %d trial steps", IHM2MPC_LS_MAX_TRIALS);
    if (h->ls_phi.size() < (size_t)n_alpha * B * N * 8) {
        HIP_TRY(hipStreamSynchronize(h->stream));       // a launch in flight may still read the old one
        HIP_TRY(h->ls_phi.alloc((size_t)n_alpha * B * N * 8));
    }
    if (n_alpha_out) *n_alpha_out = n_alpha;
    return 0;
}

// SQP mode: n_iter iterations of [copy the iterate aside -> linearise -> QP -> convergence test + line search].  join: the first
// QP waits for ev_join (ihm2mpc_step runs the plant and the reference ramp beside the first linearisation).
static int sqp_iterations(ihm2mpc_handle *h, int n_iter, bool join)
{
    if (sqp_buffers(h)) return -1;
    const size_t B = h->B;
    HIP_TRY(hipMemsetAsync(h->ls_done, 0, B * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->ls_iter, 0, B * sizeof(int32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->ls_qp_acc, 0, B * sizeof(int32_t), h->stream));
    for (int it = 0; it < n_iter; it++) {
        // the iterate the QP is built at: the line search walks from it towards the QP's full step
        ihm2_launch_copy_iterate(h);
        ihm2_launch_linearize(h);
        if (it == 0 && join) HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
        if (it == n_iter - 1) HIP_TRY(hipEventRecord(h->ev[1], h->stream));
        if (launch_qp(h)) return fail("problem exceeds the QP kernel limits (LDS or constraint slots)");
        if (const ihm2::QpSituation s = ihm2_situation(h); ihm2::ladder_rollouts(s)) {
            // collocation integrator: the rollouts of the line search's trial points (all step lengths of the ladder) in their own launch,
            // or in two (qp_select.hpp: ladder_first): the rest of the ladder only for the instances the first line-search launch leaves
            // open, which then redo their ladder -- same arithmetic as one launch
            int n_alpha = 1;
            if (sqp_phi_buffer(h, &n_alpha)) return -1;
            const int j_first = ihm2::ladder_first(s, n_alpha);
            ihm2_launch_rollout_irk(h, 0, j_first, h->ls_phi, nullptr);
            if (j_first < n_alpha) {
                ihm2_launch_line_search(h, it, it == n_iter - 1, 1, j_first);
                ihm2_launch_rollout_irk(h, j_first, n_alpha, h->ls_phi, h->ls_pending);
                ihm2_launch_line_search(h, it, it == n_iter - 1, 2, 0);
                continue;
            }
        }
        ihm2_launch_line_search(h, it, it == n_iter - 1);
    }
    return 0;
}

static int sqp_iter_count(ihm2mpc_handle *h) { return h->cfg.nlp_solver_max_iter > 0 ? h->cfg.nlp_solver_max_iter : 1; }

int ihm2mpc_solve(ihm2mpc_handle *h, int32_t n_iter)
{
    CHECK_H(h);
    if (ready(h)) return -1;
    const bool sqp = h->cfg.nlp_solver_type == IHM2MPC_SQP;
    if (n_iter <= 0) n_iter = sqp ? sqp_iter_count(h) : 1;
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    if (sqp) {
        if (sqp_iterations(h, n_iter, false)) return -1;
    } else {
        for (int it = 0; it < n_iter; it++) {
            ihm2_launch_linearize(h);
            if (it == n_iter - 1) {
                if (sens_snapshot(h)) return -1;
                HIP_TRY(hipEventRecord(h->ev[1], h->stream));
            }
            if (launch_qp(h)) return fail("problem exceeds the QP kernel limits (LDS or constraint slots)");
            if (it == n_iter - 1) sens_after_qp(h);
        }
    }
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

int ihm2mpc_set_sqp_options(ihm2mpc_handle *h, int32_t globalization, double alpha_min, double alpha_reduction, double eps_sufficient_descent,
                            int32_t use_sufficient_descent, int32_t full_step_dual, const double *tol)
{
    CHECK_H(h);
    if (globalization != IHM2MPC_FIXED_STEP && globalization != IHM2MPC_MERIT_BACKTRACKING) return fail("unknown globalization %d", globalization);
    if (!(alpha_min > 0.0 && alpha_min <= 1.0)) return fail("alpha_min must be in (0, 1]");
    if (!(alpha_reduction > 0.0 && alpha_reduction < 1.0)) return fail("alpha_reduction must be in (0, 1)");
    if (!(eps_sufficient_descent >= 0.0 && eps_sufficient_descent < 1.0)) return fail("eps_sufficient_descent must be in [0, 1)");
    if (globalization == IHM2MPC_MERIT_BACKTRACKING && ihm2::ladder_length(alpha_min, alpha_reduction) > IHM2MPC_LS_MAX_TRIALS)
        return fail("alpha_reduction %g with alpha_min %g makes a backtracking ladder of more than %d trial steps", alpha_reduction, alpha_min, IHM2MPC_LS_MAX_TRIALS);
    h->sqp_globalization = globalization; h->sqp_alpha_min = alpha_min; h->sqp_alpha_red = alpha_reduction; h->sqp_eps = eps_sufficient_descent;
    h->sqp_use_suff = use_sufficient_descent ? 1 : 0; h->sqp_full_step_dual = full_step_dual ? 1 : 0;
    if (tol)
        for (int i = 0; i < 4; i++) {
            if (!(tol[i] >= 0.0)) return fail("tolerance %d is negative", i);
            h->sqp_tol[i] = tol[i];
        }
    return 0;
}

int ihm2mpc_get_sqp_stats(ihm2mpc_handle *h, int32_t *sqp_iter, double *alpha)
{
    CHECK_H(h);
    if (!h->ls_x) return fail("no SQP-mode solve has run on this handle");
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (sqp_iter) HIP_TRY(hipMemcpy(sqp_iter, h->ls_iter, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (alpha) HIP_TRY(hipMemcpy(alpha, h->ls_alpha, (size_t)h->B * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int ihm2mpc_get_sqp_merit(ihm2mpc_handle *h, double *m)
{
    CHECK_H(h);
    if (!m) return fail("null output");
    if (!h->ls_x) return fail("no SQP-mode solve has run on this handle");
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(m, h->ls_merit, (size_t)h->B * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int ihm2mpc_get_timings(ihm2mpc_handle *h, double *ms, int32_t n)
{
    CHECK_H(h);
    if (!ms || n < 3) return fail("need room for 3 values");
    HIP_TRY(hipEventSynchronize(h->ev[2]));
    float t_total = 0, t_qp = 0;
    HIP_TRY(hipEventElapsedTime(&t_total, h->ev[0], h->ev[2]));
    HIP_TRY(hipEventElapsedTime(&t_qp, h->ev[1], h->ev[2]));
    ms[0] = t_total; ms[2] = t_qp; ms[1] = t_total - t_qp;
    return 0;
}

int ihm2mpc_get_launch_record(ihm2mpc_handle *h, int32_t *rec)
{
    CHECK_H(h);
    if (!rec) return fail("null argument");
    for (int i = 0; i < 16; i++) rec[i] = h->launch_rec[i];
    return 0;
}

int ihm2mpc_get_linearization(ihm2mpc_handle *h, double *A, double *Bm, double *b)
{
    CHECK_H(h);
    const size_t n = (size_t)h->B * h->N;
    std::vector<double> rec(n * LIN_REC);
    HIP_TRY(hipMemcpyAsync(rec.data(), h->lin, rec.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (size_t r = 0; r < n; r++) {
        if (A) memcpy(A + r * 64, rec.data() + r * LIN_REC, 64 * sizeof(double));
        if (Bm) memcpy(Bm + r * 16, rec.data() + r * LIN_REC + 64, 16 * sizeof(double));
        if (b) memcpy(b + r * 8, rec.data() + r * LIN_REC + 80, 8 * sizeof(double));
    }
    return 0;
}

#define GETTER(name, field, elems)                             \
    int ihm2mpc_get_##name(ihm2mpc_handle *h, double *v)       \
    {                                                          \
        CHECK_H(h);                                            \
        if (!v) return fail("null argument");                  \
        return download(h, h->field, v, (elems));              \
    }
GETTER(x, x, h->NS * NX)
GETTER(u, u, h->N * NU)
GETTER(u0, u0, NU)
GETTER(residuals, res, 4)
GETTER(qp_residuals, qp_res, 4)
GETTER(x0, x0, NX)
GETTER(slacks, slk, h->NS * NLAM)
#undef GETTER

int ihm2mpc_get_multipliers(ihm2mpc_handle *h, double *pi, double *lam)
{
    CHECK_H(h);
    if (pi && download(h, h->pi, pi, h->NS * NX)) return -1;
    if (lam && download(h, h->lam, lam, h->NS * NLAM)) return -1;
    return 0;
}

int ihm2mpc_get_status(ihm2mpc_handle *h, int32_t *status)
{
    CHECK_H(h);
    if (!status) return fail("null argument");
    HIP_TRY(hipMemcpyAsync(status, h->status, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_get_qp_iter(ihm2mpc_handle *h, int32_t *qp_iter)
{
    CHECK_H(h);
    if (!qp_iter) return fail("null argument");
    HIP_TRY(hipMemcpyAsync(qp_iter, h->qp_iter, (size_t)h->B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_set_x0_sensitivities(ihm2mpc_handle *h, int32_t mode)
{
    CHECK_H(h);
    if (mode < 0 || mode > 2) return fail("x0 sensitivity mode %d: 0 (off), 1 (du_0/dx_0) or 2 (the whole horizon)", mode);
    if (mode != 0 && h->cfg.nlp_solver_type == IHM2MPC_SQP)
        return fail("x0 sensitivities are implemented for SQP_RTI: in the SQP mode the line search scales the step and the multipliers, "
                    "which leaves no QP solution to differentiate");
    const size_t B = h->B, N = h->N, NS = h->NS;
    if (mode >= 1 && !h->sens_u0 && alloc_all(h->sens_xbar, B * NS * NX, h->sens_ubar, B * N * NU, h->sens_u0, B * NU * NX, h->sens_args, 64))
        return -1;
    if (mode == 2 && !h->sens_x && alloc_all(h->sens_x, B * NS * NX * NX, h->sens_u, B * N * NU * NX)) return -1;
    if (mode != h->sens_mode) h->sens_state = 0;
    h->sens_mode = mode;
    return 0;
}

int ihm2mpc_get_x0_sensitivities(ihm2mpc_handle *h, double *sens_x, double *sens_u)
{
    CHECK_H(h);
    if (sens_readable(h)) return -1;
    if (sens_x && h->sens_mode != 2) return fail("sens_x needs x0 sensitivity mode 2 (mode 1 computes du_0/dx_0 only)");
    if (sens_x && download(h, h->sens_x, sens_x, h->NS * NX * NX)) return -1;
    if (sens_u && download(h, h->sens_mode == 2 ? h->sens_u : h->sens_u0, sens_u, h->sens_mode == 2 ? h->N * NU * NX : NU * NX)) return -1;
    return 0;
}

// the adjoint entries' refusal in the SQP mode
static int adjoint_refused_in_sqp(const ihm2mpc_handle *h)
{
    if (h->cfg.nlp_solver_type == IHM2MPC_SQP)
        return fail("adjoint sensitivities are implemented for SQP_RTI: in the SQP mode the line search scales the step and the multipliers, "
                    "which leaves no QP solution to differentiate");
    return 0;
}

// the handle's seed and gradient buffers of the adjoint entries for S seeds (weights: and the two gradients in the weights), grown on demand
static int adjoint_buffers(ihm2mpc_handle *h, size_t S, bool weights)
{
    const size_t B = h->B, N = h->N, NS = h->NS;
    if (h->adj_gx0.size() < B * S * NX &&
        alloc_all(h->adj_sx, B * S * NS * NX, h->adj_su, B * S * N * NU, h->adj_gx0, B * S * NX, h->adj_gy, B * S * N * NY, h->adj_gye, B * S * NX))
        return -1;
    if (weights && h->adj_gW.size() < B * S * NY * NY && alloc_all(h->adj_gW, B * S * NY * NY, h->adj_gWe, B * S * NX * NX)) return -1;
    return 0;
}

// the refusals every adjoint entry shares, host or device seeds (unit_u0: no seed was given)
static int adjoint_refused(const ihm2mpc_handle *h, int32_t n_seeds, bool unit_u0)
{
    if (adjoint_refused_in_sqp(h)) return -1;
    if (n_seeds < 1 || n_seeds > 8) return fail("adjoint sensitivities: n_seeds = %d, one call takes 1 to 8 seeds", n_seeds);
    if (unit_u0 && n_seeds != 2)
        return fail("adjoint sensitivities: seed_x and seed_u both NULL stands for the two unit seeds on u_0 and needs n_seeds = 2, not %d", n_seeds);
    // the factorisation is that of the x0 sensitivities: their snapshot of (xbar, ubar) must belong to the last solve
    return sens_readable(h);
}

static bool any_soft_side(const ihm2mpc_handle *h);

// The host outputs of the penalty entries (ihm2mpc_eval_adjoint_sensitivities_p, ihm2mpc_eval_cost_gradient_penalties), any may be NULL,
// and their call-local device memory "penalty_grad_work" for S seeds: zeta (B,S,NS,10), then grad_z, grad_Z (B,S,NS,28), grad_za,
// grad_Za (B,S,NS,2)
struct PenaltyOut { double *z, *Z, *za, *Za, *zeta; };
struct PenaltyWork {
    WorkBuf<double> buf;
    double *zeta, *z, *Z, *za, *Za;
    int alloc(ihm2mpc_handle *h, size_t S)
    {
        const size_t n = (size_t)h->B * S * h->NS;
        buf.poison(poisoned(h, "penalty_grad_work"));
        if (buf.alloc(n * (NZ + 2 * NLAM + 4)) != hipSuccess) return fail("out of device memory");
        zeta = buf; z = zeta + n * NZ; Z = z + n * NLAM; za = Z + n * NLAM; Za = za + n * 2;
        return 0;
    }
};

// the copies of the penalty outputs onto h->stream, behind the kernels (soft: k_penalty_grad ran and wrote the four gradients)
static int penalty_download(ihm2mpc_handle *h, size_t S, const PenaltyWork &w, const PenaltyOut &o, bool soft)
{
    const size_t n = (size_t)h->B * S * h->NS;
    if (o.zeta) HIP_TRY(hipMemcpyAsync(o.zeta, w.zeta, n * NZ * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (!soft) return 0;
    if (o.z) HIP_TRY(hipMemcpyAsync(o.z, w.z, n * NLAM * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (o.Z) HIP_TRY(hipMemcpyAsync(o.Z, w.Z, n * NLAM * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (o.za) HIP_TRY(hipMemcpyAsync(o.za, w.za, n * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (o.Za) HIP_TRY(hipMemcpyAsync(o.Za, w.Za, n * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

// a handle without a soft side: no kernel ran, the four gradients are zeros, NaN for instances whose status is neither 0 nor 2 (blocking)
static int penalty_zeros(ihm2mpc_handle *h, size_t S, const PenaltyOut &o)
{
    if (!o.z && !o.Z && !o.za && !o.Za) return 0;
    std::vector<int32_t> st(h->B);
    HIP_TRY(hipMemcpyAsync(st.data(), h->status, st.size() * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t n = S * h->NS;
    for (int b = 0; b < h->B; b++) {
        const double v = (st[b] == 0 || st[b] == 2) ? 0.0 : NAN;
        if (o.z) std::fill_n(o.z + b * n * NLAM, n * NLAM, v);
        if (o.Z) std::fill_n(o.Z + b * n * NLAM, n * NLAM, v);
        if (o.za) std::fill_n(o.za + b * n * 2, n * 2, v);
        if (o.Za) std::fill_n(o.Za + b * n * 2, n * 2, v);
    }
    return 0;
}

// ihm2mpc_eval_adjoint_sensitivities, ihm2mpc_eval_adjoint_sensitivities_w (weights: grad_W / grad_W_e are computed and may be asked for),
// ihm2mpc_eval_adjoint_sensitivities_s (seed_s / seed_sa: seeds on the soft slacks, folded onto the stage seeds by k_slack_fold first) and
// ihm2mpc_eval_adjoint_sensitivities_p (pen: k_adj<true, true> keeps zeta and, on a table with a soft side, k_penalty_grad runs behind it)
static int eval_adjoint(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u, const double *seed_s, const double *seed_sa,
                        double *grad_x0, double *grad_yref, double *grad_yref_e, bool weights, double *grad_W, double *grad_W_e,
                        const PenaltyOut *pen = nullptr)
{
    CHECK_H(h);
    const bool slack = seed_s || seed_sa;
    const bool unit_u0 = !seed_x && !seed_u && !slack;
    if (adjoint_refused(h, n_seeds, unit_u0)) return -1;
    const size_t B = h->B, N = h->N, NS = h->NS, S = n_seeds;
    if (adjoint_buffers(h, S, weights)) return -1;
    if (seed_x) HIP_TRY(hipMemcpyAsync(h->adj_sx, seed_x, B * S * NS * NX * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (seed_u) HIP_TRY(hipMemcpyAsync(h->adj_su, seed_u, B * S * N * NU * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PenaltyWork pw;
    if (pen && pw.alloc(h, S)) return -1;
    double *zeta = pen ? pw.zeta : nullptr;
    const bool soft = pen && any_soft_side(h);
    const double *pen_s = nullptr, *pen_sa = nullptr;   // the slack seeds in device memory, as the fold took them
    WorkBuf<double> slack_seed_work;    // "slack_seed_work": seed_s (B,S,NS,28), then seed_sa (B,S,NS,2); the part of a NULL seed is not read
    if (slack) {
        slack_seed_work.poison(poisoned(h, "slack_seed_work"));
        if (slack_seed_work.alloc(B * S * NS * (NLAM + 2)) != hipSuccess) return fail("out of device memory");
        double *ds = slack_seed_work, *dsa = ds + B * S * NS * NLAM;
        if (seed_s) HIP_TRY(hipMemcpyAsync(ds, seed_s, B * S * NS * NLAM * sizeof(double), hipMemcpyHostToDevice, h->stream));
        if (seed_sa) HIP_TRY(hipMemcpyAsync(dsa, seed_sa, B * S * NS * 2 * sizeof(double), hipMemcpyHostToDevice, h->stream));
        // the fold adds to the stage seeds: a NULL one is zero first
        if (!seed_x) HIP_TRY(hipMemsetAsync(h->adj_sx, 0, B * S * NS * NX * sizeof(double), h->stream));
        if (!seed_u) HIP_TRY(hipMemsetAsync(h->adj_su, 0, B * S * N * NU * sizeof(double), h->stream));
        pen_s = seed_s ? ds : nullptr; pen_sa = seed_sa ? dsa : nullptr;
        ihm2_launch_slack_fold(h, 0, n_seeds, pen_s, pen_sa, h->adj_sx, h->adj_su);
        ihm2_launch_adj(h, n_seeds, h->adj_sx, h->adj_su, 0, weights ? 1 : 0, zeta);
    } else {
        ihm2_launch_adj(h, n_seeds, seed_x ? h->adj_sx.get() : nullptr, seed_u ? h->adj_su.get() : nullptr, unit_u0 ? 1 : 0, weights ? 1 : 0, zeta);
    }
    if (soft) ihm2_launch_penalty_grad(h, 0, n_seeds, pen_s, pen_sa, pw.zeta, pw.z, pw.Z, pw.za, pw.Za);
    HIP_TRY(hipGetLastError());
    if (grad_x0) HIP_TRY(hipMemcpyAsync(grad_x0, h->adj_gx0, B * S * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_yref) HIP_TRY(hipMemcpyAsync(grad_yref, h->adj_gy, B * S * N * NY * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_yref_e) HIP_TRY(hipMemcpyAsync(grad_yref_e, h->adj_gye, B * S * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_W) HIP_TRY(hipMemcpyAsync(grad_W, h->adj_gW, B * S * NY * NY * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_W_e) HIP_TRY(hipMemcpyAsync(grad_W_e, h->adj_gWe, B * S * NX * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (pen && penalty_download(h, S, pw, *pen, soft)) return -1;
    HIP_TRY(hipStreamSynchronize(h->stream));      // the seeds may be reused and the gradients read as soon as we return; the call's work buffers are released behind it
    if (pen && !soft) return penalty_zeros(h, S, *pen);
    return 0;
}

int ihm2mpc_eval_adjoint_sensitivities(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u, double *grad_x0,
                                       double *grad_yref, double *grad_yref_e)
{
    return eval_adjoint(h, n_seeds, seed_x, seed_u, nullptr, nullptr, grad_x0, grad_yref, grad_yref_e, false, nullptr, nullptr);
}

int ihm2mpc_eval_adjoint_sensitivities_w(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u, double *grad_x0,
                                         double *grad_yref, double *grad_yref_e, double *grad_W, double *grad_W_e)
{
    return eval_adjoint(h, n_seeds, seed_x, seed_u, nullptr, nullptr, grad_x0, grad_yref, grad_yref_e, true, grad_W, grad_W_e);
}

// Seeds and gradients in device memory: k_adj<true> reads the caller's seeds, the gradients leave the handle's buffers by device-to-device
// copies behind it on h->stream.  No host copy, no wait (the buffers' first allocation and their growth aside).
int ihm2mpc_eval_adjoint_sensitivities_w_device(ihm2mpc_handle *h, int32_t n_seeds, const void *seed_x, const void *seed_u, void *grad_x0,
                                                void *grad_yref, void *grad_yref_e, void *grad_W, void *grad_W_e)
{
    CHECK_H(h);
    const bool unit_u0 = !seed_x && !seed_u;
    if (adjoint_refused(h, n_seeds, unit_u0)) return -1;
    const size_t B = h->B, N = h->N, S = n_seeds;
    if (adjoint_buffers(h, S, true)) return -1;
    ihm2_launch_adj(h, n_seeds, (const double *)seed_x, (const double *)seed_u, unit_u0 ? 1 : 0, 1, nullptr);
    HIP_TRY(hipGetLastError());
    if (grad_x0) HIP_TRY(hipMemcpyAsync(grad_x0, h->adj_gx0, B * S * NX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (grad_yref) HIP_TRY(hipMemcpyAsync(grad_yref, h->adj_gy, B * S * N * NY * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (grad_yref_e) HIP_TRY(hipMemcpyAsync(grad_yref_e, h->adj_gye, B * S * NX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (grad_W) HIP_TRY(hipMemcpyAsync(grad_W, h->adj_gW, B * S * NY * NY * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (grad_W_e) HIP_TRY(hipMemcpyAsync(grad_W_e, h->adj_gWe, B * S * NX * NX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

int ihm2mpc_eval_adjoint_sensitivities_s(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u, const double *seed_s,
                                         const double *seed_sa, double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W,
                                         double *grad_W_e)
{
    return eval_adjoint(h, n_seeds, seed_x, seed_u, seed_s, seed_sa, grad_x0, grad_yref, grad_yref_e, true, grad_W, grad_W_e);
}

int ihm2mpc_eval_adjoint_sensitivities_p(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u, const double *seed_s,
                                         const double *seed_sa, double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W,
                                         double *grad_W_e, double *grad_z, double *grad_Z, double *grad_za, double *grad_Za, double *zeta)
{
    const PenaltyOut pen = {grad_z, grad_Z, grad_za, grad_Za, zeta};
    return eval_adjoint(h, n_seeds, seed_x, seed_u, seed_s, seed_sa, grad_x0, grad_yref, grad_yref_e, true, grad_W, grad_W_e, &pen);
}

// Seeds and gradients in device memory: the launches of eval_adjoint(pen) on the caller's pointers.  The fold works in place, so with a
// slack seed the stage seeds are first copied (device to device) into the handle's seed buffers, as the host entry uploads them there;
// k_slack_fold and k_penalty_grad read seed_s, seed_sa, and without a slack seed k_adj reads seed_x, seed_u, straight from the caller's
// memory.  k_adj and k_penalty_grad write zeta and the four penalty gradients straight into the caller's memory, which they fill entry
// for entry; an output that is not asked for lands in the handle's workspace (h->pd).  No host copy, no wait (the buffers' growth aside).
int ihm2mpc_eval_adjoint_sensitivities_p_device(ihm2mpc_handle *h, int32_t n_seeds, const void *seed_x, const void *seed_u, const void *seed_s,
                                                const void *seed_sa, void *grad_x0, void *grad_yref, void *grad_yref_e, void *grad_W,
                                                void *grad_W_e, void *grad_z, void *grad_Z, void *grad_za, void *grad_Za, void *zeta)
{
    CHECK_H(h);
    const bool slack = seed_s || seed_sa;
    const bool unit_u0 = !seed_x && !seed_u && !slack;
    if (adjoint_refused(h, n_seeds, unit_u0)) return -1;
    const size_t B = h->B, N = h->N, NS = h->NS, S = n_seeds, D = sizeof(double);
    if (adjoint_buffers(h, S, true)) return -1;
    const size_t n = B * S * NS;
    // (growth releases the old block, into which launches of an earlier call may still be queued: wait for them first)
    if (h->pd.buf.size() < n * (NZ + 2 * NLAM + 4)) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->pd.buf.poison(poisoned(h, "penalty_grad_work"));
        if (h->pd.buf.alloc(n * (NZ + 2 * NLAM + 4)) != hipSuccess) return fail("out of device memory");
    }
    double *w = h->pd.buf;
    double *dzeta = zeta ? (double *)zeta : w, *gz = grad_z ? (double *)grad_z : w + n * NZ, *gZ = grad_Z ? (double *)grad_Z : w + n * (NZ + NLAM);
    double *gza = grad_za ? (double *)grad_za : w + n * (NZ + 2 * NLAM), *gZa = grad_Za ? (double *)grad_Za : w + n * (NZ + 2 * NLAM + 2);
    const double *ds = (const double *)seed_s, *dsa = (const double *)seed_sa;
    if (slack) {
        if (seed_x) HIP_TRY(hipMemcpyAsync(h->adj_sx, seed_x, B * S * NS * NX * D, hipMemcpyDeviceToDevice, h->stream));
        else HIP_TRY(hipMemsetAsync(h->adj_sx, 0, B * S * NS * NX * D, h->stream));
        if (seed_u) HIP_TRY(hipMemcpyAsync(h->adj_su, seed_u, B * S * N * NU * D, hipMemcpyDeviceToDevice, h->stream));
        else HIP_TRY(hipMemsetAsync(h->adj_su, 0, B * S * N * NU * D, h->stream));
        ihm2_launch_slack_fold(h, 0, n_seeds, ds, dsa, h->adj_sx, h->adj_su);
        ihm2_launch_adj(h, n_seeds, h->adj_sx, h->adj_su, 0, 1, dzeta);
    } else {
        ihm2_launch_adj(h, n_seeds, (const double *)seed_x, (const double *)seed_u, unit_u0 ? 1 : 0, 1, dzeta);
    }
    if (any_soft_side(h)) ihm2_launch_penalty_grad(h, 0, n_seeds, ds, dsa, dzeta, gz, gZ, gza, gZa);
    else if (grad_z || grad_Z || grad_za || grad_Za)
        ihm2_launch_penalty_fill(h, n_seeds, (double *)grad_z, (double *)grad_Z, (double *)grad_za, (double *)grad_Za);
    HIP_TRY(hipGetLastError());
    if (grad_x0) HIP_TRY(hipMemcpyAsync(grad_x0, h->adj_gx0, B * S * NX * D, hipMemcpyDeviceToDevice, h->stream));
    if (grad_yref) HIP_TRY(hipMemcpyAsync(grad_yref, h->adj_gy, B * S * N * NY * D, hipMemcpyDeviceToDevice, h->stream));
    if (grad_yref_e) HIP_TRY(hipMemcpyAsync(grad_yref_e, h->adj_gye, B * S * NX * D, hipMemcpyDeviceToDevice, h->stream));
    if (grad_W) HIP_TRY(hipMemcpyAsync(grad_W, h->adj_gW, B * S * NY * NY * D, hipMemcpyDeviceToDevice, h->stream));
    if (grad_W_e) HIP_TRY(hipMemcpyAsync(grad_W_e, h->adj_gWe, B * S * NX * NX * D, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// the slack values after the last QP, device to device: slk (B,N+1,28) as ihm2mpc_get_slacks, slk_alat (B,N+1,2) as the slk of
// ihm2mpc_get_alat_multipliers; either may be NULL
int ihm2mpc_get_slacks_device(ihm2mpc_handle *h, void *slk, void *slk_alat)
{
    CHECK_H(h);
    if (!slk && !slk_alat) return fail("null argument");
    if (slk) HIP_TRY(hipMemcpyAsync(slk, h->slk, (size_t)h->B * h->NS * NLAM * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (slk_alat) HIP_TRY(hipMemcpyAsync(slk_alat, h->slk_a, (size_t)h->B * h->NS * 2 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// ---- the objective and its total gradient (kernels_cost.hip) ----
// a finite side of the constraint rows carries a slack (the lateral-acceleration row: stages 1 .. N-1)
static bool any_soft_side(const ihm2mpc_handle *h)
{
    const ihm2::ConstraintRows &r = h->rows;
    for (int k = 0; k < r.NS; k++)
        for (int c = 0; c < NC; c++)
            if ((std::isfinite(r.lb[k * NC + c]) && r.sZ[k * NLAM + c] >= 0.0) || (std::isfinite(r.ub[k * NC + c]) && r.sZ[k * NLAM + NC + c] >= 0.0))
                return true;
    return r.alat_on && r.NS > 2 &&
           ((std::isfinite(r.alat_lb) && r.alat_sZ[0] >= 0.0) || (std::isfinite(r.alat_ub) && r.alat_sZ[1] >= 0.0));
}

int ihm2mpc_eval_cost(ihm2mpc_handle *h, double *cost, double *stage_cost, double *slack_cost)
{
    CHECK_H(h);
    if (ready(h)) return -1;
    const size_t B = h->B, NS = h->NS;
    WorkBuf<double> dwork;           // "cost_work": cost (B), slack_cost (B), stage_cost (B,NS)
    dwork.poison(poisoned(h, "cost_work"));
    if (dwork.alloc(B * (2 + NS)) != hipSuccess) return fail("out of device memory");
    double *dc = dwork, *dsl = dwork + B, *dst = dwork + 2 * B;
    ihm2_launch_cost(h, 0, dc, stage_cost ? dst : nullptr, dsl, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    if (cost) HIP_TRY(hipMemcpyAsync(cost, dc, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (stage_cost) HIP_TRY(hipMemcpyAsync(stage_cost, dst, B * NS * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (slack_cost) HIP_TRY(hipMemcpyAsync(slack_cost, dsl, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

// ihm2mpc_eval_cost_gradient and ihm2mpc_eval_cost_gradient_soft (soft: every table is taken, and on one with a soft side k_slack_fold<true>
// carries dJ_slack/ds onto the seeds between the cost kernel and the adjoint) and ihm2mpc_eval_cost_gradient_penalties (pen: k_adj<true, true>
// keeps zeta and, on a table with a soft side, k_penalty_grad<true> runs behind it)
static int eval_cost_gradient(ihm2mpc_handle *h, bool soft, double *cost, double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W,
                              double *grad_W_e, double *seed_x, double *seed_u, const PenaltyOut *pen = nullptr)
{
    CHECK_H(h);
    if (adjoint_refused_in_sqp(h)) return -1;
    if (sens_readable(h)) return -1;
    const bool fold = any_soft_side(h);
    if (fold && !soft)
        return fail("the cost gradient is defined for all-hard constraint tables: with a soft side the objective depends on slacks that the "
                    "adjoint system has eliminated and that carry no seed (ihm2mpc_eval_cost evaluates the cost of any table)");
    const size_t B = h->B, N = h->N, NS = h->NS;
    if (adjoint_buffers(h, 1, true)) return -1;
    // "cost_work": cost (B), then the explicit partials, which the epilogue turns into the totals: yref (B,N,12), yref_e (B,8), W (B,12,12), W_e (B,8,8)
    WorkBuf<double> dwork;
    dwork.poison(poisoned(h, "cost_work"));
    if (dwork.alloc(B * (1 + N * NY + NX + NY * NY + NX * NX)) != hipSuccess) return fail("out of device memory");
    double *dc = dwork, *dgy = dc + B, *dgye = dgy + B * N * NY, *dgW = dgye + B * NX, *dgWe = dgW + B * NY * NY;
    // the seeds dJ/dz straight into the adjoint entries' seed buffers, k_adj<true> on them, the explicit partials added: no host round trip
    ihm2_launch_cost(h, 1, dc, nullptr, nullptr, h->adj_sx, h->adj_su, dgy, dgye, dgW, dgWe);
    PenaltyWork pw;
    if (pen && pw.alloc(h, 1)) return -1;
    if (fold) ihm2_launch_slack_fold(h, 1, 1, nullptr, nullptr, h->adj_sx, h->adj_su);
    ihm2_launch_adj(h, 1, h->adj_sx, h->adj_su, 0, 1, pen ? pw.zeta : nullptr);
    if (pen && fold) ihm2_launch_penalty_grad(h, 1, 1, nullptr, nullptr, pw.zeta, pw.z, pw.Z, pw.za, pw.Za);
    ihm2_launch_cost_epilogue(h, dgy, dgye, dgW, dgWe);
    HIP_TRY(hipGetLastError());
    if (cost) HIP_TRY(hipMemcpyAsync(cost, dc, B * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_x0) HIP_TRY(hipMemcpyAsync(grad_x0, h->adj_gx0, B * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_yref) HIP_TRY(hipMemcpyAsync(grad_yref, dgy, B * N * NY * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_yref_e) HIP_TRY(hipMemcpyAsync(grad_yref_e, dgye, B * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_W) HIP_TRY(hipMemcpyAsync(grad_W, dgW, B * NY * NY * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (grad_W_e) HIP_TRY(hipMemcpyAsync(grad_W_e, dgWe, B * NX * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (seed_x) HIP_TRY(hipMemcpyAsync(seed_x, h->adj_sx, B * NS * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (seed_u) HIP_TRY(hipMemcpyAsync(seed_u, h->adj_su, B * N * NU * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (pen && penalty_download(h, 1, pw, *pen, fold)) return -1;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (pen && !fold) return penalty_zeros(h, 1, *pen);
    return 0;
}

int ihm2mpc_eval_cost_gradient(ihm2mpc_handle *h, double *cost, double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W,
                               double *grad_W_e, double *seed_x, double *seed_u)
{
    return eval_cost_gradient(h, false, cost, grad_x0, grad_yref, grad_yref_e, grad_W, grad_W_e, seed_x, seed_u);
}

int ihm2mpc_eval_cost_gradient_soft(ihm2mpc_handle *h, double *cost, double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W,
                                    double *grad_W_e, double *seed_x, double *seed_u)
{
    return eval_cost_gradient(h, true, cost, grad_x0, grad_yref, grad_yref_e, grad_W, grad_W_e, seed_x, seed_u);
}

int ihm2mpc_eval_cost_gradient_penalties(ihm2mpc_handle *h, double *cost, double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W,
                                         double *grad_W_e, double *grad_z, double *grad_Z, double *grad_za, double *grad_Za, double *seed_x,
                                         double *seed_u)
{
    const PenaltyOut pen = {grad_z, grad_Z, grad_za, grad_Za, nullptr};
    return eval_cost_gradient(h, true, cost, grad_x0, grad_yref, grad_yref_e, grad_W, grad_W_e, seed_x, seed_u, &pen);
}

int ihm2mpc_get_sens_u0_device(ihm2mpc_handle *h, void *dptr)
{
    CHECK_H(h);
    if (!dptr) return fail("null argument");
    if (sens_readable(h)) return -1;
    HIP_TRY(hipMemcpyAsync(dptr, h->sens_u0, (size_t)h->B * NU * NX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

// ---- device-pointer variants: instance-major device buffers, no host round trip ----
#define DEVCOPY(name, dst, src, bytes)                                                                  \
    int ihm2mpc_##name(ihm2mpc_handle *h, DEVCOPY_ARG dptr)                                             \
    {                                                                                                   \
        CHECK_H(h);                                                                                     \
        if (!dptr) return fail("null argument");                                                        \
        HIP_TRY(hipMemcpyAsync((void *)(dst), (const void *)(src), (bytes), hipMemcpyDeviceToDevice, h->stream)); \
        return 0;                                                                                       \
    }
#define DEVCOPY_ARG const void *
DEVCOPY(set_x0_device, h->x0, dptr, (size_t)h->B * NX * sizeof(double))
DEVCOPY(set_yref_device, h->yref, dptr, (size_t)h->B * h->N * NY * sizeof(double))
DEVCOPY(set_yref_e_device, h->yref_e, dptr, (size_t)h->B * NX * sizeof(double))
#undef DEVCOPY_ARG
#define DEVCOPY_ARG void *
DEVCOPY(get_u0_device, dptr, h->u0, (size_t)h->B * NU * sizeof(double))
DEVCOPY(get_x_device, dptr, h->x, (size_t)h->B * h->NS * NX * sizeof(double))
DEVCOPY(get_u_device, dptr, h->u, (size_t)h->B * h->N * NU * sizeof(double))
DEVCOPY(get_status_device, dptr, h->status, (size_t)h->B * sizeof(int32_t))
#undef DEVCOPY_ARG
#undef DEVCOPY

// ---- plant ----
int ihm2mpc_sim_step(ihm2mpc_handle *h, int32_t model, int32_t M_sim, const double *x, const double *u, double *x_next)
{
    CHECK_H(h);
    if (!h->tracks_set) return fail("ihm2mpc_set_tracks has not been called");
    if (!x || !u || !x_next) return fail("null argument");
    if (check_plant(h, model, M_sim)) return -1;
    double *xs = h->scratch, *us = h->scratch + (size_t)h->B * 8, *xn = h->scratch + (size_t)h->B * 16;
    if (upload(h, x, xs, NX) || upload(h, u, us, NU)) return -1;
    ihm2_launch_sim(h, model, M_sim, xs, us, xn, h->stream, nullptr);
    HIP_TRY(hipGetLastError());
    return download(h, xn, x_next, NX);
}

int ihm2mpc_sim_advance(ihm2mpc_handle *h, int32_t model, int32_t M_sim)
{
    CHECK_H(h);
    if (!h->tracks_set) return fail("ihm2mpc_set_tracks has not been called");
    if (check_plant(h, model, M_sim)) return -1;
    ihm2_launch_sim(h, model, M_sim, h->x0, h->u0, h->x0, h->stream, h->active_set ? h->active.get() : nullptr);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- plant step with forward sensitivities (kernels_simsens.hip) ----
static int check_plant_sens(const ihm2mpc_handle *h, int model, int M_sim, const void *x, const void *u)
{
    if (!h->tracks_set) return fail("ihm2mpc_set_tracks has not been called");
    if (!x || !u) return fail("null argument");
    return check_plant(h, model, M_sim);
}

int ihm2mpc_sim_step_sens_device(ihm2mpc_handle *h, int32_t model, int32_t M_sim, const void *x, const void *u, void *x_next, void *S_x,
                                 void *S_u, void *model_used)
{
    CHECK_H(h);
    if (check_plant_sens(h, model, M_sim, x, u)) return -1;
    // the kernels of a switched plant run under the mask: without the caller's array a local one, released (which waits for the device)
    // when the call returns
    StateBuf<int32_t> mask;
    if (!model_used && model < 0) {
        HIP_TRY(mask.alloc(h->B));
        model_used = mask.get();
    }
    if (ihm2_launch_sim_sens(h, model, M_sim, (const double *)x, (const double *)u, (double *)x_next, (double *)S_x, (double *)S_u,
                             (int32_t *)model_used, h->stream))
        return fail("upload of the plant's collocation tableau failed");
    HIP_TRY(hipGetLastError());
    if (mask) HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_sim_step_sens(ihm2mpc_handle *h, int32_t model, int32_t M_sim, const double *x, const double *u, double *x_next, double *S_x,
                          double *S_u, int32_t *model_used)
{
    CHECK_H(h);
    if (check_plant_sens(h, model, M_sim, x, u)) return -1;
    const size_t B = h->B;
    StateBuf<double> din;            // the uploaded pairs: x (B,8), u (B,2)
    WorkBuf<double> dwork;           // "sim_sens_work": x_next (B,8), S_x (B,8,8), S_u (B,8,2)
    WorkBuf<int32_t> dmodel;         // model_used (B)
    dwork.poison(poisoned(h, "sim_sens_work"));
    HIP_TRY(din.alloc(B * (NX + NU)));
    if (dwork.alloc(B * (NX + NX * NX + NX * NU)) != hipSuccess || dmodel.alloc(B) != hipSuccess) return fail("out of device memory");
    double *dx = din, *du = din + B * NX, *dxn = dwork, *dSx = dwork + B * NX, *dSu = dwork + B * (NX + NX * NX);
    HIP_TRY(hipMemcpyAsync(dx, x, B * NX * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(du, u, B * NU * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (ihm2_launch_sim_sens(h, model, M_sim, dx, du, dxn, dSx, dSu, dmodel, h->stream)) return fail("upload of the plant's collocation tableau failed");
    HIP_TRY(hipGetLastError());
    if (x_next) HIP_TRY(hipMemcpyAsync(x_next, dxn, B * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (S_x) HIP_TRY(hipMemcpyAsync(S_x, dSx, B * NX * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (S_u) HIP_TRY(hipMemcpyAsync(S_u, dSu, B * NX * NU * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (model_used) HIP_TRY(hipMemcpyAsync(model_used, dmodel, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_host_alloc(uint64_t nbytes, void **p)
{
    if (!p || nbytes == 0) return fail("null argument");
    HIP_TRY(hipHostMalloc(p, nbytes, hipHostMallocDefault));
    return 0;
}

int ihm2mpc_host_free(void *p)
{
    if (p) HIP_TRY(hipHostFree(p));
    return 0;
}

// IHM2Controller.compute_control (python/main.py:297-334) in one call: x0 in, reference ramp + warm-start shift, one solve
// (RTI or the configured SQP iterations), u0 and status out -- one host-device round trip, one wait.
int ihm2mpc_compute_control(ihm2mpc_handle *h, const double *x0, double s_target, double *u0, int32_t *status)
{
    CHECK_H(h);
    if (!x0 || !u0) return fail("null argument");
    if (ready(h)) return -1;
    const size_t B = h->B;
    HIP_TRY(hipMemcpyAsync(h->x0, x0, B * NX * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (h->lap_wrap) ihm2_launch_wrap_lap(h);
    ihm2_launch_prepare(h, s_target, 3, h->stream);
    if (ihm2mpc_solve(h, 0)) return -1;
    HIP_TRY(hipMemcpyAsync(u0, h->u0, B * NU * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (status) HIP_TRY(hipMemcpyAsync(status, h->status, B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

int ihm2mpc_get_u0_async(ihm2mpc_handle *h, double *pinned_dst)
{
    CHECK_H(h);
    if (!pinned_dst) return fail("null argument");
    HIP_TRY(hipMemcpyAsync(pinned_dst, h->u0, (size_t)h->B * NU * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

int ihm2mpc_set_lap_wrap(ihm2mpc_handle *h, int32_t enable)
{
    CHECK_H(h);
    h->lap_wrap = enable != 0;
    return 0;
}

int ihm2mpc_set_active(ihm2mpc_handle *h, const int32_t *active)
{
    CHECK_H(h);
    h->active_set = active != nullptr;
    h->freeze_armed = false;      // set_active(NULL) also forgets the mask a frozen loop left behind
    if (active) {
        HIP_TRY(hipMemcpyAsync(h->active, active, (size_t)h->B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return 0;
}

int ihm2mpc_step(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double s_target)
{
    CHECK_H(h);
    if (ready(h)) return -1;
    if (check_plant(h, model, M_sim)) return -1;
    // The plant step and the reference ramp only feed the QP (through x0 and yref); the warm-start shift and the
    // linearisation only need the previous iterate.  Two branches, joined in front of the QP kernel.
    if (h->lap_wrap) ihm2_launch_wrap_lap(h);
    HIP_TRY(hipEventRecord(h->ev[0], h->stream));
    HIP_TRY(hipEventRecord(h->ev_fork, h->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream2, h->ev_fork, 0));
    ihm2_launch_sim(h, model, M_sim, h->x0, h->u0, h->x0, h->stream2, h->active_set ? h->active.get() : nullptr);
    ihm2_launch_prepare(h, s_target, 1, h->stream2);
    HIP_TRY(hipEventRecord(h->ev_join, h->stream2));
    ihm2_launch_prepare(h, s_target, 2, h->stream);
    if (h->cfg.nlp_solver_type == IHM2MPC_SQP) {
        if (sqp_iterations(h, sqp_iter_count(h), true)) return -1;
    } else {
        ihm2_launch_linearize(h);
        if (sens_snapshot(h)) return -1;
        HIP_TRY(hipStreamWaitEvent(h->stream, h->ev_join, 0));
        HIP_TRY(hipEventRecord(h->ev[1], h->stream));
        if (launch_qp(h)) return fail("problem exceeds the QP kernel limits (LDS or constraint slots)");
        sens_after_qp(h);
    }
    HIP_TRY(hipEventRecord(h->ev[2], h->stream));
    HIP_TRY(hipGetLastError());
    return 0;
}

// room for the histories of ihm2mpc_run_steps: growing them costs a few device allocations, which a caller that times its
// run_steps calls wants to have behind it (and, while an x0 sensitivity mode is on, for the gain history of ihm2mpc_run_steps_sens)
int ihm2mpc_reserve_history(ihm2mpc_handle *h, int32_t n_steps)
{
    CHECK_H(h);
    if (n_steps < 1) return fail("n_steps must be >= 1");
    const size_t B = h->B, n = n_steps;
    // (a run_steps(wait = false) launch may still write the old buffers)
    if (h->hist_u0.size() < n * B * 2) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->hist_u0.reset(); h->hist_x0.reset(); h->hist_st.reset(); h->hist_it.reset();
        if (alloc_all(h->hist_u0, n * B * 2, h->hist_x0, n * B * 8, h->hist_st, n * B, h->hist_it, n * B)) return -1;
    }
    if (h->sens_mode && h->hist_k.size() < n * B * NU * NX) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(h->hist_k.alloc(n * B * NU * NX));
    }
    return 0;
}

// n_steps control steps of the MiL loop with everything on the device (python/main.py:476-517).  Where the configuration has a
// persistent instantiation (fkin6 OCP, RTI, all-hard constraint table) this is ONE launch in which every instance runs its
// steps back to back; otherwise n_steps x ihm2mpc_step.  Same results either way.  sens (ihm2mpc_run_steps_sens): with the x0
// sensitivities of every step -- k_steps<..., SENS = 1>, or ihm2mpc_step with k_sens behind every QP -- and their history.
static int run_steps(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double s_target, int32_t n_steps, int32_t freeze, double lap_stop,
                     double *u0_hist, double *x0_hist, int32_t *status_hist, int32_t *qp_iter_hist, bool sens, double *sens_u0_hist)
{
    if (ready(h)) return -1;
    if (check_plant(h, model, M_sim)) return -1;
    if (n_steps < 1) return fail("n_steps must be >= 1");
    const size_t B = h->B, n = n_steps;
    if (ihm2mpc_reserve_history(h, n_steps)) return -1;
    if (freeze && !h->active_set && !h->freeze_armed) {       // every car starts driving; later calls keep the mask the device updated
        std::vector<int32_t> ones(B, 1);
        HIP_TRY(hipMemcpyAsync(h->active, ones.data(), B * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->freeze_armed = true;
    }
    // x0 sensitivities: without `sens` none from the persistent loop, and none from its launches per step either (the same results
    // either way); with it, the last step's are readable afterwards
    if (h->sens_mode) h->sens_state = sens ? 0 : 2;
    struct Quiet { ihm2mpc_handle *h; bool was; ~Quiet() { h->sens_quiet = was; } } quiet{h, h->sens_quiet};
    h->sens_quiet = !sens;
    if (h->cfg.nlp_solver_type == IHM2MPC_SQP && sqp_buffers(h)) return -1;
    if (h->cfg.nlp_solver_type == IHM2MPC_SQP && ihm2::ladder_rollouts(ihm2_situation(h)) && sqp_phi_buffer(h, nullptr)) return -1;
    // the loop or launches per step (qp_select.hpp: select_run), with the buffers above in place
    const ihm2::RunChoice run = ihm2::select_run(ihm2_situation(h), sens ? 1 : 0, freeze != 0);
    int per_step = run.how;
    if (run.how == ihm2::RUN_PERSISTENT) {
        HIP_TRY(hipEventRecord(h->ev[0], h->stream));
        HIP_TRY(hipEventRecord(h->ev[1], h->stream));
        // (not launched after all: the plant's tableau could not be uploaded)
        per_step = launch_steps(h, run.steps, model, M_sim, s_target, n_steps, freeze ? 1 : 0, lap_stop, sens ? 1 : 0) ? ihm2::RUN_PER_STEP_NO_INSTANTIATION : 0;
        if (!per_step) HIP_TRY(hipEventRecord(h->ev[2], h->stream));
        if (!per_step && sens) h->sens_state = 1;
    }
    if (per_step) {
        if (freeze) return fail("no persistent loop for this configuration (needs batch-shared weights and rows for soft tables or the collocation integrator, and a batch of at most %d): call ihm2mpc_step per control period", 4 * h->n_cu);
        ihm2::encode_launch(h->launch_rec, QpKey{QP_STEPS}, per_step);      // the per-step QP launches below update [0..4]
        for (size_t i = 0; i < n; i++) {      // launches per step, histories by device-to-device copies in stream order
            if (ihm2mpc_step(h, model, M_sim, s_target)) return -1;
            HIP_TRY(hipMemcpyAsync(h->hist_u0 + i * B * 2, h->u0, B * 2 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->hist_x0 + i * B * 8, h->x0, B * 8 * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->hist_st + i * B, h->status, B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->hist_it + i * B, h->qp_iter, B * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
            if (sens) HIP_TRY(hipMemcpyAsync(h->hist_k + i * B * NU * NX, h->sens_u0, B * NU * NX * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
        }
    }
    HIP_TRY(hipGetLastError());
    // histories: stream-ordered copies; pinned destinations (ihm2mpc_host_alloc) do not block the host
    if (u0_hist) HIP_TRY(hipMemcpyAsync(u0_hist, h->hist_u0, n * B * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (x0_hist) HIP_TRY(hipMemcpyAsync(x0_hist, h->hist_x0, n * B * 8 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (status_hist) HIP_TRY(hipMemcpyAsync(status_hist, h->hist_st, n * B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (qp_iter_hist) HIP_TRY(hipMemcpyAsync(qp_iter_hist, h->hist_it, n * B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (sens_u0_hist) HIP_TRY(hipMemcpyAsync(sens_u0_hist, h->hist_k, n * B * NU * NX * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return 0;
}

int ihm2mpc_run_steps(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double s_target, int32_t n_steps, int32_t freeze, double lap_stop,
                      double *u0_hist, double *x0_hist, int32_t *status_hist, int32_t *qp_iter_hist)
{
    CHECK_H(h);
    return run_steps(h, model, M_sim, s_target, n_steps, freeze, lap_stop, u0_hist, x0_hist, status_hist, qp_iter_hist, false, nullptr);
}

int ihm2mpc_run_steps_sens(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double s_target, int32_t n_steps, int32_t freeze, double lap_stop,
                           double *u0_hist, double *x0_hist, int32_t *status_hist, int32_t *qp_iter_hist, double *sens_u0_hist)
{
    CHECK_H(h);
    if (!h->sens_mode) return fail("x0 sensitivities are off: ihm2mpc_set_x0_sensitivities(h, 1 or 2) before ihm2mpc_run_steps_sens");
    return run_steps(h, model, M_sim, s_target, n_steps, freeze, lap_stop, u0_hist, x0_hist, status_hist, qp_iter_hist, true, sens_u0_hist);
}

// ---- Cartesian side of the ROS stack (N2 plants, N3 projection) ----
int ihm2mpc_set_track_geometry(ihm2mpc_handle *h, const double *X_ref, const double *Y_ref, const double *phi_ref)
{
    CHECK_H(h);
    if (!X_ref || !Y_ref || !phi_ref) return fail("null argument");
    const size_t n = (size_t)h->cfg.ntracks * h->cfg.nknots;
    if (upload_shared(h, X_ref, h->X_ref, n) || upload_shared(h, Y_ref, h->Y_ref, n) || upload_shared(h, phi_ref, h->phi_ref, n)) return -1;
    h->geometry_set = true;
    return 0;
}

static int check_cart(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double dt_sim, int32_t n_steps)
{
    if (model != IHM2MPC_PLANT_KIN6 && model != IHM2MPC_PLANT_DYN6 && model != IHM2MPC_PLANT_ROS) return fail("unknown Cartesian plant %d", model);
    if (M_sim < 1 || n_steps < 1) return fail("M_sim and n_steps must be >= 1");
    if (!(dt_sim > 0.0)) return fail("dt_sim must be positive");
    (void)h;
    return 0;
}

int ihm2mpc_sim_step_cart(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double dt_sim, int32_t n_steps, double v_dyn,
                          const double *x, const double *u, double *x_next)
{
    CHECK_H(h);
    if (!x || !u || !x_next) return fail("null argument");
    if (check_cart(h, model, M_sim, dt_sim, n_steps)) return -1;
    double *xs = h->scratch, *us = h->scratch + (size_t)h->B * 8, *xn = h->scratch + (size_t)h->B * 16;
    if (upload(h, x, xs, NX) || upload(h, u, us, NU)) return -1;
    ihm2_launch_sim_cart(h, model, M_sim, dt_sim, n_steps, v_dyn, xs, us, xn, h->stream);
    HIP_TRY(hipGetLastError());
    return download(h, xn, x_next, NX);
}

int ihm2mpc_sim_step_dyn10(ihm2mpc_handle *h, int32_t M_sim, const double *x, const double *u, double *x_next)
{
    CHECK_H(h);
    if (!h->tracks_set) return fail("ihm2mpc_set_tracks has not been called");
    if (!x || !u || !x_next) return fail("null argument");
    if (check_sim_substeps(h, M_sim, "torque lags (t_T = 1e-3 s)")) return -1;
    if (h->cfg.sim_integrator_type == IHM2MPC_INTEG_ERK_LAG)
        return fail("the plant integrator ERK_LAG (closed-form actuator lags) is implemented for the kinematic plant (model 0) only, not for the "
                    "fdyn10 plant: create the handle with another sim_integrator_type");
    const bool irk = ihm2_is_irk(h->cfg.sim_integrator_type);          // (ERK_LAG is refused above)
    if (!h->dyn10) HIP_TRY(h->dyn10.alloc((size_t)h->B * 35));
    double *xs = h->dyn10, *us = h->dyn10 + (size_t)h->B * 15, *xn = h->dyn10 + (size_t)h->B * 20;
    if (upload(h, x, xs, 15) || upload(h, u, us, 5)) return -1;
    // the handle's plant integrator (python/main.py:395-400: IRK, GAUSS_RADAU_IIA): collocation steps of at most dt / M_sim, each
    // solved to convergence within IHM2MPC_DYN10_NEWTON_MAX Newton iterations or cut (kernels_dyn10.hip) -- usable from rest
    if (irk) ihm2_launch_sim_dyn10_irk(h, h->cfg.sim_integrator_type, M_sim, IHM2MPC_DYN10_NEWTON_MAX, xs, us, xn, h->stream);
    else ihm2_launch_sim_dyn10(h, M_sim, xs, us, xn, h->stream);
    HIP_TRY(hipGetLastError());
    return download(h, xn, x_next, 15);
}

int ihm2mpc_project(ihm2mpc_handle *h, const double *x_cart, double *s_guess, double s_tol, double *x_frenet)
{
    CHECK_H(h);
    if (!x_cart || !s_guess || !x_frenet) return fail("null argument");
    if (!h->tracks_set || !h->geometry_set) return fail("ihm2mpc_set_tracks / ihm2mpc_set_track_geometry have not been called");
    if (!(s_tol > 0.0)) return fail("s_tol must be positive");
    double *xs = h->scratch, *sg = h->scratch + (size_t)h->B * 8, *xf = h->scratch + (size_t)h->B * 9;
    if (upload(h, x_cart, xs, NX) || upload(h, s_guess, sg, 1)) return -1;
    ihm2_launch_project(h, s_tol, xs, sg, xf, h->stream);
    HIP_TRY(hipGetLastError());
    if (download(h, xf, x_frenet, NX)) return -1;
    return download(h, sg, s_guess, 1);
}

int ihm2mpc_set_cart_state(ihm2mpc_handle *h, const double *x_cart, const double *s_guess)
{
    CHECK_H(h);
    if (!x_cart || !s_guess) return fail("null argument");
    if (upload(h, x_cart, h->xc, NX)) return -1;
    return upload(h, s_guess, h->s_guess, 1);
}

int ihm2mpc_get_cart_state(ihm2mpc_handle *h, double *x_cart, double *s_guess)
{
    CHECK_H(h);
    if (x_cart && download(h, h->xc, x_cart, NX)) return -1;
    if (s_guess && download(h, h->s_guess, s_guess, 1)) return -1;
    return 0;
}

int ihm2mpc_sim_advance_cart(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double dt_sim, int32_t n_steps, double v_dyn, double s_tol)
{
    CHECK_H(h);
    if (!h->tracks_set || !h->geometry_set) return fail("ihm2mpc_set_tracks / ihm2mpc_set_track_geometry have not been called");
    if (check_cart(h, model, M_sim, dt_sim, n_steps)) return -1;
    if (!(s_tol > 0.0)) return fail("s_tol must be positive");
    ihm2_launch_sim_cart(h, model, M_sim, dt_sim, n_steps, v_dyn, h->xc, h->u0, h->xc, h->stream);
    ihm2_launch_project(h, s_tol, h->xc, h->s_guess, h->x0, h->stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
