// qp_select.hpp -- which instantiation of the catalogue (qp_catalogue.hpp) a launch takes, as a function of the facts of the handle that
// decide it, and the launch record that says what was taken (ihm2mpc_get_launch_record).  Plain C++17, no HIP: api.hip fills a QpSituation
// from the handle on every launch and maps the chosen position to its kernel; tools/probes/check_qp_select.cpp fills one from a problem
// file and prints the choice, which the CPU tests compare with the tables the GPU tests assert on hardware.  A wrong choice is silent --
// the launches per step and the slower forms give the same results -- so this is where it is tested.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/ihm2mpc.h"
#include "qp_catalogue.hpp"
#include "qp_lds.hpp"

namespace ihm2 {

// The facts the selection reads, and nothing else of the handle.
struct QpSituation {
    int N, B, n_cu;                                         // horizon, batch, compute units of the device
    int model, integrator_type, sim_integrator_type;        // cfg: the OCP's model, its integrator and the plant's (IHM2MPC_MODEL_*, IHM2MPC_INTEG_*)
    int nlp_solver_type, sqp_globalization;
    int per_lane, per_blk, nsoft, m_act;                    // of the slot table (qp_tables.hpp: SlotTable)
    bool slots_full;                                        // the table, with its per-instance bounds if any, is full (qp_tables.hpp: slot_table_full)
    int path;                                               // the PATH of the instantiations that take the rows: 0 none, 1 the track rows, 2 the track rows and the lateral-acceleration row
    bool uni;                                               // uniform_H && uniform_CD
    bool inst_b, block_qp;                                  // per-instance bounds; k_qp_block allowed (IHM2MPC_BLOCK_QP)
    int qp_form;                                            // IHM2MPC_QP_FORM: 0 .. 3 (unset: 3), see factor_form
    bool irk_tab, ls_x, ls_phi;                             // the buffers exist: the collocation tableau, the line search's iterate, its trial rollouts
    int sens_lds;                                           // doubles of LDS the x0-sensitivity body takes (kernels_sens.hip)
};

// a choice: the position of the key in catalogue_keys() (-1: none) and the dynamic LDS of the launch in bytes
struct QpChoice { int pos; size_t lds; };

// the first entry of the catalogue with the fields of `want` and at least its NSLOT; -1: none
inline int find_inst(const QpKey &want)
{
    const std::vector<QpCatKey> &keys = catalogue_keys();
    for (size_t i = 0; i < keys.size(); i++) {
        const QpKey &k = keys[i].key;
        if (k.kind == want.kind && k.nsoft == want.nsoft && k.path == want.path && k.uni == want.uni && k.sqp == want.sqp &&
            k.irk == want.irk && k.dyn == want.dyn && k.sens == want.sens && k.nf == want.nf && k.full == want.full && k.nslot >= want.nslot)
            return (int)i;
    }
    return -1;
}

// The form of the factor sweep the handle's QP may take (QpKey.nf; riccati_mfma.hpp: PLAIN).  The straight-line stage keeps neither the
// symmetrising tile (the dynamic model as written needs it) nor the p_k stores (a table without active rows needs them): 0 then.  Otherwise
// 40 for the horizon 40 -- the horizon as a compile-time constant -- and -1 for every other one.  IHM2MPC_QP_FORM (QpSituation.qp_form)
// makes the forms comparable in one build: 2 keeps the slot phases on their general form (slot_form), 1 keeps the horizon 40 on the
// run-time form as well, 0 keeps every launch on the general form.
inline int factor_form(const QpSituation &s)
{
    if (s.qp_form == 0 || s.model == IHM2MPC_MODEL_FDYN6 || s.m_act == 0) return 0;
    return (s.N == 40 && s.qp_form >= 2) ? 40 : -1;
}
// The form of the slot phases (QpKey.full; kernels_qp.hip: qp_wave_body, FULL): 1 where the handle's table -- with its per-instance bounds,
// if it has any -- is full (qp_tables.hpp: slot_table_full, evaluated where the table is laid out and where bounds are uploaded) and the
// factor sweep takes the compiled-in horizon, the one form the catalogue has it with.
inline int slot_form(const QpSituation &s) { return (s.qp_form == 3 && s.slots_full && factor_form(s) == 40) ? 1 : 0; }

// find_inst with the factor sweep in the form the handle may take, where the catalogue has the instantiation in that form (the
// full slot form first, then the compile-time horizon, then the run-time one), else in the general form
inline int find_form(const QpSituation &s, QpKey want)
{
    if (slot_form(s)) {
        want.nf = 40; want.full = 1;
        if (const int e = find_inst(want); e >= 0) return e;
        want.full = 0;
    }
    for (int nf = factor_form(s); nf != 0; nf = (nf > 0) ? -1 : 0) {
        want.nf = nf;
        if (const int e = find_inst(want); e >= 0) return e;
    }
    want.nf = 0;
    return find_inst(want);
}

// the LDS layout of the QP that takes the handle's rows and weights (qp_lds.hpp): what the kernels carve up is what the launch asks for
inline QpLds qp_layout(const QpSituation &s) { return qp_lds(s.N, qp_lds_class(s.path, s.uni)); }
// the persistent loop's: the QP's with its guests (sens: k_sens' body after every QP)
inline StepsLds steps_lds(const QpSituation &s, int sens)
{
    const bool dyn_rk4 = s.model != IHM2MPC_MODEL_FKIN6 && s.integrator_type == IHM2MPC_INTEG_ERK;
    return steps_lds_doubles(qp_layout(s).total, sens ? s.sens_lds : 0, dyn_rk4);
}

// The per-step QP for the handle's table; none: no instantiation takes it (or not in the LDS)
inline QpChoice select_qp(const QpSituation &s)
{
    const size_t lds = sizeof(double) * (size_t)qp_layout(s).total;
    if (lds > 160 * 1024) return {-1, lds};
    // few instances (at most one per CU): four wavefronts per instance, slots from the 256-lane table
    // (per-instance bounds: the 64-lane table alone carries them -- k_qp_wave's results are the four-wave kernel's bit for bit)
    if (s.block_qp && !s.inst_b && s.per_blk >= 1 && s.B <= s.n_cu && s.per_lane * 64 <= (s.N + 1) * 12)
        if (const int e = find_inst({QP_BLOCK, s.per_blk, s.nsoft, s.path, s.uni, 0, 0, 0, 0, 0, 0}); e >= 0) return {e, lds};
    return {find_form(s, {QP_WAVE, s.per_lane, s.nsoft, s.path, s.uni, 0, 0, 0, 0, 0, 0}), lds};
}

// The persistent loop for the handle's configuration; none: ihm2mpc_run_steps then launches per step, which gives the same results.  The
// catalogue has it for the kinematic and the dynamic OCP models, not for the lateral-acceleration row; with soft sides, track rows, the
// collocation integrator or a dynamic model for batch-shared tables only (UNI = 1).  sens = 1 (ihm2mpc_run_steps_sens): the loop with
// x0 sensitivities, for the kinematic OCP model in the RTI mode.
inline QpChoice select_steps(const QpSituation &s, int sens = 0)
{
    const StepsLds lds = steps_lds(s, sens);
    const size_t bytes = sizeof(double) * (size_t)lds.total();
    const bool sqp = s.nlp_solver_type == IHM2MPC_SQP;
    // QpKey.irk: 0 RK4, 1 collocation, 2 RK4 with the closed-form lags
    const int irk = (s.integrator_type == IHM2MPC_INTEG_IRK_GL4 || s.integrator_type == IHM2MPC_INTEG_IRK_RADAU4) ? 1
                    : (s.integrator_type == IHM2MPC_INTEG_ERK_LAG) ? 2 : 0;
    const bool dyn = s.model != IHM2MPC_MODEL_FKIN6;
    if (irk == 1 && (!s.irk_tab || (sqp && s.sqp_globalization && !s.ls_phi))) return {-1, bytes};
    // a plant with the closed-form lags rides on lane N of the loop that linearises with them; the other loops have no such plant
    if (s.sim_integrator_type == IHM2MPC_INTEG_ERK_LAG && irk != 2) return {-1, bytes};
    if (sqp && !s.ls_x) return {-1, bytes};        // the caller allocates the line-search buffers first
    if (bytes > 160 * 1024) return {-1, bytes};
    // the dynamic models' RK4 integrator parks its base sensitivities in the QP's LDS
    if (!lds.guests_fit()) return {-1, bytes};
    // the SQP instantiations keep the sweeps' earlier form, whose unclamped prefetch of LDS operands starts in front of the block's LDS at
    // N = 2 and N = 3 (by 60 and 24 words; the values are never used): those horizons are launched per step
    if (sqp && !qp_sweeps_inside(qp_layout(s), s.N, false, 0, 0)) return {-1, bytes};
    return {find_form(s, {QP_STEPS, s.per_lane, s.nsoft, s.path, s.uni, sqp, irk, dyn, sens, 0, 0}), bytes};
}

// ---- the launch record: sixteen integers (include/ihm2mpc.h: ihm2mpc_get_launch_record; ihm2_amd/solver.py: decode_launch_record) ----
// [0..4] the per-step QP's key, [5..14] the step loop's, [15] bits 0..3 the last linearisation kernel, 4..7 the last plant kernel,
// 8..9 / 12..13 the form of the factor sweep in the QP / the loop (QpKey.nf), 10 / 14 the form of their slot phases (QpKey.full)
enum LinKernel { LIN_KERNEL_NONE = 0, LIN_K_LINEARIZE = 1, LIN_K_LINEARIZE_DYN = 2, LIN_K_LINEARIZE_COLS = 3, LIN_K_LINEARIZE_IRK = 4, LIN_K_LINEARIZE_LAG = 5 };
enum SimKernel { SIM_KERNEL_NONE = 0, SIM_K_SIM_STEP_KIN = 1, SIM_K_SIM_STEP = 2, SIM_K_SIM_IRK = 3, SIM_K_SIM_STEP_KIN_LAG = 4, SIM_K_SIM_SENS = 5 };
inline void note_lin(int32_t rec[16], LinKernel code) { rec[15] = (rec[15] & ~0xF) | code; }
inline void note_sim(int32_t rec[16], SimKernel code) { rec[15] = (rec[15] & ~0xF0) | (code << 4); }

// the record from the key of what was launched; a k_steps key with `per_step` != 0: run_steps launched per step instead (1 no
// instantiation, 2 the batch is not resident), the key's fields are 0
inline void encode_launch(int32_t r[16], const QpKey &k, int per_step = 0)
{
    const int form = (k.nf > 0) ? 2 : (k.nf < 0) ? 1 : 0;
    if (k.kind != QP_STEPS) {
        r[0] = k.kind; r[1] = k.nslot; r[2] = k.nsoft; r[3] = k.path; r[4] = k.uni;
        r[15] = (r[15] & ~0x700) | (form << 8) | ((k.full ? 1 : 0) << 10);
    } else {
        r[15] = (r[15] & ~0x7000) | ((per_step ? 0 : form) << 12) | ((!per_step && k.full ? 1 : 0) << 14);
        r[5] = per_step ? 2 : 1; r[6] = k.nslot; r[7] = k.nsoft; r[8] = k.path; r[9] = k.uni; r[10] = k.sqp; r[11] = k.irk; r[12] = k.dyn;
        r[13] = per_step; r[14] = k.sens;
    }
}

}  // namespace ihm2
