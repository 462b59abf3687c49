// qp_select.hpp -- what a launch takes, as a function of the facts of the handle that decide it: the instantiation of the catalogue
// (qp_catalogue.hpp) for the QP and the step loop, the linearisation and plant kernels, whether ihm2mpc_run_steps runs the loop or launches
// per step, the launches of the line search's ladder -- and the launch record that says what was taken (ihm2mpc_get_launch_record).
// Plain C++17, no HIP: api.hip: ihm2_situation fills a QpSituation from the handle for every launch, and the launchers switch on the
// choice; tools/probes/check_qp_select.cpp fills one from a problem file and prints the choices, which the CPU tests compare with the
// tables the GPU tests assert on hardware (tests/launch_cases.py, tests/steps_cases.py).  A wrong choice is silent -- the launches per
// step and the slower forms give the same results -- so this is where it is tested.
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
    bool linearize_cols;                                    // IHM2MPC_LINEARIZE_COLS: the column-parallel linearisation at any batch size (select_linearize)
    bool persistent_rounds;                                 // IHM2MPC_PERSISTENT_ROUNDS: the one-launch loop for batches that are not resident (select_run)
};

// The collocation integrators among IHM2MPC_INTEG_* (ERK and ERK_LAG are the explicit ones).  Not "!= ERK": ERK_LAG is explicit too.
inline bool is_irk(int type) { return type == IHM2MPC_INTEG_IRK_GL4 || type == IHM2MPC_INTEG_IRK_RADAU4; }
// the shooting intervals are integrated by collocation
inline bool collocation(const QpSituation &s) { return is_irk(s.integrator_type); }
// The 128-interval switch: the few instances of a real-time controller, whose linearisation and plant step lie on the critical path of
// ihm2mpc_step.  The same as ceil(B N / 64) <= 2: at most two blocks of the lane-per-interval linearisation.
inline bool latency_batch(const QpSituation &s) { return (long)s.B * s.N <= 128; }

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
    const int irk = collocation(s) ? 1 : (s.integrator_type == IHM2MPC_INTEG_ERK_LAG) ? 2 : 0;
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

// How ihm2mpc_run_steps proceeds.  The persistent loop pays off while every instance has a wavefront slot of its own (the QP's 40 KB of
// LDS allow 4 per CU): a larger batch would run in rounds of whole n_steps-long loops, whereas launches per step backfill the slots of
// finished QPs with the next instances.  (IHM2MPC_PERSISTENT_ROUNDS=1: the one-launch loop for larger batches too -- the workgroups then
// run in rounds of whole histories, NOTES.md R4 -- but not with `freeze`.)  The two per-step outcomes are the launch record's
// steps_fallback codes; `freeze` has no per-step form and is refused instead.
enum RunHow { RUN_PERSISTENT = 0, RUN_PER_STEP_NO_INSTANTIATION = 1, RUN_PER_STEP_NOT_RESIDENT = 2, RUN_REFUSED = 3 };
struct RunChoice { QpChoice steps; RunHow how; };
inline RunChoice select_run(const QpSituation &s, int sens, bool freeze)
{
    const QpChoice c = select_steps(s, sens);
    const bool resident = s.B <= 4 * s.n_cu || (s.persistent_rounds && !freeze);
    if (resident && c.pos >= 0) return {c, RUN_PERSISTENT};
    if (freeze) return {c, RUN_REFUSED};
    return {c, resident ? RUN_PER_STEP_NO_INSTANTIATION : RUN_PER_STEP_NOT_RESIDENT};
}

// ---- the SQP mode's backtracking ladder ----
// Trial step lengths 1, rho, rho^2, ... >= alpha_min -- the same floating-point sequence as the loop of line_search_body (sqp_body.hpp).
// ihm2mpc_set_sqp_options refuses option pairs whose ladder is longer than IHM2MPC_LS_MAX_TRIALS: one length everywhere (the buffer of
// the collocation rollouts, the rollout launches, the line search).  A longer ladder is reported as IHM2MPC_LS_MAX_TRIALS + 1.
#define IHM2MPC_LS_MAX_TRIALS 64
inline int ladder_length(double alpha_min, double alpha_red)
{
    int n = 1;
    for (double al = alpha_red; al >= alpha_min && n <= IHM2MPC_LS_MAX_TRIALS; al *= alpha_red) n++;
    return n;
}
// With the collocation integrator the line search reads the rollouts of its trial points from a launch of their own (k_rollout_irk);
// with the explicit ones it integrates them itself.
inline bool ladder_rollouts(const QpSituation &s) { return collocation(s) && s.sqp_globalization != 0; }
// The step lengths whose rollouts the first of those launches takes, of a ladder of n_alpha (0: no such launch).  Most instances accept
// one of the first three: those for everybody, the rest of the ladder in a second launch for the instances the first line-search launch
// leaves open.  A few instances -- the whole ladder is one round of wavefronts on the chip -- keep the single launch.
inline int ladder_first(const QpSituation &s, int n_alpha)
{
    if (!ladder_rollouts(s)) return 0;
    return (n_alpha < 3 || (long)n_alpha * (long)s.B * (long)s.N <= 16384) ? n_alpha : 3;
}

// ---- the launch record: sixteen integers (include/ihm2mpc.h: ihm2mpc_get_launch_record; ihm2_amd/solver.py: decode_launch_record) ----
// [0..4] the per-step QP's key, [5..14] the step loop's, [15] bits 0..3 the last linearisation kernel, 4..7 the last plant kernel,
// 8..9 / 12..13 the form of the factor sweep in the QP / the loop (QpKey.nf), 10 / 14 the form of their slot phases (QpKey.full)
enum LinKernel { LIN_KERNEL_NONE = 0, LIN_K_LINEARIZE = 1, LIN_K_LINEARIZE_DYN = 2, LIN_K_LINEARIZE_COLS = 3, LIN_K_LINEARIZE_IRK = 4, LIN_K_LINEARIZE_LAG = 5 };
enum SimKernel { SIM_KERNEL_NONE = 0, SIM_K_SIM_STEP_KIN = 1, SIM_K_SIM_STEP = 2, SIM_K_SIM_IRK = 3, SIM_K_SIM_STEP_KIN_LAG = 4, SIM_K_SIM_SENS = 5 };
inline void note_lin(int32_t rec[16], LinKernel code) { rec[15] = (rec[15] & ~0xF) | code; }
inline void note_sim(int32_t rec[16], SimKernel code) { rec[15] = (rec[15] & ~0xF0) | (code << 4); }

// The linearisation kernel of ihm2mpc_linearize, _solve and _step (kernels_linearize.hip: ihm2_launch_linearize).  ERK_LAG: one kernel at
// every batch size -- with sub-steps sized for the car (M = 4) the column-parallel latency path has nothing left to hide.  The column-parallel
// kernel -- one sensitivity column per wavefront, ten wavefronts per block of 64 intervals -- is the latency path of the kinematic model
// with RK4 (not bit-identical to the batch kernel); IHM2MPC_LINEARIZE_COLS=1 takes it at any batch size (tools/bench_linearize.py --cols).
inline LinKernel select_linearize(const QpSituation &s)
{
    if (collocation(s)) return LIN_K_LINEARIZE_IRK;
    if (s.integrator_type == IHM2MPC_INTEG_ERK_LAG) return LIN_K_LINEARIZE_LAG;
    if (s.model != IHM2MPC_MODEL_FKIN6) return LIN_K_LINEARIZE_DYN;
    if (latency_batch(s) || s.linearize_cols) return LIN_K_LINEARIZE_COLS;
    return LIN_K_LINEARIZE;
}

// The plant kernel of ihm2mpc_sim_step, _sim_advance and _step for the plant model -2 .. 2 (kernels_linearize.hip: ihm2_launch_sim); none:
// the closed-form lags integrate the plain kinematic plant only, and the API refuses the call.  The plain kinematic plant shares the
// integrator of the shooting intervals (k_sim_step_kin, bit-identical to lane N of the persistent loop); on a latency batch its discarded
// sensitivities would put 0.1 ms on the critical path of ihm2mpc_step: those take the state-only rollout (k_sim_step), and so does a handle
// whose shooting intervals are not integrated by RK4 (nothing to share: the loop runs the plant as a phase of its own on one lane).
inline SimKernel select_sim(const QpSituation &s, int plant_model)
{
    if (is_irk(s.sim_integrator_type)) return SIM_K_SIM_IRK;
    if (s.sim_integrator_type == IHM2MPC_INTEG_ERK_LAG) return plant_model == IHM2MPC_MODEL_FKIN6 ? SIM_K_SIM_STEP_KIN_LAG : SIM_KERNEL_NONE;
    if (plant_model == IHM2MPC_MODEL_FKIN6 && !latency_batch(s) && s.integrator_type == IHM2MPC_INTEG_ERK) return SIM_K_SIM_STEP_KIN;
    return SIM_K_SIM_STEP;
}

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
