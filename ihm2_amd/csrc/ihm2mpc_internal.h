// ihm2mpc_internal.h -- handle layout and kernel launchers shared by the .hip translation units.
//
// Device data layout (DESIGN.md "Data layout in HBM"): instance-major, identical to the C-ABI's host
// layout, e.g. x[b][k][i] (B, N+1, 8).  The two hot kernels are shaped around it:
//   * linearize: one lane per (instance, interval), interval fastest -> a wavefront reads 64
//     consecutive 64-byte state rows (4 KB contiguous) and writes 64 consecutive 704-byte [A|B|b] records;
//   * QP: one wavefront per instance -> every per-stage record (704 B of [A|B|b], 512 B of P) is one
//     coalesced wave access, the iterate lives in LDS, multipliers/slacks in registers.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ihm2mpc.h"
#include "ihm2_dims.h"     // NX, NU, NZ, NY, NG, NH, NC, NLAM, MAX_SLOTS

// Floating-point contraction.  The sources are compiled with -ffp-contract=on (Makefile) and switch to `fast` HERE, for everything that follows in
// the translation unit: a*b + c is then fused wherever the two operations meet, as before -- but by the `contract` flag on the operations, not by
// the back end's global switch (-ffp-contract=fast), which fuses every multiply-add pair it sees and cannot be turned off for a region.  The
// dynamic model's section of model.hpp turns contraction OFF: its results must not depend on what it is inlined into (NOTES.md R4.11).
#pragma clang fp contract(fast)

#include "qp_tables.hpp"      // ConstraintRows, SlotTable: the handle holds one of each

#define QM_PAD 24    // >= 3 x ring depth of the vector / forward sweeps: their unclamped prefetch overshoots an instance by < 3 D rows (stage-major rows;
                     // the stage-pair-major rows of the compiled-in horizon: D pair rows = 2 D stage rows, qp_mrows.hpp: qm_pair_inside)
#define LIN_REC 96   // doubles per (instance, interval) linearisation record: A (64) | B (16) | b (8) | rb (8: the QP's dynamics residual, riccati_mfma.hpp)

#include "qp_select.hpp"      // the launch decisions, host-only: QpSituation and the selectors that read it, the launch record

// the collocation integrators among IHM2MPC_INTEG_* (qp_select.hpp: is_irk, the one spelling of it)
static inline bool ihm2_is_irk(int type) { return ihm2::is_irk(type); }
// IHM2MPC_INTEG_ERK_LAG: the stage factors {E_0, E_1, E_2, e} of the torque lag, then of the steering lag, for sub-steps of h
// (ihm2mpc_lag_stage_factors on the model's two time constants; kernels_linearize.hip) -- computed on the host, a kernel argument
struct LagFac { double f[8]; };
LagFac ihm2_lag_factors(double h);

struct ihm2mpc_comm;      // comm.hip: RCCL communicator + staging buffers of a one-process-per-GPU job
namespace ihm2 { struct IrkTab; }

// The owner of one device array (host code only).  alloc(n) gives n elements, every byte set to the buffer's fill byte (0 unless the buffer
// was poisoned, see WorkBuf): the fill runs on the null stream and is waited for, since the handle's streams are non-blocking and an upload
// that overtook it would be overwritten afterwards.  It converts to T *, which the argument blocks and the launches take.
//
// Every buffer is declared through one of the two classes below (DESIGN.md "Data layout in HBM"; tests/test_buffer_classes.py fails for a
// member of the handle declared as a bare DevBuf):
//   StateBuf  state / problem data: the contents carry meaning from call to call, or zero is the documented default
//   WorkBuf   workspace / outputs: a call must write what it, or a getter after it, reads
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { reset(); }
    // the old array is released first; on failure the buffer is empty
    hipError_t alloc(size_t n)
    {
        reset();
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, n * sizeof(T));
        if (e == hipSuccess) e = hipMemset(q, fill_, n * sizeof(T));
        if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        if (e != hipSuccess) { (void)hipFree(q); return e; }
        p_ = (T *)q; n_ = n;
        return hipSuccess;
    }
    void reset()
    {
        if (p_) (void)hipFree(p_);
        p_ = nullptr; n_ = 0;
    }
    size_t size() const { return n_; }     // elements
    T *get() const { return p_; }
    operator T *() const { return p_; }
protected:
    int fill_ = 0;      // the byte alloc() fills with
private:
    T *p_ = nullptr;
    size_t n_ = 0;
};

template <typename T>
class StateBuf : public DevBuf<T> {};

// IHM2MPC_POISON_WORKSPACE (read when a handle is created, api.hip: arm_poison) poisons workspace: every later alloc() of a poisoned
// buffer, regrowth included, fills with 0xFF bytes -- NaN -- instead of zeros, so that a read of a word no call wrote shows in the results.
// Only a workspace of doubles can be poisoned: an integer read early may be an index, and an out-of-range index is a memory fault, where
// a NaN is arithmetic only.
template <typename T>
class WorkBuf : public DevBuf<T> {
public:
    void poison(bool on)
    {
        static_assert(sizeof(T) == sizeof(double) && T(0.5) != T(0), "only a workspace of doubles is poisoned");
        this->fill_ = on ? 0xFF : 0;
    }
};

// What the per-instance slack penalties (ihm2mpc_set_instance_soft / _alat_soft) keep on the device beside the constraint tables
// (i_slot_*, i_st_* of the handle, which hold the penalties of the rows 0..13 and of the slots), allocated while the mode is on: state,
// every member a StateBuf.  The handle holds the block by value (ihm2mpc_handle::ip).
struct ihm2_inst_penalties {
    StateBuf<double> alat_sz, alat_sZ;     // (B,2) the a_lat row's: the cost
    void reset() { alat_sz.reset(); alat_sZ.reset(); }
};

// The device memory of ihm2mpc_eval_adjoint_sensitivities_p_device, which must not wait for its kernels and therefore cannot release work
// buffers when it returns as the host entry does: the outputs the caller does not ask for (the layout of api.hip: PenaltyWork, named
// "penalty_grad_work" for IHM2MPC_POISON_WORKSPACE) land here, grown on demand.  The handle holds the block by value (ihm2mpc_handle::pd).
struct ihm2_penalty_device_work {
    WorkBuf<double> buf;                    // zeta (B,S,NS,10) | grad_z, grad_Z (B,S,NS,28) | grad_za, grad_Za (B,S,NS,2)
};

// Created by value-initialisation (std::make_unique<ihm2mpc_handle>() in ihm2mpc_create): there is no user-provided constructor, so every
// scalar member starts at zero and every buffer empty.  The destructor (api.hip) waits for both streams and releases what is not a buffer.
struct ihm2mpc_handle {
    ~ihm2mpc_handle();

    ihm2mpc_config cfg;
    ihm2mpc_comm *comm;            // nullptr until ihm2mpc_comm_init
    int B, N, NS;
    int n_cu;                      // compute units of the device
    hipStream_t stream;
    hipStream_t stream2;           // plant + reference ramp of ihm2mpc_step run here, beside shift + linearisation
    hipEvent_t ev_fork, ev_join;
    hipEvent_t ev[4];
    bool tracks_set, weights_set, bounds_set;
    bool uniform_H, uniform_CD;    // stage Hessians / general rows identical for all k < N (QP kernel keeps them in LDS)

    // ---- shared problem data (device) ----
    StateBuf<double> s_ref, kappa_ref;     // (ntracks, nknots)
    StateBuf<int32_t> track_id;            // (B)
    StateBuf<double> Hs;                   // (NS,10,10)  cost_scale * V'WV ; terminal: W_e padded with I
    StateBuf<double> Gy;                   // (NS,10,12)  cost_scale * V'W  ; terminal: W_e in the first 8x8
    StateBuf<double> lbx, ubx;             // (NS,8)
    StateBuf<double> lbu, ubu;             // (N,2)
    StateBuf<double> CD;                   // (N,2,10)  general rows [C D]
    StateBuf<double> lg, ug;               // (N,2)
    // the constraint rows as the setters leave them (set_bounds / set_soft / ... may come in any order), and the compact table of the
    // slots with at least one finite side that rebuild_slots lays out from them for the QP kernels (qp_tables.hpp)
    ihm2::ConstraintRows rows;
    ihm2::SlotTable slots;         // the last table that fitted, as the device holds it
    bool slots_full;               // the table (with the per-instance bounds, if any) takes the full slot form (qp_tables.hpp: slot_table_full)
    bool slots_fit;                // false: the rows set so far fit no instantiation (reported by the next solve: a later setter may still change them)
    // The constraint tables on the device, one copy of each (api.hip: tables_to_device uploads the images of qp_tables.hpp: table_images).
    // Every table is a pair of arrays with two halves, the bounds and behind them the slack penalties, so that one base serves both:
    //   the slot table    (2, entries)            lb | zw and ub | Zw, entries = slots.per_lane*64: raw bounds, +-inf if that side is absent
    //                                             (soft slots are one-sided), then the slack cost zw s + 1/2 Zw s^2 of a soft slot, Zw < 0 =
    //                                             hard slot -- the QP, the sensitivities and the adjoint kernels
    //   the stage table   (NS*NC + NS*NLAM)       rows.lb | rows.sz and rows.ub | rows.sZ per (stage, row) and (stage, side) -- the SQP
    //                                             mode's line search and the cost
    // batch-shared here; per instance (B of each, i_slot_*, i_st_* below) while a per-instance mode is on.
    StateBuf<int32_t> slot_kc;             // (entries) stage * 16 + row, -1 = padding
    StateBuf<double> slot_lb, slot_ub;     // the slot table
    StateBuf<int32_t> slot_kc_blk;         // the same rows spread over 256 lanes (k_qp_block: four wavefronts per instance), all-hard tables only
    StateBuf<double> slot_lb_blk, slot_ub_blk;
    std::string poison;            // IHM2MPC_POISON_WORKSPACE as read at creation: "" / "0" off, "1" every workspace of doubles, else a list of names
    bool block_qp;                 // use k_qp_block for batches of at most one instance per CU (IHM2MPC_BLOCK_QP=0 turns it off)
    // nonlinear track-boundary rows (rows 12, 13 of the stages 1..N); the lateral-acceleration row's switch is rows.alat_on
    int path_on;
    double car_L, car_W, lh[NH], uh[NH];
    StateBuf<double> widths;               // (ntracks, 2) = (w_R, w_L)
    // Cartesian side (ROS stack): centre-line geometry per track, Cartesian plant state and projection guess per instance
    bool geometry_set;
    StateBuf<double> X_ref, Y_ref, phi_ref;   // (ntracks, nknots)
    StateBuf<double> xc;                   // (B,8) (X, Y, phi, v_x, v_y, r, T, delta)
    StateBuf<double> s_guess;              // (B)

    // ---- per-instance state, instance-major ----
    StateBuf<double> x;      // (B,NS,8)
    StateBuf<double> u;      // (B,N,2)
    StateBuf<double> x0;     // (B,8)
    StateBuf<double> yref;   // (B,N,12)
    StateBuf<double> yref_e; // (B,8)
    StateBuf<double> pi;     // (B,NS,8)
    StateBuf<double> lam;    // (B,NS,28)
    StateBuf<double> slk;    // (B,NS,28) slack values of the soft sides after the last QP (0 for hard sides)
    StateBuf<double> lam_a, slk_a;   // (B,NS,2) multipliers and slack values of the lateral-acceleration row: lower, upper side
    WorkBuf<double> res;    // (B,4)
    // (n_alpha, B, N, 8) IRK rollouts at the trial points of the line search (SQP mode with the IRK integrator), grown on demand: its
    // n_alpha (the ladder it was grown for, sqp_body.hpp: make_ls_args) is the stride the line search reads it with
    WorkBuf<double> ls_phi;
    StateBuf<ihm2::IrkTab> irk_tab;       // the OCP integrator's collocation tableau, empty for ERK
    StateBuf<ihm2::IrkTab> sim_irk_tab;   // the same for the plant steps of the persistent loop (step dt / sim_irk_M), allocated on first use
    int sim_irk_M;
    WorkBuf<double> dyn10;  // (B,35) staging of the fdyn10 plant: x (15), u (5), x_next (15); allocated on first use
    WorkBuf<double> qp_res; // (B,4) KKT residuals of the QP at its returned point, relative to the scales of its tolerances
    StateBuf<int32_t> status, qp_iter;   // (B)
    StateBuf<int32_t> active;            // (B) plant mask of the device-resident closed loop (nullptr-equivalent while !active_set)
    bool active_set;
    bool freeze_armed;           // a run_steps(freeze) call initialised the mask: later calls keep what the device made of it
    bool lap_wrap;               // prepare_step / step move cars that passed s = L back by one lap first
    // (B,2) first control of the last solve.  State, not an output only: the plant of the next ihm2mpc_step / _sim_advance / _run_steps reads
    // it, so it carries meaning from call to call, and before the first solve it is the documented default 0 (the car coasts)
    StateBuf<double> u0;

    WorkBuf<double> lin;    // (B,N,96) linearisation records [A | B | b | rb], then B spare records (the kinematic plant's by-product)
    // ---- QP workspace in HBM/L2 (everything else of the QP lives in LDS / registers) ----
    WorkBuf<double> q_g;    // (B,NS,10) QP gradient
    WorkBuf<double> q_rg;   // (B,NS,10) stationarity residual of the interior-point iterate (follows the step between two evaluations from the data)
    WorkBuf<double> q_P;    // (B,NS,64) Riccati matrices of the current factorisation
    WorkBuf<double> q_M;    // (QM_PAD + B*N + QM_PAD, 64) closed-loop matrices A - B K (row-major; the vector recursion reads them
                           // transposed), padded at both ends: the sweeps' prefetch rings run QM_PAD rows past an instance unclamped.
                           // An instance's N x 512 bytes are stage-major or stage-pair-major by the kernel that writes and reads them (qp_mrows.hpp)
    WorkBuf<double> scratch;   // (B, 3*8) plant scratch

    // ---- SQP mode (cfg.nlp_solver_type == IHM2MPC_SQP): convergence test + merit line search, kernels_sqp.hip ----
    int sqp_globalization, sqp_use_suff, sqp_full_step_dual;   // globalization: 0 FIXED_STEP, 1 MERIT_BACKTRACKING
    double sqp_alpha_min, sqp_alpha_red, sqp_eps, sqp_tol[4];
    StateBuf<double> Wd;                     // (N,12,12) then W_e (8,8): the merit function evaluates the cost from the weights themselves
    StateBuf<double> st_lb, st_ub;           // the stage table (described at slot_lb above)
    // allocated together by the first SQP solve (api.hip: sqp_buffers): the iterate the QP was built at, merit weights, per-solve bookkeeping
    WorkBuf<double> ls_x, ls_u, ls_pi, ls_lam, ls_slk, ls_wpi, ls_wlam, ls_alpha;
    WorkBuf<double> ls_merit;               // (B,4) merit values of the last line search (ihm2mpc_get_sqp_merit; sqp_body.hpp: LsArgs.merit)
    WorkBuf<int32_t> ls_done, ls_status, ls_iter, ls_qp_acc;
    WorkBuf<int32_t> ls_pending;            // (B) instances whose line search goes past the first rollouts (two-launch ladder)
    // The three argument blocks (ls_args, step_args, sens_args) are workspace that is never poisoned: they hold pointers, counts and loop
    // bounds in the storage of doubles, so an early read would be an address, not arithmetic (api.hip: POISONABLE leaves them out)
    WorkBuf<double> ls_args;                // device copy of the line search's argument block for the persistent loop (512 B)
    WorkBuf<double> step_args;              // device copy of the persistent loop's own argument block (384 B), allocated with the handle
    void *args_host[2];             // pinned staging of both blocks (1 KB each), used alternately
    hipEvent_t args_ev[2];          // recorded after a slot's upload: the slot is free again once it has passed
    int args_idx;

    // ---- per-instance tuning (ihm2mpc_set_instance_weights / _bounds): allocated while the mode is on ----
    // Weights: one stage weight and one terminal weight per instance, expanded on the host by the code of ihm2mpc_set_weights.
    // Bounds: the VALUES of the rows 0..11 per instance; which sides are finite or soft stays batch-shared (the slot table's pattern).
    bool inst_w, inst_b;
    bool inst_b_ok;                // false: a later setter changed the shared pattern and the stored values no longer fit it
    bool shared_uniform_H;         // uniform_H of the batch-shared weights (restored when the per-instance weights go)
    StateBuf<double> iHs, iGy, iWd;          // (B,2,100) stage, terminal | (B,2,120) | (B,144+64): the layouts of Hs, Gy, Wd with one stage
    std::vector<double> ih_lb, ih_ub;      // host (B,NS,12) bounds of the rows 0..11, +-inf = absent
    StateBuf<double> i_slot_lb, i_slot_ub;   // (B,2,entries) the slot table per instance (either mode; the other's rows hold the shared values), grown on demand
    StateBuf<double> i_st_lb, i_st_ub;       // (B, NS*NC + NS*NLAM) the stage table per instance (either mode)
    StateBuf<double> i_lbu, i_ubu, i_lg, i_ug;   // (B,N,2) as given: the Stanley guess clamps to them
    // Slack penalties (ihm2mpc_set_instance_soft / _alat_soft): the VALUES z, Z per instance; which sides are soft stays batch-shared.
    // One mode for the kernels (inst_p: either entry is on); the rows an entry has not set hold the shared values in the tables above.
    bool inst_p;
    bool inst_p_ok;                // false: a later setter changed the shared pattern and the stored values no longer fit it
    std::vector<double> ih_sz, ih_sZ;      // host (B,NS,NLAM) penalties of the rows 0..13, empty: shared
    std::vector<double> ih_az, ih_aZ;      // host (B,2) penalties of the a_lat row, empty: shared
    ihm2_inst_penalties ip;                // the a_lat pairs' device copies (state; tests/test_instance_penalties_abi.py reads the struct's classes)
    // The same values from device memory (ihm2mpc_set_instance_soft_device / _alat_soft_device): the handle has no host copy of them.  The
    // device's own copy is what the cost reads anyway -- the penalty halves of i_st_* for the rows 0..13, ip for the a_lat pairs -- and
    // tables_to_device rebuilds the slot images from it (k_penalty_tables).  Per pair: 0 not set from device memory, 1 set, 2 set and a
    // shared setter changed afterwards which sides are soft: nothing can check the values against the new flags without a read-back, so
    // they count as not fitting.  dev_*_flags: which sides the shared rows held soft (sZ >= 0) when the pair was set
    int dev_sp, dev_ap;
    std::vector<char> dev_sp_flags, dev_ap_flags;
    bool inst_images;              // the per-instance images on the device are those of `slots` and of the values the handle holds: set at
                                   // the successful end of tables_to_device only, cleared when it starts and when `slots` is replaced
    bool host_p_fit;               // the penalties the host holds fit the shared pattern (tables_to_device; true where it holds none)
    ihm2_penalty_device_work pd;           // workspace of ihm2mpc_eval_adjoint_sensitivities_p_device

    // ---- history of ihm2mpc_run_steps, grown on demand ----
    WorkBuf<double> hist_u0, hist_x0;       // (steps,B,2), (steps,B,8)
    WorkBuf<int32_t> hist_st, hist_it;      // (steps,B)

    // ---- what was last launched (ihm2mpc_get_launch_record), written from the catalogue's keys (qp_select.hpp: encode_launch, note_lin, note_sim) ----
    int32_t launch_rec[16];

    // ---- x0 sensitivities of the last RTI QP (ihm2mpc_set_x0_sensitivities, kernels_sens.hip): allocated on first use ----
    int sens_mode;                  // 0 off, 1 the stage-0 gain, 2 the whole horizon
    int sens_state;                 // 0 nothing computed in this mode yet, 1 valid for the last solve / step, 2 the last step came from run_steps
    bool sens_quiet;                // run_steps' launches per step: no snapshot, no sensitivity launch (the persistent loop has none either)
    WorkBuf<double> sens_xbar, sens_ubar;   // (B,NS,8), (B,N,2) the point the last QP was linearised at
    WorkBuf<double> sens_u0;                // (B,2,8) du_0 / dx_0
    WorkBuf<double> sens_args;              // device copy of the persistent loop's SensArgs (512 B), allocated with the buffers above
    WorkBuf<double> sens_x, sens_u;         // (B,NS,8,8), (B,N,2,8) (mode 2)
    WorkBuf<double> hist_k;                 // (steps,B,2,8) du_0/dx0 of every step of ihm2mpc_run_steps_sens, grown on demand

    // ---- adjoint sensitivities (ihm2mpc_eval_adjoint_sensitivities, kernels_adj.hip): grown on demand to the largest n_seeds seen ----
    WorkBuf<double> adj_sx, adj_su;         // (B,n_seeds,NS,8), (B,n_seeds,N,2) seeds
    WorkBuf<double> adj_gx0, adj_gy, adj_gye;   // (B,n_seeds,8), (B,n_seeds,N,12), (B,n_seeds,8) gradients
    WorkBuf<double> adj_gW, adj_gWe;        // (B,n_seeds,12,12), (B,n_seeds,8,8) gradients in the weights (ihm2mpc_eval_adjoint_sensitivities_w)
};

// api.hip: what the selection reads of the handle -- the only function that turns a handle into a QpSituation.  Allocates nothing.
ihm2::QpSituation ihm2_situation(const ihm2mpc_handle *h);

// --- launchers (each defined in one .hip file) ---
// mode: bit 0 = reference ramp (needs x0), bit 1 = warm-start shift
void ihm2_launch_prepare(ihm2mpc_handle *h, double s_target, int mode, hipStream_t stream);
void ihm2_launch_build_tracks(ihm2mpc_handle *h, int max_seg, const int32_t *nseg, const double *cX, const double *cY, double *work);
void ihm2_launch_track_fit(ihm2mpc_handle *h, int max_pts, const int32_t *npts, const double *xy, double curv_weight, double *work, double *cX, double *cY,
                           int32_t *fail_flag);
void ihm2_launch_sim_dyn10(ihm2mpc_handle *h, int M, const double *x, const double *u, double *xn, hipStream_t stream);
void ihm2_launch_sim_dyn10_irk(ihm2mpc_handle *h, int integ, int M, int newton_iter, const double *x, const double *u, double *xn, hipStream_t stream);
void ihm2_launch_wrap_lap(ihm2mpc_handle *h);
void ihm2_launch_init_guess(ihm2mpc_handle *h, double v_ref_scale, int only_failed);
void ihm2_launch_linearize(ihm2mpc_handle *h);
// kernels_irk.hip: the collocation integrators (ihm2_is_irk of cfg.integrator_type / cfg.sim_integrator_type)
void ihm2_launch_linearize_irk(ihm2mpc_handle *h);
int ihm2_upload_sim_irk_tab(ihm2mpc_handle *h, int M_sim);      // 0 ok (h->sim_irk_tab holds the plant tableau for M_sim steps)
int ihm2_upload_irk_tab(ihm2mpc_handle *h);      // (re)builds h->irk_tab for the configured integrator and step; 0 ok
void ihm2_launch_rollout_irk(ihm2mpc_handle *h, int j_begin, int j_end, double *phi, const int32_t *pending);
void ihm2_launch_sim_irk(ihm2mpc_handle *h, int model, int M_sim, const double *x, const double *u, double *xn, hipStream_t stream,
                         const int32_t *active);
void ihm2_launch_copy_iterate(ihm2mpc_handle *h);   // x, u, pi, lam, slk -> ls_x, ls_u, ls_pi, ls_lam, ls_slk
void ihm2_launch_line_search(ihm2mpc_handle *h, int it, int last, int phase = 0, int j_limit = 0);
void ihm2_launch_sim(ihm2mpc_handle *h, int model, int M_sim, const double *x, const double *u, double *xn, hipStream_t stream,
                     const int32_t *active);
// kernels_simsens.hip: the plant step with forward sensitivities on `stream`; xn (B,8), Sx (B,8,8), Su (B,8,2), model_used (B) may each be
// nullptr, model_used not for the switched plants (model < 0), whose kernels run under it; 0 ok
int ihm2_launch_sim_sens(ihm2mpc_handle *h, int model, int M_sim, const double *x, const double *u, double *xn, double *Sx, double *Su,
                         int32_t *model_used, hipStream_t stream);
void ihm2_launch_sim_cart(ihm2mpc_handle *h, int model, int M, double dt, int n_steps, double v_dyn, const double *x, const double *u,
                          double *xn, hipStream_t stream);
void ihm2_launch_project(ihm2mpc_handle *h, double s_tol, const double *xc, double *s_guess, double *xf, hipStream_t stream);
// kernels_sens.hip: du/dx0, dx/dx0 of the last RTI QP's solution (h->sens_mode 1 or 2), after the QP on h->stream
void ihm2_launch_sens(ihm2mpc_handle *h);
size_t ihm2_sens_lds_bytes(const ihm2mpc_handle *h);
// kernels_adj.hip: the gradients of n_seeds scalar functions of that solution in x0, yref, yref_e into h->adj_gx0, adj_gy, adj_gye;
// seeds in device memory (nullptr = zero), unit_u0: the two unit seeds on u_0 instead; weights: also the gradients in W, W_e into
// h->adj_gW, adj_gWe (the other three are the same bits either way); zeta: with weights, also the adjoint solution into this device array
// (B,n_seeds,NS,10), nullptr = not kept (the five gradients are the same bits either way)
void ihm2_launch_adj(ihm2mpc_handle *h, int n_seeds, const double *seed_x, const double *seed_u, int unit_u0, int weights, double *zeta);
// kernels_cost.hip: the objective at the handle's (x, u) into cost (B), stage_cost (B,NS), slack_cost (B), each may be nullptr; grad: also
// its seeds dJ/dz into seed_x (B,NS,8), seed_u (B,N,2) and its explicit partials in yref, yref_e, W, W_e into ex_* ((B,N,12), (B,8),
// (B,12,12), (B,8,8); NaN for instances whose status is neither 0 nor 2).  The epilogue adds h->adj_gy, adj_gye, adj_gW, adj_gWe of one
// seed to ex_*, in place
void ihm2_launch_cost(ihm2mpc_handle *h, int grad, double *cost, double *stage_cost, double *slack_cost, double *seed_x, double *seed_u,
                      double *ex_yref, double *ex_yref_e, double *ex_W, double *ex_We);
void ihm2_launch_cost_epilogue(ihm2mpc_handle *h, double *ex_yref, double *ex_yref_e, double *ex_W, double *ex_We);
// kernels_slackseed.hip: seeds on the soft slacks folded onto seed_x (B,n_seeds,NS,8), seed_u (B,n_seeds,N,2) in place, before ihm2_launch_adj.
// cost: the slack terms' own dJ/ds (one seed, seed_s / seed_sa not read); else seed_s (B,n_seeds,NS,28), seed_sa (B,n_seeds,NS,2), nullptr = zero
void ihm2_launch_slack_fold(ihm2mpc_handle *h, int cost, int n_seeds, const double *seed_s, const double *seed_sa, double *seed_x, double *seed_u);
// kernels_penaltygrad.hip: the gradients in the slack penalties from the adjoint solution zeta (B,n_seeds,NS,10) that ihm2_launch_adj left
// behind the fold, into grad_z, grad_Z (B,n_seeds,NS,28) and grad_za, grad_Za (B,n_seeds,NS,2), all device memory.  cost: the slack seeds
// are the cost's own z + Z s and the explicit partials of J are added (one seed); else seed_s, seed_sa as the fold took them
void ihm2_launch_penalty_grad(ihm2mpc_handle *h, int cost, int n_seeds, const double *seed_s, const double *seed_sa, const double *zeta,
                              double *grad_z, double *grad_Z, double *grad_za, double *grad_Za);
// kernels_penalties.hip: the penalty halves of the per-instance images from z, Z in device memory on h->stream, the device twin of the
// penalty part of ihm2::table_images (qp_tables.hpp), bit for bit.  alat = 0: z, Z (B,NS,28), `src_stride` doubles from instance to
// instance -> zw | Zw of every slot of i_slot_lb / i_slot_ub but the a_lat row's and, with stage_out, z | Z of i_st_lb / i_st_ub; alat = 1:
// z, Z (B,2) -> the a_lat row's slots and, with stage_out, ip.alat_sz / alat_sZ.  The images and the shared slot table must be on the device
void ihm2_launch_penalty_tables(ihm2mpc_handle *h, int alat, const double *z, const double *Z, size_t src_stride, int stage_out);
// ihm2::find_penalty_mismatch of one pair on the device: code[b] = 0, or ihm2_penalty_code of instance b's first offence in its scan order
void ihm2_launch_penalty_check(ihm2mpc_handle *h, int alat, const double *z, const double *Z, int32_t *code);
// the kinds are ihm2::PenaltyMismatch::Kind's values; idx = stage * NLAM + side (the a_lat pair: 0 lower, 1 upper)
enum { ihm2_penalty_flag = 1, ihm2_penalty_negative = 2, ihm2_penalty_nan = 3, ihm2_penalty_none = 4 };
static inline __host__ __device__ int ihm2_penalty_code(int idx, int kind) { return 1 + idx * 4 + (kind - 1); }
// zeros into the four penalty gradients (device memory, any may be nullptr) of n_seeds seeds, NaN where the status is neither 0 nor 2
void ihm2_launch_penalty_fill(ihm2mpc_handle *h, int n_seeds, double *grad_z, double *grad_Z, double *grad_za, double *grad_Za);
// kernels_weights.hip: the per-instance weight tables from W (B,12,12), W_e (B,8,8) in device memory, on h->stream -- the device twin of
// ihm2::stage_weight_tables / terminal_weight_tables (qp_tables.hpp), bit for bit.  code == nullptr: writes Hs (B,2,100), Gy (B,2,120),
// Wd (B,208), every entry.  code (B) given: writes nothing but code[b], the validation of instance b (ihm2_weight_code_*; Hs, Gy, Wd unused)
void ihm2_launch_weight_tables(ihm2mpc_handle *h, const double *W, const double *W_e, double *Hs, double *Gy, double *Wd, int32_t *code);
// code[b]: 0 accepted; NAN_W + i: W[i/12][i%12] is NaN (the first such i); NAN_WE + i: W_e[i/8][i%8] is NaN; then the symmetry tests
enum { ihm2_weight_code_ok = 0, ihm2_weight_code_nan_W = 1, ihm2_weight_code_nan_We = 1 + 144, ihm2_weight_code_asym_stage = 1 + 208,
       ihm2_weight_code_asym_terminal = 2 + 208 };

// --- the kernels of kernels_qp.hip: the per-step QP (k_qp_wave, k_qp_block) and the persistent loop (k_steps) ---
// Their argument blocks, built by the launch code in api.hip.  (In the unnamed namespace, as the kernels that take them: the kernels'
// symbols name these types.)
namespace {

struct QpArgs {
    int B, N, iter_max, nslots, m_act;
    int nslots_can;     // entries of the 64-lane slot table: the order in which the slot sums (mu, mu_aff) are taken, whatever the number of waves per instance
    double tol, mu0, tau0;
    // shared
    // slot_lb, slot_ub: lb | zw and ub | Zw, the penalties nslots_can doubles behind the bounds.  unused_pad0, unused_pad1: read by nothing and
    // set to nullptr -- they keep the offsets of the members behind them, on which the compiler's grouping of the kernels' scalar loads depends
    // (without them the soft k_qp_wave instantiations change their instruction counts, NOTES.md R27)
    const double *Hs, *Gy, *CD, *slot_lb, *slot_ub, *unused_pad0, *unused_pad1;
    const int32_t *slot_kc;
    // per-instance tuning (api.hip: ihm2mpc_set_instance_weights / _bounds): doubles of Hs / Gy / slot_lb, slot_ub per instance (0: batch-shared)
    // and the offset of the terminal stage's Hs / Gy block (N * 100, N * 120 batch-shared; 100, 120 per instance: (B,2,100), (B,2,120))
    int hs_bs, hs_te, gy_bs, gy_te, sl_bs;
    // per instance
    double *x, *u;
    const double *x0, *yref, *yref_e;
    double *pi, *lam, *res, *qp_res, *u0;
    int32_t *status, *qp_iter;
    const double *lin;
    double *g, *rg, *P, *M, *slk;
    // track rows
    const int32_t *track_id;
    const double *widths;
    double car_L, car_W;
    // lateral-acceleration row (PATH == 2): its multipliers and slack values, (B, N+1, 2) = lower, upper side -- beside the 28 columns of the other rows
    double *lam_a, *slk_a;
    int symmetrize;     // P_k := (P_k + P_k') / 2 in the factor sweep (riccati_mfma.hpp): needed by the open-loop unstable dynamic model as written (fdyn6)
};

// x0 sensitivities (sens_body.hpp): k_sens takes the block by value, k_steps<..., SENS = 1> from device memory (StepArgs.sens)
struct SensArgs {
    int B, N, mode, nslots, path, alat;
    double tau;
    // stage Hessians: instance base stride, offset of the terminal block, stride between stages (0: one block for every k < N)
    const double *Hs;
    int hs_bs, hs_te, hs_ks;
    const double *CD;
    const int32_t *slot_kc;
    const double *slot_lb, *slot_ub, *unused_pad0, *unused_pad1;     // lb | zw and ub | Zw, and the padding, as QpArgs' (without it k_sens changes)
    int sl_bs;          // doubles of slot_lb / slot_ub per instance (0: batch-shared)
    const int32_t *track_id;
    const double *widths;
    double car_L, car_W;
    const double *lin, *xbar, *ubar, *x, *u, *lam, *slk, *lam_a, *slk_a;
    const int32_t *status;
    double *sens_u0, *sens_x, *sens_u;
    double *hist;       // (n_steps,B,2,8) du_0/dx0 of every step of the persistent loop, or nullptr (k_sens)
    int sweep_step;     // mode 2: the step whose solve the forward sweep differentiates (k_sens: 0, k_steps: the last)
};

struct StepArgs {
    int n_steps, model, M_sim, M, nknots, lap_wrap, freeze;
    int ocp_model;                          // the model of the shooting intervals (IHM2MPC_MODEL_FKIN6 / FDYN6 / FDYN6U); `model` is the plant's
    int sqp_iters;                          // 0: one RTI iteration per step; > 0: SQP mode, that many iterations with the line search
    double s_target, dt, lap_stop;
    const double *s_ref, *kappa_ref;
    double *x0, *yref, *yref_e, *lin;      // the same arrays as QpArgs', writable
    int32_t *active;                        // (B) or nullptr = all active
    double *hist_u0, *hist_x0;              // (n_steps,B,2), (n_steps,B,8) or nullptr
    int32_t *hist_st, *hist_it;             // (n_steps,B) or nullptr
    const ihm2::IrkTab *irk_tab;            // IRK = 1: the tableau of the shooting intervals' collocation step, in device memory
    const ihm2::IrkTab *sim_irk_tab;        // plant steps by collocation (python/main.py:395-400: Radau IIA x M_sim) instead of RK4 x M_sim; nullptr: RK4
    const SensArgs *sens;                   // SENS = 1: the x0 sensitivities' block in device memory (h->sens_args); nullptr otherwise
    // IRK = 2 (IHM2MPC_INTEG_ERK_LAG; behind the fields of the other loops, whose offsets stay): the lags' stage factors (LagFac) for the
    // shooting intervals' sub-step dt / M, then for the plant's dt / M_sim; sim_lag: the kinematic plant takes that integrator too (lane N)
    double lag[2][8];
    int sim_lag;
};

}  // namespace

// kernels_sens.hip: the SensArgs of the handle's x0 sensitivities into *out (hist = nullptr, sweep_step = 0: k_sens' own).  (Through a
// void pointer: a function with the unnamed namespace's type in its signature could not be defined in another translation unit.)
void ihm2_sens_args(const ihm2mpc_handle *h, void *out);

// The catalogue of their instantiations -- QpKey, QpInst, QpTable and the tables ihm2_qp_set0() .. ihm2_qp_set7() of the objects built from
// kernels_qp.hip -- is qp_catalogue.hpp's; qp_select.hpp (included above) chooses from it.
