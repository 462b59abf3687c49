/*
 * ihm2mpc.h -- C ABI of libihm2mpc.so: batched SQP-RTI solver for the ihm2 path-parametric
 * bicycle NMPC on AMD MI355X (gfx950).  Plain C: opaque handle, pointers and sizes only.
 *
 * This is the drop-in boundary for the reference's NMPC hot path.  Each entry point replaces an
 * acados call the reference makes (file:line relative to tudoroancea/ihm2):
 *
 *   ihm2mpc_create            <- AcadosOcpSolver(ocp, json_file=...)            python/mpc.py:111-113
 *                                ihm2_fkin6_acados_create_capsule/_create       src/ihm2/src/mpc_control_node.cpp:274-284
 *   ihm2mpc_free              <- ihm2_fkin6_acados_free/_free_capsule           mpc_control_node.cpp:398-412
 *   ihm2mpc_set_tracks        <- solver.set(i, "p", p) for all stages           python/main.py:249-252
 *                                ihm2_fkin6_acados_update_params                mpc_control_node.cpp:360-364
 *   ihm2mpc_set_weights       <- solver.cost_set(i, "W", W)                     python/main.py:253-295; mpc_control_node.cpp:287-293
 *   ihm2mpc_set_bounds        <- ocp.constraints.* / constraints_set(i,"lbx"..) python/mpc.py:79-99; dpc/main.py:226-227,259-261
 *   ihm2mpc_set_instance_weights <- solver_b.cost_set(i, "W", W_b), one solver per tuning  python/main.py:248-292
 *   ihm2mpc_set_instance_bounds  <- solver_b.constraints_set(i, "lbx".."ug", ..) per tuning python/main.py:248-292
 *   ihm2mpc_set_x0            <- solver.set(0,"lbx",x); set(0,"ubx",x)          python/main.py:299-300; mpc_control_node.cpp:177-179
 *   ihm2mpc_set_yref(_e)      <- solver.set(j,"yref",..)                        python/main.py:303-314; mpc_control_node.cpp:183-186
 *   ihm2mpc_set_x / _set_u    <- solver.set(j,"x"/"u",..) (warm start)          python/main.py:317-322
 *   ihm2mpc_prepare_step      <- the whole of python/main.py:303-322 on device (reference ramp + shift)
 *   ihm2mpc_solve             <- solver.solve()                                 python/main.py:325; mpc_control_node.cpp:189
 *   ihm2mpc_set_sqp_options   <- ocp.solver_options.globalization / alpha_min / ... / nlp_solver_tol_*   python/main.py:230-237
 *   ihm2mpc_get_sqp_stats     <- solver.get_stats("sqp_iter") / ("alpha") (acados)
 *   ihm2mpc_get_sqp_merit     <- (no acados call: the line search's merit values m(0), m(alpha), D, read back for its tests)
 *   ihm2mpc_get_x/_u/_u0      <- solver.get(i,"x"/"u")                        python/main.py:331-334; mpc_control_node.cpp:202-206
 *   ihm2mpc_get_status        <- return value of solve()                        python/main.py:325-328; dpc/main.py:287-293
 *   ihm2mpc_get_residuals     <- solver.get_stats("residuals") (acados)
 *   ihm2mpc_sim_step          <- AcadosSimSolver.simulate(x,u)                  python/main.py:476-502; python/sim.py:9-25
 *   ihm2mpc_sim_step_sens <- AcadosSimSolver.solve() with sens_forw; get("Sx" | "Su" | "S_forw")
 *   ihm2mpc_compute_control   <- IHM2Controller.compute_control(x) as one call            python/main.py:297-334
 *   ihm2mpc_step              <- one iteration of the MiL loop (plant + compute_control)  python/main.py:476-517
 *   ihm2mpc_run_steps         <- n iterations of that loop in one launch                  python/main.py:448-517
 *   ihm2mpc_set/get_x0_sensitivities <- solver.eval_param_sens(j, 0, "ex"); solver.get(k, "sens_x" / "sens_u") (acados)
 *   ihm2mpc_run_steps_sens    <- the same after every solve of ihm2mpc_run_steps' loop
 *   ihm2mpc_eval_adjoint_sensitivities <- solver.eval_adjoint_solution_sensitivity(seed_x, seed_u) (acados)
 *   ihm2mpc_eval_adjoint_sensitivities_w <- the same, and the gradients in the cost weights W, W_e (acados has no counterpart: one
 *                                           re-solve per weight entry and direction)
 *   ihm2mpc_eval_cost         <- solver.get_cost() (acados), stage terms scaled by cost_scale_stage
 *   ihm2mpc_eval_cost_gradient <- solver.eval_and_get_optimal_value_gradient("initial_state") (acados), of the RTI step's cost, and the
 *                                 gradients of that cost in yref, yref_e, W, W_e
 *   ihm2mpc_eval_adjoint_sensitivities_s, ihm2mpc_eval_cost_gradient_soft <- the same two on tables with soft sides: seeds on the slacks
 *   ihm2mpc_eval_adjoint_sensitivities_p, ihm2mpc_eval_cost_gradient_penalties <- those two, and the gradients in the slack penalties
 *   ihm2mpc_set_soft          <- ocp.constraints.idxsbx/idxsg/idxsh, cost.zl..Zu         old/generate_acaods_interface.py:380-449
 *   ihm2mpc_set_path_constraints <- model.con_h_expr (track rows), constraints.lh/uh     old/generate_acaods_interface.py:191-212,411-449
 *   ihm2mpc_set_track_geometry, ihm2mpc_project <- Track(csv), Track::project + Frenet states
 *                                                   src/ihm2/src/common/tracks.cpp:132-288; mpc_control_node.cpp:142-157
 *   ihm2mpc_sim_step_cart     <- ihm2_kin6/dyn6_acados_sim_solve + switch + clamp        src/ihm2/src/sim_node.cpp:197-257
 *
 * Conventions
 *   x = (s, n, psi, v_x, v_y, r, T, delta), u = (u_T, u_delta)   (python/models.py:236-245)
 *   All host arrays are C-contiguous, instance-major: x (B,N+1,8), u (B,N,2), yref (B,N,12) ...
 *   Every setter copies in, every getter copies out; no caller pointer is kept after return.
 *   A handle owns its device memory and its HIP streams (one, plus a helper stream inside ihm2mpc_step); it is not thread-safe; distinct handles
 *   are independent (one per device for multi-GPU sharding).
 *   Return value: 0 = ok, < 0 = API misuse or HIP error (text in ihm2mpc_last_error()).
 *   Per-instance solver status (acados codes): 0 success, 1 NaN/failure, 2 max iterations (SQP
 *   mode), 3 min step, 4 QP failure.  The reference accepts {0, 2} (python/main.py:326).
 */
#ifndef IHM2MPC_H
#define IHM2MPC_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IHM2MPC_NX 8
#define IHM2MPC_NU 2
#define IHM2MPC_NY 12
#define IHM2MPC_NYE 8
#define IHM2MPC_NG 2
#define IHM2MPC_NLAM 28 /* multipliers per stage: lower (8 bx, 2 bu, 2 g, 2 h) then upper (8, 2, 2, 2) */
#define IHM2MPC_NMAX 128 /* structural limit; the QP kernel also needs <= 640 constraint slots (two-sided rows with a finite
                            side, soft sides count separately): N <= 79 with the reference's 8 rows per stage */

#define IHM2MPC_MODEL_FKIN6 0 /* python/models.py:232-307 */
#define IHM2MPC_MODEL_FDYN6 1 /* python/models.py:455-606 */
/* fdyn6 with every wheel's lateral force on its OWN slip angle.  The reference crosses them (F_lat_FL uses alpha_RR ...,
 * python/models.py:543-546, quirk Q3); as written the model is open-loop unstable (yaw eigenvalue +34 1/s at 10 m/s) */
#define IHM2MPC_MODEL_FDYN6U 2

/* interior-point step: fraction of the distance to the boundary a step may take (primal and dual step lengths separately).  Round 4 tried
 * 0.9999: -3.6 % iterations in the oracle's closed loop, but instances of the benchmark batch start to fail and GPU / oracle / the two compiler
 * schedulers drift apart on marginal QPs (six GPU tests); 0.995 stays (NOTES.md R4) */
#define IHM2MPC_IPM_STEP_FRACTION 0.995

#define IHM2MPC_SQP_RTI 0 /* old/generate.py:21 */
#define IHM2MPC_SQP 1     /* python/main.py:230 */
#define IHM2MPC_FIXED_STEP 0         /* full steps */
#define IHM2MPC_MERIT_BACKTRACKING 1 /* python/main.py:237 */

/* integrators (AcadosOcpOptions.integrator_type / collocation_type, AcadosSimOpts): ERK = classical RK4 x M sub-steps; IRK = 4-stage
 * collocation x M steps, 3 Newton iterations per step from K = 0 with a fresh Jacobian each (acados' defaults), forward
 * sensitivities by the implicit-function theorem; GL4 = GAUSS_LEGENDRE (acados' default, python/main.py:234-236), RADAU4 =
 * GAUSS_RADAU_IIA (python/main.py:395-400, python/sim.py:28-33).  Both NLP solver types run on either integrator (the live options of
 * python/main.py:227-238 are SQP + MERIT_BACKTRACKING + IRK); the persistent loop (ihm2mpc_run_steps in one launch) takes RK4 or IRK on the
 * shooting intervals (batch-shared tables for IRK) of the kinematic and the dynamic OCP models, with RK4 or Radau IIA plants, and falls back to
 * launches per step otherwise. */
#define IHM2MPC_INTEG_ERK 0
#define IHM2MPC_INTEG_IRK_GL4 1
#define IHM2MPC_INTEG_IRK_RADAU4 2
/* ERK_LAG: classical RK4 x M on the six vehicle states with the two actuator lags (T' = (u_T - T) / t_T, t_T = 1 ms; delta' likewise,
 * t_delta = 20 ms) taken in closed form -- a named deviation from acados' ERK.  RK4 needs 25 sub-steps per 50 ms
 * interval only to stay stable on the torque lag; the lags are linear and autonomous on a constant input, so one sub-step h = dt / M from
 * (v, a) = (x[0:6], x[6:8]) under u is
 *   a+ = u + (a - u) e,  e_i = exp(-h / t_i)                                   (exact)
 *   v+ = RK4 on f[0:6], stage j (c = 0, 1/2, 1/2, 1) evaluated at X = (v + c h K_prev[0:6], u + (a - u) E_s(j)),  s = (0, 1, 1, 2)
 * where the stage factors E_0, E_1, E_2 of a lag make Simpson's rule exact for the first three moments of its transient,
 * int_0^h t^j exp(-t / t_i) dt, j = 0, 1, 2 (ihm2mpc_lag_stage_factors; sampling the closed form at the stage times instead leaves Simpson
 * with h / 6 of a transient whose integral is t_T).  The record [A | B | b] is the exact derivative of this map, with the zero pattern of
 * RK4's.  Any M >= 1 is stable.  For the OCP: IHM2MPC_MODEL_FKIN6 with IHM2MPC_SQP_RTI; for the plants: model 0.
 * Error of one 50 ms interval against Radau at rtol 1e-13 (max over states of |err| / (1 + |ref|), 60 random states on fsds_competition_1):
 *                                                  rate-feasible inputs   random inputs
 *   RK4 x 25 (ERK, M = 25)                               4.0e-8              3.2e-6
 *   closed-form lags sampled at the stage times, M = 4   3.4e-5              5.4e-3
 *   ERK_LAG, M = 4                                       2.2e-6              2.4e-5
 *   ERK_LAG, M = 8                                       1.6e-6              1.8e-6 */
#define IHM2MPC_INTEG_ERK_LAG 3
#define IHM2MPC_IRK_NEWTON_ITER 3

typedef struct ihm2mpc_handle ihm2mpc_handle;

typedef struct ihm2mpc_config {
    int32_t batch;          /* B: independent MPC instances on this device */
    int32_t N;              /* shooting intervals (python/main.py:183: Nf = 40) */
    int32_t M;              /* integrator steps per interval (sim_method_num_steps): RK4 sub-steps, >= 18 at dt = 0.05 for stability (ERK);
                             * 1 for IRK (python/main.py:236); any number for ERK_LAG (4 gives sub-steps sized for the car) */
    int32_t model;          /* IHM2MPC_MODEL_* of the OCP */
    int32_t ntracks;        /* number of track tables */
    int32_t nknots;         /* knots per table (python/motion_planning.py:25,402-428: 3*500) */
    int32_t device;         /* HIP device ordinal */
    int32_t nlp_solver_type;     /* IHM2MPC_SQP_RTI or IHM2MPC_SQP */
    int32_t nlp_solver_max_iter; /* SQP mode: iterations per solve() (python/main.py:231) */
    int32_t ipm_iter_max;   /* interior-point iteration cap */
    double dt;              /* interval length (python/main.py:184) */
    double cost_scale_stage;/* factor on the stage cost terms (acados: the time step) */
    double ipm_tol;         /* relative tolerance of the QP solver */
    double ipm_mu0;         /* initial barrier parameter factor */
    double ipm_tau0;        /* initial slack floor */
    double nlp_tol;         /* SQP mode: KKT tolerance */
    int32_t integrator_type;     /* IHM2MPC_INTEG_* of the shooting intervals (python/main.py:234: "IRK"; old/generate.py:23: "ERK") */
    int32_t sim_integrator_type; /* IHM2MPC_INTEG_* of the plant steps (python/main.py:395-400: IRK, GAUSS_RADAU_IIA, 4 stages) */
} ihm2mpc_config;

const char *ihm2mpc_last_error(void);
const char *ihm2mpc_version(void);
/* Host only (no device is touched): the stage factors of IHM2MPC_INTEG_ERK_LAG for a lag with time constant tau and sub-steps of h,
 * out4 = (E_0, E_1, E_2, e).  With r = h / tau, e = exp(-r), m0 = tau (1 - e), m1 = tau^2 (1 - e (1 + r)), m2 = 2 tau^3 (1 - e (1 + r + r^2 / 2)):
 * E_1 = 6 (m1 / h^2 - m2 / h^3), E_2 = 12 m2 / h^3 - 6 m1 / h^2, E_0 = 6 m0 / h - 4 E_1 - E_2 -- evaluated with expm1 and, for r < 1, the
 * series of the 1 - e (...) terms.  h = 12.5 ms, tau = 1 ms: (0.37708781, 0.03225617, -0.02611426).  Non-zero: h or tau not positive and finite. */
int ihm2mpc_lag_stage_factors(double h, double tau, double *out4);

/* ---- handle lifetime ----
 * ihm2mpc_create reads two environment variables, so that one process can hold handles of either kind: IHM2MPC_BLOCK_QP (ihm2mpc_run_steps
 * below) and, for testing, IHM2MPC_POISON_WORKSPACE.  An output read before the call that forms it (the linearisation, the residuals, the
 * sensitivities, the histories ...) is not defined: the getter returns whatever the workspace holds, zeros on a fresh handle.
 * IHM2MPC_POISON_WORKSPACE=1 makes that visible: every workspace buffer of doubles is filled with NaN (0xFF bytes) instead of zeros when it is
 * allocated or regrown; a comma-separated list of buffer names (the handle's WorkBuf members in csrc/ihm2mpc_internal.h, "track_work" for the
 * work buffers of ihm2mpc_build_tracks / _fit_tracks) poisons only those; unset or 0: nothing changes.  State and problem data (iterates,
 * multipliers, u0, every uploaded table) are never poisoned. */
int ihm2mpc_create(const ihm2mpc_config *cfg, ihm2mpc_handle **out);
int ihm2mpc_free(ihm2mpc_handle *h);
int ihm2mpc_synchronize(ihm2mpc_handle *h);
/* the handle's hipStream_t, as void* (for callers that enqueue their own work behind a solve) */
int ihm2mpc_get_stream(ihm2mpc_handle *h, void **stream);

/* ---- problem data shared by the whole batch ---- */
int ihm2mpc_set_tracks(ihm2mpc_handle *h, const double *s_ref, const double *kappa_ref); /* (ntracks,nknots) each */
/* The same tables (and the centre-line geometry of ihm2mpc_set_track_geometry) built ON THE DEVICE from the cubic spline coefficients of
 * the centre lines -- python/motion_planning.py:139-289 (segment lengths on 100 points, uniform arc-length resampling, heading, curvature),
 * :345-399 (offline_motion_plan: heading offset -asin(l_R kappa), lap length) and :402-428 (three laps side by side): nknots = 3 x samples
 * per lap.  coeffs_X, coeffs_Y: (ntracks, max_seg, 4), segment j of track t in [c0, c1, c2, c3] of X(t) = c0 + c1 t + c2 t^2 + c3 t^3,
 * t in [0, 1]; nseg (ntracks): segments of each track (the rest of its rows is ignored).  The closed-spline fit that produces the
 * coefficients (python/motion_planning.py:28-124: one small equality-constrained least-squares problem per track): ihm2mpc_fit_tracks, or any host fit. */
int ihm2mpc_build_tracks(ihm2mpc_handle *h, int32_t max_seg, const int32_t *nseg, const double *coeffs_X, const double *coeffs_Y);
/* The closed cubic-spline fit itself ON THE DEVICE -- replaces fit_spline of python/motion_planning.py:28-124 (there: qpsolvers / proxqp on
 * min 1/2 p'Pp + q'p s.t. Ap = 0; here: its KKT system, one workgroup per track, sparse Gaussian elimination with partial pivoting).
 * xy (ntracks, max_pts, 2): centre-line points of every track, the first npts[t] rows used (closed path: the last point is NOT the first
 * again); curv_weight: weight of the curvature term (offline_motion_plan uses 2.0, :358); out coeffs_X, coeffs_Y (ntracks, max_pts, 4), host:
 * feed them to ihm2mpc_build_tracks; the rows past a track's npts[t] are returned as 0.  3 <= npts[t] <= max_pts <= 182.
 * A track's result depends on its own points, npts[t] and curv_weight only: not on its place in the batch, its neighbours or max_pts.
 * Centre lines that cannot be fitted: two CONSECUTIVE equal points (the closing chord from the last point to the first counts: a chord of
 * length 0 has no chord ratio) and any non-finite coordinate.  The elimination then runs out of usable pivots -- a NaN never wins the pivot
 * search -- and the call returns non-zero with "the spline fit of track %d is singular" for the first such track
 * (tests/test_gpu_track_shapes.py holds one line of each kind).  After a failure coeffs_X, coeffs_Y are undefined and the handle is as usable
 * as before.  A point repeated elsewhere along the line (a crossing) is an ordinary input. */
int ihm2mpc_fit_tracks(ihm2mpc_handle *h, int32_t max_pts, const int32_t *npts, const double *xy, double curv_weight, double *coeffs_X,
                       double *coeffs_Y);
/* read the tables back, (ntracks, nknots) each; any pointer may be NULL */
int ihm2mpc_get_tracks(ihm2mpc_handle *h, double *s_ref, double *kappa_ref, double *X_ref, double *Y_ref, double *phi_ref);
int ihm2mpc_set_track_id(ihm2mpc_handle *h, const int32_t *track_id);                     /* (B) */
int ihm2mpc_set_weights(ihm2mpc_handle *h, const double *W, const double *W_e);           /* (N,12,12), (8,8) */
/* lbx/ubx (N+1,8) [row 0 unused], lbu/ubu (N,2), C (N,2,8), D (N,2,2), lg/ug (N,2); +-inf = absent */
int ihm2mpc_set_bounds(ihm2mpc_handle *h, const double *lbx, const double *ubx, const double *lbu,
                       const double *ubu, const double *C, const double *D, const double *lg,
                       const double *ug);
/* Per-instance tuning: instance b carries its own weights and bound values; its results are those of a handle whose
 * batch-shared tables hold b's tuning, bit for bit.  NULL (all arguments) = batch-shared again.
 * Weights: W (B,12,12) for every stage k < N, W_e (B,8,8); needs stage-independent C, D; ihm2mpc_set_weights first.
 * Bounds: lbx/ubx (B,N+1,8) [row 0 unused], lbu/ubu (B,N,2), lg/ug (B,N,2); ihm2mpc_set_bounds first.  Which sides are
 * finite (|v| < 1e20) must match the batch-shared table; C, D, soft penalties, track rows and the a_lat row stay shared.
 * A later ihm2mpc_set_bounds / _set_soft / _set_path_constraints / _set_alat_constraint re-applies the stored values (or the
 * next solve refuses, if the pattern no longer matches).  Errors name the instance, stage and row. */
int ihm2mpc_set_instance_weights(ihm2mpc_handle *h, const double *W, const double *W_e);
int ihm2mpc_set_instance_bounds(ihm2mpc_handle *h, const double *lbx, const double *ubx, const double *lbu,
                                const double *ubu, const double *lg, const double *ug);
/* Slack penalties per instance: the VALUES z, Z of the soft sides; which sides are soft is the batch-shared pattern of
 * ihm2mpc_set_soft (ihm2mpc_set_alat_constraint for the a_lat row), which must have been called first.  A side must be soft
 * (Z >= 0) for an instance exactly where the shared table holds it soft, with z >= 0 and, as ihm2mpc_set_soft asks, z + Z > 0 there (z = Z = 0 is no penalty) and no NaN anywhere; what
 * an instance gives on a hard side is otherwise not read.  Everything that reads a penalty follows the instance: the QP (per step
 * and in the persistent loop), the SQP mode's merit, ihm2mpc_eval_cost and the gradients of ihm2mpc_eval_adjoint_sensitivities_s /
 * _p and ihm2mpc_eval_cost_gradient_soft / _penalties, whose rows are then each instance's own.  The bounds of the a_lat row, lh / uh
 * of the track rows, the track widths and C, D stay shared.  A later ihm2mpc_set_soft / _set_bounds / _set_path_constraints /
 * _set_alat_constraint re-applies the stored values (or the next solve refuses, if the pattern no longer matches).  Errors name the
 * instance, stage and side (0..13 lower, 14..27 upper sides, as the columns of soft_z).
 * (B,N+1,28) each, layout of ihm2mpc_set_soft per instance; NULL, NULL = batch-shared penalties again */
int ihm2mpc_set_instance_soft(ihm2mpc_handle *h, const double *soft_z, const double *soft_Z);
/* (B,2) each: lower / upper side of the a_lat row; NULL, NULL = shared again */
int ihm2mpc_set_instance_alat_soft(ihm2mpc_handle *h, const double *soft_z, const double *soft_Z);
/* SOFT constraint sides (AcadosOcpConstraints idxsbx / idxsbx_e / idxsg with AcadosOcpCost zl, zu, Zl, Zu --
 * declared by the reference's OCP class, python/mpc.py:58-90 uses hard sides only): soft_z, soft_Z (N+1,28) per
 * one-sided constraint, 14 lower sides [x(8) u(2) g(2) h(2)] then 14 upper sides.  A side with soft_Z >= 0 carries a
 * slack s >= 0 with cost soft_z*s + 1/2*soft_Z*s^2; soft_Z < 0 = hard.  NULL, NULL = all hard (the default). */
int ihm2mpc_set_soft(ihm2mpc_handle *h, const double *soft_z, const double *soft_Z);
/* Nonlinear track-boundary rows (model.con_h_expr / con_h_expr_e of old/generate_acaods_interface.py:191-212), rows 12
 * and 13 of the stages 1..N:
 *     h_R = n - 1/2 L sin|psi| + 1/2 W cos(psi) - w_R ,   h_L = -n + 1/2 L sin|psi| + 1/2 W cos(psi) - w_L ,
 * lh <= h <= uh (2 entries each; |bound| >= 1e20 = absent; the reference writes lh = -1e3, uh = 0, :411-449), linearised at
 * the iterate by every RTI step.  L, W = car length / width (python/constants.py:57-58); widths (ntracks,2) = (w_R, w_L),
 * constant along a track as the reference's motion plan tiles them (python/motion_planning.py:385-386).
 * enable = 0 removes the rows (the other arguments are then ignored and may be NULL). */
int ihm2mpc_set_path_constraints(ihm2mpc_handle *h, int32_t enable, double car_length, double car_width,
                                 const double *widths, const double *lh, const double *uh);
/* The lateral-acceleration row of the KINEMATIC model's nonlinear constraint set -- old/generate_acaods_interface.py:198-209
 * (`[right, left, T_dot, delta_dot] + ([] if is_dynamic else [a_lat])`), bounds :52-53, :424, :433 (-5 / +5 m/s^2), definition :266-271 and
 * old/scripts/gen_mpc.py:182-184, with the forces and the slip angle of python/models.py:255-263:
 *     a_lat = (-F_Rx sin(beta) + F_Fx sin(delta - beta)) / m + (v_x^2 + v_y^2) sin(beta) / l_R ,   a_lat_min <= a_lat(x_k) <= a_lat_max
 * on the stages 1..N-1 (x_0 is fixed; it is no terminal row: con_h_expr_e, :209-212), linearised at the iterate by every RTI step: a
 * fifteenth row of a stage, with non-zeros in (v_x, v_y, T, delta).  soft_z, soft_Z (2 each: lower side, upper side; NULL = hard): slack
 * penalties as ihm2mpc_set_soft (the reference softens every h row, :380-395).  Needs the kinematic OCP model, the track rows
 * (ihm2mpc_set_path_constraints enabled), SQP_RTI and stage-independent weights; ihm2mpc_run_steps then launches per step.
 * The row's multipliers and slack values do not change the 28-column layout of the other rows: (B,N+1,2) = (lower, upper) arrays of
 * their own, zeroed by ihm2mpc_set_multipliers(.., NULL) / ihm2mpc_set_slacks(NULL) like the others.
 * enable = 0 removes the row. */
int ihm2mpc_set_alat_constraint(ihm2mpc_handle *h, int32_t enable, double a_lat_min, double a_lat_max, const double *soft_z,
                                const double *soft_Z);
int ihm2mpc_set_alat_multipliers(ihm2mpc_handle *h, const double *lam, const double *slk); /* (B,N+1,2) each; NULL = zero */
int ihm2mpc_get_alat_multipliers(ihm2mpc_handle *h, double *lam, double *slk);             /* (B,N+1,2) each; either may be NULL */

/* ---- per-instance data ---- */
int ihm2mpc_set_x0(ihm2mpc_handle *h, const double *x0);         /* (B,8) */
int ihm2mpc_set_x(ihm2mpc_handle *h, const double *x);           /* (B,N+1,8) */
int ihm2mpc_set_u(ihm2mpc_handle *h, const double *u);           /* (B,N,2) */
int ihm2mpc_set_yref(ihm2mpc_handle *h, const double *yref);     /* (B,N,12) */
int ihm2mpc_set_yref_e(ihm2mpc_handle *h, const double *yref_e); /* (B,8) */
int ihm2mpc_set_multipliers(ihm2mpc_handle *h, const double *pi, const double *lam); /* (B,N+1,8), (B,N+1,28); NULL = zero */

/* one stage of one instance (the AcadosOcpSolver.set/get call shape); field is one of
 * "x","u","yref","yref_e","lbx","ubx" (stage 0 only: both set x0),"pi","lam" */
int ihm2mpc_set_stage(ihm2mpc_handle *h, int32_t instance, int32_t stage, const char *field,
                      const double *value, int32_t n);
int ihm2mpc_get_stage(ihm2mpc_handle *h, int32_t instance, int32_t stage, const char *field,
                      double *value, int32_t n);

/* ---- the hot path ---- */
/* initial guess: roll the model out from x0 under a Stanley-type feedback (python/main.py:99-163) */
int ihm2mpc_init_guess(ihm2mpc_handle *h, double v_ref_scale);
/* a fresh warm start for the instances whose last solve failed (status other than 0 and 2) only: a failed instance keeps
 * its iterate, which can keep it infeasible for ever; the reference stops its single loop instead
 * (python/main.py:326-328).  The rollout is the kinematic model's (fkin6, whatever the OCP's model) from the current x0, with the actuator
 * lags in closed form and sub-steps of at most 12.5 ms; pi, lam, the slacks and the a_lat row's multipliers and slacks of those instances
 * are zeroed.  Every other instance is left as it was.  Call between solve() and the next prepare_step(). */
int ihm2mpc_reinit_failed(ihm2mpc_handle *h, double v_ref_scale);
/* reference ramp yref_j = [s0 + s_target*j/N, 0..], yref_e = [s0 + s_target, 0..] from the current
 * x0, and warm-start shift of (x,u) -- python/main.py:303-322 -- entirely on device */
int ihm2mpc_prepare_step(ihm2mpc_handle *h, double s_target);
/* n_iter RTI iterations (n_iter <= 0: the configured nlp_solver_max_iter / 1 for SQP_RTI).
 * With nlp_solver_type IHM2MPC_SQP (python/main.py:230-237) every iteration first tests the four KKT residuals of the iterate
 * against the tolerances -- a converged instance gets status 0 and is left alone -- and the QP step is scaled by the line
 * search chosen with ihm2mpc_set_sqp_options; an instance still iterating after n_iter QPs gets status 2 (ACADOS_MAXITER),
 * a QP failure ends its solve with status 1 / 4.  get_qp_iter then reports the interior-point iterations of all its QPs. */
int ihm2mpc_solve(ihm2mpc_handle *h, int32_t n_iter);
/* SQP mode only.  globalization IHM2MPC_FIXED_STEP (default) or IHM2MPC_MERIT_BACKTRACKING: backtracking on the l1 merit
 * function  cost + sum w |dynamics defect| + sum w max(0, constraint violation)  with weights following the QP multipliers
 * (|mult|, then max(|mult|, (w + |mult|)/2)); trial steps alpha = 1, alpha_reduction, alpha_reduction^2, ... >= alpha_min,
 * accepted on plain decrease or, with use_sufficient_descent, on m(alpha) - m(0) <= eps_sufficient_descent alpha D;
 * full_step_dual keeps the QP multipliers instead of moving them by alpha.  tol (4): stat, eq, ineq, comp, NULL keeps the
 * current ones (cfg.nlp_tol for all four).  Defaults: 0.05, 0.7, 1e-4, 0, 0 -- acados' defaults. */
int ihm2mpc_set_sqp_options(ihm2mpc_handle *h, int32_t globalization, double alpha_min, double alpha_reduction,
                            double eps_sufficient_descent, int32_t use_sufficient_descent, int32_t full_step_dual,
                            const double *tol);
/* QP solves made (B) and the last step length (B) of the last SQP-mode solve; either pointer may be NULL */
int ihm2mpc_get_sqp_stats(ihm2mpc_handle *h, int32_t *sqp_iter, double *alpha);
/* m (B,4): the merit values of the last line search of the last SQP-mode solve -- [0] m(0), [1] m at the last trial step (the accepted
 * alpha; when no trial step passed and the step fell to alpha_min, the last one tried: the merit is not evaluated at alpha_min), [2] D
 * (0 without use_sufficient_descent), [3] the infeasibility part of m(0), sum w |..| + sum w max(0, ..).  Zeros for an instance that
 * ran no line search in that solve (converged at once, QP failure, IHM2MPC_FIXED_STEP). */
int ihm2mpc_get_sqp_merit(ihm2mpc_handle *h, double *m);
/* phases of solve(), exposed for parity tests and profiling */
int ihm2mpc_linearize(ihm2mpc_handle *h);
int ihm2mpc_get_linearization(ihm2mpc_handle *h, double *A, double *Bm, double *b); /* (B,N,8,8),(B,N,8,2),(B,N,8) */

int ihm2mpc_get_x(ihm2mpc_handle *h, double *x);
int ihm2mpc_get_u(ihm2mpc_handle *h, double *u);
int ihm2mpc_get_u0(ihm2mpc_handle *h, double *u0);              /* (B,2); 0 before the first solve: the plants of _step / _sim_advance / _run_steps read it */
int ihm2mpc_get_status(ihm2mpc_handle *h, int32_t *status);     /* (B) */
int ihm2mpc_get_qp_iter(ihm2mpc_handle *h, int32_t *qp_iter);   /* (B) */
int ihm2mpc_get_residuals(ihm2mpc_handle *h, double *res);      /* (B,4): stat, eq, ineq, comp */
/* (B,4): inf-norm KKT residuals of the QP (stationarity, dynamics, inequalities, complementarity) at the point the interior-point
 * iteration returned, each divided by the scale its tolerance is relative to: <= ipm_tol for status 0.  acados: the qp_res of
 * solver.get_stats("qp_res_*") / print_statistics() */
int ihm2mpc_get_qp_residuals(ihm2mpc_handle *h, double *res);
int ihm2mpc_get_multipliers(ihm2mpc_handle *h, double *pi, double *lam);
/* slack values the next SQP-mode solve starts from (its line search walks from them to the QP's); NULL = zeros */
int ihm2mpc_set_slacks(ihm2mpc_handle *h, const double *sl);     /* (B,N+1,28) */
int ihm2mpc_get_slacks(ihm2mpc_handle *h, double *sl);         /* (B,N+1,28) slack of each soft side after the last QP */
/* milliseconds of the last solve(): [0] total, [1] linearize, [2] qp+update (HIP events) */
int ihm2mpc_get_timings(ihm2mpc_handle *h, double *ms, int32_t n);
/* Which kernel instantiations the handle's launchers last launched, written by the launch sites themselves (host side, no device work).
 * rec (16 int32):
 *   [0] last per-step QP launch: 0 none yet, 1 k_qp_wave, 2 k_qp_block;  [1..4] its NSLOT, NSOFT, PATH, UNI
 *       (k_qp_block: NSLOT = slots per thread of its 256-lane table, NSOFT = PATH = 0)
 *   [5] last ihm2mpc_run_steps: 0 none yet, 1 one k_steps launch, 2 launches per step (ihm2mpc_step n_steps times);
 *       [6..12] the k_steps parameters NSLOT, NSOFT, PATH, UNI, SQP, IRK, DYN (0 when [5] != 1; IRK: 0 RK4, 1 collocation, 2 ERK_LAG);
 *       [13] why it went per step: 0 it did not, 1 the configuration has no k_steps instantiation, 2 the batch exceeds the resident limit
 *       [14] SENS: 1 the k_steps launch computed x0 sensitivities (ihm2mpc_run_steps_sens), 0 otherwise (0 when [5] != 1)
 *   [15] bits 0..3 the last linearisation launch (ihm2mpc_linearize, a solve, ihm2mpc_step): 0 none yet, 1 k_linearize, 2 k_linearize_dyn,
 *       3 k_linearize_cols, 4 k_linearize_irk, 5 k_linearize with the closed-form lags (ERK_LAG);  bits 4..7 the last plant launch
 *       (ihm2mpc_sim_step, ihm2mpc_sim_advance, ihm2mpc_step): 0 none yet, 1 k_sim_step_kin, 2 k_sim_step, 3 k_sim_irk, 4 k_sim_step_kin with
 *       the closed-form lags (ERK_LAG), 5 a plant step with sensitivities (ihm2mpc_sim_step_sens, ihm2mpc_sim_step_sens_device: the
 *       kernels of kernels_simsens.hip).  Launches inside k_steps are not recorded here.
 *       bits 8..9 the form of the factor sweep in the QP of [0], bits 12..13 in the k_steps launch of [5] (0 when [5] != 1): 0 the general
 *       form, 1 the straight-line stage with the run-time horizon, 2 the straight-line stage with the horizon compiled in (N = 40).  The
 *       forms give the same bits; a table without active rows and the model IHM2MPC_MODEL_FDYN6 take the general form, and so does every
 *       configuration without an instantiation in the other two.  IHM2MPC_QP_FORM in the environment (read once) limits the choice:
 *       1 keeps N = 40 on form 1, 0 keeps every launch on form 0.
 *       bit 10 the form of the slot phases in the QP of [0], bit 14 in the k_steps launch of [5] (0 when [5] != 1): 1 the full form -- for
 *       a table of 64 x 5 hard rows with both bounds finite (per instance too) and no track or a_lat row, at N = 40 on form 2 of the factor
 *       sweep: no validity or side test per slot -- 0 the general form.  The same bits again.  IHM2MPC_QP_FORM = 2 keeps N = 40 on form 2
 *       with the general slot phases; one infinite bound anywhere does the same. */
int ihm2mpc_get_launch_record(ihm2mpc_handle *h, int32_t *rec);

/* ---- sensitivities of the solution with respect to the initial state (acados: eval_param_sens(index, 0, "ex"), then
 * get(stage, "sens_x" | "sens_u")) ----
 * The last RTI QP of an instance, linearised at (xbar, ubar), differentiated at its returned solution: the interior point's KKT system
 * at that iterate with the primal gaps t = max(gap, IHM2MPC_SENS_TAU) in place of its own slacks -- every present side adds
 * sigma r r' to the stage Hessian (hard: lam / t; soft: the slack eliminated in series, 1 / (t / lam + 1 / (Z + nu / max(s, tau))),
 * nu = max(z + Z s - lam, 0)) -- solved as an equality-constrained LQ problem from dx_0 = e_j.  One kernel after the QP;
 * the QP and every other output are unchanged.
 * mode: 0 off (the default), 1 du_0/dx_0 only (the feedback gain K0 of u0 + K0 (x - x0)), 2 the whole horizon.  Memory on first use.
 * While the mode is on, ihm2mpc_solve, ihm2mpc_compute_control and ihm2mpc_step take a copy of (x, u) after the linearisation and
 * launch the kernel after the QP of their last RTI iteration, in stream order.  Refused in the SQP mode (the line search scales the step
 * and the multipliers: no QP solution is returned).  ihm2mpc_run_steps computes none (the persistent loop is unchanged);
 * ihm2mpc_run_steps_sens computes them at every step. */
#define IHM2MPC_SENS_TAU 1e-9
int ihm2mpc_set_x0_sensitivities(ihm2mpc_handle *h, int32_t mode);
/* sens_x (B,N+1,8,8): sens_x[b][k][i][j] = d x_k,i / d x0_j (mode 2 only; stage 0 is the identity); sens_u: mode 1 (B,2,8) =
 * d u_0 / d x0, mode 2 (B,N,2,8) = d u_k / d x0.  Either pointer may be NULL.  NaN for instances whose status is neither 0 nor 2.
 * Refused before a solve with the mode on and after ihm2mpc_run_steps (after ihm2mpc_run_steps_sens: the last step's). */
int ihm2mpc_get_x0_sensitivities(ihm2mpc_handle *h, double *sens_x, double *sens_u);
/* du_0 / dx0 (B,2,8) into device memory (either mode), stream-ordered like ihm2mpc_get_u0_device */
int ihm2mpc_get_sens_u0_device(ihm2mpc_handle *h, void *dptr);

/* ---- adjoint sensitivities of the same solution: the gradient of scalar functions of it with respect to the initial state and the
 * reference (acados: eval_adjoint_solution_sensitivity(seed_x, seed_u)) ----
 * With M = [[Ht, E'], [E, 0]] the KKT matrix of the x0 sensitivities above (Ht_k = H_k + sum_i sigma_i r_i r_i', E the rows x_0 = . ,
 * x_{k+1} - A_k x_k - B_k u_k = .) a change of the stage gradients and of the initial state moves the solution by
 * M [dz; dpi] = [-dg; (dx0, 0, ..)].  For a seed s_k = dL/dz_k (seed_x[k] on x_k, seed_u[k] on u_k) let [zeta; nu] = M^-1 [s; 0]; then,
 * since g_k = H_k z_k - Gy_k yref_k,
 *     dL/dx0 = nu_0,     dL/dyref_k = Gy_k' zeta_k  (k < N),     dL/dyref_e = Gy_N' zeta_N[0:8]
 * -- one backward and one forward vector sweep on the factorisation of the x0 sensitivities (backward: l_x = -s_x + A_k' p_{k+1},
 * l_u = -s_u + B_k' p_{k+1}, kappa_k = -Quu_k^-1 l_u, p_k = l_x + K_k' l_u, p_N = -s_x,N; forward from zeta_x,0 = 0: zeta_u,k = K_k zeta_x,k
 * + kappa_k, zeta_x,k+1 = A_k zeta_x,k + B_k zeta_u,k; nu_0 = -p_0), for up to eight seeds in one launch of one kernel.
 * n_seeds: 1..8.  seed_x (B,n_seeds,N+1,8), seed_u (B,n_seeds,N,2), host arrays; either may be NULL (= zero).  Both NULL, with
 * n_seeds == 2: the two unit seeds on u_0 -- grad_x0 is then du_0/dx0 (the rows of K0) and grad_yref / grad_yref_e are du_0/dyref,
 * du_0/dyref_e.  Outputs, any may be NULL: grad_x0 (B,n_seeds,8), grad_yref (B,n_seeds,N,12), grad_yref_e (B,n_seeds,8); NaN for
 * instances whose status is neither 0 nor 2.  Per-instance weights and bounds are honoured.
 * Differentiates the last RTI solve (after ihm2mpc_run_steps_sens: the last step's) and needs x0 sensitivity mode 1 or 2 to have been on
 * for it, which is what keeps the point of linearisation.  Refused while the mode is off, before a solve with the mode on, after
 * ihm2mpc_run_steps, in the SQP mode, for n_seeds outside 1..8 and for both seeds NULL with n_seeds != 2.  The call reads the iterate,
 * the multipliers, the slacks, the reference tables and the bounds as that solve left them: it must follow the solve directly -- after
 * ihm2mpc_prepare_step, a setter of x, u, the multipliers, the slacks, weights or bounds, ihm2mpc_init_guess or ihm2mpc_reinit_failed it
 * would differentiate a mixture, which is not detected.  It changes no other output and may be called any number of times (a caller may
 * evaluate several batches of seeds against one solve).  Blocking: the seeds may be reused and the gradients read on return. */
int ihm2mpc_eval_adjoint_sensitivities(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u,
                                       double *grad_x0, double *grad_yref, double *grad_yref_e);
/* The same call with the gradients in the cost weights: a superset of ihm2mpc_eval_adjoint_sensitivities -- grad_x0, grad_yref and
 * grad_yref_e are the same bits -- with two more outputs.  The QP's stationarity row of stage k < N reads
 * H_k dz_k + g_k = c_s V' W_k (V z+_k - yref_k), with z+ the returned solution (ihm2mpc_get_x / _get_u after the solve), c_s the
 * configuration's cost_scale_stage and V the 12 x 10 output selector y = (x, u, x[6:8] - u); the terminal row reads W_e (x+_N - yref_e).
 * A change dW moves the stage's row by c_s V' dW e_k, e_k = V z+_k - yref_k, so with zeta of the seed as above
 *     grad_W = -c_s sum_{k<N} sym((V zeta_k) e_k')  (12,12),     grad_W_e = -sym(zeta_N[0:8] (x+_N - yref_e)')  (8,8),
 * sym(X) = (X + X') / 2: the gradients on the space of symmetric matrices (the weight setters refuse any other), i.e.
 * dL = <grad_W, dW> + <grad_W_e, dW_e> for every symmetric direction, and for diagonal weights dL/dq_i is the diagonal entry.
 * grad_W is the derivative in a change common to all stages k < N: exact for per-instance weights (ihm2mpc_set_instance_weights, one W
 * for every stage) and for a stage-independent shared table; for a stage-dependent shared table it is the derivative in a common shift
 * of all stages (there is no per-stage output).  Bounds are not differentiated: dL/dbound_i = sigma_i r_i' zeta, and on an active hard
 * side sigma_i = lam / max(gap, IHM2MPC_SENS_TAU) reaches 1e13 while r_i' zeta is of the order 1 / sigma_i out of a sweep whose absolute
 * error is about 1e-16 of its scale -- the product has no accuracy that could be stated in advance.
 * Outputs, any may be NULL: the three of ihm2mpc_eval_adjoint_sensitivities, grad_W (B,n_seeds,12,12), grad_W_e (B,n_seeds,8,8), both
 * exactly symmetric; NaN for instances whose status is neither 0 nor 2.  Per-instance weights and bounds are honoured (e_k does not
 * depend on W).  Both seeds NULL with n_seeds == 2: the two unit seeds on u_0, grad_W = du_0/dW.  Same preconditions and refusals as
 * ihm2mpc_eval_adjoint_sensitivities: x0 sensitivity mode 1 or 2 on for the solve; refused while the mode is off, before a solve with the
 * mode on, after ihm2mpc_run_steps (after ihm2mpc_run_steps_sens: the last step's), in the SQP mode, for n_seeds outside 1..8 and for
 * both seeds NULL with n_seeds != 2.  It also reads yref and yref_e as the solve read them: it must follow the solve directly.  Memory
 * for the two outputs on first use.  It changes no other output, those of ihm2mpc_eval_adjoint_sensitivities included.  Blocking. */
int ihm2mpc_eval_adjoint_sensitivities_w(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u,
                                         double *grad_x0, double *grad_yref, double *grad_yref_e,
                                         double *grad_W, double *grad_W_e);   /* (B,n_seeds,12,12), (B,n_seeds,8,8) */
/* The same call with seeds on the soft slacks: L may also depend on the slack values s_i of ihm2mpc_get_slacks (seed_s (B,n_seeds,N+1,28)
 * = dL/ds_i, 14 lower sides then 14 upper sides per stage) and on those of the lateral-acceleration row (seed_sa (B,n_seeds,N+1,2),
 * lower, upper; ihm2mpc_get_alat_multipliers).  The system above has every soft slack eliminated in series; with the slack kept, its row
 * reads (lam_i / t_i) (s + sgn_i r_i z) + rho_i s = c_i for a seed c_i, and eliminating it moves the right-hand side:
 *     seed_z,k  <-  seed_z,k - sum over the soft sides i of stage k with lam_i > 0 of  c_i gamma_i sgn_i r_i,
 *     gamma_i = lam_i / (t_i rho_i + lam_i),   sgn_i = +1 on a lower side and -1 on an upper side
 * (gamma_i = sigma_i / rho_i: the share of a move of the row that the slack takes; 1 for rho_i = 0).  One more kernel folds the slack
 * seeds onto seed_x / seed_u in device memory; everything behind it is ihm2mpc_eval_adjoint_sensitivities_w, unchanged.  A seed on a side
 * without a slack -- a hard side, or one with no finite bound -- is ignored, as is one on a side whose multiplier is zero.  Any of the
 * four seeds may be NULL (= zero); all four NULL with n_seeds == 2: the two unit seeds on u_0.  With seed_s and seed_sa NULL no fold
 * runs and the outputs are the bits of ihm2mpc_eval_adjoint_sensitivities_w.  Outputs, preconditions, refusals and NaN rows are that
 * entry's; instances whose status is neither 0 nor 2 are not folded.  Gradients in the soft penalties are those of
 * ihm2mpc_eval_adjoint_sensitivities_p; gradients in the bounds are not computed.  Blocking. */
int ihm2mpc_eval_adjoint_sensitivities_s(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u,
                                         const double *seed_s, const double *seed_sa,
                                         double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W, double *grad_W_e);
/* The same call with the gradients in the slack penalties z_i, Z_i of ihm2mpc_set_soft (grad_z, grad_Z, in the layout of
 * ihm2mpc_get_slacks) and of the two sides of the lateral-acceleration row (grad_za, grad_Za: lower, upper).  The slack's row above
 * linearises its stationarity z_i + Z_i s_i - lam_i - nu_i = 0, which a change of the penalties moves by dz_i + s_i dZ_i.  With zeta_k the
 * adjoint solution of stage k on the folded seeds, c_i the seed on the slack (zero where none is given) and s_i the slack value after the
 * solve,
 *     zeta_s,i = (c_i t_i - lam_i sgn_i r_i zeta_k) / (t_i rho_i + lam_i),      dL/dz_i = -zeta_s,i,      dL/dZ_i = -s_i zeta_s,i
 * (= (c_i - w_i sgn_i r_i zeta_k) / (w_i + rho_i) with w_i = lam_i / t_i, which is never formed; sgn_i = +1 on a lower and -1 on an
 * upper side).  A side whose multiplier is not positive (lam_i = 0) is dropped, as the fold drops it: both gradients are 0 -- there
 * rho_i >= nu_i / tau, so what is dropped is at most |c_i| tau / z_i.  A side without a slack -- hard, or with no finite bound -- has
 * both gradients 0, not NaN, so that the gradients can be summed over the batch for the shared table.  zeta (B,n_seeds,N+1,10), may be
 * NULL: the adjoint solution itself, (zeta_x,k, zeta_u,k) per stage, zeros on the input part of row N.  The first five gradients are
 * the bits of ihm2mpc_eval_adjoint_sensitivities_s for the same seeds; on a handle without a soft side the four new gradients are
 * zeros.  Every output may be NULL; instances whose status is neither 0 nor 2 get NaN in all of them.  Arguments, preconditions and
 * refusals are that entry's.  The memory of the new outputs lives for the call only.  Bounds stay undifferentiated: a gradient in a
 * bound would carry lam_i / t_i itself.  Blocking. */
int ihm2mpc_eval_adjoint_sensitivities_p(ihm2mpc_handle *h, int32_t n_seeds, const double *seed_x, const double *seed_u,
                                         const double *seed_s, const double *seed_sa,
                                         double *grad_x0, double *grad_yref, double *grad_yref_e, double *grad_W, double *grad_W_e,
                                         double *grad_z, double *grad_Z,      /* (B,n_seeds,N+1,28) each */
                                         double *grad_za, double *grad_Za,    /* (B,n_seeds,N+1,2) each */
                                         double *zeta);                       /* (B,n_seeds,N+1,10), may be NULL */

/* ---- the objective and its total gradient (kernels_cost.hip) ----
 * The objective at the handle's current (x, u) -- after a solve the returned solution z+ -- as acados documents get_cost, stage terms
 * scaled by cost_scale_stage:
 *     J = sum_{k<N} (c_s/2) e_k' W_k e_k + 1/2 e_N' W_e e_N + J_slack,     J_slack = sum over the soft sides of z_i s_i + 1/2 Z_i s_i^2
 * with e_k = V z_k - yref_k (k < N), e_N = x_N - yref_e, V the 12 x 10 selector y = (x, u, x[6:8] - u), c_s the configuration's
 * cost_scale_stage, W_k the weights as set (per-instance weights are honoured), s_i the slack values of ihm2mpc_get_slacks (and of
 * ihm2mpc_get_alat_multipliers for the lateral-acceleration row), z_i, Z_i the penalties of ihm2mpc_set_soft /
 * ihm2mpc_set_alat_constraint: what the merit function of the SQP mode sums at the full step.
 * Outputs, any may be NULL: cost (B); stage_cost (B,N+1), the terms of the stages with their slack terms (cost is their sum);
 * slack_cost (B) = J_slack.  Works on any ready handle at any time -- both solver modes, soft tables, the lateral-acceleration row,
 * after ihm2mpc_init_guess, after ihm2mpc_run_steps -- and for every status; it reads state only and changes no output.  Every sum is
 * taken in a fixed order: the value does not depend on the batch.  Blocking. */
int ihm2mpc_eval_cost(ihm2mpc_handle *h, double *cost, double *stage_cost, double *slack_cost);
/* The cost and its total derivative through the QP-solution map that ihm2mpc_eval_adjoint_sensitivities differentiates.  With
 * t_k = W_k e_k the seeds dJ/dz_k, in the layout of ihm2mpc_eval_adjoint_sensitivities with n_seeds = 1, are
 *     seed_z,k = c_s V' t_k  (k < N):  seed_x,k = c_s (t[0:8] + (0,..,0, t[10], t[11])),  seed_u,k = c_s (t[8:10] - t[10:12]);   seed_x,N = W_e e_N
 * and with grad_* the outputs of ihm2mpc_eval_adjoint_sensitivities_w for those seeds
 *     dJ/dx0 = grad_x0,     dJ/dyref_k = grad_yref_k - c_s t_k,     dJ/dyref_e = grad_yref_e - W_e e_N,
 *     dJ/dW = grad_W + (c_s/2) sum_{k<N} e_k e_k',     dJ/dW_e = grad_W_e + 1/2 e_N e_N'
 * -- the explicit partials of J added to the part that reaches J through the solution.  dJ/dW is the derivative in a change common to
 * all stages, as grad_W is; dJ/dW and dJ/dW_e are exactly symmetric.  This is the derivative of the cost of the RTI step's solution, not of
 * a converged NLP's optimal value (acados: eval_and_get_optimal_value_gradient differentiates the latter); bounds are not differentiated.
 * The kernel writes the seeds into the adjoint entries' device buffers, the adjoint kernel runs on them and one more kernel adds the
 * explicit partials: no host round trip.  Outputs, any may be NULL: cost (B), grad_x0 (B,8), grad_yref (B,N,12), grad_yref_e (B,8),
 * grad_W (B,12,12), grad_W_e (B,8,8), seed_x (B,N+1,8), seed_u (B,N,2); the five gradients are NaN for instances whose status is
 * neither 0 nor 2, cost and the seeds are plain evaluations and stay finite.  Same preconditions and refusals as
 * ihm2mpc_eval_adjoint_sensitivities: x0 sensitivity mode 1 or 2 on for the solve; refused while the mode is off, before a solve with the
 * mode on, after ihm2mpc_run_steps (after ihm2mpc_run_steps_sens: the last step's) and in the SQP mode; it must follow the solve directly.
 * Refused on a handle with a soft side: J_slack depends on slacks that the adjoint system has eliminated and that carry no seed, so
 * the gradient is defined for all-hard tables only (ihm2mpc_eval_cost takes every table; ihm2mpc_eval_cost_gradient_soft gives the
 * slacks their seed and takes every table).  It changes no other output, but overwrites
 * the seed and gradient buffers of the adjoint entries, as every call of those does.  Blocking. */
int ihm2mpc_eval_cost_gradient(ihm2mpc_handle *h, double *cost, double *grad_x0, double *grad_yref, double *grad_yref_e,
                               double *grad_W, double *grad_W_e, double *seed_x, double *seed_u);
/* ihm2mpc_eval_cost_gradient on every constraint table.  On a table with a soft side J_slack depends on the slacks, whose seed
 * c_i = dJ_slack/ds_i = z_i + Z_i s_i is folded onto the stage seeds as ihm2mpc_eval_adjoint_sensitivities_s folds seed_s, between the
 * cost kernel and the adjoint; x0, yref and the weights do not enter a slack's row, so the explicit partials are those above.  seed_x and
 * seed_u come back as the seeds the adjoint saw, after the fold: the five gradients are those of ihm2mpc_eval_adjoint_sensitivities_w for
 * them plus the explicit partials.  On a handle without a soft side no fold runs and every output is the bits of
 * ihm2mpc_eval_cost_gradient.  Same arguments, shapes, preconditions, refusals (but the soft-side one) and NaN rows.  Blocking. */
int ihm2mpc_eval_cost_gradient_soft(ihm2mpc_handle *h, double *cost, double *grad_x0, double *grad_yref, double *grad_yref_e,
                                    double *grad_W, double *grad_W_e, double *seed_x, double *seed_u);
/* ihm2mpc_eval_cost_gradient_soft with the total derivative of the cost in the slack penalties: the gradients of
 * ihm2mpc_eval_adjoint_sensitivities_p for the cost's seeds (c_i = z_i + Z_i s_i) plus the explicit partials of J_slack,
 *     dJ/dz_i = s_i - zeta_s,i,      dJ/dZ_i = s_i^2 / 2 - s_i zeta_s,i
 * into grad_z, grad_Z (B,N+1,28) and grad_za, grad_Za (B,N+1,2), any may be NULL; 0 on a side without a slack or with lam_i = 0, NaN for
 * instances whose status is neither 0 nor 2, zeros on a handle without a soft side.  Every other output is the bits of
 * ihm2mpc_eval_cost_gradient_soft.  Bounds stay undifferentiated.  Blocking. */
int ihm2mpc_eval_cost_gradient_penalties(ihm2mpc_handle *h, double *cost, double *grad_x0, double *grad_yref, double *grad_yref_e,
                                         double *grad_W, double *grad_W_e, double *grad_z, double *grad_Z, double *grad_za,
                                         double *grad_Za, double *seed_x, double *seed_u);

/* ---- device-pointer variants (zero-copy closed loop, RCCL gather of results) ----
 * dptr is device memory on the handle's device, SAME (instance-major) layout as the host variant */
int ihm2mpc_set_x0_device(ihm2mpc_handle *h, const void *dptr);
int ihm2mpc_get_u0_device(ihm2mpc_handle *h, void *dptr);
int ihm2mpc_get_x_device(ihm2mpc_handle *h, void *dptr);
int ihm2mpc_get_u_device(ihm2mpc_handle *h, void *dptr);
int ihm2mpc_get_status_device(ihm2mpc_handle *h, void *dptr);
/* ---- device-resident parameters in, gradients out (a learning loop around the RTI step: ihm2_amd/torch_layer.py) ----
 * All five are stream-ordered on the handle's stream like ihm2mpc_get_u0_device and do not block unless stated.
 *   ihm2mpc_set_yref_device / _set_yref_e_device <- ihm2mpc_set_yref / _set_yref_e: (B,N,12) / (B,8), device-to-device into the same buffers. */
int ihm2mpc_set_yref_device(ihm2mpc_handle *h, const void *yref);
int ihm2mpc_set_yref_e_device(ihm2mpc_handle *h, const void *yref_e);
/*   ihm2mpc_set_instance_weights_device <- ihm2mpc_set_instance_weights with W (B,12,12), W_e (B,8,8) in device memory: the tables
 * c_s V'WV, c_s V'W, the terminal blocks and the copy [W | W_e] are expanded by one kernel (k_weight_tables), bit for bit what the host
 * setter uploads.  Same preconditions and refusal texts: ihm2mpc_set_weights first, stage-independent C, D, both pointers or both NULL
 * (NULL, NULL = the batch-shared weights again).  check != 0: validated as the host setter validates -- no NaN entry, both expanded
 * Hessians symmetric to |a - b| <= 1e-12 (1 + |a|) -- and refused with the host setter's message for the first offending instance; this
 * reads one int32 per instance back and BLOCKS; on a refusal the handle's tables and mode are untouched.  check == 0: nothing is read
 * back and the call does not block -- THE CALLER VOUCHES for symmetric weights without NaN: nothing validates them; a NaN weight then
 * surfaces as QP status 1 of that instance (its documented meaning), an asymmetric one gives a QP that is not the one asked for.
 * W and W_e are read in stream order: keep them alive and unchanged until the stream has passed.  Memory for the tables on first use. */
int ihm2mpc_set_instance_weights_device(ihm2mpc_handle *h, const void *W, const void *W_e, int32_t check);
/* The expanded per-instance tables as the QP reads them, to host arrays: Hs (B,2,10,10) stage then terminal, Gy (B,2,10,12), Wd (B,208)
 * = [W | W_e]; any may be NULL.  Blocking.  Refused while the per-instance weights are off.  (For comparing the two setters entry for
 * entry: a comparison through solves cannot tell -0.0 from 0.0.) */
int ihm2mpc_get_instance_weight_tables(ihm2mpc_handle *h, double *Hs, double *Gy, double *Wd);
/*   ihm2mpc_eval_adjoint_sensitivities_w_device <- ihm2mpc_eval_adjoint_sensitivities_w with seeds and gradients in device memory: same
 * shapes, NULL rules (either seed NULL = zero; both NULL with n_seeds == 2 = the unit seeds on u_0; any output NULL = skipped), NaN rows,
 * preconditions and refusal texts, same bits.  The kernel reads the seeds straight from the caller's memory and the gradients reach the
 * caller's memory in stream order: no host copy, no wait.  THE CALLER KEEPS the seeds alive and unchanged, and the outputs alive, until
 * the stream has passed the call (ihm2mpc_synchronize, or an event on ihm2mpc_get_stream).  Memory for the gradients on first use and
 * when n_seeds grows.
 * Not offered with device pointers: the cost-gradient entries (ihm2mpc_eval_cost_gradient*), the persistent loop (ihm2mpc_run_steps*)
 * and the SQP mode. */
int ihm2mpc_eval_adjoint_sensitivities_w_device(ihm2mpc_handle *h, int32_t n_seeds, const void *seed_x, const void *seed_u,
                                                void *grad_x0, void *grad_yref, void *grad_yref_e, void *grad_W, void *grad_W_e);
/* ---- the penalty side of the same loop: slack penalties in, slack values out, penalty gradients back ----
 *   ihm2mpc_set_instance_soft_device / _set_instance_alat_soft_device <- ihm2mpc_set_instance_soft / _set_instance_alat_soft with soft_z,
 * soft_Z (B,N+1,28) / (B,2) in device memory.  One kernel (k_penalty_tables) writes the penalty halves of the per-instance constraint
 * tables -- the slots' zw | Zw, the (stage, side) z | Z, the a_lat pairs -- bit for bit what the host setter uploads: the instance's
 * values on the soft slots, the side the slot's finite bound names, the a_lat row's slots from the a_lat pair, the shared values on hard
 * slots and padding.  The bounds halves keep what they hold (the shared bounds, or those of ihm2mpc_set_instance_bounds).  Same
 * preconditions and refusal texts as the host setters (a soft side in the shared table first; both pointers or both NULL; NULL, NULL =
 * batch-shared penalties again, the host setter's own path), and ihm2mpc_set_bounds must have been called.  check != 0: the four rules
 * of the host setter run on the device in its scan order -- no NaN; soft exactly where the shared table is soft; soft_z >= 0 and
 * soft_z + soft_Z > 0 on a soft side -- and the call is refused with the host setter's message for the first offending (instance, stage,
 * side); this reads one int32 per instance back and BLOCKS; on a refusal the handle's tables and mode are untouched.  check == 0:
 * nothing is read back and the call does not block once the per-instance tables exist (the first call builds them, which blocks) --
 * THE CALLER VOUCHES for penalties that follow the four rules: nothing validates them.  soft_z, soft_Z are read in stream order:
 * THE CALLER KEEPS them alive and unchanged until the stream has passed.  The values replace the pair's host-set ones; the other pair
 * stays what it was.  The handle keeps NO HOST COPY of device-set values.  They were admitted under the sides the shared table held
 * soft at that moment (the four rules read nothing else of it), so a later ihm2mpc_set_soft (the rows 0..13) or
 * ihm2mpc_set_alat_constraint (the a_lat pair) that changes WHICH SIDES ARE SOFT cannot check them against the new flags and
 * marks them as no longer fitting -- the next solve is refused ("the per-instance penalties do not fit the batch-shared constraint
 * pattern any more") until every such pair is set again or dropped with NULL, NULL.  Shared setters that leave those flags as they
 * are -- other shared penalty values, ihm2mpc_set_bounds, ihm2mpc_set_path_constraints, finite sides that come or go -- keep the
 * device-set values, as they keep host-set ones: the slot tables are rebuilt from the device's own copy.
 * ihm2mpc_set_instance_bounds and the host setter of the other pair leave device-set values in place as well.  Only a refusal by a
 * precondition or by the check leaves the handle untouched: if building the per-instance tables fails behind them (out of device
 * memory; per-instance bounds that no longer fit the shared table) the pair's previous values are put back as the host setter puts
 * them back, and a previous device-set pair then counts as not fitting. */
int ihm2mpc_set_instance_soft_device(ihm2mpc_handle *h, const void *soft_z, const void *soft_Z, int32_t check);
int ihm2mpc_set_instance_alat_soft_device(ihm2mpc_handle *h, const void *soft_z, const void *soft_Z, int32_t check);
/* The penalty halves of the per-instance tables as the kernels read them, to host arrays: slot_z, slot_Z (B,640) -- zw, Zw of the slot
 * table's entries in table order, then padding (0, -1) up to the structural limit of 640 slots --, stage_z, stage_Z (B,N+1,28), alat_z,
 * alat_Z (B,2); any may be NULL.  Blocking.  Refused while the per-instance tables do not exist (no per-instance bounds or penalties
 * are on).  (For comparing the two setters entry for entry, as ihm2mpc_get_instance_weight_tables does for the weights.) */
int ihm2mpc_get_instance_penalty_tables(ihm2mpc_handle *h, double *slot_z, double *slot_Z, double *stage_z, double *stage_Z,
                                        double *alat_z, double *alat_Z);
/*   ihm2mpc_get_slacks_device <- ihm2mpc_get_slacks and the slk of ihm2mpc_get_alat_multipliers: slk (B,N+1,28), slk_alat (B,N+1,2),
 * device to device in stream order; either may be NULL.  THE CALLER KEEPS the outputs alive until the stream has passed. */
int ihm2mpc_get_slacks_device(ihm2mpc_handle *h, void *slk, void *slk_alat);
/*   ihm2mpc_eval_adjoint_sensitivities_p_device <- ihm2mpc_eval_adjoint_sensitivities_p with the four seeds and the ten outputs in device
 * memory: same shapes, NULL rules (any seed NULL = zero; all four NULL with n_seeds == 2 = the unit seeds on u_0; any output NULL =
 * skipped), NaN rows, preconditions and refusal texts, same bits.  The kernels read the seeds from the caller's memory (with a slack
 * seed the stage seeds are first copied into the handle's seed buffers, where the fold works in place) and the results reach the
 * caller's memory in stream order: no host copy, no wait.  THE CALLER KEEPS the seeds alive and unchanged, and the outputs alive, until
 * the stream has passed the call.  With seed_s, seed_sa and the five new outputs NULL the first five are the bits of
 * ihm2mpc_eval_adjoint_sensitivities_w_device.  Workspace for outputs that are not asked for belongs to the handle, on first use and when
 * n_seeds grows. */
int ihm2mpc_eval_adjoint_sensitivities_p_device(ihm2mpc_handle *h, int32_t n_seeds, const void *seed_x, const void *seed_u,
                                                const void *seed_s, const void *seed_sa,
                                                void *grad_x0, void *grad_yref, void *grad_yref_e, void *grad_W, void *grad_W_e,
                                                void *grad_z, void *grad_Z, void *grad_za, void *grad_Za, void *zeta);

/* ---- plant step (closed-loop MiL): x_next = RK4 x M_sim over dt of `model` under u ---- */
int ihm2mpc_sim_step(ihm2mpc_handle *h, int32_t model, int32_t M_sim, const double *x,
                     const double *u, double *x_next); /* host (B,8),(B,2) -> (B,8) */
/* on device: x0 <- plant(x0, u0 of the last solve); model = -1: kin/dyn switch of python/main.py:482-489 (-2: the same
 * switch with IHM2MPC_MODEL_FDYN6U as the dynamic model) */
int ihm2mpc_sim_advance(ihm2mpc_handle *h, int32_t model, int32_t M_sim);
int ihm2mpc_get_x0(ihm2mpc_handle *h, double *x0);
/* Plant step with forward sensitivities (acados: AcadosSimSolver.solve() with sens_forw, then get("Sx" | "Su" | "S_forw")):
 *   ihm2mpc_sim_step_sens <- AcadosSimSolver.solve() with sens_forw; get("Sx" | "Su" | "S_forw")
 * x (B,8), u (B,2) -> x_next (B,8), S_x (B,8,8) with S_x[b][i][j] = d x_next,i / d x_j, S_u (B,8,2) with S_u[b][i][j] = d x_next,i / d u_j
 * (S_forw = [S_x S_u]), and model_used (B) int32: the model that integrated instance b, 0, 1 or 2 (IHM2MPC_MODEL_*).  Any output may be
 * NULL.
 * model is 0, 1, 2, -1 or -2 as for ihm2mpc_sim_step; the integrator is the handle's sim_integrator_type with M_sim steps over the
 * handle's dt, and the sensitivities are the exact derivative of that discrete map, in its three integrator families:
 *   IHM2MPC_INTEG_ERK      the derivative of the RK4 x M_sim map, propagated through the same stages;
 *   IHM2MPC_INTEG_ERK_LAG  model 0 only: the same with the actuator lags in closed form, stage factors of h = dt / M_sim;
 *   IHM2MPC_INTEG_IRK_GL4 / _IRK_RADAU4  collocation: per step IHM2MPC_IRK_NEWTON_ITER Newton iterations from K = 0 and the
 *                          implicit-function sensitivities at the final stage values (as the linearisation of the shooting intervals),
 *                          with the plant's tableau for h = dt / M_sim; the steps are chained.
 * For a switched plant (model -1 / -2) model_used is the branch the kin / dyn switch of python/main.py:482-489 took at x_b, decided
 * once at the start of the period, and the derivative is that of the branch taken: the rule is PIECEWISE -- on the switching surface
 * x_next itself jumps, and S_x, S_u say nothing about that jump.  An instance gets the bits of a call with its model fixed.
 * Refused as ihm2mpc_sim_step refuses: an unknown model, ERK_LAG with a dynamic or switched plant, too few RK4 sub-steps for the
 * actuator lags, tracks not set, NULL x or u.  The Cartesian plants (IHM2MPC_PLANT_*, ihm2mpc_sim_step_cart) and fdyn10
 * (ihm2mpc_sim_step_dyn10) have no such entry: their model numbers are refused as unknown.
 * Nothing else of the handle changes: x0, u0, the iterate, the linearisation records that ihm2mpc_get_linearization reads and every
 * getter keep their values; of the launch record only [15] bits 4..7 move (code 5).  Staging is local to the call.
 * The host variant blocks.  The device variant takes device memory of the handle's device (or pinned host memory) in the same layouts
 * and is stream-ordered like the other _device entries: inputs and outputs must stay valid, and must not overlap, until the stream has
 * passed; with model_used NULL on a switched plant it waits for the stream itself (the mask is then local to the call). */
int ihm2mpc_sim_step_sens(ihm2mpc_handle *h, int32_t model, int32_t M_sim, const double *x, const double *u,
                          double *x_next, double *S_x, double *S_u, int32_t *model_used);
int ihm2mpc_sim_step_sens_device(ihm2mpc_handle *h, int32_t model, int32_t M_sim, const void *x, const void *u,
                                 void *x_next, void *S_x, void *S_u, void *model_used);
/* one iteration of the MiL loop (python/main.py:476-517) on the device: sim_advance(model, M_sim), prepare_step(s_target) and
 * one RTI iteration.  Same results as the three calls; the plant step and the reference ramp run beside the warm-start
 * shift and the linearisation (they only meet in the QP), which hides the plant's latency. */
int ihm2mpc_step(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double s_target);
/* plant mask (B) for sim_advance / step: an instance with active[b] == 0 keeps its x0 (a car that failed or finished its lap is
 * frozen, as the reference's loop stops, python/main.py:503-517); NULL = all active */
int ihm2mpc_set_active(ihm2mpc_handle *h, const int32_t *active);
/* closed loops longer than the three laps the track tables hold (python/motion_planning.py:405-430): with enable != 0,
 * prepare_step / step first move every car that has passed s = L (L = -s_ref[0], Track::length) back by one lap -- x0 and the
 * s-component of its iterate.  Off by default: the reference's loop stops one metre after a lap (python/main.py:514-517). */
int ihm2mpc_set_lap_wrap(ihm2mpc_handle *h, int32_t enable);
/* pipelined read-back: u0 (B,2) of the last solve is copied to PINNED host memory (ihm2mpc_host_alloc) in stream order, without
 * waiting -- the next ihm2mpc_step can be enqueued at once; the data is valid after ihm2mpc_synchronize (or any blocking getter) */
int ihm2mpc_host_alloc(uint64_t nbytes, void **p);
int ihm2mpc_host_free(void *p);
int ihm2mpc_get_u0_async(ihm2mpc_handle *h, double *pinned_dst);

/* IHM2Controller.compute_control (python/main.py:297-334) in ONE call for the whole batch: x0 (B,8) in, reference ramp +
 * warm-start shift + solve (one RTI iteration, or the configured SQP iterations), u0 (B,2) and status (B, may be NULL) out;
 * one host-device round trip and one wait -- the call of a real-time controller (mpc_control_node.cpp:105-255). */
int ihm2mpc_compute_control(ihm2mpc_handle *h, const double *x0, double s_target, double *u0, int32_t *status);
/* device room for the histories of up to n_steps steps (run_steps grows it on demand; reserving keeps the allocations out of
 * a timed call); while an x0 sensitivity mode is on, also for the gain history of ihm2mpc_run_steps_sens */
int ihm2mpc_reserve_history(ihm2mpc_handle *h, int32_t n_steps);
/* n_steps control steps of the MiL loop (python/main.py:476-517: plant, reference ramp + shift, one RTI iteration) in ONE
 * launch: every instance runs its steps back to back on its own wavefront, so no instance waits for the slowest QP of the
 * batch at every step (throughput follows the mean interior-point iteration count instead of the maximum).  Results are
 * those of n_steps calls of ihm2mpc_step -- bit for bit where both take the single-wave QP kernel and the batch linearisation, i.e.
 * for batches of more than one instance per compute unit; smaller batches take the latency kernels in ihm2mpc_step (four wavefronts
 * per instance in the QP -- the environment variable IHM2MPC_BLOCK_QP=0 turns that off --, results equal to 1e-9); ihm2mpc_step, ihm2mpc_solve and
 * ihm2mpc_compute_control linearise batches of up to 128 intervals (batch <= 3 at N = 40) one sensitivity column per wavefront
 * (the latency path of the single real-time controller), whose records agree with the loop's to 1e-15, not bit for bit.  The persistent loop exists for the three OCP models (fkin6, fdyn6,
 * fdyn6u) -- all-hard constraint tables (the reference's OCP) and soft / track-row tables with batch-shared weights and rows, in the RTI and the SQP mode --
 * and pays off while every instance has a wavefront of its own (batch <= 4 per compute unit); any other case runs
 * n_steps x ihm2mpc_step internally (freeze == 0) or is refused (freeze != 0).
 * freeze != 0: the rules of the reference's loop per car -- a solve status other than 0 / 2 (python/main.py:326-328) or a NaN
 * plant state (:503-504) stops the car where it is, s > lap_stop ends its run (:514-517).  A stopped car's rows hold u0 = 0, its x0 and
 * its last status repeated, and 0 QP iterations.  The loop keeps the stopped cars in a plant mask for later calls with freeze != 0, until
 * ihm2mpc_set_active(NULL): after ihm2mpc_set_active(mask) that is the caller's mask, whose entries the loop clears (ihm2mpc_step and
 * ihm2mpc_sim_advance then see them cleared); otherwise a mask of its own that starts with every car driving, and that one is read by
 * later ihm2mpc_run_steps / ihm2mpc_run_steps_sens calls with freeze != 0 ONLY -- ihm2mpc_step, ihm2mpc_sim_advance and freeze == 0 read
 * a mask only after ihm2mpc_set_active(mask), and move a car again that a frozen loop had stopped.  freeze == 0: a car masked
 * by ihm2mpc_set_active keeps solving, only its plant stands still (as in ihm2mpc_step).  Histories (any may be NULL): u0 (n_steps,B,2), x0 after the plant
 * (n_steps,B,8), status and QP iterations (n_steps,B); copied in stream order (pinned destinations do not block).  ihm2mpc_get_residuals
 * afterwards: the NLP residuals of the iterate the LAST step started from, as after n_steps calls of ihm2mpc_step (in the RTI mode the
 * loop does not form them on the steps before -- they are an output, not an input of the iteration; a car that stopped earlier in the
 * launch keeps what an earlier call left). */
int ihm2mpc_run_steps(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double s_target, int32_t n_steps, int32_t freeze,
                      double lap_stop, double *u0_hist, double *x0_hist, int32_t *status_hist, int32_t *qp_iter_hist);
/* ihm2mpc_run_steps, and x0 sensitivities at every step (acados: eval_param_sens(j, 0, "ex") after each solve of the MiL loop).
 * Needs x0 sensitivity mode 1 or 2 (ihm2mpc_set_x0_sensitivities; refused while it is off).
 * sens_u0_hist (n_steps,B,2,8): du_0/dx0 of every step's solve, the value ihm2mpc_step followed by ihm2mpc_get_x0_sensitivities gives at
 * that step -- bit for bit wherever ihm2mpc_run_steps equals n_steps x ihm2mpc_step bit for bit; may be NULL.  NaN where the solve's
 * status is neither 0 nor 2 and, with freeze, on every step of a car that no longer solves, from the step it stopped (its u0 row is 0).
 * Afterwards ihm2mpc_get_x0_sensitivities and ihm2mpc_get_sens_u0_device read the last step's (mode 2: its whole horizon; NaN for a car
 * that did not solve it).  Every other output -- the four histories, x, u, pi, lam, the slacks -- is that of ihm2mpc_run_steps bit for bit.
 * One launch of the persistent loop with the sensitivity kernel's body behind every QP (kinematic OCP, the tables ihm2mpc_run_steps takes
 * in one launch); otherwise n_steps x ihm2mpc_step with the sensitivity kernel after each QP (freeze refused there, as in
 * ihm2mpc_run_steps).  The history is copied in stream order like the others. */
int ihm2mpc_run_steps_sens(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double s_target, int32_t n_steps, int32_t freeze,
                           double lap_stop, double *u0_hist, double *x0_hist, int32_t *status_hist, int32_t *qp_iter_hist,
                           double *sens_u0_hist);

/* ---- Cartesian side of the ROS stack ----
 * Plants of the simulation node (src/ihm2/src/sim_node.cpp:197-257), state (X, Y, phi, v_x, v_y, r, T, delta): */
#define IHM2MPC_PLANT_KIN6 3    /* python/models.py:168-229 */
#define IHM2MPC_PLANT_DYN6 4    /* python/models.py:310-452 (implicit there; solved for xdot on device) */
#define IHM2MPC_PLANT_ROS (-3)  /* kin6 while hypot(v_x, v_y) < v_dyn, else dyn6; no reversing (sim_node.cpp:200,246-250) */
/* centre line of every track on the s_ref grid of ihm2mpc_set_tracks: X_ref, Y_ref, phi_ref (ntracks, nknots) -- the columns of
 * the track file the C++ Track loads (src/ihm2/src/common/tracks.cpp:132-181) */
int ihm2mpc_set_track_geometry(ihm2mpc_handle *h, const double *X_ref, const double *Y_ref, const double *phi_ref);
/* n_steps plant steps of length dt_sim (the node: 0.01 s), each RK4 x M_sim, under a constant u; host (B,8),(B,2) -> (B,8) */
int ihm2mpc_sim_step_cart(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double dt_sim, int32_t n_steps, double v_dyn,
                          const double *x, const double *u, double *x_next);
/* plant step of the 15-state Frenet model with wheel speeds, fdyn10 (python/models.py:609-801; the DYN10 plant of python/main.py:490-502):
 * x (B,15) = (s, n, psi, v_x, v_y, r, omega_FL, omega_FR, omega_RL, omega_RR, tau_FL, tau_FR, tau_RL, tau_RR, delta), u (B,5) = (four
 * torque commands, u_delta), over the handle's dt on the handle's track tables, with the handle's plant integrator
 * (ihm2mpc_config.sim_integrator_type):
 *   IHM2MPC_INTEG_IRK_RADAU4 -- replaces AcadosSimSolver.simulate of python/main.py:395-400,490-502 (IRK, GAUSS_RADAU_IIA, 4 stages,
 *     num_steps = M_sim): collocation steps of at most dt / M_sim, each solved to convergence (at most IHM2MPC_DYN10_NEWTON_MAX Newton
 *     iterations, else the step is cut by four), so that the reference's start at REST (python/main.py:438-441) integrates -- at
 *     standstill the slip-ratio denominators smooth_abs_nonzero(0) = 1e-6 defeat a fixed number of Newton iterations; NaN rows if a
 *     step cannot be made;
 *   IHM2MPC_INTEG_ERK -- RK4 x M_sim, for moving cars only. */
#define IHM2MPC_DYN10_NEWTON_MAX 10
int ihm2mpc_sim_step_dyn10(ihm2mpc_handle *h, int32_t M_sim, const double *x, const double *u, double *x_next);
/* Track::project (tracks.cpp:183-288) + the Frenet states of the control node (src/ihm2/src/mpc_control_node.cpp:142-157):
 * x_cart (B,8) -> x_frenet (B,8) = (s, n, psi, v_x, v_y, r, T, delta); s_guess (B) in: centre of the search window of
 * half-width s_tol (the node: 2.0), out: fmod(s + 0.05 v_x, lap length) */
int ihm2mpc_project(ihm2mpc_handle *h, const double *x_cart, double *s_guess, double s_tol, double *x_frenet);
/* device-resident Cartesian plant state for closed loops: sim_advance_cart = plant(x_cart, u0 of the last solve), then
 * x0 <- project(x_cart) */
int ihm2mpc_set_cart_state(ihm2mpc_handle *h, const double *x_cart, const double *s_guess);
int ihm2mpc_get_cart_state(ihm2mpc_handle *h, double *x_cart, double *s_guess);
int ihm2mpc_sim_advance_cart(ihm2mpc_handle *h, int32_t model, int32_t M_sim, double dt_sim, int32_t n_steps, double v_dyn,
                             double s_tol);

/* ---- multi-GPU: the one exchange step of the path, RCCL over xGMI behind this ABI, no PyTorch ----
 * Instances are independent: every GPU owns a contiguous block of the global batch and no collective runs on the data path; the
 * results (u0, status: 20 bytes per instance) are gathered once at the end.  Blocks may differ in size (block split): they are
 * padded to the largest block for the collective and trimmed on the host. */
typedef struct ihm2mpc_group ihm2mpc_group;
/* single process, one handle per device (ncclCommInitAll) */
int ihm2mpc_group_create(ihm2mpc_handle *const *handles, int32_t n, ihm2mpc_group **out);
/* u0_all (sum of the batches, 2), status_all (sum of the batches): host, in handle order */
int ihm2mpc_group_allgather_results(ihm2mpc_group *g, double *u0_all, int32_t *status_all);
int ihm2mpc_group_free(ihm2mpc_group *g);
/* one process per GPU (as `python -m torch.distributed.run` launches bench.py): rank 0 makes the 128-byte id, a side channel
 * carries it to the others (ihm2_amd/dist.py: a TCP socket on MASTER_ADDR), every rank joins; sizes (world) = instances per rank */
int ihm2mpc_comm_unique_id(uint8_t *id128);
int ihm2mpc_comm_init(ihm2mpc_handle *h, int32_t world, int32_t rank, const uint8_t *id128, const int32_t *sizes);
int ihm2mpc_comm_allgather_results(ihm2mpc_handle *h, double *u0_all, int32_t *status_all);      /* host, rank order, on every rank */
int ihm2mpc_comm_allreduce_max(ihm2mpc_handle *h, double *value);      /* in place; doubles as a barrier */
/* what the communicator spans, for the record of a multi-GPU run: *count <- ncclCommCount; device_ids (world) <- the PCI identity
 * (domain << 24 | bus << 8 | device; bits 48..62: a tag of the device's UUID, which tells partitions of one package apart) of every rank's
 * device, gathered over the communicator: N ranks on fewer than N devices repeat one */
int ihm2mpc_comm_info(ihm2mpc_handle *h, int32_t *count, int64_t *device_ids);
int ihm2mpc_comm_free(ihm2mpc_handle *h);

#ifdef __cplusplus
}
#endif
#endif
