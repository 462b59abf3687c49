"""The stop rules of the persistent control-step loop (ihm2mpc_run_steps with freeze != 0; include/ihm2mpc.h, csrc/kernels_qp.hip:
k_steps) in plain numpy.  A helper: no GPU, no product code.

The cars of a batch do not see one another, so what the frozen loop returns for a car is what the loop without freeze returns up to
the step the car stops at, and constant rows from there on.  `apply` takes the histories of a run WITHOUT freeze (launches per step
or one launch, they are the same bits) and gives the histories the frozen run must return.  Per car and control step t, in the
kernel's order:

  1. a car whose mask entry is 0 at the start of step t stops at t; so does one whose last solve (the one before the call for t = 0,
     row t - 1 after that) ended with a status other than 0 / 2.  Its mask entry becomes 0 and the rows t .. T - 1 hold
         u0 = 0,  x0 = its x0 before step t,  status = that last status,  qp_iter = 0,  sens_u0 = NaN;
  2. a car whose plant state after step t's plant has a NaN (row t of the x0 history without freeze) stops at t in the same way, with
     the x0 from before the step;
  3. a car with x0[t, b, 0] > lap_stop keeps row t -- the step was driven and solved -- and its mask entry becomes 0: it stops at t + 1
     by rule 1 (in the next call if t was the last step).

tests/test_freeze_ref.py checks the rules on hand-written histories and against the bookkeeping of
ihm2_amd.closed_loop_sim.run_closed_loop; tests/test_gpu_freeze_rules.py holds every k_steps instantiation to them."""
import numpy as np

NONE, MASK, STATUS, NAN, LAP = 0, 1, 2, 3, 4          # `cause`: why a car's mask entry went to 0 (MASK: it was 0 before the call)
ACCEPTED = (0, 2)


def apply(hist, status_before, x0_before, active_before, lap_stop):
    """hist: u0 (T,B,2), x0 (T,B,8), status (T,B), qp_iter (T,B) and optionally sens_u0 (T,B,2,8) of a run without freeze;
    status_before (B), x0_before (B,8), active_before (B) or None (all driving): the handle's state when the frozen call starts.

    Returns a dict with the same histories as the frozen call must return them, and
      stop_step (B)  the first step whose row is a stopped car's (T for a car that drove every step of the call),
      cause (B)      NONE, MASK, STATUS, NAN or LAP: why the mask entry is 0 (NONE where it is still 1 -- also for a car whose LAST
                     row has a failed status: rule 1 stops it at the next call's step 0),
      active (B)     the mask the call leaves (int32),
      x0_final (B,8) the plant state the call leaves."""
    T, B = hist["status"].shape
    out = {k: np.array(hist[k], copy=True) for k in ("u0", "x0", "status", "qp_iter")}
    if hist.get("sens_u0") is not None:
        out["sens_u0"] = np.array(hist["sens_u0"], copy=True)
    active = np.ones(B, dtype=np.int32) if active_before is None else (np.asarray(active_before) != 0).astype(np.int32)
    cause = np.where(active != 0, NONE, MASK).astype(np.int32)
    stop_step = np.full(B, T, dtype=np.int64)
    x0_final = np.array(x0_before, dtype=np.float64, copy=True).reshape(B, 8)
    for b in range(B):
        last_status, x_prev = int(status_before[b]), x0_final[b].copy()
        for t in range(T):
            stop = active[b] == 0
            if not stop and last_status not in ACCEPTED:                          # rule 1
                stop, cause[b] = True, STATUS
            if not stop and np.isnan(hist["x0"][t, b]).any():                     # rule 2
                stop, cause[b] = True, NAN
            if stop:
                active[b], stop_step[b] = 0, t
                out["u0"][t:, b] = 0.0
                out["x0"][t:, b] = x_prev
                out["status"][t:, b] = last_status
                out["qp_iter"][t:, b] = 0
                if "sens_u0" in out:
                    out["sens_u0"][t:, b] = np.nan
                break
            last_status, x_prev = int(hist["status"][t, b]), hist["x0"][t, b].copy()
            if x_prev[0] > lap_stop:                                              # rule 3
                active[b], cause[b] = 0, LAP
        x0_final[b] = x_prev
    return dict(out, stop_step=stop_step, cause=cause, active=active, x0_final=x0_final)


def stopped_in_call(ref) -> np.ndarray:
    """(B) bool: the cars with at least one stopped row in the call `ref` was computed for."""
    return ref["stop_step"] < ref["status"].shape[0]
