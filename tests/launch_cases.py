"""The linearisation and plant kernels a handle launches (csrc/qp_select.hpp: select_linearize, select_sim), as the GPU tests assert
them from the launch record: one table, situation -> (``linearize``, ``sim``) of ``BatchedOcpSolver.get_launch_record``.  The GPU tests
look their handle up here (``names``); tests/test_launch_select.py runs the selectors themselves on every row, without a GPU, through
tools/probes/check_qp_select.cpp.

The rule the rows are instances of is the selectors' own text; the one number of it the tests need, the 128-interval switch
(qp_select.hpp: latency_batch), is ``latency_batch`` below and is checked against the selectors at the boundary rows."""
import dataclasses
import itertools

FKIN6, FDYN6, FDYN6U = 0, 1, 2                  # include/ihm2mpc.h: IHM2MPC_MODEL_*
ERK, IRK_GL, IRK_RADAU, ERK_LAG = 0, 1, 2, 3    # IHM2MPC_INTEG_*
PLANTS = (0, 1, 2, -1, -2)


@dataclasses.dataclass(frozen=True)
class Row:
    model: int          # the OCP's model
    integ: int          # the integrator of the shooting intervals
    sim_integ: int      # ... of the plant
    B: int
    N: int
    plant: int          # the plant model of sim_step / step: -2 .. 2
    cols: bool          # IHM2MPC_LINEARIZE_COLS=1
    lin: str            # the launch record's "linearize"
    sim: str            # ... and "sim"; None: no kernel, the API refuses the plant

    @property
    def key(self):
        return (self.model, self.integ, self.sim_integ, self.B, self.N, self.plant, self.cols)


def _rows(lin, sim, shapes, models=(FKIN6,), integ=(ERK,), sim_integ=ERK, plants=(0,), cols=False):
    return [Row(m, i, sim_integ, B, N, p, cols, lin, sim) for m, i, (B, N), p in itertools.product(models, integ, shapes, plants)]


ALL = (FKIN6, FDYN6, FDYN6U)
DYN = (FDYN6, FDYN6U)
IRK = (IRK_GL, IRK_RADAU)
# the horizons of tests/test_gpu_factor_sweep_forms.py -> the batch just past the switch it compares bit for bit (its other batch is 8)
PAST_THE_SWITCH = {2: 65, 3: 44, 4: 33, 5: 26, 7: 19, 9: 15}

ROWS = (
    # tests/test_gpu_edge_states.py, the linearisation: SHAPES batch and two_tracks (5, 40), odd_horizon (27, 5), columns (3, 40)
    _rows("k_linearize", "k_sim_step_kin", [(5, 40), (27, 5)])
    + _rows("k_linearize_cols", "k_sim_step", [(3, 40)])
    + _rows("k_linearize_dyn", "k_sim_step_kin", [(5, 40), (27, 5)], models=DYN)
    + _rows("k_linearize_dyn", "k_sim_step", [(3, 40)], models=DYN)
    + _rows("k_linearize_irk", "k_sim_step", [(5, 40), (27, 5), (3, 40)], models=ALL, integ=IRK)
    # tests/test_gpu_edge_states.py, the plants on the table itself (B = 87): RK4, the handle of a collocation OCP -- the kinematic plant has
    # no integrator to share there -- and the collocation plants
    + _rows("k_linearize", "k_sim_step_kin", [(87, 40)])
    + _rows("k_linearize", "k_sim_step", [(87, 40)], plants=(1, 2, -1, -2))
    + _rows("k_linearize_irk", "k_sim_step", [(87, 40)], integ=(IRK_GL,), plants=PLANTS)
    + _rows("k_linearize", "k_sim_irk", [(87, 40)], sim_integ=IRK_RADAU, plants=PLANTS)
    # tests/test_gpu_factor_sweep_forms.py: B = 8 at its horizons, and the smallest batch past the switch; the speed-switched plant
    + _rows("k_linearize_cols", "k_sim_step", [(8, N) for N in PAST_THE_SWITCH], plants=(-1,))
    + _rows("k_linearize", "k_sim_step", [(B, N) for N, B in PAST_THE_SWITCH.items()], plants=(-1,))
    # tests/test_gpu_fkin6_forms.py: N = 5, both batches, RK4 and the closed-form lags (one kernel at every batch size)
    + _rows("k_linearize", "k_sim_step_kin", [(67, 5)])
    + _rows("k_linearize_cols", "k_sim_step", [(3, 5)])
    + _rows("k_linearize_lag", "k_sim_step_kin_lag", [(67, 5), (3, 5)], integ=(ERK_LAG,), sim_integ=ERK_LAG)
    # tests/test_gpu_sim_sens.py: handles whose plant integrates as their shooting intervals do
    + _rows("k_linearize_lag", "k_sim_step_kin_lag", [(5, 40)], integ=(ERK_LAG,), sim_integ=ERK_LAG)
    + _rows("k_linearize_irk", "k_sim_irk", [(5, 40)], models=(FKIN6, FDYN6), integ=(IRK_GL,), sim_integ=IRK_GL)
    # tests/test_gpu_workspace_poison.py: one controller
    + _rows("k_linearize_cols", "k_sim_step", [(1, 40)])
    # the boundary: 128 and 129 intervals, and the batches around it at the horizon 40
    + _rows("k_linearize_cols", "k_sim_step", [(2, 64)])
    + _rows("k_linearize", "k_sim_step_kin", [(3, 43), (4, 40)])
    # IHM2MPC_LINEARIZE_COLS=1 above the switch: the column kernel; the plant does not read the switch
    + _rows("k_linearize_cols", "k_sim_step_kin", [(4, 40)], cols=True)
    # an RK4 plant behind an OCP with the closed-form lags: no integrator to share either
    + _rows("k_linearize_lag", "k_sim_step", [(5, 40)], integ=(ERK_LAG,))
    # a plant with the closed-form lags behind an RK4 OCP: the kinematic plant only
    + _rows("k_linearize", "k_sim_step_kin_lag", [(5, 40)], sim_integ=ERK_LAG)
    + _rows("k_linearize", None, [(5, 40)], sim_integ=ERK_LAG, plants=(1, 2, -1, -2))
)
TABLE = {r.key: r for r in ROWS}
assert len(TABLE) == len(ROWS), "a situation is listed twice"
# pairs of (B, N) on the two sides of the switch
BOUNDARY_PAIRS = [((2, 64), (3, 43)), ((3, 40), (4, 40))]


def latency_batch(B, N) -> bool:
    """qp_select.hpp: latency_batch -- the few instances of a real-time controller, which ihm2mpc_step linearises with the column kernel and
    whose kinematic plant is the state-only rollout: its results agree with the persistent loop's to rounding, not bit for bit."""
    return B * N <= 128


def names(solver, plant=0, cols=False):
    """(linearize, sim) of the launch record for a BatchedOcpSolver and the plant model of its sim_step / step calls; a handle that is not
    in the table is a KeyError: add its row, which tests/test_launch_select.py then checks against the selectors."""
    d = solver.ocp.flatten()
    r = TABLE[(d.model, d.integrator, d.sim_integrator, solver.B, solver.N, plant, cols)]
    return r.lin, r.sim
