"""The per-instance weight tables expanded on the device (kernels_weights.hip: k_weight_tables, ihm2mpc_set_instance_weights_device)
against the host setter (ihm2mpc_set_instance_weights), entry for entry through ihm2mpc_get_instance_weight_tables: equality of bits on
ordinary and on edge weights, the refusals of the validating form with the host setter's messages, the solves behind both setters, and
a poisoned workspace.  No tolerance anywhere: the kernel restates the host's sums term by term."""
import ctypes as C

import numpy as np
import pytest

import drive
from devmem import DevMem
from test_gpu_adjoint_weights import _coupled
from test_gpu_qp_layouts import TABLE, _solver

pytestmark = pytest.mark.gpu


def _bits(t):
    return {k: np.ascontiguousarray(v).view(np.uint64) for k, v in t.items()}


def _assert_same_tables(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.keys() == b.keys() == {"Hs", "Gy", "Wd"}
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")


def _weight_sets(B):
    """name -> (W (B,12,12), W_e (B,8,8)): symmetric, no NaN; instance b's weights differ from every other's."""
    from ihm2_amd import ocp as O

    W0, We0 = O.default_weights()
    fac = (1.0 + 0.01 * np.arange(B))[:, None, None]
    rng = np.random.default_rng(2024)

    def sym_random(n):
        G = rng.uniform(-3.0, 1.0, (B, n, n))           # mostly negative off-diagonal entries
        S = 0.5 * (G + np.swapaxes(G, 1, 2))
        S[:, np.arange(n), np.arange(n)] = rng.uniform(0.5, 50.0, (B, n))
        return S

    def edge(n):
        # 0.0, -0.0, the smallest subnormal and 1e300 in symmetric places; 1.7e308 where the selector adds four entries (rows 6, 10 of W:
        # acc = W[6][6] + W[10][6] + W[6][10] + W[10][10] overflows before c_s is applied) -- inf on both sides, and inf - inf in the
        # symmetry test is a NaN that no comparison refuses
        E = np.zeros((B, n, n))
        vals = [0.0, -0.0, 5e-324, 1e300, -5e-324, -1e300, 1.0]
        for i in range(n):
            for j in range(i, n):
                E[:, i, j] = E[:, j, i] = vals[(3 * i + j) % len(vals)]
        E[1::2] = -E[1::2]                              # every other instance: the signs flipped (-0.0 <-> 0.0 too)
        if n == 12:
            E[:, 6, 6] = E[:, 10, 10] = E[:, 6, 10] = E[:, 10, 6] = 1.7e308
        return E

    return {"default": (fac * W0[None], fac * We0[None]),
            "coupled": (fac * _coupled(W0)[None], fac * _coupled(We0)[None]),
            "random_symmetric": (sym_random(12), sym_random(8)),
            "edge_values": (edge(12), edge(8))}


@pytest.mark.parametrize("B", [1, 65])
def test_tables_equal_the_host_setters_bit_for_bit(track, B):
    """B = 65: one instance past a wavefront of lanes.  The device setter comes first on a fresh handle (it allocates the tables), with
    and without the validating form; the host setter follows on the same handle."""
    dm = DevMem()
    s = _solver(track, TABLE["hard_5_per_lane"][0], B, "default", "0")
    with pytest.raises(Exception, match="per-instance weights are off"):
        s.get_instance_weight_tables()
    for name, (W, We) in _weight_sets(B).items():
        dW, dWe = dm.up(W), dm.up(We)
        got = {}
        for check in (False, True):
            s.set_instance_weights_device(dW, dWe, check=check)
            got[check] = s.get_instance_weight_tables()
            s.set_instance_weights_device(0, 0)            # shared again: the next call allocates anew
            with pytest.raises(Exception, match="per-instance weights are off"):
                s.get_instance_weight_tables()
        s.set_instance_weights(W, We)
        host = s.get_instance_weight_tables()
        assert host["Hs"].shape == (B, 2, 10, 10) and host["Gy"].shape == (B, 2, 10, 12) and host["Wd"].shape == (B, 208)
        _assert_same_tables(got[False], host, f"{name}, check = 0")
        _assert_same_tables(got[True], host, f"{name}, check = 1")
        np.testing.assert_array_equal(host["Wd"].view(np.uint64), np.concatenate([W.reshape(B, -1), We.reshape(B, -1)], 1).view(np.uint64))
        if name == "edge_values":
            assert np.isinf(host["Hs"][:, 0, 6, 6]).all() and np.signbit(host["Wd"]).any() and (host["Wd"] == 5e-324).any()
    s.free(); dm.free()


def _message(fn):
    from ihm2_amd._lib import Ihm2mpcError

    with pytest.raises(Ihm2mpcError) as e:
        fn()
    return str(e.value)


def test_refusals_carry_the_host_setters_messages_and_leave_the_tables(track):
    from ihm2_amd import _lib
    from ihm2_amd import ocp as O

    B = 8
    dm = DevMem()
    s = _solver(track, TABLE["hard_5_per_lane"][0], B, "default", "0")
    W0, We0 = O.default_weights()
    good = _weight_sets(B)["coupled"]
    s.set_instance_weights_device(dm.up(good[0]), dm.up(good[1]), check=True)
    last_good = s.get_instance_weight_tables()

    def tile():
        return np.tile(W0[None], (B, 1, 1)), np.tile(We0[None], (B, 1, 1))

    cases = {}
    W, We = tile(); W[3, 7, 2] = np.nan; We[1, 0, 0] = np.nan; W[6, 0, 0] = np.nan      # the first offender: instance 1 (W_e), not 3
    cases["nan_first_instance"] = (W, We, "instance 1: W_e[0][0] is NaN")
    W, We = tile(); W[3, 7, 2] = np.nan; W[3, 9, 11] = np.nan; We[3, 2, 2] = np.nan     # within an instance: W before W_e, the first entry
    cases["nan_W"] = (W, We, "instance 3: W[7][2] is NaN")
    W, We = tile(); We[4, 7, 6] = np.nan; W[2, 1, 4] += 1e-6                            # NaN of a later instance after an asymmetric one
    cases["asym_before_nan"] = (W, We, "instance 2: the weight matrix of the stages 0..39 is not symmetric")
    W, We = tile(); W[5, 2, 9] += 1e-6
    cases["asym_stage"] = (W, We, "instance 5: the weight matrix of the stages 0..39 is not symmetric")
    W, We = tile(); We[2, 0, 5] += 1e-6
    cases["asym_terminal"] = (W, We, "instance 2: the weight matrix of stage 40 (terminal) is not symmetric")
    for name, (W, We, want) in cases.items():
        dW, dWe = dm.up(W), dm.up(We)
        dev = _message(lambda: s.set_instance_weights_device(dW, dWe, check=True))
        _assert_same_tables(s.get_instance_weight_tables(), last_good, f"{name}: after the device setter's refusal")
        host = _message(lambda: s.set_instance_weights(W, We))
        assert dev == host == want, (name, dev, host)
    # W without W_e, at the C boundary (the Python wrappers refuse it themselves)
    dW = dm.up(good[0])
    dev = _message(lambda: _lib.check(s.lib.ihm2mpc_set_instance_weights_device(s._h, C.c_void_p(dW), None, 1)))
    host = _message(lambda: _lib.check(s.lib.ihm2mpc_set_instance_weights(s._h, good[0].ctypes.data_as(_lib.c_double_p), None)))
    assert dev == host and "both be given" in dev
    _assert_same_tables(s.get_instance_weight_tables(), last_good, "after W without W_e")
    # inside the tolerance of the symmetry test: accepted by both, same tables
    W, We = tile(); W[5, 2, 9] *= 1.0 + 1e-14; W[5, 3, 3] *= 1.0 + 1e-14; We[2, 0, 0] *= 1.0 + 1e-14
    W[4, 0, 1] += 1e-14; We[6, 4, 5] += 1e-14
    assert W[4, 0, 1] != W[4, 1, 0] and We[6, 4, 5] != We[6, 5, 4]
    s.set_instance_weights_device(dm.up(W), dm.up(We), check=True)
    dev_t = s.get_instance_weight_tables()
    s.set_instance_weights(W, We)
    _assert_same_tables(dev_t, s.get_instance_weight_tables(), "asymmetric by 1e-14")
    assert not np.array_equal(dev_t["Hs"], last_good["Hs"])
    s.free()

    # before ihm2mpc_set_weights: a bare handle
    cfg = _lib.Config(batch=B, N=10, M=25, model=0, ntracks=1, nknots=10, device=0, nlp_solver_type=0, nlp_solver_max_iter=1, ipm_iter_max=10,
                      dt=0.05, cost_scale_stage=0.05, ipm_tol=1e-6, ipm_mu0=0.03, ipm_tau0=0.1, nlp_tol=1e-6)
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.ihm2mpc_create(C.byref(cfg), C.byref(h)))
    dW, dWe = dm.up(good[0]), dm.up(good[1])
    dev = _message(lambda: _lib.check(lib.ihm2mpc_set_instance_weights_device(h, C.c_void_p(dW), C.c_void_p(dWe), 1)))
    dev0 = _message(lambda: _lib.check(lib.ihm2mpc_set_instance_weights_device(h, C.c_void_p(dW), C.c_void_p(dWe), 0)))
    host = _message(lambda: _lib.check(lib.ihm2mpc_set_instance_weights(h, good[0].ctypes.data_as(_lib.c_double_p), good[1].ctypes.data_as(_lib.c_double_p))))
    assert dev == dev0 == host and "ihm2mpc_set_weights has not been called" in dev
    assert "per-instance weights are off" in _message(lambda: _lib.check(lib.ihm2mpc_get_instance_weight_tables(h, None, None, None)))
    _lib.check(lib.ihm2mpc_free(h))
    dm.free()


@pytest.mark.parametrize("name", ["hard_5_per_lane", "soft_2_per_lane_split_rows"])
def test_solves_behind_the_device_setter_equal_the_host_setters(track, name):
    """Three weight sets assigned by b % 3 (test_gpu_adjoint_weights.py::test_per_instance_weights), two RTI steps: the same bits."""
    from ihm2_amd import ocp as O

    lay, B = TABLE[name][0], 30
    assign = np.arange(B) % 3
    W0, We0 = O.default_weights()
    var = [(W0 * (1.0 + 0.5 * j), We0 * (1.0 + 0.25 * j)) for j in range(3)]
    W, We = np.stack([var[a][0] for a in assign]), np.stack([var[a][1] for a in assign])
    x0 = drive.clipped_start(track, B, 4343)
    dm = DevMem()
    res = []
    for device in (False, True):
        s = _solver(track, lay, B, "default", "0")
        if device:
            s.set_instance_weights_device(dm.up(W), dm.up(We), check=False)
        else:
            s.set_instance_weights(W, We)
        s.set_x0(x0); s.init_guess()
        out = []
        for _ in range(2):
            s.prepare_step(40.0)
            st = s.solve()
            out.append(dict(status=st, qp_iter=s.get_qp_iter(), x=s.get_x(), u=s.get_u(), lam=s.get_multipliers()[1]))
        res.append(out)
        s.free()
    for a, b in zip(*res):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert (res[0][-1]["status"] == 0).mean() > 0.5
    assert not np.array_equal(res[0][-1]["u"][0], res[0][-1]["u"][1])
    dm.free()


def test_poisoned_workspace_gives_the_same_tables(track):
    from poison_cases import ENV, environ, poison_value

    B = 65
    W, We = _weight_sets(B)["coupled"]
    dm = DevMem()
    dW, dWe = dm.up(W), dm.up(We)
    res = []
    for value in (None, poison_value()):
        with environ(**{ENV: value}):
            s = _solver(track, TABLE["hard_5_per_lane"][0], B, "default", "0")
        if value is not None:
            assert all(np.isnan(a).all() for a in s.get_linearization()), "the poisoned handle's workspace is not NaN"
        s.set_instance_weights_device(dW, dWe, check=True)
        first = s.get_instance_weight_tables()
        s.set_instance_weights_device(dW, dWe, check=False)
        res.append((first, s.get_instance_weight_tables()))
        s.free()
    _assert_same_tables(res[0][0], res[1][0], "poisoned vs clean, check = 1")
    _assert_same_tables(res[0][1], res[1][1], "poisoned vs clean, check = 0")
    _assert_same_tables(res[0][0], res[0][1], "check = 1 vs check = 0")
    assert all(np.isfinite(v).all() for v in res[1][0].values())
    dm.free()
