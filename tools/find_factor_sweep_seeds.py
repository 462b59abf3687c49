#!/usr/bin/env python3
"""The seeds of tests/test_gpu_factor_sweep_forms.py: for each horizon (and for fdyn6 at N = 5) the first seed of conftest.sample_x0 for which
the oracle's rti_step from the Stanley guess returns status 0 on all 8 instances.  Runs on the CPU (the oracle only).  usage: python tools/find_factor_sweep_seeds.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import make_ocp, sample_x0  # noqa: E402
from ihm2_amd.track import track_table  # noqa: E402
from oracle import oracle as orc  # noqa: E402

B = 8
track = track_table("fsds_competition_1")
for model, horizons in (("fkin6", (1, 2, 3, 4, 5, 7, 9)), ("fdyn6", (5,))):
    for N in horizons:
        ocp = make_ocp(N=N, model=model)
        P = orc.OracleProblem(ocp.flatten().as_dict(track.s_ref, track.kappa_ref))
        for seed in range(200):
            x0 = sample_x0(track, B, seed=seed)
            x0[:, 3] = np.clip(x0[:, 3], 4.0, 12.0)
            x, u = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
            yref, yref_e = orc.prepare_step(N, x0, 40.0, x, u)
            out = P.rti_step(x, u, x0, yref, yref_e)
            if np.all(out["status"] == 0):
                print(f"{model} N={N}: seed {seed}, qp_iter {out['qp_iter'].tolist()}")
                break
        else:
            print(f"{model} N={N}: no seed below 200")
