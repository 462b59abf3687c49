#!/usr/bin/env python3
"""The seeds of tests/test_gpu_factor_sweep_forms.py: for each horizon (and for fdyn6 at N = 5) the first seed of conftest.sample_x0 for which
the oracle's rti_step from the Stanley guess returns status 0 on all 8 instances.  With --slot-forms those of tests/test_gpu_slot_forms.py
instead (N = 40, the reference's rows): the first such seed, and the next one whose solution has at least one active rate row and one active
box (a multiplier above 1e-3 on the rows 10, 11 and on the rows 0..9), so that every slot's arithmetic matters to the result.  Runs on the
CPU (the oracle only).  usage: python tools/find_factor_sweep_seeds.py [--slot-forms]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

B = 8


def solved_seeds(track, model, N, limit):
    """(seed, the oracle's output) for every seed below `limit` whose eight instances all return status 0"""
    from conftest import make_ocp, sample_x0
    from oracle import oracle as orc

    P = orc.OracleProblem(make_ocp(N=N, model=model).flatten().as_dict(track.s_ref, track.kappa_ref))
    for seed in range(limit):
        x0 = sample_x0(track, B, seed=seed)
        x0[:, 3] = np.clip(x0[:, 3], 4.0, 12.0)
        x, u = orc.stanley_guess(P, track.s_ref, track.kappa_ref, x0, N)
        yref, yref_e = orc.prepare_step(N, x0, 40.0, x, u)
        out = P.rti_step(x, u, x0, yref, yref_e)
        if np.all(out["status"] == 0):
            yield seed, out


def main(argv):
    from ihm2_amd.track import track_table

    track = track_table("fsds_competition_1")
    if "--slot-forms" in argv:
        N, first = 40, None
        for seed, out in solved_seeds(track, "fkin6", N, 400):
            lam = out["lam"].reshape(B, N + 1, 2, -1)
            rate, box = lam[..., 10:12].max(), lam[..., 0:10].max()
            if first is None:
                first = seed
                print(f"fkin6 N={N}: seed {seed}, qp_iter {out['qp_iter'].tolist()}, max lam rate rows {rate:.3g}, boxes {box:.3g}")
            elif rate > 1e-3 and box > 1e-3:
                print(f"fkin6 N={N}, an active rate row and an active box: seed {seed}, qp_iter {out['qp_iter'].tolist()}, max lam rate rows {rate:.3g}, boxes {box:.3g}")
                return
        print(f"fkin6 N={N}: no second seed below 400")
        return
    for model, horizons in (("fkin6", (1, 2, 3, 4, 5, 7, 9)), ("fdyn6", (5,))):
        for N in horizons:
            for seed, out in solved_seeds(track, model, N, 200):
                print(f"{model} N={N}: seed {seed}, qp_iter {out['qp_iter'].tolist()}")
                break
            else:
                print(f"{model} N={N}: no seed below 200")


if __name__ == "__main__":
    main(sys.argv[1:])
