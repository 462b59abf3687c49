"""Per-section table of two cycle-stamp dumps of tools/run_stamped_qp.py (the `[stamps b=.. it=..]` lines), side by side.

    python tools/stamps_table.py LABEL_A=dump_a.txt LABEL_B=dump_b.txt [--sections 7,9] [--stages 40]

With --stages the chosen sections are also given per sweep stage: S:7 runs one sweep per iteration, S:9 two.
"""
import re
import sys

NAMES = {31: "QP data, NLP residuals, slot load", 0: "initial point", 1: "slack residuals, complementarity", 14: "exact residual (i)", 2: "dyn_residual (ii)",
         3: "norms, convergence test", 4: "slot_coeffs + add_coeffs", 5: "factor sweep", 6: "corrector: p base", 7: "vector sweep", 8: "kff, c_k",
         9: "forward sweep (both passes)", 10: "du", 16: "dpi: addresses, loads issued", 18: "dpi: first chain (the wait for P_k)", 19: "dpi: the other chains", 11: "slack / multiplier steps", 15: "step length reductions, mu_aff, sigma", 12: "step test",
         17: "update: r_g loads issued, H dz of the first element", 20: "update: first r_g used (the wait for it)", 21: "update: the other r_g",
         22: "update: r_b, z, pi, slots", 13: "RTI update, outputs"}
SWEEPS_PER_ITER = {7: 1, 9: 2}


def read(path):
    out = {}
    for line in open(path):
        m = re.match(r"\[stamps b=(\d+) it=(\d+)\](.*)", line)
        if m:
            out[int(m.group(1))] = (int(m.group(2)), [int(v) for v in m.group(3).split()])
    return out


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if "=" in a and not a.startswith("--")]
    secs = [int(s) for s in sys.argv[sys.argv.index("--sections") + 1].split(",")] if "--sections" in sys.argv else list(NAMES)
    stages = int(sys.argv[sys.argv.index("--stages") + 1]) if "--stages" in sys.argv else 0
    labels = [a.split("=", 1)[0] for a in args]
    dumps = [read(a.split("=", 1)[1]) for a in args]
    print("iterations of the instances 0..15:", [dumps[0][b][0] for b in sorted(dumps[0])])
    for b in sorted(dumps[0]):
        if any(b not in d or d[b][0] != dumps[0][b][0] for d in dumps):
            print("instance %d: iteration counts differ between the dumps" % b)
            continue
        it = dumps[0][b][0]
        print("\ninstance %d: %d interior-point iterations" % (b, it))
        print("  %-44s" % "section" + "".join("%12s" % l for l in labels) + "".join("%14s" % (l + "/" + labels[0]) for l in labels[1:])
              + ("".join("%16s" % (l + " /stage") for l in labels) if stages else ""))
        for s in secs:
            v = [d[b][1][s] for d in dumps]
            row = "  S:%-2d %-39s" % (s, NAMES[s]) + "".join("%12d" % x for x in v) + "".join("%14.3f" % (x / v[0]) for x in v[1:])
            if stages and s in SWEEPS_PER_ITER:
                row += "".join("%16.1f" % (x / (it * SWEEPS_PER_ITER[s] * stages)) for x in v)
            print(row)
        print("  %-44s" % "total" + "".join("%12d" % sum(d[b][1]) for d in dumps))
