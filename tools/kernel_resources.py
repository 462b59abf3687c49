#!/usr/bin/env python3
"""Register / scratch / occupancy / static LDS listing of every kernel of libihm2mpc.so (hipcc -Rpass-analysis=kernel-resource-usage on each source
with the Makefile's flags; the QP source once per instantiation set).  usage: tools/kernel_resources.py [source directory] > profiles/rN/kernel_resources.txt
(the directory: a copy of csrc made by tools/build_variant.sh, for the table of another commit)"""
import os, re, subprocess, sys
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "ihm2_amd", "csrc")
BASE = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-c", "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
QP = ["-mllvm", "-amdgpu-mfma-vgpr-form=1"]
jobs = [(f, []) for f in ("kernels_misc.hip", "kernels_linearize.hip", "kernels_cart.hip", "kernels_dyn10.hip", "kernels_sqp.hip", "kernels_irk.hip", "kernels_sens.hip", "kernels_adj.hip",
                             "kernels_cost.hip", "kernels_slackseed.hip", "kernels_penaltygrad.hip")]
jobs += [("kernels_qp.hip", ["-DQP_SET=0"] + QP), ("kernels_qp.hip", ["-DQP_SET=1"] + QP), ("kernels_qp.hip", ["-DQP_SET=2"] + QP),
         ("kernels_qp.hip", ["-DQP_SET=3"] + QP), ("kernels_qp.hip", ["-DQP_SET=4"] + QP + ["-fno-unroll-loops"]),
         ("kernels_qp.hip", ["-DQP_SET=5"] + QP), ("kernels_qp.hip", ["-DQP_SET=6"] + QP + ["-fno-unroll-loops"]),
         ("kernels_qp.hip", ["-DQP_SET=7"] + QP + ["-fno-unroll-loops"])]
with ThreadPoolExecutor(max_workers=max(1, min(8, len(os.sched_getaffinity(0))))) as pool:       # the compilers run side by side, the table keeps the order of `jobs`
    outs = list(pool.map(lambda j: subprocess.run(BASE + j[1] + [j[0]], cwd=SRC, capture_output=True, text=True).stderr, jobs))
for (f, extra), out in zip(jobs, outs):
    recs, cur = [], None
    for line in out.splitlines():
        m = re.search(r"remark: +(Function Name|TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m: continue
        k, v = m.group(1), m.group(2)
        if k == "Function Name":
            cur = {"mangled": v}; recs.append(cur)
        elif cur is not None:
            cur.setdefault(k.split(" ")[0], v)
    names = subprocess.run(["c++filt"], input="\n".join(r["mangled"] for r in recs), capture_output=True, text=True).stdout.splitlines()
    for r, n in zip(recs, names):
        if "k_" not in n: continue          # kernels only (device functions called from them are listed by the compiler as well)
        n = re.sub(r"\(.*", "", n.replace("(anonymous namespace)::", "").replace("void ", ""))
        print(f"{f:22s} {n:40s} SGPRs {r.get('TotalSGPRs', '?'):>3s}  VGPRs {r.get('VGPRs', '?'):>3s}  AGPRs {r.get('AGPRs', '?'):>3s}  scratch {r.get('ScratchSize', '?'):>5s} B/lane  occupancy {r.get('Occupancy', '?')} waves/SIMD  static LDS {r.get('LDS', '?')} B")
