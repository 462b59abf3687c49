"""Lists the loops of one kernel in a hipcc -S listing with their instruction mix (a quick look at where a latency-bound
kernel spends its issue slots).   python tools/asm_loops.py file.s <first_line> <last_line>

python tools/asm_loops.py file.s --mfma-loop <kernel name filter> [...]
    for every kernel of the listing whose (mangled) name holds a filter: the instruction classes of the loop that holds the
    matrix instructions -- of the backward-branch loops with the most v_mfma in them the smallest: in the QP kernels the factor
    sweep's pass of RIC_RING stages (riccati_mfma.hpp).  Classes only: what an instruction is for is read off its prefix.  Runs on a listing made
    without a GPU (hipcc -S --cuda-device-only with the Makefile's flags)."""
import re
import sys
from collections import Counter

CLASSES = ["fp64 arithmetic", "matrix", "scalar ALU", "accvgpr moves", "lane reads/writes", "vector integer", "other moves/selects",
           "nop + waitcnt", "LDS", "memory", "scratch", "branch", "other"]


def sweep_class(op):
    """class of a mnemonic for the --mfma-loop table"""
    if op.startswith("v_mfma"): return "matrix"
    if op.startswith("v_accvgpr"): return "accvgpr moves"
    if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")): return "lane reads/writes"
    if op.startswith(("s_nop", "s_waitcnt")): return "nop + waitcnt"
    if op.startswith(("s_cbranch", "s_branch")): return "branch"
    if op.startswith("s_"): return "scalar ALU"
    if op.startswith("ds_"): return "LDS"
    if op.startswith("scratch_"): return "scratch"
    if op.startswith(("global_", "buffer_", "flat_")): return "memory"
    if op.startswith("v_") and "f64" in op and not op.startswith("v_cmp"): return "fp64 arithmetic"
    if op.startswith(("v_mov", "v_cndmask", "v_cmp", "v_pk_mov", "v_swap")): return "other moves/selects"
    if op.startswith("v_"): return "vector integer"
    return "other"


def instructions(lines, lo, hi):
    """[(line index, mnemonic)] of the listing's lines lo .. hi - 1, and {label: line index}"""
    ins, labels = [], {}
    for i in range(lo, hi):
        t = lines[i].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if m:
            labels[m.group(1)] = i
            continue
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        ins.append((i, t.split()[0], t))
    return ins, labels


def loops_of(ins, labels):
    """(first line, last line) of every backward branch"""
    out = []
    for i, op, t in ins:
        if op.startswith(("s_cbranch", "s_branch")):
            m = re.search(r"(\.LBB\d+_\d+)", t)
            if m and m.group(1) in labels and labels[m.group(1)] < i:
                out.append((labels[m.group(1)], i))
    return out


def mfma_loop_report(path, filters):
    lines = open(path).read().split("\n")
    funcs, name, start = [], None, 0
    for n, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            name, start = m.group(1), n
        elif l.startswith(".Lfunc_end") and name:
            funcs.append((name, start, n)); name = None
    for name, a, b in funcs:
        if not any(f in name for f in filters):
            continue
        ins, labels = instructions(lines, a + 1, b)
        # the compiler lays a stage's early exits out as backward branches of their own: of the loops that hold the most matrix
        # instructions, the smallest is the pass
        best, most = None, 0
        for lo, hi in loops_of(ins, labels):
            body = [op for i, op, _ in ins if lo <= i <= hi]
            n = sum(op.startswith("v_mfma") for op in body)
            if n and (n > most or (n == most and len(body) < len(best))):
                best, most = body, n
        print(f"{name}: {len(ins)} instructions in the kernel")
        if best is None:
            print("    no loop with a matrix instruction"); continue
        mix = Counter(sweep_class(op) for op in best)
        print(f"    loop with the matrix instructions: {len(best)} instructions, {mix['matrix']} of them matrix")
        for c in CLASSES:
            if mix[c]:
                print(f"        {c:22s} {mix[c]:5d}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[2] == "--mfma-loop":
        mfma_loop_report(sys.argv[1], sys.argv[3:] or [""])
        sys.exit(0)
    lines = open(sys.argv[1]).read().split("\n")
    lo, hi = int(sys.argv[2]), int(sys.argv[3])
    labels = {}
    for i in range(lo, hi):
        m = re.match(r"^(\.LBB\d+_\d+):", lines[i])
        if m:
            labels[m.group(1)] = i
    loops = []
    for i in range(lo, hi):
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)|^\s+s_branch\s+(\.LBB\d+_\d+)", lines[i])
        if m:
            t = m.group(1) or m.group(2)
            if t in labels and labels[t] < i:
                loops.append((labels[t], i))
    for a, b in sorted(loops):
        mix = Counter()
        for l in lines[a:b + 1]:
            l = l.strip()
            if not l or l.startswith((";", ".")) or l.endswith(":"):
                continue
            op = l.split()[0]
            key = ("valu_f64" if re.match(r"v_(fma|mul|add|fmac|max|min|rcp|div|cmp\w*)_f64|v_(fma|mul|add)_f64", op) else
                   "valu" if op.startswith("v_") else "lds" if op.startswith("ds_") else "scratch" if op.startswith("scratch_") else
                   "global" if op.startswith(("global_", "buffer_", "flat_")) else "waitcnt" if op.startswith("s_waitcnt") else
                   "salu" if op.startswith("s_") else "other")
            mix[key] += 1
        print(f"loop {a + 1}-{b + 1}: {sum(mix.values())} instr", dict(mix))
