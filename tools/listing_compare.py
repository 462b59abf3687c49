#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds, object by object and function by function.

usage: tools/listing_compare.py DIR_A DIR_B [-o FILE]

DIR_A, DIR_B: two directories of objects (*.o) built from ihm2_amd/csrc, e.g. the parent commit's (tools/build_variant.sh, or a copy of csrc built
with its Makefile) and this tree's.  For every object present in both, the gfx950 code object is taken out of the .hip_fatbin section,
disassembled with llvm-objdump, and cut at the function labels.  Two functions are identical when their instruction texts agree line for line with
addresses and encodings (the trailing comment of every line) left out, together with the literal pc-relative offsets that follow an s_getpc_b64
(calls and references to other symbols: they move with the layout of the object, not with the function) and the padding behind the last
instruction.  A function whose name exists on one side only is paired with a function of the other side that has the same body, if there is one
(a kernel that lost a template parameter).  One line per object: the counts, then the names of the functions that differ or have no partner.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
LABEL = re.compile(r"^[0-9a-f]+ <(.*)>:$")
LITERAL = re.compile(r"^(s_addc?_u32 \S+ \S+) (0x[0-9a-f]+|-?\d+)$")


def functions(obj, tmp):
    fb, co = os.path.join(tmp, "fatbin"), os.path.join(tmp, "code.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fb}", obj], check=True, stderr=subprocess.DEVNULL)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fb}", f"--targets={TARGET}", f"--output={co}"], check=True)
    text = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-C", co], check=True, capture_output=True, text=True).stdout
    out, body, after_getpc = {}, None, 0
    for line in text.splitlines():
        m = LABEL.match(line)
        if m:
            body = out.setdefault(m.group(1), [])
            continue
        if body is None or not line.startswith("\t"):
            continue
        ins = " ".join(line.split("//")[0].split())
        if ins.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc:
            after_getpc -= 1
            ins = LITERAL.sub(r"\1 <pc-relative>", ins)
        body.append(ins)
    for body in out.values():
        while body and (body[-1].startswith("s_nop") or body[-1].startswith("s_code_end")):
            body.pop()
    return out


def short(name):
    """k_steps<5, 0, 0, 1, 0, 0, 0, 0, 0> of `void (anonymous namespace)::k_steps<5, ...>(StepArgs const*, ...)`: no namespaces, no arguments"""
    name = re.sub(r"\(anonymous namespace\)::|ihm2::|^void ", "", name)
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir_a")
    ap.add_argument("dir_b")
    ap.add_argument("-o", "--out")
    a = ap.parse_args()
    lines = []
    objs = sorted(f for f in os.listdir(a.dir_a) if f.endswith(".o") and os.path.exists(os.path.join(a.dir_b, f)))
    for o in objs:
        with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
            try:
                fa, fb = functions(os.path.join(a.dir_a, o), ta), functions(os.path.join(a.dir_b, o), tb)
            except subprocess.CalledProcessError:
                continue        # no device code in this object
        same = [n for n in fa if n in fb and fa[n] == fb[n]]
        differ = [n for n in fa if n in fb and fa[n] != fb[n]]
        only_a, only_b = [n for n in fa if n not in fb], [n for n in fb if n not in fa]
        renamed = []
        for n in list(only_a):
            twin = next((m for m in only_b if fb[m] == fa[n]), None)
            if twin is not None:
                renamed.append((n, twin)); only_a.remove(n); only_b.remove(twin)
        line = f"{o}: {len(same) + len(renamed)} functions identical, {len(differ)} differ"
        if renamed:
            line += "; identical under a new name: " + ", ".join(f"{short(n)} -> {short(m)}" for n, m in renamed)
        if differ:
            line += "; differ: " + ", ".join(f"{short(n)} ({len(fa[n])} -> {len(fb[n])} instructions)" for n in differ)
        if only_a:
            line += "; only in the first: " + ", ".join(short(n) for n in only_a)
        if only_b:
            line += "; only in the second: " + ", ".join(short(n) for n in only_b)
        lines.append(line)
        print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
