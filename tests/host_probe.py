"""Build and run a stand-alone host probe of tools/probes: a program with its own main, run on the CPU.  The C++ probes are compiled with
the address and undefined-behaviour sanitizers and every warning an error; the one C probe (a numerical comparison with libm) with the
flags its call names and nothing else."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ihm2_amd", "csrc")
COMPILER = {"c++": ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", CSRC],
            "c": ["gcc"]}


def build(name, tmp_dir, defines=(), extra=(), lang="c++"):
    """tools/probes/<name> (the extension may be left out) -> the executable in tmp_dir.  defines: "NAME=value" strings; extra: flags
    of this probe alone, behind the common ones."""
    src = os.path.join(ROOT, "tools", "probes", name if "." in name else name + {"c++": ".cpp", "c": ".c"}[lang])
    exe = os.path.join(str(tmp_dir), os.path.splitext(os.path.basename(src))[0])
    libs = [f for f in extra if f.startswith("-l")]
    subprocess.check_call(COMPILER[lang] + ["-D" + d for d in defines] + [f for f in extra if f not in libs] + ["-o", exe, src] + libs)
    return exe


def run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True)


def passed(out, prefix=""):
    """exit 0 and the last line "all checks passed", behind the probe's own prefix where it prints one"""
    lines = out.stdout.splitlines()
    return out.returncode == 0 and bool(lines) and lines[-1] == prefix + "all checks passed"


def tail(out):
    return out.stdout[-4000:] + out.stderr[-4000:]
