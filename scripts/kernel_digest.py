#!/usr/bin/env python3
"""Digest of every device function of libmarinenav_hip.so: prints `file  kernel  md5`.

A pull request that must not touch a kernel's machine code runs this at its parent and at its head and diffs the two
outputs (sort them first if a kernel moved to another translation unit: the mangled name is the key).

Each translation unit of csrc/Makefile is compiled device-only to assembly with the flags the Makefile gives it (taken
from `make -n -B`).  A function's text runs from its label (`^_Z\\w+:`) through its kernel descriptor and resource
comment block; the file's trailer (metadata of all kernels, the per-compilation `__hip_cuid` symbol) belongs to nobody.
Local labels carry the function's index within its file (`.LBB7_2`, `.Lfunc_end7`, `Header=BB7_10` in loop comments); the
index is dropped and runs of blanks are collapsed, so a kernel hashes the same wherever it stands in whichever file.
"""
import hashlib, os, re, shlex, subprocess, sys, tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distributional_rl_navigation_amd", "csrc")
LABEL = re.compile(r"^(_Z\w+):")
LOCAL = re.compile(r"(\.L(?:BB|func_begin|func_end|JTI|tmp)|\bBB)\d+")


def functions(asm):
    """{mangled name: text} of one assembly file."""
    out, name, ended = {}, None, False
    for line in asm.splitlines():
        m = LABEL.match(line)
        if m:
            name, ended = m.group(1), False
            out[name] = []
        elif name and (line.startswith("\t.section\t.AMDGPU.gpr_maximums") or (ended and line.startswith("\t.section\t.text"))):
            name = None
        if name and "__hip_cuid" not in line:
            ended = ended or "-- End function" in line
            out[name].append(" ".join(LOCAL.sub(r"\1", line).split()))      # (comment columns move with a label's width)
    return {k: "\n".join(v) for k, v in out.items()}


def main():
    plan = subprocess.run(["make", "-n", "-B", "-C", CSRC], check=True, capture_output=True, text=True).stdout
    with tempfile.TemporaryDirectory() as tmp:
        for cmd in plan.splitlines():
            argv = shlex.split(cmd)
            if "-c" not in argv:
                continue
            src = argv[argv.index("-c") + 1]
            asm = os.path.join(tmp, src + ".s")
            argv[argv.index("-c"):] = ["--cuda-device-only", "-S", src, "-o", asm]
            subprocess.run(argv, check=True, cwd=CSRC, stderr=subprocess.DEVNULL)
            with open(asm) as f:
                for name, text in sorted(functions(f.read()).items()):
                    print(f"{src}  {name}  {hashlib.md5(text.encode()).hexdigest()}", flush=True)


if __name__ == "__main__":
    sys.exit(main())
