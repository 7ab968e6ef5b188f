"""Static instruction counts of the cplxfn.hip kernels, read from the code object's assembly.

    python scripts/cplxfn_isa.py          (compiles csrc/cplxfn.hip with --save-temps into a temporary directory)

Per kernel: all instructions and the vector-ALU ones (v_*, of which transcendental: v_exp / v_log / v_rcp / v_rsq /
v_sqrt / v_sin / v_cos _f32), divided by the elements one loop iteration handles (4 float32, 8 bf16).  The count covers the
whole kernel -- the scalar tail and the rarely taken branches (large-argument range reduction of sin / cos / tan,
|t| > 88 in cosh / sinh) included -- so it is an upper bound of the work per element; the executed count comes from
the SQ_INSTS_VALU counter (profiles/r07_cplxfn.txt).
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "cplxmodule_amd", "csrc", "cplxfn.hip")
FUNCTIONS = ("exp", "log", "sin", "cos", "tan", "sinh", "cosh", "tanh")
TRANSCENDENTAL = re.compile(r"v_(exp|log|rcp|rsq|sqrt|sin|cos)_f32")


def main():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-value", "--save-temps",
                        "-c", SRC, "-o", os.path.join(d, "cplxfn.o")], cwd=d, check=True, stderr=subprocess.DEVNULL)
        asm = open(os.path.join(d, "cplxfn-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    print(f"{'kernel':<14}{'insts':>7}{'valu':>7}{'transc':>8}{'valu/elt':>10}")
    for m in re.finditer(r"^(_ZN7cplxamd14cplx_fn_kernelI(f|t)Li(\d)ELb(\d)\w*):.*?$(.*?)^\.Lfunc_end", asm, re.M | re.S):
        _, t, fn, bwd, body = m.groups()
        insts = [ln.strip() for ln in body.splitlines()]
        insts = [ln for ln in insts if ln and re.match(r"[sv]_|global_|buffer_|flat_|ds_", ln)]
        valu = [ln for ln in insts if ln.startswith("v_")]
        per = 4 if t == "f" else 8
        name = f"{'f32' if t == 'f' else 'bf16'} {FUNCTIONS[int(fn)]} {'bwd' if bwd == '1' else 'fwd'}"
        print(f"{name:<14}{len(insts):>7}{len(valu):>7}{sum(bool(TRANSCENDENTAL.match(v)) for v in valu):>8}"
              f"{len(valu) / per:>10.1f}")


if __name__ == "__main__":
    sys.exit(main())
