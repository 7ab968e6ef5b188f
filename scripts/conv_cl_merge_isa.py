#!/usr/bin/env python
"""Compare the gfx950 machine code of the channels-last convolution kernels with that of a parent commit.

A one-off record for the merge of conv_cl_real.hip into conv_cl.hip and of conv_cl_wgrad_real.hip into conv_cl_wgrad.hip
(it produced profiles/conv_cl_merge_isa.txt), not a tool to reuse: the parent revision, its file names and its kernel names
are fixed below.  The complex and the real kernels are now instantiations of one source; this script shows which kernels
the merge left instruction for instruction as they were and what moved in the others: it compiles the kernel sources of
a parent revision (taken with `git show`) and of the working tree for the device only, with the flags of csrc/build.sh,
splits the assembly per kernel, normalises what cannot be equal (see `normalise`) and compares kernel by kernel, code and
resource blocks alike.

    python scripts/conv_cl_merge_isa.py [--parent REV] [--out profiles/conv_cl_merge_isa.txt]

Needs hipcc and c++filt; no GPU.  Exit status 1 if a kernel differs.
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "cplxmodule_amd/csrc"
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-unused-value --cuda-device-only -S".split()
SOURCES = ["conv_cl.hip", "conv_cl_real.hip", "conv_cl_wgrad.hip", "conv_cl_wgrad_real.hip", "conv_cl_wgrad_f16.hip"]

# (label, regular expression on the demangled name in the parent, ... in the result)
KERNELS = [
    ("complex forward / dgrad", r"cl::conv_cl_kernel<3>", r"cl::conv_cl_kernel<3, true>"),
    ("real forward / dgrad", r"clr::conv_clr_kernel<3>", r"cl::conv_cl_kernel<3, false>"),
    ("complex pack", r"cl::pack_kernel\(", r"cl::pack_kernel<true>"),
    ("real pack", r"clr::pack_kernel\(", r"cl::pack_kernel<false>"),
    ("complex wgrad", r"clw::conv_cl_wgrad_kernel<false>", r"clw::conv_cl_wgrad_kernel<true, false>"),
    ("complex wgrad, FOLD", r"clw::conv_cl_wgrad_kernel<true>", r"clw::conv_cl_wgrad_kernel<true, true>"),
    ("real wgrad", r"clwr::conv_clr_wgrad_kernel", r"clw::conv_cl_wgrad_kernel<false, false>"),
    ("complex wgrad reduce", r"clw::wgrad_reduce_kernel\(", r"clw::wgrad_reduce_kernel<true>"),
    ("real wgrad reduce", r"clwr::wgrad_reduce_kernel\(", r"clw::wgrad_reduce_kernel<false>"),
    ("half-operand complex wgrad", r"clwh::conv_cl_wgrad_kernel<false>", r"clwh::conv_cl_wgrad_kernel<true, false>"),
    ("half-operand complex wgrad reduce", r"clwh::wgrad_reduce_kernel\(", r"clwh::wgrad_reduce_kernel<true>"),
]


def tool(name):
    for d in (os.environ.get("ROCM_PATH", "/opt/rocm") + "/bin", os.environ.get("ROCM_PATH", "/opt/rocm") + "/llvm/bin"):
        if os.path.exists(os.path.join(d, name)):
            return os.path.join(d, name)
    return name


def compile_tree(tree, out):
    """tree: a directory with include/cplxamd.h and cplxmodule_amd/csrc; returns the assembly of every source present"""
    procs = []
    for f in SOURCES:
        if os.path.exists(os.path.join(tree, CSRC, f)):
            s = os.path.join(out, f[:-4] + ".s")
            procs.append((s, subprocess.Popen([os.environ.get("HIPCC", tool("hipcc"))] + FLAGS + [f, "-o", s],
                                              cwd=os.path.join(tree, CSRC), stderr=subprocess.PIPE, text=True)))
    text = ""
    for s, p in procs:
        err = p.communicate()[1]
        if p.returncode:
            sys.exit(err)
        text += open(s).read()
    return text


def checkout(rev, dst):
    names = subprocess.run(["git", "ls-tree", "--name-only", rev, CSRC + "/", "include/cplxamd.h"], cwd=ROOT, check=True,
                           capture_output=True, text=True).stdout.split()
    for n in names:
        if n.endswith((".h", ".hip")):
            os.makedirs(os.path.dirname(os.path.join(dst, n)), exist_ok=True)
            with open(os.path.join(dst, n), "wb") as f:
                f.write(subprocess.run(["git", "show", rev + ":" + n], cwd=ROOT, check=True, capture_output=True).stdout)


def normalise(name, lines):
    """What is dropped or renamed: the kernel's mangled name (-> KERNEL), comment lines and trailing comments, .file /
    .ident, the function index in local labels (.LBB<n>_, .Lfunc_end<n>, which counts the kernels of a file), and the
    linkage of the symbol (.globl / .weak and the .section / .text switches around it: a kernel that became a template
    instantiation lives in a COMDAT section of its own)."""
    out = []
    for l in lines:
        l = l.replace(name, "KERNEL")
        l = re.sub(r"\s*;.*$", "", l).rstrip()
        l = re.sub(r"\.LBB\d+_", ".LBB_", l)
        l = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", l)
        if not l.strip() or re.match(r"\s*\.(file|ident|globl|weak|text|section)\b", l):
            continue
        out.append(l)
    return out


def kernels_of(text):
    """mangled name -> normalised lines of (function with its .amdhsa_kernel block and resource .set lines) + (its entry
    in the metadata)"""
    lines = text.split("\n")
    names = sorted({m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel (\S+)", l)] if m})
    out = {n: [] for n in names}
    cur = None                     # the kernel whose function the lines belong to
    meta = None                    # the metadata entry being collected

    def close(meta):
        for l in meta or []:
            m = re.match(r"\s*\.name:\s+(\S+)", l)
            if m:
                out[m.group(1)] += ["METADATA"] + meta

    for l in lines:
        m = re.match(r"\s*\.protected\s+(\S+)", l)
        if m and m.group(1) in out:
            cur = m.group(1)
        elif re.match(r"\s*\.p2alignl|\s*\.section\s+\.AMDGPU\.gpr_maximums", l):
            cur = None
        elif re.match(r"  - \.agpr_count", l):
            close(meta)
            meta = []
        elif re.match(r"amdhsa\.target", l):
            close(meta)
            meta = None
        if cur is not None:
            out[cur].append(l)
        if meta is not None:
            meta.append(l)
    return {n: normalise(n, body) for n, body in out.items()}


def demangle(names):
    r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.split("\n")))


def find(kernels, dem, pattern):
    hits = [n for n in kernels if re.search(pattern, dem[n])]
    return hits[0] if len(hits) == 1 else None


def figure(body, key):
    for l in body:
        m = re.match(r"\s*(?:- )?\.%s:?\s+(\d+)" % key, l)
        if m:
            return int(m.group(1))
    return -1


HOT = [("v_mfma", r"\s+v_mfma"), ("ds_read", r"\s+ds_read"), ("lds dma", r"\s+buffer_load\S* .*\blds\b"),
       ("s_waitcnt", r"\s+s_waitcnt"), ("s_barrier", r"\s+s_barrier")]


def hot_counts(body):
    """Per stretch of code between two labels: how many of each instruction class of HOT it holds (stretches without any
    are left out, so that a renumbered or an empty block does not count as a difference)."""
    out, cur = [], [0] * len(HOT)
    for l in body:
        if l == "METADATA":
            break
        if re.match(r"\.LBB_\d+:", l):
            if any(cur):
                out.append(tuple(cur))
            cur = [0] * len(HOT)
        for i, (_, pat) in enumerate(HOT):
            cur[i] += bool(re.match(pat, l))
    if any(cur):
        out.append(tuple(cur))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", default="59b407e", help="revision to compare the working tree with (default: the last "
                    "commit that had the kernels in separate files)")
    ap.add_argument("--out", default=None, help="write the report here as well")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(tmp + "/parent_s")
        os.makedirs(tmp + "/result_s")
        checkout(a.parent, tmp + "/parent")
        par = kernels_of(compile_tree(tmp + "/parent", tmp + "/parent_s"))
        res = kernels_of(compile_tree(ROOT, tmp + "/result_s"))
    dp, dr = demangle(list(par)), demangle(list(res))
    rev = subprocess.run(["git", "rev-parse", "--short", a.parent], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    rep = ["conv_cl kernels, gfx950 assembly: working tree against %s" % rev, "flags: " + " ".join(FLAGS), ""]
    bad = 0
    for label, pp, pr in KERNELS:
        kp, kr = find(par, dp, pp), find(res, dr, pr)
        if kp is None or kr is None:
            rep.append("%-36s MISSING (parent: %s, result: %s)" % (label, kp, kr))
            bad += 1
            continue
        x, y = par[kp], res[kr]
        same = x == y
        bad += not same
        res_of = lambda b: tuple(figure(b, k) for k in (  # noqa: E731
            "vgpr_count", "agpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size",
            "vgpr_spill_count", "sgpr_spill_count"))
        rep.append("%-36s %5d lines  vgpr %3d  agpr %d  sgpr %3d  static lds %d  scratch %d  vgpr spills %d  sgpr -> vgpr-lane "
                   "spills %d   %s" % ((label, len(y)) + res_of(y) + ("identical" if same else "DIFFERENT",)))
        rep.append("    parent: %s\n    result: %s" % (dp[kp], dr[kr]))
        if not same:
            rep.append("    registers / LDS / scratch / spills as the parent's: %s;  v_mfma / ds_read / LDS-DMA / s_waitcnt / "
                       "s_barrier per stretch between labels as the parent's: %s (%d stretches)" % (
                           "yes" if res_of(x) == res_of(y) else "NO %s" % (res_of(x),),
                           "yes" if hot_counts(x) == hot_counts(y) else "NO", len(hot_counts(y))))
            rep += ["    " + l for l in difflib.unified_diff(x, y, "parent", "result", lineterm="", n=2)]
    extra = sorted(set(dr.values()) - {dr[k] for _, _, pr in KERNELS for k in [find(res, dr, pr)] if k})
    rep += ["", "other kernels in the result's sources (not compared): " + (", ".join(extra) or "none")]
    text = "\n".join(rep) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
