"""Condense hipcc's `-Rpass-analysis=kernel-resource-usage` remarks into one line per kernel, to compare two builds or to
check that no kernel uses scratch:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Rpass-analysis=kernel-resource-usage -c X.hip -o /dev/null 2> X.remarks
    python scripts/kernel_resources.py X.remarks [--demangle] [--only REGEX] [--families]

Each line: kernel, VGPRs, AGPRs, SGPRs, scratch bytes per lane, LDS bytes, occupancy.  `--families` groups the kernels by
template name and prints the range of every figure instead.
"""
import argparse
import collections
import re
import subprocess
import sys

FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("SGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("LDS Size [bytes/block]", "lds"), ("Occupancy [waves/SIMD]", "occ"))


def parse(path):
    out, cur = collections.OrderedDict(), None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def demangle(names):
    res = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return res.stdout.split("\n")[:len(names)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("remarks")
    ap.add_argument("--demangle", action="store_true")
    ap.add_argument("--only", default=None, help="keep kernels whose (demangled) name matches this regex")
    ap.add_argument("--families", action="store_true")
    a = ap.parse_args()
    ks = parse(a.remarks)
    names = list(ks)
    shown = demangle(names) if a.demangle or a.families else names
    rows = [(s, ks[n]) for n, s in zip(names, shown) if not a.only or re.search(a.only, s)]
    keys = [k for _, k in FIELDS]
    if a.families:
        fam = collections.OrderedDict()
        for s, r in rows:
            # a family: the kernel's name and its leading type arguments (up to the first number or bool)
            m = re.match(r"(?:void )?([\w:]+)<(.*?)>\(", s)
            if m:
                types = []
                for arg in m.group(2).split(", "):
                    if re.fullmatch(r"\d+|true|false", arg):
                        break
                    types.append(arg)
                s = f"{m.group(1)}<{', '.join(types + ['...'])}>"
            fam.setdefault(s, []).append(r)
        for f, rs in fam.items():
            print(f"{f}  kernels={len(rs)}  " + "  ".join(
                f"{k}={min(r.get(k, 0) for r in rs)}..{max(r.get(k, 0) for r in rs)}" for k in keys))
    else:
        for s, r in rows:
            print(s + "  " + "  ".join(f"{k}={r.get(k, 0)}" for k in keys))
    bad = [s for s, r in rows if r.get("scratch", 0)]
    print(f"# {len(rows)} kernels, {len(bad)} with scratch", file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
