#!/usr/bin/env python3
"""Compare the device code of two builds of one source file, kernel by kernel.

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --save-temps -c xcorr.hip     (once per tree)
    python profiles/isa_compare.py OLD/xcorr-hip-amdgcn-amd-amdhsa-gfx950.s NEW/xcorr-hip-amdgcn-amd-amdhsa-gfx950.s

For every kernel of OLD the script finds the kernel of NEW with the same name and checks that its instruction sequence,
its `.amdhsa_*` descriptor (VGPR/AGPR/SGPR counts, LDS, scratch ...) and its resource `.set` lines are identical.  Symbol
names are replaced by a placeholder and local labels (.LBB, .Ltmp, .Lfunc_end) are renumbered in order of appearance, so two
builds that differ only in where a kernel sits in the file or in how it is mangled compare equal.  Linkage directives
(.globl / .weak, comdat sections) are not compared.

Names are matched after demangling with `--drop-int-arg V`: a leading integer template argument V is dropped (the old
timing-only `ABL` parameter was 0 in every shipped launch: `xcorr_fused_kernel<0, true>` matches `xcorr_fused_kernel<true>`).
Exit status 0 when every kernel of OLD is present in NEW and identical, and NEW has no kernel that OLD lacks.
"""
import argparse
import re
import shutil
import subprocess
import sys

LABEL = re.compile(r"\.(LBB\d+_\d+|Ltmp\d+|Lfunc_end\d+|Lfunc_begin\d+)\b")


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return out.splitlines()


def kernels(path):
    """{mangled name: [lines from its .type directive up to the next kernel's or the file's metadata block]}"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+([^,]+),@function", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.strip().startswith(".amdgpu_metadata"):
            cur = None
        if cur is not None:
            cur.append(line.rstrip("\n"))
    return out


def normalise(name, lines):
    """(instructions and labels, .amdhsa_* lines, resource .set lines) with the symbol and local labels made neutral"""
    labels = {}
    def relabel(m):
        return ".L%d" % labels.setdefault(m.group(1), len(labels))
    code, desc, res = [], [], []
    for line in lines:
        line = LABEL.sub(relabel, line.replace(name, "@K")).split(";")[0].rstrip()
        s = line.strip()
        if not s:
            continue
        if s.startswith(".amdhsa_"):
            desc.append(s)
        elif s.startswith(".set @K."):
            res.append(s)
        elif s.endswith(":") or not s.startswith("."):
            code.append(s)
    return code, desc, res


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--drop-int-arg", default="0", help="leading integer template argument to ignore in names (default 0)")
    a = ap.parse_args()
    ko, kn = kernels(a.old), kernels(a.new)

    def key(dm):
        dm = re.sub(r"^void ", "", dm)
        v = re.escape(a.drop_int_arg)
        return re.sub(r"<%s>" % v, "", re.sub(r"<%s, " % v, "<", dm))

    keys_o = dict(zip((key(d) for d in demangle(list(ko))), ko))
    keys_n = dict(zip((key(d) for d in demangle(list(kn))), kn))
    bad = 0
    for k, mo in keys_o.items():
        mn = keys_n.get(k)
        if mn is None:
            print("MISSING  %s" % k)
            bad += 1
            continue
        co, do, ro = normalise(mo, ko[mo])
        cn, dn, rn = normalise(mn, kn[mn])
        what = [w for w, x, y in (("instructions", co, cn), ("descriptor", do, dn), ("resources", ro, rn)) if x != y]
        print("%-9s%s  (%d instructions)" % ("DIFFERS" if what else "same", k, sum(1 for c in co if not c.endswith(":"))) +
              ("  " + ", ".join(what) if what else ""))
        bad += bool(what)
    for k in keys_n.keys() - keys_o.keys():
        print("NEW      %s" % k)
        bad += 1
    print("%d kernels compared, %d problems" % (len(keys_o), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
