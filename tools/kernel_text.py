#!/usr/bin/env python3
"""Compare the device instruction text of two source trees, kernel by kernel.

    tools/kernel_text.py <tree-a> <tree-b> [--probes] [--only gemm_bf16,gemm_f16] [--jobs N]

Every l4p_amd/csrc/*.hip of both trees is compiled to gfx950 assembly (device side only) with the flags the tree's own Makefile
gives that file (`make -n`, with -c replaced by -S --cuda-device-only; --probes adds PROBES=1).  A function is the text from its
`.type <name>,@function` to its `.size <name>` line, which includes the kernel descriptor (.amdhsa_kernel block).  Comments are
stripped and the ordinals of local labels (.LBB<n>_<m>, .Ltmp<n>, .Lfunc_end<n>, ...) are normalised; nothing else is touched.
Prints, per translation unit, how many functions are identical and names the ones that differ or exist on one side only.
It only diffs two trees: it looks for nothing inside the text.  Exit status 1 if anything differs.  No GPU is needed.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

LABEL = re.compile(r"\.L(BB|tmp|func_begin|func_end|JTI|CPI|_unnamed_)\d+")


def commands(tree, probes, out_dir):
    """{unit: argv} from the tree's Makefile: its compile line per .hip, turned into an assembly-only device compile"""
    csrc = os.path.join(tree, "l4p_amd", "csrc")
    make = ["make", "-n", "-B", "-C", csrc, "ISA_LINT=0", "OBJ=" + out_dir, "PROBES=%d" % probes]
    cmds = {}
    for line in subprocess.run(make, check=True, capture_output=True, text=True).stdout.splitlines():
        m = re.search(r"^(\S*hipcc .*) -c (\S+)\.hip -o \S+", line)
        if m:
            cmds[m.group(2)] = m.group(1).split() + ["-S", "--cuda-device-only", m.group(2) + ".hip", "-o", os.path.join(out_dir, m.group(2) + ".s")]
    return csrc, cmds


def functions(path):
    """{name: normalised text} of every function in an assembly file"""
    out, name, body = {}, None, []
    for raw in open(path):
        line = LABEL.sub(lambda m: ".L" + m.group(1), raw.split(";")[0].rstrip())
        if not line.strip():
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            name, body = m.group(1), []
        if name is not None:
            body.append(line)
            if re.match(r"\s*\.size\s+" + re.escape(name) + ",", line):
                out[name], name = "\n".join(body), None
    return out


def build(tree, probes, only, jobs, out_dir):
    out_dir = os.path.abspath(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    csrc, cmds = commands(tree, probes, out_dir)
    units = sorted(u for u in cmds if not only or u in only)
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        runs = list(pool.map(lambda u: subprocess.run(cmds[u], cwd=csrc, capture_output=True, text=True), units))
    for u, r in zip(units, runs):
        if r.returncode != 0:
            sys.exit("%s: %s.hip does not compile:\n%s" % (tree, u, r.stderr))
    return {u: functions(os.path.join(out_dir, u + ".s")) for u in units}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("--probes", action="store_true", help="compile with PROBES=1 (-DL4P_PROBE_KERNELS)")
    ap.add_argument("--only", default="", help="comma-separated translation units (default: all)")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    a = ap.parse_args()
    only = set(filter(None, a.only.split(",")))
    with tempfile.TemporaryDirectory() as tmp:
        fa = build(os.path.abspath(a.tree_a), a.probes, only, a.jobs, os.path.join(tmp, "a"))
        fb = build(os.path.abspath(a.tree_b), a.probes, only, a.jobs, os.path.join(tmp, "b"))
    bad = 0
    for u in sorted(set(fa) | set(fb)):
        xa, xb = fa.get(u, {}), fb.get(u, {})
        same = [n for n in xa if xb.get(n) == xa[n]]
        diff = sorted(n for n in xa if n in xb and xb[n] != xa[n])
        only_a, only_b = sorted(set(xa) - set(xb)), sorted(set(xb) - set(xa))
        print("%-16s %4d identical, %d differing, %d only in a, %d only in b" % (u, len(same), len(diff), len(only_a), len(only_b)))
        for tag, names in (("differs", diff), ("only in a", only_a), ("only in b", only_b)):
            for n in names:
                print("    %s: %s (%d / %d lines)" % (tag, n, xa.get(n, "").count("\n"), xb.get(n, "").count("\n")))
        bad += len(diff) + len(only_a) + len(only_b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
