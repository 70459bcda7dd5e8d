#!/usr/bin/env python3
"""Compare the device code of every kernel between a base revision and the working tree.  CPU only.

    python tools/kernel_isa_diff.py BASE_REV [--jobs N] [--keep DIR]

BASE_REV is unpacked with `git archive`.  Every atlaspatch_amd/csrc/*.hip of both trees is compiled to device assembly with
that tree's Makefile flags plus `-S --cuda-device-only` (gemm256.hip a second time under ALT_FLAGS, the A/B twin), the
assembly is split into kernels, and one line per kernel is printed:

    IDENTICAL  the same instruction text in the same order and the same resource fields
    REORDERED  the same resource fields and the same count of every mnemonic other than s_waitcnt / s_nop
    CHANGED    anything else

Exit status 1 when the two trees' kernel name sets differ or any kernel is CHANGED.  The comparison is textual: comments
are dropped, the per-build `__hip_cuid_<hash>` symbol and the per-file function index of local labels are masked.
"""
import argparse
import collections
import concurrent.futures
import os
import re
import shlex
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("atlaspatch_amd", "csrc")
RESOURCE_FIELDS = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")
UNCOUNTED = ("s_waitcnt", "s_nop")


def make_vars(csrc):
    """The Makefile's plain assignments, $(NAME) references expanded."""
    out = {}
    for line in open(os.path.join(csrc, "Makefile")):
        m = re.match(r"^([A-Z_]+)\s*\??=\s*(.*)$", line.rstrip("\n"))
        if m:
            out[m.group(1)] = re.sub(r"\$\((\w+)\)", lambda r: out.get(r.group(1), ""), m.group(2))
    return out


def compile_tree(tree, outdir, jobs):
    """-> {unit: path of its device assembly}; unit = file name, or 'gemm256.hip[alt]' for the twin build."""
    csrc = os.path.join(tree, CSRC)
    mk = make_vars(csrc)
    flags = shlex.split(mk["CXXFLAGS"])
    units = [(f, []) for f in sorted(os.listdir(csrc)) if f.endswith(".hip")]
    units.append(("gemm256.hip", shlex.split(mk["ALT_FLAGS"])))
    os.makedirs(outdir, exist_ok=True)

    def one(unit):
        src, extra = unit
        name = src + ("[alt]" if extra else "")
        dst = os.path.join(outdir, name + ".s")
        cmd = [mk["HIPCC"]] + flags + extra + ["-S", "--cuda-device-only", "-o", dst, src]
        r = subprocess.run(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("%s failed in %s:\n%s" % (" ".join(cmd), csrc, r.stdout))
        return name, dst

    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        return dict(pool.map(one, units))


def split_kernels(path):
    """-> {kernel name: (body lines, {resource field: value})}"""
    text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_", open(path).read())
    lines = text.split("\n")
    resources, name = {}, None
    for line in lines:
        t = line.strip()
        if t.startswith(".amdhsa_kernel "):
            name = t.split()[1]
            resources[name] = {}
        elif t == ".end_amdhsa_kernel":
            name = None
        elif name is not None and t.startswith(".amdhsa_"):
            key, _, value = t[len(".amdhsa_"):].partition(" ")
            if key in RESOURCE_FIELDS:
                resources[name][key] = value.strip()
    kernels, body, name = {}, None, None
    for line in lines:
        t = line.split(";", 1)[0].strip()
        if not t:
            continue
        if body is None:
            if t.endswith(":") and t[:-1] in resources:
                name, body = t[:-1], []
        elif t.startswith(".Lfunc_end"):
            kernels[name] = (body, resources[name])
            body = None
        else:
            body.append(re.sub(r"\.L(BB|JTI|tmp)\d+_", r".L\1_", t))
    missing = set(resources) - set(kernels)
    if missing:
        raise RuntimeError("%s: no body found for %s" % (path, sorted(missing)))
    return kernels


def mnemonic_counts(body):
    c = collections.Counter()
    for t in body:
        if t.startswith(".") or t.endswith(":"):
            continue
        m = t.split()[0]
        if m not in UNCOUNTED:
            c[m] += 1
    return c


def classify(base, new):
    if base[1] != new[1]:
        return "CHANGED", "resources %s -> %s" % (base[1], new[1])
    if base[0] == new[0]:
        return "IDENTICAL", ""
    cb, cn = mnemonic_counts(base[0]), mnemonic_counts(new[0])
    if cb == cn:
        return "REORDERED", ""
    diff = ", ".join("%s %d -> %d" % (m, cb[m], cn[m]) for m in sorted(set(cb) | set(cn)) if cb[m] != cn[m])
    return "CHANGED", diff


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("base_rev")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--keep", metavar="DIR", help="leave the unpacked base tree and both sets of assembly here")
    args = ap.parse_args()

    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        base_tree = os.path.join(work, "base")
        os.makedirs(base_tree, exist_ok=True)
        archive = subprocess.Popen(["git", "-C", ROOT, "archive", args.base_rev, CSRC, "include"], stdout=subprocess.PIPE)
        subprocess.run(["tar", "-x", "-C", base_tree], stdin=archive.stdout, check=True)
        if archive.wait() != 0:
            sys.exit("git archive %s failed" % args.base_rev)
        asm = {"base": compile_tree(base_tree, os.path.join(work, "asm_base"), args.jobs),
               "new": compile_tree(ROOT, os.path.join(work, "asm_new"), args.jobs)}
        kernels = {side: {(unit, k): v for unit, path in units.items() for k, v in split_kernels(path).items()}
                   for side, units in asm.items()}

    base, new = kernels["base"], kernels["new"]
    bad = False
    for key in sorted(set(base) ^ set(new)):
        print("%-9s %s  %s" % ("REMOVED" if key in base else "ADDED", key[0], key[1]))
        bad = True
    totals = collections.Counter()
    for key in sorted(set(base) & set(new)):
        cls, why = classify(base[key], new[key])
        totals[cls] += 1
        print("%-9s %s  %s%s" % (cls, key[0], key[1], "  (" + why + ")" if why else ""))
    print("kernels: base %d, new %d; IDENTICAL %d, REORDERED %d, CHANGED %d"
          % (len(base), len(new), totals["IDENTICAL"], totals["REORDERED"], totals["CHANGED"]))
    sys.exit(1 if bad or totals["CHANGED"] else 0)


if __name__ == "__main__":
    main()
