#!/usr/bin/env python3
"""Compare the gfx950 device code of the exact-distance kernel units between two git revisions, kernel by kernel.

    python tools/compare_kernels.py REV_A REV_B [--units kernels.hip,batch.hip] [--keep DIR]

Each revision is checked out into a temporary worktree and every unit is compiled with the library's flags plus
`--cuda-device-only -S -cuid=<fixed>` (needs hipcc, no GPU). REV_B may be `WORKTREE`: the files as they are on disk.
One line per kernel (and per out-of-line device function): `identical`, or `DIFFERENT` with both resource lines
(VGPRs, AGPR offset, SGPRs, LDS bytes, scratch bytes). Comments are dropped and local labels renumbered per function, so a
kernel that only moved inside its file compares equal. Exit status 1 if anything differs.
`--renamed OLD=NEW` (demangled names, repeatable) compares REV_A's OLD with REV_B's NEW: a kernel that became one instantiation of a
template keeps its instructions under another symbol. Every mention of either symbol inside the text is replaced by one token first.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = ["kernels.hip", "mirror_scan.hip", "multiscan.hip", "batch.hip"]
RESOURCES = [("vgpr", ".amdhsa_next_free_vgpr"), ("accum_offset", ".amdhsa_accum_offset"), ("sgpr", ".amdhsa_next_free_sgpr"),
             ("lds", ".amdhsa_group_segment_fixed_size"), ("scratch", ".amdhsa_private_segment_fixed_size")]
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    sys.exit("hipcc not found")


def compile_unit(tree, unit, out):
    cmd = [hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(tree, "include"),
           "--cuda-device-only", "-S", "-cuid=compare", os.path.join(tree, "wax_amd", "csrc", unit), "-o", out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    return out


def parse(path):
    """-> {function: (normalised instruction text, normalised .amdhsa block or None, {resource: value})}"""
    body, hsa, cur, lines = {}, {}, None, open(path).read().splitlines()
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"\s*\.type\s+(\S+),@function", ln)
        if m:
            cur, body[m.group(1)] = m.group(1), []
        elif cur is not None:
            if re.match(r"\.Lfunc_end\d+:", ln):
                cur = None
            else:
                body[cur].append(ln)
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            hsa[m.group(1)] = [x.strip() for x in lines[i + 1:j]]
            i = j
        i += 1
    out = {}
    for name, text in body.items():
        names = {}
        text = [t.split(";")[0].rstrip() for t in text if "__hip_cuid" not in t]   # comments name block numbers of the whole unit
        text = [t for t in text if t]
        norm = "\n".join(LABEL.sub(lambda mm: names.setdefault(mm.group(0), ".L%d" % len(names)), t) for t in text)
        block = hsa.get(name)
        res = {}
        for key, directive in RESOURCES:
            for x in block or []:
                if x.split()[0] == directive:
                    res[key] = x.split()[1]
        out[name] = (norm, "\n".join(block) if block is not None else None, res)
    return out


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt:
        return {n: n for n in names}
    res = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, res))


def fmt(res):
    return " ".join("%s=%s" % (k, res.get(k, "-")) for k, _ in RESOURCES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rev_a")
    ap.add_argument("rev_b")
    ap.add_argument("--units", default=",".join(UNITS))
    ap.add_argument("--keep", default=None, help="keep the .s files in this directory")
    ap.add_argument("--renamed", action="append", default=[], metavar="OLD=NEW", help="REV_A's kernel OLD is REV_B's kernel NEW (demangled names)")
    args = ap.parse_args()
    units = args.units.split(",")
    work = tempfile.mkdtemp(prefix="compare_kernels.")
    trees, added = {}, []
    try:
        for side, rev in (("a", args.rev_a), ("b", args.rev_b)):
            if rev == "WORKTREE":
                trees[side] = ROOT
            else:
                trees[side] = os.path.join(work, "tree_" + side)
                subprocess.run(["git", "-C", ROOT, "worktree", "add", "--detach", trees[side], rev], check=True, capture_output=True)
                added.append(trees[side])
        jobs = [(side, u) for side in "ab" for u in units]
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 2, 16)) as pool:
            outs = list(pool.map(lambda j: compile_unit(trees[j[0]], j[1], os.path.join(work, "%s_%s.s" % (j[0], j[1]))), jobs))
        if args.keep:
            os.makedirs(args.keep, exist_ok=True)
            for o in outs:
                shutil.copy(o, args.keep)
        print("# %s -> %s" % (args.rev_a, args.rev_b))
        differ = 0
        for u in units:
            a, b = parse(os.path.join(work, "a_%s.s" % u)), parse(os.path.join(work, "b_%s.s" % u))
            pretty = demangle(sorted(set(a) | set(b)))
            for pair in args.renamed:
                old, new = pair.split("=", 1)
                olds = [m for m in a if old in pretty[m] and m not in b]       # (demangled names carry the signature: match by substring)
                news = [m for m in b if new in pretty[m] and m not in a]
                if len(olds) == 1 and len(news) == 1:
                    # one entry under the old symbol on both sides. Made equal first: the symbol's own mentions, the section directive
                    # (a template's instantiation sits in a comdat section of its own) and the kernel-argument size, which is printed
                    # beside the name when it changed (a trailing argument the old kernel does not read)
                    def strip(t):
                        if t is None:
                            return None
                        t = t.replace(news[0], "@KERNEL").replace(olds[0], "@KERNEL")
                        return "\n".join(x for x in t.split("\n") if x.split()[:1] not in ([".text"], [".section"], [".amdhsa_kernarg_size"]))
                    karg = [[x.split()[1] for x in (t[1] or "").split("\n") if x.startswith(".amdhsa_kernarg_size")] for t in (a[olds[0]], b[news[0]])]
                    a[olds[0]] = (strip(a[olds[0]][0]), strip(a[olds[0]][1]), a[olds[0]][2])
                    b[olds[0]] = (strip(b[news[0]][0]), strip(b[news[0]][1]), b[news[0]][2])
                    del b[news[0]]
                    if karg[0] != karg[1]:
                        new += "; kernarg bytes %s -> %s" % ("".join(karg[0]), "".join(karg[1]))
                    pretty[olds[0]] = "%s  (now %s)" % (old, new)
            same = 0
            print("## %s: %d functions before, %d after" % (u, len(a), len(b)))
            for name in sorted(set(a) | set(b), key=lambda n: pretty[n]):
                if name not in a or name not in b:
                    differ += 1
                    print("%s  %s" % ("ONLY-AFTER " if name not in a else "ONLY-BEFORE", pretty[name]))
                elif a[name][:2] == b[name][:2]:
                    same += 1
                    print("identical    %s" % pretty[name])
                else:
                    differ += 1
                    what = "code" if a[name][0] != b[name][0] else "descriptor"
                    print("DIFFERENT    %s\n    (%s) before: %s\n    %s  after: %s" %
                          (pretty[name], what, fmt(a[name][2]), " " * len(what), fmt(b[name][2])))
            print("## %s: %d identical, %d not" % (u, same, len(set(a) | set(b)) - same))
        return 1 if differ else 0
    finally:
        for t in added:
            subprocess.run(["git", "-C", ROOT, "worktree", "remove", "--force", t], check=False, capture_output=True)
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    sys.exit(main())
