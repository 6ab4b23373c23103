#!/usr/bin/env python3
"""What the compiler made of the kernels of one translation unit: registers, LDS, scratch and occupancy per instantiation, from
hipcc's kernel-resource-usage remarks. Cross-compiles for gfx950; needs no GPU.

    python tools/kernel_resources.py multiscan.hip --match scan_multi_pooled_kernel --out profiles/r16/pooled_scan_resources.json
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wax_amd import build as wb  # noqa: E402

FIELDS = {"vgprs": "VGPRs", "agprs": "AGPRs", "sgprs": "TotalSGPRs", "scratch_bytes_per_lane": "ScratchSize [bytes/lane]",
          "sgpr_spills": "SGPRs Spill", "vgpr_spills": "VGPRs Spill", "occupancy_waves_per_simd": "Occupancy [waves/SIMD]",
          "static_lds_bytes": "LDS Size [bytes/block]"}


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return names
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return out[:len(names)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", help="a .hip file of wax_amd/csrc")
    ap.add_argument("--match", default="", help="keep kernels whose demangled name contains this")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [wb._hipcc(), f"--offload-arch={wb.ARCH}", "-O3", "-std=c++17", "-fPIC", "-I" + os.path.join(ROOT, "include"),
               "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(wb.CSRC, args.source), "-o", os.path.join(tmp, "unit.o")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    blocks = re.split(r"remark: [^\n]*?Function Name: ", text)[1:]
    names = demangle([b.split(" ")[0] for b in blocks])
    rows = []
    for name, b in zip(names, blocks):
        if args.match not in name:
            continue
        row = {"kernel": name}
        for key, label in FIELDS.items():
            row[key] = int(re.search(re.escape(label) + r": (\d+)", b).group(1))
        rows.append(row)
    rows.sort(key=lambda r: r["kernel"])
    doc = {"source": args.source, "arch": wb.ARCH, "flags": "-O3 -std=c++17", "kernels": rows}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    for r in rows:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
