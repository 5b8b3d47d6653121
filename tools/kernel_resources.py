#!/usr/bin/env python3
"""Resource table of the kernels of one or more sources of diffnet_amd/csrc, from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage under the flags of diffnet_amd/build.py): VGPRs, AGPRs, SGPRs, scratch, VGPR spills, occupancy, LDS.
Nothing is linked or run.  Exit status 1 when a kernel has scratch or spills.

Usage: python tools/kernel_resources.py eikonal3d.hip eikonal3d_g3.hip eikonal3d_g4.hip [--extra-flags "..."]
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from diffnet_amd import build as B  # noqa: E402

FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"), ("VGPRs Spill", "spill"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))


def resources(src, extra=()):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [B._hipcc(), *B.FLAGS, *extra, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, src), "-o", os.path.join(tmp, "a.o")]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, check=True).stdout
    rows, cur = [], None
    for line in out.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        key, val = m.group(1).strip(), m.group(2)
        if key == "Function Name":
            name = subprocess.run(["c++filt", val], stdout=subprocess.PIPE, text=True).stdout.strip() or val
            cur = {"name": re.sub(r"\(.*", "", name.replace("void dn::", ""))}
            rows.append(cur)
        elif cur is not None:
            for k, short in FIELDS:
                if key == k:
                    cur[short] = int(val)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--extra-flags", default="")
    a = ap.parse_args()
    bad = 0
    print(f"{'kernel':<64} {'VGPR':>5} {'AGPR':>5} {'SGPR':>5} {'scratch':>8} {'spill':>6} {'occ':>4} {'LDS':>6}")
    for src in a.sources:
        for r in sorted(resources(src, a.extra_flags.split()), key=lambda r: r["name"]):
            print(f"{r['name']:<64} {r['vgpr']:>5} {r['agpr']:>5} {r['sgpr']:>5} {r['scratch']:>8} {r['spill']:>6} {r['occ']:>4} {r['lds']:>6}")
            bad += r["scratch"] != 0 or r["spill"] != 0
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
