#!/usr/bin/env python3
"""Registers, spills, scratch, LDS and occupancy of every kernel of the given HIP files, as the compiler reports them
(-Rpass-analysis=kernel-resource-usage, gfx950, the library's flags), one markdown table row per kernel, sorted by name.
Run it in two checkouts and diff the outputs to see whether a change moved a kernel it did not mean to touch:

  python tools/kernel_resource_usage.py loam_livox_amd/csrc/ll_reg_*_kernels.hip > after.md
"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def kernels_of(src):
    from loam_livox_amd import build
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.hipcc()] + build.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "x.o")]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, check=True).stdout.decode(errors="replace")
    table, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"remark:\s*(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(":")
        if key == "Function Name":
            cur = table.setdefault(val.strip(), {})
        elif cur is not None:
            cur[key.strip()] = val.strip()
    return table


def main():
    rows = {}
    for src in sys.argv[1:]:
        rows.update(kernels_of(src))
    names = subprocess.run(["c++filt"], input="\n".join(rows).encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    print("| kernel | " + " | ".join(FIELDS) + " |")
    print("|---" * (len(FIELDS) + 1) + "|")
    for name, mangled in sorted(zip(names, rows)):
        short = re.sub(r"\(.*", "", name).replace("void ", "").replace("ll::", "")
        print(f"| `{short}` | " + " | ".join(rows[mangled].get(f, "") for f in FIELDS) + " |")


if __name__ == "__main__":
    main()
