#!/usr/bin/env python3
"""Did a source move change device code?  Compares the gfx950 assembly of two sets of translation units PER SYMBOL: every kernel and
every non-inlined device function's instruction stream (comments and directives stripped, the function's ordinal in its module taken
out of the local labels -- it changes when functions move between files) and every kernel's .amdhsa_* descriptor (registers,
scratch, LDS).  A symbol emitted by several units (a device function two kernels' modules share) is compared as the set of its bodies.

  python tools/compare_kernel_asm.py --emit DIR loam_livox_amd/csrc/ll_reg_*_kernels.hip    # in each checkout: DIR/<unit>.s
  python tools/compare_kernel_asm.py PARENT_DIR CHILD_DIR                                    # exit status 1 on any difference
"""
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ORDINAL = re.compile(r"\.(LBB|LJTI|Ltmp|Lfunc_begin|Lfunc_end)\d+")


def emit(out_dir, sources):
    from loam_livox_amd import build
    os.makedirs(out_dir, exist_ok=True)
    rc = 0
    for i in range(0, len(sources), 8):  # at most eight compilers at a time
        procs = [subprocess.Popen([build.hipcc()] + build.FLAGS + ["--cuda-device-only", "-S", src, "-o",
                                                                  os.path.join(out_dir, os.path.basename(src).replace(".hip", ".s"))]) for src in sources[i:i + 8]]
        rc = max([rc] + [p.wait() for p in procs])
    return rc


def symbols_of(asm_dir):
    """{symbol: set of (body, descriptor)} over every .s file of the directory"""
    table = {}
    for path in sorted(glob.glob(os.path.join(asm_dir, "*.s"))):
        text = open(path).read()
        desc = {m.group(1): "\n".join(sorted(l.strip() for l in m.group(2).splitlines() if ".amdhsa_" in l))
                for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S)}
        for m in re.finditer(r"\.type\s+(\S+),@function\n(.*?)\n\.Lfunc_end\d+:", text, re.S):
            body = []
            for line in m.group(2).splitlines():
                line = ORDINAL.sub(r".\1", line.split(";")[0]).strip()
                if line and not (line.startswith(".") and not line.endswith(":")):
                    body.append(line)
            table.setdefault(m.group(1), set()).add(("\n".join(body), desc.get(m.group(1), "")))
    return table


def main():
    if len(sys.argv) < 3 or (sys.argv[1] == "--emit" and len(sys.argv) < 4):
        sys.exit(__doc__)
    if sys.argv[1] == "--emit":
        sys.exit(emit(sys.argv[2], sys.argv[3:]))
    a, b = symbols_of(sys.argv[1]), symbols_of(sys.argv[2])
    bad = sorted(set(a) ^ set(b)) + sorted(s for s in set(a) & set(b) if a[s] != b[s])
    for s in bad:
        what = "only in " + (sys.argv[1] if s not in b else sys.argv[2]) if (s in a) != (s in b) else "differs"
        print(f"{what}: {s}")
    print(f"{len(set(a) | set(b))} symbols, {len(bad)} differing")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
