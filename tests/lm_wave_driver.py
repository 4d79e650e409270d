"""Builds and runs tests/lm_wave_host.cpp (the wavefront form of the LM controller as a loop over 64 lanes, against the scalar form) for
tests/test_lm_wave_host.py and tests/test_gpu_lm_wave.py."""
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "lm_wave_host.cpp")
# bit k of a sequence's mask (the enum of lm_wave_host.cpp)
BRANCHES = ["accept", "reject", "reuse0", "reuse1", "invalid", "invalid5", "param_tol", "func_tol", "gmax", "nactive0", "radius", "unbounded", "cubic",
            "fit", "first_fallback", "clamped", "nd0", "nd_big", "nonfinite_cost", "maxiter", "first_at_once", "search_ok"]
MAX_CALLS = 32        # LMW_MAX_CALLS: evaluations per sequence in a dump
NACC = 28
HDR = 12


def build_driver(exe, extra=()):
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", *extra, "-o", exe, SRC]
    subprocess.run(cmd, check=True)
    return exe


def run_driver(exe, n, dump=None, n_dump=0):
    """-> rows (index, kind, calls, set of branch names, mismatches), and with dump = a path the first n_dump sequences' (hdr, evals)"""
    cmd = [exe, str(n)] + ([dump, str(n_dump)] if dump else [])
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode in (0, 1) and (p.returncode == 0) == (p.stderr == ""), (p.returncode, p.stderr[-2000:])
    rows = []
    for line in p.stdout.splitlines():
        i, kind, calls, mask, mism = (int(v) for v in line.split())
        rows.append((i, kind, calls, {b for k, b in enumerate(BRANCHES) if mask >> k & 1}, mism))
    assert len(rows) == n
    if not dump:
        return rows
    rec = np.fromfile(dump, np.float64).reshape(n_dump, HDR + MAX_CALLS * NACC)
    return rows, np.ascontiguousarray(rec[:, :HDR]), np.ascontiguousarray(rec[:, HDR:]).reshape(n_dump, MAX_CALLS, NACC)
