"""CPU tier of the LM controller's wavefront form (tests/test_gpu_lm_wave.py is the GPU tier).

loam_livox_amd/csrc/ll_lm_wave.h -- the text the solver kernels run, a loop over 64 lanes standing in for the wavefront -- against the
scalar controller of ll_reg_core.h (the specification), both compiled by g++ with -ffp-contract=off (tests/lm_wave_host.cpp): 2 048
scripted sequences with fixed seeds, the whole LmCtl compared byte for byte after every call and the return codes with it.  Sequence
i is of kind i % 16: kinds 0 - 8 evaluate a random 6-parameter Huber problem (planes and lines) at the points the controller asks for,
kinds 9 - 15 feed hand-made sums that reach the rare branches.  Which kind reaches which branch is asserted below, from the pieces
lm_update is made of (lm_update_pre / _post / _close, whose answers the driver sees) and from the controller's state.
The same program once more under the address and undefined-behaviour sanitizers, with its own main.
The debug entry point ll_debug_lm_sequence: declared, exported, bound; refuses bad arguments without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from loam_livox_amd import capi
from tests.lm_wave_driver import build_driver, run_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    exe = build_driver(str(tmp_path_factory.mktemp("lm_wave") / "lm_wave_host"))
    return run_driver(exe, N)


def of_kind(rows, kind):
    return [r for r in rows if r[1] == kind]


def test_every_call_of_every_sequence_leaves_the_same_bytes(rows):
    assert len(rows) == N >= 2000
    calls = sum(r[2] for r in rows)
    print(f"{N} sequences, {calls} controller calls, longest {max(r[2] for r in rows)}")
    assert [r[0] for r in rows if r[4]] == []
    assert calls > 30000 and all(r[2] >= 1 for r in rows)


# kind -> branches EVERY sequence of the kind reaches / branches SOME sequence of the kind reaches
EVERY = {
    0: {"accept", "reuse0", "unbounded", "func_tol"},                       # small motion, no bound: ends on the function tolerance
    1: {"accept", "reuse0", "func_tol"},                                    # bound far away: the search never contracts
    3: {"accept", "reuse0", "clamped"},                                     # a bound the translation runs into at once
    4: {"accept", "unbounded"},
    7: {"accept"},
    8: {"nactive0"},                                                        # n_active == 0 ends lm_init
    9: {"invalid", "invalid5", "reuse0"},                                   # non-positive pivot: five invalid steps end the solve
    10: {"invalid", "invalid5"},                                            # non-finite solution
    11: {"invalid", "invalid5"},                                            # model cost change <= 0
    12: {"reject", "reuse1", "radius", "unbounded", "nd_big"},              # rejected steps halve, quarter, ... the radius below 1e-32
    13: {"accept", "nd0", "gmax"},                                          # a step without rotation; then gmax <= 1e-10
    14: {"nonfinite_cost", "cubic", "fit", "search_ok", "accept", "nd_big", "maxiter"},
    15: {"cubic", "fit", "first_fallback", "first_at_once", "reject", "reuse1", "param_tol"},
}
SOME = {
    2: {"reject", "reuse1", "cubic", "fit", "first_fallback", "clamped", "search_ok"},   # Armijo failures of a real problem at its bound
    3: {"reject", "cubic", "fit", "first_fallback", "search_ok"},
    4: {"nd_big"},                                                          # a rotation of a radian: state_plus beyond its Taylor range
    5: {"nd_big", "clamped", "fit"},
    6: {"maxiter", "unbounded", "clamped"},
    7: {"param_tol", "gmax"},                                               # exact data: ends on the parameter tolerance or on gmax
    13: {"unbounded", "clamped"},
}


@pytest.mark.parametrize("kind", sorted(EVERY))
def test_every_sequence_of_a_kind_reaches_its_branches(rows, kind):
    for r in of_kind(rows, kind):
        assert EVERY[kind] <= r[3], (r[0], sorted(EVERY[kind] - r[3]))
    if kind in (8, 9, 10, 11):
        assert {r[2] for r in of_kind(rows, kind)} == {1}                   # the solve ends inside lm_init
    if kind == 12:
        assert {r[2] for r in of_kind(rows, kind)} == {16}                  # 1e4 / 2^(k (k + 1) / 2) < 1e-32 from k = 15
    if kind in (0, 4, 8, 9, 10, 11, 12):
        assert all("clamped" not in r[3] for r in of_kind(rows, kind))     # bound < 0: nothing clamps, no search


@pytest.mark.parametrize("kind", sorted(SOME))
def test_some_sequence_of_a_kind_reaches_its_branches(rows, kind):
    seen = set().union(*(r[3] for r in of_kind(rows, kind)))
    assert SOME[kind] <= seen, sorted(SOME[kind] - seen)


def test_driver_runs_clean_under_the_sanitizers(tmp_path, rows):
    exe = build_driver(str(tmp_path / "lm_wave_host_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    again = run_driver(exe, N)          # (asserts exit status 0 and an empty stderr)
    assert again == rows


# ------------------------------------------------------------------------------------------------ the entry point without a device
def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    decl = re.search(r"\bint\s+ll_debug_lm_sequence\s*\(([^;]*)\);", header)
    fn = capi.load().ll_debug_lm_sequence
    assert decl and "ll_debug_lm_sequence" in capi.SYMBOLS
    assert len(decl.group(1).split(",")) == len(fn.argtypes) == 10 and fn.restype is C.c_int32


def test_bad_arguments_are_refused_and_the_size_is_told_without_a_device():
    L = capi.load()
    size = np.zeros(1, np.int32)
    assert L.ll_debug_lm_sequence(0, None, None, 0, 0, None, None, None, None, capi.ptr(size)) == 0
    assert size[0] > 0 and size[0] % 8 == 0
    assert L.ll_debug_lm_sequence(0, None, None, 0, 0, None, None, None, None, None) < 0 and b"ll_debug_lm_sequence" in L.ll_last_error()
    assert L.ll_debug_lm_sequence(0, None, None, -1, 4, None, None, None, None, capi.ptr(size)) < 0
    assert L.ll_debug_lm_sequence(0, None, None, 2, 4, None, None, None, None, capi.ptr(size)) < 0 and b"bad argument" in L.ll_last_error()
