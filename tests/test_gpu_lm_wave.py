"""-m gpu: the LM controller on its wavefront (loam_livox_amd/csrc/ll_lm_wave.h) against the controller on lane 0 (ll_reg_core.h, the
specification), on the device.  tests/test_lm_wave_host.py is the CPU tier.

Tap.  ll_debug_lm_sequence runs both forms in one kernel, one wavefront per sequence, over the first 512 sequences of the CPU tier's
generator (tests/lm_wave_host.cpp: kinds 0 - 15, at most 32 calls each, the evaluations recorded from the host run): after every call
the two LmCtl are equal byte for byte and so are the answers.  The evaluations are scripted, so a form that strayed would still be fed
the same sums; a sequence ends with the first call either form answers with 0.

End to end.  The smallest shapes of every solver form (tests/lm_wave_worker.py, inputs and call of tests/test_gpu_solver_size_classes.py):
the small-scan solver with one, two, four and eight wavefronts per scan, reg_solve_kernel with one workgroup per scan (B = 17) and
grouped (B = 2), reg_solve_big_kernel<0> and <1> at B = 2 -- registered by the product library and by the variant the same tree gives
with -DLL_LM_LANE0 (loam_livox_amd/build.py build_lm_lane0), each in a fresh child process: results, poses and the report structures
are equal byte for byte.  The variant also counts, per scan, the three-sample fits of its line searches and the solves that ended on a
rejected step (-DLL_LM_COUNTS, ll_reg_debug_cycles slots 14 and 15; the report structure has no field for either): between them the
cases hold both, in the small-scan solver and in reg_solve_kernel.  The product library's counters stay zero: it counts nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

from loam_livox_amd import build as ll_build
from loam_livox_amd import capi
from tests import lm_wave_worker as worker
from tests.lm_wave_driver import MAX_CALLS, build_driver, run_driver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_TAP = 512


# ------------------------------------------------------------------------------------------------ tap
@pytest.fixture(scope="module")
def tap(gpu_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("lm_wave_tap")
    exe = build_driver(str(d / "lm_wave_host"))
    rows, hdr, evals = run_driver(exe, N_TAP, str(d / "dump.bin"), N_TAP)
    size = np.zeros(1, np.int32)
    assert gpu_lib.ll_debug_lm_sequence(0, None, None, 0, 0, None, None, None, None, capi.ptr(size)) == 0
    nb = int(size[0])
    img0, img1 = np.zeros((N_TAP, MAX_CALLS, nb), np.uint8), np.zeros((N_TAP, MAX_CALLS, nb), np.uint8)
    ret0, ret1 = np.zeros((N_TAP, MAX_CALLS), np.int32), np.zeros((N_TAP, MAX_CALLS), np.int32)
    assert gpu_lib.ll_debug_lm_sequence(0, capi.ptr(hdr), capi.ptr(evals), N_TAP, MAX_CALLS, capi.ptr(img0), capi.ptr(img1), capi.ptr(ret0), capi.ptr(ret1),
                                        capi.ptr(size)) == 0, gpu_lib.ll_last_error()
    return rows, hdr, img0, img1, ret0, ret1


def test_tap_both_forms_leave_the_same_bytes_after_every_call(tap):
    rows, hdr, img0, img1, ret0, ret1 = tap
    called = ret0 >= 0
    print(f"{N_TAP} sequences, {int(called.sum())} calls on the device ({int(hdr[:, 10].sum())} scripted); sequences cut short by the device: "
          f"{int((called.sum(axis=1) < hdr[:, 10]).sum())}")
    bad = [(i, k) for i, k in zip(*np.nonzero((img0 != img1).any(axis=2) | (ret0 != ret1)))]
    assert bad == [], bad[:8]
    assert called[:, 0].all() and called.sum() > 5000           # every sequence ran, and most of the script with it
    assert img0[called].any(axis=1).all()                       # (a state was written for every call made)


# ------------------------------------------------------------------------------------------------ end to end
def run_worker(out, lib=None):
    env = dict(os.environ)
    env.pop("LOAM_LIVOX_LIB", None)
    if lib:
        env["LOAM_LIVOX_LIB"] = lib
    p = subprocess.run([sys.executable, "-m", "tests.lm_wave_worker", out], cwd=ROOT, env=env, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-3000:]
    return dict(np.load(out))


@pytest.fixture(scope="module")
def both(gpu_lib, tmp_path_factory):
    d = tmp_path_factory.mktemp("lm_wave_e2e")
    variant = ll_build.build_lm_lane0()
    return run_worker(str(d / "wave.npz")), run_worker(str(d / "lane0.npz"), variant)


@pytest.mark.parametrize("name", list(worker.CASES))
def test_wavefront_controller_registers_like_the_lane0_build(both, name):
    wave, lane0 = both
    kernel, grouped = worker.expected_form(name)
    fits, rejected = lane0[name + "/counts"][:, 0], lane0[name + "/counts"][:, 1]
    print(f"{name}: {kernel}{' grouped' if grouped else ''}, results {wave[name + '/res'].tolist()}, LM iterations {wave[name + '/lm'].tolist()}, "
          f"fits {fits.tolist()}, solves ended on a rejected step {rejected.tolist()}")
    assert kernel == ("small" if name.startswith("small") else "fast" if name.startswith("fast") else "big")
    assert grouped == (name == "fast_grouped_b2")
    for key in ("/res", "/pose", "/reports"):
        assert wave[name + key].tobytes() == lane0[name + key].tobytes(), key
    assert (wave[name + "/lm"] > 0).all()
    assert not wave[name + "/counts"].any()                     # the product library counts nothing


def test_the_cases_hold_fits_and_solves_that_end_on_a_rejected_step(both):
    _, lane0 = both
    for form in ("small", "fast"):
        fits = sum(int(lane0[n + "/counts"][:, 0].sum()) for n in worker.CASES if n.startswith(form))
        rejected = sum(int(lane0[n + "/counts"][:, 1].sum()) for n in worker.CASES if n.startswith(form))
        print(f"{form}: three-sample fits {fits}, solves ended on a rejected step {rejected}")
        assert fits > 0 and rejected > 0, form
