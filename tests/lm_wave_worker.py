"""Child process of tests/test_gpu_lm_wave.py: registers the end-to-end cases with the library LOAM_LIVOX_LIB names (default: the product
library) and writes results, poses, the raw report structures and the debug counters of every scan to an .npz.

    python -m tests.lm_wave_worker OUT.npz

The inputs and the registration call are those of tests/test_gpu_solver_size_classes.py (imported, not copied)."""
import sys

import numpy as np

from tests import test_gpu_solver_size_classes as T
from tests import test_solver_size_classes_host as H

# name -> (scans as (nC, nS) of the concatenated cloud, registration switches, start pose offset in metres)
CASES = {
    "small_w1": ([(40, 300), (0, 200), (7, 65)], dict(small_solver_waves=1), None),
    "small_w2": ([(40, 300), (0, 200), (7, 65)], dict(small_solver_waves=2), None),
    "small_w4": ([(40, 300), (0, 200), (7, 65)], dict(small_solver_waves=4), None),
    "small_w4_far_start": ([(40, 300), (100, 900)], dict(small_solver_waves=4), (0.45, -0.4, 0.35)),   # the step runs into the bound on t_inc
    "small_w8": ([(100, 1100), (0, 1025)], dict(), None),                                              # more than 1 024 features: eight wavefronts
    "fast_b17": (H.batch_of_17((300, 4097), [(0, 2049), (1025, 1023), (0, 513)]), dict(), None),        # one workgroup per scan
    "fast_b17_far_start": (H.batch_of_17((300, 4097), [(0, 2049), (1025, 1023), (0, 513)]), dict(), (0.45, -0.4, 0.35)),
    "fast_grouped_b2": ([(300, 6000), (0, 6500)], dict(), None),                                       # eight workgroups per scan
    "big_b2": ([(1, 24065), (0, 513)], dict(), None),                                                  # 24 577 padded blocks: reg_solve_big_kernel<0>
    "big_deblur_b2": ([(300, 4097), (0, 513)], dict(deblur=True), None),                               # reg_solve_big_kernel<1>
}


def expected_form(name):
    scans, sw, _ = CASES[name]
    deblur = bool(sw.get("deblur"))
    kernel = H.batch_kernel(scans, deblur=deblur)
    return kernel, kernel == "fast" and H.grouped(scans, deblur=deblur)   # (only reg_solve_kernel spreads a scan over a group)


class Scan:
    def __init__(self, fc, fs, pose):
        self.fc, self.fs, self.pose = np.ascontiguousarray(fc), np.ascontiguousarray(fs), pose


class World:
    def __init__(self):
        self.inp = H.inputs()
        self.map = T.Map_buffer()
        self.map.setInputCloud(T.Map_buffer.CORNER, self.inp["corner"])
        self.map.setInputCloud(T.Map_buffer.SURF, self.inp["surf"])


def main(out):
    w = World()
    inp = w.inp
    result = {}
    for name, (scans, switches, offset) in CASES.items():
        pose = inp["pose"].copy()
        if offset is not None:
            pose[4:7] += offset
        cases = [Scan(inp["fc"][:nc], inp["fs"][:ns], pose) for nc, ns in scans]
        sw = dict(switches)
        deblur = sw.pop("deblur", False)
        res, pc, reps, reg = T.solve(w, cases, deblur=deblur, debug=True, **sw)
        counts = np.stack([reg.debug_cycles(i)[14:16] for i in range(len(cases))])
        reg.close()
        result[name + "/res"] = np.asarray(res)
        result[name + "/pose"] = np.asarray(pc)
        result[name + "/reports"] = np.frombuffer(b"".join(bytes(r) for r in reps), np.uint8)
        result[name + "/lm"] = np.array([r.lm_iterations_total for r in reps])
        result[name + "/counts"] = counts
    w.map.close()
    np.savez(out, **result)


if __name__ == "__main__":
    main(sys.argv[1])
