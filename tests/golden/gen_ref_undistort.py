#!/usr/bin/env python3
"""Generates tests/golden/ref_undistort.npz from the REFERENCE ITSELF (oracle/_ref/libll_ref.so, `make -C oracle ref`): the state a
motion-deblur registration leaves in the reference's Point_cloud_registration and the clouds its pointcloudAssociateToMap( ., ., 1 )
makes of it (point_cloud_registration.hpp:607-661, 673-685).

Inputs are those of the committed tests/golden/ref_scene2.npz (its feature clouds, start pose, time range; the synthetic map re-created
from its seed and checked by checksum) -- tests/undistort_pin.py holds them and the four cases.  Outputs only are stored, per case:
  <case>_ret, _pose_out, _pose_incre, _theta, _omega_hat, _omega_hat_sq2      the return value and the object's state
  <case>_corners, _surface, _full, _shifted                                   xyz [n, 3] of the deskewed clouds (the intensity is the input's)
`shifted` is the surface cloud with stamps a range-width below and above the range and a few NaN stamps (undistort_pin.shifted_stamps).

The fixture travels to where the reference does not exist; tests/test_ref_undistort_golden.py holds the oracle, the host build of
csrc/ll_reg_core.h and the numpy restatement (CPU) and the HIP path (-m gpu) to it.

Run from the repo root (needs the reference's sources):  python tests/golden/gen_ref_undistort.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref  # noqa: E402
from tests import undistort_pin as up  # noqa: E402


def main():
    assert ref.can_build(), "needs the reference's sources"
    s = up.scene()
    out = {}
    for case in up.CASES:
        RR = ref.RefRegistration()
        RR.set_params(up.case_params(case))
        RR.set_maps(s["corner_map"], s["surf_map"])
        ret, pc, pi, rep = RR.solve(s["corners"], s["surface"], s["pose_init"], s["pose_init"], up.start_increment(case))
        st = RR.state()
        assert np.array_equal(st["pose_curr"], pc) and np.array_equal(st["pose_incre"], pi) and np.array_equal(st["pose_last"], s["pose_init"])
        out.update({f"{case}_ret": np.int32(ret), f"{case}_pose_out": pc, f"{case}_pose_incre": pi, f"{case}_theta": np.float64(st["theta"]),
                    f"{case}_omega_hat": st["omega_hat"], f"{case}_omega_hat_sq2": st["omega_hat_sq2"]})
        for name in up.CLOUDS:
            moved = RR.cloud_associate(s[name], 1)
            assert up.same_bits(moved[:, 3], s[name][:, 3])
            out[f"{case}_{name}"] = np.ascontiguousarray(moved[:, :3])
        print(case, "ret", ret, "theta", st["theta"], "increment", pi, "blocks", rep["n_blocks_last"])
    np.savez_compressed(up.FIXTURE, **out)
    print(up.FIXTURE, os.path.getsize(up.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
