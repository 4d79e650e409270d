"""Writes tests/golden/ref_spin_*.npz: recorded outputs of the spinning-lidar feature extraction (the branch of
hku-mars/loam_livox source/laser_feature_extractor.hpp:393-811) for seeded synthetic scans that the tests regenerate with
synth.make_spin_scan.  Recorded with the host restatement tests/spin_ref.c, which tests/test_spin_ref_pin.py holds bit-identical
to the reference's own text compiled on this host.  Each file: the scan's parameters, full_src (input index of each laserCloud
point), the intensities of laserCloud, the sharp / less_sharp / flat / less_flat_pre position lists and the less-flat cloud.

    python tests/golden/gen_ref_spin.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from loam_livox_amd import synth  # noqa: E402
from tests import spin_ref  # noqa: E402

CASES = [  # name, k, scan_line, n_azimuth, range_sigma
    ("vlp16_a", 900, 16, 900, 0.01),
    ("vlp16_noisefree", 901, 16, 600, 0.0),
    ("hdl64_a", 902, 64, 700, 0.01),
]


def main():
    world = synth.make_world(4, 4)
    for name, k, L, n_az, sigma in CASES:
        sc = synth.make_spin_scan(world, k, scan_line=L, n_azimuth=n_az, range_sigma=sigma)
        r = spin_ref.extract(sc.xyzi, scan_line=L)
        path = os.path.join(HERE, f"ref_spin_{name}.npz")
        np.savez_compressed(path, k=k, scan_line=L, n_azimuth=n_az, range_sigma=sigma, full_src=r["full_src"], intensity=r["full"][:, 3],
                            sharp=r["sharp"], less_sharp=r["less_sharp"], flat=r["flat"], less_flat_pre=r["less_flat_pre"],
                            less_flat=r["less_flat"])
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
