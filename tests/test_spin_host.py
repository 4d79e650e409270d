"""CPU tier: the host restatement of the spinning-lidar feature extraction (tests/spin_ref.c) on the edges include/loam_livox_hip.h
defines (ll_spin_*), its parameter check, the shared decision helpers of ll_spin_core.h, and the recorded goldens."""
import glob
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd import synth
from tests import spin_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "loam_livox_amd", "csrc")


@pytest.fixture(scope="module")
def world():
    return synth.make_world(4, 4)


def test_scan_line_other_than_16_or_64_is_refused():
    pts = np.zeros((20, 4), np.float32)
    with pytest.raises(spin_ref.SpinRefError):
        spin_ref.extract(pts, scan_line=32)


def test_more_than_max_points_is_an_error():
    with pytest.raises(spin_ref.SpinRefError):
        spin_ref.extract(np.ones((spin_ref.MAX_POINTS + 1, 4), np.float32), voxel=False)


@pytest.mark.parametrize("n", [0, 1, 4, 5, 10])
def test_ten_points_or_fewer_get_no_curvature(world, n):
    x = synth.make_spin_scan(world, 1, scan_line=16, n_azimuth=40).xyzi[:n]
    r = spin_ref.extract(x)
    assert len(r["full"]) == n
    assert not np.any(r["curvature"]) and len(r["sharp"]) == len(r["flat"]) == len(r["less_flat"]) == 0


def test_nan_and_near_points_are_dropped_and_start_ori_uses_the_filtered_cloud(world):
    x = synth.make_spin_scan(world, 2, scan_line=16, n_azimuth=300).xyzi.copy()
    x[0, :3] = np.nan
    x[1, :3] = (0.01, 0.0, 0.0)  # inside minimum_range
    x[7::11, :3] = np.nan
    r = spin_ref.extract(x)
    src = r["full_src"]
    assert 0 not in src and 1 not in src and not np.any(np.isin(src, np.arange(7, len(x), 11)))
    # the relative time of the first kept point is 0: startOri came from it (x[2]), not from the NaN at x[0]
    first = np.flatnonzero(src == 2)[0]
    assert r["full"][first, 3] == np.float32(np.floor(r["full"][first, 3]))


def test_lines_are_in_scan_id_order_and_input_order(world):
    x = synth.make_spin_scan(world, 3, scan_line=64, n_azimuth=200).xyzi
    r = spin_ref.extract(x, scan_line=64)
    sid = np.floor(r["full"][:, 3]).astype(int)
    assert np.all(np.diff(sid) >= 0) and np.all(r["line_n"][51:] == 0)
    for line in range(64):
        s = r["full_src"][sid == line]
        assert np.all(np.diff(s) > 0)


def test_sharp_walk_reaches_the_ends_of_the_cloud():
    t = np.linspace(0, 1, 400, dtype=np.float32)
    x = np.stack([10 + 0.01 * t, 1 + 0.01 * t, np.full_like(t, -0.524), np.ones_like(t)], 1).astype(np.float32)
    x[9:380:9, 0] += 0.8
    r = spin_ref.extract(x)
    assert len(r["less_sharp"]) > 0
    # the last sub-region's sharp point walks forward over the smooth tail to the last point, which stays unlabelled
    assert r["less_sharp"].max() >= 370


def test_flat_pass_stops_at_five_per_subregion(world):
    x = synth.make_spin_scan(world, 4, scan_line=16, n_azimuth=1800, range_sigma=0.0).xyzi
    r = spin_ref.extract(x)
    assert len(r["flat"]) <= 5 * 6 * 16 and len(r["flat"]) > 16 * 6 * 3


def test_host_decision_helpers_agree_with_the_restatement(tmp_path):
    """ll_spin_core.h compiled for the host (what ll_spin_resolve runs) gives the restatement's scan IDs for angles on and off
    the bin boundaries, and its ulp band brackets every boundary"""
    src = tmp_path / "t.cpp"
    src.write_text(r'''
#include <cstdio>
#include <initializer_list>
#include "ll_spin_core.h"
using namespace ll;
int main() {
    int bad = 0;
    for (int L : {16, 64}) for (float a = -26.f; a < 4.f; a += 0.0625f) {
        const float lo = spin_step_ulps(a, -1), hi = spin_step_ulps(a, 1);
        if (spin_scan_id(lo, L) != spin_scan_id(hi, L) && !spin_angle_ambiguous(a, L)) bad++;
    }
    if (spin_step_ulps(1.0f, 1) != nextafterf(1.0f, 2.0f) || spin_step_ulps(-1.0f, 1) != nextafterf(-1.0f, 0.0f)) bad++;
    if (spin_step_ulps(0.0f, -1) != -nextafterf(0.0f, 1.0f)) bad++;
    printf("%d\n", bad);
    return 0;
}
''')
    exe = tmp_path / "t"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", CSRC, str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().strip() == "0"


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "ref_spin_*.npz"))))
def test_restatement_matches_goldens(world, path):
    g = np.load(path)
    sc = synth.make_spin_scan(world, int(g["k"]), scan_line=int(g["scan_line"]), n_azimuth=int(g["n_azimuth"]),
                              range_sigma=float(g["range_sigma"]))
    r = spin_ref.extract(sc.xyzi, scan_line=int(g["scan_line"]))
    for k in ("full_src", "sharp", "less_sharp", "flat", "less_flat_pre"):
        assert np.array_equal(r[k], g[k]), k
    assert np.array_equal(r["full"][:, 3], g["intensity"])
    assert np.array_equal(r["less_flat"], g["less_flat"])


def test_goldens_exist():
    assert len(glob.glob(os.path.join(GOLDEN, "ref_spin_*.npz"))) >= 2
