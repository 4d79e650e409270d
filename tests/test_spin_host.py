"""CPU tier: the host restatement of the spinning-lidar feature extraction (tests/spin_ref.c) on the edges include/loam_livox_hip.h
defines (ll_spin_*), its parameter check, the shared decision helpers of ll_spin_core.h, and the recorded goldens."""
import glob
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd import synth
from tests import spin_inputs, spin_ref

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


# ---------------------------------------------------------------------------------------------------------------------------------
# What the builders of tests/spin_inputs.py reach, read from the restatement's own outputs.  These are conditions, not measurements:
# the device tests of tests/test_gpu_spin.py run the same scans, and mean what they claim only while these hold.
def reach(name):
    return spin_inputs.reach(spin_inputs.family(name)[1])


@pytest.mark.parametrize("name", sorted(spin_inputs.FAMILIES))
def test_families_are_deterministic_and_in_domain(name):
    x, r = spin_inputs.family(name)
    assert np.array_equal(x, spin_inputs.FAMILIES[name]()) and np.all(np.isfinite(x))
    assert len(r["full"]) == len(x) and np.all(np.linalg.norm(x[:, :3], axis=1) > 0.5)  # nothing filtered, minimum_range 0.1


def test_ring_reaches_both_sort_forms_the_cap_and_deep_ranks():
    _, r = spin_inputs.family("ring")
    rows = reach("ring")
    assert r["line_n"][6] == 11 + 6 * 4096 + 3 and [w["size"] for w in rows] == [4096, 4097] * 3
    assert all(w["sharp"] == 20 and 21 <= w["less_sharp"] <= 200 and w["candidates"] >= 201 for w in rows)
    assert any(w["less_sharp"] == 200 for w in rows) and any(w["less_sharp"] < 200 for w in rows)
    assert all(w["deepest"] > 1024 and w["in_order"] for w in rows)  # picks follow the sorted order, four or more 64-candidate chunks deep
    assert spin_inputs.tied_curvatures(r) >= 1000
    for size in (4096, 4097):  # a deep pick out of a run of tied curvatures, in either sort form: the position half of the key decides
        assert any(w["size"] == size and w["deepest"] > 1024 for w in rows)


def test_ring_rebuilds_the_candidate_mask_inside_a_chunk():
    """two picks of one 64-candidate chunk with, between them in the sorted order, a candidate that no rule pre-marked: a walk of the
    sub-region's earlier picks marked it, so the chunk's candidate mask has to be read again after a pick"""
    _, r = spin_inputs.family("ring")
    curv, ls, hits = r["curvature"], r["less_sharp"], 0
    for w in reach("ring"):
        sp, ep = w["sp"], w["ep"]
        pos = np.arange(sp, ep + 1)
        order = pos[np.lexsort((pos, curv[sp:ep + 1]))][::-1]
        picked = np.isin(order, ls)
        ranks = np.flatnonzero(picked)
        for a, b in zip(ranks[:-1], ranks[1:]):
            between = order[a + 1:b]
            hits += int(a // 64 == b // 64 and np.any((r["picked0"][between] == 0) & (curv[between] > spin_inputs.SHARP_CURV)))
    assert hits >= 10


def test_zigzag_picks_are_exact():
    """m = 199, 200, 201: 199, 200 and 200 less-sharp picks, 20 of them sharp, the top (curvature, position) entries in order; every
    walk breaks on its first step"""
    for name in ("zigzag", "zigzag_jitter"):
        _, r = spin_inputs.family(name)
        rows = reach(name)
        for line, m in ((6, 199), (7, 200), (8, 201)):
            exact = [w for w in rows if w["line"] == line and w["top"] and w["less_sharp"] == min(m, 200)]
            assert all(w["size"] == m and w["candidates"] == m and w["sharp"] == 20 and w["deepest"] == w["less_sharp"] - 1 for w in exact)
            assert len(exact) >= (3 if name == "zigzag" else 1), (name, line)
        for p in r["less_sharp"][::97]:
            assert spin_inputs.walk_len(r["full"], p, 1) == 0 and spin_inputs.walk_len(r["full"], p, -1) == 0
    assert spin_inputs.tied_curvatures(spin_inputs.family("zigzag_jitter")[1]) == 0
    # the stop at the 201st pick, and no stop at the 200th
    assert any(w["less_sharp"] == 200 and w["candidates"] == 201 and w["top"] for w in reach("zigzag"))
    assert any(w["less_sharp"] == 200 and w["candidates"] == 200 for w in reach("zigzag"))
    assert any(w["less_sharp"] == 199 and w["candidates"] == 199 for w in reach("zigzag"))


@pytest.mark.parametrize("name", ["ladder", "ladder_noise"])
def test_ladder_has_every_size_and_picks_in_all_of_them(name):
    _, r = spin_inputs.family(name)
    rows = reach(name)
    assert list(r["line_n"][:14]) == [11 + 6 * m for m in spin_inputs.LADDER]
    for line, m in enumerate(spin_inputs.LADDER):
        mine = [w for w in rows if w["line"] == line]
        assert len(mine) == 6 and all(w["size"] == m for w in mine)
        if m >= 63:
            assert sum(w["less_sharp"] for w in mine) > 0, m
        if m >= 1025:  # deep into the order: the merge steps of the padded network and the rank sort decide the picks
            assert max(w["deepest"] for w in mine) > min(m // 2, 1024)
    assert any(w["size"] == 4096 and w["less_sharp"] == 200 for w in rows) and any(w["size"] > 4096 and w["less_sharp"] == 200 for w in rows)
    assert any(21 <= w["less_sharp"] <= 199 for w in rows)
    if name == "ladder":
        assert spin_inputs.tied_curvatures(r) >= 1000
    else:
        assert spin_inputs.tied_curvatures(r) < spin_inputs.tied_curvatures(spin_inputs.family("ladder")[1])


def test_walks_run_500_steps_are_cut_at_499_and_stop_at_the_cloud_ends():
    a, wl = spin_inputs.WALK_A, spin_inputs.walk_len
    x, r = spin_inputs.family("walk_limit")
    assert r["less_sharp"].tolist() == [a]  # the probes at a +- 500 were reached
    assert wl(r["full"], a, 1) == wl(r["full"], a, -1) == 500
    assert np.all(r["curvature"][[a - 500, a + 500]] > spin_inputs.SHARP_CURV) and not np.any(r["picked0"][[a - 500, a, a + 500]])
    x, r = spin_inputs.family("walk_past")
    assert r["less_sharp"].tolist() == [a, a - 501, a + 501]  # one step past the limit: picked
    assert not np.any(r["picked0"][[a - 501, a, a + 501]])
    sub = [w for w in spin_inputs.reach(r) if w["sp"] <= a <= w["ep"]][0]
    assert sub["sp"] <= a - 501 and a + 501 <= sub["ep"]  # walker and probes share a sub-region: the walker, of higher curvature, goes first
    x, r = spin_inputs.family("walk_cut")
    assert wl(r["full"], a, 1) == wl(r["full"], a, -1) == 499
    assert r["less_sharp"][0] == a and a - 500 in r["less_sharp"] and (a + 500 in r["less_sharp"] or a + 501 in r["less_sharp"])
    x, r = spin_inputs.family("walk_ends")
    n = len(x)
    assert r["less_sharp"].tolist() == [99, n - 100]
    assert wl(r["full"], 99, -1) == 99 and wl(r["full"], n - 100, 1) == 99 and 99 > 64  # more than one ballot round, then the cloud's end
    assert wl(r["full"], 99, 1) == 500 and wl(r["full"], n - 100, -1) == 500


def test_a_walk_crosses_a_line_boundary_unless_a_gap_stops_it():
    (x, walker, probe), (_, r) = spin_inputs.line_boundary(False), spin_inputs.family("boundary_near")
    n = r["line_n"][6]
    assert r["line_n"][7] == n and walker < n - 6 and probe >= n + 5
    d = r["full"][n, :3] - r["full"][n - 1, :3]
    assert float(d @ d) < 0.05  # the last point of line 6 and the first of line 7
    assert r["curvature"][probe] > spin_inputs.SHARP_CURV and r["picked0"][probe] == 0  # a sharp candidate at the start of line 7 ...
    assert r["less_sharp"].tolist() == [walker]                                          # ... that is not picked
    assert spin_inputs.walk_len(r["full"], walker, 1) > probe - walker
    _, rf = spin_inputs.family("boundary_far")
    assert rf["less_sharp"].tolist() == [walker, probe] and spin_inputs.walk_len(rf["full"], walker, 1) == n - 1 - walker


def test_long_lines_pass_the_one_workgroup_voxel_filter():
    from oracle import orc
    _, r = spin_inputs.family("long_line")
    assert r["lf_line_n"][6] > 24576 and 0 < len(r["less_flat"]) < 1000  # filtered
    assert all(w["less_sharp"] == 200 and w["size"] > 4096 for w in reach("long_line"))
    _, r = spin_inputs.family("long_zigzag")
    assert r["lf_line_n"][6] > 24576 and len(r["less_flat"]) == r["lf_line_n"][6]  # "leaf size is too small": passed through
    assert orc.voxel_grid(r["full"][r["less_flat_pre"]], np.float32(0.4))[0] == 1
    for name in ("ladder", "ladder_noise"):
        lf = spin_inputs.family(name)[1]["lf_line_n"]
        assert np.count_nonzero(lf > 24576) >= 1 and np.count_nonzero((lf > 0) & (lf <= 24576)) >= 10


def test_the_families_as_a_whole_reach_every_branch():
    rows = [w for name in spin_inputs.FAMILIES for w in reach(name)]
    assert any(w["less_sharp"] == 200 and w["candidates"] >= 201 for w in rows)
    assert any(21 <= w["less_sharp"] <= 199 for w in rows)
    assert any(w["size"] > 4096 for w in rows) and any(w["size"] == 4096 for w in rows)
    assert max(w["deepest"] for w in rows) > 1024
    assert all(w["sharp"] == min(w["less_sharp"], 20) and w["less_sharp"] <= 200 and w["in_order"] for w in rows)
    # the old inputs for comparison: a world scan stays far from all of it
    w = synth.make_world(4, 4)
    old = spin_inputs.reach(spin_ref.extract(synth.make_spin_scan(w, 16, scan_line=16, n_azimuth=1800).xyzi, voxel=False))
    assert max(v["size"] for v in old) < 1024 and max(v["less_sharp"] for v in old) < 20
