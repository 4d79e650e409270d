"""-m gpu: the scene alignment of two key frames on the device (ll_cellmap_feature_clouds, ll_scene_align_*; api.Cell_map.feature_clouds,
api.Scene_aligner, Scene_alignment( on_device=True ), Keyframe_assembly( device_alignment=True ), the adapter's Scene_alignment) against
the host route of loam_livox_amd/scene_alignment.py -- bit for bit: both run the same kernels on the same values in the same order --
and against the oracle's keyframe_clouds / SceneAlignment.  tests/test_scene_align_host.py is the CPU tier."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_cellmap import bits, keyframe_pair
from tests.test_scene_align_host import MAPS, geometry, oracle_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (seed of keyframe_pair, resolution, maximum_icp_iteration, accepted_threshold): the class defaults, then the loop detector's values and
# the early stop of tests/test_cellmap.py test_oracle_scene_alignment_equals_the_reference_driver
SETTINGS = {"defaults": (3, 0.4, 10, 0.2), "loop detector": (4, 0.2, 2, 0.35), "early stop": (5, 0.4, 3, 0.01)}


def xyzi(pts):
    return np.c_[pts, np.zeros(len(pts), np.float32)].astype(np.float32)


def device_map(cloud):
    from loam_livox_amd.api import Cell_map
    m = Cell_map(max_points=max(1, len(cloud)), resolution=1.0)
    m.append_cloud(cloud)
    return m


def same_result(a, b):
    """two runs agree to the bit: threshold, pose, number of registrations and every report's block, ICP and LM counts"""
    (thr_a, pose_a, rep_a), (thr_b, pose_b, rep_b) = a, b
    assert np.float64(thr_a).tobytes() == np.float64(thr_b).tobytes()
    assert np.array_equal(np.asarray(pose_a, np.float64).view(np.uint64), np.asarray(pose_b, np.float64).view(np.uint64))
    assert len(rep_a) == len(rep_b)
    for x, y in zip(rep_a, rep_b):
        assert (x.n_blocks_last, x.icp_iterations, x.lm_iterations_total) == (y.n_blocks_last, y.icp_iterations, y.lm_iterations_total)
        assert np.float64(x.inlier_threshold).tobytes() == np.float64(y.inlier_threshold).tobytes()


def align(da, db, res, max_icp, accepted, on_device, max_points=1 << 18):
    from loam_livox_amd.scene_alignment import Scene_alignment
    sa = Scene_alignment(res, res, max_icp, accepted, max_points=max_points, on_device=on_device)
    thr = sa.find_tranfrom_of_two_mappings(da, db)
    work = sa._aligner.work() if on_device else None
    out = (thr, sa.pose.copy(), list(sa.reports))
    sa.close()
    return out, work


@pytest.fixture(scope="module")
def pairs(gpu_lib):
    """per setting: the two clouds, their device cell maps, and both routes' results -- computed once, shared, not changed"""
    out = {}
    for name, (seed, res, max_icp, accepted) in SETTINGS.items():
        a, b, _ = keyframe_pair(seed)
        da, db = device_map(a), device_map(b)
        host, _ = align(da, db, res, max_icp, accepted, False)
        dev, work = align(da, db, res, max_icp, accepted, True)
        out[name] = dict(a=a, b=b, da=da, db=db, host=host, dev=dev, work=work)
    yield out
    for r in out.values():
        r["da"].close()
        r["db"].close()


# ---------------------------------------------------------------------------------------------------------------- 1: the selection
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MAPS) + ["empty map"])
def test_feature_clouds_equal_the_oracle_and_the_host_selection(gpu_lib, name):
    from loam_livox_amd.api import Cell_map
    from loam_livox_amd.scene_alignment import keyframe_clouds as host_clouds
    from oracle.orc_scene_alignment import keyframe_clouds
    pts = geometry(**MAPS[name])[0] if name in MAPS else np.zeros((0, 3), np.float32)
    want = keyframe_clouds(oracle_map(pts))
    dm = Cell_map(max_points=max(1, len(pts)), resolution=1.0)    # (exactly full: the two clouds share the map's scratch)
    dm.append_cloud(xyzi(pts))
    got, host = dm.feature_clouds(), host_clouds(dm)
    for g, w, h in zip(got, want, host):
        assert g.shape == w.shape == h.shape and g.dtype == np.float32
        assert np.array_equal(bits(g), bits(w)) and np.array_equal(bits(g), bits(h))
    if name.startswith("all kinds"):
        assert len(got[0]) > 257 and len(got[1]) > 1000
    if name in ("no line cell", "only sphere cells", "empty map"):
        assert len(got[0]) == 0
    if name in ("no plane cell", "only sphere cells", "empty map"):
        assert len(got[1]) == 0
    # the counts alone, and a buffer that is too small: an error, nothing written
    import ctypes as C
    nl, npl = C.c_int64(-1), C.c_int64(-1)
    assert gpu_lib.ll_cellmap_feature_clouds(dm.h, None, 0, C.byref(nl), None, 0, C.byref(npl), None) == 0
    assert (nl.value, npl.value) == (len(got[0]), len(got[1]))
    if len(got[1]) > 1:
        small = np.full((len(got[1]) - 1, 4), 7.0, np.float32)
        nl.value = npl.value = -1
        assert gpu_lib.ll_cellmap_feature_clouds(dm.h, None, 0, C.byref(nl), small.ctypes.data_as(C.c_void_p), len(small), C.byref(npl), None) < 0
        assert b"ll_cellmap_feature_clouds: buffer too small" in gpu_lib.ll_last_error()
        assert (small == 7.0).all() and (nl.value, npl.value) == (-1, -1)
    dm.close()


# ------------------------------------------------------------------------------------------------------ 2, 3: parity of the two routes
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETTINGS))
def test_device_route_equals_the_host_route_and_the_oracle(pairs, name):
    from loam_livox_amd import synth
    from oracle.orc_cellmap import CellMap
    from oracle.orc_scene_alignment import SceneAlignment
    r = pairs[name]
    _, res, max_icp, accepted = SETTINGS[name]
    same_result(r["dev"], r["host"])
    thr, pose, reports = r["dev"]
    ka, kb = CellMap(1.0), CellMap(1.0)
    ka.append(r["a"]); kb.append(r["b"])
    so = SceneAlignment(res, res, max_icp, accepted)
    thr_o = so.find_tranfrom_of_two_mappings(ka, kb)
    dt, dr = synth.pose_error(pose, so.pose)
    assert dt < 1e-7 and dr < 1e-7 and abs(thr - thr_o) < 1e-9     # (the bounds of tests/test_cellmap.py test_device_scene_alignment_matches_oracle)
    assert len(reports) == len(so.reports)
    assert [x.n_blocks_last for x in reports] == [x.n_blocks_last for x in so.reports]
    assert [x.icp_iterations for x in reports] == [x.icp_iterations for x in so.reports]
    if name == "early stop":
        assert len(reports) < 3 and len(r["host"][2]) < 3            # SA:350-351: stopped after a coarse round, on both routes
    else:
        assert len(reports) == 3


# ------------------------------------------------------------------------------------------- 4: nothing to register against
@pytest.mark.gpu
def test_a_map_side_without_line_cells_runs_no_registration(gpu_lib):
    # (another seed for b: other cells, so the two centres differ)
    da, db = device_map(xyzi(geometry(**MAPS["no line cell"])[0])), device_map(xyzi(geometry(seed=8, remainder=5)[0]))
    host, _ = align(da, db, 0.4, 10, 0.2, False)
    dev, work = align(da, db, 0.4, 10, 0.2, True, max_points=512)
    same_result(dev, host)
    thr, pose, reports = dev
    ca, cb = da.feature_clouds()[2], db.feature_clouds()[2]
    assert thr == 0.0 and len(reports) == 0 and work[2] == 0
    assert np.array_equal(pose, np.r_[0.0, 0.0, 0.0, 1.0, (ca - cb).astype(np.float64)]) and np.abs(pose[4:]).max() > 0
    da.close(); db.close()


@pytest.mark.gpu
def test_refusals_come_before_any_launch_and_leave_the_handle_usable(pairs):
    from loam_livox_amd.api import Scene_aligner
    from loam_livox_amd.capi import LoamLivoxError
    r = pairs["loop detector"]
    _, res, max_icp, accepted = SETTINGS["loop detector"]
    sa = Scene_aligner(initial_points=1 << 16)
    p = sa.params
    p.line_res = p.plane_res = res
    p.maximum_icp_iteration, p.accepted_threshold = max_icp, accepted
    with pytest.raises(LoamLivoxError, match="ll_scene_align_run: the two key frames are the same map"):
        sa.run(r["da"], r["da"])
    p.plane_res = 0.0
    with pytest.raises(LoamLivoxError, match="ll_scene_align_run: resolutions must be positive"):
        sa.run(r["da"], r["db"])
    p.plane_res, p.maximum_icp_iteration = res, 0
    with pytest.raises(LoamLivoxError, match="ll_scene_align_run: maximum_icp_iteration must be positive"):
        sa.run(r["da"], r["db"])
    assert sa.work().tolist() == [0, 0, 0, 0]                       # nothing has run on this handle
    p.maximum_icp_iteration = max_icp
    pose, thr, reports = sa.run(r["da"], r["db"])
    same_result((thr, pose, reports), r["dev"])
    sa.close()


# ---------------------------------------------------------------------------------------------- 5: one handle, two pairs
@pytest.mark.gpu
def test_a_second_pair_through_one_handle_equals_a_fresh_handle(pairs):
    """nothing of the first pair leaks into the second, and the handle grows: it starts at 1024 points, the second pair's clouds hold
    tens of thousands"""
    from loam_livox_amd.scene_alignment import Scene_alignment
    small_a, small_b = device_map(xyzi(geometry(**MAPS["all kinds, a multiple of the block"])[0])), device_map(xyzi(geometry(seed=8, remainder=5)[0]))
    r = pairs["defaults"]
    sa = Scene_alignment(max_points=1024, on_device=True)
    first = (sa.find_tranfrom_of_two_mappings(small_a, small_b), sa.pose.copy(), list(sa.reports))
    second = (sa.find_tranfrom_of_two_mappings(r["da"], r["db"]), sa.pose.copy(), list(sa.reports))
    same_result(second, r["dev"])          # (r["dev"]: a fresh handle that started at 2^18 points)
    assert len(r["a"]) > 16 * 1024 and not np.array_equal(first[1], second[1])
    again = (sa.find_tranfrom_of_two_mappings(small_a, small_b), sa.pose.copy(), list(sa.reports))
    same_result(again, first)              # ... and back: the large pair left nothing behind either
    sa.close(); small_a.close(); small_b.close()


# ------------------------------------------------------------------------------------------------------------- 6: the work tap
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETTINGS))
def test_work_tap_no_point_crosses_and_every_registration_is_counted(pairs, name):
    work, reports = pairs[name]["work"], pairs[name]["dev"][2]
    print("ll_scene_align_work", name, work.tolist(), "registrations", len(reports))
    assert work[0] == 0
    assert work[2] == len(reports)
    assert work[3] == 10               # per key frame: cell labels, centre, flag, scan, gather


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SETTINGS))
def test_work_tap_one_host_wait_per_registration(pairs, name):
    """one wait for every size, centre and bounding box of the run, then one per registration (to collect it: the early stop needs that
    scale's report)"""
    work = pairs[name]["work"]
    print("ll_scene_align_work", name, work.tolist())
    assert work[1] == 1 + work[2]


# ---------------------------------------------------------------------------------------------------------------- 7: the adapter
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["loop detector", "early stop"])
def test_adapter_scene_alignment_equals_the_python_device_route(pairs, tmp_path, name):
    from loam_livox_amd import build
    lib = build.build()
    exe = str(tmp_path / "adapter_scene_align")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "adapter_scene_align.cpp"), lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    r = pairs[name]
    _, res, max_icp, accepted = SETTINGS[name]
    fa, fb, out = str(tmp_path / "a.bin"), str(tmp_path / "b.bin"), str(tmp_path / "out.txt")
    r["a"].astype(np.float32).tofile(fa)
    r["b"].astype(np.float32).tofile(fb)
    subprocess.check_call([exe, fa, fb, repr(res), str(max_icp), repr(accepted), out], timeout=120)
    lines = open(out).read().strip().split("\n")
    la, pa, _ = r["da"].feature_clouds()
    lb, pb, _ = r["db"].feature_clouds()
    assert [int(v) for v in lines[0].split()] == [len(la), len(pa), len(lb), len(pb)]
    h = 14695981039346656037
    for byte in la.tobytes() + pa.tobytes():
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    assert int(lines[1]) == h
    thr, pose, reports = r["dev"]
    # (accepted_threshold is a float in the C ABI on both routes; the program reads the same decimal text)
    assert float.fromhex(lines[2]) == thr and np.float64(float.fromhex(lines[2])).tobytes() == np.float64(thr).tobytes()
    got = np.array([float.fromhex(v) for v in lines[3].split()], np.float64)
    assert np.array_equal(got.view(np.uint64), np.asarray(pose, np.float64).view(np.uint64))
    tail = [int(v) for v in lines[4].split()]
    assert tail[0] == len(reports) and tail[1:] == r["work"].tolist()


# ------------------------------------------------------------------------------------------------------- 8: the loop detector
def out_and_back_sequence():
    """the scans of tests/test_keyframes.py test_out_and_back_sequence_closes_a_loop -- a place swept, another one, the first again with
    0.6 m / 0.5 degrees of drift -- as (cloud in the map frame, estimated pose, frame index); that test builds them inline, so they are
    restated here, value for value"""
    from loam_livox_amd import synth
    world = synth.world_for_map_size(200_000)
    rng = np.random.default_rng(77)
    start = synth.sensor_pose_in_world(world, rng)
    per_kf = 40
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    zax, yax = np.array([0.0, 0.0, 1.0]), np.array([0.0, 1.0, 0.0])
    away = synth.pose_compose(start, np.r_[synth.quat_from_axis_angle(zax, np.deg2rad(170.0)), np.array([12.0, 6.0, 0.0])])
    drift = np.r_[synth.quat_from_axis_angle(zax, np.deg2rad(0.5)), np.array([0.6, -0.4, 0.1])]
    k = 0
    for grp, (base, est_err, span, pitch, jit) in enumerate([(start, ident, 220.0, 15.0, 0.0), (away, ident, 300.0, 20.0, 0.0), (start, drift, 360.0, 30.0, 0.5)]):
        for j in range(per_kf):
            yaw, pit = np.deg2rad(span * (j / (per_kf - 1) - 0.5)), np.deg2rad(pitch * np.sin(3.1 * j))
            rot = synth.quat_mul(synth.quat_from_axis_angle(zax, yaw), synth.quat_from_axis_angle(yax, pit))
            true_pose = synth.pose_compose(base, np.r_[rot, jit * np.array([np.sin(1.7 * j), np.cos(2.3 * j), 0.0])])
            sc = synth.make_moving_scan(world, 9100 + 100 * grp + j, 24000, inc_true=ident, pose_start=true_pose, t_phase=0.07 * j)
            est = synth.pose_compose(est_err, true_pose)
            ok = np.isfinite(sc.xyzi[:, :3]).all(axis=1) & (np.abs(sc.xyzi[:, :3]).sum(axis=1) > 0)
            cloud = np.c_[synth.transform_points(est, sc.xyzi[ok, :3]), np.zeros(int(ok.sum()), np.float32)].astype(np.float32)
            k += 1
            yield cloud, est, k


@pytest.mark.gpu
def test_keyframe_assembly_with_device_alignment_gives_the_same_log_and_loops(gpu_lib):
    from loam_livox_amd.keyframes import Keyframe_assembly
    kw = dict(scans_of_each_keyframe=40, scans_between_two_keyframe=40, minimum_keyframe_differen=2, maximum_keyframe_in_waiting_list=3,
              map_alignment_inlier_threshold=0.35, map_alignment_maximum_icp_iteration=4, max_points=1 << 22, avail_ratio_plane=0.02,
              avail_ratio_line=0.0)
    host, dev = Keyframe_assembly(**kw), Keyframe_assembly(device_alignment=True, **kw)
    found = ([], [])
    for cloud, est, k in out_and_back_sequence():     # (the scans are made once and fed to both)
        for ka, loops in zip((host, dev), found):
            ka.add_scan(cloud, est, k)
            loops.extend(ka.process_waiting())

    def same(x, y):
        assert sorted(x) == sorted(y)
        for key in x:
            if isinstance(x[key], np.ndarray):
                assert np.array_equal(np.asarray(x[key], np.float64).view(np.uint64), np.asarray(y[key], np.float64).view(np.uint64)), key
            else:
                assert x[key] == y[key], key
    assert len(host.log) == len(dev.log) and len(host.loops) == len(dev.loops) == len(found[0]) == len(found[1]) == 1
    for x, y in zip(host.log + host.loops, dev.log + dev.loops):
        same(x, y)
    assert any("inlier_threshold" in r for r in dev.log)          # a pair was aligned
    assert dev._scene_alignment is not None and host._scene_alignment is None   # one object for every pair on the device route only
    host.close(); dev.close()
