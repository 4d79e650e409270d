"""-m gpu: deskewed clouds from a motion-deblur registration (ll_reg_interpolation, ll_cloud_undistort, ll_cloud_undistort_fe_device,
ll_history_set_undistort, Laser_mapping( if_motion_deblur, if_undistort )).

The yardstick is the float64 numpy restatement of point_cloud_registration.hpp:641-646 and :607-620 in tests/undistort_ref.py, fed the
device's own state (ll_reg_interpolation), under that module's rule: every coordinate within one fp32 ulp, at most 1 in 10 000 unequal.

The 40 k-point rooms map and batches of 3 slots.  The registrar's start-up gate (init_accumulate_frames, PCR:199) is one decision per
enqueue of a single-map batch, so the gated slot is slot 0 of a batch of its own (`gated`); the two accepted slots of the issue are slots
1 and 2 of the batch `live`: slot 1 starts 0.1 m / 0.02 rad off, every time stamp of slot 2 equals maximum_pt_time_stamp."""
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd import build, capi, mapping, synth
from loam_livox_amd.api import History_buffer, Livox_laser, Map_buffer, Point_cloud_registration, Spinning_laser, VoxelGrid
from tests import undistort_ref as ur

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, B = 24000, 3
T0, DT = 0.5, 1e-5
MIN_TS, MAX_TS = float(np.float32(T0)), float(np.float32(np.float64(T0) + np.float64(np.float32(N - 1) * np.float32(DT))))
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
LINE_RES, PLANE_RES = 0.1, 0.4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def set_params(reg, deblur=1, frame_index=100):
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = 4, 20, 1
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = frame_index, 50
    p.if_motion_deblur, p.minimum_pt_time_stamp, p.maximum_pt_time_stamp = deblur, MIN_TS, MAX_TS
    return p


@pytest.fixture(scope="module")
def rig(gpu_lib):
    world, corner, surf = synth.make_maps(40_000)
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, corner)
    m.setInputCloud(Map_buffer.SURF, surf)
    scans = [synth.make_moving_scan(world, k, N) for k in range(B)]
    fe = Livox_laser(max_points=N, max_scans=B, piecewise_number=1)
    fe.upload(np.stack([s.xyzi for s in scans]), np.full(B, T0))
    fe.extract_batch(B)
    fe.resolve()
    fe.select_batch(B, -1, 0.0, 1.0)
    feats = [fe.get_features(scan=b) for b in range(B)]
    stamps = [fe.pts_info(b)["time_stamp"] for b in range(B)]
    fc, fs = [f["pc_corners"] for f in feats], [f["pc_surface"] for f in feats]
    assert all(len(c) > 50 and len(s) > 2000 for c, s in zip(fc, fs))
    assert max(float(s.max()) for s in stamps) == MAX_TS and min(float(s.min()) for s in stamps) == MIN_TS
    fc[2], fs[2] = fc[2].copy(), fs[2].copy()
    fc[2][:, 3] = MAX_TS     # slot 2: every stamp at the end of the range (s == 1)
    fs[2][:, 3] = MAX_TS
    poses = np.stack([s.pose_init for s in scans])
    off = np.r_[synth.quat_from_axis_angle(np.array([0.3, -0.5, 1.0]), 0.02), 0.06, -0.07, 0.04]   # 0.1 m, 0.02 rad
    assert abs(np.linalg.norm(off[4:]) - 0.1) < 2e-3
    poses[1] = synth.pose_compose(poses[1], off)
    reg = Point_cloud_registration(max_scans=B, max_features=N)
    yield dict(map=m, fe=fe, feats=feats, stamps=stamps, fc=fc, fs=fs, poses=poses, reg=reg, scans=scans)
    for h in (reg, fe, m):
        h.close()


def register(rig, deblur=1, frame_index=100, poses=None):
    reg = rig["reg"]
    set_params(reg, deblur, frame_index)
    pl = rig["poses"] if poses is None else poses
    res, pc, pi, reps = reg.solve_batch(rig["map"], rig["fc"], rig["fs"], pl, pl)
    return res, pc, pi, reps


def cloud(rng, n):
    """points around the sensor with stamps across, below and above the range and on both of its ends"""
    c = np.zeros((n, 4), np.float32)
    c[:, :3] = rng.uniform(-40, 40, (n, 3))
    c[:, 3] = rng.uniform(MIN_TS - 0.05, MAX_TS + 0.05, n)
    c[::17, 3] = MAX_TS
    c[5::19, 3] = MIN_TS
    return c


def restated(it, b, pose_curr, xyzi, deblur=1):
    return ur.undistort(xyzi, it["pose_last"][b], pose_curr, it["pose_incre"][b], it["theta"][b], it["omega_hat"][b], deblur, MIN_TS, MAX_TS)


# ------------------------------------------------------------------------------------------------ 1, 2
def test_interpolation_and_cloud_undistort_of_a_live_batch(rig):
    reg = rig["reg"]
    res, pc, pi, reps = register(rig)
    assert res.tolist() == [1, 1, 1] and not any(r.gated for r in reps)
    it = reg.interpolation(B)
    assert np.array_equal(it["pose_last"], rig["poses"]) and np.array_equal(it["pose_incre"], pi)
    for b in range(B):   # 1: the state against the restatement of the returned increment
        theta, hat = ur.interp(pi[b, :4])
        assert abs(it["theta"][b] - theta) <= 1e-12 and np.abs(it["omega_hat"][b] - hat).max() <= 1e-12
        assert it["theta"][b] > 1e-4   # a start pose that was off: there is an increment to interpolate
    rng = np.random.default_rng(11)
    for n in (0, 1, 255, 256, 257, 5000):   # 2
        c = cloud(rng, n)
        for b in (0, 1):
            got = reg.pointcloudAssociateToMap(c, if_undistore=1, slot=b)
            assert got.shape == (n, 4) and same_bits(got[:, 3], c[:, 3])
            ur.check_rule(got[:, :3], restated(it, b, pc[b], c), f"ll_cloud_undistort slot {b} n {n}")
    c = cloud(rng, 5000)
    got = reg.pointcloudAssociateToMap(c, if_undistore=1, slot=1)
    assert np.abs(got[:, :3] - reg.pointcloudAssociateToMap(c, pc[1])[:, :3]).max() > 1e-3   # not the plain transform
    # slot 2's own cloud: every stamp is maximum_pt_time_stamp, the end-of-scan pose, bit for bit
    own = rig["fs"][2]
    assert same_bits(reg.pointcloudAssociateToMap(own, if_undistore=1, slot=2), reg.pointcloudAssociateToMap(own, pc[2]))
    # refusals: a slot beyond the batch, and an enqueue that has not been collected
    with pytest.raises(capi.LoamLivoxError, match="n_scans"):
        reg.pointcloudAssociateToMap(c, if_undistore=1, slot=B)
    reg.upload_features(rig["fc"], rig["fs"])
    reg.enqueue_uploaded(rig["map"], B, rig["poses"], rig["poses"])
    for call in (lambda: reg.pointcloudAssociateToMap(c, if_undistore=1), lambda: reg.interpolation(B)):
        with pytest.raises(capi.LoamLivoxError, match="collect"):
            call()
    reg.collect(B)
    assert same_bits(reg.pointcloudAssociateToMap(c, if_undistore=1, slot=1), got)   # the same registration again: the same cloud
    with pytest.raises(capi.LoamLivoxError, match="n_scans"):
        reg.interpolation(B + 1)


def test_refused_before_a_first_collect(rig):
    reg = Point_cloud_registration(max_scans=1, max_features=100)
    h = History_buffer(4, 100, LINE_RES, PLANE_RES)
    for call in (lambda: reg.interpolation(1), lambda: reg.pointcloudAssociateToMap(np.zeros((1, 4), np.float32), if_undistore=1), lambda: h.set_undistort(reg)):
        with pytest.raises(capi.LoamLivoxError, match="collect"):
            call()
    h.close()
    reg.close()


def test_gated_slot_is_the_plain_transform_with_pose_last(rig):
    reg = rig["reg"]
    res, pc, pi, reps = register(rig, frame_index=10)   # 10 <= init_accumulate_frames: PCR:199
    assert all(r.gated for r in reps)
    it = reg.interpolation(B)
    assert not it["theta"].any() and not it["omega_hat"].any() and np.array_equal(it["pose_incre"], np.tile(IDENT, (B, 1)))
    c = cloud(np.random.default_rng(12), 5000)
    assert same_bits(reg.pointcloudAssociateToMap(c, if_undistore=1, slot=0), reg.pointcloudAssociateToMap(c, rig["poses"][0]))


def test_rejected_slot_keeps_its_increment_and_ends_at_pose_last(rig):
    """PCR:561-573: pose_curr = pose_last, the increment of the last ICP iteration stays in place"""
    reg = rig["reg"]
    set_params(reg)
    reg.params.max_final_cost = 1e-12   # every registration is rejected
    pl = rig["poses"]
    res, pc, pi, reps = reg.solve_batch(rig["map"], rig["fc"], rig["fs"], pl, pl)
    assert res.tolist() == [0, 0, 0] and np.array_equal(pc, pl) and not any(r.gated for r in reps)
    it = reg.interpolation(B)
    assert np.array_equal(it["pose_incre"], pi) and it["theta"][1] > 1e-4 and np.abs(pi[1, 4:]).max() > 1e-3
    c = cloud(np.random.default_rng(14), 5000)
    got = reg.pointcloudAssociateToMap(c, if_undistore=1, slot=1)
    ur.check_rule(got[:, :3], restated(it, 1, pl[1], c), "rejected slot")
    end = c.copy()
    end[:, 3] = MAX_TS
    assert same_bits(reg.pointcloudAssociateToMap(end, if_undistore=1, slot=1), reg.pointcloudAssociateToMap(end, pl[1]))


def test_without_motion_deblur_every_form_is_the_plain_transform(rig):
    reg = rig["reg"]
    res, pc, pi, reps = register(rig, deblur=0)
    c = cloud(np.random.default_rng(13), 5000)
    for b in range(B):
        assert same_bits(reg.pointcloudAssociateToMap(c, if_undistore=1, slot=b), reg.pointcloudAssociateToMap(c, pc[b]))
    import torch
    out_u = torch.zeros((B * N, 4), dtype=torch.float32, device="cuda")
    out_p = torch.zeros((B * N, 4), dtype=torch.float32, device="cuda")
    acc = np.ones(B, np.int32)
    for kind in (0, 1):
        nu = reg.cloud_undistort_fe_device(rig["fe"], B, kind, acc, out_u, 0)
        assert nu == reg.append_to_submap_device(rig["fe"], B, kind, acc, pc, out_p, 0) and nu > 0
        assert torch.equal(out_u[:nu].view(torch.int32), out_p[:nu].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 3
def test_fe_device_equals_the_host_form_of_the_clouds_read_back(rig):
    import torch
    reg, fe = rig["reg"], rig["fe"]
    register(rig)
    acc = np.array([1, 0, 1], np.int32)   # slot 1 refused
    for kind in (0, 1, 2):
        if kind == 2:   # the full selection: point full_idx of the scan with intensity := its time stamp (LFE:246,255)
            clouds = []
            for b in range(B):
                full = rig["scans"][b].xyzi[rig["feats"][b]["full_idx"]].copy()
                full[:, 3] = rig["stamps"][b][rig["feats"][b]["full_idx"]]
                clouds.append(full)
        else:
            clouds = [rig["feats"][b]["pc_corners" if kind == 0 else "pc_surface"] for b in range(B)]
        want = np.concatenate([reg.pointcloudAssociateToMap(clouds[b], if_undistore=1, slot=b) for b in range(B) if acc[b]])
        lead = 7   # appended behind what the buffer holds
        out = torch.full((lead + len(want) + 5, 4), -1.0, dtype=torch.float32, device="cuda")
        n = reg.cloud_undistort_fe_device(fe, B, kind, acc, out, lead)
        host = out.cpu().numpy()
        assert n == lead + len(want) and len(want) > (300 if kind == 0 else 10000)
        # (NaN points of a full cloud stay NaN on both routes: compare bits)
        assert same_bits(host[lead:n], want) and (host[:lead] == -1.0).all() and (host[n:] == -1.0).all()
        small = torch.full((lead + len(want) - 1, 4), -1.0, dtype=torch.float32, device="cuda")
        with pytest.raises(capi.LoamLivoxError, match="too small"):
            reg.cloud_undistort_fe_device(fe, B, kind, acc, small, lead)
        assert (small.cpu().numpy() == -1.0).all()   # the refusal wrote nothing
    n_points = capi.C.c_int64(3)
    small = torch.zeros((4, 4), dtype=torch.float32, device="cuda")
    rc = reg.L.ll_cloud_undistort_fe_device(reg.h, fe.h, B, 1, capi.ptr(acc), capi.C.c_void_p(small.data_ptr()), 4, capi.C.byref(n_points))
    assert rc != 0 and n_points.value == 3


# ------------------------------------------------------------------------------------------------ 4, 5
def history_clouds(h, m):
    h.refresh(m)
    return h.map_cloud(0), h.map_cloud(1)


def test_history_adds_with_the_setter_equal_the_host_route(rig):
    reg, fe = rig["reg"], rig["fe"]
    res, pc, pi, reps = register(rig)
    b = 1
    fc, fs = rig["feats"][b]["pc_corners"], rig["feats"][b]["pc_surface"]
    uc, us = (reg.pointcloudAssociateToMap(c, if_undistore=1, slot=b) for c in (fc, fs))
    gate = rig["poses"][b]

    def host_route(corner, surf):
        h, m = History_buffer(10, N, LINE_RES, PLANE_RES), Map_buffer()
        h.set_gate_pose(gate)
        assert h.add(corner, surf, IDENT)
        out = history_clouds(h, m)
        h.close(); m.close()
        return out

    want = host_route(uc, us)
    plain = host_route(*(reg.pointcloudAssociateToMap(c, pc[b]) for c in (fc, fs)))
    assert not same_bits(want[1], plain[1])
    for form in ("add_fe", "add"):
        h, m = History_buffer(10, N, LINE_RES, PLANE_RES), Map_buffer()
        h.set_gate_pose(gate)
        h.set_undistort(reg, b)
        assert h.add_fe(fe, b, pc[b]) if form == "add_fe" else h.add(fc, fs, pc[b])
        got = history_clouds(h, m)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), form
        # the setter applies to the next add only: a second add is the plain one
        h2, m2 = History_buffer(10, N, LINE_RES, PLANE_RES), Map_buffer()
        h.set_gate_pose(gate); h2.set_gate_pose(gate)
        h2.set_undistort(reg, b)
        assert h2.add(fc, fs, pc[b]) and h2.add(fc, fs, pc[b]) and h.add(fc, fs, pc[b])
        two = history_clouds(h2, m2)
        assert same_bits(two[0], history_clouds(h, m)[0]) and same_bits(two[1], history_clouds(h, m)[1])
        for x in (h, m, h2, m2):
            x.close()
    # add_voxel: the down-sampled stacks of a registration of the extractor's batch
    vox = (VoxelGrid(N, B), VoxelGrid(N, B))
    set_params(reg)
    reg.enqueue_fe_downsampled(rig["map"], fe, vox[0], vox[1], LINE_RES, PLANE_RES, B, rig["poses"], rig["poses"])
    res, pc, _, _ = reg.collect(B)
    stacks = []
    for leaf, c in ((LINE_RES, fc), (PLANE_RES, fs)):
        hv = VoxelGrid(N, 1)
        hv.setLeafSize(leaf, leaf, leaf)
        hv.setInputCloud(c)
        stacks.append(hv.filter())
        hv.close()
    h, m = History_buffer(10, N, LINE_RES, PLANE_RES), Map_buffer()
    h.set_gate_pose(gate)
    h.set_undistort(reg, b)
    assert h.add_voxel(vox[0], vox[1], b, pc[b])
    got = history_clouds(h, m)
    want = host_route(*(reg.pointcloudAssociateToMap(c, if_undistore=1, slot=b) for c in stacks))
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    # add_spin refuses the setter, drops it, and the handle goes on
    spin = Spinning_laser(scan_line=16, max_points=20000, max_scans=1)
    h.set_undistort(reg, b)
    with pytest.raises(capi.LoamLivoxError, match="time stamp"):
        h.add_spin(spin, 0, pc[b])
    h.set_gate_pose(gate)
    assert h.add(fc, fs, pc[b]) and len(h) == 2
    for x in (spin, h, m, vox[0], vox[1]):
        x.close()


def test_the_record_outlives_the_registrars_next_enqueue(rig):
    reg, fe = rig["reg"], rig["fe"]
    b = 1
    fc, fs = rig["feats"][b]["pc_corners"], rig["feats"][b]["pc_surface"]
    other = rig["poses"].copy()
    other[:, 4:] += 0.05
    frames = []
    for sync in (False, True):
        res, pc, _, _ = register(rig)
        h, m = History_buffer(10, N, LINE_RES, PLANE_RES), Map_buffer()
        h.set_undistort(reg, b)
        first = reg.pointcloudAssociateToMap(fs, if_undistore=1, slot=b)
        reg.params.current_frame_index = 10   # the next registration is gated at poses 5 cm away: a state that moves clouds elsewhere
        if sync:
            import torch
            torch.cuda.synchronize()
            assert h.add_fe(fe, b, pc[b])
            torch.cuda.synchronize()
            reg.upload_features(rig["fc"], rig["fs"])
            reg.enqueue_uploaded(rig["map"], B, other, other)
        else:   # the setter, then at once the next registration on the same registrar -- collected, and deskewed with, so that the
            # registrar's own records are rewritten with the other poses' state -- and only then the add: it must use the history's copy
            reg.upload_features(rig["fc"], rig["fs"])
            reg.enqueue_uploaded(rig["map"], B, other, other)
            _, pc_other, _, _ = reg.collect(B)
            moved = reg.pointcloudAssociateToMap(fs, if_undistore=1, slot=b)
            assert np.abs(moved[:, :3] - first[:, :3]).max() > 0.02   # the registrar's records are the other registration's now
            assert h.add_fe(fe, b, pc[b])
            reg.upload_features(rig["fc"], rig["fs"])
            reg.enqueue_uploaded(rig["map"], B, other, other)
        reg.collect(B)
        frames.append(history_clouds(h, m))
        h.close(); m.close()
    assert same_bits(frames[0][0], frames[1][0]) and same_bits(frames[0][1], frames[1][1]) and len(frames[0][1]) > 100


# ------------------------------------------------------------------------------------------------ 6
FRAMES, INIT = 7, 2


@pytest.fixture(scope="module")
def sequence():
    world, _, _ = synth.make_maps(40_000)
    scans, _ = synth.make_livox_sequence(world, 77, n_frames=FRAMES, n_static=3, n_points=12000)
    stamps = [1.0 + k * 12000 * DT for k in range(FRAMES)]   # frame k + 1 starts where frame k ended
    return scans, stamps


def run_loop(sequence, **flags):
    scans, stamps = sequence
    lm = mapping.Laser_mapping(scan_points=12000, maximum_history_size=5, init_accumulate_frames=INIT, icp_max_iterations=4, **flags)
    out = []
    for xyzi, t in zip(scans, stamps):
        res = lm.process_new_scan(xyzi, t)
        out.append((res, lm.pose.copy(), lm.history.map_cloud(0), lm.history.map_cloud(1)))
    lm.close()
    return out


def run_composed(sequence, deblur, undistort):
    """the loop of Laser_mapping.process_new_scan from the public pieces (laser_mapping.hpp:1311-1520)"""
    scans, stamps = sequence
    P = 12000
    fe, reg, m = Livox_laser(max_points=P, max_scans=1, piecewise_number=1), Point_cloud_registration(max_scans=1, max_features=P), Map_buffer()
    vox, h = (VoxelGrid(P, 1), VoxelGrid(P, 1)), History_buffer(5, P, LINE_RES, PLANE_RES)
    mapping._set_registrar_params(reg.params, scan_points=P, icp_max_iterations=4, ceres_max_iterations=100, max_allow_incre_R=200.0 / 50.0,
                                  max_allow_incre_T=100.0 / 50.0, max_allow_final_cost=100.0, init_accumulate_frames=INIT, minimum_icp_R_diff=0.01,
                                  minimum_icp_T_diff=0.01, maximum_residual_blocks=0, subsample_seed=1)
    reg.params.if_motion_deblur = deblur
    pose, last_t, out = IDENT.copy(), 0.0, []
    for k, (xyzi, t) in enumerate(zip(scans, stamps)):
        fe.upload(xyzi[None], np.full(1, t))
        fe.extract_batch(1)
        fe.resolve()
        fe.select_batch(1, -1, 0.0, 1.0)
        if deblur:   # :1336-1347
            full_idx = fe.get_features(scan=0)["full_idx"]
            max_t = float(fe.pts_info(0)["time_stamp"][full_idx].max())
            reg.params.minimum_pt_time_stamp, reg.params.maximum_pt_time_stamp = last_t, max_t
            last_t = max_t
        reg.params.current_frame_index = k
        reg.enqueue_fe_downsampled(m, fe, vox[0], vox[1], LINE_RES, PLANE_RES, 1, pose[None], pose[None])
        res, pc, _, _ = reg.collect(1)
        if res[0]:
            h.set_gate_pose(pose)
            if undistort:
                h.set_undistort(reg, 0)
            h.add_voxel(vox[0], vox[1], 0, pc[0])
            pose = pc[0].copy()
            h.refresh(m)
        out.append((int(res[0]), pose.copy(), h.map_cloud(0), h.map_cloud(1)))
    for x in (fe, reg, m, vox[0], vox[1], h):
        x.close()
    return out


def loops_equal(a, b):
    assert len(a) == len(b) == FRAMES
    for k, (x, y) in enumerate(zip(a, b)):
        assert x[0] == y[0] and np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64)), k
        assert same_bits(x[2], y[2]) and same_bits(x[3], y[3]), k


def test_laser_mapping_with_the_flags(gpu_lib, sequence):
    both = run_loop(sequence, if_motion_deblur=1, if_undistort=1)
    assert [o[0] for o in both] == [1] * FRAMES and np.linalg.norm(both[-1][1][4:]) > 0.05   # registered, and the sensor moved
    loops_equal(both, run_composed(sequence, 1, 1))                                            # (a)
    deblur_only = run_loop(sequence, if_motion_deblur=1)
    loops_equal(deblur_only, run_composed(sequence, 1, 0))                                     # (b)
    loops_equal(run_loop(sequence, if_undistort=1), run_loop(sequence))                        # (c)
    # (d) the deskew is not a no-op: frames up to INIT agree (gated: nothing to interpolate), the first registered frame's history cloud
    # -- the same pose history before it in both runs -- holds points that moved by more than a millimetre
    k = INIT + 1
    assert same_bits(both[INIT][3], deblur_only[INIT][3])
    a, b = both[k][3], deblur_only[k][3]
    moved = np.abs(a[:, :3] - b[:, :3]).max() if a.shape == b.shape else np.inf
    print(f"frame {k}: largest coordinate difference between the deskewed and the plain history cloud {moved:.4g} m")
    assert moved > 1e-3
    last = np.abs(both[-1][3][:, :3] - deblur_only[-1][3][:, :3]).max() if both[-1][3].shape == deblur_only[-1][3].shape else np.inf
    assert last > 1e-3
    for kw in (dict(if_motion_deblur=1), dict(if_undistort=1)):                               # (e)
        with pytest.raises(ValueError):
            mapping.Laser_mapping(scan_points=12000, lidar_type="velodyne", **kw)


def test_process_new_scan_with_key_frames_deskews_the_stamped_full_cloud(gpu_lib, sequence):
    """laser_mapping.hpp:1442 with g_if_undistore = 1: the cloud the key frames and the full map receive is the scan's full selection
    with intensity := the extractor's time stamp (LFE:246,255), moved by ll_cloud_undistort -- not the raw scan's reflectivity read as a stamp"""
    scans, stamps = sequence
    lc = dict(scans_of_each_keyframe=6, scans_between_two_keyframe=3, minimum_keyframe_differen=1, avail_ratio_plane=0, avail_ratio_line=0,
              map_alignment_maximum_icp_iteration=2, max_points=1 << 17)
    lm = mapping.Laser_mapping(scan_points=12000, maximum_history_size=5, init_accumulate_frames=INIT, icp_max_iterations=4, loop_closure_if_enable=1,
                               loop_closure=lc, if_motion_deblur=1, if_undistort=1)
    seen = []
    add_scan = lm.keyframes.add_scan

    def spy(cloud, *a, **k):
        seen.append(np.array(cloud, np.float32, copy=True))
        return add_scan(cloud, *a, **k)
    lm.keyframes.add_scan = spy
    for k, (xyzi, t) in enumerate(zip(scans, stamps)):
        assert lm.process_new_scan(xyzi, t) == 1 and len(seen) == k + 1
        full_idx = lm.fe.get_features(scan=0)["full_idx"]
        full = xyzi[full_idx].copy()
        raw = full[np.isfinite(full[:, :3]).all(axis=1)]
        full[:, 3] = lm.fe.pts_info(0)["time_stamp"][full_idx]
        full = full[np.isfinite(full[:, :3]).all(axis=1)]
        assert len(full) > 8000 and not np.array_equal(raw[:, 3], full[:, 3])
        assert same_bits(seen[-1], lm.reg.pointcloudAssociateToMap(full, if_undistore=1))
        if k > INIT:   # a registered frame: the deskew moved points, and the reflectivity read as a stamp would have put them elsewhere
            assert np.abs(seen[-1][:, :3] - lm.reg.pointcloudAssociateToMap(full, lm.pose)[:, :3]).max() > 1e-3
            assert np.abs(seen[-1][:, :3] - lm.reg.pointcloudAssociateToMap(raw, if_undistore=1)[:, :3]).max() > 1e-3
    lm.close()


# ------------------------------------------------------------------------------------------------ 7
def test_adapter_forms_against_the_c_call(tmp_path, rig):
    lib = build.build()
    exe = str(tmp_path / "adapter_undistort")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "adapter_undistort.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    _, corner, surf = synth.make_maps(40_000)
    xyzi = lambda a: np.ascontiguousarray(np.c_[a[:, :3], np.zeros(len(a))] if a.shape[1] == 3 else a, np.float32)
    paths = [str(tmp_path / n) for n in ("mc.f32", "ms.f32", "sc.f32", "ss.f32", "pose.f64", "out.bin")]
    fc, fs = rig["feats"][1]["pc_corners"], rig["feats"][1]["pc_surface"]
    for p, a in zip(paths, (xyzi(corner), xyzi(surf), fc, fs)):
        a.tofile(p)
    np.asarray(rig["poses"][1], np.float64).tofile(paths[4])
    done = subprocess.run([exe] + paths[:5] + [repr(MIN_TS), repr(MAX_TS), paths[5]], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert done.returncode == 0, done.stderr.decode(errors="replace")
    raw = open(paths[5], "rb").read()
    head = np.frombuffer(raw[:16], np.int32)
    n = int(head[1])
    clouds = np.frombuffer(raw[16:], np.float32).reshape(3, n, 4)
    assert head[0] == 1 and n == len(fs) and head[2] == 1 and head[3] == 1
    assert same_bits(clouds[0], clouds[1])                       # pointcloudAssociateToMap( ..., 1 ) is the C call
    assert same_bits(clouds[2][:, 3], clouds[1][:, 3])
    ulp = np.spacing(np.maximum(np.abs(clouds[1][:, :3]), np.abs(clouds[2][:, :3])))
    worst = float((np.abs(clouds[2][:, :3].astype(np.float64) - clouds[1][:, :3].astype(np.float64)) / ulp).max())
    print(f"adapter per-point form against ll_cloud_undistort: worst distance {worst:.3g} fp32 ulp, {(clouds[2] != clouds[1]).sum()} coordinates unequal")
    assert worst <= 1.0
