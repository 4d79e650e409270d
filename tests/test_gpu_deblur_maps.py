"""-m gpu: motion deblur with a map per slot -- ll_reg_set_time_ranges in front of ll_reg_enqueue_fe_maps / _downsampled_maps, the
solver form reg_solve_big_maps_kernel, the per-slot ranges in the information and deskew records, ll_fe_selection_last.

The yardstick of a running slot is the single-map registration of that scan alone with the slot's range in the params
(ll_reg_enqueue_fe[_downsampled], n_scans = 1, reg_solve_big_kernel<1>): results, poses, increments, report costs and counts and the
information record are compared bit for bit.  The running slots of the map-per-slot test are also held to the oracle's deblur
registration by tests/test_gpu_solver_size_classes.py's check_oracle, with its tolerances.  The deskewed clouds are held to
tests/undistort_ref.py under that module's rule (one fp32 ulp, at most 1 coordinate in 10 000 unequal).

Three moving scans of 12 000 points with different start stamps, so every slot has a time range of its own; five extractor slots hold
scans 0, 1, 2, 0, 1 (slots 3 and 4 are the idle and the gated slot of the map-per-slot test)."""
import numpy as np
import pytest

from loam_livox_amd import capi, mapping, synth
from loam_livox_amd.api import Livox_laser, Map_buffer, Point_cloud_registration, VoxelGrid
from oracle import orc
from tests import test_gpu_solver_size_classes as G
from tests import test_solver_size_classes_host as H
from tests import undistort_ref as ur

pytestmark = pytest.mark.gpu
N, S = 12000, 5
DT = 1e-5
SCAN_OF = (0, 1, 2, 0, 1)
T0 = (0.5, 1.3, 2.1, 0.9, 1.7)
LINE_RES, PLANE_RES = 0.1, 0.4
ICP = H.ICP
REPORT_FIELDS = ("final_cost", "initial_cost", "inlier_threshold", "angular_diff_deg", "t_diff", "icp_iterations", "n_blocks_last", "corner_avail",
                 "surf_avail", "lm_iterations_total", "accepted", "gated", "aborted")


def stamp_range(t0):
    """the stamps of a scan's first and last point, as the extractor computes them"""
    return float(mapping._point_time_stamp(t0, 0, DT)), float(mapping._point_time_stamp(t0, N - 1, DT))


RANGES = [stamp_range(t) for t in T0]


def set_params(reg, deblur=1, ts=(0.0, 1.0), frame_index=100):
    p = reg.params   # (tests/test_gpu_solver_size_classes.py solve(): what check_oracle's cases are computed with)
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = ICP, H.CERES, 1
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = frame_index, 50
    p.maximum_allow_residual_block, p.subsample_seed = H.MAX_BLOCKS, 0
    p.if_motion_deblur, p.minimum_pt_time_stamp, p.maximum_pt_time_stamp = deblur, ts[0], ts[1]


def extracted(scans, stamps):
    fe = Livox_laser(max_points=N, max_scans=len(scans), piecewise_number=1)
    fe.upload(np.stack(scans), np.asarray(stamps, np.float64))
    fe.extract_batch(len(scans))
    fe.resolve()
    fe.select_batch(len(scans), -1, 0.0, 1.0)
    return fe


@pytest.fixture(scope="module")
def rig(gpu_lib):
    world, corner, surf = synth.make_maps(40_000)
    clouds = [(corner, surf), (synth.sample_corner_map(world, 6_000, 31), synth.sample_surface_map(world, 26_000, 32)),
              (synth.sample_corner_map(world, 10_000, 41), synth.sample_surface_map(world, 40_000, 42))]
    maps = []
    for c, s in clouds:
        m = Map_buffer()
        m.setInputCloud(Map_buffer.CORNER, c)
        m.setInputCloud(Map_buffer.SURF, s)
        maps.append(m)
    scans = [synth.make_moving_scan(world, k, N) for k in range(3)]
    fe = extracted([scans[k].xyzi for k in SCAN_OF], T0)
    fe1 = [extracted([scans[k].xyzi], [T0[k]]) for k in range(3)]
    poses = np.stack([scans[k].pose_init for k in SCAN_OF])
    reg = Point_cloud_registration(max_scans=S, max_features=N)
    reg1 = Point_cloud_registration(max_scans=1, max_features=N)
    vox = (VoxelGrid(N, S), VoxelGrid(N, S))
    vox1 = (VoxelGrid(N, 1), VoxelGrid(N, 1))
    for r in (reg, reg1):
        r.set_information(True)
    yield dict(world=world, clouds=clouds, maps=maps, scans=scans, fe=fe, fe1=fe1, poses=poses, reg=reg, reg1=reg1, vox=vox, vox1=vox1, memo={})
    for h in [reg, reg1, fe] + fe1 + maps + list(vox) + list(vox1):
        h.close()


def single(rig, b, m, ts, down):
    """scan b alone through the single-map entry point against map m with ts in the params; computed once, never changed"""
    key = (b, m, ts, down)
    if key not in rig["memo"]:
        reg, fe = rig["reg1"], rig["fe1"][b]
        set_params(reg, 1, ts)
        pose = rig["poses"][b][None]
        if down:
            reg.enqueue_fe_downsampled(rig["maps"][m], fe, rig["vox1"][0], rig["vox1"][1], LINE_RES, PLANE_RES, 1, pose, pose)
        else:
            reg.enqueue_fe(rig["maps"][m], fe, 1, pose, pose)
        res, pc, pi, reps = reg.collect(1)
        rig["memo"][key] = (int(res[0]), pc[0].copy(), pi[0].copy(), reps[0], reg.information(1)[0], reg.interpolation(1))
    return rig["memo"][key]


def batch(rig, n, maps, ranges, down, frame_index=None, deblur=1):
    reg, fe = rig["reg"], rig["fe"]
    set_params(reg, deblur)   # (the params' own pair, 0 .. 1, is not read)
    reg.set_time_ranges([r[0] for r in ranges], [r[1] for r in ranges])
    pl = rig["poses"][:n]
    tab = [None if m is None else rig["maps"][m] for m in maps]
    if down:
        reg.enqueue_fe_downsampled_maps(tab, fe, rig["vox"][0], rig["vox"][1], LINE_RES, PLANE_RES, n, pl, pl, frame_index)
    else:
        reg.enqueue_fe_maps(tab, fe, n, pl, pl, frame_index)
    return reg.collect(n)


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_slot(tag, got, want):
    """(res, pose, increment, report, information record) of a slot against the single run's, bit for bit"""
    res, pc, pi, rep, info = got
    w_res, w_pc, w_pi, w_rep, w_info, _ = want
    dt, dr = synth.pose_error(pc, w_pc)
    print(f"{tag}: result {res} ({w_res}), pose against the single run {dt:.2e} m {dr:.2e} rad, cost {rep.final_cost:.17g} ({w_rep.final_cost:.17g}), "
          f"blocks {rep.n_blocks_last} ({w_rep.n_blocks_last}), LM {rep.lm_iterations_total} ({w_rep.lm_iterations_total})")
    assert res == w_res, tag
    assert np.array_equal(u64(pc), u64(w_pc)) and np.array_equal(u64(pi), u64(w_pi)), (tag, dt, dr)
    for f in REPORT_FIELDS:
        a, b = getattr(rep, f), getattr(w_rep, f)
        assert (np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)) if isinstance(a, float) else a == b, (tag, f, a, b)
    if info is not None:
        assert info["status"] == w_info["status"] == 0 and (info["n_line"], info["n_plane"]) == (w_info["n_line"], w_info["n_plane"]), tag
        for f in ("H", "g"):
            assert np.array_equal(u64(info[f]), u64(w_info[f])), (tag, f)
        assert np.float64(info["cost"]).view(np.uint64) == np.float64(w_info["cost"]).view(np.uint64), tag


# ------------------------------------------------------------------------------------------------ 1, 3, 4
@pytest.mark.parametrize("down", [False, True], ids=["plain", "downsampled"])
def test_ranges_are_per_slot(rig, down):
    """three scans against ONE map handle in all slots, three ranges: every slot is its single-map deblur registration, information
    record included; and the range matters -- slot 1 under slot 0's range ends somewhere else"""
    reg = rig["reg"]
    res, pc, pi, reps = batch(rig, 3, [0, 0, 0], RANGES[:3], down)
    infos = reg.information(3)
    assert res.tolist() == [1, 1, 1] and not any(r.gated for r in reps)
    for b in range(3):
        same_slot(f"slot {b} of 3, one map", (int(res[b]), pc[b], pi[b], reps[b], infos[b]), single(rig, b, 0, RANGES[b], down))
    wrong = [RANGES[0], RANGES[0], RANGES[2]]
    res_w, pc_w, pi_w, reps_w = batch(rig, 3, [0, 0, 0], wrong, down)
    dt, dr = synth.pose_error(pc_w[1], pc[1])
    print(f"slot 1 with slot 0's range: {dt:.2e} m {dr:.2e} rad away from its own")
    assert not np.array_equal(u64(pc_w[1]), u64(pc[1]))
    assert np.array_equal(u64(pc_w[0]), u64(pc[0])) and np.array_equal(u64(pc_w[2]), u64(pc[2]))   # ... and its neighbours do not notice
    same_slot("slot 1 under slot 0's range", (int(res_w[1]), pc_w[1], pi_w[1], reps_w[1], None), single(rig, 1, 0, RANGES[0], down))


# ------------------------------------------------------------------------------------------------ 2
def test_map_per_slot_with_an_idle_and_a_gated_slot(rig):
    """three maps and three ranges in the running slots 0 .. 2, slot 3 idle (None), slot 4 gated by its frame index"""
    reg = rig["reg"]
    fi = np.array([100, 100, 100, 100, 10], np.int32)
    res, pc, pi, reps = batch(rig, S, [0, 1, 2, None, 1], RANGES, False, fi)
    infos = reg.information(S)
    it = reg.interpolation(S)
    assert [r.gated for r in reps] == [0, 0, 0, 1, 1] and res.tolist() == [1] * S
    cases = []
    for b in range(3):
        same_slot(f"slot {b} of {S}, map {b}", (int(res[b]), pc[b], pi[b], reps[b], infos[b]), single(rig, b, b, RANGES[b], False))
        assert it["theta"][b] > 1e-5   # a moving scan: there is an increment to interpolate
        f = rig["fe"].get_features(scan=b)
        corner, surf = rig["clouds"][b]
        prm = H.oracle_params(ICP, 1, RANGES[b][0], RANGES[b][1])
        ret, opc, _, orep = orc.reg_solve(orc.KdTree(corner), orc.KdTree(surf), f["pc_corners"], f["pc_surface"], prm, rig["poses"][b], rig["poses"][b])
        cases.append(G.Case(f"slot {b}", f["pc_corners"], f["pc_surface"], rig["poses"][b], ret, opc, orep))
    G.check_oracle("reg_solve_big_maps_kernel", cases, res[:3], pc[:3], reps[:3])
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    for b in (3, 4):   # idle and gated: nothing was estimated -- pose untouched, status 1, and the deskew record is the identity increment
        assert np.array_equal(pc[b], rig["poses"][b]) and infos[b]["status"] == 1
        assert it["theta"][b] == 0.0 and not it["omega_hat"][b].any() and np.array_equal(it["pose_incre"][b], ident)
    c = rig["fe"].get_features(scan=4)["pc_surface"]
    assert np.array_equal(reg.pointcloudAssociateToMap(c, if_undistore=1, slot=4).view(np.uint32), reg.pointcloudAssociateToMap(c, rig["poses"][4]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5
def test_deskew_records_carry_the_slots_range(rig):
    import torch
    reg, fe = rig["reg"], rig["fe"]
    res, pc, pi, reps = batch(rig, 3, [0, 1, 2], RANGES[:3], False)
    it = reg.interpolation(3)
    assert np.array_equal(it["pose_incre"], pi) and np.array_equal(it["pose_last"], rig["poses"][:3])
    feats = [fe.get_features(scan=b) for b in range(3)]
    stamps = [fe.pts_info(b)["time_stamp"] for b in range(3)]
    acc = np.ones(3, np.int32)
    out = torch.zeros((3 * N, 4), dtype=torch.float32, device="cuda")
    for kind in (0, 1, 2):
        clouds = []
        for b in range(3):
            if kind == 2:   # the full selection with intensity := time stamp (LFE:246,255)
                full = rig["scans"][b].xyzi[feats[b]["full_idx"]].copy()
                full[:, 3] = stamps[b][feats[b]["full_idx"]]
                clouds.append(full)
            else:
                clouds.append(feats[b]["pc_corners" if kind == 0 else "pc_surface"])
        n = reg.cloud_undistort_fe_device(fe, 3, kind, acc, out, 0)
        host = out[:n].cpu().numpy()
        assert n == sum(len(c) for c in clouds)
        at = 0
        for b in range(3):
            got = host[at:at + len(clouds[b])]
            at += len(clouds[b])
            ok = np.isfinite(clouds[b][:, :3]).all(axis=1)
            want = ur.undistort(clouds[b][ok], it["pose_last"][b], pc[b], it["pose_incre"][b], it["theta"][b], it["omega_hat"][b], 1, *RANGES[b])
            ur.check_rule(got[ok, :3], want, f"ll_cloud_undistort_fe_device kind {kind} slot {b}")
            assert np.array_equal(got[:, 3].view(np.uint32), clouds[b][:, 3].view(np.uint32))
            if kind == 1 and b > 0:   # ... and not slot 0's range: the restatement under it lies elsewhere
                other = ur.undistort(clouds[b][ok], it["pose_last"][b], pc[b], it["pose_incre"][b], it["theta"][b], it["omega_hat"][b], 1, *RANGES[0])
                assert np.abs(other - got[ok, :3]).max() > 1e-3
    c = feats[1]["pc_surface"]
    want = ur.undistort(c, it["pose_last"][1], pc[1], it["pose_incre"][1], it["theta"][1], it["omega_hat"][1], 1, *RANGES[1])
    ur.check_rule(reg.pointcloudAssociateToMap(c, if_undistore=1, slot=1)[:, :3], want, "ll_cloud_undistort slot 1")


# ------------------------------------------------------------------------------------------------ 6
def test_refusals_leave_a_working_handle(rig):
    reg, fe = rig["reg"], rig["fe"]
    lo, hi = [r[0] for r in RANGES], [r[1] for r in RANGES]
    pl = rig["poses"][:3]
    tab = [rig["maps"][0]] * 3
    set_params(reg, 1)
    with pytest.raises(capi.LoamLivoxError, match="n_scans"):
        reg.set_time_ranges(lo + [0.0], hi + [1.0])                  # beyond max_scans
    with pytest.raises(capi.LoamLivoxError, match="deblur"):          # no table pending: refused as ever
        reg.enqueue_fe_maps(tab, fe, 3, pl, pl)
    reg.set_time_ranges(lo[:2], hi[:2])                               # a table of the wrong length
    with pytest.raises(capi.LoamLivoxError, match="n_scans"):
        reg.enqueue_fe_maps(tab, fe, 3, pl, pl)
    with pytest.raises(capi.LoamLivoxError, match="deblur"):          # ... which that enqueue took with it
        reg.enqueue_fe_maps(tab, fe, 3, pl, pl)
    reg.set_time_ranges(lo[:3], hi[:3])                               # a table pending at a single-map enqueue: refused and dropped
    with pytest.raises(capi.LoamLivoxError, match="time ranges"):
        reg.enqueue_fe(rig["maps"][0], fe, 3, pl, pl)
    set_params(reg, 1, RANGES[0])
    reg.enqueue_fe(rig["maps"][0], fe, 3, pl, pl)                     # the table is gone: the single-map deblur registration runs
    assert reg.collect(3)[0].tolist() == [1, 1, 1]
    flags = getattr(reg, "debug_flags", 0)
    reg.set_debug(False, force_general_solver=True)                   # a scan the single-map entry points would hand to solve_general
    reg.set_time_ranges(lo[:3], hi[:3])
    with pytest.raises(capi.LoamLivoxError, match="compact solver"):
        reg.enqueue_fe_maps(tab, fe, 3, pl, pl)
    reg.set_debug_flags(flags)
    set_params(reg, 0)                                                # without deblur a pending table is taken and not used
    reg.enqueue_fe_maps(tab, fe, 3, pl, pl)
    plain = reg.collect(3)
    reg.set_time_ranges(lo[:3], hi[:3])
    reg.enqueue_fe_maps(tab, fe, 3, pl, pl)
    tabled = reg.collect(3)
    assert np.array_equal(u64(plain[1]), u64(tabled[1])) and plain[0].tolist() == tabled[0].tolist()
    res, pc, pi, reps = batch(rig, 3, [0, 0, 0], RANGES[:3], False)   # and the handle still works
    same_slot("after the refusals, slot 2", (int(res[2]), pc[2], pi[2], reps[2], None), single(rig, 2, 0, RANGES[2], False))


# ------------------------------------------------------------------------------------------------ 7
def test_selection_last_against_the_full_selection(rig):
    fe = Livox_laser(max_points=N, max_scans=3, piecewise_number=1)
    empty = np.zeros((1, 0, 4), np.float32)
    for s, xyzi in enumerate((rig["scans"][0].xyzi[None], empty, rig["scans"][2].xyzi[None, :7001])):   # slot 1 holds no points
        fe.upload(xyzi, np.full(1, T0[s]), first_scan=s)
    fe.extract_batch(3)
    fe.resolve()
    fe.select_batch(3, -1, 0.0, 1.0)
    for kind, name in ((2, "full_idx"), (0, "corner_idx"), (1, "surf_idx")):
        last = fe.selection_last(3, kind)
        want = [int(idx[-1]) if len(idx) else -1 for idx in (fe.get_features(scan=s)[name] for s in range(3))]
        assert last.dtype == np.int32 and last.tolist() == want, (kind, last, want)
        assert want[1] == -1 and want[0] > 0 and want[2] > 0
    assert fe.selection_last(3, 2)[0] == fe.full_selection(0)[-1] and fe.selection_last(1, 2).tolist() == [int(fe.full_selection(0)[-1])]
    for bad in ((0, 2), (4, 2), (3, 3), (3, -1)):
        with pytest.raises(capi.LoamLivoxError):
            fe.selection_last(*bad)
    fe.close()
