"""-m gpu: the registration information on the device (ll_reg_set_information / ll_reg_information; tests/test_reg_information_host.py is the
CPU tier).

The reference record of a scan is the oracle's: the pose of the scan's last linearisation from a registration stopped one ICP iteration
earlier (the registrar is deterministic), the features moved there by orc.cloud_transform, neighbours by orc.KdTree, the activity
decisions made here (five neighbours inside the match radius, |a - b| >= 1e-4 for a line, a non-degenerate triple 0, 2, 4 for a plane),
blocks by orc.make_block_line / make_block_plane, summed by orc.blocks_eval at the device's pose_incre.  Bound: tests/reg_info_inputs.py."""
import ctypes as C

import numpy as np
import pytest

from loam_livox_amd import api, capi, synth
from loam_livox_amd.api import Livox_laser, Map_buffer, Point_cloud_registration, VoxelGrid
from oracle import orc
from tests import reg_info_inputs as ri
from tests.conftest import oracle_features
from tests.test_solver_size_classes_host import header_constant

pytestmark = pytest.mark.gpu

LL_SMALL_MAX_BLOCKS = header_constant("LL_SMALL_MAX_BLOCKS", "ll_device.h")
LL_GRP_MIN_BLOCKS = header_constant("LL_GRP_MIN_BLOCKS", "ll_device.h")
LL_KNN_TILE_MIN_SURF = header_constant("LL_KNN_TILE_MIN_SURF", "ll_device.h")
CAP = 8192
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_record(a, b):
    return (np.array_equal(bits(a["H"]), bits(b["H"])) and np.array_equal(bits(a["g"]), bits(b["g"])) and bits([a["cost"]])[0] == bits([b["cost"]])[0]
            and (a["n_line"], a["n_plane"], a["status"]) == (b["n_line"], b["n_plane"], b["status"]))


@pytest.fixture(scope="module")
def dev_map(gpu_lib, small_world):
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, small_world["corner"])
    m.setInputCloud(Map_buffer.SURF, small_world["surf"])
    yield m
    m.close()


@pytest.fixture(scope="module")
def feats(scans):
    """per scan: its feature clouds thinned to the three sizes the solver forms switch at"""
    out = []
    for sc in scans:
        fe_o, _, _, _, fc, fs = oracle_features(sc)
        small = (fc[:150], fs[::12][:LL_KNN_TILE_MIN_SURF + 100])        # the small solver (and enough surface queries for the tile search)
        table = (fc[:250], fs[::4][:4000])                                # one workgroup of the table solver
        group = (fc, fs[::2][:LL_GRP_MIN_BLOCKS])                         # a group of workgroups
        assert len(small[0]) + len(small[1]) <= LL_SMALL_MAX_BLOCKS < len(table[0]) + len(table[1]) < LL_GRP_MIN_BLOCKS <= len(group[0]) + len(group[1]) <= CAP
        out.append(dict(small=small, table=table, group=group, ts=(float(fe_o.time_stamp.min()), float(fe_o.time_stamp.max()))))
    return out


def set_params(reg, icp, force=1, deblur=0, ts=(0.0, 1.0)):
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = icp, 20, force
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    p.if_motion_deblur, p.minimum_pt_time_stamp, p.maximum_pt_time_stamp = deblur, ts[0], ts[1]
    return p


def register(m, clouds, poses, icp, force=1, deblur=0, ts=(0.0, 1.0), information=True, debug=None, max_scans=None, tweak=None, tap=None):
    """one batch through upload_features / enqueue_uploaded / collect -> (res, pc, pi, reps, records or None[, the neighbour tap])"""
    n = len(clouds)
    reg = Point_cloud_registration(max_scans=max_scans or n, max_features=CAP)
    reg.set_debug(tap is not None, **(debug or {}))
    set_params(reg, icp, force, deblur, ts)
    if tweak:
        tweak(reg.params)
    if tap is not None:
        reg.set_debug_knn_iteration(tap)
    reg.set_information(information)
    reg.upload_features([c[0] for c in clouds], [c[1] for c in clouds])
    pl = np.ascontiguousarray(poses, np.float64).reshape(n, 7)
    reg.enqueue_uploaded(m, n, pl, pl)
    out = reg.collect(n)
    out = out + (reg.information(n) if information else None,)
    if tap is not None:
        out = out + ([reg.debug_knn(b, len(clouds[b][0]), len(clouds[b][1])) for b in range(n)],)
    reg.close()
    return out


def oracle_blocks(world, cloud, pose_last, pose_lin, deblur=0, ts=(0.0, 1.0), neighbours=None):
    """the blocks of the linearisation at pose_lin, corner candidates first -> (blocks, n_line, n_plane).  neighbours: (corner idx [n, 5],
    surface idx [n, 5]) instead of the oracle's search (motion deblur: the oracle has no interpolated transform to search from)"""
    blocks, counts = [], []
    for kind, (f, pts, tree, thr) in enumerate(((cloud[0], world["corner"], world["tree_c"], 2.0), (cloud[1], world["surf"], world["tree_s"], 50.0))):
        n = 0
        if len(f):
            if neighbours is None:
                q = orc.cloud_transform(pose_lin, f)
                ok = np.isfinite(f[:, :3]).all(axis=1)
                idx, d2 = tree.knn(np.where(ok[:, None], q[:, :3], 1e9).astype(np.float32), 5)
                found = ok & (idx[:, 4] >= 0) & (d2[:, 4].astype(np.float64) < thr)
            else:
                idx = neighbours[kind]
                found = idx[:, 4] >= 0
            for i in np.nonzero(found)[0]:
                s = ri.refine_blur(f[i, 3], ts[0], ts[1]) if deblur else 1.0
                fd = f[i, :3].astype(np.float64)
                if kind == 0:
                    a, b = pts[idx[i, 0], :3].astype(np.float64), pts[idx[i, 1], :3].astype(np.float64)
                    if np.sqrt(((a - b) ** 2).sum()) < 1e-4:   # PCR:302
                        continue
                    blocks.append(orc.make_block_line(fd, a, b, s))
                else:
                    a, b, c = (pts[idx[i, k], :3].astype(np.float64) for k in (0, 2, 4))
                    if not (b - a).any() or not (c - a).any():
                        continue
                    blocks.append(orc.make_block_plane(fd, a, b, c, s))
                n += 1
        counts.append(n)
    return blocks, counts[0], counts[1]


def assert_reference(world, cloud, pose_last, pose_lin, x, rec, what, deblur=0, ts=(0.0, 1.0), neighbours=None, blocks=None):
    if blocks is None:
        blocks = oracle_blocks(world, cloud, pose_last, pose_lin, deblur, ts, neighbours)
    bl, n_line, n_plane = blocks
    assert rec["status"] == 0 and (rec["n_line"], rec["n_plane"]) == (n_line, n_plane), (what, rec["n_line"], rec["n_plane"], n_line, n_plane)
    ref = ri.oracle_record(bl, pose_last, x, deblur=deblur, huber_a=0.1)
    worst = ri.worst_ratio(rec, ref)
    print(f"{what}: {n_line} lines, {n_plane} planes, worst |v - v_orc| / bound = {worst:.3g}")
    assert worst <= 1.0, what
    assert np.array_equal(rec["H"], rec["H"].T)
    assert np.array_equal(rec["eigenvalues"], np.linalg.eigh(rec["H"])[0])
    return blocks


def pose_of_last_linearisation(m, cloud, pose, iterations, **kw):
    """the scan alone, stopped one ICP iteration before its last"""
    if iterations <= 1:
        return np.asarray(pose, np.float64).copy()
    _, pc, _, reps, _ = register(m, [cloud], [pose], iterations - 1, information=False, **kw)
    assert reps[0].icp_iterations == iterations - 1
    return pc[0]


# ------------------------------------------------------------------------------------------------ the reference record
@pytest.mark.parametrize("K", [1, 4])
def test_record_equals_the_oracles(dev_map, small_world, scans, feats, K):
    clouds = [feats[0]["table"], feats[1]["table"]]
    poses = [scans[0].pose_init, scans[1].pose_init]
    res, pc, pi, reps, infos = register(dev_map, clouds, poses, K)
    for b in range(2):
        assert reps[b].icp_iterations == K
        lin = pose_of_last_linearisation(dev_map, clouds[b], poses[b], K, debug=dict(no_solver_groups=True))
        assert_reference(small_world, clouds[b], poses[b], lin, pi[b], infos[b], f"K={K} scan {b}")
        assert infos[b]["n_line"] + infos[b]["n_plane"] >= reps[b].n_blocks_last   # (the solve pruned its set; the record does not)


def test_a_scan_that_converges_early_keeps_its_own_last_iteration(dev_map, small_world, scans, feats):
    """one scan starts at its solution and converges before the batch's last iteration, the other does not: the early one's buffers are
    still those of its own last iteration when the kernel runs"""
    cloud = feats[0]["table"]
    _, pc0, _, _, _ = register(dev_map, [cloud], [scans[0].pose_init], 8, information=False)
    clouds, poses = [cloud, feats[1]["table"]], [pc0[0], scans[1].pose_init]
    res, pc, pi, reps, infos = register(dev_map, clouds, poses, 8, force=0)
    its = [reps[b].icp_iterations for b in range(2)]
    assert its[0] < its[1], its
    for b in range(2):
        lin = pose_of_last_linearisation(dev_map, clouds[b], poses[b], its[b], force=0, debug=dict(no_solver_groups=True))
        assert_reference(small_world, clouds[b], poses[b], lin, pi[b], infos[b], f"early convergence scan {b} ({its[b]} iterations)")


# ------------------------------------------------------------------------------------------------ every form
def test_every_solver_and_search_form_gives_the_scans_record(dev_map, small_world, scans, feats):
    """group of workgroups / one workgroup (bit 5) / general path (bit 1), with and without neighbour reuse, the tile search (bit 11) on a
    batch of three: each equals the reference at its own increment; forms whose increments have the same bits give the same bits"""
    K = 4
    cloud, pose = feats[0]["group"], scans[0].pose_init
    runs = {}
    for name, debug in (("group", {}), ("one workgroup", dict(no_solver_groups=True)), ("general", dict(force_general_solver=True)),
                        ("no reuse", dict(no_knn_reuse=True)), ("one workgroup, no reuse", dict(no_solver_groups=True, no_knn_reuse=True))):
        _, _, pi, reps, infos = register(dev_map, [cloud], [pose], K, debug=debug)
        assert reps[0].icp_iterations == K and reps[0].aborted == 0
        runs[name] = (pi[0], infos[0])
    others = [feats[1]["group"], feats[2]["group"]]
    _, _, pi, reps, infos = register(dev_map, [others[0], others[1], cloud], [scans[1].pose_init, scans[2].pose_init, pose], K,
                                     debug=dict(knn_tile_small_batches=True))
    runs["tile search, slot 2 of 3"] = (pi[2], infos[2])
    lin = pose_of_last_linearisation(dev_map, cloud, pose, K, debug=dict(no_solver_groups=True))
    blocks = None
    for name, (x, rec) in runs.items():
        blocks = assert_reference(small_world, cloud, pose, lin, x, rec, name, blocks=blocks)
    names = list(runs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if np.array_equal(bits(runs[a][0]), bits(runs[b][0])):
                assert same_record(runs[a][1], runs[b][1]), (a, b)
    # the search forms leave the same lists, so these pairs do have the same increment
    for a, b in (("group", "no reuse"), ("one workgroup", "one workgroup, no reuse")):
        assert np.array_equal(bits(runs[a][0]), bits(runs[b][0])) and same_record(runs[a][1], runs[b][1]), (a, b)


def test_small_solver_and_tile_search_on_a_small_scan(dev_map, small_world, scans, feats):
    K = 4
    cloud, pose = feats[1]["small"], scans[1].pose_init
    _, _, pi, reps, infos = register(dev_map, [cloud], [pose], K)
    lin = pose_of_last_linearisation(dev_map, cloud, pose, K)
    blocks = assert_reference(small_world, cloud, pose, lin, pi[0], infos[0], "small solver")
    batch = [feats[0]["small"], cloud, feats[2]["small"]]
    _, _, pi3, _, infos3 = register(dev_map, batch, [scans[0].pose_init, pose, scans[2].pose_init], K, debug=dict(knn_tile_small_batches=True))
    assert_reference(small_world, cloud, pose, lin, pi3[1], infos3[1], "small solver behind the tile search", blocks=blocks)
    if np.array_equal(bits(pi[0]), bits(pi3[1])):
        assert same_record(infos[0], infos3[1])


def test_motion_deblur_through_the_big_path(dev_map, small_world, scans, feats):
    K = 3
    cloud, pose, ts = feats[1]["table"], scans[1].pose_init, feats[1]["ts"]
    # (no neighbour reuse: every query is searched, and so recorded by the tap, in the last iteration too)
    _, _, pi, reps, infos, taps = register(dev_map, [cloud], [pose], K, deblur=1, ts=ts, tap=K - 1, debug=dict(no_knn_reuse=True))
    assert reps[0].icp_iterations == K
    ci, _, si, _ = taps[0]
    # the neighbour lists of the last iteration from the debug tap (original map indices); the decisions on them are made here
    assert_reference(small_world, cloud, pose, None, pi[0], infos[0], "motion deblur", deblur=1, ts=ts, neighbours=(ci, si))


# ------------------------------------------------------------------------------------------------ slots, batches, a map per slot
def test_a_scans_record_does_not_depend_on_slot_batch_or_map_form(gpu_lib, dev_map, small_world, scans):
    """the scan alone, in slot 2 of 3, and through enqueue_fe_maps with three different maps: bit for bit the same record"""
    S = 3
    other = [Map_buffer(), Map_buffer()]
    for k, m in enumerate(other):
        m.setInputCloud(Map_buffer.CORNER, small_world["corner"][k::2])
        m.setInputCloud(Map_buffer.SURF, small_world["surf"][k::2])
    poses = np.stack([scans[b].pose_init for b in range(S)])

    def run(n_slots, maps):
        fe = Livox_laser(max_points=24000, max_scans=n_slots, piecewise_number=1)
        batch = np.stack([scans[b].xyzi for b in (range(S) if n_slots == S else [2])])
        fe.upload(batch, np.full(n_slots, 1.0))
        fe.extract_batch(n_slots); fe.resolve(); fe.select_batch(n_slots, -1, 0.0, 1.0)
        reg = Point_cloud_registration(max_scans=n_slots, max_features=24000)
        vox = (VoxelGrid(24000, n_slots), VoxelGrid(24000, n_slots))
        set_params(reg, 4)
        reg.set_information(True)
        pl = poses if n_slots == S else poses[2:3]
        if maps is None:
            reg.enqueue_fe_downsampled(dev_map, fe, vox[0], vox[1], 0.1, 0.4, n_slots, pl, pl)
        else:
            reg.enqueue_fe_downsampled_maps(maps, fe, vox[0], vox[1], 0.1, 0.4, n_slots, pl, pl)
        out = reg.collect(n_slots) + (reg.information(n_slots),)
        for h in (fe, reg) + vox:
            h.close()
        return out

    alone, batch, maps = run(1, None), run(S, None), run(S, [other[0], other[1], dev_map])
    assert alone[4][0]["status"] == 0 and alone[4][0]["n_plane"] > 100
    for name, got in (("slot 2 of 3", batch), ("a map per slot", maps)):
        assert np.array_equal(bits(alone[2][0]), bits(got[2][2])), name
        assert same_record(alone[4][0], got[4][2]), name
    assert not same_record(maps[4][0], batch[4][0])   # (the other slots did see other maps)
    for m in other:
        m.close()


# ------------------------------------------------------------------------------------------------ status codes
def test_status_codes(dev_map, scans, feats):
    cloud, pose = feats[0]["group"], scans[0].pose_init
    empty = (np.zeros((0, 4), np.float32), np.zeros((0, 4), np.float32))

    def gated(p):
        p.current_frame_index = 10
    _, _, _, reps, infos = register(dev_map, [cloud], [pose], 3, tweak=gated)
    assert reps[0].gated == 1 and infos[0]["status"] == 1 and not infos[0]["H"].any() and infos[0]["n_plane"] == 0
    _, _, _, reps, infos = register(dev_map, [empty, feats[1]["small"]], [pose, scans[1].pose_init], 3)
    assert infos[0]["status"] == 1 and not infos[0]["H"].any() and infos[1]["status"] == 0 and infos[1]["n_plane"] > 100
    # an aborted slot: the grouped solver gives up at once (test_group_abort)
    reg = Point_cloud_registration(max_scans=1, max_features=CAP)
    reg.set_debug(False, test_group_abort=True)
    set_params(reg, 3)
    reg.set_information(True)
    reg.upload_features([cloud[0]], [cloud[1]])
    pl = pose.reshape(1, 7).copy()
    reg.enqueue_uploaded(dev_map, 1, pl, pl)
    pc, pi = np.zeros((1, 7)), np.zeros((1, 7))
    reps, res = (capi.RegReport * 1)(), np.ones(1, np.int32)
    assert reg.L.ll_reg_collect(reg.h, 1, capi.ptr(pc), capi.ptr(pi), reps, capi.ptr(res)) == 1 and reps[0].aborted == 1
    info = reg.information(1)[0]
    assert info["status"] == 2 and not info["H"].any() and not info["g"].any() and info["cost"] == 0.0
    reg.close()

    # a rejected scan is computed like any other
    def reject(p):
        p.max_final_cost = 1e-6
    _, _, _, reps_ok, infos_ok = register(dev_map, [cloud], [pose], 3)
    res, pc, _, reps, infos = register(dev_map, [cloud], [pose], 3, tweak=reject)
    assert res[0] == 0 and reps[0].accepted == 0 and np.array_equal(pc[0], pose)
    assert infos[0]["status"] == 0 and same_record(infos[0], infos_ok[0]) and infos[0]["n_plane"] > 1000


# ------------------------------------------------------------------------------------------------ the wall
def test_a_wall_on_the_device(gpu_lib):
    """one ICP iteration against a map whose surface points all have z == 0 exactly, the corner map out of match range: rotation about z
    and translation along x, y are exactly unconstrained, the other three directions are constrained"""
    rng = np.random.default_rng(4)
    gx, gy = np.meshgrid(np.arange(-10, 10, 0.1), np.arange(-10, 10, 0.1))
    surf = np.c_[gx.ravel() + rng.uniform(-0.03, 0.03, gx.size), gy.ravel() + rng.uniform(-0.03, 0.03, gx.size), np.zeros(gx.size)].astype(np.float32)
    corner = (np.array([1000.0, 1000.0, 1000.0]) + rng.uniform(-1, 1, (100, 3))).astype(np.float32)
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, corner)
    m.setInputCloud(Map_buffer.SURF, surf)
    pose = np.r_[synth.quat_from_axis_angle(np.array([0.0, 0.0, 1.0]), 0.3), 0.2, -0.4, 1.5]
    fs = np.c_[rng.uniform(-6, 6, (700, 2)), -1.5 + rng.normal(0, 0.02, 700), np.ones(700)].astype(np.float32)
    fc = np.c_[rng.uniform(-6, 6, (20, 3)), np.ones(20)].astype(np.float32)
    _, _, _, reps, infos = register(m, [(fc, fs)], [pose], 1)
    m.close()
    rec = infos[0]
    assert rec["status"] == 0 and rec["n_line"] == 0 and rec["n_plane"] == 700 and reps[0].icp_iterations == 1
    H, free, held = rec["H"], [2, 3, 4], [0, 1, 5]
    assert np.all(H[free, :] == 0.0) and np.all(H[:, free] == 0.0) and np.all(rec["g"][free] == 0.0)
    assert np.all(np.linalg.eigvalsh(H[np.ix_(held, held)]) > 0.0)


# ------------------------------------------------------------------------------------------------ the switch
def test_switch_off_changes_nothing_and_switch_on_adds_one_launch_and_no_wait(dev_map, scans, feats):
    clouds, poses = [feats[0]["table"], feats[1]["small"], feats[2]["table"]], [scans[b].pose_init for b in range(3)]
    out = {}
    for on in (False, True):
        reg = Point_cloud_registration(max_scans=3, max_features=CAP)
        set_params(reg, 4, force=0)
        reg.set_profiling(True)
        if on:
            reg.set_information(True)
        reg.upload_features([c[0] for c in clouds], [c[1] for c in clouds])
        pl = np.stack(poses)
        reg.enqueue_uploaded(dev_map, 3, pl, pl)
        res, pc, pi, reps = reg.collect(3)          # the one wait of a registration; information() below is a host copy
        ms, launches = reg.kernel_times()
        out[on] = (res, pc, pi, [tuple(getattr(r, f) for f, _ in capi.RegReport._fields_) for r in reps], launches.copy(), reg.information_time())
        if on:
            first = reg.information(3)
            assert all(same_record(a, b) for a, b in zip(first, reg.information(3))) and first[0]["status"] == 0
        reg.close()
    off, on = out[False], out[True]
    assert np.array_equal(off[0], on[0]) and np.array_equal(bits(off[1]), bits(on[1])) and np.array_equal(bits(off[2]), bits(on[2])) and off[3] == on[3]
    assert np.array_equal(off[4], on[4]) and off[4][2] == 1      # the same launches in the classes ll_reg_kernel_times reports
    assert off[5] == 0.0 and on[5] > 0.0
    print(f"information kernel, 3 scans: {on[5] * 1e3:.1f} us")


def test_refusals_carry_their_text_and_leave_the_handle_usable(dev_map, scans, feats):
    L = capi.load()
    cloud, pose = feats[1]["small"], scans[1].pose_init.reshape(1, 7).copy()
    reg = Point_cloud_registration(max_scans=2, max_features=CAP)
    set_params(reg, 2)
    recs = (capi.RegInformation * 2)()

    def refused(rc, text):
        msg = L.ll_last_error().decode()
        assert rc != 0 and "ll_reg_information" in msg and text in msg, (rc, msg)

    refused(L.ll_reg_information(reg.h, 1, recs), "collected")                 # before any collect
    reg.upload_features([cloud[0]], [cloud[1]])
    reg.enqueue_uploaded(dev_map, 1, pose, pose)
    refused(L.ll_reg_information(reg.h, 1, recs), "collected")                 # enqueued, not collected
    reg.collect(1)
    refused(L.ll_reg_information(reg.h, 1, recs), "switch off")                # the enqueue was made with the switch off
    reg.set_information(True)
    refused(L.ll_reg_information(reg.h, 1, recs), "switch off")                # ... the switch holds from the next enqueue on
    reg.enqueue_uploaded(dev_map, 1, pose, pose)
    reg.collect(1)
    refused(L.ll_reg_information(reg.h, 2, recs), "n_scans")
    refused(L.ll_reg_information(reg.h, 1, None), "null output")
    refused(L.ll_reg_information(None, 1, recs), "null handle")
    good = reg.information(1)[0]                                               # the handle is usable, the records still there
    assert good["status"] == 0 and good["n_plane"] > 100
    reg.set_information(False)
    reg.enqueue_uploaded(dev_map, 1, pose, pose)
    reg.collect(1)
    with pytest.raises(capi.LoamLivoxError, match="switch off"):
        reg.information(1)
    reg.close()


# ------------------------------------------------------------------------------------------------ the loops
MAP_ARGS = dict(maximum_history_size=5, init_accumulate_frames=2, line_res=0.1, plane_res=0.15, icp_max_iterations=6, ceres_max_iterations=20,
                max_allow_incre_R=20.0, max_allow_incre_T=0.3)
N_PTS = 12000


def standalone_information(lm, xyzi):
    """the registration Laser_mapping is about to make of this scan, on handles of its own, against lm's map"""
    fe = Livox_laser(max_points=N_PTS, max_scans=1, piecewise_number=1)
    fe.upload(xyzi[None], np.full(1, 1.0))
    fe.extract_batch(1); fe.resolve(); fe.select_batch(1, -1, 0.0, 1.0)
    reg = Point_cloud_registration(max_scans=1, max_features=N_PTS)
    vox = (VoxelGrid(N_PTS, 1), VoxelGrid(N_PTS, 1))
    C.memmove(C.byref(reg.params), C.byref(lm.reg.params), C.sizeof(capi.RegParams))
    reg.params.current_frame_index = lm.m_current_frame_index
    reg.set_information(True)
    pose = lm.pose[None]
    reg.enqueue_fe_downsampled(lm.map, fe, vox[0], vox[1], lm.line_res, lm.plane_res, 1, pose, pose)
    reg.collect(1)
    info = reg.information(1)[0]
    for h in (fe, reg) + vox:
        h.close()
    return info


def test_laser_mapping_with_information(gpu_lib, small_world):
    from loam_livox_amd.mapping import Laser_mapping
    from tests.test_mapping_sequence import make_sequence
    frames, _ = make_sequence(small_world["world"], n_frames=60)
    plain, with_info = Laser_mapping(scan_points=N_PTS, **MAP_ARGS), Laser_mapping(scan_points=N_PTS, information=True, **MAP_ARGS)
    computed = 0
    for k, xyzi in enumerate(frames):
        alone = standalone_information(with_info, xyzi)
        pose_before = with_info.pose.copy()
        ra, rb = plain.process_new_scan(xyzi), with_info.process_new_scan(xyzi)
        assert ra == rb and np.array_equal(bits(plain.pose), bits(with_info.pose)), k
        info = with_info.last_information
        assert same_record(info, alone), k
        assert np.array_equal(info["H_pose"], api.information_in_pose_frame(info["H"], pose_before))
        assert info["status"] == (1 if with_info.last_report.gated else 0)
        computed += info["status"] == 0
    assert computed >= 50 and plain.last_information is None
    assert with_info.degenerate_directions(np.inf).shape == (6, 6) and with_info.degenerate_directions(0.0).shape == (0, 6)
    plain.close(); with_info.close()


def test_laser_mapping_batch_with_information(gpu_lib, small_world):
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    S, n = 3, 8
    seqs = [synth.make_livox_sequence(small_world["world"], 77 + s, n_frames=n)[0] for s in range(S)]
    lb = Laser_mapping_batch(S, scan_points=N_PTS, information=True, **MAP_ARGS)
    singles = [Laser_mapping(scan_points=N_PTS, information=True, **MAP_ARGS) for _ in range(S)]
    for k in range(n):
        out = lb.process_new_scans([seqs[s][k] for s in range(S)])
        for s in range(S):
            assert singles[s].process_new_scan(seqs[s][k]) == out[s]
            assert np.array_equal(bits(singles[s].pose), bits(lb.poses[s])), (k, s)
            assert same_record(singles[s].last_information, lb.last_information[s]), (k, s)
            assert np.array_equal(bits(singles[s].last_information["H_pose"]), bits(lb.last_information[s]["H_pose"]))
    assert lb.last_information[0]["status"] == 0 and lb.last_information[0]["n_plane"] > 100
    lb.close()
    for lm in singles:
        lm.close()
