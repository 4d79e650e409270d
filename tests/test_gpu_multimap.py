"""-m gpu: a map per slot (ll_reg_enqueue_fe_maps / ll_reg_enqueue_fe_downsampled_maps) and the lock-step mapping loop built on it
(mapping.Laser_mapping_batch).  The contract is equality: slot b of a batch gives, bit for bit, what the single-map entry point
gives for that scan alone against maps[b]; a sequence of the batched loop gives the bits of Laser_mapping run alone on it.

Inputs: synth.make_livox_sequence( world, seed ), seeds 77 .. 100, under MAP_ARGS of tests/test_mapping_sequence.py (every frame
accepted by the oracle loop, tests/test_multimap_host.py); seed 81 with teleport = ( 4, 2.0 ) is rejected at frame 4 and only there.

The solver forms agree with each other to rounding only, and the single-map launcher picks one per batch from the batch's size and its
largest scan; the map-per-slot launcher picks the form per slot (ll_device.h reg_maps_class).  The cases here cover every boundary of that
choice: four / eight wavefronts of the small solver (1 024 candidate blocks; also where no scan of a batch exceeds it but the largest
corner and surface counts together do), one workgroup / a group (6 000 features, un-filtered scans), and batches of 512 scans."""
import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.capi import LoamLivoxError
from oracle import orc
from oracle.orc_mapping import LaserMapping

pytestmark = pytest.mark.gpu

N_PTS = 12000
SEEDS = list(range(77, 101))
MAP_ARGS = dict(maximum_history_size=5, init_accumulate_frames=2, line_res=0.1, plane_res=0.15, icp_max_iterations=6, ceres_max_iterations=20,
                max_allow_incre_R=20.0, max_allow_incre_T=0.3)
REPORT_FIELDS = ("final_cost", "initial_cost", "inlier_threshold", "angular_diff_deg", "t_diff", "icp_iterations", "n_blocks_last", "corner_avail",
                 "surf_avail", "lm_iterations_total", "accepted", "gated", "aborted")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def report_tuple(rep):
    return tuple(np.float64(getattr(rep, f)).view(np.uint64) if isinstance(getattr(rep, f), float) else getattr(rep, f) for f in REPORT_FIELDS)


def set_params(reg, frame_index=5):
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations = MAP_ARGS["icp_max_iterations"], MAP_ARGS["ceres_max_iterations"]
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = MAP_ARGS["max_allow_incre_R"], MAP_ARGS["max_allow_incre_T"], 100.0
    p.mapping_init_accumulate_frames = MAP_ARGS["init_accumulate_frames"]
    p.maximum_allow_residual_block, p.subsample_seed = N_PTS, 0
    p.current_frame_index = frame_index


@pytest.fixture(scope="module")
def sequences(small_world):
    return {seed: synth.make_livox_sequence(small_world["world"], seed, n_frames=6)[0] for seed in SEEDS}


@pytest.fixture(scope="module")
def built(gpu_lib, sequences):
    """per seed: a Laser_mapping that has taken frames 0 .. 4 (its map is the match buffer of five frames, its pose the start of frame 5)"""
    from loam_livox_amd.mapping import Laser_mapping
    out = {}
    for seed in SEEDS:
        lm = Laser_mapping(scan_points=N_PTS, **MAP_ARGS)
        for k in range(5):
            assert lm.process_new_scan(sequences[seed][k]) == 1
        out[seed] = lm
    yield out
    for lm in out.values():
        lm.close()


class Rig:
    """an extractor, a registrar and two voxel filters for S slots, with the frames given already extracted"""

    def __init__(self, scans):
        from loam_livox_amd.api import Livox_laser, Point_cloud_registration, VoxelGrid
        S = len(scans)
        self.S = S
        self.fe = Livox_laser(max_points=N_PTS, max_scans=S, piecewise_number=1)
        self.reg = Point_cloud_registration(max_scans=S, max_features=N_PTS)
        self.vox = (VoxelGrid(N_PTS, S), VoxelGrid(N_PTS, S))
        set_params(self.reg)
        self.fe.upload(np.stack(scans), np.ones(S))
        self.fe.extract_batch(S)
        self.fe.resolve()
        self.fe.select_batch(S, -1, 0.0, 1.0)

    def close(self):
        for h in (self.fe, self.reg, self.vox[0], self.vox[1]):
            h.close()

    def run_maps(self, maps, poses, downsample=True, frame_index=None, between=None):
        if downsample:
            self.reg.enqueue_fe_downsampled_maps(maps, self.fe, self.vox[0], self.vox[1], MAP_ARGS["line_res"], MAP_ARGS["plane_res"], self.S, poses, poses,
                                                 frame_index)
        else:
            self.reg.enqueue_fe_maps(maps, self.fe, self.S, poses, poses, frame_index)
        if between is not None:
            between()
        return self.reg.collect(self.S)

    def run_one_map(self, m, poses, downsample=True):
        if downsample:
            self.reg.enqueue_fe_downsampled(m, self.fe, self.vox[0], self.vox[1], MAP_ARGS["line_res"], MAP_ARGS["plane_res"], self.S, poses, poses)
        else:
            self.reg.enqueue_fe(m, self.fe, self.S, poses, poses)
        return self.reg.collect(self.S)


def solo(scan, m, pose, downsample=True, frame_index=5):
    rig = Rig([scan])
    set_params(rig.reg, frame_index)
    out = rig.run_one_map(m, pose[None], downsample)
    rig.close()
    return out


def assert_slot_equal(batch, b, alone, what):
    res, pc, pi, reps = batch
    ares, apc, api_, areps = alone
    assert res[b] == ares[0], (what, "result")
    assert np.array_equal(pc[b].view(np.uint64), apc[0].view(np.uint64)), (what, "pose", pc[b] - apc[0])
    assert np.array_equal(pi[b].view(np.uint64), api_[0].view(np.uint64)), (what, "increment")
    assert report_tuple(reps[b]) == report_tuple(areps[0]), (what, "report")


# ---- 1. slots against themselves ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("downsample", [True, False])
@pytest.mark.parametrize("S", [1, 5, 16, 24])
def test_every_slot_equals_its_own_single_map_registration(sequences, built, S, downsample):
    seeds = SEEDS[:S]
    scans = [sequences[s][5] for s in seeds]
    poses = np.stack([built[s].pose for s in seeds])
    rig = Rig(scans)
    batch = rig.run_maps([built[s].map for s in seeds], poses, downsample)
    rig.close()
    sizes = []
    for b, s in enumerate(seeds):
        assert batch[3][b].gated == 0 and batch[3][b].icp_iterations > 0
        sizes.append(batch[3][b].n_blocks_last)
        print(f"S={S} downsample={downsample} slot {b} seed {s}: blocks {batch[3][b].n_blocks_last} result {batch[0][b]}")
        assert_slot_equal(batch, b, solo(scans[b], built[s].map, poses[b], downsample), (S, downsample, s))
    assert min(sizes) > 100


def test_slots_of_a_large_batch_equal_their_single_map_registration(sequences, built):
    """512 slots: from LL_SMALL_W1_MIN_SCANS scans on the single-map batch gives small scans one or two wavefronts each, a scan alone gets
    four, and the forms agree to rounding only -- a slot of a map-per-slot batch must still give the bits of its own registration.  Two
    sequences alternate over the slots (some 450 residual blocks each: four such scans fit a CU, so a single-map batch of this size gives
    them two wavefronts), each with its own map."""
    S, pair = 512, (82, 93)
    scans = [sequences[pair[b % 2]][5] for b in range(S)]
    poses = np.stack([built[pair[b % 2]].pose for b in range(S)])
    rig = Rig(scans)
    batch = rig.run_maps([built[pair[b % 2]].map for b in range(S)], poses)
    rig.close()
    alone = [solo(scans[b], built[pair[b]].map, poses[b]) for b in range(2)]
    assert batch[3][0].corner_avail + batch[3][0].surf_avail < 620 and batch[3][1].corner_avail + batch[3][1].surf_avail < 620
    for b in range(S):
        assert_slot_equal(batch, b, alone[b % 2], (S, pair[b % 2], b))


# ---- 2. one map S times = the single-map batch -----------------------------------------------------------------------------------------
def test_one_map_in_every_slot_equals_the_single_map_batch(sequences, built):
    S, seed = 24, 77
    scans = [sequences[seed][5]] * S
    poses = np.stack([built[seed].pose] * S)
    poses[1::2, 4] += 0.01  # (every other slot starts a centimetre off: the slots do not all do the same work)
    rig = Rig(scans)
    a = rig.run_maps([built[seed].map] * S, poses)
    b = rig.run_one_map(built[seed].map, poses)
    rig.close()
    for k in range(S):
        assert a[0][k] == b[0][k]
        assert np.array_equal(a[1][k].view(np.uint64), b[1][k].view(np.uint64)) and np.array_equal(a[2][k].view(np.uint64), b[2][k].view(np.uint64))
        assert report_tuple(a[3][k]) == report_tuple(b[3][k])
    assert not np.array_equal(a[1][0], a[1][1])


# ---- 3. the gate is per slot ----------------------------------------------------------------------------------------------------------
def test_gate_is_decided_per_slot(sequences, built, small_world):
    from loam_livox_amd.api import Map_buffer
    seeds = SEEDS[:8]
    scans = [sequences[s][5] for s in seeds]
    poses = np.stack([built[s].pose for s in seeds])
    empty = Map_buffer()
    few = Map_buffer()
    few.setInputCloud(Map_buffer.CORNER, small_world["corner"][:500])
    few.setInputCloud(Map_buffer.SURF, small_world["surf"][:40])  # PCR:199 wants more than 50 surface points
    maps = [built[s].map for s in seeds]
    maps[1], maps[3], maps[6] = empty, few, None
    fi = np.full(8, 5, np.int32)
    fi[5] = MAP_ARGS["init_accumulate_frames"]  # not beyond the accumulation phase
    rig = Rig(scans)
    batch = rig.run_maps(maps, poses, frame_index=fi)
    rig.close()
    res, pc, pi, reps = batch
    for b in (1, 3, 5, 6):
        assert reps[b].gated == 1 and res[b] == 1 and reps[b].icp_iterations == 0 and reps[b].accepted == 1
        assert np.array_equal(pc[b], poses[b])
    for b in (0, 2, 4, 7):
        assert reps[b].gated == 0 and reps[b].icp_iterations > 0
        assert_slot_equal(batch, b, solo(scans[b], maps[b], poses[b]), ("gate", b))
    # a gated slot alone comes back the same way
    alone = solo(scans[3], few, poses[3])
    assert alone[3][0].gated == 1
    assert_slot_equal(batch, 3, alone, ("gate", "few"))
    empty.close()
    few.close()


# ---- 4. snapshots -----------------------------------------------------------------------------------------------------------------------
def test_maps_are_pinned_from_enqueue_to_collect(sequences, built, small_world):
    from loam_livox_amd.api import Map_buffer
    seeds = SEEDS[:5]
    scans = [sequences[s][5] for s in seeds]
    poses = np.stack([built[s].pose for s in seeds])
    own = []
    for s in seeds:  # copies of the match buffers: the test replaces one of them
        m = Map_buffer()
        for kind in (0, 1):
            m.setInputCloud(kind, built[s].history.map_cloud(kind))
        own.append(m)
    rig = Rig(scans)
    before = rig.run_maps(own, poses)

    def replace():
        own[2].setInputCloud(Map_buffer.CORNER, small_world["corner"][:3000])
        own[2].setInputCloud(Map_buffer.SURF, small_world["surf"][:20000])

    during = rig.run_maps(own, poses, between=replace)
    after = rig.run_maps(own, poses)
    rig.close()
    for b in range(5):
        assert np.array_equal(before[1][b], during[1][b]) and report_tuple(before[3][b]) == report_tuple(during[3][b])
    assert report_tuple(after[3][2]) != report_tuple(before[3][2])  # (the next enqueue does see the new map)
    for b in (0, 1, 3, 4):
        assert np.array_equal(before[1][b], after[1][b])
    for m in own:
        m.close()


# ---- 5. against the oracle ----------------------------------------------------------------------------------------------------------------
def test_slots_match_the_oracle(sequences, built):
    seeds = SEEDS[:5]
    scans = [sequences[s][5] for s in seeds]
    poses = np.stack([built[s].pose for s in seeds])
    rig = Rig(scans)
    res, pc, _, reps = rig.run_maps([built[s].map for s in seeds], poses)
    rig.close()
    prm = orc.RegParams.defaults(icp_iters=MAP_ARGS["icp_max_iterations"], ceres_iters=MAP_ARGS["ceres_max_iterations"], force_all=0)
    prm.para_max_angular_rate, prm.para_max_speed, prm.max_final_cost = MAP_ARGS["max_allow_incre_R"], MAP_ARGS["max_allow_incre_T"], 100.0
    prm.mapping_init_accumulate_frames, prm.current_frame_index = MAP_ARGS["init_accumulate_frames"], 5
    for b, s in enumerate(seeds):
        o = orc.fe_extract(scans[b], 1.0)
        ci, si, _ = orc.fe_get_features(o, 0.0, 1.0)
        fc = orc.voxel_grid(orc.feature_cloud(o, ci), MAP_ARGS["line_res"])[1]
        fs = orc.voxel_grid(orc.feature_cloud(o, si), MAP_ARGS["plane_res"])[1]
        mc, ms = built[s].history.map_cloud(0), built[s].history.map_cloud(1)
        ret, opc, _, orep = orc.reg_solve(orc.KdTree(mc), orc.KdTree(ms), fc, fs, prm, poses[b], poses[b])
        dt, dr = synth.pose_error(pc[b], opc)
        print(f"oracle slot {b} seed {s}: dt {dt:.3e} dr {dr:.3e} blocks {reps[b].n_blocks_last}/{orep.n_blocks_last}")
        assert res[b] == ret and dt < 1e-7 and dr < 1e-7
        assert (reps[b].icp_iterations, reps[b].lm_iterations_total, reps[b].n_blocks_last) == (orep.icp_iterations, orep.lm_iterations_total, orep.n_blocks_last)


# ---- 6. the loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_inputs(small_world):
    out = {}
    for seed in SEEDS:
        out[seed] = synth.make_livox_sequence(small_world["world"], seed, teleport=(4, 2.0) if seed == 81 else None)[0]
    return out


def run_alone(scans):
    from loam_livox_amd.mapping import Laser_mapping
    lm = Laser_mapping(scan_points=N_PTS, **MAP_ARGS)
    out = []
    for xyzi in scans:
        r = lm.process_new_scan(xyzi)
        out.append((r, lm.pose.copy(), report_tuple(lm.last_report), lm.map_sizes, bits(lm.history.map_cloud(0)).copy(), bits(lm.history.map_cloud(1)).copy(),
                    len(lm.history)))
    lm.close()
    return out


@pytest.mark.parametrize("refresh_threads", [1, None])
def test_lockstep_loop_equals_the_sequences_run_alone(gpu_lib, loop_inputs, refresh_threads):
    from loam_livox_amd.mapping import Laser_mapping_batch
    S, n_frames = len(SEEDS), 9
    lb = Laser_mapping_batch(S, refresh_threads=refresh_threads, scan_points=N_PTS, **MAP_ARGS)
    got = [[] for _ in range(S)]
    for step in range(n_frames + 2):  # ragged: sequence s starts at step s % 3, so gated, running and idle slots share steps
        frame = [step - s % 3 for s in range(S)]
        scans = [loop_inputs[SEEDS[s]][frame[s]] if 0 <= frame[s] < n_frames else None for s in range(S)]
        out = lb.process_new_scans(scans)
        for s in range(S):
            if scans[s] is None:
                assert out[s] == -1
                continue
            got[s].append((int(out[s]), lb.poses[s].copy(), report_tuple(lb.last_reports[s]), lb.map_sizes[s], bits(lb.histories[s].map_cloud(0)).copy(),
                           bits(lb.histories[s].map_cloud(1)).copy(), len(lb.histories[s])))
    assert list(lb.frame_index) == [n_frames] * S
    for s, seed in enumerate(SEEDS):
        want = run_alone(loop_inputs[seed])
        assert len(got[s]) == len(want) == n_frames
        for k in range(n_frames):
            g, w = got[s][k], want[k]
            assert g[0] == w[0], (seed, k, "result")
            assert np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64)), (seed, k, "pose", g[1] - w[1])
            assert g[2] == w[2], (seed, k, "report")
            assert g[3] == w[3] and g[6] == w[6], (seed, k, "map sizes")
            assert np.array_equal(g[4], w[4]) and np.array_equal(g[5], w[5]), (seed, k, "match buffer")
        if seed == 81:  # the teleported frame is rejected and not added
            assert [g[0] for g in got[s]] == [1, 1, 1, 1, 0, 1, 1, 1, 1]
            assert got[s][4][6] == got[s][3][6] and np.array_equal(got[s][4][5], got[s][3][5])
        else:
            assert all(g[0] == 1 for g in got[s])
    lb.close()


def test_lockstep_loop_matches_the_oracle_loop(gpu_lib, loop_inputs):
    from loam_livox_amd.mapping import Laser_mapping_batch
    seeds = [77, 81, 90]
    lb = Laser_mapping_batch(3, scan_points=N_PTS, **MAP_ARGS)
    oms = [LaserMapping(**MAP_ARGS) for _ in seeds]
    for k in range(9):
        out = lb.process_new_scans([loop_inputs[s][k] for s in seeds])
        for i, om in enumerate(oms):
            r = om.process_new_scan(loop_inputs[seeds[i]][k])
            dt, dr = synth.pose_error(lb.poses[i], om.pose)
            print(f"oracle loop seed {seeds[i]} frame {k}: result {out[i]}/{r} dt {dt:.3e} dr {dr:.3e}")
            assert out[i] == r and dt < 1e-7 and dr < 1e-7
            assert lb.map_sizes[i] == (len(om.maps[0]), len(om.maps[1]))
            assert lb.last_reports[i].n_blocks_last == om.report.n_blocks_last
    lb.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(sequences, built):
    from loam_livox_amd.mapping import Laser_mapping_batch
    seeds = SEEDS[:2]
    scans = [sequences[s][5] for s in seeds]
    poses = np.stack([built[s].pose for s in seeds])
    maps = [built[s].map for s in seeds]
    rig = Rig(scans)
    L, reg = rig.reg.L, rig.reg
    import ctypes as C
    tab = (C.c_void_p * 2)(maps[0].h, maps[1].h)
    pl = np.ascontiguousarray(poses)
    P = pl.ctypes.data_as(C.c_void_p)
    prm = C.byref(reg.params)
    for args in ((None, tab, rig.fe.h, 2, prm, None, P, P, None), (reg.h, None, rig.fe.h, 2, prm, None, P, P, None),
                 (reg.h, tab, None, 2, prm, None, P, P, None), (reg.h, tab, rig.fe.h, 2, None, None, P, P, None),
                 (reg.h, tab, rig.fe.h, 2, prm, None, None, P, None), (reg.h, tab, rig.fe.h, 2, prm, None, P, None, None),
                 (reg.h, tab, rig.fe.h, 0, prm, None, P, P, None), (reg.h, tab, rig.fe.h, 3, prm, None, P, P, None)):
        assert L.ll_reg_enqueue_fe_maps(*args) < 0
    v0, v1 = rig.vox[0].h, rig.vox[1].h
    for args in ((reg.h, None, rig.fe.h, v0, v1, 0.1, 0.15, 2, prm, None, P, P, None), (reg.h, tab, rig.fe.h, None, v1, 0.1, 0.15, 2, prm, None, P, P, None),
                 (reg.h, tab, rig.fe.h, v0, v0, 0.1, 0.15, 2, prm, None, P, P, None), (reg.h, tab, rig.fe.h, v0, v1, 0.1, 0.15, 3, prm, None, P, P, None)):
        assert L.ll_reg_enqueue_fe_downsampled_maps(*args) < 0
    reg.params.if_motion_deblur = 1
    with pytest.raises(LoamLivoxError, match="deblur"):
        rig.run_maps(maps, poses)
    with pytest.raises(LoamLivoxError, match="deblur"):
        rig.run_maps(maps, poses, downsample=False)
    reg.params.if_motion_deblur = 0
    reg.set_debug(False, force_general_solver=True)  # the solver for scans beyond the compact one has no map-per-slot form
    with pytest.raises(LoamLivoxError, match="compact solver"):
        rig.run_maps(maps, poses, downsample=False)
    reg.set_debug(False)
    with pytest.raises(ValueError):
        reg.enqueue_fe_maps(maps[:1], rig.fe, 2, poses, poses)
    # capacities: more scans than the extractor or the voxel filters hold, a registrar with fewer features than the extractor has points
    from loam_livox_amd.api import Livox_laser, Point_cloud_registration, VoxelGrid
    fe1 = Livox_laser(max_points=N_PTS, max_scans=1, piecewise_number=1)
    vox1 = (VoxelGrid(N_PTS, 1), VoxelGrid(N_PTS, 1))
    small_reg = Point_cloud_registration(max_scans=2, max_features=N_PTS // 2)
    set_params(small_reg)
    with pytest.raises(LoamLivoxError, match="extractor capacity"):
        reg.enqueue_fe_maps(maps, fe1, 2, poses, poses)
    with pytest.raises(LoamLivoxError, match="extractor capacity"):
        reg.enqueue_fe_downsampled_maps(maps, fe1, rig.vox[0], rig.vox[1], 0.1, 0.15, 2, poses, poses)
    with pytest.raises(LoamLivoxError, match="max_clouds"):
        reg.enqueue_fe_downsampled_maps(maps, rig.fe, vox1[0], vox1[1], 0.1, 0.15, 2, poses, poses)
    with pytest.raises(LoamLivoxError, match="feature capacity"):
        small_reg.enqueue_fe_maps(maps, rig.fe, 2, poses, poses)
    with pytest.raises(LoamLivoxError, match="feature capacity"):
        small_reg.enqueue_fe_downsampled_maps(maps, rig.fe, rig.vox[0], rig.vox[1], 0.1, 0.15, 2, poses, poses)
    for h in (fe1, vox1[0], vox1[1], small_reg):
        h.close()
    assert rig.run_maps(maps, poses)[0].tolist() == [1, 1]  # the handle still works after every refusal
    rig.close()
    for kw in (dict(lidar_type="velodyne"), dict(matching_mode=1), dict(loop_closure_if_enable=1), dict(keep_cell_maps=True)):
        with pytest.raises(ValueError):
            Laser_mapping_batch(2, scan_points=N_PTS, **kw)
    with pytest.raises(ValueError):
        Laser_mapping_batch(2, refresh_threads=17, scan_points=N_PTS)


# ---- the adapter's overloads ---------------------------------------------------------------------------------------------------------------
def test_adapter_demo_slots_equal_their_single_map_runs(tmp_path, sequences, built):
    import os
    import subprocess
    from loam_livox_amd import build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build.build()
    exe = str(tmp_path / "multimap_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp", "multimap_demo.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    seeds = SEEDS[:2]
    files = []
    for s in seeds:
        for kind in (0, 1):
            p = str(tmp_path / f"map_{s}_{kind}.bin")
            np.ascontiguousarray(built[s].history.map_cloud(kind)[:, :3], np.float32).tofile(p)
            files.append(p)
    for s in seeds:
        p = str(tmp_path / f"scan_{s}.bin")
        sequences[s][5].astype(np.float32).tofile(p)
        files.append(p)
    pp, out = str(tmp_path / "poses.bin"), str(tmp_path / "out.bin")
    np.stack([built[s].pose for s in seeds]).astype(np.float64).tofile(pp)
    subprocess.check_call([exe] + files + [pp, out], timeout=180)
    data = open(out, "rb").read()
    rec = [(int(np.frombuffer(data, np.int32, 1, 60 * i)[0]), data[60 * i + 4:60 * i + 60]) for i in range(8)]
    # records: maps (2 scans), maps down-sampled (2), alone scan 0 / 1, alone down-sampled scan 0 / 1
    assert rec[0] == rec[4] and rec[1] == rec[5] and rec[2] == rec[6] and rec[3] == rec[7]
    assert all(r[0] == 1 for r in rec) and rec[0][1] != rec[1][1]
    assert int(np.frombuffer(data, np.int32, 1, 480)[0]) == 1
