"""-m gpu: the batched match buffer (ll_history_batch_*, api.History_buffer_batch) and the lock-step loop on it
(mapping.Laser_mapping_batch(batched_history=True)).

The yardsticks are the per-sequence ll_history path (History_buffer + Map_buffer, one pair per sequence), Laser_mapping run alone, and
the oracle loop; the batched code is never compared with itself.  Every comparison is equality of bits unless said otherwise.

Inputs: synth.make_livox_sequence( world, seed ), seeds 77 .. 100, under MAP_ARGS of tests/test_gpu_multimap.py (history 5: the FIFO
wraps within nine frames) at 12 000 points; seed 81 with teleport = ( 4, 2.0 ) is rejected at frame 4 and only there."""
import ctypes as C

import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.capi import LoamLivoxError
from oracle.orc_mapping import LaserMapping
from tests.test_gpu_multimap import MAP_ARGS, N_PTS, SEEDS, bits, report_tuple, run_alone, set_params

pytestmark = pytest.mark.gpu

BLOCK_PATH_MAX = 24576  # the largest cloud the one-workgroup VoxelGrid takes (ll_voxel_kernels.hip)


@pytest.fixture(scope="module")
def seqs(small_world):
    """seed -> (scans, true poses), nine frames"""
    return {seed: synth.make_livox_sequence(small_world["world"], seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def loop_inputs(small_world):
    return {seed: synth.make_livox_sequence(small_world["world"], seed, teleport=(4, 2.0) if seed == 81 else None)[0] for seed in SEEDS}


_alone = {}


def alone(loop_inputs, seed, n_frames=9):
    """Laser_mapping alone on the sequence (cached: several tests compare against it)"""
    if seed not in _alone:
        _alone[seed] = run_alone(loop_inputs[seed])
    return _alone[seed][:n_frames]


class Rig:
    """S slots: a batched extractor and filter pair, ONE History_buffer_batch with S maps, and per slot the yardstick -- a
    History_buffer and a Map_buffer of its own that take the same frames"""

    def __init__(self, S, line_res=MAP_ARGS["line_res"], plane_res=MAP_ARGS["plane_res"], hist=MAP_ARGS["maximum_history_size"]):
        from loam_livox_amd.api import History_buffer, History_buffer_batch, Livox_laser, Map_buffer, Point_cloud_registration, VoxelGrid
        self.S, self.res = S, (line_res, plane_res)
        self.fe = Livox_laser(max_points=N_PTS, max_scans=S, piecewise_number=1)
        self.reg = Point_cloud_registration(max_scans=S, max_features=N_PTS)
        set_params(self.reg)
        self.vox = (VoxelGrid(N_PTS, S), VoxelGrid(N_PTS, S))
        self.hb = History_buffer_batch(S, hist, N_PTS, line_res, plane_res)
        self.bmaps = [Map_buffer() for _ in range(S)]
        self.singles = [History_buffer(hist, N_PTS, line_res, plane_res) for _ in range(S)]
        self.smaps = [Map_buffer() for _ in range(S)]
        self.rng = np.random.default_rng(2024)

    def close(self):
        for h in [self.fe, self.reg, self.vox[0], self.vox[1], self.hb] + self.bmaps + self.singles + self.smaps:
            h.close()

    def load(self, scans):
        """scans[s]: (n, 4) or None (an empty scan)"""
        S = self.S
        empty = np.zeros((1, 0, 4), np.float32)
        for s in range(S):
            self.fe.upload(empty if scans[s] is None else np.ascontiguousarray(scans[s], np.float32)[None], np.ones(1), first_scan=s)
        self.fe.extract_batch(S)
        self.fe.resolve()
        self.fe.select_batch(S, -1, 0.0, 1.0)

    def filters(self):
        """the voxel-filtered stacks as ll_reg_enqueue_fe_downsampled_maps leaves them (every slot idle: nothing is registered)"""
        S = self.S
        ident = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (S, 1))
        self.reg.enqueue_fe_downsampled_maps([None] * S, self.fe, self.vox[0], self.vox[1], self.res[0], self.res[1], S, ident, ident, np.zeros(S, np.int32))
        self.reg.collect(S)

    def generations(self, maps):
        L = self.hb.L
        return [(L.ll_map_generation(m.h, 0), L.ll_map_generation(m.h, 1)) for m in maps]

    def step(self, mode, poses, gate=None, active=None, t_step=0.0, a_step=0.0):
        """one add + refresh on both routes; returns the added flags after checking that every slot equals its yardstick"""
        S = self.S
        on = np.ones(S, bool) if active is None else np.asarray(active, bool)
        gen0 = self.generations(self.bmaps)
        before = [(self.hb.size(s), bits(self.hb.map_cloud(s, 0)).copy(), bits(self.hb.map_cloud(s, 1)).copy()) for s in range(S)]
        if mode == "voxel":
            added = self.hb.add_voxel(self.vox[0], self.vox[1], poses, gate, active, t_step, a_step)
        else:
            added = self.hb.add_fe(self.fe, poses, gate, active, t_step, a_step)
        want = np.zeros(S, bool)
        for s in range(S):
            if not on[s]:
                continue
            h = self.singles[s]
            if gate is not None:
                h.set_gate_pose(gate[s])
            want[s] = h.add_voxel(self.vox[0], self.vox[1], s, poses[s], t_step, a_step) if mode == "voxel" else h.add_fe(self.fe, s, poses[s], t_step, a_step)
        assert added.tolist() == want.tolist(), "added flags"
        nc, ns = self.hb.refresh([self.bmaps[s] if on[s] else None for s in range(S)], active)
        gen1 = self.generations(self.bmaps)
        for s in range(S):
            if not on[s]:  # an inactive slot is not read and not changed
                assert gen1[s] == gen0[s], (s, "generation of an inactive slot")
                assert self.hb.size(s) == before[s][0]
                assert np.array_equal(bits(self.hb.map_cloud(s, 0)), before[s][1]) and np.array_equal(bits(self.hb.map_cloud(s, 1)), before[s][2])
                continue
            assert gen1[s] == (gen0[s][0] + 1, gen0[s][1] + 1), (s, "one publication per kind")
            sizes = self.singles[s].refresh(self.smaps[s])
            assert (int(nc[s]), int(ns[s])) == sizes, (s, "match-buffer sizes")
            self.compare_slot(s)
        return added

    def compare_slot(self, s):
        from loam_livox_amd.api import Map_buffer
        assert self.hb.size(s) == len(self.singles[s]), (s, "len")
        for kind in (Map_buffer.CORNER, Map_buffer.SURF):
            got, want = self.hb.map_cloud(s, kind), self.singles[s].map_cloud(kind)
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (s, kind, "match-buffer cloud")
            bm, sm = self.bmaps[s], self.smaps[s]
            assert bm.size(kind) == sm.size(kind) == len(want), (s, kind, "Map_buffer.size")
            assert bm.cells(kind) == sm.cells(kind), (s, kind, "cells")
            if len(want) == 0:
                continue
            # 2 000 seeded queries around the cloud's own points: most have five neighbours inside the radius, some have fewer
            q = want[self.rng.integers(0, len(want), 2000), :3] + self.rng.normal(0.0, 0.4, (2000, 3)).astype(np.float32)
            q = np.ascontiguousarray(q, np.float32)
            gi, gd = bm.nearestKSearch(kind, q, 1.0)
            wi, wd = sm.nearestKSearch(kind, q, 1.0)
            assert np.array_equal(gi, wi), (s, kind, "k-NN indices")
            assert np.array_equal(bits(gd), bits(wd)), (s, kind, "k-NN squared distances")


# ---- 1. nine steps against separate handles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["voxel", "fe"])
@pytest.mark.parametrize("S", [1, 5, 24])
def test_nine_steps_equal_separate_handles(gpu_lib, seqs, S, mode):
    rig = Rig(S)
    seeds = SEEDS[:S]
    sizes = []
    for k in range(9):
        rig.load([seqs[s][0][k] for s in seeds])
        if mode == "voxel":
            rig.filters()
        added = rig.step(mode, np.stack([seqs[s][1][k] for s in seeds]))
        assert added.all()  # both steps are 0: every frame is pushed
        sizes.append(rig.hb.size(0))
    assert sizes == [1, 2, 3, 4, 5, 5, 5, 5, 5]  # the FIFO wraps
    rig.close()


# ---- 2. the add rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gate", [False, True])
def test_add_rule_pushes_and_rejects_like_the_single_handle(gpu_lib, seqs, with_gate):
    """a frame of these sequences moves by 4.3 cm: with a translation step of 6 cm a frame right after a push is not pushed, the one
    after it is -- once the history is full (the first five frames are pushed whatever the distance)"""
    S = 5
    rig = Rig(S)
    seeds = SEEDS[:S]
    flags = []
    for k in range(9):
        rig.load([seqs[s][0][k] for s in seeds])
        rig.filters()
        poses = np.stack([seqs[s][1][k] for s in seeds])
        gate = np.stack([seqs[s][1][max(k - 1, 0)] for s in seeds]) if with_gate else None  # the pose before the registration
        flags.append(rig.step("voxel", poses, gate, None, 0.06, 10.0).tolist())
    late = np.array(flags[5:])
    assert late.any() and not late.all(), "both outcomes of the add rule must occur"
    assert np.array(flags[:5]).all()
    rig.close()


# ---- 3. ragged activity -------------------------------------------------------------------------------------------------------------------
def test_ragged_activity_leaves_inactive_slots_alone(gpu_lib, seqs):
    S = 7
    rig = Rig(S)
    seeds = SEEDS[:S]
    for step in range(11):
        frame = [step - s % 3 for s in range(S)]  # the schedule of the loop test
        on = np.array([0 <= f < 9 for f in frame])
        rig.load([seqs[seeds[s]][0][frame[s]] if on[s] else None for s in range(S)])
        rig.filters()
        poses = np.stack([seqs[seeds[s]][1][min(max(frame[s], 0), 8)] for s in range(S)])
        added = rig.step("voxel", poses, None, on)  # (checks the generations and the untouched clouds of the inactive slots)
        assert added.tolist() == on.tolist()
    assert [rig.hb.size(s) for s in range(S)] == [5] * S
    rig.close()


# ---- 4. both sides of the block-path boundary, and an empty cloud -------------------------------------------------------------------------
def test_concatenations_on_both_sides_of_the_block_path_boundary(gpu_lib, seqs):
    """un-filtered frames (some 3 000 surface points each) at a 5 cm leaf and a history of 10: slot s joins at step 2 s, so in the last
    call the concatenations hold 10, 8, 6, 4 and 2 frames; slot 5 is active throughout with an empty scan"""
    from loam_livox_amd.api import VoxelGrid
    S, res, hist = 6, 0.05, 10
    rig = Rig(S, line_res=res, plane_res=res, hist=hist)
    seeds = SEEDS[:S]
    vg = VoxelGrid(N_PTS, 1)
    vg.setLeafSize(res, res, res)
    frame_sizes = [[] for _ in range(S)]  # per slot: the surface points of the frames its history holds
    for k in range(hist):
        on = np.array([k >= 2 * s for s in range(5)] + [True])
        scans = [seqs[seeds[s]][0][k % 9] if on[s] and s < 5 else None for s in range(S)]
        rig.load(scans)
        poses = np.stack([seqs[seeds[s]][1][k % 9] for s in range(S)])
        for s in range(5):
            if on[s]:  # the frame as the add filters it, by the library's stand-alone pieces
                pc = rig.fe.get_features(scan=s)["pc_surface"]
                vg.setInputCloud(rig.reg.pointcloudAssociateToMap(pc, poses[s]))
                frame_sizes[s].append(len(vg.filter()))
        added = rig.step("fe", poses, None, on)
        assert added.tolist() == on.tolist()
    totals = [sum(f) for f in frame_sizes[:5]]
    print("surface concatenations of the last call:", totals)
    assert min(totals) < BLOCK_PATH_MAX < max(totals), totals
    assert sum(t > BLOCK_PATH_MAX for t in totals) >= 1 and sum(t <= BLOCK_PATH_MAX for t in totals) >= 2
    # the empty slot: ten (empty) frames, an empty match buffer, an empty grid -- as the single handle (checked in every step)
    assert rig.hb.size(5) == hist and len(rig.hb.map_cloud(5, 1)) == 0 and rig.bmaps[5].size(1) == 0
    vg.close()
    rig.close()


# ---- 5. pinning ---------------------------------------------------------------------------------------------------------------------------
def test_a_registration_in_flight_keeps_its_snapshots_across_a_batched_refresh(gpu_lib, loop_inputs):
    from loam_livox_amd.mapping import Laser_mapping_batch
    S = 5
    seeds = [77, 78, 79, 80, 82]  # (not 81: its frame 4 is the teleported one)
    lb = Laser_mapping_batch(S, batched_history=True, scan_points=N_PTS, **MAP_ARGS)
    for k in range(5):
        assert lb.process_new_scans([loop_inputs[s][k] for s in seeds]).tolist() == [1] * S
    scans = [loop_inputs[s][5] for s in seeds]
    lb._upload(scans, np.ones(S), [True] * S)
    lb.fe.extract_batch(S)
    lb.fe.resolve()
    lb.fe.select_batch(S, -1, 0.0, 1.0)
    fi = np.full(S, 5, np.int32)
    lb._enqueue(lb.maps, fi)
    before = lb.reg.collect(S)
    gen0 = [lb.history_batch.L.ll_map_generation(m.h, 1) for m in lb.maps]
    lb._enqueue(lb.maps, fi)
    lb.history_batch.add_fe(lb.fe, before[1], lb.poses)  # (waits for the extractor only: the registration is still running)
    lb.history_batch.refresh(lb.maps)
    during = lb.reg.collect(S)
    assert [lb.history_batch.L.ll_map_generation(m.h, 1) for m in lb.maps] == [g + 1 for g in gen0]
    lb._enqueue(lb.maps, fi)
    after = lb.reg.collect(S)
    for b in range(S):
        assert before[0][b] == during[0][b] == 1
        assert np.array_equal(before[1][b].view(np.uint64), during[1][b].view(np.uint64)), (b, "pose across the refresh")
        assert report_tuple(before[3][b]) == report_tuple(during[3][b]), (b, "report across the refresh")
    assert any(report_tuple(after[3][b]) != report_tuple(before[3][b]) for b in range(S))  # the next enqueue sees the new maps
    lb.close()


# ---- 6. the loop against the sequences run alone ------------------------------------------------------------------------------------------
def run_loop(loop_inputs, seeds, n_frames, ragged, **kw):
    from loam_livox_amd.mapping import Laser_mapping_batch
    S = len(seeds)
    lb = Laser_mapping_batch(S, scan_points=N_PTS, **kw, **MAP_ARGS)
    got = [[] for _ in range(S)]
    for step in range(n_frames + (2 if ragged else 0)):
        frame = [step - (s % 3 if ragged else 0) for s in range(S)]
        scans = [loop_inputs[seeds[s]][frame[s]] if 0 <= frame[s] < n_frames else None for s in range(S)]
        out = lb.process_new_scans(scans)
        for s in range(S):
            if scans[s] is None:
                assert out[s] == -1
                continue
            got[s].append((int(out[s]), lb.poses[s].copy(), report_tuple(lb.last_reports[s]), lb.map_sizes[s], bits(lb.histories[s].map_cloud(0)).copy(),
                           bits(lb.histories[s].map_cloud(1)).copy(), len(lb.histories[s])))
    assert list(lb.frame_index) == [n_frames] * S
    lb.close()
    return got


def assert_same_run(g, w, tag):
    assert g[0] == w[0], (tag, "result")
    assert np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64)), (tag, "pose", g[1] - w[1])
    assert g[2] == w[2], (tag, "report")
    assert g[3] == w[3] and g[6] == w[6], (tag, "map sizes")
    assert np.array_equal(g[4], w[4]) and np.array_equal(g[5], w[5]), (tag, "match buffer")


def test_batched_loop_equals_the_sequences_run_alone_and_the_default_loop(gpu_lib, loop_inputs):
    n_frames = 9
    got = run_loop(loop_inputs, SEEDS, n_frames, True, batched_history=True)
    default = run_loop(loop_inputs, SEEDS, n_frames, True)
    for s, seed in enumerate(SEEDS):
        want = alone(loop_inputs, seed)
        assert len(got[s]) == len(default[s]) == len(want) == n_frames
        for k in range(n_frames):
            assert_same_run(got[s][k], want[k], (seed, k, "alone"))
            assert_same_run(got[s][k], default[s][k], (seed, k, "default histories"))
        if seed == 81:  # the teleported frame is rejected and not added
            assert [g[0] for g in got[s]] == [1, 1, 1, 1, 0, 1, 1, 1, 1]
            assert got[s][4][6] == got[s][3][6] and np.array_equal(got[s][4][5], got[s][3][5])
        else:
            assert all(g[0] == 1 for g in got[s])


def test_batched_loop_of_64_sequences(gpu_lib, loop_inputs):
    """five frames; slot s runs the sequence of seed 77 + s % 24"""
    seeds = [SEEDS[s % len(SEEDS)] for s in range(64)]
    got = run_loop(loop_inputs, seeds, 5, False, batched_history=True)
    for s, seed in enumerate(seeds):
        want = alone(loop_inputs, seed, 5)
        for k in range(5):
            assert_same_run(got[s][k], want[k], (s, seed, k))


# ---- 7. the loop against the oracle loop --------------------------------------------------------------------------------------------------
def test_batched_loop_matches_the_oracle_loop(gpu_lib, loop_inputs):
    from loam_livox_amd.mapping import Laser_mapping_batch
    seeds = [77, 81, 90]
    lb = Laser_mapping_batch(3, batched_history=True, scan_points=N_PTS, **MAP_ARGS)
    oms = [LaserMapping(**MAP_ARGS) for _ in seeds]
    worst = (0.0, 0.0)
    for k in range(9):
        out = lb.process_new_scans([loop_inputs[s][k] for s in seeds])
        for i, om in enumerate(oms):
            r = om.process_new_scan(loop_inputs[seeds[i]][k])
            dt, dr = synth.pose_error(lb.poses[i], om.pose)
            worst = (max(worst[0], dt), max(worst[1], dr))
            print(f"oracle loop seed {seeds[i]} frame {k}: result {out[i]}/{r} dt {dt:.3e} dr {dr:.3e}")
            assert out[i] == r and dt < 1e-7 and dr < 1e-7
            assert lb.map_sizes[i] == (len(om.maps[0]), len(om.maps[1]))
            assert lb.last_reports[i].n_blocks_last == om.report.n_blocks_last
    print(f"largest difference to the oracle loop: {worst[0]:.3e} m {worst[1]:.3e} rad")
    lb.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(gpu_lib, seqs):
    from loam_livox_amd.api import History_buffer_batch, Livox_laser, VoxelGrid
    S = 2
    rig = Rig(S)
    seeds = SEEDS[:S]
    L, hb = rig.hb.L, rig.hb
    rig.load([seqs[s][0][0] for s in seeds])
    rig.filters()
    poses = np.ascontiguousarray(np.stack([seqs[s][1][0] for s in seeds]))
    P = poses.ctypes.data_as(C.c_void_p)
    v0, v1 = rig.vox[0].h, rig.vox[1].h
    tab = (C.c_void_p * S)(*[m.h for m in rig.bmaps])
    # null handles or poses
    for args in ((None, v0, v1, None, P, None, 0.0, 0.0, None), (hb.h, None, v1, None, P, None, 0.0, 0.0, None),
                 (hb.h, v0, None, None, P, None, 0.0, 0.0, None), (hb.h, v0, v1, None, None, None, 0.0, 0.0, None)):
        assert L.ll_history_batch_add_voxel(*args) < 0 and b"null" in L.ll_last_error()
    for args in ((None, rig.fe.h, None, P, None, 0.0, 0.0, None), (hb.h, None, None, P, None, 0.0, 0.0, None), (hb.h, rig.fe.h, None, None, None, 0.0, 0.0, None)):
        assert L.ll_history_batch_add_fe(*args) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_refresh(None, tab, None, None, None) < 0 and L.ll_history_batch_refresh(hb.h, None, None, None, None) < 0
    # a null map in an active slot, the same map twice
    with pytest.raises(LoamLivoxError, match="null map"):
        hb.refresh([rig.bmaps[0], None])
    with pytest.raises(LoamLivoxError, match="two active slots"):
        hb.refresh([rig.bmaps[0], rig.bmaps[0]])
    hb.refresh([rig.bmaps[0], rig.bmaps[0]], [True, False])  # (fine: the second slot is inactive)
    # n_sequences < 1, and a capacity the 32-bit sorts cannot index
    h = C.c_void_p()
    assert L.ll_history_batch_create(0, 0, 5, N_PTS, 0.1, 0.15, C.byref(h)) < 0 and b"n_sequences" in L.ll_last_error()
    assert L.ll_history_batch_create(0, 1024, 1024, 2048, 0.1, 0.15, C.byref(h)) < 0 and b"2^31" in L.ll_last_error()
    assert L.ll_history_batch_create(0, 2, 5, N_PTS, 0.1, 0.15, None) < 0
    # filters / an extractor with fewer slots than n_sequences
    fe1 = Livox_laser(max_points=N_PTS, max_scans=1, piecewise_number=1)
    vox1 = (VoxelGrid(N_PTS, 1), VoxelGrid(N_PTS, 1))
    with pytest.raises(LoamLivoxError, match="fewer scans"):
        hb.add_fe(fe1, poses)
    with pytest.raises(LoamLivoxError, match="fewer clouds"):
        hb.add_voxel(vox1[0], vox1[1], poses)
    # a frame larger than max_points_per_frame
    tiny = History_buffer_batch(S, 5, 16, 0.1, 0.15)
    with pytest.raises(LoamLivoxError, match="max_points_per_frame"):
        tiny.add_voxel(rig.vox[0], rig.vox[1], poses)
    with pytest.raises(LoamLivoxError, match="max_points_per_frame"):
        tiny.add_fe(rig.fe, poses)
    assert tiny.size(0) == 0 and tiny.size(1) == 0
    tiny.add_fe(rig.fe, poses, active=[False, False])  # (inactive slots are not read: nothing to refuse)
    # handles on different devices (where the box has a second one)
    import torch
    if torch.cuda.device_count() > 1:
        other = History_buffer_batch(S, 5, N_PTS, 0.1, 0.15, device=1)
        with pytest.raises(LoamLivoxError, match="device"):
            other.add_voxel(rig.vox[0], rig.vox[1], poses)
        with pytest.raises(LoamLivoxError, match="device"):
            other.add_fe(rig.fe, poses)
        with pytest.raises(LoamLivoxError, match="device"):
            other.refresh(rig.bmaps)
        other.close()
    for x in (fe1, vox1[0], vox1[1], tiny):
        x.close()
    # nothing was added by any refused call, and the handle works
    assert hb.size(0) == 0 and hb.size(1) == 0
    assert rig.step("voxel", poses).all()
    assert L.ll_history_batch_size(hb.h, 2) == -1 and L.ll_history_batch_size(hb.h, -1) == -1
    with pytest.raises(LoamLivoxError):
        hb.map_cloud(2, 0)
    rig.close()
    from loam_livox_amd.mapping import Laser_mapping_batch
    for kw in (dict(lidar_type="velodyne"), dict(matching_mode=1), dict(loop_closure_if_enable=1), dict(keep_cell_maps=True)):
        with pytest.raises(ValueError):
            Laser_mapping_batch(2, batched_history=True, scan_points=N_PTS, **kw)


# ---- 9. the adapter -----------------------------------------------------------------------------------------------------------------------
def test_adapter_demo_slots_equal_the_python_route(tmp_path, gpu_lib, seqs):
    import os
    import subprocess
    from loam_livox_amd import build
    from loam_livox_amd.api import History_buffer_batch, Livox_laser, Map_buffer, Point_cloud_registration, VoxelGrid
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = build.build()
    exe = str(tmp_path / "history_batch_demo")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(root, "include"), "-o", exe,
                           os.path.join(root, "tests", "cpp", "history_batch_demo.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    seeds = SEEDS[:2]
    files = []
    for s in seeds:
        p = str(tmp_path / f"scan_{s}.bin")
        seqs[s][0][5].astype(np.float32).tofile(p)
        files.append(p)
    poses = np.stack([seqs[s][1][5] for s in seeds] + [seqs[s][1][6] for s in seeds]).astype(np.float64)
    pp, out = str(tmp_path / "poses.bin"), str(tmp_path / "out.bin")
    poses.tofile(pp)
    subprocess.check_call([exe] + files + [pp, out], timeout=180)
    data = open(out, "rb").read()

    # the same two steps through api.py
    fe = Livox_laser(max_points=N_PTS, max_scans=2, piecewise_number=1)
    fe.upload(np.stack([seqs[s][0][5] for s in seeds]).astype(np.float32), np.ones(2))
    fe.extract_batch(2)
    fe.resolve()
    fe.select_batch(2, -1, 0.0, 1.0)
    hb = History_buffer_batch(2, 3, N_PTS, 0.1, 0.4)
    maps = [Map_buffer(), Map_buffer()]
    reg = Point_cloud_registration(max_scans=2, max_features=N_PTS)
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.current_frame_index, p.mapping_init_accumulate_frames = 2, 5, 100, 50
    p.maximum_allow_residual_block, p.subsample_seed = N_PTS, 0
    vox = (VoxelGrid(N_PTS, 2), VoxelGrid(N_PTS, 2))
    want = b""

    def state(added):
        nonlocal want
        for s in range(2):
            want += np.array([int(added[s]), hb.size(s)], np.int32).tobytes() + np.array([hb.L.ll_map_generation(maps[s].h, 0)], np.int64).tobytes()
            for k in (0, 1):
                want += np.array([maps[s].size(k), maps[s].cells(k)], np.int64).tobytes()
            for k in (0, 1):
                c = hb.map_cloud(s, k)
                want += np.array([len(c)], np.int64).tobytes() + c.tobytes()

    added = hb.add_fe(fe, poses[:2])
    hb.refresh(maps)
    state(added)
    reg.enqueue_fe_downsampled_maps(maps, fe, vox[0], vox[1], 0.1, 0.4, 2, poses[:2], poses[:2])
    reg.collect(2)
    added = hb.add_voxel(vox[0], vox[1], poses[2:], poses[:2], [True, False])
    hb.refresh(maps, [True, False])
    state(added)
    assert added.tolist() == [True, False] and hb.size(0) == 2 and hb.size(1) == 1
    assert len(data) == len(want) and data == want
    for h in [fe, hb, reg, vox[0], vox[1]] + maps:
        h.close()
