"""-m gpu: the full-cloud maps of the batched match buffer (ll_history_batch_enable_full_maps, api.History_buffer_batch.append_full /
cell_map(s, 2)) and the lock-step loop that keeps them and the key frames on top of them
(mapping.Laser_mapping_batch(batched_history=True, full_maps=True, key_frames=True)).

Every yardstick is the per-sequence route: a Cell_map fed append_cloud_touched( pointcloudAssociateToMap( scan[full_idx], pose ), 3 )
for the store, Laser_mapping(loop_closure_if_enable=1) run alone for the loop -- the route tests/test_cellmap.py, tests/test_keyframes.py
and tests/test_ref_cells.py hold to the oracle and to the reference's own classes.  The batched code is never compared with itself;
everything compared is integer work or fp32 work in a fixed order, so every comparison is equality of bits.

Seeds, MAP_ARGS and the 12 000-point scans are those of tests/test_gpu_multimap.py."""
import ctypes as C

import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.capi import LoamLivoxError
from tests import placement as pl
from tests.test_gpu_multimap import MAP_ARGS, N_PTS, SEEDS, bits, report_tuple

pytestmark = pytest.mark.gpu

CELL_RES, THR = 1.0, 3


@pytest.fixture(scope="module")
def seqs(small_world):
    """seed -> (scans, true poses), nine frames"""
    return {seed: synth.make_livox_sequence(small_world["world"], seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def loop_inputs(small_world):
    return {seed: synth.make_livox_sequence(small_world["world"], seed, teleport=(4, 2.0) if seed == 81 else None)[0] for seed in SEEDS}


@pytest.fixture(scope="module")
def long_inputs(small_world):
    """twenty frames for five sequences: the solo route alone closes and processes four key frames of six scans on them"""
    return {seed: synth.make_livox_sequence(small_world["world"], seed, n_frames=20)[0] for seed in SEEDS[:5]}


class FullRig:
    """S slots: a batched extractor, ONE History_buffer_batch with full maps, and per slot the yardstick -- a Cell_map of its own that
    takes the same scans through the host, as Laser_mapping._keyframe_step feeds m_pt_cell_map_full"""

    def __init__(self, S, first=N_PTS, max_pts=N_PTS, enable=True):
        from loam_livox_amd.api import Cell_map, History_buffer_batch, Livox_laser, Point_cloud_registration
        self.S = S
        self.fe = Livox_laser(max_points=N_PTS, max_scans=S, piecewise_number=1)
        self.reg = Point_cloud_registration(max_scans=1, max_features=N_PTS)
        self.hb = History_buffer_batch(S, MAP_ARGS["maximum_history_size"], max_pts, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
        if enable:
            self.hb.enable_full_maps(first, CELL_RES, THR)
        self.singles = [Cell_map(1 << 15, CELL_RES, THR) for _ in range(S)]
        self.scans = [None] * S
        self.want_touched = [np.zeros((0, 3), np.int32) for _ in range(S)]
        self.reads_after_append, self.fresh = 0, False  # reads that followed an append of at least one point: each of them materialises
        self.dropped = [np.zeros(0, np.int64) for _ in range(S)]  # per slot: the scan indices of the non-finite points the yardstick's host filter took out of the last step

    def close(self):
        for h in [self.fe, self.reg, self.hb] + self.singles:
            h.close()

    def load(self, scans):
        """scans[s]: (n, 4) or None (an empty scan)"""
        empty = np.zeros((0, 4), np.float32)
        self.scans = [empty if x is None else np.ascontiguousarray(x, np.float32) for x in scans]
        for s in range(self.S):
            self.fe.upload(self.scans[s][None], np.ones(1), first_scan=s)
        self.fe.extract_batch(self.S)
        self.fe.resolve()
        self.fe.select_batch(self.S, -1, 0.0, 1.0)

    def step(self, poses, active=None):
        """one append_full, and the same scans into the yardsticks; returns the batch's touched arrays"""
        on = np.ones(self.S, bool) if active is None else np.asarray(active, bool)
        got = self.hb.append_full(self.fe, poses, active, 3)
        self.fresh = self.fresh or any(on[s] and len(self.scans[s]) for s in range(self.S))  # (an append of no point leaves nothing to put in order)
        for s in range(self.S):
            if not on[s]:
                continue
            full_idx = self.fe.get_features(0.0, 1.0, scan=s)["full_idx"]
            full = self.scans[s][full_idx]
            ok = np.isfinite(full[:, :3]).all(axis=1)  # (Laser_mapping._keyframe_step)
            self.dropped[s] = np.asarray(full_idx, np.int64)[~ok]
            full = full[ok]
            cloud = self.reg.pointcloudAssociateToMap(full, poses[s]) if len(full) else full
            cm = self.singles[s]
            need = cm.stats()[1] + len(cloud)
            if need > cm.max_points:
                cm.reserve(max(2 * cm.max_points, need))
            self.want_touched[s] = cm.append_cloud_touched(cloud, 3)
        return got

    def compare(self, s, got_touched, tag):
        self.reads_after_append += self.fresh
        self.fresh = False
        assert got_touched.dtype == np.int32 and np.array_equal(got_touched, self.want_touched[s]), (tag, s, "touched cells")
        assert np.array_equal(self.hb.full_touched(s), self.want_touched[s]), (tag, s, "touched cells, read again")
        got, want = self.hb.cell_map(s, 2), self.singles[s]
        assert got.stats() == want.stats(), (tag, s, "cells, points, frame_idx", got.stats(), want.stats())
        g, w = got.dump(), want.dump()
        assert g[0].shape == w[0].shape and np.array_equal(bits(g[0]), bits(w[0])), (tag, s, "points")
        assert np.array_equal(g[1], w[1]), (tag, s, "cell_ijk")
        assert np.array_equal(g[2], w[2]), (tag, s, "cell_start")
        assert np.array_equal(g[3], w[3]), (tag, s, "last-update stamps")
        return want.stats()


# ---- parity per slot, the cost contract -------------------------------------------------------------------------------------------------
AWAY = np.array([0, 0, 0, 0, 0, 500.0, 0])
_work = {}


def nine_steps(seqs, S, place=None, first=N_PTS):
    """Nine steps, ragged: slot 0 spends steps 3 - 5 five hundred metres away and comes back to cells that went stale (revisit threshold
    3), slot 1 sits out steps 2 - 6 (past the threshold: its own counter does not move, nothing of it is reset), slot 2 (slot 0 when it is
    alone) passes an empty scan at step 2, slot 0's scan of step 1 holds a non-finite point where the generator left a finite one (beside
    the NaN returns synth.make_moving_scan puts into every scan, p_nan = 0.001), every third slot skips step 7"""
    rig = FullRig(S, first=first)
    seeds = SEEDS[:S]
    every = range(9) if S <= 5 else (0, 4, 8)
    empty_slot = 2 if S > 2 else 0
    came_back_smaller = nan_reached_the_filter = False
    for k in range(9):
        scans = [seqs[s][0][k] for s in seeds]
        if k == 1:
            scans[0] = scans[0].copy()
            assert np.isfinite(scans[0][N_PTS // 2, :3]).all()
            scans[0][N_PTS // 2, 1] = np.nan
        if k == 2:
            scans[empty_slot] = None
        rig.load(scans)
        poses = np.stack([seqs[s][1][k] for s in seeds])
        if k in (3, 4, 5):
            poses[0] = poses[0] + AWAY
        if place is not None:
            poses = np.stack([pl.place_pose(place, p) for p in poses])
        on = np.ones(S, bool)
        if S > 1 and 2 <= k <= 6:
            on[1] = False
        if k == 7:
            on[3::3] = False
        before = [rig.singles[s].stats() for s in range(S)]
        got = rig.step(poses, on)
        if k == 1:  # the non-finite point reached the full selection and the yardstick's filter
            nan_reached_the_filter = N_PTS // 2 in rig.dropped[0]
        if k in every:
            for s in range(S):
                after = rig.compare(s, got[s], (S, k))
                if s == empty_slot and k == 2:  # an empty selection lists nothing and still moves the counter
                    assert after[:2] == before[s][:2] and after[2] == before[s][2] + 1 and len(got[s]) == 0
                if not on[s]:
                    assert after == before[s]
        if k == 6:  # on the yardstick: coming back dropped what the stale cells held -- more than the scan brought
            came_back_smaller = rig.singles[0].stats()[1] < before[0][1]
    assert nan_reached_the_filter
    assert came_back_smaller
    if S > 1:
        assert rig.singles[1].stats()[2] == 5 and rig.singles[0].stats()[2] == 10  # per-slot counters: + 2 on the empty map, + 1 afterwards
    out = (rig.hb.full_map_work(), rig.reads_after_append, [rig.hb.cell_map(s, 2).dump() for s in range(S)], [rig.hb.full_touched(s) for s in range(S)])
    rig.close()
    return out


@pytest.mark.parametrize("S", [1, 5, 24])
def test_nine_steps_equal_a_cell_map_per_slot(gpu_lib, seqs, S):
    work, reads, _, _ = nine_steps(seqs, S)
    assert reads == {1: 8, 5: 9, 24: 3}[S]  # (alone, the slot with the empty scan appends nothing at step 2)
    _work[S] = (work, reads)


def test_cost_contract_by_the_tap(gpu_lib, seqs):
    for S in (1, 24):
        if S not in _work:  # (run alone)
            work, reads, _, _ = nine_steps(seqs, S)
            _work[S] = (work, reads)
    (w1, r1), (w24, r24) = _work[1], _work[24]
    print(f"tap: S=1 {w1.tolist()} S=24 {w24.tolist()} reads after an append {r1} {r24}")
    assert w1[0] == w24[0] > 0 and w1[1] == w24[1] > 0   # enqueues and host waits of an append do not depend on S
    assert w1[2] == 0 and w24[2] == 0                     # no stored point went through a sort or a gather inside the nine appends
    assert w1[3] == r1 == 8 and w24[3] == r24 == 3        # one materialisation per read that followed an append (of at least one point)


def test_a_store_that_grows_equals_one_that_was_large_from_the_start(gpu_lib, seqs):
    """S = 2: a first allocation of one scan per map is outgrown in step 2 (and again later); 2^18 points per map never are"""
    _, _, small, t_small = nine_steps(seqs, 2, first=N_PTS)
    _, _, large, t_large = nine_steps(seqs, 2, first=1 << 18)
    for s in range(2):
        assert len(small[s][0]) > 2 * N_PTS  # (it did outgrow two scans per map)
        for g, w in zip(small[s], large[s]):
            assert g.shape == w.shape and g.tobytes() == w.tobytes()
        assert np.array_equal(t_small[s], t_large[s])


def test_far_from_the_origin(gpu_lib, seqs):
    """every pose moved by the placement (52000, -31000, 120) m, where one fp32 ulp is 4 mm: touched lists and dumps against the yardsticks"""
    work, reads, dumps, _ = nine_steps(seqs, 2, place=pl.PLACEMENTS["far"])
    assert reads == 8  # (step 2 appends nothing: slot 0 passes an empty scan, slot 1 sits out)
    assert np.abs(dumps[0][0][:, 0] - 52000.0).max() < 1000.0 and dumps[0][1][:, 0].min() > 100000  # the stored points lie there, cell indices past 10^5


# ---- the loop -----------------------------------------------------------------------------------------------------------------------------
LOOP_CLOSURE = dict(scans_of_each_keyframe=6, scans_between_two_keyframe=3, minimum_keyframe_differen=1, avail_ratio_plane=0, avail_ratio_line=0,
                    map_alignment_maximum_icp_iteration=2, max_points=1 << 15)
FULL_KW = dict(cell_resolution=CELL_RES, threshold_cell_revisit=5000)


def same_value(a, b):
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, float) or isinstance(b, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()  # (similarities and thresholds: equal in bits)
    return a == b


def same_records(a, b):
    return len(a) == len(b) and all(sorted(x) == sorted(y) and all(same_value(x[k], y[k]) for k in x) for x, y in zip(a, b))


def assert_same_keyframes(got, want, tag):
    """two Keyframe_assembly objects: the lists, every processed key frame, the detector's log and its loops"""
    assert got.state() == want.state(), (tag, "state", got.state(), want.state())
    assert len(got.keyframe_vec) == len(want.keyframe_vec), (tag, "processed key frames")
    for i, (g, w) in enumerate(zip(got.keyframe_vec, want.keyframe_vec)):
        assert g.m_set_cell == w.m_set_cell, (tag, i, "cell set")
        assert (g.m_accumulate_frames, g.m_ending_frame_idx) == (w.m_accumulate_frames, w.m_ending_frame_idx), (tag, i)
        assert same_value(g.m_pose_q, w.m_pose_q) and same_value(g.m_pose_t, w.m_pose_t), (tag, i, "pose")
        assert sorted(g.analysis) == sorted(w.analysis) and all(same_value(g.analysis[k], w.analysis[k]) for k in g.analysis), (tag, i, "images and ratios")
        assert same_value(g.points, w.points), (tag, i, "points")
    assert same_records(got.log, want.log), (tag, "detector log")
    assert same_records(got.loops, want.loops), (tag, "loops")


def test_loop_with_key_frames_equals_the_sequences_run_alone(gpu_lib, long_inputs):
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    seeds, n_frames = SEEDS[:5], 20
    S = len(seeds)
    lb = Laser_mapping_batch(S, scan_points=N_PTS, batched_history=True, full_maps=True, key_frames=True, loop_closure=LOOP_CLOSURE, **FULL_KW, **MAP_ARGS)
    plain = Laser_mapping_batch(S, scan_points=N_PTS, batched_history=True, **MAP_ARGS)
    alone = [Laser_mapping(scan_points=N_PTS, loop_closure_if_enable=1, loop_closure=LOOP_CLOSURE, **FULL_KW, **MAP_ARGS) for _ in range(S)]
    for step in range(n_frames + 2):
        frame = [step - s % 3 for s in range(S)]  # ragged
        scans = [long_inputs[seeds[s]][frame[s]] if 0 <= frame[s] < n_frames else None for s in range(S)]
        out, out_plain = lb.process_new_scans(scans), plain.process_new_scans(scans)
        for s in range(S):
            lm = alone[s]
            if scans[s] is not None:
                r = lm.process_new_scan(scans[s])
                for other, pose, rep, tag in ((r, lm.pose, lm.last_report, "alone"), (int(out_plain[s]), plain.poses[s], plain.last_reports[s], "full_maps=False")):
                    assert int(out[s]) == int(other), (s, step, tag, "result")
                    assert np.array_equal(lb.poses[s].view(np.uint64), pose.view(np.uint64)), (s, step, tag, "pose")
                    assert report_tuple(lb.last_reports[s]) == report_tuple(rep), (s, step, tag, "report")
            assert_same_keyframes(lb.keyframes[s], lm.keyframes, (s, step))
            assert same_records(lb.loops[s], lm.loops), (s, step, "loops found")
    for s in range(S):
        lm = alone[s]
        assert len(lm.keyframes.keyframe_vec) >= 2, (s, "the solo route processed too few key frames")
        assert lb.full_map(s).stats() == lm.keyframes.m_pt_cell_map_full.stats()
        for g, w in zip(lb.full_map(s).dump(), lm.keyframes.m_pt_cell_map_full.dump()):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (s, "full map")
        lm.close()
    lb.close()
    plain.close()


def test_full_maps_only_equal_the_solo_full_map(gpu_lib, loop_inputs):
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    n_frames, S = 8, len(SEEDS)
    lb = Laser_mapping_batch(S, scan_points=N_PTS, batched_history=True, full_maps=True, loop_closure=dict(max_points=1 << 15), **FULL_KW, **MAP_ARGS)
    results = []
    for k in range(n_frames):
        results.append(lb.process_new_scans([loop_inputs[seed][k] for seed in SEEDS]).copy())
    assert lb.keyframes is None
    assert [int(r[SEEDS.index(81)]) for r in results] == [1, 1, 1, 1, 0, 1, 1, 1]  # the teleported frame is rejected: not appended
    solo_kw = dict(LOOP_CLOSURE, scans_of_each_keyframe=1000, scans_between_two_keyframe=1000)  # (no key frame closes within the run)
    for s, seed in enumerate(SEEDS):
        lm = Laser_mapping(scan_points=N_PTS, loop_closure_if_enable=1, loop_closure=solo_kw, **FULL_KW, **MAP_ARGS)
        for k in range(n_frames):
            assert lm.process_new_scan(loop_inputs[seed][k]) == int(results[k][s])
        want = lm.keyframes.m_pt_cell_map_full
        assert lb.full_map(s).stats() == want.stats(), (seed, "stats")
        for g, w in zip(lb.full_map(s).dump(), want.dump()):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (seed, "full map")
        lm.close()
    lb.close()


def test_full_maps_and_cell_maps_do_not_see_each_other(gpu_lib, loop_inputs):
    """cell_maps + cell_matching on the same handle: kinds 0 and 1, the match buffers and both existing taps with and without full maps; the
    full store with and without them"""
    from loam_livox_amd.mapping import Laser_mapping_batch
    seeds, n_frames = SEEDS[:3], 9
    cell_kw = dict(cell_maps=True, cell_matching=True, cell_map_max_points=1 << 16)

    def run(**kw):
        lb = Laser_mapping_batch(3, scan_points=N_PTS, batched_history=True, loop_closure=dict(max_points=1 << 15), **FULL_KW, **kw, **MAP_ARGS)
        steps = []
        for k in range(n_frames):
            out = lb.process_new_scans([loop_inputs[seed][k] for seed in seeds])
            steps.append((out.tobytes(), lb.poses.tobytes(), [report_tuple(r) for r in lb.last_reports],
                          [lb.histories[s].map_cloud(kind).tobytes() for s in range(3) for kind in (0, 1)],
                          (lb.history_batch.cell_map_work().tolist(), lb.history_batch.cell_match_work().tolist()) if lb.cell_maps else None))
        cells = [lb.cell_map(s, kind).dump() + (lb.cell_map(s, kind).stats(),) for s in range(3) for kind in (0, 1)] if lb.cell_maps else None
        full = [lb.full_map(s).dump() + (lb.full_map(s).stats(),) for s in range(3)] if lb.full_maps else None
        taps = (lb.history_batch.cell_map_work().tolist(), lb.history_batch.cell_match_work().tolist()) if lb.cell_maps else None
        mats = int(lb.history_batch.full_map_work()[3]) if lb.full_maps else None
        lb.close()
        return steps, cells, full, taps, mats

    def same_dumps(a, b):
        return len(a) == len(b) and all(len(x) == len(y) and all(same_value(p, q) for p, q in zip(x, y)) for x, y in zip(a, b))

    both, cells_only = run(full_maps=True, **cell_kw), run(**cell_kw)
    assert both[0] == cells_only[0]                   # results, poses, reports, match buffers and both taps after every step
    assert same_dumps(both[1], cells_only[1]) and both[3] == cells_only[3]  # kinds 0 and 1 and the taps after the reads
    assert both[4] == 1                               # reading kinds 0 and 1 did not order the full store; reading kind 2 did, once
    # in history mode (the poses do not depend on what is kept): the full store beside the feature cell maps and on its own
    beside, full_only = run(full_maps=True, cell_maps=True, cell_map_max_points=1 << 16), run(full_maps=True)
    assert beside[0] != full_only[0] and [st[:4] for st in beside[0]] == [st[:4] for st in full_only[0]]  # (only the taps' entry differs)
    assert same_dumps(beside[2], full_only[2]) and beside[4] == full_only[4] == 1
    # ... and beside cell matching against the solo route in that mode
    from loam_livox_amd.mapping import Laser_mapping
    for s, seed in enumerate(seeds):
        lm = Laser_mapping(scan_points=N_PTS, matching_mode=1, loop_closure_if_enable=1, cell_map_max_points=1 << 16,
                           loop_closure=dict(LOOP_CLOSURE, scans_of_each_keyframe=1000, scans_between_two_keyframe=1000), **FULL_KW, **MAP_ARGS)
        for k in range(n_frames):
            lm.process_new_scan(loop_inputs[seed][k])
        want = lm.keyframes.m_pt_cell_map_full
        assert both[2][s][4] == want.stats()
        assert all(same_value(g, w) for g, w in zip(both[2][s][:4], want.dump())), (seed, "full map beside the cell maps")
        lm.close()


def test_full_store_is_the_same_with_and_without_cell_maps(gpu_lib, seqs):
    """the same nine appends on a handle that also keeps (and feeds) the feature cell maps"""
    S = 3
    _, _, want, t_want = nine_steps(seqs, S)
    rig = FullRig(S)
    rig.hb.enable_cell_maps(N_PTS, CELL_RES, 5000)
    seeds = SEEDS[:S]
    for k in range(9):  # nine_steps' inputs once more, with an add of the features before every append
        scans = [seqs[s][0][k] for s in seeds]
        if k == 1:
            scans[0] = scans[0].copy()
            scans[0][N_PTS // 2, 1] = np.nan
        if k == 2:
            scans[2] = None
        rig.load(scans)
        poses = np.stack([seqs[s][1][k] for s in seeds])
        if k in (3, 4, 5):
            poses[0] = poses[0] + AWAY
        on = np.ones(S, bool)
        if 2 <= k <= 6:
            on[1] = False
        rig.hb.add_fe(rig.fe, poses, None, on)
        rig.hb.append_full(rig.fe, poses, on, 3)
        if k == 4:
            rig.hb.cell_map(0, 1).stats()  # a read of a feature kind in between
    assert rig.hb.full_map_work()[3] == 0
    for s in range(S):
        for g, w in zip(rig.hb.cell_map(s, 2).dump(), want[s]):
            assert g.shape == w.shape and g.tobytes() == w.tobytes()
        assert np.array_equal(rig.hb.full_touched(s), t_want[s])
    assert rig.hb.full_map_work()[3] == 1 and rig.hb.cell_map_work()[2] == 1
    rig.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(gpu_lib, seqs):
    from loam_livox_amd.api import History_buffer_batch, Livox_laser
    S = 2
    rig = FullRig(S, enable=False)
    seeds = SEEDS[:S]
    L, hb = rig.hb.L, rig.hb
    n64 = np.zeros(S, np.int64)
    poses = np.stack([seqs[s][1][0] for s in seeds])
    rig.load([seqs[s][0][0] for s in seeds])
    # before the enable
    for call in (lambda: hb.append_full(rig.fe, poses), lambda: hb.full_touched(0), lambda: hb.full_map_work(), lambda: hb.cell_map(0, 2).stats(),
                 lambda: hb.sync_cell_maps()):
        with pytest.raises(LoamLivoxError, match="not enabled"):
            call()
    with pytest.raises(LoamLivoxError, match="cell_resolution"):
        hb.enable_full_maps(N_PTS, 0.0, 3)
    with pytest.raises(LoamLivoxError, match="max_points_per_frame"):
        hb.enable_full_maps(N_PTS - 1, CELL_RES, 3)
    with pytest.raises(LoamLivoxError, match="2\\^31"):
        hb.enable_full_maps(1 << 30, CELL_RES, 3)  # a store that would pass 2^31 points
    with pytest.raises(LoamLivoxError, match="not enabled"):  # none of them enabled anything
        hb.full_map_work()
    hb.enable_full_maps(N_PTS, CELL_RES, THR)
    with pytest.raises(LoamLivoxError, match="already enabled"):
        hb.enable_full_maps(N_PTS, CELL_RES, THR)
    hb.sync_cell_maps()  # orders whatever is enabled: the full store alone
    with pytest.raises(LoamLivoxError, match="not enabled"):
        hb.cell_map(0, 0).stats()  # kinds 0 and 1 are still off
    # null arguments
    pp, nn = poses.ctypes.data_as(C.c_void_p), n64.ctypes.data_as(C.c_void_p)
    for args in ((None, rig.fe.h, None, pp, 3, nn), (hb.h, None, None, pp, 3, nn), (hb.h, rig.fe.h, None, None, 3, nn), (hb.h, rig.fe.h, None, pp, 3, None)):
        assert L.ll_history_batch_append_full_fe(*args) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_full_touched(hb.h, 0, None, 0, None) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_full_map_work(hb.h, None) < 0 and b"null" in L.ll_last_error()
    # min_points < 1, an extractor with fewer slots, a sequence out of range
    with pytest.raises(LoamLivoxError, match="min_points"):
        hb.append_full(rig.fe, poses, None, 0)
    small = Livox_laser(max_points=N_PTS, max_scans=1, piecewise_number=1)
    with pytest.raises(LoamLivoxError, match="fewer scans"):
        hb.append_full(small, poses)
    small.close()
    import torch
    if torch.cuda.device_count() > 1:  # (an extractor on another device needs a second one)
        other = Livox_laser(max_points=N_PTS, max_scans=S, device=1, piecewise_number=1)
        with pytest.raises(LoamLivoxError, match="another device"):
            hb.append_full(other, poses)
        other.close()
    with pytest.raises(LoamLivoxError, match="sequence"):
        hb.full_touched(S)
    # a full selection larger than the handle's max_points_per_frame
    tight = History_buffer_batch(S, MAP_ARGS["maximum_history_size"], 4000, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
    tight.enable_full_maps(4000, CELL_RES, THR)
    with pytest.raises(LoamLivoxError, match="max_points_per_frame"):
        tight.append_full(rig.fe, poses)
    assert tight.cell_map(0, 2).stats() == (0, 0, 0) and tight.full_map_work().tolist() == [0, 0, 0, 0]  # nothing was appended or enqueued
    half = [x[:4000] for x in rig.scans]
    tight.close()
    # nothing of all that reached the store; the handle works: this step and the next equal their yardsticks
    assert hb.cell_map(0, 2).stats() == (0, 0, 0) and len(hb.full_touched(0)) == 0
    got = rig.step(poses)
    for s in range(S):
        rig.compare(s, got[s], "first step")
    assert L.ll_history_batch_full_touched(hb.h, 0, np.zeros(3, np.int32).ctypes.data_as(C.c_void_p), 1, n64.ctypes.data_as(C.c_void_p)) < 0
    assert b"too small" in L.ll_last_error() and n64[0] == len(got[0]) > 1
    rig.load([x for x in half])  # 4 000-point scans
    poses = np.stack([seqs[s][1][1] for s in seeds])
    got = rig.step(poses)
    for s in range(S):
        rig.compare(s, got[s], "second step")
    rig.close()
    from loam_livox_amd.mapping import Laser_mapping_batch
    with pytest.raises(ValueError):
        Laser_mapping_batch(2, full_maps=True, scan_points=N_PTS)
    with pytest.raises(ValueError):
        Laser_mapping_batch(2, batched_history=True, key_frames=True, scan_points=N_PTS)
    with pytest.raises(ValueError):
        Laser_mapping_batch(2, batched_history=True, full_maps=True, loop_closure_if_enable=1, scan_points=N_PTS)
