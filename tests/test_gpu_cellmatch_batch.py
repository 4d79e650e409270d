"""-m gpu: the cell-mode refresh of the batched match buffer (ll_history_batch_refresh_cells, api.History_buffer_batch.refresh_cells) and
the lock-step loop on it (mapping.Laser_mapping_batch(batched_history=True, cell_maps=True, cell_matching=True)).

Every yardstick is the per-sequence route: a History_buffer per slot with enable_cell_map, set_cell_map_async(False) and
refresh_cells, and Laser_mapping(matching_mode=1) run alone -- both held to the oracle and to the reference's own text by
tests/test_cellmap.py -- and the oracle loop.  The batched code is never compared with itself (except where a call must leave the
handle as it was); every comparison is equality of bits unless said otherwise.

Rig / CellRig, seeds, MAP_ARGS and the nine-frame 12 000-point sequences are those of tests/test_gpu_cellmap_batch.py."""
import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.capi import LoamLivoxError
from oracle.orc_mapping import LaserMapping
from tests.test_gpu_cellmap_batch import CELL_RES, CellRig
from tests.test_gpu_multimap import MAP_ARGS, N_PTS, SEEDS, bits, report_tuple

pytestmark = pytest.mark.gpu

RANGES, FOV, YAW = (6.0, 7.0), 20.0, 12.0


@pytest.fixture(scope="module")
def seqs(small_world):
    """seed -> (scans, true poses), nine frames"""
    return {seed: synth.make_livox_sequence(small_world["world"], seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def loop_inputs(small_world):
    return {seed: synth.make_livox_sequence(small_world["world"], seed, teleport=(4, 2.0) if seed == 81 else None)[0] for seed in SEEDS}


def yawed(pose, deg=YAW):
    """the pose turned by deg about the world's z axis, at the same place"""
    a = np.deg2rad(deg) / 2
    x1, y1, z1, w1 = 0.0, 0.0, np.sin(a), np.cos(a)
    x2, y2, z2, w2 = pose[:4]
    q = [w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2,
         w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2]
    return np.array(q + list(pose[4:]), np.float64)


class MatchRig(CellRig):
    """CellRig whose step is add + refresh_cells on both routes"""

    def step_cells(self, mode, poses, view, active=None, replace=1, ranges=RANGES, fov=FOV, need_partial=True):
        S = self.S
        on = np.ones(S, bool) if active is None else np.asarray(active, bool)
        gen0 = self.generations(self.bmaps)
        before = [(self.hb.size(s), bits(self.hb.map_cloud(s, 0)).copy(), bits(self.hb.map_cloud(s, 1)).copy()) for s in range(S)]
        if mode == "voxel":
            added = self.hb.add_voxel(self.vox[0], self.vox[1], poses, None, active)
        else:
            added = self.hb.add_fe(self.fe, poses, None, active)
        want = np.zeros(S, bool)
        for s in range(S):
            if on[s]:
                h = self.singles[s]
                want[s] = h.add_voxel(self.vox[0], self.vox[1], s, poses[s]) if mode == "voxel" else h.add_fe(self.fe, s, poses[s])
        assert added.tolist() == want.tolist(), "added flags"
        self.fresh_add = True
        nc, ns = self.hb.refresh_cells([self.bmaps[s] if on[s] else None for s in range(S)], view, active, ranges[0], ranges[1], fov, replace)
        gen1 = self.generations(self.bmaps)
        selected = []
        for s in range(S):
            if not on[s]:  # an inactive slot is not read and not changed
                assert gen1[s] == gen0[s], (s, "generation of an inactive slot")
                assert self.hb.size(s) == before[s][0]
                assert np.array_equal(bits(self.hb.map_cloud(s, 0)), before[s][1]) and np.array_equal(bits(self.hb.map_cloud(s, 1)), before[s][2])
                selected.append(None)
                continue
            assert gen1[s] == (gen0[s][0] + 1, gen0[s][1] + 1), (s, "one publication per kind")
            sel = []
            for kind in (0, 1):  # on the yardstick, without changing it: how many cells the query selects
                cm = self.singles[s].cell_map(kind)
                n_sel = cm.query_filter(view[s], ranges[kind], fov, self.res[kind], 0)[1]
                sel.append((n_sel, cm.stats()[0]))
                if need_partial:
                    assert 0 < n_sel < cm.stats()[0], (s, kind, "the query must select some cells and not all", sel[-1])
            selected.append(sel)
            sizes = self.singles[s].refresh_cells(self.smaps[s], view[s], ranges[0], ranges[1], fov, replace)
            assert (int(nc[s]), int(ns[s])) == sizes, (s, "match-buffer sizes", (int(nc[s]), int(ns[s])), sizes)
            self.compare_slot(s)  # both clouds, ll_map_size, ll_map_cells, 2 000 seeded k-NN queries per kind
        return added, selected


_runs = {}


def nine_steps(seqs, S, mode, replace=1, threshold=5000):
    """nine steps of add + refresh_cells; returns the tap after the last step, the yardstick's final stats and the batched handle's
    final dumps (cached)"""
    key = (S, mode, replace, threshold)
    if key in _runs:
        return _runs[key]
    rig = MatchRig(S, threshold=threshold)
    seeds = SEEDS[:S]
    fractions = []
    for k in range(9):
        rig.load([seqs[s][0][k] for s in seeds])
        if mode == "voxel":
            rig.filters()
        poses = np.stack([seqs[s][1][k] for s in seeds])
        view = np.stack([yawed(p) for p in poses])
        _, selected = rig.step_cells(mode, poses, view, None, replace)
        fractions += [n / c for sel in selected for n, c in sel]
        for s in range(S):
            rig.compare_cells(s, full=k in (2, 8))  # full dumps of both cell maps after steps 3 and 9
    work = rig.hb.cell_match_work()
    final = [[rig.singles[s].cell_map(kind).stats() for kind in (0, 1)] for s in range(S)]
    dumps = [[rig.hb.cell_map(s, kind).dump() for kind in (0, 1)] for s in range(S)]  # the batched handle's own, after the last step
    rig.close()
    print(f"S={S} {mode} replace={replace} threshold={threshold}: selected fraction {min(fractions):.2f} .. {max(fractions):.2f}, tap {work.tolist()}")
    _runs[key] = (work, final, dumps)
    return _runs[key]


# ---- 1. nine steps against separate handles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["voxel", "fe"])
@pytest.mark.parametrize("S", [1, 5, 24])
def test_nine_steps_equal_separate_handles(gpu_lib, seqs, S, mode):
    work, final, _ = nine_steps(seqs, S, mode)
    assert work[1] == 3  # host waits: the leaf counts, and the two of the second half


# ---- 2. replace off: the stores are the add-only route's -----------------------------------------------------------------------------------
def test_without_replace_the_stores_stay_the_add_only_ones(gpu_lib, seqs):
    S = 5
    _, final, dumps = nine_steps(seqs, S, "voxel", replace=0)
    rig = CellRig(S)  # adds only, no query at all: the yardstick handles of tests/test_gpu_cellmap_batch.py
    seeds = SEEDS[:S]
    for k in range(9):
        rig.load([seqs[s][0][k] for s in seeds])
        rig.filters()
        for s in range(S):
            rig.singles[s].add_voxel(rig.vox[0], rig.vox[1], s, seqs[seeds[s]][1][k])
    for s in range(S):
        for kind in (0, 1):
            cm = rig.singles[s].cell_map(kind)
            assert cm.stats() == final[s][kind]
            got, want = dumps[s][kind], cm.dump()  # the batched handle's store after nine refreshes against the add-only route's
            assert got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])), (s, kind, "points")
            for i, what in ((1, "cell_ijk"), (2, "cell_start"), (3, "last-update stamps")):
                assert np.array_equal(got[i], want[i]), (s, kind, what)
    rig.close()


# ---- 3. cells reset between refreshes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold", [3, 2])
def test_revisit_resets_between_refreshes(gpu_lib, seqs, threshold):
    S = 5
    _, plain, _ = nine_steps(seqs, S, "voxel")
    _, final, _ = nine_steps(seqs, S, "voxel", threshold=threshold)
    for s in range(S):  # on the yardstick: the surface stores ended smaller than without resets
        print(f"threshold {threshold} seed {SEEDS[s]}: surface store {final[s][1][1]} points, {plain[s][1][1]} without resets")
        assert final[s][1][1] < plain[s][1][1], (s, "resets must have happened")


# ---- 4. activity -----------------------------------------------------------------------------------------------------------------------------
def test_inactive_slots_stay_and_a_returning_slot_is_exact(gpu_lib, seqs):
    S = 3
    rig = MatchRig(S)
    seeds = SEEDS[:S]
    active = [[1, 1, 1], [1, 1, 0], [1, 1, 0], [1, 1, 0], [1, 1, 1], [0, 1, 1]]  # slot 2 sits out three steps; slot 0 is left out of the last
    kept = {}
    for k in range(6):
        on = np.array(active[k], bool)
        rig.load([None if (s == 1 and k == 2) else seqs[seeds[s]][0][k] for s in range(S)])  # slot 1 passes an empty scan at step 2
        rig.filters()
        poses = np.stack([seqs[seeds[s]][1][k] for s in range(S)])
        view = np.stack([yawed(p) for p in poses])
        rig.step_cells("voxel", poses, view, on)  # (checks generations and clouds of the inactive slots)
        for s in range(S):
            if on[s]:
                rig.compare_cells(s, full=True)
                kept[s] = [rig.hb.cell_map(s, kind).dump() for kind in (0, 1)], [rig.hb.cell_map(s, kind).stats() for kind in (0, 1)]
            else:  # the store of an inactive slot: stats and dump as they were
                for kind in (0, 1):
                    assert rig.stats(s, kind) == kept[s][1][kind] == rig.singles[s].cell_map(kind).stats()
                    for g, w in zip(rig.hb.cell_map(s, kind).dump(), kept[s][0][kind]):
                        assert g.shape == w.shape and g.tobytes() == w.tobytes()
    rig.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
def store_state(hb, S):
    return [[(hb.cell_map(s, kind).stats(),) + tuple(a.tobytes() for a in hb.cell_map(s, kind).dump()) for kind in (0, 1)] for s in range(S)]


def test_refusals_leave_the_handle_as_it_was(gpu_lib, seqs):
    from loam_livox_amd.api import History_buffer_batch
    S = 2
    seeds = SEEDS[:S]
    rig = MatchRig(S, enable=False)
    poses = np.stack([seqs[s][1][0] for s in seeds])
    view = np.stack([yawed(p) for p in poses])
    with pytest.raises(LoamLivoxError, match="not enabled"):
        rig.hb.refresh_cells(rig.bmaps, view)
    with pytest.raises(LoamLivoxError, match="not enabled"):
        rig.hb.cell_match_work()
    rig.hb.enable_cell_maps(N_PTS, CELL_RES, 5000)
    rig.load([seqs[s][0][0] for s in seeds])
    rig.filters()
    rig.step_cells("voxel", poses, view)
    state = store_state(rig.hb, S)
    clouds = [[bits(rig.hb.map_cloud(s, kind)).copy() for kind in (0, 1)] for s in range(S)]
    gens = rig.generations(rig.bmaps)
    for maps, args, what in (([rig.bmaps[0], None], (view,), "null map"), ([rig.bmaps[0], rig.bmaps[0]], (view,), "same map"),
                             (rig.bmaps, (None,), "null"), (rig.bmaps, (view, None, -1.0), "negative"), (rig.bmaps, (view, None, 5.0, -2.0), "negative")):
        with pytest.raises(LoamLivoxError, match=what):
            rig.hb.refresh_cells(maps, *args)
        assert store_state(rig.hb, S) == state and rig.generations(rig.bmaps) == gens, what
        assert [[bits(rig.hb.map_cloud(s, kind)).tolist() for kind in (0, 1)] for s in range(S)] == [[c.tolist() for c in row] for row in clouds]
    # the handle works: the next step equals its yardsticks
    rig.load([seqs[s][0][1] for s in seeds])
    rig.filters()
    poses = np.stack([seqs[s][1][1] for s in seeds])
    rig.step_cells("voxel", poses, np.stack([yawed(p) for p in poses]))
    for s in range(S):
        rig.compare_cells(s, full=True)
    # a leaf too small for the cell: cells of 150 m, leaves of 0.1 m
    wide = History_buffer_batch(1, 2, N_PTS, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
    wide.enable_cell_maps(N_PTS, 300.0, 5000)
    with pytest.raises(LoamLivoxError, match="1020 leaves"):
        wide.refresh_cells(rig.bmaps[:1], view[:1])
    wide.close()
    # a concatenation beyond the slot's match buffer: one frame thirty times, 20 m apart, into a handle that holds one frame per slot
    small = History_buffer_batch(1, 1, N_PTS, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
    small.enable_cell_maps(N_PTS, CELL_RES, 5000)
    for i in range(30):
        small.add_voxel(rig.vox[0], rig.vox[1], poses[:1] + np.array([0, 0, 0, 0, 0, 20.0 * i, 0]))
    n_stored = small.cell_map(0, 1).stats()[1]
    assert n_stored > N_PTS, "the surface store must exceed the match buffer of the slot"
    state = store_state(small, 1)
    with pytest.raises(LoamLivoxError, match=rf"slot 0 hold \d+ (corner|surface) leaves.*holds {N_PTS} points"):
        small.refresh_cells(rig.bmaps[:1], poses[:1], None, 1e4, 1e4, 360.0, 1)
    assert store_state(small, 1) == state and small.cell_map(0, 1).stats()[1] == n_stored  # refused before anything changed
    nc, ns = small.refresh_cells(rig.bmaps[:1], poses[:1], None, 10.0, 10.0, 360.0, 1)     # ... and the handle works
    assert 0 < ns[0] <= N_PTS and len(small.map_cloud(0, 1)) == ns[0]
    small.close()
    rig.close()


# ---- 6. the cost contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["voxel", "fe"])
def test_enqueues_and_waits_do_not_depend_on_the_number_of_slots(gpu_lib, seqs, mode):
    w1, w24 = nine_steps(seqs, 1, mode)[0], nine_steps(seqs, 24, mode)[0]
    print(f"tap {mode}: S=1 {w1.tolist()} S=24 {w24.tolist()}")
    assert w1[0] == w24[0] > 0 and w1[1] == w24[1] == 3
    for w in (w1, w24):
        assert 0 < w[4] <= w[3] and 0 < w[6] <= w[5] and w[7] > 0


def test_sixteen_refreshes_keep_the_log_short_and_give_the_same_bits(gpu_lib, seqs):
    S = 5
    rig = MatchRig(S)
    seeds = SEEDS[:S]
    for k in range(4):
        rig.load([seqs[s][0][k] for s in seeds])
        rig.filters()
        poses = np.stack([seqs[s][1][k] for s in seeds])
        view = np.stack([yawed(p) for p in poses])
        rig.step_cells("voxel", poses, view)  # (the last of these is the first of the refreshes below, held to its yardsticks)
    first = [[bits(rig.hb.map_cloud(s, kind)).copy() for kind in (0, 1)] for s in range(S)]
    longest = 0.0
    for i in range(16):
        nc, ns = rig.hb.refresh_cells(rig.bmaps, view, None, RANGES[0], RANGES[1], FOV, 1)
        w = rig.hb.cell_match_work()
        assert w[3] <= 4 * w[4] and w[5] <= 4 * w[6], (i, w.tolist())  # (without compaction: 17 times the live entries at the end)
        longest = max(longest, w[3] / w[4], w[5] / w[6])
        for s in range(S):
            for kind in (0, 1):
                assert np.array_equal(bits(rig.hb.map_cloud(s, kind)), first[s][kind]), (i, s, kind, "replace is idempotent")
    print(f"log / live at most {longest:.2f}, compactions {w[2]}")
    assert w[2] >= 1
    for s in range(S):  # the stores after sixteen replaces: the yardstick's after its one
        rig.compare_cells(s, full=True)
    rig.close()


# ---- 7. a registration in flight -----------------------------------------------------------------------------------------------------------
LOOP_KW = dict(maximum_in_fov_angle=50.0, threshold_cell_revisit=2000)


def test_a_registration_in_flight_keeps_its_snapshots_across_refresh_cells(gpu_lib, loop_inputs):
    from loam_livox_amd.mapping import Laser_mapping_batch
    S = 5
    seeds = [77, 78, 79, 80, 82]  # (not 81: its frame 4 is the teleported one)
    lb = Laser_mapping_batch(S, batched_history=True, cell_maps=True, cell_matching=True, cell_map_max_points=1 << 16, scan_points=N_PTS, **LOOP_KW,
                             **MAP_ARGS)
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
    lb.history_batch.refresh_cells(lb.maps, before[1], None, 100.0, 100.0, 50.0, 1)
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


# ---- 8. the loop ---------------------------------------------------------------------------------------------------------------------------
_alone = {}


def alone(loop_inputs, seed, n_frames=9):
    """Laser_mapping(matching_mode=1) alone on the sequence (cached): per frame (result, pose, report, map sizes), and the final dumps"""
    from loam_livox_amd.mapping import Laser_mapping
    if seed not in _alone:
        lm = Laser_mapping(scan_points=N_PTS, matching_mode=1, cell_map_max_points=1 << 18, **LOOP_KW, **MAP_ARGS)
        out = []
        for xyzi in loop_inputs[seed][:n_frames]:
            r = lm.process_new_scan(xyzi)
            out.append((int(r), lm.pose.copy(), report_tuple(lm.last_report), tuple(int(x) for x in lm.map_sizes)))
        dumps = [lm.history.cell_map(kind).dump() + (lm.history.cell_map(kind).stats(),) for kind in (0, 1)]
        lm.close()
        _alone[seed] = (out, dumps)
    return _alone[seed]


def run_loop(loop_inputs, seeds, n_frames, ragged):
    from loam_livox_amd.mapping import Laser_mapping_batch
    S = len(seeds)
    lb = Laser_mapping_batch(S, batched_history=True, cell_maps=True, cell_matching=True, cell_map_max_points=1 << 16, scan_points=N_PTS, **LOOP_KW,
                             **MAP_ARGS)
    got = [[] for _ in range(S)]
    for step in range(n_frames + (2 if ragged else 0)):
        frame = [step - (s % 3 if ragged else 0) for s in range(S)]  # ragged: sequences start one and two steps late
        scans = [loop_inputs[seeds[s]][frame[s]] if 0 <= frame[s] < n_frames else None for s in range(S)]
        out = lb.process_new_scans(scans)
        for s in range(S):
            if scans[s] is None:
                assert out[s] == -1
                continue
            got[s].append((int(out[s]), lb.poses[s].copy(), report_tuple(lb.last_reports[s]), tuple(int(x) for x in lb.map_sizes[s])))
    lb.sync()
    dumps = [[lb.cell_map(s, kind).dump() + (lb.cell_map(s, kind).stats(),) for kind in (0, 1)] for s in range(S)]
    lb.close()
    return got, dumps


@pytest.mark.parametrize("S", [5, 24])
def test_loop_in_cell_mode_equals_the_sequences_run_alone(gpu_lib, loop_inputs, S):
    seeds = SEEDS[:S]
    got, dumps = run_loop(loop_inputs, seeds, 9, ragged=S == 5)
    for s, seed in enumerate(seeds):
        want, wdumps = alone(loop_inputs, seed)
        assert len(got[s]) == len(want) == 9
        for k in range(9):
            g, w = got[s][k], want[k]
            assert g[0] == w[0], (seed, k, "result")
            assert np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64)), (seed, k, "pose", g[1] - w[1])
            assert g[2] == w[2], (seed, k, "report")
            assert g[3] == w[3], (seed, k, "map_sizes", g[3], w[3])
        for kind in (0, 1):
            gd, wd = dumps[s][kind], wdumps[kind]
            assert gd[4] == wd[4], (seed, kind, "stats")
            assert gd[0].shape == wd[0].shape and np.array_equal(bits(gd[0]), bits(wd[0])), (seed, kind, "points")
            for i in (1, 2, 3):
                assert np.array_equal(gd[i], wd[i]), (seed, kind, i)
    assert all(g[0] == 1 for g in got[0]) and got[0][-1][3][1] > 300


def test_loop_in_cell_mode_matches_the_oracle_loop(gpu_lib, loop_inputs):
    from loam_livox_amd.mapping import Laser_mapping_batch
    seeds = [77, 90]
    lb = Laser_mapping_batch(2, batched_history=True, cell_maps=True, cell_matching=True, cell_map_max_points=1 << 16, scan_points=N_PTS, **LOOP_KW,
                             **MAP_ARGS)
    om = LaserMapping(matching_mode=1, **LOOP_KW, **MAP_ARGS)
    for k in range(7):
        out = lb.process_new_scans([loop_inputs[s][k] for s in seeds])
        r = om.process_new_scan(loop_inputs[77][k])
        dt, dr = synth.pose_error(lb.poses[0], om.pose)
        print(f"oracle cell-mode loop seed 77 frame {k}: result {out[0]}/{r} dt {dt:.3e} dr {dr:.3e}")
        assert out[0] == r == 1 and dt < 1e-7 and dr < 1e-7
        assert tuple(int(x) for x in lb.map_sizes[0]) == (len(om.maps[0]), len(om.maps[1]))
        assert lb.last_reports[0].n_blocks_last == om.report.n_blocks_last
    lb.close()
