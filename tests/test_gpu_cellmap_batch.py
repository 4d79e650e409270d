"""-m gpu: the cell maps of the batched match buffer (ll_history_batch_enable_cell_maps, api.History_buffer_batch.cell_map) and the
lock-step loop that keeps them (mapping.Laser_mapping_batch(batched_history=True, cell_maps=True)).

Every yardstick is the per-sequence route: a History_buffer per slot with enable_cell_map and set_cell_map_async(False), which
tests/test_cellmap.py and tests/test_ref_cells.py hold to the oracle and to the reference's own class.  The batched code is never
compared with itself; every comparison is equality of bits.

Rig, seeds, MAP_ARGS and the 12 000-point scans are those of tests/test_gpu_history_batch.py."""
import ctypes as C

import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.capi import LoamLivoxError
from tests.test_gpu_history_batch import Rig
from tests.test_gpu_multimap import MAP_ARGS, N_PTS, SEEDS, bits, report_tuple

pytestmark = pytest.mark.gpu

CELL_RES = 1.0


@pytest.fixture(scope="module")
def seqs(small_world):
    """seed -> (scans, true poses), nine frames"""
    return {seed: synth.make_livox_sequence(small_world["world"], seed) for seed in SEEDS}


@pytest.fixture(scope="module")
def loop_inputs(small_world):
    return {seed: synth.make_livox_sequence(small_world["world"], seed, teleport=(4, 2.0) if seed == 81 else None)[0] for seed in SEEDS}


class CellRig(Rig):
    """Rig with cell maps on both routes.  The batched store starts at max_points_per_frame points per map, so it outgrows its first
    allocation on the way; the yardsticks double theirs as they always do."""

    def __init__(self, S, threshold=5000, enable=True):
        super().__init__(S)
        self.threshold = threshold
        if enable:
            self.hb.enable_cell_maps(N_PTS, CELL_RES, threshold)
        for h in self.singles:
            h.enable_cell_map(N_PTS, CELL_RES, threshold)
            h.set_cell_map_async(False)
        self.reads_after_add = 0   # reads that followed an add: each of them materialises
        self.fresh_add = False

    def step(self, *a, **kw):
        out = super().step(*a, **kw)
        self.fresh_add = True
        return out

    def _reading(self):
        self.reads_after_add += self.fresh_add
        self.fresh_add = False

    def stats(self, s, kind):
        self._reading()
        return self.hb.cell_map(s, kind).stats()

    def compare_cells(self, s, full):
        """slot s of the batch against its own History_buffer; returns the yardstick's stats of both kinds"""
        import torch
        out = []
        for kind in (0, 1):
            self._reading()
            got, want = self.hb.cell_map(s, kind), self.singles[s].cell_map(kind)
            assert got.stats() == want.stats(), (s, kind, "cells, points, frame_idx", got.stats(), want.stats())
            out.append(want.stats())
            if not full:
                continue
            g, w = got.dump(), want.dump()
            assert g[0].shape == w[0].shape and np.array_equal(bits(g[0]), bits(w[0])), (s, kind, "points")
            assert np.array_equal(g[1], w[1]), (s, kind, "cell_ijk")
            assert np.array_equal(g[2], w[2]), (s, kind, "cell_start")
            assert np.array_equal(g[3], w[3]), (s, kind, "last-update stamps")
            (gp, gk), (wp, wk) = got.device_view(), want.device_view()
            assert gp.shape == wp.shape == (want.stats()[1], 4) and torch.equal(gp.view(torch.int32), wp.view(torch.int32)), (s, kind, "device points")
            assert torch.equal(gk, wk), (s, kind, "per-point keys")
        return out


# ---- 1. nine steps against separate handles, 3. the cost contract ---------------------------------------------------------------------
_work = {}


def nine_steps(seqs, S, mode, t_step=0.0):
    rig = CellRig(S)
    seeds = SEEDS[:S]
    grown = []
    for k in range(9):
        rig.load([seqs[s][0][k] for s in seeds])
        if mode == "voxel":
            rig.filters()
        added = rig.step(mode, np.stack([seqs[s][1][k] for s in seeds]), None, None, t_step, t_step)
        stats = [rig.compare_cells(s, full=k in (2, 8)) for s in range(S)]  # full dumps after steps 3 and 9: adds land behind a store and behind a log
        grown.append((added.copy(), [st[1][1] for st in stats]))
        assert all(st[1][2] == k + 2 for st in stats)  # the surface maps' frame_idx: + 2 on the empty map, + 1 afterwards
    work = rig.hb.cell_map_work()
    reads = rig.reads_after_add
    rig.close()
    return grown, work, reads


@pytest.mark.parametrize("mode", ["voxel", "fe"])
@pytest.mark.parametrize("S", [1, 5, 24])
def test_nine_steps_equal_separate_handles(gpu_lib, seqs, S, mode):
    grown, work, reads = nine_steps(seqs, S, mode)
    assert all(a.all() for a, _ in grown)  # history 5, both steps 0: every frame is pushed
    assert reads == 9
    _work[(S, mode)] = (work, reads)


def test_frames_that_are_not_pushed_still_reach_the_cell_maps(gpu_lib, seqs):
    """add steps of 1e9: once the history is full (five frames) no frame is pushed any more"""
    grown, _, _ = nine_steps(seqs, 5, "voxel", t_step=1e9)
    for k in range(9):
        added, n_surf = grown[k]
        assert added.tolist() == [k < 5] * 5
        if k >= 5:  # (asserted on the yardstick's figures) not pushed, yet the surface map grew
            assert all(n_surf[s] > grown[k - 1][1][s] for s in range(5))


@pytest.mark.parametrize("mode", ["voxel", "fe"])
def test_cost_contract_by_the_tap(gpu_lib, seqs, mode):
    for S in (1, 24):
        if (S, mode) not in _work:  # (run alone)
            _, work, reads = nine_steps(seqs, S, mode)
            _work[(S, mode)] = (work, reads)
    (w1, r1), (w24, r24) = _work[(1, mode)], _work[(24, mode)]
    print(f"tap {mode}: S=1 {w1.tolist()} S=24 {w24.tolist()} reads after an add {r1} {r24}")
    assert w24[0] > 0 and w24[1] <= w24[0] and w1[1] <= w1[0]   # adds sort at most the new points, never the store
    assert w1[3] == w24[3] > 0                                    # the launches of an add do not depend on S
    assert w1[2] == r1 == 9 and w24[2] == r24 == 9                # one materialisation per read that followed an add, not per read


# ---- 2. the revisit rule, per-slot counters, ragged activity ---------------------------------------------------------------------------
def test_revisit_rule_counters_and_ragged_activity(gpu_lib, seqs):
    from loam_livox_amd.api import History_buffer
    S, thr = 3, 3
    rig = CellRig(S, threshold=thr)
    seeds = SEEDS[:S]
    away = np.array([0, 0, 0, 0, 0, 500.0, 0])
    active = [[1, 1, 1], [1, 1, 0], [1, 1, 0], [1, 1, 0], [1, 1, 1]]
    kept = {}
    for k in range(5):
        on = np.array(active[k], bool)
        rig.load([None if (s == 1 and k == 2) else seqs[seeds[s]][0][k] for s in range(S)])  # slot 1 passes an empty scan at step 2
        rig.filters()
        poses = np.stack([seqs[seeds[s]][1][k] for s in range(S)])
        if k in (1, 2, 3):
            poses[0] = poses[0] + away  # slot 0 spends three steps 500 m away, then comes back
        before = [[rig.singles[s].cell_map(kind).stats() for kind in (0, 1)] for s in range(S)]
        probes = None
        if k == 4:  # what this step appends to slots 0 and 2: the same frames into maps that hold nothing else
            probes = {}
            for s in (0, 2):
                p = History_buffer(MAP_ARGS["maximum_history_size"], N_PTS, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
                p.enable_cell_map(N_PTS, CELL_RES, thr)
                p.add_voxel(rig.vox[0], rig.vox[1], s, poses[s])
                probes[s] = [p.cell_map(kind).stats()[1] for kind in (0, 1)]
                p.close()
        rig.step("voxel", poses, None, on)
        for s in range(S):
            if on[s]:
                after = rig.compare_cells(s, full=True)
                kept[s] = [rig.hb.cell_map(s, kind).dump() for kind in (0, 1)], [rig.hb.cell_map(s, kind).stats() for kind in (0, 1)]
                if s == 1 and k == 2:  # an empty cloud still moves the counter
                    assert [a[:2] for a in after] == [b[:2] for b in before[s]] and [a[2] for a in after] == [b[2] + 1 for b in before[s]]
            else:  # an inactive slot: stats and dump as they were
                for kind in (0, 1):
                    assert rig.stats(s, kind) == kept[s][1][kind] == rig.singles[s].cell_map(kind).stats()
                    for g, w in zip(rig.hb.cell_map(s, kind).dump(), kept[s][0][kind]):
                        assert g.shape == w.shape and g.tobytes() == w.tobytes()
        if k == 4:  # on the yardsticks: slot 0 lost stored points to a reset, slot 2 (counter at 2, stamps at 0) did not
            for kind in (0, 1):
                n0 = rig.singles[0].cell_map(kind).stats()[1] - before[0][kind][1]
                n2 = rig.singles[2].cell_map(kind).stats()[1] - before[2][kind][1]
                print(f"step 4 kind {kind}: slot 0 grew {n0} of {probes[0][kind]} appended, slot 2 grew {n2} of {probes[2][kind]}")
                assert probes[0][kind] > 0 and n0 < probes[0][kind], (kind, "a reset must have happened in slot 0")
                assert n2 == probes[2][kind] > 0, (kind, "no reset may have happened in slot 2")
    assert [rig.singles[s].cell_map(1).stats()[2] for s in range(S)] == [6, 6, 3]  # per-slot counters
    rig.close()


# ---- 4. the loop ------------------------------------------------------------------------------------------------------------------------
CELL_KW = dict(cell_map_max_points=1 << 16, cell_resolution=CELL_RES, threshold_cell_revisit=5000)


def run_loop(loop_inputs, seeds, n_frames, **kw):
    from loam_livox_amd.mapping import Laser_mapping_batch
    S = len(seeds)
    lb = Laser_mapping_batch(S, scan_points=N_PTS, batched_history=True, **kw, **MAP_ARGS)
    got = [[] for _ in range(S)]
    for step in range(n_frames + 2):
        frame = [step - s % 3 for s in range(S)]  # ragged lengths
        scans = [loop_inputs[seeds[s]][frame[s]] if 0 <= frame[s] < n_frames else None for s in range(S)]
        out = lb.process_new_scans(scans)
        for s in range(S):
            if scans[s] is not None:
                got[s].append((int(out[s]), lb.poses[s].copy(), report_tuple(lb.last_reports[s])))
    dumps = None
    if kw.get("cell_maps"):
        lb.sync()
        dumps = [[lb.cell_map(s, kind).dump() + (lb.cell_map(s, kind).stats(),) for kind in (0, 1)] for s in range(S)]
    lb.close()
    return got, dumps


def test_loop_with_cell_maps_equals_the_sequences_run_alone(gpu_lib, loop_inputs):
    from loam_livox_amd.mapping import Laser_mapping
    n_frames = 9
    got, dumps = run_loop(loop_inputs, SEEDS, n_frames, cell_maps=True, **CELL_KW)
    plain, _ = run_loop(loop_inputs, SEEDS, n_frames)
    for s, seed in enumerate(SEEDS):
        lm = Laser_mapping(scan_points=N_PTS, keep_cell_maps=True, **CELL_KW, **MAP_ARGS)
        want = []
        for xyzi in loop_inputs[seed][:n_frames]:
            r = lm.process_new_scan(xyzi)
            want.append((int(r), lm.pose.copy(), report_tuple(lm.last_report)))
        lm.sync()
        assert len(got[s]) == len(plain[s]) == len(want) == n_frames
        for k in range(n_frames):
            for other, tag in ((want[k], "alone"), (plain[s][k], "cell_maps=False")):
                assert got[s][k][0] == other[0], (seed, k, tag, "result")
                assert np.array_equal(got[s][k][1].view(np.uint64), other[1].view(np.uint64)), (seed, k, tag, "pose")
                assert got[s][k][2] == other[2], (seed, k, tag, "report")
        assert [g[0] for g in got[s]] == ([1, 1, 1, 1, 0, 1, 1, 1, 1] if seed == 81 else [1] * 9)  # the teleported frame is rejected
        for kind in (0, 1):
            cm = lm.history.cell_map(kind)
            w, g = cm.dump(), dumps[s][kind]
            assert g[4] == cm.stats(), (seed, kind, "stats")
            assert g[0].shape == w[0].shape and np.array_equal(bits(g[0]), bits(w[0])), (seed, kind, "points")
            for i in (1, 2, 3):
                assert np.array_equal(g[i], w[i]), (seed, kind, i)
        lm.close()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(gpu_lib, seqs):
    S = 2
    rig = CellRig(S, enable=False)
    seeds = SEEDS[:S]
    L, hb = rig.hb.L, rig.hb
    n64, i32 = C.c_int64(0), C.c_int32(0)
    p, q = C.c_void_p(), C.c_void_p()
    buf = np.zeros((4, 4), np.float32)
    ibuf = np.zeros(64, np.int32)
    work = np.zeros(4, np.int64)
    # a read before the enable
    with pytest.raises(LoamLivoxError, match="not enabled"):
        hb.cell_map(0, 0).stats()
    with pytest.raises(LoamLivoxError, match="not enabled"):
        hb.cell_map(0, 0).dump()
    with pytest.raises(LoamLivoxError, match="not enabled"):
        hb.cell_map(0, 0).device_view()
    with pytest.raises(LoamLivoxError, match="not enabled"):
        hb.sync_cell_maps()
    with pytest.raises(LoamLivoxError, match="not enabled"):
        hb.cell_map_work()
    # null handle
    assert L.ll_history_batch_enable_cell_maps(None, N_PTS, 1.0, 3) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_sync_cell_maps(None) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_stats(None, 0, 0, C.byref(n64), C.byref(n64), C.byref(i32)) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_dump(None, 0, 0, None, 0, None, None, None, 0) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_device_view(None, 0, 0, C.byref(p), C.byref(q), C.byref(n64), None) < 0 and b"null" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_work(None, work.ctypes.data_as(C.c_void_p)) < 0 and b"null" in L.ll_last_error()
    # cell_resolution <= 0, a first allocation below one frame, a store beyond 2^31 points per kind
    with pytest.raises(LoamLivoxError, match="cell_resolution"):
        hb.enable_cell_maps(N_PTS, 0.0, 3)
    with pytest.raises(LoamLivoxError, match="max_points_per_frame"):
        hb.enable_cell_maps(N_PTS - 1, CELL_RES, 3)
    with pytest.raises(LoamLivoxError, match="2\\^31"):
        hb.enable_cell_maps(1 << 30, CELL_RES, 3)
    with pytest.raises(LoamLivoxError, match="not enabled"):  # none of them enabled anything
        hb.cell_map(0, 0).stats()
    hb.enable_cell_maps(N_PTS, CELL_RES, 5000)
    with pytest.raises(LoamLivoxError, match="already enabled"):
        hb.enable_cell_maps(N_PTS, CELL_RES, 5000)
    # one step, then sequence / kind out of range and buffers too small
    rig.load([seqs[s][0][0] for s in seeds])
    rig.filters()
    poses = np.stack([seqs[s][1][0] for s in seeds])
    assert rig.step("voxel", poses).all()
    for seq, kind, what in ((2, 0, "sequence"), (-1, 0, "sequence"), (0, 2, "kind"), (0, -1, "kind")):
        with pytest.raises(LoamLivoxError, match=what):
            hb.cell_map(seq, kind).stats()
        assert L.ll_history_batch_cell_map_dump(hb.h, seq, kind, None, 0, None, None, None, 0) < 0 and what.encode() in L.ll_last_error()
        assert L.ll_history_batch_cell_map_device_view(hb.h, seq, kind, C.byref(p), C.byref(q), C.byref(n64), None) < 0 and what.encode() in L.ll_last_error()
    assert L.ll_history_batch_cell_map_device_view(hb.h, 0, 0, None, C.byref(q), C.byref(n64), None) < 0 and b"null" in L.ll_last_error()
    nc, npts, _ = hb.cell_map(0, 1).stats()
    assert npts > 4 and nc > 0
    assert L.ll_history_batch_cell_map_dump(hb.h, 0, 1, buf.ctypes.data_as(C.c_void_p), 4, None, None, None, 0) < 0 and b"too small" in L.ll_last_error()
    assert L.ll_history_batch_cell_map_dump(hb.h, 0, 1, None, 0, None, ibuf.ctypes.data_as(C.c_void_p), None, 0) < 0 and b"too small" in L.ll_last_error()
    assert not buf.any() and not ibuf.any()
    # the handle works: this step and the next equal their yardsticks
    for s in range(S):
        rig.compare_cells(s, full=True)
    rig.load([seqs[s][0][1] for s in seeds])
    rig.filters()
    assert rig.step("voxel", np.stack([seqs[s][1][1] for s in seeds])).all()
    for s in range(S):
        rig.compare_cells(s, full=True)
    rig.close()
    from loam_livox_amd.mapping import Laser_mapping_batch
    with pytest.raises(ValueError):
        Laser_mapping_batch(2, cell_maps=True, scan_points=N_PTS)
    with pytest.raises(ValueError):
        Laser_mapping_batch(2, batched_history=True, cell_maps=True, keep_cell_maps=True, scan_points=N_PTS)
