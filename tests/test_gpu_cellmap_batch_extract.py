"""-m gpu: key frames' cells out of the batched store on the device (ll_history_batch_extract_cells, api.History_buffer_batch.extract_cells,
Cell_map_slot.extract_cells_into) and the lock-step loop that takes that route (mapping.Laser_mapping_batch._full_step).

The yardstick is never the code under test: the numpy selection Keyframe_assembly._materialize_host makes on the slot's dump -- isin
over packed cells, then the points cell after cell -- and Cell_map.extract_cells on a per-sequence Cell_map fed the same clouds
(tests/test_gpu_fullmap_batch.py FullRig, tests/test_gpu_cellmap_batch.py CellRig).  Everything compared is integer work or copies: every
comparison is equality of bits -- stats, the four dump arrays, and the point keys through device_view.

Seeds, MAP_ARGS and the 12 000-point scans are those of tests/test_gpu_multimap.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.capi import LoamLivoxError, ptr
from tests import placement as pl
from tests.test_gpu_fullmap_batch import AWAY, CELL_RES, FULL_KW, LOOP_CLOSURE, THR, FullRig, assert_same_keyframes, same_records
from tests.test_gpu_multimap import MAP_ARGS, N_PTS, SEEDS, bits, report_tuple

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 1 << 20


@pytest.fixture(scope="module")
def seqs(small_world):
    """seed -> (scans, true poses), nine frames"""
    return {seed: synth.make_livox_sequence(small_world["world"], seed) for seed in SEEDS}


def pack(ijk):
    c = np.asarray(ijk, np.int64).reshape(-1, 3) + LIMIT
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def select(dump, want_ijk):
    """_materialize_host's selection on a dump (xyz, cell_ijk, cell_start, stamps): (xyz, cell_ijk, cell_start) of the selected cells"""
    xyz, ijk, start, _ = dump
    want = np.asarray(want_ijk, np.int64).reshape(-1, 3)
    want = want[(np.abs(want) < LIMIT).all(axis=1)]
    sel = np.flatnonzero(np.isin(pack(ijk), pack(want)))
    start = np.asarray(start, np.int64)
    lens = start[sel + 1] - start[sel]
    first = np.cumsum(lens) - lens
    idx = np.repeat(start[sel] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    return xyz[idx], ijk[sel], np.r_[first, lens.sum()].astype(np.int32) if len(sel) else np.zeros(1, np.int32)


def new_map(n=1024):
    from loam_livox_amd.api import Cell_map
    return Cell_map(n, CELL_RES)


def assert_is_selection(dst, slot_dump, want, counts, tag):
    """dst against the numpy selection on the slot's dump"""
    xyz, ijk, start = select(slot_dump, want)
    assert counts == (len(ijk), len(xyz)), (tag, "counts", counts, (len(ijk), len(xyz)))
    assert dst.stats() == (len(ijk), len(xyz), 2 if len(xyz) else 0), (tag, "stats", dst.stats())
    assert dst.max_points >= len(xyz), (tag, "max_points")
    g = dst.dump()
    assert g[0].shape == xyz.shape and np.array_equal(bits(g[0]), bits(xyz)), (tag, "points")
    assert np.array_equal(g[1], ijk) and np.array_equal(g[2], start) and not g[3].any(), (tag, "cells, cell_start, stamps")


def assert_same_maps(got, want, tag):
    """two Cell_map: stats, the four dump arrays, points and point keys on the device"""
    import torch
    assert got.stats() == want.stats(), (tag, "stats", got.stats(), want.stats())
    for a, b in zip(got.dump(), want.dump()):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (tag, "dump")
    (gp, gk), (wp, wk) = got.device_view(), want.device_view()
    assert gp.shape == wp.shape and torch.equal(gp.view(torch.int32), wp.view(torch.int32)) and torch.equal(gk, wk), (tag, "device points and keys")


def check_requests(hb, kind, slots, wants, singles, tag, dsts=None):
    """one batched call; every destination against both yardsticks.  Returns the destinations (the caller closes them)."""
    dsts = dsts or [new_map() for _ in slots]
    counts = hb.extract_cells(kind, slots, wants, dsts)
    for r, s in enumerate(slots):
        assert_is_selection(dsts[r], hb.cell_map(s, kind).dump(), wants[r], counts[r], (tag, r, s))
        ref = new_map()
        assert singles[s].extract_cells(wants[r], ref) == counts[r], (tag, r, s, "per-sequence counts")
        assert_same_maps(dsts[r], ref, (tag, r, s))
        ref.close()
    return dsts


def close_all(maps):
    for m in maps:
        m.close()


# ---- kind 2 ---------------------------------------------------------------------------------------------------------------------------
def ragged_steps(seqs, S, steps=range(9), place=None):
    """tests/test_gpu_fullmap_batch.py's nine ragged steps without a read in between: slot 0 goes away and comes back to stale cells,
    slot 1 sits out steps 2 - 6, slot 2 (slot 0 when alone) passes an empty scan at step 2, every third slot skips step 7.  Returns
    the rig and per slot the union of the cells its scans of steps 2 - 6 touched: the key frame."""
    rig = FullRig(S)
    seeds = SEEDS[:S]
    union = [set() for _ in range(S)]
    for k in steps:
        scans = [seqs[s][0][k] for s in seeds]
        if k == 2:
            scans[2 if S > 2 else 0] = None
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
        got = rig.step(poses, on)
        if 2 <= k <= 6:
            for s in range(S):
                if on[s]:
                    union[s] |= set(map(tuple, got[s].tolist()))
    return rig, [np.array(sorted(u), np.int32).reshape(-1, 3) for u in union]


@pytest.fixture(scope="module")
def five(gpu_lib, seqs):
    rig, wants = ragged_steps(seqs, 5)
    yield rig, wants
    rig.close()


def test_first_extraction_materialises_once_and_repeats_do_not(gpu_lib, seqs):
    rig, _ = ragged_steps(seqs, 2, steps=(0, 1))
    hb = rig.hb
    want = hb.full_touched(0)
    assert hb.full_map_work()[3] == 0 and hb.extract_work().tolist() == [0, 0, 0, 0]   # nothing has read the store since the appends
    d = new_map()
    hb.extract_cells(2, [0], [want], [d])
    w = hb.extract_work()
    assert w[3] == 1 and hb.full_map_work()[3] == 1 and w[2] == 0 and w[0] > 0 and w[1] == 2
    hb.extract_cells(2, [0], [want], [d])
    assert hb.cell_map(0, 2).extract_cells_into(want, d) == d.stats()[:2]
    assert hb.extract_work()[3] == 1 and hb.full_map_work()[3] == 1   # no append in between: the store is in order
    assert_is_selection(d, hb.cell_map(0, 2).dump(), want, d.stats()[:2], "slot 0")
    rig.load([seqs[s][0][2] for s in SEEDS[:2]])
    rig.step(np.stack([seqs[s][1][2] for s in SEEDS[:2]]), np.array([False, True]))
    hb.extract_cells(2, [0], [want], [d])                              # an append to ANOTHER slot: the store is one, it is put in order again
    assert hb.extract_work()[3] == 2 and hb.full_map_work()[3] == 2
    assert_is_selection(d, hb.cell_map(0, 2).dump(), want, d.stats()[:2], "slot 0 after an append to slot 1")
    d.close()
    rig.close()


@pytest.mark.parametrize("slots", [[0, 1, 2, 3, 4], [4], [3, 0, 2], [1], [2, 1]])
def test_key_frames_of_the_ragged_steps(five, slots):
    """all five slots, one, and [3, 0, 2]; slot 1 sat out steps 2 - 6 (its key frame is empty), slot 2 passed an empty scan"""
    rig, wants = five
    assert len(wants[1]) == 0 and all(len(wants[s]) > 100 for s in (0, 2, 3, 4))
    hb = rig.hb
    before = [hb.cell_map(s, 2).dump() + (hb.cell_map(s, 2).stats(), hb.full_touched(s)) for s in range(5)]
    dsts = check_requests(hb, 2, slots, [wants[s] for s in slots], rig.singles, slots)   # 1 024-point destinations: they grow
    assert all(d.stats()[1] > 1024 for d, s in zip(dsts, slots) if s != 1) and all(d.stats() == (0, 0, 0) for d, s in zip(dsts, slots) if s == 1)
    close_all(dsts)
    after = [hb.cell_map(s, 2).dump() + (hb.cell_map(s, 2).stats(), hb.full_touched(s)) for s in range(5)]
    for a, b in zip(before, after):    # the store, its mirrors, the touched lists and the frame counters
        assert a[4] == b[4] and all(x.tobytes() == y.tobytes() for x, y in zip(a[:4] + a[5:], b[:4] + b[5:]))
    assert hb.extract_work()[2] == 0


def test_lists_are_sets_and_other_slots_cells_are_not_found(five):
    rig, wants = five
    hb = rig.hb
    only0 = np.array(sorted(set(map(tuple, wants[0].tolist())) - set(map(tuple, hb.cell_map(3, 2).dump()[1].tolist()))), np.int32)
    assert len(only0) > 10                                     # cells slot 0 holds and slot 3 does not
    beyond = np.array([[LIMIT, 0, 0], [0, -LIMIT, 0], [wants[3][0][0] + (1 << 21), wants[3][0][1], wants[3][0][2]]], np.int32)
    rng = np.random.default_rng(3)
    dirty = np.concatenate([wants[3], wants[3][::2], only0, beyond])
    dirty = dirty[rng.permutation(len(dirty))]
    clean, mixed = new_map(), new_map()
    c = hb.extract_cells(2, [3, 0], [wants[3], only0], [clean, new_map()])
    m = hb.extract_cells(2, [0, 3], [only0, dirty], [new_map(), mixed])
    assert m[1] == c[0] and m[0] == c[1] and c[1][0] == len(only0)
    assert_same_maps(mixed, clean, "doubled, shuffled and polluted")
    close_all([clean, mixed])


def test_growth_of_one_destination_of_several_and_reuse(five):
    rig, wants = five
    hb = rig.hb
    slots = [0, 3, 4]
    dsts = [new_map(1 << 18), new_map(1024), new_map(1 << 18)]   # only the second is too small
    for d in dsts:
        d.append_cloud(np.array([[0.5, 0.5, 0.5, 0], [7.5, 0.5, 0.5, 0]], np.float32))   # (used maps: all of it must go)
    dsts = check_requests(hb, 2, slots, [wants[s] for s in slots], rig.singles, "one of three grows", dsts)
    assert dsts[1].max_points >= dsts[1].stats()[1] > 1024 and dsts[0].max_points == dsts[2].max_points == 1 << 18
    assert 1 << 15 < dsts[0].stats()[1] < 1 << 18 and 1 << 15 < dsts[2].stats()[1] < 1 << 18
    big = dsts[1].stats()
    small = wants[3][: len(wants[3]) // 8]
    check_requests(hb, 2, [3], [small], rig.singles, "a smaller selection into the same map", [dsts[1]])
    assert 0 < dsts[1].stats()[1] < big[1]
    dsts[1].append_cloud(np.array([[0.5, 0.5, 0.5, 0]], np.float32))   # the grown map takes an append as any other
    assert dsts[1].stats()[2] == 3
    close_all(dsts)


def test_refusals_change_no_destination(five, gpu_lib):
    from loam_livox_amd.api import Cell_map, History_buffer, History_buffer_batch
    rig, wants = five
    hb, L = rig.hb, rig.hb.L
    a, b = new_map(), new_map()
    cloud = np.array([[0.5, 0.5, 0.5, 0], [7.5, 0.5, 0.5, 0], [7.6, 0.5, 0.5, 0]], np.float32)
    a.append_cloud(cloud)
    b.append_cloud(cloud[:2])
    state = lambda: [m.dump() + (m.stats(),) for m in (a, b)]
    before = state()

    def same():
        return all(x[4] == y[4] and all(p.tobytes() == q.tobytes() for p, q in zip(x[:4], y[:4])) for x, y in zip(before, state()))
    w = [wants[0], wants[3]]
    coarse = Cell_map(1024, 2.0 * CELL_RES)
    hist = History_buffer(MAP_ARGS["maximum_history_size"], N_PTS, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
    hist.enable_cell_map(N_PTS, CELL_RES, 5000)
    work = hb.extract_work().copy()
    cases = [("n_requests", lambda: hb.extract_cells(2, [], [], [])),
             ("n_requests", lambda: hb.extract_cells(2, list(range(6)), [w[0]] * 6, [a, b, a, b, a, b])),
             ("sequence out of range", lambda: hb.extract_cells(2, [0, 5], w, [a, b])),
             ("sequence out of range", lambda: hb.extract_cells(2, [-1, 0], w, [a, b])),
             ("named twice", lambda: hb.extract_cells(2, [3, 3], w, [a, b])),
             ("destination is named twice", lambda: hb.extract_cells(2, [0, 3], w, [a, a])),
             ("owned by a history", lambda: hb.extract_cells(2, [0, 3], w, [a, hist.cell_map(0)])),
             ("another resolution", lambda: hb.extract_cells(2, [0, 3], w, [a, coarse])),
             ("not enabled", lambda: hb.extract_cells(0, [0, 3], w, [a, b])),
             ("kind out of range", lambda: hb.extract_cells(3, [0, 3], w, [a, b]))]
    for match, call in cases:
        with pytest.raises(LoamLivoxError, match=match):
            call()
        assert same(), match
    import torch
    if torch.cuda.device_count() > 1:   # (a destination on another device needs a second one)
        far = Cell_map(1024, CELL_RES, device=1)
        with pytest.raises(LoamLivoxError, match="another device"):
            hb.extract_cells(2, [0, 3], w, [a, far])
        far.close()
    # null arguments and descending offsets: the C ABI itself
    seq = np.array([0, 3], np.int32)
    off, bad = np.array([0, 2, 4], np.int64), np.array([0, 3, 2], np.int64)
    ijk = np.ascontiguousarray(wants[0][:4], np.int32)
    arr, n64 = (C.c_void_p * 2)(a.h, b.h), np.zeros(2, np.int64)
    none_second = (C.c_void_p * 2)(a.h, None)
    for args, match in (((None, 2, 2, ptr(seq), ptr(off), ptr(ijk), arr, ptr(n64), ptr(n64)), b"null"),
                        ((hb.h, 2, 2, None, ptr(off), ptr(ijk), arr, ptr(n64), ptr(n64)), b"null"),
                        ((hb.h, 2, 2, ptr(seq), None, ptr(ijk), arr, ptr(n64), ptr(n64)), b"null"),
                        ((hb.h, 2, 2, ptr(seq), ptr(off), None, arr, ptr(n64), ptr(n64)), b"null"),
                        ((hb.h, 2, 2, ptr(seq), ptr(off), ptr(ijk), None, ptr(n64), ptr(n64)), b"null"),
                        ((hb.h, 2, 2, ptr(seq), ptr(off), ptr(ijk), none_second, ptr(n64), ptr(n64)), b"null"),
                        ((hb.h, 2, 2, ptr(seq), ptr(off), ptr(ijk), arr, None, ptr(n64)), b"null"),
                        ((hb.h, 2, 2, ptr(seq), ptr(off), ptr(ijk), arr, ptr(n64), None), b"null"),
                        ((hb.h, 2, 2, ptr(seq), ptr(bad), ptr(ijk), arr, ptr(n64), ptr(n64)), b"descend")):
        assert L.ll_history_batch_extract_cells(*args) < 0 and match in L.ll_last_error(), match
        assert same(), match
    assert L.ll_history_batch_extract_work(hb.h, None) < 0 and b"null" in L.ll_last_error()
    assert np.array_equal(hb.extract_work(), work)                 # nothing of all that was enqueued
    plain = History_buffer_batch(2, MAP_ARGS["maximum_history_size"], N_PTS, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
    with pytest.raises(LoamLivoxError, match="not enabled"):
        plain.extract_cells(2, [0], [w[0]], [a])
    with pytest.raises(LoamLivoxError, match="enabled"):
        plain.extract_work()
    plain.close()
    assert same()
    # the handle works, and so do the destinations
    close_all(check_requests(hb, 2, [0, 3], w, rig.singles, "after the refusals", [a, b]))
    coarse.close()
    hist.close()


def test_one_call_for_24_slots_costs_what_one_request_costs(gpu_lib, seqs):
    rig, _ = ragged_steps(seqs, 24, steps=(0, 1, 2))
    hb = rig.hb
    wants = [hb.full_touched(s) for s in range(24)]   # the cells the last appended scan of every slot touched
    d = new_map()
    hb.extract_cells(2, [7], [wants[7]], [d])
    one = hb.extract_work().copy()
    d.close()
    order = [int(s) for s in np.random.default_rng(5).permutation(24)]
    dsts = check_requests(hb, 2, order, [wants[s] for s in order], rig.singles, "R = 24")
    all24 = hb.extract_work()
    print(f"tap: R=1 {one.tolist()} R=24 {all24.tolist()}")
    assert all24[0] == one[0] > 0 and all24[1] == one[1] == 2 and all24[2] == 0 and all24[3] == one[3] == 1
    assert sum(d.stats()[1] for d in dsts) > 24 * 1024
    close_all(dsts)
    rig.close()


def test_far_from_the_origin(gpu_lib, seqs):
    """the placement (52000, -31000, 120) m on one slot: cell indices past 10^5, keys copied as they are"""
    rig, _ = ragged_steps(seqs, 1, steps=(0, 1, 6), place=pl.PLACEMENTS["far"])
    want = np.concatenate([rig.hb.full_touched(0), [[0, 0, 0]]]).astype(np.int32)
    assert want[:-1, 0].min() > 100000
    dsts = check_requests(rig.hb, 2, [0], [want], rig.singles, "far")
    assert dsts[0].stats()[0] == len(want) - 1 and dsts[0].stats()[1] > 1024
    close_all(dsts)
    rig.close()


# ---- kinds 0 and 1 ----------------------------------------------------------------------------------------------------------------------
def test_feature_cell_maps_against_the_per_sequence_maps(gpu_lib, seqs):
    from tests.test_gpu_cellmap_batch import CellRig
    S = 3
    rig = CellRig(S)
    seeds = SEEDS[:S]
    for k in range(4):
        rig.load([seqs[s][0][k] for s in seeds])
        rig.step("fe", np.stack([seqs[s][1][k] for s in seeds]), None, None, 0.0, 0.0)
    hb = rig.hb
    mats = int(hb.cell_map_work()[2])
    for kind in (0, 1):
        singles = [rig.singles[s].cell_map(kind) for s in range(S)]
        cells = [singles[s].dump()[1] for s in range(S)]
        assert all(len(c) > 20 for c in cells)
        wants = [np.concatenate([cells[s][::2], cells[(s + 1) % S][1::3], [[900, 900, 900]]]).astype(np.int32) for s in range(S)]
        for slots in ([2, 0, 1], [1]):
            close_all(check_requests(hb, kind, slots, [wants[s] for s in slots], singles, ("kind", kind, slots)))
    assert hb.cell_map_work()[2] == mats + 1 and hb.extract_work()[3] == 1 and hb.extract_work()[2] == 0   # both kinds were put in order once
    with pytest.raises(LoamLivoxError, match="not enabled"):
        hb.extract_cells(2, [0], [wants[0]], [new_map()])
    rig.close()


# ---- the loop ----------------------------------------------------------------------------------------------------------------------------
def test_loop_on_the_batched_route_equals_the_host_route_and_the_sequences_alone(gpu_lib, small_world, monkeypatch):
    from loam_livox_amd import keyframes
    from loam_livox_amd.api import Full_map_slot
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    seeds, n_frames = SEEDS[:5], 20
    S = len(seeds)
    inputs = {seed: synth.make_livox_sequence(small_world["world"], seed, n_frames=n_frames)[0] for seed in seeds}
    kw = dict(scan_points=N_PTS, batched_history=True, full_maps=True, key_frames=True, loop_closure=LOOP_CLOSURE, **FULL_KW, **MAP_ARGS)
    batched, host = Laser_mapping_batch(S, **kw), Laser_mapping_batch(S, **kw)
    for ka in host.keyframes:       # materialize forced to the route through the host, and nothing extracted in advance
        ka.materialize = ka._materialize_host
    host.rounds.store = None
    alone = [Laser_mapping(scan_points=N_PTS, loop_closure_if_enable=1, loop_closure=LOOP_CLOSURE, **FULL_KW, **MAP_ARGS) for _ in range(S)]
    real_dump, real_step = Full_map_slot.dump, Laser_mapping_batch._full_step
    in_full_step = []

    def guarded_dump(self):
        if in_full_step and self.batch is batched.history_batch:
            raise AssertionError("Full_map_slot.dump during _full_step on the batched route")
        return real_dump(self)

    def traced_step(self, *a):
        in_full_step.append(1)
        try:
            return real_step(self, *a)
        finally:
            in_full_step.pop()
    monkeypatch.setattr(Full_map_slot, "dump", guarded_dump)
    monkeypatch.setattr(Laser_mapping_batch, "_full_step", traced_step)
    for step in range(n_frames + 2):
        frame = [step - s % 3 for s in range(S)]  # ragged
        scans = [inputs[seeds[s]][frame[s]] if 0 <= frame[s] < n_frames else None for s in range(S)]
        out_b, out_h = batched.process_new_scans(scans), host.process_new_scans(scans)
        assert np.array_equal(out_b, out_h) and batched.poses.tobytes() == host.poses.tobytes(), step
        for s in range(S):
            lm = alone[s]
            if scans[s] is not None:
                assert lm.process_new_scan(scans[s]) == int(out_b[s]), (s, step, "result")
                assert np.array_equal(batched.poses[s].view(np.uint64), lm.pose.view(np.uint64)), (s, step, "pose")
                assert report_tuple(batched.last_reports[s]) == report_tuple(lm.last_report), (s, step, "report")
            assert_same_keyframes(batched.keyframes[s], host.keyframes[s], (s, step, "host route"))
            assert_same_keyframes(batched.keyframes[s], lm.keyframes, (s, step, "alone"))
            assert same_records(batched.loops[s], host.loops[s]) and same_records(batched.loops[s], lm.loops), (s, step, "loops found")
    processed = sum(len(ka.keyframe_vec) for ka in batched.keyframes)
    assert processed >= 2 * S
    tap_b, tap_h = batched.history_batch.extract_work(), host.history_batch.extract_work()
    assert tap_b[0] > 0 and tap_b[1] == 2 and tap_b[2] == 0 and tap_h.tolist() == [0, 0, 0, 0]   # extractions on one route, none on the other
    for s in range(S):
        for g, w in zip(batched.full_map(s).dump(), alone[s].keyframes.m_pt_cell_map_full.dump()):
            assert g.shape == w.shape and g.tobytes() == w.tobytes(), (s, "full map")
        alone[s].close()
    batched.close()
    host.close()


# ---- the adapter -------------------------------------------------------------------------------------------------------------------------
def test_adapter_extract_cells_equals_the_python_route(tmp_path, gpu_lib, seqs):
    from loam_livox_amd import build
    from loam_livox_amd.api import History_buffer_batch, Livox_laser
    lib = build.build()
    exe = str(tmp_path / "adapter_batch_extract_cells")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "adapter_batch_extract_cells.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib),
                           "-Wl,-rpath,/opt/rocm/lib"])
    seeds = SEEDS[:2]
    poses = np.stack([seqs[s][1][5] for s in seeds]).astype(np.float64)
    fe = Livox_laser(max_points=N_PTS, max_scans=2, piecewise_number=1)
    fe.upload(np.stack([seqs[s][0][5] for s in seeds]).astype(np.float32), np.ones(2))
    fe.extract_batch(2)
    fe.resolve()
    fe.select_batch(2, -1, 0.0, 1.0)
    hb = History_buffer_batch(2, 3, N_PTS, 0.1, 0.4)
    hb.enable_cell_maps(N_PTS, 1.0, 5000)
    hb.add_fe(fe, poses)
    wants = [np.concatenate([hb.cell_map(s, 1).dump()[1][::2], [[900, 900, 900]]]).astype(np.int32) for s in range(2)]
    files = []
    for i, s in enumerate(seeds):
        files.append(str(tmp_path / f"scan_{s}.bin"))
        seqs[s][0][5].astype(np.float32).tofile(files[-1])
    poses.tofile(str(tmp_path / "poses.bin"))
    for i in range(2):
        wants[i].tofile(str(tmp_path / f"cells_{i}.bin"))
    out = str(tmp_path / "out.txt")
    subprocess.check_call([exe] + files + [str(tmp_path / "poses.bin"), str(tmp_path / "cells_0.bin"), str(tmp_path / "cells_1.bin"), out], timeout=180)
    lines = open(out).read().split()

    def fnv(arrays):
        h = 14695981039346656037
        for a in arrays:
            for byte in np.ascontiguousarray(a).tobytes():
                h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return h
    dsts = [new_map(16), new_map(16)]
    hb.extract_cells(1, [1, 0], [wants[1], wants[0]], [dsts[1], dsts[0]])
    for s in range(2):
        assert_is_selection(dsts[s], hb.cell_map(s, 1).dump(), wants[s], dsts[s].stats()[:2], ("python route", s))
        nc, npts, frame = dsts[s].stats()
        xyz, ijk, start, last = dsts[s].dump()
        xyz0 = np.zeros((npts, 4), np.float32)
        xyz0[:, :3] = xyz
        got = lines[5 * s: 5 * s + 5]
        assert [int(v) for v in got[:4]] == [nc, npts, frame, 1] and nc > 10 and npts > 16, (s, got)   # (one filtered frame: the destinations of 16 points grew)
        assert int(got[4]) == fnv([xyz0, ijk, start, last]), (s, "checksum of the dump")
    close_all(dsts)
    hb.close()
    fe.close()
