"""-m gpu: the key-frame descriptor bank on the device (ll_keyframe_bank_*; api.Keyframe_bank, Keyframe_assembly( device_bank=True ),
Laser_mapping_batch( loop_closure=dict( device_bank=True ) ), the adapter's Keyframe_bank) against the pairwise route it stands in for
-- api.keyframe_similarity, which tests/test_cellmap.py and tests/test_ref_cells.py hold to the oracle and to the reference's own
class -- float for float IN ITS BITS, and against the CPU driver of the kernel's own tile body for every sum of the test tap.
tests/test_keyframe_bank_host.py is the CPU tier.  Every image is 60 x 60: the shapes are the smallest there are."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_cellmap import bits, keyframe_pair
from tests.test_keyframe_bank_host import build_driver, run_driver

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 10      # LL_KB_R: the consecutive shifts of one work item (six items, one per wavefront, cover a row of shifts)


def device_map(cloud):
    from loam_livox_amd.api import Cell_map
    m = Cell_map(max_points=max(1, len(cloud)), resolution=1.0)
    m.append_cloud(cloud)
    return m


def host_images():
    """ten (line, plane) entries from the host: random, zero, one bin, and copies of the first rolled so that the maxima sit on item,
    wavefront and wrap edges"""
    rng = np.random.default_rng(23)
    r0 = (rng.uniform(0, 1, (60, 60)).astype(np.float32) ** 8, rng.uniform(0, 1, (60, 60)).astype(np.float32) ** 4)
    r1 = (rng.uniform(0, 1, (60, 60)).astype(np.float32) ** 8, rng.normal(0, 1, (60, 60)).astype(np.float32))
    zero = (np.zeros((60, 60), np.float32), np.zeros((60, 60), np.float32))
    one = (np.zeros((60, 60), np.float32), np.zeros((60, 60), np.float32))
    one[0][59, 17], one[1][0, 0] = 0.7, 3.0
    out = [r0, r1, zero, one]
    for shift in [(0, 1), (R - 1, R), (29, 30), (30, 31), (59, 59)]:
        out.append(tuple(np.roll(x, shift, (0, 1)) for x in r0))
    out.append((r1[1].copy(), r0[0].T.copy()))
    return out


@pytest.fixture(scope="module")
def bank12(gpu_lib):
    """a bank of 12 entries -- two device key frames, ten host entries -- with every entry's images, and the pairwise route's float for
    every ordered pair and both kinds: computed once, shared, not changed"""
    from loam_livox_amd.api import Keyframe_bank, keyframe_similarity
    a, b, _ = keyframe_pair(3)
    bank = Keyframe_bank(initial_entries=16)
    imgs, analyses = [], []
    for cloud in (a, b):
        dm = device_map(cloud)
        want = dm.keyframe_images()
        got, eid = bank.add_cell_map(dm)
        dm.close()
        assert eid == len(imgs)
        analyses.append((got, want))
        imgs.append((got["images"][0].copy(), got["images"][1].copy()))
    for line, plane in host_images():
        assert bank.add_images(line, plane) == len(imgs)
        imgs.append((line, plane))
    n = len(imgs)
    assert n == 12 and len(bank) == 12
    want = np.zeros((2, n, n), np.float32)
    for i in range(n):
        for j in range(n):
            for kind in range(2):
                want[kind, i, j] = keyframe_similarity(imgs[i][kind], imgs[j][kind])
    yield dict(bank=bank, imgs=imgs, want=want, analyses=analyses)
    bank.close()


def all_pairs(n):
    ids = np.array([(i, j) for i in range(n) for j in range(n)], np.int64)
    return ids[:, 0].copy(), ids[:, 1].copy()


# ------------------------------------------------------------------------------------------------------- 1: match against the pairwise route
def test_one_pair_equals_keyframe_similarity_in_its_bits(bank12):
    bank, want = bank12["bank"], bank12["want"]
    for i, j in [(0, 1), (1, 0), (4, 9), (11, 5)]:
        line, plane = bank.match([i], [j])
        assert line.dtype == plane.dtype == np.float32 and line.shape == plane.shape == (1,)
        assert bits(line)[0] == bits(want[0, i, j]) and bits(plane)[0] == bits(want[1, i, j]), (i, j, line, plane, want[:, i, j])


def test_all_ordered_pairs_and_self_pairs_equal_keyframe_similarity_in_their_bits(bank12):
    bank, want = bank12["bank"], bank12["want"]
    ia, ib = all_pairs(12)
    assert len(ia) == 144                                   # 132 ordered pairs and the 12 self pairs
    line, plane = bank.match(ia, ib)
    bad = [(int(i), int(j), kind) for kind, got in enumerate((line, plane)) for i, j, g in zip(ia, ib, got) if bits(g) != bits(want[kind, i, j])]
    assert not bad, bad[:10]
    # the cases are what they were made to be: a zero image gives 0, a rolled copy gives 1 within float rounding
    assert want[0, 4, 2] == 0.0 and want[1, 2, 4] == 0.0 and want[1, 4, 4] == 0.0
    assert all(abs(float(want[kind, 2, k]) - 1.0) <= 2.0 ** -23 for kind in range(2) for k in range(6, 11))
    assert 0.0 < want[1, 0, 1] < 1.0 and 0.0 < want[0, 0, 1] < 1.0


# ------------------------------------------------------------------------------------------------------- 2: every sum, through the tap
def test_debug_surface_equals_the_cpu_driver_bit_for_bit(bank12, tmp_path):
    bank, imgs = bank12["bank"], bank12["imgs"]
    exe = build_driver(str(tmp_path / "keyframe_bank_host"))
    cases = [(0, 1, 0), (0, 1, 1), (2, 7, 0), (2, 7, 1)]    # two pairs, both kinds: device key frames; a random image against its (9, 10) roll
    want = run_driver(exe, str(tmp_path), [(imgs[a][kind], imgs[b][kind]) for a, b, kind in cases])
    for (a, b, kind), w in zip(cases, want):
        got = bank.surface(a, b, kind)
        assert got.shape == (60, 60) and np.array_equal(got.view(np.uint64), w["tiled"].view(np.uint64)), (a, b, kind)
        assert np.count_nonzero(got) > 0


# ------------------------------------------------------------------------------------------------------- 3: add, growth, tap, refusals
def test_add_cell_map_returns_keyframe_images_and_stores_its_first_two(bank12):
    for k, (got, want) in enumerate(bank12["analyses"]):
        assert sorted(got) == sorted(want)
        for key in want:
            if isinstance(want[key], np.ndarray):
                assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape and got[key].tobytes() == want[key].tobytes(), key
            else:
                assert np.float64(got[key]).tobytes() == np.float64(want[key]).tobytes(), key
        line, plane = bank12["bank"].images(k)
        assert line.tobytes() == want["images"][0].tobytes() and plane.tobytes() == want["images"][1].tobytes()
        assert np.count_nonzero(want["images"][0]) and np.count_nonzero(want["images"][1])
    line, plane = bank12["bank"].images(7)
    assert line.tobytes() == bank12["imgs"][7][0].tobytes() and plane.tobytes() == bank12["imgs"][7][1].tobytes()


def test_a_bank_that_grew_answers_as_one_created_large(bank12):
    from loam_livox_amd.api import Keyframe_bank
    small = Keyframe_bank(initial_entries=2)
    for k, (line, plane) in enumerate(bank12["imgs"][:9]):      # 2 -> 4 -> 8 -> 16 entries
        assert small.add_images(line, plane) == k
    ia, ib = all_pairs(9)
    line, plane = small.match(ia, ib)
    want = bank12["want"]
    assert all(bits(g) == bits(want[0, i, j]) for i, j, g in zip(ia, ib, line)) and all(bits(g) == bits(want[1, i, j]) for i, j, g in zip(ia, ib, plane))
    for k in (0, 1, 8):
        got = small.images(k)
        assert got[0].tobytes() == bank12["imgs"][k][0].tobytes() and got[1].tobytes() == bank12["imgs"][k][1].tobytes()
    small.close()


def test_work_tap_one_wait_and_no_image_byte_whatever_the_pairs(bank12):
    bank = bank12["bank"]
    bank.match([3], [4])
    one = bank.work().tolist()
    bank.match(*all_pairs(12))
    many = bank.work().tolist()
    print("ll_keyframe_bank_work", one, many)
    assert one[:3] == many[:3] and one[1] == 1 and one[2] == 0 and (one[3], many[3]) == (1, 144)
    line, plane = bank.match([], [])
    assert len(line) == len(plane) == 0 and bank.work().tolist() == [0, 0, 0, 0]


def test_refusals_leave_earlier_entries_and_their_answers_unchanged(bank12, gpu_lib):
    import ctypes as C
    from loam_livox_amd import capi
    from loam_livox_amd.api import History_buffer, Keyframe_bank
    from loam_livox_amd.capi import LoamLivoxError
    bank, want = bank12["bank"], bank12["want"]
    img = np.zeros((60, 60), np.float32)
    with pytest.raises(LoamLivoxError, match="ll_keyframe_bank_match: id out of range"):
        bank.match([0, 12], [1, 1])
    with pytest.raises(LoamLivoxError, match="ll_keyframe_bank_match: id out of range"):
        bank.match([0], [-1])
    with pytest.raises(LoamLivoxError, match="ll_keyframe_bank_debug_surface: id out of range"):
        bank.surface(0, 12, 0)
    with pytest.raises(LoamLivoxError, match="ll_keyframe_bank_debug_surface: kind"):
        bank.surface(0, 1, 2)
    with pytest.raises(LoamLivoxError, match="ll_keyframe_bank_images: id out of range"):
        bank.images(12)
    ids, sims = np.zeros(1, np.int64), np.zeros(1, np.float32)
    assert gpu_lib.ll_keyframe_bank_match(bank.h, -1, capi.ptr(ids), capi.ptr(ids), capi.ptr(sims), capi.ptr(sims)) < 0
    assert b"n_pairs out of range" in gpu_lib.ll_last_error()
    assert gpu_lib.ll_keyframe_bank_match(bank.h, 1, capi.ptr(ids), None, capi.ptr(sims), capi.ptr(sims)) < 0 and b"null" in gpu_lib.ll_last_error()
    eid = C.c_int64(-7)
    assert gpu_lib.ll_keyframe_bank_add_images(bank.h, capi.ptr(img), None, C.byref(eid)) < 0 and eid.value == -7
    dm = device_map(np.zeros((1, 4), np.float32))
    with pytest.raises(LoamLivoxError, match="roi_ratio must lie in"):
        bank.add_cell_map(dm, roi_ratio=1.5)
    assert gpu_lib.ll_keyframe_bank_add_cellmap(bank.h, dm.h, 0.9, None, None, None, None, None, None) < 0 and b"null" in gpu_lib.ll_last_error()
    dm.close()
    assert len(bank) == 12
    line, plane = bank.match(*all_pairs(12))
    assert np.array_equal(bits(line), bits(want[0].ravel())) and np.array_equal(bits(plane), bits(want[1].ravel()))
    # a history's own cell map (fed by the history) is accepted as any other: an empty map gives zero images and similarity 0
    fresh = Keyframe_bank(initial_entries=1)
    hb = History_buffer(4, 1000)
    hb.enable_cell_map(1 << 10)
    got, eid = fresh.add_cell_map(hb.cell_map(0))
    assert eid == 0 and not got["images"].any() and fresh.match([0], [0])[0][0] == 0.0
    hb.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------------- 4: the loops
def test_keyframe_assembly_with_the_bank_gives_the_same_log_and_loops(gpu_lib):
    """the out-and-back run of tests/test_gpu_scene_align.py:269, the similarities through the bank against the pairwise route"""
    from loam_livox_amd.keyframes import Keyframe_assembly
    from tests.test_gpu_fullmap_batch import same_records, same_value
    from tests.test_gpu_scene_align import out_and_back_sequence
    kw = dict(scans_of_each_keyframe=40, scans_between_two_keyframe=40, minimum_keyframe_differen=2, maximum_keyframe_in_waiting_list=3,
              map_alignment_inlier_threshold=0.35, map_alignment_maximum_icp_iteration=4, max_points=1 << 22, avail_ratio_plane=0.02,
              avail_ratio_line=0.0)
    off, on = Keyframe_assembly(**kw), Keyframe_assembly(device_bank=True, **kw)
    found = ([], [])
    for cloud, est, k in out_and_back_sequence():     # (the scans are made once and fed to both)
        for ka, loops in zip((off, on), found):
            ka.add_scan(cloud, est, k)
            loops.extend(ka.process_waiting())
    assert off.state() == on.state() and off.if_end == on.if_end
    assert len(off.log) == len(on.log) >= 1 and len(off.loops) == len(on.loops) == len(found[0]) == len(found[1]) == 1
    assert same_records(on.log, off.log) and same_records(on.loops, off.loops) and same_records(found[1], found[0])
    for g, w in zip(on.keyframe_vec, off.keyframe_vec):
        assert sorted(g.analysis) == sorted(w.analysis) and all(same_value(g.analysis[k], w.analysis[k]) for k in g.analysis)
    assert any("sim_plane" in r for r in on.log) and len(on.rounds.bank()) == len(on.keyframe_vec) == 3 and on.rounds.bank.own and off.rounds.bank.handle is None
    off.close(); on.close()


def test_batched_loop_with_one_bank_equals_the_loop_without_and_the_sequences_alone(gpu_lib, long_inputs):
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    from tests.test_gpu_fullmap_batch import FULL_KW, LOOP_CLOSURE, assert_same_keyframes, same_records
    from tests.test_gpu_multimap import MAP_ARGS, N_PTS, SEEDS
    seeds, n_frames = SEEDS[:5], 20
    S = len(seeds)
    kw = dict(scan_points=N_PTS, batched_history=True, full_maps=True, key_frames=True, **FULL_KW, **MAP_ARGS)
    on = Laser_mapping_batch(S, loop_closure=dict(LOOP_CLOSURE, device_bank=True), **kw)
    off = Laser_mapping_batch(S, loop_closure=LOOP_CLOSURE, **kw)
    alone = [Laser_mapping(scan_points=N_PTS, loop_closure_if_enable=1, loop_closure=LOOP_CLOSURE, **FULL_KW, **MAP_ARGS) for _ in range(S)]
    assert on.keyframe_bank is not None and off.keyframe_bank is None and all(ka.rounds.bank() is on.keyframe_bank for ka in on.keyframes)
    matches = 0
    for step in range(n_frames + 2):
        frame = [step - s % 3 for s in range(S)]  # ragged, as tests/test_gpu_fullmap_batch.py runs them
        scans = [long_inputs[seeds[s]][frame[s]] if 0 <= frame[s] < n_frames else None for s in range(S)]
        on.process_new_scans(scans)
        off.process_new_scans(scans)
        for s in range(S):
            if scans[s] is not None:
                alone[s].process_new_scan(scans[s])
            assert np.array_equal(on.poses[s].view(np.uint64), off.poses[s].view(np.uint64)), (s, step)
            assert_same_keyframes(on.keyframes[s], off.keyframes[s], (s, step, "bank off"))
            assert_same_keyframes(on.keyframes[s], alone[s].keyframes, (s, step, "alone"))
            assert same_records(on.loops[s], off.loops[s]) and same_records(on.loops[s], alone[s].loops), (s, step, "loops found")
    compared = sum(len([r for r in ka.log if "sim_plane" in r]) for ka in on.keyframes)
    assert compared >= S and all(len(ka.keyframe_vec) >= 2 for ka in on.keyframes)
    assert len(on.keyframe_bank) == sum(len(ka.keyframe_vec) for ka in on.keyframes)       # one bank holds every slot's key frames
    for lm in alone + [on, off]:
        lm.close()


@pytest.fixture(scope="module")
def long_inputs(small_world):
    """tests/test_gpu_fullmap_batch.py's long_inputs: twenty frames for five sequences"""
    from loam_livox_amd import synth
    from tests.test_gpu_multimap import SEEDS
    return {seed: synth.make_livox_sequence(small_world["world"], seed, n_frames=20)[0] for seed in SEEDS[:5]}


# ------------------------------------------------------------------------------------------------------- 5: the adapter
def test_adapter_keyframe_bank_reports_the_python_routes_floats(bank12, tmp_path):
    from loam_livox_amd import build
    lib = build.build()
    exe = str(tmp_path / "adapter_keyframe_bank")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "adapter_keyframe_bank.cpp"), lib,
                           "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath,/opt/rocm/lib"])
    n = 5
    src, out = str(tmp_path / "images.bin"), str(tmp_path / "out.txt")
    np.concatenate([np.stack(e).ravel() for e in bank12["imgs"][:n]]).astype(np.float32).tofile(src)
    subprocess.check_call([exe, src, str(n), out], timeout=120)
    lines = open(out).read().strip().split("\n")
    assert int(lines[0]) == n and len(lines) == n * n + 2
    line, plane = bank12["bank"].match(*all_pairs(n))
    got = np.array([[float.fromhex(v) for v in l.split()] for l in lines[1:-1]], np.float32)
    assert np.array_equal(bits(got[:, 0]), bits(line)) and np.array_equal(bits(got[:, 1]), bits(plane))
    assert [int(v) for v in lines[-1].split()] == [4, 1, 0, n * n]
