"""CPU tier of the full-cloud maps of the batched match buffer (tests/test_gpu_fullmap_batch.py is the GPU tier): the entry points
are declared, exported and bound and refuse null arguments without a device; the launch chains of an append -- the gather, cb_append
on a third store, the touched chain -- compiled for the CPU from the kernel units themselves (tests/fullmap_batch_host.cpp on
tests/cellmap_batch_shim) give, after every step, the touched cells of append_cloud( pts, &cell_vec ) and the store of the oracle's
cell map; and Laser_mapping_batch(full_maps=True, key_frames=True) makes one append_full per step for exactly the accepted slots and
feeds every accepted slot's key frames with its own frame index (against stubbed device handles)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi, keyframes, mapping
from oracle.orc_cellmap import CellMap
from tests.test_multimap_host import _Stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ll_history_batch_enable_full_maps", "ll_history_batch_append_full_fe", "ll_history_batch_full_touched", "ll_history_batch_full_map_work")


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name in NEW:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl, name
        assert name in capi.SYMBOLS
        fn = getattr(L, name)
        assert fn.restype is C.c_int32
        assert len(decl.group(1).split(",")) == len(fn.argtypes), name
    from loam_livox_amd.api import Full_map_slot, History_buffer_batch
    for m in ("enable_full_maps", "append_full", "full_touched", "full_map", "full_map_work", "cell_map"):
        assert callable(getattr(History_buffer_batch, m))
    for m in ("append_cloud_touched", "stats", "dump", "close"):  # what a Keyframe_assembly asks of its full map
        assert callable(getattr(Full_map_slot, m))
    assert callable(mapping.Laser_mapping_batch.full_map)


def test_null_arguments_are_refused_without_a_device():
    L = capi.load()
    n = C.c_int64(0)
    out = (C.c_int64 * 4)()
    assert L.ll_history_batch_enable_full_maps(None, 1000, 1.0, 3) < 0 and b"ll_history_batch_enable_full_maps: null" in L.ll_last_error()
    assert L.ll_history_batch_append_full_fe(None, None, None, None, 3, None) < 0 and b"ll_history_batch_append_full_fe: null" in L.ll_last_error()
    assert L.ll_history_batch_full_touched(None, 0, None, 0, C.byref(n)) < 0 and b"ll_history_batch_full_touched: null" in L.ll_last_error()
    assert L.ll_history_batch_full_map_work(None, out) < 0 and b"ll_history_batch_full_map_work: null" in L.ll_last_error()


# ---- the chains on the host ---------------------------------------------------------------------------------------------------------------
THR, RES, MIN_POINTS, N_STEPS = 3, 1.0, 3, 12
BOX = float(CellMap(RES).box)  # the edge of a cell (set_resolution halves the resolution it is given)


def in_cell(k, n, rng):
    """n points inside cell k, well away from its faces"""
    c = CellMap(RES).centre(np.asarray(k))
    return (c + rng.uniform(-0.2, 0.2, (n, 3)).astype(np.float32) * np.float32(BOX)).astype(np.float32)


CELL_2, CELL_3, CELL_4 = (40, 1, 1), (41, 1, 1), (42, 1, 1)  # the cells cloud Q gives exactly 2, 3 and 4 points


def clouds():
    rng = np.random.default_rng(23)
    D = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)             # dense: 4^3 cells with a handful of points each
    Fc = (D + np.array([0, 50, 0], np.float32)).astype(np.float32)      # the same, elsewhere
    P = np.concatenate([in_cell((4 * i, -7, 3), 1, rng) for i in range(40)])  # forty one-point cells
    Q = np.concatenate([in_cell(CELL_2, 2, rng), in_cell(CELL_3, 3, rng), in_cell(CELL_4, 4, rng), in_cell((60, 0, 0), 1, rng),
                        np.array([[np.nan, 0, 0], [0, 3e6, 0]], np.float32),  # not finite; beyond 2^20 cells
                        in_cell((61, 0, 0), 1, rng)]).astype(np.float32)
    Q = Q[rng.permutation(len(Q))]                                        # (in no cell order)
    return dict(D=D, F=Fc, P=P, Q=Q, E=np.zeros((0, 3), np.float32))


# per map a cloud per step; "-": the map sits the step out, "E": an empty cloud
SCHEDULE = ["DFFFDQEDPFQD",   # step 4: the cells of D were last stamped three appends ago, are reset and receive D again
            "P---QQEDDP-F",   # a first cloud of one-point cells; three steps out; Q twice
            "EQDD-FQQED-F"]   # an empty cloud first: Q then meets a map without cells


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fullmap_batch") / "fullmap_batch_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "tests", "cellmap_batch_shim"),
                           "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "fullmap_batch_host.cpp")])
    return exe


def run_host(exe, tmp, reads):
    cl = clouds()
    buf = np.array([3, N_STEPS, THR, MIN_POINTS], np.int32).tobytes() + np.float32(RES).tobytes()
    for t in range(N_STEPS):
        buf += np.int32(reads[t]).tobytes()
        for m in range(3):
            c = SCHEDULE[m][t]
            buf += np.int32(-1).tobytes() if c == "-" else np.int32(len(cl[c])).tobytes() + cl[c].tobytes()
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(pin, "wb").write(buf)
    subprocess.check_call([exe, pin, pout])
    raw = np.fromfile(pout, np.int32)
    pos, touched, dumps = 0, {}, {}
    for t in range(N_STEPS):
        for m in range(3):
            n = int(raw[pos])
            touched[(t, m)] = raw[pos + 1:pos + 1 + 3 * n].reshape(n, 3)
            pos += 1 + 3 * n
        if not reads[t]:
            continue
        for m in range(3):
            frame, nc, npts = raw[pos:pos + 3]
            pos += 3
            ijk = raw[pos:pos + 3 * nc].reshape(nc, 3)
            pos += 3 * nc
            start = raw[pos:pos + nc + 1]
            pos += nc + 1
            last = raw[pos:pos + nc]
            pos += nc
            pts = raw[pos:pos + 3 * npts].reshape(npts, 3)  # (bits)
            pos += 3 * npts
            dumps[(t, m)] = (int(frame), ijk, start, last, pts)
    assert pos + 1 == len(raw) and raw[pos] == sum(bool(r) for r in reads)  # one materialisation per read step
    return touched, dumps


def rule(cmap, cloud):
    """append_cloud( pts, &cell_vec ) restated (cell_map_keyframe.hpp:596-607, 619-666) on the map as it is BEFORE the append: the cells
    that receive at least MIN_POINTS of the cloud's storable points, every cell that receives one when the map has no cells"""
    k, ok = cmap.cell_index(cloud) if len(cloud) else (np.zeros((0, 3), np.int64), np.zeros(0, bool))
    cells, counts = np.unique(k[ok], axis=0, return_counts=True) if ok.any() else (np.zeros((0, 3), np.int64), np.zeros(0, np.int64))
    need = 1 if len(cmap.cells) == 0 else MIN_POINTS
    return cells[counts >= need].astype(np.int32).reshape(-1, 3)  # (np.unique sorts the rows: ascending (i, j, k), the cell-key order)


def oracle_run():
    """per (step, map): the touched list the map holds, its state, and what the schedule is there for"""
    from oracle import ref_cells
    cl = clouds()
    maps = [CellMap(RES, THR) for _ in range(3)]
    refs = [ref_cells.RefCellMap(RES, THR) for _ in range(3)] if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libll_ref_cells.so")) else None
    touched, states, facts = {}, {}, {}
    held = [np.zeros((0, 3), np.int32) for _ in range(3)]
    for t in range(N_STEPS):
        for m in range(3):
            c = SCHEDULE[m][t]
            if c != "-":
                cm = maps[m]
                want = rule(cm, cl[c])
                k, ok = cm.cell_index(cl[c]) if len(cl[c]) else (np.zeros((0, 3), np.int64), np.zeros(0, bool))
                stale_hit = {key for key in map(tuple, k[ok].tolist()) if key in cm.cells and cm.frame - cm.cells[key]["last"] >= THR}
                facts[(t, m)] = dict(was_empty=len(cm.cells) == 0, reset_and_listed=len(stale_hit & set(map(tuple, want.tolist()))), dropped=int((~ok).sum()))
                own = cm.append(cl[c])  # the oracle's own cell_vec: the same rule, stated once more
                assert [tuple(x) for x in want.tolist()] == own, (t, m)
                if refs is not None:  # the reference's own append_cloud( pts, &cell_vec ), on what the store keeps of the cloud
                    got = refs[m].append(cl[c][ok], True)
                    assert np.array_equal(np.unique(got.reshape(-1, 3), axis=0), want.astype(np.int64)), (t, m, "reference cell_vec")
                held[m] = want
            touched[(t, m)] = held[m]
            keys = sorted(maps[m].cells)
            pts = [maps[m].cell_points(key) for key in keys]
            start = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int32)
            states[(t, m)] = (maps[m].frame, np.array(keys, np.int32).reshape(-1, 3), start, np.array([maps[m].cells[key]["last"] for key in keys], np.int32),
                              (np.concatenate(pts) if pts else np.zeros((0, 3), np.float32)).astype(np.float32).view(np.int32))
    return touched, states, facts


def assert_same(got, want, tag):
    assert got[0] == want[0], (tag, "frame counter", got[0], want[0])
    assert np.array_equal(got[1], want[1]), (tag, "cell indices")
    assert np.array_equal(got[2], want[2]), (tag, "cell_start")
    assert np.array_equal(got[3], want[3]), (tag, "last-update stamps")
    assert got[4].shape == want[4].shape and np.array_equal(got[4], want[4]), (tag, "points in order")


def test_schedule_holds_the_cases():
    """what the inputs are there for, on the oracle alone"""
    touched, states, facts = oracle_run()
    rows = lambda a: set(map(tuple, a.tolist()))
    assert facts[(4, 0)]["reset_and_listed"] > 0 and not facts[(4, 0)]["was_empty"]  # stale, reset by the append, >= 3 points of that append
    assert states[(4, 0)][4].shape[0] < states[(3, 0)][4].shape[0] + 300             # ... and the reset dropped what those cells held
    assert facts[(0, 1)]["was_empty"] and len(touched[(0, 1)]) == 40 and states[(0, 1)][2].tolist() == list(range(41))  # forty one-point cells, all listed
    assert all(np.array_equal(touched[(t, 1)], touched[(0, 1)]) for t in (1, 2, 3))  # a map that sits out keeps its list
    assert rows(touched[(4, 1)]) == {CELL_3, CELL_4}                                 # 2 points: not listed; 3 and 4: listed
    assert facts[(4, 1)]["dropped"] == 2                                             # the NaN point and the one beyond 2^20 cells
    assert facts[(1, 2)]["was_empty"] and rows(touched[(1, 2)]) == {CELL_2, CELL_3, CELL_4, (60, 0, 0), (61, 0, 0)}  # after an empty cloud: still no cells
    assert len(touched[(6, 0)]) == 0 and states[(6, 0)][0] == states[(5, 0)][0] + 1  # an empty cloud lists nothing and moves the counter


@pytest.mark.parametrize("reads", ["every step", "once at the end"])
def test_chains_on_the_host_equal_the_rule_and_the_oracle(host_exe, tmp_path, reads):
    touched, states, _ = oracle_run()
    flags = [1] * N_STEPS if reads == "every step" else [0] * (N_STEPS - 1) + [1]
    got_touched, got_dumps = run_host(host_exe, str(tmp_path), flags)
    for t in range(N_STEPS):
        for m in range(3):
            assert np.array_equal(got_touched[(t, m)], touched[(t, m)]), (t, m, "touched cells", reads)
    assert sorted({t for t, _ in got_dumps}) == [t for t in range(N_STEPS) if flags[t]]
    for key, g in got_dumps.items():
        assert_same(g, states[key], key + (reads,))


# ---- the loop's bookkeeping, device handles stubbed ---------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    st = _Stubs()
    outer = st

    class Slot:
        def __init__(self, s):
            self.s = s

    class HistBatch:
        def __init__(self, n_sequences, *a, **kw):
            self.S = n_sequences
            self.frames = [0] * n_sequences

        def enable_full_maps(self, initial_points_per_map, cell_resolution, threshold_cell_revisit):
            outer.log.append(("enable_full_maps", initial_points_per_map, cell_resolution, threshold_cell_revisit))

        def enable_cell_maps(self, *a):
            outer.log.append(("enable_cell_maps",) + a)

        def full_map(self, s):
            return Slot(s)

        def add_voxel(self, vc, vs, poses, gate=None, active=None, t=0.0, a=0.0):
            on = [bool(x) for x in active]
            outer.log.append(("add_voxel", tuple(on)))
            for s in range(self.S):
                self.frames[s] += on[s]
            return np.array(on)

        def append_full(self, fe, poses, active=None, min_points=3, lists=True):
            outer.log.append(("append_full", tuple(bool(x) for x in active), np.array(poses, np.float64).copy(), min_points))
            return [np.zeros((0, 3), np.int32)] * self.S if lists else np.zeros(self.S, np.int64)

        def refresh(self, maps, active=None):
            outer.log.append(("refresh",))
            return np.array(self.frames), np.array(self.frames)

        def size(self, s):
            return min(self.frames[s], 5)

        def close(self):
            pass

    class Assembly:
        def __init__(self, **kw):
            self.kw = kw
            self.slot = kw["full_cell_map"].s
            outer.log.append(("assembly", self.slot, {k: v for k, v in kw.items() if k != "full_cell_map"}))

        def add_scan(self, cloud, pose, frame_index):
            outer.log.append(("add_scan", self.slot, len(cloud), np.array(pose, np.float64).copy(), frame_index))

        def close(self):
            outer.log.append(("assembly_close", self.slot))

    class Rounds:
        """stands in for keyframes.Keyframe_rounds: the key-frame rounds of a step, asked for once, for the slots named"""

        def __init__(self, assemblies, store=None, **services):
            assert not any(services.values())

        def run(self, slots):
            outer.log.append(("process_waiting", list(slots)))
            return [[("loop", s)] if s == 0 else [] for s in slots]

        def close(self):
            pass

    def no_single_handles(*a, **kw):
        raise AssertionError("the batched mode must not create per-sequence History_buffer handles")

    classes = dict(st.classes, History_buffer=no_single_handles, History_buffer_batch=HistBatch)
    for k, v in classes.items():
        monkeypatch.setattr(mapping, k, v)
    monkeypatch.setattr(keyframes, "Keyframe_assembly", Assembly)
    monkeypatch.setattr(keyframes, "Keyframe_rounds", Rounds)
    return st


def test_loop_appends_once_per_step_for_the_accepted_slots_and_feeds_their_key_frames(stubbed):
    st = stubbed
    st.reject.add((1, 4))  # sequence 1 is rejected at its frame 4
    lc = dict(scans_of_each_keyframe=6, scans_between_two_keyframe=3, max_points=5000)
    lb = mapping.Laser_mapping_batch(3, batched_history=True, full_maps=True, key_frames=True, scan_points=100, init_accumulate_frames=2,
                                     cell_resolution=0.8, threshold_cell_revisit=7, loop_closure=lc)
    assert [e for e in st.log if e[0] == "enable_full_maps"] == [("enable_full_maps", 5000, 0.8, 7)]  # the first allocation is loop_closure["max_points"]
    assert not [e for e in st.log if e[0] == "enable_cell_maps"]
    made = [e for e in st.log if e[0] == "assembly"]
    assert [e[1] for e in made] == [0, 1, 2]
    assert all(e[2] == dict(device=0, cell_resolution=0.8, threshold_cell_revisit=7, scans_of_each_keyframe=6, scans_between_two_keyframe=3) for e in made)
    assert lc == dict(scans_of_each_keyframe=6, scans_between_two_keyframe=3, max_points=5000)  # the caller's dictionary is left alone
    scan = np.zeros((100, 4), np.float32)
    n_loops = 0
    for step in range(6):
        st.log.clear()
        out = lb.process_new_scans([scan, scan if step >= 1 else None, scan])
        accepted = tuple(bool(out[s] == 1) for s in range(3))
        names = [e[0] for e in st.log]
        appends = [e for e in st.log if e[0] == "append_full"]
        assert len(appends) == 1 and appends[0][1] == accepted and appends[0][3] == 3
        assert names.index("add_voxel") < names.index("append_full") < names.index("refresh")  # after the add, as laser_mapping.hpp:1439-1527 has it
        for s in range(3):
            if accepted[s]:
                assert np.array_equal(appends[0][2][s], lb.poses[s])  # at the pose the step accepted
        scans = [e for e in st.log if e[0] == "add_scan"]
        assert [e[1] for e in scans] == [s for s in range(3) if accepted[s]]  # rejected and idle slots get none
        for e in scans:
            assert e[2] == 0 and np.array_equal(e[3], lb.poses[e[1]]) and e[4] == int(lb.frame_index[e[1]])  # its own frame index, after the increment
        assert [e[1] for e in st.log if e[0] == "process_waiting"] == [[e[1] for e in scans]]
        n_loops += accepted[0]
    assert out.tolist() == [1, 0, 1]  # (sequence 1 started a step late: this is its frame 4)
    assert lb.frame_index.tolist() == [6, 5, 6]
    assert lb.loops == [[("loop", 0)] * n_loops, [], []]
    assert lb.full_map(2).s == 2
    st.log.clear()
    lb.close()
    assert [e[1] for e in st.log if e[0] == "assembly_close"] == [0, 1, 2]
    # full maps alone: no key frames are made; a first allocation below one scan is raised to it, without the key the store starts at 2^18
    st.log.clear()
    lb = mapping.Laser_mapping_batch(2, batched_history=True, full_maps=True, scan_points=100, loop_closure=dict(max_points=10))
    assert lb.keyframes is None and lb.loops is None
    lb.process_new_scans([scan, scan])
    assert not [e for e in st.log if e[0] in ("assembly", "add_scan")]
    lb.close()
    mapping.Laser_mapping_batch(2, batched_history=True, full_maps=True, scan_points=100).close()
    assert [e[1] for e in st.log if e[0] == "enable_full_maps"] == [100, 1 << 18]


def test_the_two_new_refusals_hold_and_loop_closure_if_enable_stays_refused(stubbed):
    with pytest.raises(ValueError, match="batched_history"):
        mapping.Laser_mapping_batch(2, full_maps=True, scan_points=100)
    with pytest.raises(ValueError, match="batched_history"):
        mapping.Laser_mapping_batch(2, batched_history=False, full_maps=True, key_frames=True, scan_points=100)
    with pytest.raises(ValueError, match="full_maps"):
        mapping.Laser_mapping_batch(2, batched_history=True, key_frames=True, scan_points=100)
    for kw in (dict(loop_closure_if_enable=1), dict(loop_closure_if_enable=1, full_maps=True), dict(loop_closure_if_enable=1, full_maps=True, key_frames=True),
               dict(keep_cell_maps=True, full_maps=True), dict(matching_mode=1, full_maps=True), dict(lidar_type="velodyne", full_maps=True)):
        with pytest.raises(ValueError):
            mapping.Laser_mapping_batch(2, batched_history=True, scan_points=100, **kw)
    with pytest.raises(TypeError):
        mapping.Laser_mapping(scan_points=100, full_maps=True)  # not an argument of Laser_mapping
    lb = mapping.Laser_mapping_batch(2, batched_history=True, scan_points=100)
    assert lb.full_maps is False and lb.key_frames is False and not [e for e in stubbed.log if e[0] == "enable_full_maps"]
    with pytest.raises(ValueError):
        lb.full_map(0)
    lb.close()
