"""CPU tier of the scan log of the batched match buffer and of the map refinement in the lock-step loop (tests/test_gpu_scan_log.py is
the GPU tier): the entry points are declared, exported and bound and refuse null arguments without a device; the two kernels, compiled
for the CPU from their own unit (tests/scan_log_host.cpp on tests/cellmap_batch_shim) with the bookkeeping of ll_scan_log.h, replay
twelve steps and equal a numpy replay of the FIFO rule, also under -fsanitize=address,undefined; and Laser_mapping_batch with the full
set of switches, against stubbed handles, makes one log_full per step for exactly accepted & added, hands over where the solo
assembly flushes, and makes one add_logged per round and one refine per round with loops."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import api, capi, keyframes, mapping
from tests.test_keyframes_accumulate import StubCellMap, StubRefine, StubSolver
from tests.test_multimap_host import _Stubs

REAL_ASSEMBLY = keyframes.Keyframe_assembly   # (the loop tests put a subclass in its place)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ll_history_batch_enable_scan_log", "ll_history_batch_log_full_fe", "ll_history_batch_scan_log_hand_over", "ll_history_batch_scan_log_drop",
       "ll_history_batch_scan_log_read", "ll_history_batch_scan_log_work", "ll_map_refine_add_logged")


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
    for m in ("enable_scan_log", "log_full", "hand_over", "drop_groups", "read_group", "scan_log_work", "scan_log"):
        assert callable(getattr(api.History_buffer_batch, m))
    assert callable(api.Map_refine.add_logged)
    for m in ("hand_over", "drop"):  # what a Keyframe_assembly asks of its scan log
        assert callable(getattr(api.Scan_log_slot, m))
    adapter = open(os.path.join(ROOT, "include", "loam_livox_adapter.hpp")).read()
    for name in NEW:
        assert name in adapter, name


def test_null_arguments_are_refused_without_a_device():
    L = capi.load()
    n = C.c_int64(0)
    out = (C.c_int64 * 4)()
    assert L.ll_history_batch_enable_scan_log(None, 3, 8) < 0 and b"ll_history_batch_enable_scan_log: null" in L.ll_last_error()
    assert L.ll_history_batch_log_full_fe(None, None, None) < 0 and b"ll_history_batch_log_full_fe: null" in L.ll_last_error()
    assert L.ll_history_batch_scan_log_hand_over(None, 0, C.byref(n)) < 0 and b"ll_history_batch_scan_log_hand_over: null" in L.ll_last_error()
    assert L.ll_history_batch_scan_log_drop(None, 0, None) < 0 and b"ll_history_batch_scan_log_drop: null" in L.ll_last_error()
    assert L.ll_history_batch_scan_log_read(None, 1, None, 0, C.byref(n)) < 0 and b"ll_history_batch_scan_log_read: null" in L.ll_last_error()
    assert L.ll_history_batch_scan_log_work(None, out) < 0 and b"ll_history_batch_scan_log_work: null" in L.ll_last_error()
    assert L.ll_map_refine_add_logged(None, None, 0, None, None, 0.5, None, None, None) < 0 and b"ll_map_refine_add_logged: null" in L.ll_last_error()


# ---- the kernels and the bookkeeping on the host --------------------------------------------------------------------------------------
S, T, HISTORY, MAX_PTS, CHUNK_BLOCKS = 3, 12, 3, 300, 2
HOST_CHUNK = 128   # points of a work item of the gather in the host build (2048 on the device): a 300-point scan is three items
SIZES = [300, 257, 256, 1, 0, -1]   # the 256-thread boundary from both sides, one point, an empty scan, an idle slot (-1)


def schedule():
    """per step, per slot: (n, named, xf [n, 4], scan [MAX_PTS, 4], full_idx [n]); the hand-overs and drops behind the step.  Shared with the
    GPU tier, which makes the same steps with real scans."""
    rng = np.random.default_rng(41)
    steps = []
    for t in range(T):
        slots = []
        for s in range(S):
            n = SIZES[(t + 2 * s) % len(SIZES)]
            named = n >= 0 and not (t == 6 and s == 0) and not (t == 9 and s == 2)   # two scans the add rule kept out: active, not logged
            if n < 0:
                slots.append((n, False, None, None, None))
                continue
            scan = rng.uniform(-5, 5, (MAX_PTS, 4)).astype(np.float32)
            idx = rng.permutation(MAX_PTS)[:n].astype(np.int32)
            xf = np.c_[scan[idx, :3] + np.float32(100.0 * (s + 1)), np.zeros(n, np.float32)].astype(np.float32)
            if n >= 256:   # two refused points: the gather's marker for a non-finite point, and for an index outside the scan
                scan[idx[7], 1] = np.nan
                idx[200] = MAX_PTS + 5
                xf[[7, 200]] = [np.nan, np.nan, np.nan, 0.0]
            slots.append((n, named, xf, scan, idx))
        hands = list(range(S)) if t % 4 == 3 else []
        drops = [1] if t == 8 else []   # the second group ever handed over
        steps.append((slots, hands, drops))
    return steps


REQUESTS = [[3], [4, 6], [8], []]   # by ordinal: one group, two groups, whatever slot 2 held at the last hand-over, no group at all


def replay(steps):
    """the FIFO rule in numpy -> (groups by ordinal, None when dropped; blocks in use after every step)"""
    fifo, groups, in_use = [[] for _ in range(S)], [], []
    for slots, hands, drops in steps:
        for s, (n, named, xf, scan, idx) in enumerate(slots):
            if n < 0:
                continue
            if named:
                ok = (idx >= 0) & (idx < MAX_PTS)
                w = np.where(ok, scan[np.clip(idx, 0, MAX_PTS - 1), 3], np.float32(0))
                w = np.where(ok & np.isfinite(scan[np.clip(idx, 0, MAX_PTS - 1), :3]).all(axis=1), w, np.float32(0)).astype(np.float32)
                fifo[s].append(np.c_[xf[:, :3], w].astype(np.float32))
            if len(fifo[s]) > HISTORY:
                fifo[s].pop(0)
        for s in hands:
            groups.append(list(fifo[s]))
            fifo[s] = []
        for g in drops:
            groups[g] = None
        in_use.append(sum(len(f) for f in fifo) + sum(len(g) for g in groups if g is not None))
    return groups, in_use


def cat(scans):
    return np.concatenate(scans) if scans else np.zeros((0, 4), np.float32)


def build_host(tmp, flags=()):
    exe = os.path.join(tmp, "scan_log_host" + ("_san" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-DSL_CHUNK=%d" % HOST_CHUNK, *flags, "-x", "c++", "-I",
                           os.path.join(ROOT, "tests", "cellmap_batch_shim"), "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "scan_log_host.cpp")])
    return exe


def run_host(exe, tmp):
    steps = schedule()
    buf = np.array([S, T, HISTORY, MAX_PTS, CHUNK_BLOCKS], np.int32).tobytes()
    for slots, hands, drops in steps:
        for n, named, xf, scan, idx in slots:
            buf += np.array([n, int(named)], np.int32).tobytes()
            if n >= 0:
                buf += xf.tobytes() + scan.tobytes() + idx.tobytes()
        buf += np.array([len(hands)] + hands + [len(drops)] + drops, np.int32).tobytes()
    off = np.concatenate([[0], np.cumsum([len(r) for r in REQUESTS])])
    buf += np.array([len(REQUESTS)] + off.tolist() + [g for r in REQUESTS for g in r], np.int32).tobytes()
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(pin, "wb").write(buf)
    done = subprocess.run([exe, pin, pout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert done.returncode == 0, done.stdout.decode()
    raw = np.fromfile(pout, np.int32)
    per_step = raw[:3 * T].reshape(T, 3)
    pos = 3 * T
    n_groups = int(raw[pos])
    pos += 1
    groups = []
    for _ in range(n_groups):
        alive, n = int(raw[pos]), int(raw[pos + 1])
        pos += 2
        groups.append(raw[pos:pos + 4 * n].reshape(n, 4).copy() if alive else None)
        pos += 4 * n if alive else 0
    R = len(REQUESTS)
    req_off = raw[pos:pos + 2 * (R + 1)].view(np.int64)
    pos += 2 * (R + 1)
    stage = raw[pos:pos + 4 * int(req_off[-1])].reshape(-1, 4)
    pos += 4 * int(req_off[-1])
    tail = raw[pos:]
    assert len(tail) == 3
    return per_step, groups, req_off, stage, tail


def check_host_run(per_step, groups, req_off, stage, tail):
    want, in_use = replay(schedule())
    assert len(groups) == len(want) == 9
    for k, (g, w) in enumerate(zip(groups, want)):
        assert (g is None) == (w is None), k
        if w is not None:
            assert np.array_equal(g, cat(w).view(np.int32)), (k, "group in bits")
    assert per_step[:, 0].tolist() == in_use                                  # blocks in use = the FIFOs and the live groups
    assert (np.diff(per_step[:, 1]) >= 0).all() and per_step[0, 1] > CHUNK_BLOCKS and (per_step[:, 1] % CHUNK_BLOCKS == 0).all()   # it grew, by chunks
    # ... and only for want of blocks: a step holds at most S blocks more than it leaves in use (the trims), a chunk is allocated
    # only when the free list is short, so the pool stays below the peak in use + S + one chunk
    assert (per_step[:, 1] < np.maximum.accumulate(per_step[:, 0]) + S + CHUNK_BLOCKS).all()
    assert per_step[:, 2].all()                                                # every step had something to log
    wants = [cat([sc for g in r for sc in want[g]]) for r in REQUESTS]
    assert req_off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in wants])]).tolist()
    assert np.array_equal(stage, cat(wants).view(np.int32))
    assert len(wants[3]) == 0 and len(wants[1]) > 2 * HOST_CHUNK           # an empty request; one whose scans are several work items each
    assert tail[:2].tolist() == [1, 1]
    assert tail[2] == in_use[-1] - sum(len(want[g]) for r in REQUESTS for g in r)   # the gather's groups were consumed


def test_schedule_holds_the_cases():
    steps = schedule()
    want, _ = replay(steps)
    sizes = {n for slots, _, _ in steps for n, *_ in slots}
    assert sizes == set(SIZES)
    assert [(steps[t][0][s][0] > 0, steps[t][0][s][1]) for t, s in ((6, 0), (9, 2))] == [(True, False)] * 2   # active, kept out by the add rule
    assert max(len(g) for g in want if g is not None) == HISTORY               # a FIFO was trimmed: four pushes between two hand-overs
    assert any(np.isnan(sc).any() for g in want if g is not None for sc in g)  # the markers of refused points stay in the blocks
    assert any(len(sc) == 0 for g in want if g is not None for sc in g)        # an empty scan is a scan of the FIFO
    assert want[1] is None and sum(g is not None for g in want) == 8
    # the intensity is the scan's through full_idx, not the gather's 0
    assert all(np.any(sc[:, 3] != 0) for g in want if g is not None for sc in g if len(sc) > 1)


def test_kernels_and_bookkeeping_on_the_host_equal_the_replay(tmp_path):
    check_host_run(*run_host(build_host(str(tmp_path)), str(tmp_path)))


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone executable with its own main, instrumented as a whole: nothing is preloaded"""
    exe = build_host(str(tmp_path), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"))
    check_host_run(*run_host(exe, str(tmp_path)))


# ---- the loop's bookkeeping, device handles stubbed ---------------------------------------------------------------------------------------
EACH, BETWEEN = 6, 3
REJECTED_BY_ADD_RULE = {(0, 4), (2, 7), (1, 5), (1, 6)}   # (slot, its add number): accepted by the registrar, kept out of the history


@pytest.fixture
def stubbed(monkeypatch):
    st = _Stubs()
    outer = st
    st.adds = [0, 0, 0]          # add_scan calls per slot so far

    class Slot:
        def __init__(self, s):
            self.s = s

        def append_cloud_touched(self, cloud=None, min_points=3):
            return np.array([[self.s, 0, 0]], np.int32)

        def close(self):
            pass

    class LogSlot:
        def __init__(self, batch, s):
            self.batch, self.s = batch, s

        def hand_over(self):
            outer.next_group = getattr(outer, "next_group", 0) + 1
            outer.log.append(("hand_over", self.s, outer.adds[self.s], outer.next_group))
            return outer.next_group

        def drop(self, ids):
            outer.log.append(("drop", self.s, list(ids)))

    class HistBatch:
        def __init__(self, n_sequences, *a, **kw):
            self.S = n_sequences
            self.frames = [0] * n_sequences

        def enable_full_maps(self, *a):
            outer.log.append(("enable_full_maps",) + a)

        def enable_scan_log(self, maximum_history_size, initial_scans=None):
            outer.log.append(("enable_scan_log", maximum_history_size))

        def full_map(self, s):
            return Slot(s)

        def scan_log(self, s):
            return LogSlot(self, s)

        def add_voxel(self, vc, vs, poses, gate=None, active=None, t=0.0, a=0.0):
            on = [bool(x) for x in active]
            added = []
            for s in range(self.S):
                self.frames[s] += on[s]
                added.append(on[s] and (s, self.frames[s]) not in REJECTED_BY_ADD_RULE)
            outer.log.append(("add_voxel", tuple(on), tuple(added)))
            return np.array(added)

        def append_full(self, fe, poses, active=None, min_points=3, lists=True):
            outer.log.append(("append_full", tuple(bool(x) for x in active)))
            return np.zeros(self.S, np.int64)

        def log_full(self, fe, active=None):
            outer.log.append(("log_full", tuple(bool(x) for x in active)))

        def extract_cells(self, kind, seqs, wants, dsts):
            outer.log.append(("extract_cells", tuple(seqs)))

        def refresh(self, maps, active=None):
            outer.log.append(("refresh",))
            return np.array(self.frames), np.array(self.frames)

        def size(self, s):
            return min(self.frames[s], 5)

        def close(self):
            pass

    class Refine(StubRefine):
        def __init__(self, **kw):
            super().__init__()

        def __len__(self):   # (as api.Map_refine: an empty store is falsy, and is a handle all the same)
            return len(self.clouds)

        def add_logged(self, batch, groups_per_request, leaf=0.5):
            outer.log.append(("add_logged", [list(g) for g in groups_per_request], leaf))
            first = len(self.clouds)
            self.clouds += [np.full((1, 4), first + r, np.float32) for r in range(len(groups_per_request))]
            R = len(groups_per_request)
            return np.arange(first, first + R), np.ones(R, np.int64), np.zeros(R, np.int32)

        def refine(self, ids, poses_ori, poses_opm, leaf=0.2, transform_first=False):
            outer.log.append(("refine", list(ids), leaf))
            return super().refine(ids, poses_ori, poses_opm, leaf, transform_first)

    class Solver(StubSolver):
        def __init__(self, **kw):
            pass

    class Asm(REAL_ASSEMBLY):
        """the real assembly on stubbed maps; its detector accepts a loop when its third key frame is processed"""

        def new_keyframe_map(self, n_cells):
            return StubCellMap()

        def add_scan(self, cloud, pose, index, history_added=True):
            outer.adds[self.m_pt_cell_map_full.s] += 1
            outer.log.append(("add_scan", self.m_pt_cell_map_full.s, bool(history_added)))
            return super().add_scan(cloud, pose, index, history_added=history_added)

        def walk_front(self, sims=None):
            last, _ = self._front
            self._front = None
            if len(self.keyframe_vec) != 3:
                return []
            loop = dict(his=0, last=2, inlier_threshold=0.1, icp_q=np.array([0, 0, 0, 1.0]), icp_t=np.zeros(3))
            self.loops.append(loop)
            self.pending_loops.append(loop)
            self.if_end = True
            return [loop]

    def no_single_handles(*a, **kw):
        raise AssertionError("the batched mode must not create per-sequence History_buffer handles")

    classes = dict(st.classes, History_buffer=no_single_handles, History_buffer_batch=HistBatch)
    for k, v in classes.items():
        monkeypatch.setattr(mapping, k, v)
    monkeypatch.setattr(keyframes, "Keyframe_assembly", Asm)
    monkeypatch.setattr(api, "Map_refine", Refine)
    monkeypatch.setattr(api, "Pose_graph", Solver)
    return st


def solo_flushes(n_scans):
    """the add numbers at which the solo assembly (host FIFO) flushes: where it opens a key frame behind a back one"""
    ka = REAL_ASSEMBLY(full_cell_map=type("M", (), dict(append_cloud_touched=lambda self, c, m=3: np.array([[0, 0, 0]], np.int32), close=lambda self: None))(),
                                     scans_of_each_keyframe=EACH, scans_between_two_keyframe=BETWEEN, pose_graph=StubSolver(), map_refinement=StubRefine())
    out = []
    for k in range(1, n_scans + 1):
        back = ka.m_keyframe_of_updating_list[-1]
        ka.add_scan(np.zeros((1, 4), np.float32), np.array([0, 0, 0, 1, 0, 0, 0.0]), k)
        ka.m_keyframe_need_precession_list.clear()
        if ka.m_keyframe_of_updating_list[-1] is not back:
            out.append(k)
    return out


def test_loop_logs_hands_over_adds_and_refines_once_per_step_and_round(stubbed):
    st = stubbed
    st.reject.add((1, 4))  # sequence 1 is rejected by the registrar at its frame 4
    lc = dict(scans_of_each_keyframe=EACH, scans_between_two_keyframe=BETWEEN, pose_graph=True, map_refinement=True, minimum_keyframe_differen=10 ** 6)
    # construction with the full set of switches no longer raises
    lb = mapping.Laser_mapping_batch(3, batched_history=True, full_maps=True, key_frames=True, scan_points=100, init_accumulate_frames=2,
                                     maximum_history_size=4, loop_closure=lc)
    assert [e for e in st.log if e[0] == "enable_scan_log"] == [("enable_scan_log", 4)]
    assert isinstance(lb.map_refine, StubRefine) and lb.rounds.assemblies == lb.keyframes and all(ka.rounds is lb.rounds for ka in lb.keyframes) and lb.rounds.map_refine.handle is lb.map_refine
    assert lc["map_refinement"] is True                                        # the caller's dictionary is left alone
    scan = np.zeros((100, 4), np.float32)
    hand_overs, rounds_with_loops, refines, n_steps = {0: [], 1: [], 2: []}, 0, 0, 16
    for step in range(n_steps):
        st.log.clear()
        out = lb.process_new_scans([scan, scan if step >= 1 else None, scan])
        accepted = tuple(bool(out[s] == 1) for s in range(3))
        names = [e[0] for e in st.log]
        added = [e for e in st.log if e[0] == "add_voxel"][0][2]
        logs = [e for e in st.log if e[0] == "log_full"]
        assert len(logs) == 1 and logs[0][1] == tuple(a and b for a, b in zip(accepted, added))   # one per step, exactly accepted & added
        assert names.index("append_full") < names.index("log_full") < names.index("add_scan")   # :1442, :1456, :1524
        assert [(e[1], e[2]) for e in st.log if e[0] == "add_scan"] == [(s, added[s]) for s in range(3) if accepted[s]]
        for e in st.log:
            if e[0] == "hand_over":
                hand_overs[e[1]].append(e[2])
        # a round is one extract_cells; behind each at most one add_logged, with one request per key frame analysed in it
        cuts = [i for i, n in enumerate(names) if n == "extract_cells"] + [len(names)]
        for a, b in zip(cuts, cuts[1:]):
            seg = st.log[a:b]
            adds = [e for e in seg if e[0] == "add_logged"]
            assert len(adds) == 1 and len(adds[0][1]) == len(seg[0][1]) and adds[0][2] == 0.5
            runs = [e for e in seg if e[0] == "refine"]
            assert len(runs) <= 1
            rounds_with_loops += len(runs)
        refines += sum(1 for e in st.log if e[0] == "refine")
    assert st.adds == [16, 14, 16] and rounds_with_loops == refines
    for s in range(3):
        assert hand_overs[s] == [k for k in solo_flushes(st.adds[s])], s       # the scans where the solo assembly flushes
    # slots 0 and 2 move in lock step: their loops close in one round and are refined in ONE run; slot 1 started late: a run of its own
    assert refines == 2 and all(ka.refined is not None and [i for i, _ in ka.refined] == [2, 0] for ka in lb.keyframes)
    assert all(kf.cloud_id is not None and kf.m_accumulated_point_cloud == [] for ka in lb.keyframes for kf in ka.keyframe_vec)
    ids = [[kf.cloud_id for kf in ka.keyframe_vec] for ka in lb.keyframes]
    assert sorted(i for row in ids for i in row) == list(range(9))             # one store: consecutive ids over the three assemblies
    for ka in lb.keyframes:                                                    # every assembly got its own selections back
        assert [float(c[0, 0]) for _, c in ka.refined] == [float(ka.keyframe_vec[2].cloud_id), float(ka.keyframe_vec[0].cloud_id)]
    st.log.clear()
    lb.close()
    dropped = [g for e in st.log if e[0] == "drop" for g in e[2]]
    assert len(dropped) == len(set(dropped)) and len(dropped) > 0              # close drops the groups of the key frames still open or waiting


def test_map_refinement_off_makes_the_calls_of_before(stubbed):
    st = stubbed
    lc = dict(scans_of_each_keyframe=EACH, scans_between_two_keyframe=BETWEEN, pose_graph=True)
    lb = mapping.Laser_mapping_batch(2, batched_history=True, full_maps=True, key_frames=True, scan_points=100, init_accumulate_frames=2, loop_closure=lc)
    assert lb.map_refine is None and all(ka.scan_log is None and not ka.map_refinement for ka in lb.keyframes)
    scan = np.zeros((100, 4), np.float32)
    for step in range(15):
        lb.process_new_scans([scan, scan])
    names = {e[0] for e in st.log}
    assert not names & {"enable_scan_log", "log_full", "hand_over", "drop", "add_logged", "refine"}
    assert {"append_full", "add_scan", "extract_cells"} <= names and all(e[2] for e in st.log if e[0] == "add_scan")
    assert all(ka.refined is None and ka.poses_opm is not None for ka in lb.keyframes)   # the loops still close, nothing is refined
    lb.close()


def test_refusals_keep_their_words(stubbed):
    lc = dict(pose_graph=True, map_refinement=True)
    for kw in (dict(), dict(batched_history=True), dict(batched_history=True, full_maps=True)):   # (the last: no key_frames)
        with pytest.raises(ValueError, match="map_refinement is not available in the batched loop"):
            mapping.Laser_mapping_batch(2, scan_points=100, loop_closure=lc, **kw)
    with pytest.raises(ValueError, match="map_refinement is not available in the batched loop"):   # no pose graph
        mapping.Laser_mapping_batch(2, batched_history=True, full_maps=True, key_frames=True, scan_points=100, loop_closure=dict(map_refinement=True))
