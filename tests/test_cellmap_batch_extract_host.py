"""CPU tier of ll_history_batch_extract_cells (tests/test_gpu_cellmap_batch_extract.py is the GPU tier): the entry points are declared,
exported and bound and refuse null handles without a device; the launch chain -- mark, scan, totals, table, gather -- compiled for the
CPU from the kernel unit itself (tests/cellmap_batch_extract_host.cpp on tests/cellmap_batch_shim), over a store of three slots that
the append and materialise chains built, gives bit for bit what the numpy selection of Keyframe_assembly._materialize_host takes out
of each slot's dump; the same driver runs clean as a stand-alone program under the address and undefined-behaviour sanitizers;
Keyframe_assembly.materialize takes its routes in the documented order; and Laser_mapping_batch._full_step extracts once per round,
after every add_scan and before any process_waiting, without ever dumping a slot."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 2.0          # set_resolution halves what it is given: cells of 1 m, cell k covers [k, k + 1) on every axis
LIMIT = 1 << 20
S = 3


def pack(ijk):
    c = (np.asarray(ijk, np.int64).reshape(-1, 3) + LIMIT).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def unpack(ckey):
    k = np.asarray(ckey, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([(k >> np.uint64(42)) & m, (k >> np.uint64(21)) & m, k & m], axis=1).astype(np.int64) - LIMIT


def select(src, want_ijk):
    """_materialize_host's selection on one slot's map in dump form: isin over the packed cells, then the points of the selected
    cells, cell after cell.  An index beyond +-2^20 names no cell."""
    want = np.asarray(want_ijk, np.int64).reshape(-1, 3)
    want = want[(np.abs(want) < LIMIT).all(axis=1)]
    sel = np.flatnonzero(np.isin(src["ckey"], pack(want)))
    start = src["cstart"].astype(np.int64)
    lens = start[sel + 1] - start[sel]
    first = np.cumsum(lens) - lens
    idx = np.repeat(start[sel] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    return dict(pts=src["pts"][idx], pkey=src["pkey"][idx], ckey=src["ckey"][sel],
                cstart=np.r_[first, lens.sum()].astype(np.int32) if len(sel) else np.zeros(1, np.int32), n_found=len(sel), n_points=int(lens.sum()))


def cloud(cells_and_sizes, rng):
    """points well inside their cells, in a shuffled insertion order"""
    cell = np.repeat(np.array([c for c, _ in cells_and_sizes], np.int64), [n for _, n in cells_and_sizes], axis=0)
    pts = (cell.astype(np.float64) + 0.5 + rng.uniform(-0.3, 0.3, cell.shape)).astype(np.float32)
    return pts[rng.permutation(len(pts))]


A, B, Cc, X, Y = (0, 0, 0), (1, 0, 0), (2, 0, 0), (5, 5, 5), (6, 5, 5)
EDGE_HI, EDGE_LO = (LIMIT - 1, 0, 0), (-(LIMIT - 1), 0, 0)
RUN = [(10, j, 0) for j in range(70)]       # more than 64 one-point cells ...
BIG = (11, 0, 0)                            # ... followed, in key order, by a cell of more than 128 points
ABSENT = [(40 + i, -3, 7) for i in range(6)]
SLOT0 = [(A, 63), (B, 64), (Cc, 65), (X, 7), (EDGE_HI, 3), (EDGE_LO, 3), (BIG, 150)] + [(c, 1) for c in RUN]


def slot2_cells(rng):
    ks = set()
    while len(ks) < 40:
        k = tuple(int(v) for v in rng.integers(-9, 10, 3))
        if k not in (X, Y):
            ks.add(k)
    return [(X, 9), (Y, 4)] + [(k, int(rng.integers(1, 21))) for k in sorted(ks)]


def whole_slot_lists():
    """'every cell of slot s' after the further append, by name"""
    rng = np.random.default_rng(17)
    cloud(SLOT0, rng)
    return {"ALL0": [c for c, _ in SLOT0] + [(3, 3, 3)], "ALL1": [X, (-2, -2, -2)], "ALL2": [c for c, _ in slot2_cells(rng)]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("cellmap_batch_extract")
    base = ["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "tests", "cellmap_batch_shim"), "-I",
            os.path.join(ROOT, "loam_livox_amd", "csrc")]
    src = os.path.join(ROOT, "tests", "cellmap_batch_extract_host.cpp")
    plain, san = str(d / "cellmap_batch_extract_host"), str(d / "cellmap_batch_extract_host_san")
    subprocess.check_call(base + ["-O1", "-o", plain, src])
    subprocess.check_call(base + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san, src])
    return dict(plain=plain, san=san, dir=str(d))


def make_input():
    """the two first clouds and the writers of the driver's input: append( clouds per slot ), op( code ), extract( name, slots, lists )"""
    cells = whole_slot_lists()
    rng = np.random.default_rng(17)
    s0, s2 = cloud(SLOT0, rng), cloud(slot2_cells(rng), rng)
    buf, ops = [np.array([S], np.int32).tobytes(), np.array([RES], np.float32).tobytes()], []

    def append(clouds):
        buf.append(np.array([1], np.int32).tobytes())
        for c in clouds:
            buf.append(np.array([-1 if c is None else len(c)], np.int32).tobytes())
            if c is not None:
                buf.append(np.ascontiguousarray(c, np.float32).tobytes())

    def op(code):
        buf.append(np.array([code], np.int32).tobytes())
        if code == 4:
            ops.append(("dump",))

    def extract(name, seq, lists):
        lists = [np.asarray(cells[l] if isinstance(l, str) else l, np.int64).reshape(-1, 3) for l in lists]
        off = np.r_[0, np.cumsum([len(l) for l in lists])].astype(np.int32)
        buf.append(np.array([3, len(seq)], np.int32).tobytes() + np.array(seq, np.int32).tobytes() + off.tobytes())
        buf.append(wrap32(np.concatenate(lists)).tobytes())
        ops.append(("extract", name, list(seq), lists))
    return buf, ops, append, op, extract, s0, s2


def wrap32(ijk):
    """int64 indices as the int32 the ABI takes (an index of 2^21 and more stays what it is: far beyond the range check)"""
    return np.asarray(ijk, np.int64).astype(np.int32)


def the_input():
    buf, ops, append, op, extract, s0, s2 = make_input()
    half0, half2 = len(s0) // 2, len(s2) // 2
    append([s0[:half0], None, s2[:half2]])          # slot 1 sits out: its map stays empty
    append([s0[half0:], np.zeros((0, 3), np.float32), s2[half2:]])
    op(2)
    op(4)
    beyond = [(LIMIT, 0, 0), (-LIMIT, 0, 0), (A[0] + (1 << 21), 0, 0), (0, -1, (1 << 21))]   # out of range; unchecked, the last two would alias A
    extract("slots [2, 0]", [2, 0], [[X, Y, ABSENT[0], X], [A, X, Y, A] + beyond + ABSENT])   # Y lives in slot 2 only: not found in slot 0
    extract("shared cell named in one list only", [0, 2], [[B], [X]])
    extract("R = 1, the run and the big cell", [0], [RUN[::-1] + [BIG]])
    extract("R = 3, boundary inside a group", [0, 1, 2], [[A], [A, X, Y], "ALL2"])
    for name, c in (("63 points", A), ("64 points", B), ("65 points", Cc)):
        extract(name, [0], [[c]])
    extract("nothing found and an empty list", [2, 0], [ABSENT, []])
    extract("empty map alone", [1], [[A, X]])
    extract("edges of the index range", [0], [[EDGE_HI, EDGE_LO] + beyond])
    op(4)
    more = np.random.default_rng(23)
    append([cloud([(A, 5), ((3, 3, 3), 66)], more), cloud([(X, 12), ((-2, -2, -2), 1)], more), None])
    op(2)
    op(4)
    extract("after a further append", [1, 2, 0], ["ALL1", "ALL2", "ALL0"])
    op(4)
    return b"".join(buf), ops


def parse(raw, ops):
    pos = 0

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos)
        pos += a.nbytes
        return a
    out = []
    for o in ops:
        if o[0] == "dump":
            slots = []
            for _ in range(S):
                nc, npts = take(np.int32, 2)
                slots.append(dict(ckey=take(np.uint64, nc), cstart=take(np.int32, nc + 1), pts=take(np.float32, 4 * npts).reshape(-1, 4),
                                  pkey=take(np.uint64, npts)))
            out.append(slots)
        else:
            reqs = []
            for _ in o[2]:
                found, points, frame, m_cells, m_pts = take(np.int32, 5)
                reqs.append(dict(n_found=int(found), n_points=int(points), frame=int(frame), mirrors=(int(m_cells), int(m_pts)),
                                 ckey=take(np.uint64, found), cstart=take(np.int32, found + 1), clast=take(np.int32, found),
                                 pts=take(np.float32, 4 * points).reshape(-1, 4), pkey=take(np.uint64, points)))
            out.append(reqs)
    assert pos == len(raw)
    return out


@pytest.fixture(scope="module")
def run(exes):
    data, ops = the_input()
    pin, pout = os.path.join(exes["dir"], "in.bin"), os.path.join(exes["dir"], "out.bin")
    open(pin, "wb").write(data)
    subprocess.check_call([exes["plain"], pin, pout])
    raw = open(pout, "rb").read()
    res = parse(raw, ops)
    named, dumps, store = {}, [], None
    for o, r in zip(ops, res):
        if o[0] == "dump":
            dumps.append(r)
            store = r
        else:
            named[o[1]] = (o[2], o[3], r, store)   # slots, lists, results, the store's dump at the time
    return dict(named=named, dumps=dumps, pin=pin, raw=raw)


def assert_same(got, want, what):
    assert (got["n_found"], got["n_points"]) == (want["n_found"], want["n_points"]), what
    assert got["mirrors"] == ((want["n_found"], want["n_points"]) if want["n_points"] else (0, 0)), what
    assert got["frame"] == (2 if want["n_points"] else 0), what
    assert np.array_equal(got["ckey"], want["ckey"]), what
    assert np.array_equal(got["cstart"], want["cstart"]), what
    assert not got["clast"].any(), what
    assert np.array_equal(got["pts"].view(np.uint32), want["pts"].view(np.uint32)), what
    assert np.array_equal(got["pkey"], want["pkey"]), what


CASES = ["slots [2, 0]", "shared cell named in one list only", "R = 1, the run and the big cell", "R = 3, boundary inside a group", "63 points",
         "64 points", "65 points", "nothing found and an empty list", "empty map alone", "edges of the index range", "after a further append"]


def test_the_store_has_the_shapes_the_cases_need(run):
    d = run["dumps"][0]
    assert len(d[1]["ckey"]) == 0 and len(d[1]["pts"]) == 0           # the empty map
    lens0 = dict(zip(map(tuple, unpack(d[0]["ckey"])), np.diff(d[0]["cstart"])))
    assert [lens0[c] for c in (A, B, Cc, X, BIG, EDGE_HI, EDGE_LO)] == [63, 64, 65, 7, 150, 3, 3]
    assert all(lens0[c] == 1 for c in RUN) and len(RUN) > 64
    cells2 = set(map(tuple, unpack(d[2]["ckey"])))
    assert X in cells2 and Y in cells2 and Y not in lens0 and A not in cells2
    assert sorted(run["named"]) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_chain_on_the_host_equals_the_selection(run, case):
    slots, lists, got, store = run["named"][case]
    for r, s in enumerate(slots):
        assert_same(got[r], select(store[s], lists[r]), f"{case}: request {r}, slot {s}")


def test_the_cases_hit_what_they_are_there_for(run):
    n = run["named"]
    g = n["slots [2, 0]"][2]
    assert (g[0]["n_found"], g[0]["n_points"]) == (2, 13) and (g[1]["n_found"], g[1]["n_points"]) == (2, 70)   # X + Y of slot 2; A + X of slot 0
    g = n["shared cell named in one list only"][2]
    assert (g[0]["n_found"], g[0]["n_points"]) == (1, 64) and (g[1]["n_found"], g[1]["n_points"]) == (1, 9)
    g = n["R = 1, the run and the big cell"][2][0]
    assert (g["n_found"], g["n_points"]) == (71, 220) and np.diff(g["cstart"]).tolist() == [1] * 70 + [150]
    g = n["R = 3, boundary inside a group"][2]
    assert g[0]["n_points"] == 63 and g[1]["n_points"] == 0 and g[2]["n_points"] == len(n["R = 3, boundary inside a group"][3][2]["pts"])
    assert [n[k][2][0]["n_points"] for k in ("63 points", "64 points", "65 points")] == [63, 64, 65]
    assert [x["n_points"] for x in n["nothing found and an empty list"][2]] == [0, 0]
    assert n["empty map alone"][2][0]["n_found"] == 0
    g = n["edges of the index range"][2][0]
    assert (g["n_found"], g["n_points"]) == (2, 6) and sorted(map(tuple, unpack(g["ckey"]))) == sorted([EDGE_HI, EDGE_LO])
    slots, _, g, store = n["after a further append"]
    for r, s in enumerate(slots):        # every cell of every slot: the destination is the slot's map
        for k in ("pts", "pkey", "ckey", "cstart"):
            assert np.array_equal(g[r][k], store[s][k]), (s, k)
    assert len(store[1]["pts"]) == 13 and len(store[0]["ckey"]) == len(SLOT0) + 1


def test_the_store_is_unchanged_by_extractions(run):
    d = run["dumps"]
    assert len(d) == 4
    for a, b in ((d[0], d[1]), (d[2], d[3])):
        for s in range(S):
            for k in ("ckey", "cstart", "pts", "pkey"):
                assert np.array_equal(a[s][k], b[s][k]), (s, k)
    assert not np.array_equal(d[1][0]["cstart"], d[2][0]["cstart"])   # (the further append did change it)


def test_the_driver_runs_clean_under_the_sanitizers(exes, run):
    """the same driver as a stand-alone program built with -fsanitize=address,undefined, run as a program on the CPU"""
    pout = os.path.join(exes["dir"], "out_san.bin")
    p = subprocess.run([exes["san"], run["pin"], pout], capture_output=True, text=True)
    assert p.returncode == 0 and "ERROR" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-2000:]
    assert open(pout, "rb").read() == run["raw"]


# ---- declarations ------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name, n_args in (("ll_history_batch_extract_cells", 9), ("ll_history_batch_extract_work", 2)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl and name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert fn.restype is C.c_int32 and len(decl.group(1).split(",")) == len(fn.argtypes) == n_args, name
    from loam_livox_amd.api import Cell_map_slot, Full_map_slot, History_buffer_batch
    assert callable(History_buffer_batch.extract_cells) and callable(Cell_map_slot.extract_cells_into)
    assert Full_map_slot.extract_cells_into is Cell_map_slot.extract_cells_into
    from loam_livox_amd import build
    assert "ll_cellmap_batch_extract_kernels.hip" in build.SOURCES and "ll_cellmap_batch_extract_core.h" in build.HEADERS
    adapter = open(os.path.join(ROOT, "include", "loam_livox_adapter.hpp")).read()
    assert "ll_history_batch_extract_cells(" in adapter


def test_null_handles_are_refused_without_a_device():
    L = capi.load()
    n = (C.c_int64 * 1)(0)
    assert L.ll_history_batch_extract_cells(None, 2, 1, None, None, None, None, n, n) < 0
    assert b"ll_history_batch_extract_cells: null" in L.ll_last_error()
    assert L.ll_history_batch_extract_work(None, n) < 0
    assert b"ll_history_batch_extract_work: null" in L.ll_last_error()


# ---- Keyframe_assembly.materialize: prefetched, extract_cells, extract_cells_into, host ----------------------------------------------
class _Km:
    def __init__(self, *a, **k):
        self.args = a


def _assembly(full, monkeypatch):
    from loam_livox_amd import keyframes
    monkeypatch.setattr(keyframes, "Cell_map", _Km)
    ka = keyframes.Keyframe_assembly(full_cell_map=full)
    ka._cell_map_from_points = lambda xyz: ("host", xyz.copy())
    kf = keyframes.Maps_keyframe()
    kf.add_cells(np.array([[2, 0, 0], [9, 9, 9]]))
    return ka, kf


DUMP = (np.array([[1, 2, 3], [4, 5, 6]], np.float32), np.array([[0, 0, 0], [2, 0, 0]], np.int32), np.array([0, 1, 2], np.int32), np.zeros(2, np.int32))


def test_materialize_takes_its_routes_in_order(monkeypatch):
    calls = []

    class Both:
        def dump(self):
            calls.append("dump")
            return DUMP

        def extract_cells(self, want, km):
            calls.append(("extract_cells", sorted(map(tuple, np.asarray(want).tolist()))))

        def extract_cells_into(self, want, km):
            calls.append(("extract_cells_into", sorted(map(tuple, np.asarray(want).tolist()))))

    class Into:
        dump = Both.dump
        extract_cells_into = Both.extract_cells_into

    class Host:
        dump = Both.dump

    ka, kf = _assembly(Both(), monkeypatch)
    ready = object()
    ka.prefetch(kf, ready)
    assert ka.materialize(kf) is ready and calls == []                       # handed over in advance: nothing is read
    assert isinstance(ka.materialize(kf), _Km) and calls == [("extract_cells", [(2, 0, 0), (9, 9, 9)])]   # ... and consumed once
    other = type(kf)()
    other.add_cells(np.array([[2, 0, 0]]))
    ka.prefetch(other, ready)
    del calls[:]
    assert isinstance(ka.materialize(kf), _Km) and calls[0][0] == "extract_cells"   # a map handed over for another key frame is not this one's
    assert ka.materialize(other) is not ready and len(calls) == 2                  # ... and is dropped, not kept for later
    del calls[:]
    ka, kf = _assembly(Into(), monkeypatch)
    assert isinstance(ka.materialize(kf), _Km) and calls == [("extract_cells_into", [(2, 0, 0), (9, 9, 9)])]
    del calls[:]
    ka, kf = _assembly(Host(), monkeypatch)
    tag, xyz = ka.materialize(kf)
    assert tag == "host" and calls == ["dump"] and np.array_equal(xyz, [[4, 5, 6]])


# ---- Laser_mapping_batch._full_step against stubbed handles --------------------------------------------------------------------------
def test_full_step_extracts_once_per_round_between_the_adds_and_the_processing(monkeypatch):
    from loam_livox_amd import keyframes, mapping
    from loam_livox_amd.api import Full_map_slot
    events = []

    class Batch:
        n_sequences = 4
        _full_resolution, _full_min_points = 1.0, 3
        fail = False

        def append_full(self, fe, poses, active, min_points, lists=True):
            events.append("append_full")

        def full_touched(self, s, n=None):
            return np.array([[s, 0, 0], [s, 1, 0]], np.int32)

        def extract_cells(self, kind, sequences, cell_lists, dsts):
            lists = [sorted(map(tuple, np.asarray(c).tolist())) for c in cell_lists]
            events.append(("extract", kind, list(sequences), lists))
            if self.fail:
                raise RuntimeError("extraction failed")
            for d, c in zip(dsts, lists):
                d.cells = c           # what the destination now holds
            return [(len(c), 5) for c in cell_lists]

    def no_dump(self):
        raise AssertionError("Full_map_slot.dump called during _full_step")
    monkeypatch.setattr(Full_map_slot, "dump", no_dump)

    class Km:
        def __init__(self, *a, **k):
            self.max_points, self.cells = 1024, None
            made.append(self)

        def keyframe_images(self, *a):
            events.append("analyse")
            analysed.append(self.cells)
            return dict(images=np.zeros((4, 60, 60), np.float32), ratio_nonzero=np.zeros(4, np.float32), eigen_R=np.zeros((2, 3, 3), np.float32),
                        n_vectors=np.zeros(4, np.int32), centre=np.zeros(3, np.float32), roi_range=1.0)

        def dump(self):
            return (np.zeros((0, 3), np.float32),)

        def close(self):
            closed.append(self)
    analysed, made, closed = [], [], []
    monkeypatch.setattr(keyframes, "Cell_map", Km)
    lm = mapping.Laser_mapping_batch.__new__(mapping.Laser_mapping_batch)
    batch = Batch()
    lm.history_batch, lm.key_frames, lm.full_maps, lm.full_map_s, lm.fe = batch, True, True, 0.0, None
    lm.keyframes = [keyframes.Keyframe_assembly(full_cell_map=Full_map_slot(batch, s), scans_of_each_keyframe=2, scans_between_two_keyframe=1)
                    for s in range(4)]
    lm.loops, lm.map_refine = [[] for _ in range(4)], None
    lm.rounds = keyframes.Keyframe_rounds(lm.keyframes, store=batch)
    lm.frame_index = np.zeros(4, np.int32)
    for s in range(4):      # ("process": the slot's key frame goes through its pass, walk_front being the half the driver calls by name)
        real_add, real_proc = lm.keyframes[s].add_scan, lm.keyframes[s].walk_front
        lm.keyframes[s].add_scan = lambda *a, _f=real_add, _s=s: (events.append(("add_scan", _s)), _f(*a))[1]
        lm.keyframes[s].walk_front = lambda *a, _f=real_proc, _s=s, **k: (events.append(("process", _s)), _f(*a, **k))[1]
    pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    jobs = [(s, pose, pose) for s in (0, 2, 3)]
    on = np.array([True, False, True, True])
    for step in range(3):
        del events[:]
        lm.frame_index[[0, 2, 3]] += 1
        lm._full_step(jobs, on, np.tile(pose, (4, 1)))
        ex = [e for e in events if isinstance(e, tuple) and e[0] == "extract"]
        adds = [i for i, e in enumerate(events) if isinstance(e, tuple) and e[0] == "add_scan"]
        procs = [i for i, e in enumerate(events) if isinstance(e, tuple) and e[0] == "process"]
        assert events[0] == "append_full" and len(adds) == 3
        if step == 0:
            assert ex == [] and events.count("analyse") == 0        # no key frame has closed yet
            continue
        assert len(ex) == 1 and ex[0][1] == 2 and ex[0][2] == [0, 2, 3], events    # one batched extraction for the three closing slots
        assert ex[0][3][1] == [(2, 0, 0), (2, 1, 0)]
        i = events.index(ex[0])
        assert max(adds) < i < min(procs) and events.count("analyse") == 3
    # two key frames waiting in one slot: a round each, one key frame per slot and round, every one analysed on the map extracted for it
    extra = keyframes.Maps_keyframe()
    extra.add_cells(np.array([[7, 7, 7]]))
    extra.m_pose_q, extra.m_pose_t, extra.m_ending_frame_idx = pose[:4].copy(), pose[4:].copy(), 99
    del events[:], analysed[:]
    lm.frame_index[[0, 2, 3]] += 1
    real_add2 = lm.keyframes[2].add_scan
    lm.keyframes[2].add_scan = lambda *a: (real_add2(*a), lm.keyframes[2].m_keyframe_need_precession_list.appendleft(extra))[0]
    lm._full_step(jobs, on, np.tile(pose, (4, 1)))
    ex = [e for e in events if isinstance(e, tuple) and e[0] == "extract"]
    assert [e[2] for e in ex] == [[0, 2, 3], [2]], events
    assert ex[0][3][1] == [(7, 7, 7)] and ex[1][3][0] == [(2, 0, 0), (2, 1, 0)]          # slot 2: the older key frame first
    assert analysed == [ex[0][3][0], ex[0][3][1], ex[0][3][2], ex[1][3][0]]                # each analysed on the cells extracted for it
    assert [kf.m_ending_frame_idx for kf in lm.keyframes[2].keyframe_vec[-2:]][0] == 99 and not lm.keyframes[2].m_keyframe_need_precession_list
    second = events.index(ex[1])
    assert [e for e in events[second:] if isinstance(e, tuple) and e[0] == "process"] == [("process", 2)]
    # a failing extraction closes the destinations it made and leaves the key frames waiting
    lm.keyframes[2].add_scan = real_add2
    batch.fail = True
    del made[:], closed[:]
    lm.frame_index[[0, 2, 3]] += 1
    with pytest.raises(RuntimeError, match="extraction failed"):
        lm._full_step(jobs, on, np.tile(pose, (4, 1)))
    assert len(made) == 3 and closed == made and all(len(lm.keyframes[s].m_keyframe_need_precession_list) == 1 for s in (0, 2, 3))
