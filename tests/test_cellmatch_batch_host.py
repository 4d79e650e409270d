"""CPU tier of the cell-mode refresh of the batched match buffer (tests/test_gpu_cellmatch_batch.py is the GPU tier): the entry points
are declared, exported, bound and in the adapter; null arguments are refused without a device; Laser_mapping_batch(cell_matching=True)
makes one add and one refresh_cells per step for exactly the accepted slots at their new poses and never calls refresh (against
stubbed device handles); and the chain itself -- the launch chains of ll_cellmap_batch_kernels.hip and ll_cellmatch_batch_kernels.hip
compiled for the CPU (tests/cellmatch_batch_host.cpp against tests/cellmap_batch_shim), whose decisions are the functions of
ll_cellmatch_batch_core.h -- equals the oracle's History.refresh_cells and the dump() of its CellMap after every step."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi, mapping
from oracle import orc
from oracle.orc_mapping import History
from tests.test_multimap_host import _Stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ll_history_batch_refresh_cells", "ll_history_batch_cell_match_work")


def test_entry_points_are_declared_exported_bound_and_in_the_adapter():
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
    from loam_livox_amd.api import History_buffer_batch
    for m in ("refresh_cells", "cell_match_work"):
        assert callable(getattr(History_buffer_batch, m))
    adapter = open(os.path.join(ROOT, "include", "loam_livox_adapter.hpp")).read()
    body = adapter[adapter.index("class History_batch"):adapter.index("class Points_cloud_map")]
    for name in NEW:
        assert name in body, name
    assert "void refresh_cells(" in body and "void cell_match_work(" in body
    from loam_livox_amd import build
    assert "ll_cellmatch_batch_kernels.hip" in build.SOURCES and "ll_cellmatch_batch_core.h" in build.HEADERS


def test_null_arguments_are_refused_without_a_device():
    L = capi.load()
    out = (C.c_int64 * 8)()
    maps = (C.c_void_p * 1)()
    poses = (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)
    assert L.ll_history_batch_refresh_cells(None, maps, None, poses, 1.0, 1.0, 30.0, 1, None, None) < 0
    assert b"ll_history_batch_refresh_cells: null" in L.ll_last_error()
    assert L.ll_history_batch_cell_match_work(None, out) < 0 and b"ll_history_batch_cell_match_work: null" in L.ll_last_error()


# ---- the loop's bookkeeping, device handles stubbed ---------------------------------------------------------------------------------------
@pytest.fixture
def stubbed(monkeypatch):
    st = _Stubs()
    outer = st

    class HistBatch:
        def __init__(self, n_sequences, *a, **kw):
            self.S = n_sequences
            self.frames = [0] * n_sequences

        def enable_cell_maps(self, initial_points_per_map, cell_resolution, threshold_cell_revisit):
            outer.log.append(("enable_cell_maps", initial_points_per_map, cell_resolution, threshold_cell_revisit))

        def sync_cell_maps(self):
            outer.log.append(("sync_cell_maps",))

        def add_voxel(self, vc, vs, poses, gate=None, active=None, t=0.0, a=0.0):
            on = [bool(x) for x in active]
            outer.log.append(("add_voxel", tuple(on)))
            for s in range(self.S):
                self.frames[s] += on[s]
            return np.array(on)

        def refresh(self, maps, active=None):
            outer.log.append(("refresh", tuple(bool(x) for x in active)))
            return np.array(self.frames), np.array(self.frames)

        def refresh_cells(self, maps, poses, active, rc, rs, fov, replace):
            on = tuple(bool(x) for x in active)
            assert tuple(m is not None for m in maps) == on  # a map for every accepted slot and for no other
            outer.log.append(("refresh_cells", on, np.array(poses, np.float64).copy(), (rc, rs, fov, replace)))
            return np.array(self.frames) * 10, np.array(self.frames) * 20

        def size(self, s):
            return min(self.frames[s], 5)

        def close(self):
            pass

    def no_single_handles(*a, **kw):
        raise AssertionError("the batched mode must not create per-sequence History_buffer handles")

    classes = dict(st.classes, History_buffer=no_single_handles, History_buffer_batch=HistBatch)
    for k, v in classes.items():
        monkeypatch.setattr(mapping, k, v)
    return st


def test_loop_makes_one_refresh_cells_per_step_at_the_new_poses_and_never_a_refresh(stubbed):
    st = stubbed
    st.reject.add((1, 4))  # sequence 1 is rejected at its frame 4
    lb = mapping.Laser_mapping_batch(3, batched_history=True, cell_maps=True, cell_matching=True, scan_points=100, init_accumulate_frames=2,
                                     maximum_search_range_corner=11.0, maximum_search_range_surface=12.0, maximum_in_fov_angle=33.0, down_sample_replace=0)
    assert lb.cell_matching is True
    scan = np.zeros((100, 4), np.float32)
    rejected = 0
    for step in range(7):
        st.log.clear()
        before = lb.poses.copy()
        out = lb.process_new_scans([scan, scan if step >= 1 else None, scan])
        adds = [e for e in st.log if e[0] == "add_voxel"]
        cells = [e for e in st.log if e[0] == "refresh_cells"]
        accepted = tuple(bool(out[s] == 1) for s in range(3))
        assert len(adds) == len(cells) == 1 and adds[0][1] == cells[0][1] == accepted
        assert not [e for e in st.log if e[0] in ("refresh", "sync_cell_maps", "enable_cell_maps")]
        assert [e[0] for e in st.log if e[0] in ("add_voxel", "refresh_cells")] == ["add_voxel", "refresh_cells"]  # the add first
        assert cells[0][3] == (11.0, 12.0, 33.0, 0)
        for s in range(3):
            if accepted[s]:  # the pose the step just accepted, which the loop keeps from here on
                assert np.array_equal(cells[0][2][s], lb.poses[s])
                assert lb.map_sizes[s] == (10 * lb.history_batch.frames[s], 20 * lb.history_batch.frames[s])
            else:
                assert np.array_equal(lb.poses[s], before[s])
        rejected += int(out[1] == 0)
        if step >= 4:  # past the accumulation frames a registered frame moves (the stub: by a metre), so the new pose is not the old one
            assert any(accepted[s] and not np.array_equal(cells[0][2][s], before[s]) for s in range(3))
    assert rejected == 1
    lb.close()
    # the defaults are Laser_mapping's
    st.log.clear()
    lb = mapping.Laser_mapping_batch(2, batched_history=True, cell_maps=True, cell_matching=True, scan_points=100)
    lb.process_new_scans([scan, scan])
    assert [e[3] for e in st.log if e[0] == "refresh_cells"] == [(100.0, 100.0, 30.0, 1)]
    lb.close()


def test_without_the_keyword_nothing_changes_and_the_refusals_stay(stubbed):
    st = stubbed
    scan = np.zeros((100, 4), np.float32)
    lb = mapping.Laser_mapping_batch(2, batched_history=True, cell_maps=True, scan_points=100)
    assert lb.cell_matching is False
    lb.process_new_scans([scan, scan])
    assert [e[0] for e in st.log if e[0] in ("refresh", "refresh_cells", "sync_cell_maps")] == ["refresh"]
    lb.close()
    with pytest.raises(ValueError, match="cell_maps"):
        mapping.Laser_mapping_batch(2, batched_history=True, cell_matching=True, scan_points=100)
    with pytest.raises(ValueError):
        mapping.Laser_mapping_batch(2, cell_matching=True, scan_points=100)
    with pytest.raises(ValueError, match="batched_history"):
        mapping.Laser_mapping_batch(2, cell_maps=True, cell_matching=True, scan_points=100)
    on = dict(batched_history=True, cell_maps=True, cell_matching=True)
    for kw in (dict(matching_mode=1), dict(keep_cell_maps=True), dict(lidar_type="velodyne"), dict(loop_closure_if_enable=1),
               dict(matching_mode=1, keep_cell_maps=True)):
        with pytest.raises(ValueError):
            mapping.Laser_mapping_batch(2, scan_points=100, **on, **kw)
    with pytest.raises(TypeError):
        mapping.Laser_mapping(scan_points=100, cell_matching=True)  # not an argument of Laser_mapping


# ---- the chain on the host ---------------------------------------------------------------------------------------------------------------
THR, CELL_RES, N_STEPS = 3, 2.0, 12          # cells of 1 m; a cell not hit for 3 appends is reset by the next hit
LEAF, RANGES, FOV = (0.25, 0.5), (3.5, 4.5), 70.0
IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
# per map: a cloud per step, "-" = the map sits the step out, "E" = an empty cloud
SCHEDULE = ["ABBBACABEACB",   # a revisit after three appends elsewhere (steps 0 - 4): cells reset between refreshes; an empty cloud
            "A---ABB-BAAC",   # sits out three steps, then the same cells again
            "CEAA-BCCCA-B"]


def clouds():
    rng = np.random.default_rng(11)
    A = np.zeros((300, 4), np.float32)
    A[:, :3] = rng.uniform(-4.0, 4.0, (300, 3))
    B = A.copy()
    B[:, 1] += np.float32(5.0)
    Cc = A.copy()
    Cc[:, :3] += np.float32(0.17)
    return dict(A=A, B=B, C=Cc, E=np.zeros((0, 4), np.float32))


def view_pose(m, t):
    a = np.deg2rad(35.0 * t + 50.0 * m)
    return np.array([0, 0, np.sin(a / 2), np.cos(a / 2), 0.3 * t - 1.0, 0.5 * m, 0.1], np.float64)


def filtered(cloud, kind):
    """the frame as History.add hands it to the cell map (identity pose)"""
    if len(cloud) == 0:
        return np.zeros((0, 4), np.float32)
    return orc.voxel_grid(orc.cloud_transform(IDENT, cloud), LEAF[kind])[1]


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cellmatch_batch") / "cellmatch_batch_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "tests", "cellmap_batch_shim"),
                           "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cellmatch_batch_host.cpp")])
    return exe


def run_host(exe, tmp, replace, reads):
    cl = clouds()
    buf = np.array([3, N_STEPS, THR, replace], np.int32).tobytes() + np.array([CELL_RES, *LEAF, *RANGES, FOV], np.float32).tobytes()
    for t in range(N_STEPS):
        buf += np.int32(reads[t]).tobytes()
        for kind in (0, 1):
            for m in range(3):
                c = SCHEDULE[m][t]
                w = None if c == "-" else filtered(cl[c], kind)
                assert w is None or len(w) <= 400
                buf += np.int32(-1).tobytes() if w is None else np.int32(len(w)).tobytes() + np.ascontiguousarray(w[:, :3], np.float32).tobytes()
        for m in range(3):
            buf += view_pose(m, t).tobytes()
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(pin, "wb").write(buf)
    subprocess.check_call([exe, pin, pout])
    raw = np.fromfile(pout, np.int32)
    pos, cats, dumps, counts = 0, {}, {}, []
    for t in range(N_STEPS):
        row = []
        for kind in (0, 1):
            row += [int(raw[pos]), int(raw[pos + 1])]
            pos += 2
            for m in range(3):
                n = raw[pos]
                cats[(t, kind, m)] = raw[pos + 1:pos + 1 + 3 * n].reshape(n, 3)  # (bits)
                pos += 1 + 3 * n
        counts.append(tuple(row) + (int(raw[pos]),))
        pos += 1
        if not reads[t]:
            continue
        for kind in (0, 1):
            for m in range(3):
                frame, nc, npts = raw[pos:pos + 3]
                pos += 3
                ijk = raw[pos:pos + 3 * nc].reshape(nc, 3)
                pos += 3 * nc
                start = raw[pos:pos + nc + 1]
                pos += nc + 1
                last = raw[pos:pos + nc]
                pos += nc
                pts = raw[pos:pos + 3 * npts].reshape(npts, 3)
                pos += 3 * npts
                dumps[(t, kind, m)] = (int(frame), ijk, start, last, pts)
    assert pos + 1 == len(raw)
    return cats, dumps, counts, int(raw[pos])


_oracle = {}


def oracle_run(replace):
    """per step and map: the concatenation of the per-cell filters, History.refresh_cells' two buffers, the CellMap dumps; computed once"""
    if replace in _oracle:
        return _oracle[replace]
    cl = clouds()
    hist = []
    for _ in range(3):
        h = History(5, *LEAF)
        h.enable_cell_map(CELL_RES, THR)
        hist.append(h)
    cats, bufs, dumps, sel = {}, {}, {}, []
    for t in range(N_STEPS):
        for m in range(3):
            c = SCHEDULE[m][t]
            if c != "-":
                hist[m].add(cl[c], cl[c], IDENT)
                shadow = copy.deepcopy(hist[m].cells)
                for kind in (0, 1):
                    cat, keys = shadow[kind].query_filter(view_pose(m, t), RANGES[kind], FOV, LEAF[kind], replace)
                    cats[(t, kind, m)] = np.ascontiguousarray(cat[:, :3], np.float32).view(np.int32).reshape(-1, 3)
                    sel.append((len(keys), len(shadow[kind].cells)))
                bufs[(t, m)] = hist[m].refresh_cells(view_pose(m, t), RANGES, FOV, replace)
            else:
                for kind in (0, 1):
                    cats[(t, kind, m)] = np.zeros((0, 3), np.int32)
            for kind in (0, 1):
                xyz, ijk, start, last = hist[m].cells[kind].dump()
                dumps[(t, kind, m)] = (hist[m].cells[kind].frame, ijk, start, last, np.ascontiguousarray(xyz, np.float32).view(np.int32).reshape(-1, 3),
                                       hist[m].cells[kind].n_points())
    _oracle[replace] = (cats, bufs, dumps, sel)
    return _oracle[replace]


def assert_step(got_cats, got_dumps, want, t, tag):
    cats, bufs, dumps, _ = want
    for kind in (0, 1):
        for m in range(3):
            g, w = got_cats[(t, kind, m)], cats[(t, kind, m)]
            assert g.shape == w.shape and np.array_equal(g, w), (tag, t, kind, m, "concatenation of the per-cell filters")
            if (t, m) in bufs and len(g):  # History.refresh_cells: the VoxelGrid over the concatenation (laser_mapping.hpp:533-537)
                cloud = np.concatenate([g.view(np.float32), np.zeros((len(g), 1), np.float32)], 1)
                got_buf = orc.voxel_grid(cloud, LEAF[kind])[1]
                assert np.array_equal(got_buf.view(np.int32), bufs[(t, m)][kind].view(np.int32)), (tag, t, kind, m, "refresh_cells")
            if (t, kind, m) in got_dumps:
                gd, wd = got_dumps[(t, kind, m)], dumps[(t, kind, m)]
                assert gd[0] == wd[0], (tag, t, kind, m, "frame counter")
                for i, what in ((1, "cell indices"), (2, "cell_start"), (3, "stamps"), (4, "points in order")):
                    assert gd[i].shape == wd[i].shape and np.array_equal(gd[i], wd[i]), (tag, t, kind, m, what)


@pytest.mark.parametrize("replace", [1, 0])
def test_chain_on_the_host_equals_the_oracle_after_every_step(host_exe, tmp_path, replace):
    want = oracle_run(replace)
    sel = want[3]
    # what the parameters are there for, on the oracle: most queries select some cells and not all of them
    assert sum(0 < a < b for a, b in sel) >= len(sel) * 3 // 4 and all(b > 0 for _, b in sel)
    if replace:  # ... and cells are reset between refreshes: map 0's surface store at step 4 is smaller than the five appends put in
        no_reset = History(5, *LEAF)
        no_reset.enable_cell_map(CELL_RES, 1 << 30)
        cl = clouds()
        for t in range(5):
            no_reset.add(cl[SCHEDULE[0][t]], cl[SCHEDULE[0][t]], IDENT)
            no_reset.refresh_cells(view_pose(0, t), RANGES, FOV, replace)
        assert want[2][(4, 1, 0)][5] < no_reset.cells[1].n_points()
    cats, dumps, counts, compactions = run_host(host_exe, str(tmp_path), replace, [1] * N_STEPS)
    assert len(dumps) == N_STEPS * 6
    for t in range(N_STEPS):
        assert_step(cats, dumps, want, t, "read after every step")
    # the same steps with the stores put in order three times only: leaves and new frames land behind a log that holds dead entries
    reads = [int(t in (3, 7, 11)) for t in range(N_STEPS)]
    cats, dumps, counts, compactions = run_host(host_exe, str(tmp_path), replace, reads)
    assert sorted({k[0] for k in dumps}) == [3, 7, 11]
    for t in range(N_STEPS):
        assert_step(cats, dumps, want, t, "three reads")
    # the bound: after every refresh the dead entries do not outnumber the live ones, or the handle compacts
    for log_c, live_c, log_s, live_s, compacted in counts:
        assert live_c <= log_c and live_s <= log_s
        assert compacted or (log_c <= 2 * live_c and log_s <= 2 * live_s), counts
    print("log / live per step:", counts, "compactions", compactions)
    # ... and with no read before the last step the handle's own rule is what keeps the log short
    cats, dumps, counts, compactions = run_host(host_exe, str(tmp_path), replace, [int(t == N_STEPS - 1) for t in range(N_STEPS)])
    for t in range(N_STEPS):
        assert_step(cats, dumps, want, t, "one read")
    for log_c, live_c, log_s, live_s, compacted in counts:
        assert compacted or (log_c <= 2 * live_c and log_s <= 2 * live_s), counts
    print("log / live per step, one read:", counts, "compactions", compactions)
    if replace:
        assert compactions >= 1, "the replace leaves dead entries: the rule must have fired"
