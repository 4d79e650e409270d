"""CPU tier of ll_cellmap_extract_cells (tests/test_gpu_cellmap_extract.py is the GPU tier): the entry point is declared, exported and
bound and refuses its arguments without a device; and the launch chain -- mark, scan, table, gather -- compiled for the CPU from the
kernel unit itself (tests/cellmap_extract_host.cpp on tests/cellmap_batch_shim) gives, bit for bit, what a numpy restatement of
Keyframe_assembly._materialize_host's selection takes out of the same map in dump form: the cells of the list that the map holds, in
key order, every cell's points in stored order, every point under the key it had."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES = 1.0
BOX = np.float32(0.5)    # the edge of a cell: set_resolution halves the resolution it is given
LIMIT = 1 << 20
# cells of exactly one point, of 65 (one more than a wavefront), 257 (one more than a block) and 1000 points; 1000 + 23 + 1 = 4 * 256
SIZES = [1, 1, 1, 65, 257, 1000, 23]
N_CELLS = 300


def geometry(seed=5):
    """(points [n, 3] in a shuffled insertion order, the cell index of every point): about 5000 points in 300 cells around the origin"""
    rng = np.random.default_rng(seed)
    ks = set()
    while len(ks) < N_CELLS:
        ks.add(tuple(int(v) for v in rng.integers(-12, 13, 3)))
    ks = np.array(sorted(ks), np.int64)[rng.permutation(N_CELLS)]
    sizes = np.array(SIZES + list(rng.integers(1, 25, N_CELLS - len(SIZES))), np.int64)
    cell = np.repeat(ks, sizes, axis=0)
    centre = cell.astype(np.float32) * BOX + BOX * np.float32(0.5)
    # flat patches well inside their cells: the cells with enough points are planes, so the key-frame images of the GPU tier are not empty
    pts = (centre + rng.uniform(-0.2, 0.2, cell.shape).astype(np.float32) * np.array([1, 1, 0.05], np.float32) * BOX).astype(np.float32)
    order = rng.permutation(len(pts))
    return pts[order], cell[order], ks, sizes


def pack(ijk):
    """the device's cell key (ll_cellmap_core.h cell_pack): ascending key = lexicographic (i, j, k)"""
    c = (np.asarray(ijk, np.int64).reshape(-1, 3) + LIMIT).astype(np.uint64)
    return (c[:, 0] << np.uint64(42)) | (c[:, 1] << np.uint64(21)) | c[:, 2]


def dump_form(pts, cell):
    """the store one append of the points to an empty map leaves: points ordered by (cell key, insertion order), the table beside them"""
    key = pack(cell)
    o = np.argsort(key, kind="stable")
    pkey = key[o]
    ckey, cstart = np.unique(pkey, return_index=True)
    xyzw = np.zeros((len(pts), 4), np.float32)
    xyzw[:, :3] = pts[o]
    return dict(pts=xyzw, pkey=pkey, ckey=ckey, cstart=np.r_[cstart, len(pkey)].astype(np.int32))


def select(src, want_ijk):
    """_materialize_host's selection on a map in dump form: isin over the packed cells, then the points of the selected cells, cell
    after cell.  An index beyond +-2^20 names no cell."""
    want = np.asarray(want_ijk, np.int64).reshape(-1, 3)
    want = want[(np.abs(want) < LIMIT).all(axis=1)]
    sel = np.flatnonzero(np.isin(src["ckey"], pack(want)))
    start = src["cstart"].astype(np.int64)
    lens = start[sel + 1] - start[sel]
    first = np.cumsum(lens) - lens
    idx = np.repeat(start[sel] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)
    return dict(pts=src["pts"][idx], pkey=src["pkey"][idx], ckey=src["ckey"][sel], cstart=np.r_[first, lens.sum()].astype(np.int32) if len(sel) else
                np.zeros(1, np.int32), n_found=len(sel), n_points=int(lens.sum()))


def unpack(ckey):
    k = np.asarray(ckey, np.uint64)
    m = np.uint64(0x1fffff)
    return np.stack([(k >> np.uint64(42)) & m, (k >> np.uint64(21)) & m, k & m], axis=1).astype(np.int64) - LIMIT


def absent_cells(n=10):
    return np.array([[40 + i, -3, 7] for i in range(n)], np.int64)   # (the geometry stays within +-12)


def lists(src, seed=11):
    """the cases of the issue, by name -> cell list [n, 3]"""
    rng = np.random.default_rng(seed)
    cells = unpack(src["ckey"])
    nc = len(cells)
    lens = np.diff(src["cstart"].astype(np.int64))
    half = cells[rng.permutation(nc)[:nc // 2]]
    by_len = lambda n: cells[np.flatnonzero(lens == n)[0]]
    out = {"random half": half, "first and last": cells[[0, nc - 1]], "every cell": cells[rng.permutation(nc)],
           "empty": np.zeros((0, 3), np.int64), "only absent": absent_cells(),
           "1024 points": np.stack([by_len(1000), by_len(23), by_len(1)]), "322 points": np.stack([by_len(257), by_len(65)])}
    for name in ("random half", "first and last", "every cell"):
        base = out[name]
        # two entries beyond +-2^20 which, packed without a range check, would alias cells of the map (one that the list does not name,
        # where there is one): i + 2^21 drops out of the 64 bits, k + 2^21 carries into j
        rest = np.array(sorted(set(map(tuple, cells)) - set(map(tuple, base))) or [tuple(cells[0])], np.int64)
        a, b = rest[0], rest[-1]
        beyond = np.array([[a[0] + (1 << 21), a[1], a[2]], [b[0], b[1] - 1, b[2] + (1 << 21)]], np.int64)
        mixed = np.concatenate([base, base, absent_cells(), beyond])
        out[name + ", doubled and polluted"] = mixed[rng.permutation(len(mixed))]
    return out


CASES = ["random half", "first and last", "every cell", "empty", "only absent", "random half, doubled and polluted",
         "first and last, doubled and polluted", "every cell, doubled and polluted", "1024 points", "322 points"]


@pytest.fixture(scope="module")
def source():
    pts, cell, _, _ = geometry()
    return dump_form(pts, cell)


def test_the_geometry_has_the_shapes_the_cases_need(source):
    lens = np.diff(source["cstart"])
    assert 4500 <= len(source["pts"]) <= 5500 and len(lens) == N_CELLS
    for n in (1, 65, 257, 1000):
        assert (lens == n).any()
    assert (unpack(source["ckey"]) < 0).any()
    ls = lists(source)
    assert sorted(ls) == sorted(CASES)
    assert select(source, ls["1024 points"])["n_points"] == 1024 and select(source, ls["322 points"])["n_points"] == 322
    assert select(source, ls["random half"])["n_points"] % 256 != 0
    assert select(source, ls["every cell"])["n_points"] == len(source["pts"])


def test_entry_point_is_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "ll_cellmap_extract_cells"
    decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\);", header)
    assert decl and name in capi.SYMBOLS
    fn = getattr(capi.load(), name)
    assert fn.restype is C.c_int32 and len(decl.group(1).split(",")) == len(fn.argtypes) == 6
    from loam_livox_amd.api import Cell_map, Cell_map_slot, Full_map_slot
    assert callable(Cell_map.extract_cells)
    assert not hasattr(Cell_map_slot, "extract_cells") and not hasattr(Full_map_slot, "extract_cells")  # they keep the dump route


def test_null_handles_are_refused_without_a_device():
    L = capi.load()
    n = C.c_int64(0)
    assert L.ll_cellmap_extract_cells(None, None, 0, None, C.byref(n), C.byref(n)) < 0
    assert b"ll_cellmap_extract_cells: null" in L.ll_last_error()


def test_materialize_takes_the_host_route_for_a_map_without_the_method():
    """test stubs and Full_map_slot: anything with dump() but no extract_cells goes through _materialize_host, as before"""
    from loam_livox_amd import keyframes

    class Full:
        def dump(self):
            return (np.array([[1, 2, 3], [4, 5, 6]], np.float32), np.array([[0, 0, 0], [2, 0, 0]], np.int32), np.array([0, 1, 2], np.int32),
                    np.zeros(2, np.int32))

    ka = keyframes.Keyframe_assembly(full_cell_map=Full())
    ka._cell_map_from_points = lambda xyz: ("built from", xyz.copy())
    kf = keyframes.Maps_keyframe()
    kf.add_cells(np.array([[2, 0, 0], [9, 9, 9]]))
    tag, xyz = ka.materialize(kf)
    assert tag == "built from" and np.array_equal(xyz, [[4, 5, 6]])
    cells = np.array([[-5, 0, 7], [1 << 19, -(1 << 20) + 1, 3]], np.int64)
    assert np.array_equal(keyframes._unpack_cells(keyframes._pack_cells(cells)), cells)


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cellmap_extract") / "cellmap_extract_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-x", "c++", "-I", os.path.join(ROOT, "tests", "cellmap_batch_shim"),
                           "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cellmap_extract_host.cpp")])
    return exe


def run_host(exe, tmp, src, want):
    want = np.ascontiguousarray(want, np.int32).reshape(-1, 3)
    buf = np.array([len(src["pts"]), len(src["ckey"]), len(want)], np.int32).tobytes()
    buf += src["pts"].tobytes() + src["pkey"].tobytes() + src["ckey"].tobytes() + src["cstart"].tobytes() + want.tobytes()
    pin, pout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    open(pin, "wb").write(buf)
    subprocess.check_call([exe, pin, pout])
    raw = open(pout, "rb").read()
    found, points, frame, m_cells, m_pts = np.frombuffer(raw, np.int32, 5)
    pos = 20

    def take(dtype, n):
        nonlocal pos
        a = np.frombuffer(raw, dtype, n, pos)
        pos += a.nbytes
        return a
    got = dict(n_found=int(found), n_points=int(points), frame=int(frame), mirrors=(int(m_cells), int(m_pts)), ckey=take(np.uint64, found),
               cstart=take(np.int32, found + 1), clast=take(np.int32, found), pts=take(np.float32, 4 * points).reshape(-1, 4),
               pkey=take(np.uint64, points))
    assert pos == len(raw)
    return got


def assert_same(got, want, what):
    assert (got["n_found"], got["n_points"]) == (want["n_found"], want["n_points"]), what
    assert got["mirrors"] == (want["n_found"], want["n_points"]), what
    assert got["frame"] == (2 if want["n_points"] else 0), what
    assert np.array_equal(got["ckey"], want["ckey"]), what
    assert np.array_equal(got["cstart"], want["cstart"]), what
    assert not got["clast"].any(), what
    assert np.array_equal(got["pts"].view(np.uint32), want["pts"].view(np.uint32)), what
    assert np.array_equal(got["pkey"], want["pkey"]), what


@pytest.mark.parametrize("case", CASES)
def test_chain_on_the_host_equals_the_selection(host_exe, tmp_path, source, case):
    want_list = lists(source)[case]
    want = select(source, want_list)
    got = run_host(host_exe, str(tmp_path), source, want_list)
    assert_same(got, want, case)
    if case.startswith("every cell"):
        for k in ("pts", "pkey", "ckey", "cstart"):
            assert np.array_equal(got[k], source[k]), k
    if case in ("empty", "only absent"):
        assert got["n_found"] == 0 and got["n_points"] == 0
    if case.endswith("polluted"):   # the same set as the clean list
        clean = select(source, lists(source)[case.split(",")[0]])
        assert (got["n_found"], got["n_points"]) == (clean["n_found"], clean["n_points"])


def test_a_key_is_copied_not_recomputed(host_exe, tmp_path, source):
    """a stored point that lies outside its cell's cube (a VoxelGrid centroid on a face, after down_sample_replace) stays in its cell"""
    src = {k: v.copy() for k, v in source.items()}
    c = int(np.flatnonzero(np.diff(src["cstart"]) == 65)[0])
    src["pts"][src["cstart"][c] + 3, :3] += np.float32(3.0) * BOX   # three cells away by its coordinates
    want_list = unpack(src["ckey"][[c]])
    got = run_host(host_exe, str(tmp_path), src, want_list)
    assert_same(got, select(src, want_list), "moved point")
    assert got["n_points"] == 65 and (got["pkey"] == src["ckey"][c]).all()


def test_an_empty_source(host_exe, tmp_path):
    src = dict(pts=np.zeros((0, 4), np.float32), pkey=np.zeros(0, np.uint64), ckey=np.zeros(0, np.uint64), cstart=np.zeros(1, np.int32))
    got = run_host(host_exe, str(tmp_path), src, [[0, 0, 0], [1, 2, 3]])
    assert (got["n_found"], got["n_points"], got["frame"], got["mirrors"]) == (0, 0, 0, (0, 0))
