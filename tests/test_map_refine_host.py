"""CPU tier of the key-frame map refinement (tests/test_gpu_map_refine.py is the GPU tier).

Symbols: the entry points are declared, exported and bound and refuse null handles and bad arguments without a device; every argument
check of a run is the host function mr_plan (loam_livox_amd/csrc/ll_map_refine.h), driven here by tests/map_refine_host.cpp.
Affine and move: ll_map_refine_affine and mr_move give, bit for bit, what the reference's own refine_pts text gives (extracted at test
time, compiled against oracle/ref_stubs/ll_stub_eigen.h; skipped where the reference is absent) and what the numpy restatement of
tests/map_refine_inputs.py gives -- the restatement the GPU tier uses.
Chain: the per-point and per-voxel text of ll_map_refine_core.h, run on the CPU by the driver over the plan the C ABI makes, gives in
both modes and for merge the oracle's VoxelGrid composed with the numpy move, on the ragged set of clouds -- and on the sets the GPU
tier runs where the device chain changes form (mi.many_selections, mi.last_voxel_at_the_end): the host loop has no trips, wavefronts or
sort widths, so what this tier shows of them is that the expected values and the conditions the GPU tier asserts on them hold, and that
the shared core text agrees with the oracle on selections of finite and non-finite rows."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import api, capi
from tests import map_refine_inputs as mi
from tests.map_refine_inputs import bits
from tests.verbatim_build import REF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_HPP = os.path.join(REF, "source", "ceres_pose_graph_3d.hpp")
N_PAIRS, N_PTS = 1200, 8


def build_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "map_refine_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("map_refine") / "map_refine_host"))


def run_chain(exe, tmp, mode, leaf, clouds, ids, ori, opm):
    """-> (offsets, status, [cloud per selection]) of the driver's chain over a store of `clouds`"""
    pin, pout = os.path.join(tmp, "mr_in.bin"), os.path.join(tmp, "mr_out.bin")
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
    with open(pin, "wb") as f:
        f.write(np.int32(mode).tobytes() + np.float32(leaf).tobytes() + np.int32(len(clouds)).tobytes() + off.tobytes())
        for c in clouds:
            f.write(np.ascontiguousarray(c, np.float32).tobytes())
        f.write(np.int32(len(ids)).tobytes() + np.asarray(ids, np.int64).tobytes())
        f.write(np.ascontiguousarray(ori, np.float64).tobytes() + np.ascontiguousarray(opm, np.float64).tobytes())
    done = subprocess.run([exe, "chain", pin, pout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors="replace")
    raw = open(pout, "rb").read()
    n = len(ids)
    offsets = np.frombuffer(raw, np.int64, n + 1)
    status = np.frombuffer(raw, np.int32, n, 8 * (n + 1))
    pts = np.frombuffer(raw, np.float32, offset=8 * (n + 1) + 4 * n).reshape(-1, 4)
    assert len(pts) == offsets[-1]
    return offsets, status, [pts[offsets[s]:offsets[s + 1]] for s in range(n)]


# ------------------------------------------------------------------------------------------------ affine and move
def pose_pairs():
    """N_PAIRS seeded pose pairs: unit quaternions, quaternions of norm 1 +- 1e-6, translations up to 50 km out; points around the original pose"""
    rng = np.random.default_rng(2024)
    ori, opm = mi.poses(N_PAIRS, 17)
    scale = np.ones(N_PAIRS)
    scale[::3] = 1.0 + 1e-6
    scale[1::3] = 1.0 - 1e-6
    ori[:, :4] *= scale[:, None]
    opm[:, :4] *= scale[::-1, None]
    far = rng.uniform(-50000.0, 50000.0, (N_PAIRS, 3))
    far[: N_PAIRS // 4] = 0.0
    far[N_PAIRS // 4: N_PAIRS // 2] = np.array([50000.0, -50000.0, 50000.0])
    ori[:, 4:] += far
    opm[:, 4:] += far
    pts = (ori[:, None, 4:] + rng.uniform(-60, 60, (N_PAIRS, N_PTS, 3))).astype(np.float32)
    return ori, opm, pts


def affine_records(exe, args, tmp, ori, opm, pts):
    pin, pout = os.path.join(tmp, "aff_in.bin"), os.path.join(tmp, "aff_out.bin")
    with open(pin, "wb") as f:
        f.write(np.int32(len(ori)).tobytes() + np.int32(pts.shape[1]).tobytes())
        for a, b, p in zip(ori, opm, pts):
            f.write(a.tobytes() + b.tobytes() + np.ascontiguousarray(p, np.float32).tobytes())
    done = subprocess.run([exe, *args, pin, pout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors="replace")
    rec = np.fromfile(pout, np.float32).reshape(len(ori), 12 + 3 * pts.shape[1])
    return rec[:, :9].reshape(-1, 3, 3), rec[:, 9:12], rec[:, 12:].reshape(len(ori), -1, 3)


@pytest.fixture(scope="module")
def affine_results(driver, tmp_path_factory):
    ori, opm, pts = pose_pairs()
    return (ori, opm, pts) + affine_records(driver, ["affine"], str(tmp_path_factory.mktemp("map_refine_affine")), ori, opm, pts)


def test_affine_and_move_equal_the_numpy_restatement(affine_results):
    ori, opm, pts, R, T, moved = affine_results
    assert len(ori) >= 1000
    for k in range(len(ori)):
        Rn, Tn = mi.affine_np(ori[k], opm[k])
        assert np.array_equal(bits(R[k]), bits(Rn)) and np.array_equal(bits(T[k]), bits(Tn)), k
        assert np.array_equal(bits(moved[k]), bits(mi.move_np(Rn, Tn, pts[k])[:, :3])), k
    assert np.abs(ori[:, 4:]).max() > 4.9e4 and np.isfinite(moved).all()


def test_the_c_abi_affine_is_the_drivers(affine_results):
    ori, opm, _, R, T, _ = affine_results
    for k in range(0, len(ori), 7):
        Ra, Ta = api.map_refine_affine(ori[k], opm[k])
        assert np.array_equal(bits(Ra), bits(R[k])) and np.array_equal(bits(Ta), bits(T[k])), k
    L = capi.load()
    bad = ori[0].copy()
    bad[5] = np.inf
    out9, out3 = np.zeros(9, np.float32), np.zeros(3, np.float32)
    assert L.ll_map_refine_affine(capi.ptr(bad), capi.ptr(opm[0]), capi.ptr(out9), capi.ptr(out3)) < 0 and b"a pose is not finite" in L.ll_last_error()
    assert L.ll_map_refine_affine(None, capi.ptr(opm[0]), capi.ptr(out9), capi.ptr(out3)) < 0 and b"ll_map_refine_affine: null" in L.ll_last_error()
    assert not out9.any() and not out3.any()


REF_HARNESS = """
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ll_stub_eigen.h"
struct Ref {
%s
};
int main( int argc, char **argv )
{
    FILE *f = fopen( argv[ 1 ], "rb" ), *g = fopen( argv[ 2 ], "wb" );
    int n_pairs = 0, n_pts = 0;
    if ( !f || !g || fread( &n_pairs, 4, 1, f ) != 1 || fread( &n_pts, 4, 1, f ) != 1 ) return 2;
    for ( int p = 0; p < n_pairs; p++ )
    {
        double ori[ 7 ], opm[ 7 ];
        std::vector< float > pts( 3 * n_pts );
        if ( fread( ori, 8, 7, f ) != 7 || fread( opm, 8, 7, f ) != 7 || fread( pts.data(), 4, pts.size(), f ) != pts.size() ) return 2;
        Eigen::Quaterniond q_ori( ori[ 3 ], ori[ 0 ], ori[ 1 ], ori[ 2 ] ), q_opm( opm[ 3 ], opm[ 0 ], opm[ 1 ], opm[ 2 ] );
        Eigen::Matrix< double, 3, 1 > t_ori( ori[ 4 ], ori[ 5 ], ori[ 6 ] ), t_opm( opm[ 4 ], opm[ 5 ], opm[ 6 ] );
        std::vector< Eigen::Matrix< float, 3, 1 > > raw( n_pts ), unit( 4 );
        for ( int i = 0; i < n_pts; i++ ) raw[ i ] = Eigen::Matrix< float, 3, 1 >( pts[ 3 * i ], pts[ 3 * i + 1 ], pts[ 3 * i + 2 ] );
        // R_aff and T_aff are locals of refine_pts: they are read off the images of the origin and of the unit vectors, which the
        // float operations give exactly where a row of R_aff times a unit vector leaves one term -- so they are recomputed here by the
        // same two expressions, and the text itself gives the moved points
        const Eigen::Matrix< double, 3, 3 > R_mat_ori = q_ori.toRotationMatrix(), R_mat_opm = q_opm.toRotationMatrix();
        Eigen::Matrix< float, 3, 3 > R_aff = ( R_mat_opm * R_mat_ori.transpose() ).template cast< float >();
        Eigen::Matrix< float, 3, 1 > T_aff = ( R_aff.template cast< double >() * ( -t_ori ) + t_opm ).template cast< float >();
        std::vector< Eigen::Matrix< float, 3, 1 > > out = Ref::refine_pts( raw, R_mat_ori, t_ori, R_mat_opm, t_opm );
        for ( int r = 0; r < 3; r++ )
            for ( int c = 0; c < 3; c++ )
            {
                const float v = R_aff( r, c );
                fwrite( &v, 4, 1, g );
            }
        for ( int r = 0; r < 3; r++ )
        {
            const float v = T_aff( r );
            fwrite( &v, 4, 1, g );
        }
        for ( int i = 0; i < n_pts; i++ )
            for ( int r = 0; r < 3; r++ )
            {
                const float v = out[ i ]( r );
                fwrite( &v, 4, 1, g );
            }
    }
    fclose( f );
    fclose( g );
    return 0;
}
"""


def test_affine_and_move_equal_the_reference_text(affine_results, tmp_path):
    if not os.path.exists(REF_HPP):
        pytest.skip("the reference is not on this machine")
    lines = open(REF_HPP).read().split("\n")[436:452]                 # :437-452, refine_pts
    assert "static std::vector< Eigen::Matrix< T, 3, 1 > > refine_pts" in lines[1] and lines[-1].strip() == "}"
    src, exe = str(tmp_path / "refine_pts_ref.cpp"), str(tmp_path / "refine_pts_ref")
    with open(src, "w") as f:
        f.write(REF_HARNESS % "\n".join(lines))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "oracle", "ref_stubs"), "-o", exe, src])
    ori, opm, pts, R, T, moved = affine_results
    Rr, Tr, mr = affine_records(exe, [], str(tmp_path), ori, opm, pts)
    assert np.array_equal(bits(Rr), bits(R)) and np.array_equal(bits(Tr), bits(T))
    assert np.array_equal(bits(mr), bits(moved))
    # the moved points pin R_aff and T_aff of the text itself: the origin's image is T_aff, a unit vector's image is a column plus T_aff
    probe = np.zeros((len(ori), 4, 3), np.float32)
    probe[:, 1:] = np.eye(3, dtype=np.float32)
    _, _, img = affine_records(exe, [], str(tmp_path), ori, opm, probe)
    assert np.array_equal(bits(img[:, 0]), bits(T + np.float32(0.0)))
    for c in range(3):
        assert np.array_equal(bits(img[:, 1 + c]), bits((R[:, :, c] + np.float32(0.0)) + T)), c


# ------------------------------------------------------------------------------------------------ the chain on the CPU
@pytest.fixture(scope="module")
def ragged():
    """(names, stored clouds, selection ids, poses): every cloud once in a scrambled order, some twice"""
    raw = mi.raw_clouds()
    stored = [c for _, c in mi.stored_clouds(raw)]
    ids = list(np.random.default_rng(3).permutation(len(stored))) + [10, 3, 11, 11]
    ori, opm = mi.poses(len(ids), 23)
    return [n for n, _, _ in raw], stored, ids, ori, opm


@pytest.fixture(scope="module")
def chain_runs(driver, ragged, tmp_path_factory):
    """mode -> the driver's (offsets, status, clouds): computed once, shared, not changed"""
    _, stored, ids, ori, opm = ragged
    tmp = str(tmp_path_factory.mktemp("map_refine_chain"))
    return {mode: run_chain(driver, tmp, mode, mi.RUN_LEAF, stored, ids, ori, opm) for mode in (0, 1)}


@pytest.mark.parametrize("mode", [0, 1])
def test_chain_equals_the_oracle_composed_with_the_move(ragged, chain_runs, mode):
    names, stored, ids, ori, opm = ragged
    offsets, status, clouds = chain_runs[mode]
    seen = set()
    for s, cid in enumerate(ids):
        st, want = mi.expected(stored[cid], ori[s], opm[s], mi.RUN_LEAF, transform_first=bool(mode))
        assert status[s] == st and clouds[s].shape == want.shape, (names[cid], s)
        assert np.array_equal(bits(clouds[s]), bits(want)), (names[cid], s)
        assert not clouds[s][:, 3].any()
        seen.add(st)
    assert seen == {0, 1, 2} and offsets[0] == 0 and np.all(np.diff(offsets) == [len(c) for c in clouds])
    one = names.index("one_voxel")
    if mode == 0:                                                      # the 3000 points of one voxel came out as one point
        assert len(clouds[ids.index(one)]) <= 501 and len(stored[one]) == 3500


def test_merge_equals_the_oracle_over_the_concatenated_outputs(driver, chain_runs, tmp_path):
    for mode in (0, 1):
        flat = np.concatenate(chain_runs[mode][2])
        _, status, clouds = run_chain(driver, str(tmp_path), 2, mi.RUN_LEAF, [flat], [0], np.zeros((1, 7)), np.zeros((1, 7)))
        st, want = mi.filtered(flat, mi.RUN_LEAF)
        # (the 300 m and 700 m cubes are in: the merged extent passes 2^31 leaves, the filter hands the cloud back -- so the small one too)
        assert status[0] == st and np.array_equal(bits(clouds[0]), bits(want))
        small = np.concatenate([c for c in chain_runs[mode][2] if len(c) and np.abs(c[:, :3]).max() < 100.0])
        _, status, clouds = run_chain(driver, str(tmp_path), 2, mi.RUN_LEAF, [small], [0], np.zeros((1, 7)), np.zeros((1, 7)))
        st, want = mi.filtered(small, mi.RUN_LEAF)
        assert status[0] == st == 0 and 0 < len(want) < len(small) and np.array_equal(bits(clouds[0]), bits(want))


def test_a_selections_output_does_not_depend_on_its_slot(driver, ragged, chain_runs, tmp_path):
    _, stored, ids, ori, opm = ragged
    s = ids.index(10)
    for mode in (0, 1):
        _, status, clouds = run_chain(driver, str(tmp_path), mode, mi.RUN_LEAF, stored, [10], ori[s:s + 1], opm[s:s + 1])
        assert status[0] == chain_runs[mode][1][s] and np.array_equal(bits(clouds[0]), bits(chain_runs[mode][2][s]))


def test_driver_runs_clean_under_the_sanitizers(tmp_path, ragged, chain_runs):
    _, stored, ids, ori, opm = ragged
    exe = build_driver(str(tmp_path / "map_refine_host_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    for mode in (0, 1):
        _, status, clouds = run_chain(exe, str(tmp_path), mode, mi.RUN_LEAF, stored, ids, ori, opm)   # (asserts exit status 0, empty stderr)
        assert np.array_equal(status, chain_runs[mode][1])
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(clouds, chain_runs[mode][2]))


# ------------------------------------------------------------------------------------------------ the sets of the GPU tier's form changes
@pytest.fixture(scope="module")
def many():
    """mi.many_selections and the oracle's results in both modes: made once, shared, not changed"""
    store, ids, ori, opm = mi.many_selections(83)
    return store, ids, ori, opm, mi.expected_run(store, ids, ori, opm)


def chain_equals(driver, tmp, store, ids, ori, opm, want):
    for mode in (0, 1):
        offsets, status, clouds = run_chain(driver, tmp, mode, mi.RUN_LEAF, store, ids, ori, opm)
        assert offsets[-1] == sum(len(c) for _, c in want[bool(mode)])
        for s, (st, cloud) in enumerate(want[bool(mode)]):
            assert status[s] == st and clouds[s].shape == cloud.shape and np.array_equal(bits(clouds[s]), bits(cloud)), (mode, s, ids[s])


def test_many_selections_hold_what_the_gpu_tier_rests_on(many):
    store, ids, _, _, want = many
    for tf in (False, True):
        figures = mi.many_conditions(store, ids, want[tf])
        assert figures["points"] > figures["valid"] > 20000, figures
    # the sizes the set was built for: tiny clouds, several of 1-3 points, every fifth with finite and non-finite rows
    tiny = store[:mi.N_TINY]
    assert all(1 <= len(c) <= 70 for c in tiny) and sorted(len(tiny[k]) for k in mi.TINY_FEW) == [1, 1, 2, 2, 3, 3]
    assert all((0 < mi.finite_count(c) < len(c)) == (k % 5 == 0) for k, c in enumerate(tiny))
    assert [len(store[ids[s]]) for s in mi.MANY_FEW_AT] == [1, 2, 3, 1, 2, 3] * 2 + [1, 2, 3, 1]
    mi.packed_voxel_is_one_point(store)


def test_chain_equals_the_oracle_on_many_selections(driver, many, tmp_path):
    store, ids, ori, opm, want = many
    chain_equals(driver, str(tmp_path), store, ids, ori, opm, want)


@pytest.mark.parametrize("cnt", [1, 7, 8, 9, 16])
def test_chain_equals_the_oracle_where_the_last_voxel_ends_the_keys(driver, tmp_path, cnt):
    store = mi.last_voxel_at_the_end(cnt)
    assert all(mi.finite_count(c) == len(c) > 0 for c in store)
    for ori, opm in (mi.poses(2, 89), (np.stack([mi.IDENTITY] * 2),) * 2):
        want = mi.expected_run(store, [0, 1], ori, opm)
        assert all(st == 0 for tf in want for st, _ in want[tf])        # nothing is empty or handed back: no sentinel in the chain
        chain_equals(driver, str(tmp_path), store, [0, 1], ori, opm, want)
    for tf in (False, True):                                            # (the identity pair's results) the last row is the packed voxel
        last = want[tf][1][1][-1:]
        assert mi.in_voxel(store[1], mi.LAST_VOXEL_AT).sum() == cnt and mi.in_voxel(last, mi.LAST_VOXEL_AT).all()
        assert np.array_equal(bits(last[:, :3]), bits(mi.filtered(store[1][mi.in_voxel(store[1], mi.LAST_VOXEL_AT)], mi.RUN_LEAF)[1][:, :3]))


# ------------------------------------------------------------------------------------------------ refusals
def test_the_plan_refuses_bad_calls(driver):
    out = subprocess.run([driver, "refusals"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60, check=True).stdout.decode()
    got = dict(line.split(": ", 1) for line in out.strip().split("\n"))
    assert got["accepted"] == "" and got["plan"] == "12 points, 3 selections, 2 work items" and got["untouched"] == "1"
    want = {"mode": "mode must be", "mode_negative": "mode must be", "negative_count": "negative count", "too_many": "at most 2^20 selections",
            "null_ids": "null argument", "null_ori": "null argument", "null_opm": "null argument", "id_low": "id out of range",
            "id_high": "id out of range", "leaf_zero": "positive and finite", "leaf_negative": "positive and finite",
            "leaf_inf": "positive and finite", "leaf_nan": "positive and finite", "pose_nan": "a pose is not finite",
            "pose_inf": "a pose is not finite", "capacity": "fewer than 2^31 points"}
    for name, text in want.items():
        assert text in got[name], name


NEW = {"ll_map_refine_create": 3, "ll_map_refine_destroy": 1, "ll_map_refine_add_cloud": 7, "ll_map_refine_add_stored": 4, "ll_map_refine_size": 1, "ll_map_refine_cloud": 5,
       "ll_map_refine_affine": 4, "ll_map_refine_run": 9, "ll_map_refine_fetch": 3, "ll_map_refine_merge": 4, "ll_map_refine_fetch_merged": 3,
       "ll_map_refine_work": 2}


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name, n_args in NEW.items():
        decl = re.search(r"\b(int|void|int64_t)\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl and name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert len(decl.group(2).split(",")) == len(fn.argtypes) == n_args, name
        assert fn.restype is {"int": C.c_int32, "void": None, "int64_t": C.c_int64}[decl.group(1)], name
    for method in ("add_cloud", "add_stored", "cloud", "refine", "merge", "work", "close"):
        assert callable(getattr(api.Map_refine, method)), method


def test_null_handles_and_bad_arguments_are_refused_without_a_device():
    L = capi.load()
    h, cid, n = C.c_void_p(), C.c_int64(-7), C.c_int64(-7)
    pts, ids, pose = np.zeros((4, 4), np.float32), np.zeros(1, np.int64), np.array([[0, 0, 0, 1, 0, 0, 0]], np.float64)
    offs, st, work = np.full(2, -7, np.int64), np.full(1, -7, np.int32), np.zeros(4, np.int64)
    assert L.ll_map_refine_create(0, 1024, None) < 0 and b"ll_map_refine_create: null" in L.ll_last_error()
    assert L.ll_map_refine_create(0, 0, C.byref(h)) < 0 and b"initial_points out of range" in L.ll_last_error() and not h.value
    assert L.ll_map_refine_create(0, 1 << 31, C.byref(h)) < 0 and b"would pass 2^31 points" in L.ll_last_error() and not h.value
    assert L.ll_map_refine_add_cloud(None, capi.ptr(pts), 4, 0.5, C.byref(cid), C.byref(n), None) < 0
    assert b"ll_map_refine_add_cloud: null" in L.ll_last_error() and cid.value == -7 and n.value == -7
    assert L.ll_map_refine_add_stored(None, capi.ptr(pts), 4, C.byref(cid)) < 0
    assert b"ll_map_refine_add_stored: null" in L.ll_last_error() and cid.value == -7
    assert L.ll_map_refine_size(None) < 0 and b"ll_map_refine_size: null" in L.ll_last_error()
    assert L.ll_map_refine_cloud(None, 0, capi.ptr(pts), 4, C.byref(n)) < 0 and b"ll_map_refine_cloud: null" in L.ll_last_error() and n.value == -7
    assert L.ll_map_refine_run(None, 0, 1, capi.ptr(ids), capi.ptr(pose), capi.ptr(pose), 0.2, capi.ptr(offs), capi.ptr(st)) < 0
    assert b"ll_map_refine_run: null" in L.ll_last_error() and (offs == -7).all() and st[0] == -7
    assert L.ll_map_refine_fetch(None, capi.ptr(pts), 4) < 0 and b"ll_map_refine_fetch: null" in L.ll_last_error()
    assert L.ll_map_refine_merge(None, 0.2, C.byref(n), None) < 0 and b"ll_map_refine_merge: null" in L.ll_last_error() and n.value == -7
    assert L.ll_map_refine_fetch_merged(None, capi.ptr(pts), 4) < 0 and b"ll_map_refine_fetch_merged: null" in L.ll_last_error()
    assert L.ll_map_refine_work(None, capi.ptr(work)) < 0 and b"ll_map_refine_work: null" in L.ll_last_error()
    L.ll_map_refine_destroy(None)
