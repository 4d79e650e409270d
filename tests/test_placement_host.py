"""No-GPU tier of tests/placement.py: the device math headers compiled for the host (tests/hostcheck) and the host chain of the batched
deferred store, against the oracle, with the world placed where a real trajectory takes it -- across zero on every axis, kilometres out
with walls that are not parallel to the grid, and 50 km out where one fp32 ulp is 4 mm -- and on search grids a stray point has coarsened.
tests/test_gpu_placement.py runs the kernels on the same inputs."""
import copy

import numpy as np
import pytest

from loam_livox_amd import synth
from oracle import orc
from oracle.orc_cellmap import CellMap
from tests import placement as pl
from tests import test_cellmatch_batch_host as chain
from tests.conftest import oracle_features
from tests.hostcheck import hc
from tests.test_cellmap import bits, clouds, same_store, some_pose, structured_cloud
from tests.test_cellmatch_batch_host import host_exe  # noqa: F401  (that file's fixture: the same recipe, not a second one)
from tests.test_hostcheck import hc_reg_params

NAMES = list(pl.PLACEMENTS)


@pytest.fixture(scope="module")
def placed(small_world):
    """name -> the placed maps and their k-d trees"""
    out = {}
    for name, P in pl.PLACEMENTS.items():
        corner, surf = pl.place_points(P, small_world["corner"]), pl.place_points(P, small_world["surf"])
        out[name] = dict(P=P, corner=corner, surf=surf, tree_c=orc.KdTree(corner), tree_s=orc.KdTree(surf))
    return out


@pytest.fixture(scope="module")
def feats(scans):
    return [oracle_features(sc)[4:] for sc in scans[:2]]


def check_search(grid, tree, q, max_d2):
    wi, wd = pl.knn_within(tree, q, max_d2)
    hi, hd = grid.knn5(q, max_d2)
    assert np.array_equal(wi, hi) and np.array_equal(bits(wd), bits(hd))
    ti, td, _, _ = grid.knn5_tile(q, max_d2)
    assert np.array_equal(hi, ti) and np.array_equal(bits(hd), bits(td))
    return hi


@pytest.mark.parametrize("name", NAMES)
def test_search_at_a_placement(placed, scans, feats, name):
    w = placed[name]
    pose = pl.place_pose(w["P"], scans[0].pose_init)
    fc, fs = feats[0]
    gi = check_search(hc.Grid(w["surf"], 0.6), w["tree_s"], pl.search_queries(pose, fs, w["surf"]), 50.0)
    assert (gi[:len(fs)] >= 0).all() and (gi[-50:, 0] >= 0).all()
    gi = check_search(hc.Grid(w["corner"], 1.45), w["tree_c"], pl.search_queries(pose, fc, w["corner"]), 2.0)
    assert (gi[:len(fc), 0] >= 0).mean() > 0.5 and (gi[-50:, 0] >= 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_registration_at_a_placement(placed, scans, feats, name):
    w = placed[name]
    gc, gs = hc.Grid(w["corner"], 0.5), hc.Grid(w["surf"], 1.0)
    for k in (0, 1):
        fc, fs = feats[k]
        start = pl.place_pose(w["P"], scans[k].pose_init)
        for force in (0, 1):
            prm = orc.RegParams.defaults(icp_iters=6, ceres_iters=20, force_all=force)
            ret, pc, pi, rep = orc.reg_solve(w["tree_c"], w["tree_s"], fc, fs, prm, start, start)
            hret, hpc, hpi, hrep = hc.reg_solve(gc, gs, fc, fs, hc_reg_params(6, 20, force), start, start)
            dt, dr = synth.pose_error(pc, hpc)
            print(f"{name} scan {k} force {force}: dt {dt:.2e} dr {dr:.2e}")
            assert ret == hret == 1 and dt < 1e-9 and dr < 1e-9
            assert rep.icp_iterations == hrep[3] and rep.n_blocks_last == hrep[4]
            assert rep.corner_avail == hrep[5] and rep.surf_avail == hrep[6] and rep.lm_iterations_total == hrep[7]
            assert np.isclose(rep.final_cost, hrep[0], rtol=1e-9) and np.isclose(rep.inlier_threshold, hrep[2], rtol=1e-9)


GEOMETRY = {"two_axes": (25.62890625, (7804, 7808, 1)), "diagonal": (129.746337890625, (463, 463, 463)), "wide_x": (1.5, (666667, 61, 3))}


@pytest.mark.parametrize("stray", list(pl.STRAYS))
def test_search_on_a_coarsened_grid(small_world, scans, feats, stray):
    """two stray points are enough for map_grid_geometry to grow the cell until the dense table fits: the 200 k-point world then sits in a
    handful of cells (hc.Grid does not coarsen: it is built with the grown edge)"""
    surf = small_world["surf"]
    pts = pl.with_strays(surf, pl.STRAYS[stray])
    h, dims = pl.coarsened_cell(pts, 1.0)
    assert dims == GEOMETRY[stray][1] and abs(h / GEOMETRY[stray][0] - 1) < 1e-4
    assert dims[0] * dims[1] * dims[2] <= 1 << 27
    q = np.concatenate([pl.search_queries(scans[0].pose_init, feats[0][1], surf), pl.stray_queries(pl.STRAYS[stray])])
    gi = check_search(hc.Grid(pts, h), orc.KdTree(pts), q, 50.0)
    n = len(pl.STRAYS[stray])
    assert gi[-1 - n:-1, 0].tolist() == list(range(len(surf), len(surf) + n)) and (gi[-1] == -1).all()   # each stray found; nothing near (1e5, 44, 2)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("replace", [1, 0])
def test_cell_map_at_a_placement(name, replace):
    """tests/test_cellmap.py test_host_build_of_device_store_matches_oracle with its clouds and poses placed"""
    P = pl.PLACEMENTS[name]
    o, h = CellMap(1.0, 3), hc.CellMap(1.0, 3)
    for f, c in enumerate(clouds()):
        c = pl.place_points(P, c)
        o.append(c); h.append(c)
        same_store(o.dump(), h.dump())
        assert h.sizes() == (len(o.cells), o.n_points(), o.frame)
        if f % 2 == 1:
            pose = pl.place_pose(P, some_pose(f))
            ca, keys = o.query_filter(pose, 4.0, 45.0, 0.2, replace)
            cb, nsel = h.query_filter(pose, 4.0, 45.0, 0.2, replace)
            assert nsel == len(keys) > 20 and len(ca) > 100
            assert np.array_equal(bits(ca), bits(cb))
            same_store(o.dump(), h.dump())
    assert o.n_points() < 8 * 2000 - 3000   # the revisit rule fired


def test_oracle_cell_features_stay_solid_across_zero():
    """what tests/test_gpu_placement.py relies on when it applies same_features in full at `straddle`"""
    o = CellMap(1.0)
    o.append(pl.place_points(pl.PLACEMENTS["straddle"], structured_cloud()))
    assert (o.features()["margin"] > 1e-3).mean() > 0.95


@pytest.mark.parametrize("name", ["straddle", "far"])
@pytest.mark.parametrize("replace", [1, 0])
def test_batched_deferred_store_at_a_placement(host_exe, tmp_path, monkeypatch, name, replace):  # noqa: F811
    """the host chain of tests/test_cellmatch_batch_host.py once more, its clouds and view poses placed: equal to the oracle after every step"""
    P = pl.PLACEMENTS[name]
    base_clouds, base_view = chain.clouds, chain.view_pose
    monkeypatch.setattr(chain, "clouds", lambda: {k: pl.place_points(P, v) for k, v in base_clouds().items()})
    monkeypatch.setattr(chain, "view_pose", lambda m, t: pl.place_pose(P, base_view(m, t)))
    monkeypatch.setattr(chain, "_oracle", {})
    want = copy.copy(chain.oracle_run(replace))
    sel = want[3]
    assert sum(0 < a < b for a, b in sel) >= len(sel) * 3 // 4 and all(b > 0 for _, b in sel)
    cats, dumps, counts, _ = chain.run_host(host_exe, str(tmp_path), replace, [1] * chain.N_STEPS)
    assert len(dumps) == chain.N_STEPS * 6
    for t in range(chain.N_STEPS):
        chain.assert_step(cats, dumps, want, t, name + ": read after every step")
    reads = [int(t in (3, 7, 11)) for t in range(chain.N_STEPS)]
    cats, dumps, counts, _ = chain.run_host(host_exe, str(tmp_path), replace, reads)
    assert sorted({k[0] for k in dumps}) == [3, 7, 11]
    for t in range(chain.N_STEPS):
        chain.assert_step(cats, dumps, want, t, name + ": three reads")
