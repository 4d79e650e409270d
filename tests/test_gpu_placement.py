"""-m gpu: the device path far from the origin and on coarsened search grids (tests/placement.py; tests/test_placement_host.py is the CPU
tier on the same inputs).  The world every other device test uses sits in [0, 90] x [0, 90] x [0, 4] m and the loops start at the identity;
here map and poses are moved across zero on every axis (`straddle`), kilometres out with tilted walls (`km`) and 50 km out, where one fp32
ulp is 4 mm (`far`), and stray points coarsen the grid until 200 k points sit in a handful of cells.

Every comparison is against the oracle or the k-d tree on the same floats, except where a per-sequence route (Laser_mapping run alone,
separate handles) is the yardstick for the batched code -- and that route is held to the oracle here, at the same placement."""
import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.api import (Cell_map, History_buffer, History_buffer_batch, Livox_laser, Map_buffer, Point_cloud_registration,
                                VoxelGrid)
from loam_livox_amd.capi import LoamLivoxError
from oracle import orc
from oracle.orc_cellmap import CellMap
from oracle.orc_mapping import History, LaserMapping
from tests import placement as pl
from tests.conftest import oracle_features
from tests.test_cellmap import IDENT, clouds, same_features, same_store, some_pose, structured_cloud
from tests.test_gpu_cellmatch_batch import LOOP_KW
from tests.test_gpu_multimap import MAP_ARGS, N_PTS, bits, report_tuple

pytestmark = pytest.mark.gpu
NAMES = list(pl.PLACEMENTS)
POSE_TOL_M, POSE_TOL_RAD = 1e-4, 1e-4
worst = {}  # (placement, path) -> largest (dt, dr) against the oracle, printed per test


def note(name, path, dt, dr):
    a, b = worst.get((name, path), (0.0, 0.0))
    worst[(name, path)] = (max(a, dt), max(b, dr))
    print(f"placement {name:8s} path {path:22s} dt {dt:.3e} m dr {dr:.3e} rad (largest so far {worst[(name, path)][0]:.3e} / {worst[(name, path)][1]:.3e})")


# ---- inputs, cached per module ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def feats(scans):
    """per scan: (oracle extraction, corner features, surface features)"""
    out = []
    for sc in scans:
        fe, _, _, _, fc, fs = oracle_features(sc)
        out.append((fe, fc, fs))
    return out


@pytest.fixture(scope="module")
def placed(gpu_lib, small_world):
    """name -> the placed maps, their k-d trees and a Map_buffer that holds them"""
    out = {}
    for name, P in pl.PLACEMENTS.items():
        corner, surf = pl.place_points(P, small_world["corner"]), pl.place_points(P, small_world["surf"])
        m = Map_buffer()
        m.setInputCloud(Map_buffer.CORNER, corner)
        m.setInputCloud(Map_buffer.SURF, surf)
        out[name] = dict(P=P, corner=corner, surf=surf, tree_c=orc.KdTree(corner), tree_s=orc.KdTree(surf), map=m)
    yield out
    for w in out.values():
        w["map"].close()


@pytest.fixture(scope="module")
def strayed(gpu_lib, small_world):
    """stray set -> the surface map with the strays behind it (grid asked for at 1 m), the un-placed corner map, trees, a Map_buffer"""
    out = {}
    for name, st in pl.STRAYS.items():
        surf = pl.with_strays(small_world["surf"], st)
        m = Map_buffer()
        m.setInputCloud(Map_buffer.CORNER, small_world["corner"])
        m.setInputCloud(Map_buffer.SURF, surf, 1.0)
        out[name] = dict(P=IDENT, corner=small_world["corner"], surf=surf, tree_c=small_world["tree_c"], tree_s=orc.KdTree(surf), map=m)
    yield out
    for w in out.values():
        w["map"].close()


def set_params(reg, icp=10, ceres=20, force=1):
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = icp, ceres, force
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    return p


_oracle_reg = {}


def oracle_reg(tag, w, fc, fs, start, icp=10, force=1, deblur=None):
    """orc.reg_solve on the k-d trees of the world w (cached under tag)"""
    key = (tag, icp, force, deblur)
    if key not in _oracle_reg:
        prm = orc.RegParams.defaults(icp_iters=icp, ceres_iters=20, force_all=force, **({} if deblur is None else {"deblur": 1}))
        if deblur is not None:
            prm.minimum_pt_time_stamp, prm.maximum_pt_time_stamp = deblur
        ret, pc, _, rep = orc.reg_solve(w["tree_c"], w["tree_s"], fc, fs, prm, start, start)
        _oracle_reg[key] = (ret, pc, rep)
    return _oracle_reg[key]


def assert_registration(name, path, want, gret, pose, g, knn=None):
    """the assertions of tests/test_gpu_reg.py test_registration_matches_oracle; knn = (w, start, fc, fs, (ci, cd, si, sd))"""
    ret, pc, rep = want
    dt, dr = synth.pose_error(pose, pc)
    note(name, path, dt, dr)
    assert gret == ret
    assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD
    assert dt < 1e-7 and dr < 1e-7, (name, path, dt, dr)  # identical algorithms in fp64
    assert g.icp_iterations == rep.icp_iterations and g.n_blocks_last == rep.n_blocks_last
    assert g.corner_avail == rep.corner_avail and g.surf_avail == rep.surf_avail
    assert g.lm_iterations_total == rep.lm_iterations_total
    assert np.isclose(g.final_cost, rep.final_cost, rtol=1e-8) and np.isclose(g.initial_cost, rep.initial_cost, rtol=1e-8)
    assert np.isclose(g.inlier_threshold, rep.inlier_threshold, rtol=1e-8)
    assert np.isclose(g.angular_diff_deg, rep.angular_diff_deg, atol=1e-6) and np.isclose(g.t_diff, rep.t_diff, atol=1e-8)
    if knn is not None:
        assert_first_iteration_lists(*knn)


def assert_first_iteration_lists(w, start, fc, fs, lists):
    ci, cd, si, sd = lists
    wi, wd = pl.knn_within(w["tree_s"], synth.transform_points(start, fs[:, :3]), 50.0)
    assert np.array_equal(wi, si) and np.array_equal(bits(wd), bits(sd))
    wi, wd = pl.knn_within(w["tree_c"], synth.transform_points(start, fc[:, :3]), 2.0)
    assert np.array_equal(wi, ci)


def solve_one(w, fc, fs, start, icp=10, force=1, deblur=None, max_features=24000, **debug):
    reg = Point_cloud_registration(max_scans=1, max_features=max_features)
    reg.set_debug(True, **debug)
    p = set_params(reg, icp, 20, force)
    if deblur is not None:
        p.if_motion_deblur, p.minimum_pt_time_stamp, p.maximum_pt_time_stamp = 1, deblur[0], deblur[1]
    reg.m_pose_w_last, reg.m_pose_w_curr = start.copy(), start.copy()
    gret = reg.find_out_incremental_transfrom(w["map"], fc, fs)
    out = (gret, reg.m_pose_w_curr.copy(), reg.report, reg.debug_knn(0, len(fc), len(fs)))
    reg.close()
    return out


_batch20 = {}


def batch20(tag, w, scans, feats, icp=10):
    """a batch of 20 (tile search + one workgroup per scan) on the world w, slot i = scans[i % 4] from its placed start pose; cached"""
    if tag not in _batch20:
        n = 20
        reg = Point_cloud_registration(max_scans=n, max_features=24000)
        reg.set_debug(True, knn_tile_small_batches=True)
        set_params(reg, icp, 20, 1)
        start = np.stack([pl.place_pose(w["P"], scans[i % len(scans)].pose_init) for i in range(n)])
        res, pc, _, reps = reg.solve_batch(w["map"], [feats[i % len(scans)][1] for i in range(n)], [feats[i % len(scans)][2] for i in range(n)], start, start)
        knn = [reg.debug_knn(i, len(feats[i][1]), len(feats[i][2])) for i in range(len(scans))]
        reg.close()
        _batch20[tag] = (res.copy(), pc.copy(), reps, knn, start)
    return _batch20[tag]


def search_forms(m, kind, q, max_d2):
    """both stand-alone forms of the search over the queries q: one wavefront per query (up to 8192 queries), one lane per query (more)"""
    q = np.ascontiguousarray(q, np.float32)
    step = len(q) // 7936 + 1
    sub = q if step == 1 else np.concatenate([q[:-256:step], q[-256:]])  # (the last 256 hold the queries outside, on the map and at the strays)
    assert len(sub) <= 8192
    gi, gd = m.nearestKSearch(kind, sub, max_d2)
    reps = 8192 // len(q) + 1
    li, ld = m.nearestKSearch(kind, np.tile(q, (reps, 1)), max_d2)
    assert len(q) * reps > 8192
    for r in range(1, reps):  # (the tiled copies answer alike)
        assert np.array_equal(li[:len(q)], li[r * len(q):(r + 1) * len(q)]) and np.array_equal(bits(ld[:len(q)]), bits(ld[r * len(q):(r + 1) * len(q)]))
    return (sub, gi, gd), (q, li[:len(q)], ld[:len(q)])


def assert_search(m, kind, tree, q, max_d2):
    for qq, gi, gd in search_forms(m, kind, q, max_d2):
        wi, wd = pl.knn_within(tree, qq, max_d2)
        assert np.array_equal(wi, gi) and np.array_equal(bits(wd), bits(gd))


# ---- A. search --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_search_at_a_placement(placed, scans, feats, name):
    w = placed[name]
    start = pl.place_pose(w["P"], scans[0].pose_init)
    assert_search(w["map"], Map_buffer.SURF, w["tree_s"], pl.search_queries(start, feats[0][2], w["surf"]), 50.0)
    assert_search(w["map"], Map_buffer.CORNER, w["tree_c"], pl.search_queries(start, feats[0][1], w["corner"]), 2.0)
    # the registrar's tile search: the first ICP iteration's lists of a batch of 20
    res, pc, reps, knn, starts = batch20(name, w, scans, feats)
    for i in range(len(scans)):
        assert_first_iteration_lists(w, starts[i], feats[i][1], feats[i][2], knn[i])


@pytest.mark.parametrize("name", NAMES)
def test_fp16_point_map_knn_is_exact_on_the_dequantised_cloud_at_a_placement(placed, name):
    """tests/test_gpu_voxel.py test_fp16_point_map_knn_is_exact_on_the_dequantised_cloud, its method unchanged, on the placed surface map"""
    rng = np.random.default_rng(21)
    surf = placed[name]["surf"][:, :3].copy()
    surf[5] = surf[9]
    surf[17, 1] = np.nan
    m = Map_buffer()
    m.setInputCloud(Map_buffer.SURF, surf)
    q = (surf[rng.choice(len(surf), 3000)] + rng.normal(0, 0.3, (3000, 3))).astype(np.float32)
    q[0] = surf[5]
    i32, d32 = m.nearestKSearch(Map_buffer.SURF, q, 50.0)
    m.to_f16(Map_buffer.SURF)
    deq = m.dequantized(Map_buffer.SURF)
    ok = np.isfinite(surf).all(1)
    assert np.isnan(deq[~ok]).all() and np.isfinite(deq[ok]).all()
    err = np.abs(deq[ok].astype(np.float64) - surf[ok].astype(np.float64)).max()
    print(f"placement {name}: fp16 records move a point by at most {err:.3e} m")
    assert err <= 0.6 * 2.0 ** -11 * 1.01 + 1e-5
    i16, d16 = m.nearestKSearch(Map_buffer.SURF, q, 50.0)
    tree = orc.KdTree(np.where(np.isfinite(deq), deq, 1e9).astype(np.float32))
    oi, od = tree.knn(q, 5)
    assert np.array_equal(oi, i16) and np.array_equal(bits(od), bits(d16))
    assert i16[0, 0] == 5 and i16[0, 1] == 9 and d16[0, 0] == d16[0, 1]
    assert (np.sort(i16, 1) == np.sort(i32, 1)).all(1).mean() > 0.95
    m.close()


# ---- B. registration ------------------------------------------------------------------------------------------------------------------------
PATHS = {"compact group of 8": {}, "compact one workgroup": {"no_solver_groups": True}, "general": {"force_general_solver": True}}


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("path", list(PATHS))
def test_registration_at_a_placement(placed, scans, feats, name, path):
    w = placed[name]
    for k in (0, 1):
        _, fc, fs = feats[k]
        start = pl.place_pose(w["P"], scans[k].pose_init)
        for force in (0, 1):
            want = oracle_reg((name, k), w, fc, fs, start, 10, force)
            gret, pose, rep, lists = solve_one(w, fc, fs, start, 10, force, **PATHS[path])
            assert_registration(name, path, want, gret, pose, rep, (w, start, fc, fs, lists))


@pytest.mark.parametrize("name", NAMES)
def test_motion_deblur_at_a_placement(placed, scans, feats, name):
    w = placed[name]
    fe, fc, fs = feats[1]
    span = (float(fe.time_stamp.min()), float(fe.time_stamp.max()))
    start = pl.place_pose(w["P"], scans[1].pose_init)
    want = oracle_reg((name, 1), w, fc, fs, start, 6, 1, span)
    for general in (False, True):
        gret, pose, rep, _ = solve_one(w, fc, fs, start, 6, 1, span, force_general_solver=general)
        assert_registration(name, "motion deblur" + (" general" if general else ""), want, gret, pose, rep)


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("waves", [1, 4])
def test_small_solver_at_a_placement(placed, scans, feats, name, waves):
    """the registrar's input in input_downsample_mode (VoxelGrid 0.1 / 0.4 m on the feature clouds), as tests/test_gpu_small.py sets it"""
    w = placed[name]
    filtered = [(orc.voxel_grid(f[1], 0.1)[1], orc.voxel_grid(f[2], 0.4)[1]) for f in feats]
    start = np.stack([pl.place_pose(w["P"], sc.pose_init) for sc in scans])
    reg = Point_cloud_registration(max_scans=len(scans), max_features=2048)
    reg.set_debug(False, small_solver_waves=waves)
    set_params(reg, 10, 20, 1)
    res, pc, _, reps = reg.solve_batch(w["map"], [f[0] for f in filtered], [f[1] for f in filtered], start, start)
    reg.close()
    for b in range(len(scans)):
        fc, fs = filtered[b]
        assert len(fc) + len(fs) <= 1024
        want = oracle_reg((name, "filtered", b), w, fc, fs, start[b], 10, 1)
        assert_registration(name, f"small solver {waves} wave", want, res[b], pc[b], reps[b])


@pytest.mark.parametrize("name", NAMES)
def test_batch_of_20_at_a_placement(placed, scans, feats, name):
    w = placed[name]
    res, pc, reps, knn, starts = batch20(name, w, scans, feats)
    for i in range(20):
        k = i % len(scans)
        want = oracle_reg((name, k), w, feats[k][1], feats[k][2], starts[i], 10, 1)
        assert_registration(name, "batch of 20", want, res[i], pc[i], reps[i])
        assert np.array_equal(pc[i], pc[k])  # the same scan in another slot: the same bits


# ---- C. VoxelGrid -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_voxel_grid_at_a_placement(placed, scans, feats, name):
    w = placed[name]
    start = pl.place_pose(w["P"], scans[0].pose_init)
    vg = VoxelGrid(max_points=24000)
    for cloud in (feats[0][1], feats[0][2]):
        p = pl.place_points(start, cloud)
        for leaf in (0.1, 0.4):
            vg.setLeafSize(leaf, leaf, leaf)
            vg.setInputCloud(p)
            out = vg.filter()
            st, ref = orc.voxel_grid(p, leaf)
            assert vg.status == st == 0 and out.shape == ref.shape and np.array_equal(bits(out), bits(ref))
    vg.close()


@pytest.mark.parametrize("name", NAMES)
def test_downsampled_registration_at_a_placement(placed, scans, feats, name):
    """tests/test_gpu_voxel.py test_downsampled_registration_matches_oracle on the placed map, from the placed start poses"""
    w = placed[name]
    B = len(scans)
    fe = Livox_laser(max_points=24000, max_scans=B, piecewise_number=1)
    fe.upload(np.stack([s.xyzi for s in scans]), np.full(B, 1.0))
    fe.extract_batch(B); fe.resolve(); fe.select_batch(B, -1, 0.0, 1.0)
    vc, vs = VoxelGrid(24000, B), VoxelGrid(24000, B)
    reg = Point_cloud_registration(max_scans=B, max_features=24000)
    set_params(reg, 10, 20, 1)
    start = np.stack([pl.place_pose(w["P"], s.pose_init) for s in scans])
    reg.enqueue_fe_downsampled(w["map"], fe, vc, vs, 0.1, 0.4, B, start, start)
    res, pc, pi, reps = reg.collect(B)
    nc, _ = vc.counts(B)
    ns, _ = vs.counts(B)
    for b in range(B):
        fc_ds, fs_ds = orc.voxel_grid(feats[b][1], 0.1)[1], orc.voxel_grid(feats[b][2], 0.4)[1]
        assert nc[b] == len(fc_ds) and ns[b] == len(fs_ds) and len(fs_ds) < len(feats[b][2])
        want = oracle_reg((name, "filtered", b), w, fc_ds, fs_ds, start[b], 10, 1)
        assert_registration(name, "downsampled on device", want, res[b], pc[b], reps[b])
    for h in (fe, vc, vs, reg):
        h.close()


# ---- D. the loops, started at a placement -----------------------------------------------------------------------------------------------------
N_FRAMES, SEED = 7, 77


@pytest.fixture(scope="module")
def sequence(small_world):
    return synth.make_livox_sequence(small_world["world"], SEED)[0][:N_FRAMES]


_alone, _oracle_loop = {}, {}


def oracle_loop(sequence, name, mode):
    """the oracle loop started at the placement: per frame (result, pose, map sizes, n_blocks_last)"""
    if (name, mode) not in _oracle_loop:
        om = LaserMapping(matching_mode=mode, **(LOOP_KW if mode else {}), **MAP_ARGS)
        om.pose = pl.PLACEMENTS[name].copy()
        out = []
        for xyzi in sequence:
            r = om.process_new_scan(xyzi)
            out.append((int(r), om.pose.copy(), (len(om.maps[0]), len(om.maps[1])), om.report.n_blocks_last))
        _oracle_loop[(name, mode)] = out
    return _oracle_loop[(name, mode)]


def alone(sequence, name, mode):
    """Laser_mapping alone, started at the placement: per frame (result, pose, report, map sizes), and in cell mode the final dumps"""
    from loam_livox_amd.mapping import Laser_mapping
    if (name, mode) not in _alone:
        kw = dict(matching_mode=1, cell_map_max_points=1 << 18, **LOOP_KW) if mode else dict(matching_mode=0)
        lm = Laser_mapping(scan_points=N_PTS, **kw, **MAP_ARGS)
        lm.pose = pl.PLACEMENTS[name].copy()
        out = []
        for xyzi in sequence:
            r = lm.process_new_scan(xyzi)
            out.append((int(r), lm.pose.copy(), report_tuple(lm.last_report), tuple(int(x) for x in lm.map_sizes), lm.last_report.n_blocks_last))
        dumps = [lm.history.cell_map(kind).dump() + (lm.history.cell_map(kind).stats(),) for kind in (0, 1)] if mode else None
        lm.close()
        _alone[(name, mode)] = (out, dumps)
    return _alone[(name, mode)]


def assert_loop_matches_oracle(name, path, got, want):
    """the assertions of tests/test_gpu_cellmatch_batch.py test_loop_in_cell_mode_matches_the_oracle_loop; got[k] = (result, pose, map sizes,
    n_blocks_last)"""
    assert len(got) == len(want) == N_FRAMES
    for k in range(N_FRAMES):
        dt, dr = synth.pose_error(got[k][1], want[k][1])
        note(name, path, dt, dr)
        assert got[k][0] == want[k][0] == 1, (name, k)
        assert dt < 1e-7 and dr < 1e-7, (name, path, k, dt, dr)
        assert got[k][2] == want[k][2], (name, k, "map sizes", got[k][2], want[k][2])
        assert got[k][3] == want[k][3], (name, k, "n_blocks_last")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("mode", [0, 1])
def test_loop_started_at_a_placement_matches_the_oracle_loop(gpu_lib, sequence, name, mode):
    out, _ = alone(sequence, name, mode)
    assert_loop_matches_oracle(name, f"loop mode {mode}", [(o[0], o[1], o[3], o[4]) for o in out], oracle_loop(sequence, name, mode))


@pytest.mark.parametrize("cell_matching", [True, False])
def test_batched_loop_with_a_placement_per_slot(gpu_lib, sequence, cell_matching):
    """three slots of ONE handle at the three placements: one batched add and one batched refresh serve grids 50 km apart.  Every slot against
    the oracle loop at its placement, and bit for bit against Laser_mapping run alone from the same start pose."""
    from loam_livox_amd.mapping import Laser_mapping_batch
    S, mode = len(NAMES), int(cell_matching)
    kw = dict(cell_maps=True, cell_matching=True, cell_map_max_points=1 << 16, **LOOP_KW) if cell_matching else {}
    lb = Laser_mapping_batch(S, batched_history=True, scan_points=N_PTS, **kw, **MAP_ARGS)
    for s, name in enumerate(NAMES):
        lb.poses[s] = pl.PLACEMENTS[name]
    got = [[] for _ in range(S)]
    for xyzi in sequence:
        out = lb.process_new_scans([xyzi] * S)
        for s in range(S):
            got[s].append((int(out[s]), lb.poses[s].copy(), report_tuple(lb.last_reports[s]), tuple(int(x) for x in lb.map_sizes[s]),
                           lb.last_reports[s].n_blocks_last))
    dumps = None
    if cell_matching:
        lb.sync()
        dumps = [[lb.cell_map(s, kind).dump() + (lb.cell_map(s, kind).stats(),) for kind in (0, 1)] for s in range(S)]
    lb.close()
    for s, name in enumerate(NAMES):
        assert_loop_matches_oracle(name, f"batched loop mode {mode}", [(g[0], g[1], g[3], g[4]) for g in got[s]], oracle_loop(sequence, name, mode))
        want, wdumps = alone(sequence, name, mode)
        for k in range(N_FRAMES):
            g, w = got[s][k], want[k]
            assert g[0] == w[0], (name, k, "result")
            assert np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64)), (name, k, "pose", g[1] - w[1])
            assert g[2] == w[2], (name, k, "report")
            assert g[3] == w[3], (name, k, "map_sizes", g[3], w[3])
        if cell_matching:
            for kind in (0, 1):
                gd, wd = dumps[s][kind], wdumps[kind]
                assert gd[4] == wd[4], (name, kind, "stats")
                assert gd[0].shape == wd[0].shape and np.array_equal(bits(gd[0]), bits(wd[0])), (name, kind, "points")
                for i in (1, 2, 3):
                    assert np.array_equal(gd[i], wd[i]), (name, kind, i)


# ---- E. the single-handle cell map ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["straddle", "far"])
@pytest.mark.parametrize("replace", [1, 0])
def test_device_cell_map_at_a_placement(gpu_lib, name, replace):
    """the pattern of tests/test_cellmap.py test_device_cell_map_bit_exact on placed clouds, at placed poses"""
    P = pl.PLACEMENTS[name]
    o, d = CellMap(1.0, 3), Cell_map(max_points=40000, resolution=1.0, minimum_revisit_threshold=3)
    for f, c in enumerate(clouds()):
        c = pl.place_points(P, c)
        if f == 2:
            c[5, 1] = np.nan; c[6, 2] = np.inf; c[7, 0] = 3.0e6   # dropped: non-finite / beyond the key range
        o.append(c); d.append_cloud(c)
        assert d.stats() == (len(o.cells), o.n_points(), o.frame)
        same_store(o.dump(), d.dump())
        if f % 2 == 1:
            pose = pl.place_pose(P, some_pose(f))
            ca, keys = o.query_filter(pose, 4.0, 45.0, 0.2, replace)
            cb, nsel = d.query_filter(pose, 4.0, 45.0, 0.2, replace)
            assert nsel == len(keys) > 20
            assert np.array_equal(bits(ca), bits(cb))
            same_store(o.dump(), d.dump())
    assert o.n_points() < 8 * 2000 - 3000   # the revisit rule fired
    d.close()


@pytest.mark.parametrize("name", NAMES)
def test_device_cell_features_at_a_placement(gpu_lib, name):
    """both sides do the same float sums in the same order, so the moments cancel identically wherever the cloud sits; eigenvalues, labels
    and vectors are held to the oracle where the float moments still carry them: across zero"""
    c = pl.place_points(pl.PLACEMENTS[name], structured_cloud())
    o, d = CellMap(1.0), Cell_map(max_points=1 << 17, resolution=1.0)
    o.append(c); d.append_cloud(c)
    fo, fd = o.features(), d.features()
    assert len(fo["mean"]) > 100
    assert np.array_equal(bits(fo["mean"]), bits(fd["mean"])) and np.array_equal(bits(fo["cov"]), bits(fd["cov"]))
    if name == "straddle":
        same_features(fo, fd)
    d.close()


# ---- F. coarsened grids and stray points ------------------------------------------------------------------------------------------------------
GEOMETRY = {"two_axes": (7804, 7808, 1), "diagonal": (463, 463, 463), "wide_x": (666667, 61, 3)}
F_ICP = 4  # (every query of a coarsened grid scans most of the map: four ICP iterations keep a batch of 20 within seconds)


@pytest.mark.parametrize("stray", list(pl.STRAYS))
def test_search_on_a_coarsened_grid(strayed, small_world, scans, feats, stray):
    w = strayed[stray]
    h, dims = pl.coarsened_cell(w["surf"], 1.0)
    assert dims == GEOMETRY[stray]
    assert w["map"].cells(Map_buffer.SURF) == dims[0] * dims[1] * dims[2] <= 1 << 27
    q = np.concatenate([pl.search_queries(scans[0].pose_init, feats[0][2], small_world["surf"]), pl.stray_queries(pl.STRAYS[stray])])
    assert_search(w["map"], Map_buffer.SURF, w["tree_s"], q, 50.0)
    res, pc, reps, knn, starts = batch20(("stray", stray), w, scans, feats, F_ICP)
    for i in range(len(scans)):
        assert_first_iteration_lists(w, starts[i], feats[i][1], feats[i][2], knn[i])


@pytest.mark.parametrize("stray", list(pl.STRAYS))
def test_registration_on_a_coarsened_grid(strayed, scans, feats, stray):
    w = strayed[stray]
    _, fc, fs = feats[0]
    start = scans[0].pose_init
    want = oracle_reg(("stray", stray, 0), w, fc, fs, start, F_ICP, 1)
    for path in ("compact group of 8", "general"):
        gret, pose, rep, lists = solve_one(w, fc, fs, start, F_ICP, 1, **PATHS[path])
        assert_registration("stray " + stray, path, want, gret, pose, rep, (w, start, fc, fs, lists))
    res, pc, reps, knn, starts = batch20(("stray", stray), w, scans, feats, F_ICP)
    for i in range(20):
        k = i % len(scans)
        want = oracle_reg(("stray", stray, k), w, feats[k][1], feats[k][2], starts[i], F_ICP, 1)
        assert_registration("stray " + stray, "batch of 20", want, res[i], pc[i], reps[i])


def test_fp16_conversion_is_refused_on_a_grid_too_wide(strayed, small_world):
    w = strayed["wide_x"]
    m = Map_buffer()
    m.setInputCloud(Map_buffer.SURF, w["surf"], 1.0)
    with pytest.raises(LoamLivoxError, match="16 bits of the cell x index"):
        m.to_f16(Map_buffer.SURF)
    rng = np.random.default_rng(8)
    q = np.concatenate([small_world["surf"][rng.choice(len(small_world["surf"]), 3000)] + rng.normal(0, 0.3, (3000, 3)),
                        pl.stray_queries(pl.STRAYS["wide_x"])]).astype(np.float32)
    gi, gd = m.nearestKSearch(Map_buffer.SURF, q, 50.0)   # the handle still answers, from its fp32 records
    wi, wd = pl.knn_within(w["tree_s"], q, 50.0)
    assert np.array_equal(wi, gi) and np.array_equal(bits(wd), bits(gd))
    m.close()


MATCH_CELL_SURF = 0.45  # the cell a match buffer asks for at MAP_ARGS' plane_res: three leaves, at least 0.45 m (ll_api_history.hip match_cell_size)


def history_frames(small_world, scans, feats, stray_at=None):
    """three frames for a match buffer: the features of scans 0 .. 2 through the VoxelGrid (MAP_ARGS' leaves), in the map frame poses of their
    scans; stray_at: that frame's surface cloud carries the first stray set behind it"""
    out = []
    for k in range(3):
        fc, fs = orc.voxel_grid(feats[k][1], MAP_ARGS["line_res"])[1], orc.voxel_grid(feats[k][2], MAP_ARGS["plane_res"])[1]
        if k == stray_at:
            st = pl.STRAYS["two_axes"]  # given in the map frame: moved into the sensor's, so that the add puts them (nearly) there
            local = synth.transform_points(synth.pose_inverse(scans[k].pose_true), st)
            fs = np.concatenate([fs, np.c_[local, np.zeros(len(st), np.float32)]]).astype(np.float32)
        out.append((fc, fs, scans[k].pose_true))
    return out


def assert_match_buffer(cloud_c, cloud_s, m, ora, seed):
    want = ora.refresh()
    for kind, got in ((0, cloud_c), (1, cloud_s)):
        assert got.shape == want[kind].shape and np.array_equal(bits(got), bits(want[kind])), (kind, "match-buffer cloud")
        rng = np.random.default_rng(seed + kind)
        q = (want[kind][rng.integers(0, len(want[kind]), 2000), :3] + rng.normal(0.0, 0.4, (2000, 3))).astype(np.float32)
        gi, gd = m.nearestKSearch(kind, q, 1.0)
        wi, wd = pl.knn_within(orc.KdTree(want[kind]), q, 1.0)
        assert np.array_equal(wi, gi) and np.array_equal(bits(wd), bits(gd)), (kind, "k-NN")
    return want


def test_history_buffer_with_a_stray_in_its_second_frame(gpu_lib, small_world, scans, feats):
    dev, ora, m = History_buffer(5, N_PTS, MAP_ARGS["line_res"], MAP_ARGS["plane_res"]), History(5, MAP_ARGS["line_res"], MAP_ARGS["plane_res"]), Map_buffer()
    for fc, fs, pose in history_frames(small_world, scans, feats, stray_at=1):
        assert dev.add(fc, fs, pose) == ora.add(fc, fs, pose)
        dev.refresh(m)
        want = assert_match_buffer(dev.map_cloud(0), dev.map_cloud(1), m, ora, 40)
    assert np.abs(want[1][:, :3]).max() > 1.9e5   # the strays are in the match buffer
    h, dims = pl.coarsened_cell(want[1], MATCH_CELL_SURF)
    assert m.cells(Map_buffer.SURF) == dims[0] * dims[1] * dims[2] <= 1 << 27 and h > 10.0
    dev.close(); m.close()


def test_history_buffer_batch_with_a_stray_in_one_slot(gpu_lib, small_world, scans, feats):
    """S = 3, slot 1 alone carries strays: it holds the oracle History's cloud, and slots 0 and 2 the bits of a batch without any stray"""
    S, B = 3, 3
    res = (MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
    clean, stray = history_frames(small_world, scans, feats), history_frames(small_world, scans, feats, stray_at=1)
    stride = max(max(len(f[0]), len(f[1])) for f in stray)
    runs = {}
    for tag, per_slot in (("stray", [clean, stray, clean]), ("clean", [clean, clean, clean])):
        hb = History_buffer_batch(S, 5, stride, *res)
        vox = (VoxelGrid(stride, S), VoxelGrid(stride, S))
        for kind in (0, 1):
            vox[kind].setLeafSize(*([res[kind]] * 3))
        maps = [Map_buffer() for _ in range(S)]
        oras = [History(5, *res) for _ in range(S)]
        for k in range(B):
            for kind in (0, 1):  # (the frames are filtered already: the filter hands them on as they are, or leaf for leaf)
                buf, n = np.zeros((S, stride, 4), np.float32), np.zeros(S, np.int32)
                for s in range(S):
                    c = per_slot[s][k][kind]
                    buf[s, :len(c)], n[s] = c, len(c)
                out, n_out, st = vox[kind].filter_batch(buf, n)
                for s in range(S):
                    want = orc.voxel_grid(per_slot[s][k][kind], res[kind])[1]
                    assert n_out[s] == len(want) and np.array_equal(bits(out[s, :n_out[s]]), bits(want))
            poses = np.stack([per_slot[s][k][2] for s in range(S)])
            added = hb.add_voxel(vox[0], vox[1], poses)
            for s in range(S):
                fc, fs = (orc.voxel_grid(per_slot[s][k][kind], res[kind])[1] for kind in (0, 1))
                assert bool(added[s]) == oras[s].add(fc, fs, poses[s])
            hb.refresh(maps)
        runs[tag] = [(hb.map_cloud(s, 0), hb.map_cloud(s, 1)) for s in range(S)]
        if tag == "stray":
            for s in range(S):  # every slot against the oracle and the k-d tree
                assert_match_buffer(runs[tag][s][0], runs[tag][s][1], maps[s], oras[s], 50 + s)
            assert np.abs(runs[tag][1][1][:, :3]).max() > 1.9e5 and np.abs(runs[tag][0][1][:, :3]).max() < 200.0
            h, dims = pl.coarsened_cell(runs[tag][1][1], MATCH_CELL_SURF)
            assert maps[1].cells(Map_buffer.SURF) == dims[0] * dims[1] * dims[2] <= 1 << 27 and h > 10.0
        for h in [hb, vox[0], vox[1]] + maps:
            h.close()
    for s in (0, 2):
        for kind in (0, 1):
            assert np.array_equal(bits(runs["stray"][s][kind]), bits(runs["clean"][s][kind])), (s, kind)
