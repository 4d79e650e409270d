"""Drives every public method of loam_livox_amd/api.py once over the recording stand-in (tests/api_standin.py) with small fixed inputs,
and gives, per case, the full log of C calls and the returned values in JSON form.  tests/test_api_calls_host.py compares that with
tests/api_calls.json, which `python -m tests.api_calls_driver tests/api_calls.json` writes: the file in the tree was written that way by
this driver at the commit before the api.py helpers (a3c4a91), so it pins the order and the arguments of the calls each method makes."""
import contextlib
import json
import sys
import types

import numpy as np

from loam_livox_amd import api, capi, mapping
from tests.api_standin import Recording_library, plain

IDENT = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def cloud(n, cols=4, first=0.0):
    return (first + 0.25 * np.arange(n * cols, dtype=np.float32)).reshape(n, cols)


def poses(n, first=0.0):
    return np.tile(IDENT, (n, 1)) + first + 0.5 * np.arange(n)[:, None]


class _Tensor:
    """what the *_device methods ask of a torch tensor"""

    def __init__(self, address, shape):
        self.address, self.shape = address, shape

    def data_ptr(self):
        return self.address

    def is_contiguous(self):
        return True


@contextlib.contextmanager
def fake_torch():
    """`import torch` inside a method finds a module whose zeros() names its arguments: the empty device results without a device"""
    fake = types.ModuleType("torch")
    fake.float32, fake.int64 = "float32", "int64"
    fake.zeros = lambda shape, dtype=None, device=None: ["torch.zeros", plain(shape), dtype, device]
    saved = sys.modules.get("torch")
    sys.modules["torch"] = fake
    try:
        yield
    finally:
        if saved is None:
            del sys.modules["torch"]
        else:
            sys.modules["torch"] = saved


def raised(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except (capi.LoamLivoxError, ValueError, TypeError, AttributeError) as e:
        return {"raises": type(e).__name__}


# ---- the cases: each takes the stand-in and returns the list of what its calls returned -------------------------------------------------

def livox_laser(lib):
    fe = api.Livox_laser(max_points=60, max_scans=2, thr_corner_curvature=0.125)
    out = [raised(api.Livox_laser, no_such_tunable=1)]
    lib.answer("ll_fe_extract", out={4: 3})
    out.append(fe.extract_laser_features(cloud(5), 9.0))
    lib.answer("ll_fe_select", out={4: 2, 6: 3, 8: 5})
    out.append(fe.get_features(0.0, 0.5))
    out.append(fe.get_features(scan=1))
    out.append(fe.pts_info())
    lib.answer("ll_fe_splits", out={3: 2, 4: 7, 5: 1})
    out.append(fe.splits())
    out.append(fe.upload(cloud(12).reshape(2, 6, 4), np.array([1.0, 2.0])))
    out.append(fe.upload(cloud(6).reshape(1, 6, 4), np.array([3.0]), first_scan=1, wait=False))
    out += [fe.extract_batch(2), fe.resolve(), fe.select_batch(2), fe.select_batch(2, 1, 0.1, 0.9), fe.counts(2), fe.sync(), fe.pts_info(1)]
    fe.close()
    return out


def spinning_laser(lib):
    sp = api.Spinning_laser(scan_line=16, max_points=8, max_scans=2, max_line_points=8)
    out = [sp.upload([cloud(3), cloud(5, first=1.0)]), sp.upload([], first_scan=1)]
    lib.answer("ll_spin_resolve", ret=2)
    lib.answer("ll_spin_cloud", out={5: 2})
    out.append(sp.extract_batch([cloud(2)]))
    out += [sp.n_ambiguous, sp.extract_batch_async(2), sp.resolve(), sp.sync(), sp.extract(cloud(4)), sp.extract(np.zeros((0, 4)))]
    lib.answer("ll_spin_extract", ret=1)
    out.append(raised(sp.extract, cloud(4)))
    out += [sp.counts(2), sp.cloud(1, sp.SHARP), sp.cloud(0, sp.LESS_FLAT), sp.cloud(0, sp.FLAT, with_idx=False), sp.lines(1), sp.clouds(1)]
    lib.answer("ll_spin_handoff_time", out={1: 1.5})
    out += [sp.handoff_time(), sp.kernel_times()]
    sp.close()
    return out


def voxel_grid(lib):
    v = api.VoxelGrid(max_points=16, max_clouds=2)
    v.setLeafSize(0.1, 0.2, 0.3)
    v.setInputCloud(cloud(5))
    out = [v.filter(), v.status, v.filter_batch(cloud(12).reshape(2, 6, 4), [6, 4]), v.filter_batch(np.zeros((2, 0, 4)), [0, 0]), v.counts(2)]
    v.close()
    return out


def history_buffer(lib):
    h = api.History_buffer(maximum_history_size=5, max_points_per_frame=16, line_res=0.2, plane_res=0.8)
    fe, sp = api.Livox_laser(max_points=16), api.Spinning_laser(max_points=16)
    vc, vs, m = api.VoxelGrid(16), api.VoxelGrid(16), api.Map_buffer()
    lib.answer("ll_history_size", ret=4)
    out = [len(h), h.add(cloud(3), cloud(4, first=2.0), IDENT), h.add(cloud(3), cloud(4), IDENT + 1, 0.5, 0.25)]
    lib.answer("ll_history_add_fe", out={6: 1})
    out += [h.add_fe(fe, 0, IDENT), h.add_fe(fe, 1, IDENT + 1, 0.5, 0.25)]
    lib.answer("ll_history_add_spin", out={6: 1})
    out += [h.add_spin(sp, 0, IDENT), h.add_spin(sp, 1, IDENT + 2, 0.5, 0.25)]
    lib.answer("ll_history_add_voxel", out={7: 1})
    out += [h.add_voxel(vc, vs, 0, IDENT), h.add_voxel(vc, vs, 1, IDENT + 3, 0.5, 0.25)]
    lib.answer("ll_history_refresh", out={2: 11, 3: 12})
    out.append(h.refresh(m))
    out.append(raised(h.cell_map, 0))   # not enabled: the library answers null
    out += [h.enable_cell_map(64, 0.5, 7), h.set_cell_map_async(), h.set_cell_map_async(False), h.sync_cell_maps()]
    lib.answer("ll_history_cell_map", ret=0x7000)
    cm = h.cell_map(1)
    out.append([type(cm).__name__, cm.owned, cm.resolution, cm.max_points, cm.h.value])
    cm.close()
    out.append(cm.h)
    lib.answer("ll_history_refresh_cells", out={7: 5, 8: 6})
    out += [h.refresh_cells(m, IDENT), h.refresh_cells(m, IDENT + 1, 50.0, 60.0, 20.0, 0), h.set_gate_pose(IDENT + 2)]
    out.append(h.map_cloud(0))
    lib.answer("ll_history_map_cloud", ret=3)
    out.append(h.map_cloud(1))
    with fake_torch():
        out.append(h.map_cloud_device(1))
    for x in (h, fe, sp, vc, vs, m):
        x.close()
    return out


def history_buffer_map_cloud_negative(lib):
    h = api.History_buffer(5, 16)
    lib.answer("ll_history_map_cloud", ret=-1)
    out = [raised(h.map_cloud, 0)]
    h.close()
    return out


def _history_batch(lib, S):
    b = api.History_buffer_batch(S, maximum_history_size=5, max_points_per_frame=16, line_res=0.2, plane_res=0.8)
    fe, vc, vs = api.Livox_laser(max_points=16, max_scans=S), api.VoxelGrid(16, S), api.VoxelGrid(16, S)
    maps = [api.Map_buffer() for _ in range(S)]
    holes = [None] + maps[1:]
    mask = [True] + [False] * (S - 1)
    out = [b.add_voxel(vc, vs, poses(S)), b.add_voxel(vc, vs, poses(S), poses(S, 1.0), mask, 0.5, 0.25),
           b.add_fe(fe, poses(S)), b.add_fe(fe, poses(S), poses(S, 1.0), np.array(mask), 0.5, 0.25),
           b.refresh(maps), b.refresh(holes, active=mask[::-1]), raised(b.refresh, maps + [None]),
           b.refresh_cells(maps, poses(S)), b.refresh_cells(holes, None, mask, 50.0, 60.0, 20.0, 0), raised(b.refresh_cells, [], poses(S)),
           b.cell_match_work()]
    lib.answer("ll_history_batch_size", ret=3)
    out += [b.size(S - 1), b.map_cloud(0, 0)]
    lib.answer("ll_history_batch_map_cloud", ret=2)
    out.append(b.map_cloud(S - 1, 1))
    lib.answer("ll_history_batch_map_cloud", ret=-1)
    out.append(raised(b.map_cloud, 0, 1))
    out += [b.enable_cell_maps(64, 0.5, 7), b.sync_cell_maps(), b.cell_map_work(), b.enable_full_maps(32, 0.25, 9)]
    lib.answer("ll_history_batch_append_full_fe", out={})
    out += [b.append_full(fe, poses(S)), b.append_full(fe, poses(S), mask, min_points=2, lists=False)]
    lib.answer("ll_history_batch_full_touched", out={4: 2})
    out += [b.full_touched(S - 1), b.full_touched(0, 3)]
    dsts = [api.Cell_map(8, 0.25) for _ in range(S)]
    out += [b.extract_cells(2, [], [], []), b.extract_cells(1, list(range(S))[::-1], [cloud(2, 3).astype(int)] + [[]] * (S - 1), dsts),
            b.extract_cells(0, [0], [[]], dsts[:1]), raised(b.extract_cells, 0, [0], [], dsts[:1]), [d.max_points for d in dsts],
            b.extract_work(), b.full_map_work()]
    out += [b.enable_scan_log(), b.enable_scan_log(7, 3), b.log_full(fe), b.log_full(fe, mask)]
    lib.answer("ll_history_batch_scan_log_hand_over", out={2: 5})
    out += [b.hand_over(S - 1), b.drop_groups([]), b.drop_groups([5, 6]), b.read_group(5)]
    lib.answer("ll_history_batch_scan_log_read", out={4: 3})
    out += [b.read_group(6), b.scan_log_work()]
    # the views of a slot
    log = b.scan_log(S - 1)
    out += [type(log).__name__, log.hand_over(), log.drop([]), log.drop([5])]
    slot = b.cell_map(S - 1, 1)
    lib.answer("ll_history_batch_cell_map_stats", out={3: 2, 4: 5, 5: 1})
    with fake_torch():
        out += [type(slot).__name__, slot.resolution, slot.stats(), slot.dump(), slot.device_view(), slot.device_view(1)]
    out += [slot.extract_cells_into([[1, 2, 3]], dsts[0]), b.cell_map(0, 2).resolution]
    full = b.full_map(0)
    out += [type(full).__name__, full.kind, full.resolution, full.stats(), full.dump(), full.append_cloud_touched(min_points=2),
            raised(full.append_cloud_touched), full.close()]
    for x in [b, fe, vc, vs] + maps + dsts:
        x.close()
    return out


def history_buffer_batch_one_slot(lib):
    return _history_batch(lib, 1)


def history_buffer_batch_two_slots(lib):
    return _history_batch(lib, 2)


def full_map_slot_before_an_append(lib):
    b = api.History_buffer_batch(1)
    out = [raised(b.full_map(0).append_cloud_touched), b.cell_map(0, 0).resolution, b.cell_map(0, 2).resolution]
    b.close()
    return out


def cell_map(lib):
    a, d = api.Cell_map(max_points=8, resolution=0.5, minimum_revisit_threshold=9), api.Cell_map(4)
    out = [a.owned, a.resolution, a.max_points, a.reserve(6), a.reserve(20), a.max_points, a.append_cloud(cloud(3)),
           a.extract_cells([], d), a.extract_cells([[1, 2, 3], [4, 5, 6]], d)]
    lib.answer("ll_cellmap_extract_cells", out={5: 30})
    out += [a.extract_cells([[1, 2, 3]], d), d.max_points, a.append_cloud_touched(cloud(3)), a.append_cloud_touched(np.zeros((0, 4)), 2)]
    lib.answer("ll_cellmap_append_touched", out={6: 2})
    out += [a.append_cloud_touched(cloud(3)), a.stats(), a.dump(), a.features(), a.feature_clouds(), a.query_filter(IDENT, 5.0, 30.0, 0.4)]
    lib.answer("ll_cellmap_stats", out={1: 2, 2: 5, 3: 1})
    lib.answer("ll_cellmap_query_filter", out={6: 2, 7: 3})
    lib.answer("ll_cellmap_feature_clouds", out={3: 1, 6: 2})
    with fake_torch():
        out += [a.stats(), a.dump(), a.features(), a.feature_clouds(), a.query_filter(IDENT + 1, 5.0, 30.0, 0.4, 0), a.keyframe_images(),
                a.keyframe_images(0.5), a.device_view(), a.device_view(1)]
    a.close()
    d.close()
    return out


def scene_aligner(lib):
    sa, a, b = api.Scene_aligner(initial_points=32), api.Cell_map(8), api.Cell_map(8)
    out = [sa.run(a, b)]
    lib.answer("ll_scene_align_run", out={5: 0.75, 7: 2})
    out += [sa.run(b, a), sa.work()]
    for x in (sa, a, b):
        x.close()
    return out


def keyframe_bank(lib):
    kb, cm = api.Keyframe_bank(initial_entries=2), api.Cell_map(8)
    lib.answer("ll_keyframe_bank_size", ret=3)
    img = np.arange(3600, dtype=np.float32).reshape(60, 60)
    out = [len(kb), kb.add_cell_map(cm), kb.add_cell_map(cm, 0.5)]
    lib.answer("ll_keyframe_bank_add_images", out={3: 4})
    out += [kb.add_images(img, img + 1), raised(kb.add_images, img[:59], img), kb.images(1), kb.match([2, 3], [0, 1]), kb.match([], []),
            raised(kb.match, [1], []), kb.surface(2, 1, 1), kb.work()]
    kb.close()
    cm.close()
    return out


def map_refine(lib):
    mr, b = api.Map_refine(initial_points=64), api.History_buffer_batch(1)
    lib.answer("ll_map_refine_size", ret=2)
    out = [len(mr), mr.add_cloud(cloud(3)), mr.add_cloud(cloud(3), 0.25), mr.add_logged(b, [[5, 6], [], [7]]), mr.add_logged(b, [], 0.25),
           mr.add_logged(b, [[]]), raised(mr.add_logged, mr, [[1]]), mr.add_stored(cloud(2)), mr.cloud(0)]
    lib.answer("ll_map_refine_cloud", out={4: 3})
    out += [mr.cloud(1), mr.run([0, 1], poses(2), poses(2, 1.0)), mr.status, mr.run([1], poses(1), poses(1, 1.0), 0.5, True),
            raised(mr.run, [0, 1], poses(1), poses(2)), mr.refine([0, 1], poses(2), poses(2, 1.0)), mr.refine([], [], [], 0.5, True), mr.merge()]
    lib.answer("ll_map_refine_merge", out={2: 4, 3: 1})
    out += [mr.merge(0.5), mr.merge_status, mr.work()]
    mr.close()
    b.close()
    return out


def pose_graph(lib):
    chain = dict(poses=poses(3), ab=[[0, 1], [1, 2]], meas=poses(2, 1.0))
    loop = dict(poses=poses(4), ab=[[0, 1], [1, 2], [2, 3], [3, 0]], meas=poses(4, 1.0), information=np.tile(2.0 * np.eye(6).ravel(), (4, 1)))
    pg = api.Pose_graph(2, 8, 8, 16)
    out = [pg.capacity, api.Pose_graph.envelope_blocks(4, loop["ab"]), api.Pose_graph.envelope_blocks(1, []), pg.solve([]), pg.solve([chain]),
           pg.solve([chain, loop]), pg.capacity, raised(pg.solve, [dict(poses=poses(2), ab=[[0, 1]], meas=poses(2))]),
           raised(pg.solve, [dict(chain, information=np.zeros((1, 36)))]), pg.work()]
    pg.close()
    return out


def pose_graph_grows(lib):
    pg = api.Pose_graph(1, 2, 1, 1)
    first = pg.h.value
    out = [pg.capacity, pg.solve([dict(poses=poses(3), ab=[[0, 1], [1, 2]], meas=poses(2, 1.0))]), pg.capacity, first, pg.h.value]
    pg.close()
    return out


def map_buffer(lib):
    m = api.Map_buffer(device=1)
    lib.answer("ll_map_size", ret=3)
    lib.answer("ll_map_cells", ret=7)
    out = [m.setInputCloud(m.CORNER, cloud(4)), m.setInputCloud(m.SURF, cloud(4, 3), 0.5), m.size(0), m.cells(1), m.to_f16(1), m.dequantized(0),
           m.nearestKSearch(1, cloud(2, 3), 4.0), m.nearestKSearch_device(0, _Tensor(0x9000, (2, 3)), 4.0, _Tensor(0x9100, (2, 5)), _Tensor(0x9200, (2, 5)))]
    m.close()
    return out


def free_functions(lib):
    img = np.arange(3600, dtype=np.float32).reshape(60, 60)
    return [api.map_grid_geometry([0, 0, 0, 4, 5, 6], 0.5), api.map_refine_affine(IDENT, IDENT + 1), api.keyframe_similarity(img, img + 1, 1),
            raised(api.keyframe_similarity, img[:59], img), api.relative_constraint(IDENT, IDENT + 1),
            api.loop_constraint(3, 1, IDENT, IDENT + 1, [0, 0, 0, 1], [1, 2, 3])]


def _registration(lib, S):
    reg = api.Point_cloud_registration(max_scans=S, max_features=16, device=1)
    fe, sp, vc, vs = api.Livox_laser(max_points=16, max_scans=2 * S), api.Spinning_laser(max_points=16, max_scans=S), api.VoxelGrid(16, S), api.VoxelGrid(16, S)
    maps = [api.Map_buffer() for _ in range(S)]
    m, holes = maps[0], [None] + maps[1:]
    reg.params.icp_max_iterations = 7
    reg.m_pose_w_last, reg.m_pose_w_curr = IDENT + 1, IDENT + 2
    pl, pc = poses(S), poses(S, 1.0)
    ragged_c, ragged_s = [cloud(2 + i) for i in range(S)], [cloud(3 - i, first=1.0) for i in range(S)]
    out = [reg.find_out_incremental_transfrom(m, cloud(3), cloud(4)), reg.m_pose_w_curr, reg.m_para_buffer_incremental, reg.m_inlier_threshold,
           reg.solve_batch(m, ragged_c, ragged_s, pl, pc), reg.solve_batch(m, [np.zeros((0, 4))] * S, [np.zeros((0, 4))] * S, pl, pc),
           reg.upload_features(ragged_c, ragged_s),
           reg.enqueue_uploaded(m, S, pl, pc), reg.enqueue_fe(m, fe, S, pl, pc), reg.enqueue_fe_merged(m, fe, S, 2, pl, pc),
           reg.enqueue_fe_downsampled(m, fe, vc, vs, 0.2, 0.8, S, pl, pc),
           reg.enqueue_fe_maps(maps, fe, S, pl, pc), reg.enqueue_fe_maps(holes, fe, S, pl, pc, frame_index=list(range(3, 3 + S))),
           raised(reg.enqueue_fe_maps, maps + [None], fe, S, pl, pc),
           reg.enqueue_fe_downsampled_maps(maps, fe, vc, vs, 0.2, 0.8, S, pl, pc),
           reg.enqueue_fe_downsampled_maps(holes, fe, vc, vs, 0.2, 0.8, S, pl, pc, np.arange(S) + 5),
           reg.enqueue_spin(m, sp, S, pl, pc), reg.enqueue_spin_downsampled(m, sp, vc, vs, 0.2, 0.8, S, pl, pc),
           reg.collect(S), reg.solve_batch_fe(m, fe, S, pl.ravel(), pc.ravel()),
           reg.set_debug(), reg.debug_flags, reg.set_debug(True, no_knn_reuse=True, small_solver_waves=2, no_solve_order=True), reg.debug_flags,
           reg.set_debug_flags(5), reg.debug_flags, reg.set_debug_knn_iteration(3), reg.debug_knn(0, 2, 3), reg.set_profiling(), reg.set_profiling(False),
           reg.debug_worklists(), reg.debug_worklists(S), reg.debug_worklists_by_kind(), reg.debug_worklists_by_kind(S), reg.debug_cycles(),
           reg.debug_cycles(S - 1), reg.kernel_times(),
           reg.append_to_submap_device(fe, S, 1, np.ones(S, np.int32), pl, _Tensor(0x9000, (32, 4)), 4),
           reg.append_to_submap_device_spin(sp, S, 2, np.ones(S, np.int32), pl, _Tensor(0x9000, (32, 4)), 4),
           reg.pointcloudAssociateToMap(cloud(3)), reg.pointcloudAssociateToMap(cloud(3), IDENT + 3)]
    for x in [reg, fe, sp, vc, vs] + maps:
        x.close()
    return out


def point_cloud_registration_one_scan(lib):
    return _registration(lib, 1)


def point_cloud_registration_two_scans(lib):
    return _registration(lib, 2)


_MAPPING_ARGS = dict(scan_points=32, init_accumulate_frames=5, icp_max_iterations=7, ceres_max_iterations=30, max_allow_incre_R=1.5, max_allow_incre_T=0.75,
                     max_allow_final_cost=9.0, minimum_icp_R_diff=0.02, minimum_icp_T_diff=0.03)


def mapping_registrar_parameters(lib):
    """Laser_mapping and Laser_mapping_batch set the registrar's parameters from the same arguments"""
    out = []
    for extra in (dict(), dict(maximum_residual_blocks=200, subsample_seed=4)):
        for lm in (mapping.Laser_mapping(**_MAPPING_ARGS, **extra), mapping.Laser_mapping_batch(2, batched_history=True, **_MAPPING_ARGS, **extra)):
            out.append([type(lm).__name__, lm.reg.params])
            lm.close()
    return out


CASES = {f.__name__: f for f in (
    livox_laser, spinning_laser, voxel_grid, history_buffer, history_buffer_map_cloud_negative, history_buffer_batch_one_slot,
    history_buffer_batch_two_slots, full_map_slot_before_an_append, cell_map, scene_aligner, keyframe_bank, map_refine, pose_graph,
    pose_graph_grows, map_buffer, free_functions, point_cloud_registration_one_scan, point_cloud_registration_two_scans,
    mapping_registrar_parameters)}


def run(name: str, install) -> dict:
    """one case on a fresh stand-in; install( lib ) puts it in capi's place (monkeypatch.setattr in the tests)"""
    lib = Recording_library()
    install(lib)
    returns = plain(CASES[name](lib))
    return {"calls": lib.calls, "returns": returns}


def record(path: str) -> None:
    saved = capi._lib
    try:
        out = {name: run(name, lambda lib: setattr(capi, "_lib", lib)) for name in CASES}
    finally:
        capi._lib = saved
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    record(sys.argv[1])
