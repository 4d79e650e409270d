"""-m gpu: the late ICP iterations' tile search of the unsettled surface queries alone (ll_knn_kernels.hip: reg_knn_classify_kernel +
reg_knn_tile_kernel<true, KT_SPARSE>, from ICP iteration LL_KNN_SPARSE_FROM on) against the tile search of every query in every
iteration (debug switch no_knn_sparse) and against the per-lane search (no_knn_tile): pose bits, reports, and what the solver reads
of every slot after the last iteration -- neighbour record and block flag (Point_cloud_registration.debug_blocks).

Batches: 17 scans (the size from which the tile search is the default) and 2 scans with knn_tile_small_batches; scans thinned to just
above LL_KNN_TILE_MIN_SURF = 1024 surface features (a list of a few dozen entries, less than one wavefront, a scan of five workgroups)
plus one full scan (lists of several wavefronts from several classification workgroups)."""
import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.api import Map_buffer, Point_cloud_registration
from tests.conftest import oracle_features

pytestmark = pytest.mark.gpu
ICP = 10
SPARSE_FROM = 4  # LL_KNN_SPARSE_FROM (ll_device.h)


@pytest.fixture(scope="module")
def dev_map(gpu_lib, small_world):
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, small_world["corner"])
    m.setInputCloud(Map_buffer.SURF, small_world["surf"])
    yield m
    m.close()


@pytest.fixture(scope="module")
def batch(scans):
    """per distinct scan: (corner features, surface features thinned to just above 1024); index 0 keeps every feature"""
    out = []
    for k, sc in enumerate(scans):
        _, _, _, _, fc, fs = oracle_features(sc)
        if k > 0:
            fs = fs[::max(1, len(fs) // 1025)]
            assert 1024 < len(fs) < 1300
        out.append((np.ascontiguousarray(fc), np.ascontiguousarray(fs)))
    return out


@pytest.fixture(scope="module")
def batch_full(scans):
    """every scan with all of its features (~17 k surface queries each)"""
    return [tuple(np.ascontiguousarray(f) for f in oracle_features(sc)[4:6]) for sc in scans]


def run(dev_map, batch, n, poses, kw, force=1, subsample=None):
    reg = Point_cloud_registration(max_scans=n, max_features=24000)
    reg.set_debug(False, **kw)
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = ICP, 20, force
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    if subsample:
        p.maximum_allow_residual_block, p.subsample_seed = subsample
    fcs = [batch[i % len(batch)][0] for i in range(n)]
    fss = [batch[i % len(batch)][1] for i in range(n)]
    res, pc, pi, reps = reg.solve_batch(dev_map, fcs, fss, poses, poses)
    blocks = [reg.debug_blocks(i, len(fcs[i]), len(fss[i])) for i in range(n)]
    listed = reg.debug_worklists_by_kind(n)[0][1]  # sum over scans and sparse iterations of the list lengths
    out = dict(res=res.copy(), pc=pc.copy(), pi=pi.copy(), reps=[bytes(r) for r in reps], blocks=blocks, listed=listed,
               surf=sum(len(f) for f in fss), iters=[r.icp_iterations for r in reps])
    reg.close()
    return out


def same(a, b):
    assert np.array_equal(a["res"], b["res"]) and a["pc"].tobytes() == b["pc"].tobytes() and a["pi"].tobytes() == b["pi"].tobytes()
    assert a["reps"] == b["reps"]


def same_blocks(a, b, found_only=False):
    """every slot's neighbour record and flag; found_only: the three positions only where five neighbours were found (the solver reads
    no others) -- a query with fewer keeps the positions of a partial list after a search and -1 after a re-sort of the reuse lists"""
    for i, (x, y) in enumerate(zip(a["blocks"], b["blocks"])):
        for nn, flag in ((0, 1), (2, 3)):
            assert np.array_equal(x[flag], y[flag]), (i, flag)
            assert np.array_equal(x[nn][:, 3], y[nn][:, 3]), (i, nn)
            keep = x[nn][:, 3] == 1 if found_only else slice(None)
            assert np.array_equal(x[nn][keep], y[nn][keep]), (i, nn)


def modes(n):
    small = {"knn_tile_small_batches": True} if n <= 16 else {}
    return small, dict(small, no_knn_sparse=True), {"no_knn_tile": True}


def guesses(scans, n, kind, rng):
    out = []
    for i in range(n):
        sc = scans[i % len(scans)]
        if kind == "init":
            out.append(sc.pose_init)
        elif kind == "true":
            out.append(sc.pose_true)
        else:  # far off: every query leaves every budget in every iteration (the speed bound keeps the steps large to the end)
            out.append(synth.pose_compose(sc.pose_true, np.r_[synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(8.0)), rng.uniform(0.8, 1.2, 3)]))
    return np.stack(out)


@pytest.mark.parametrize("n", [17, 2])
@pytest.mark.parametrize("guess", ["init", "true", "far"])
def test_sparse_tile_search_changes_nothing(dev_map, scans, batch, n, guess):
    poses = guesses(scans, n, guess, np.random.default_rng(5))
    sparse, dense, lane = (run(dev_map, batch, n, poses, kw) for kw in modes(n))
    same(sparse, dense)
    same(sparse, lane)
    same_blocks(sparse, dense)
    same_blocks(sparse, lane, found_only=True)
    assert dense["listed"] == 0
    sparse_iters = ICP - SPARSE_FROM
    assert sparse["listed"] <= sparse_iters * sparse["surf"]
    print(f"n={n} guess={guess}: listed {sparse['listed']} of {sparse_iters * sparse['surf']} query-iterations")
    if guess == "init":
        assert 0 < sparse["listed"] < sparse_iters * sparse["surf"]  # the path was taken, and it left queries out
    if guess == "true":
        assert sparse["listed"] < 0.5 * sparse_iters * sparse["surf"]


@pytest.mark.parametrize("n,unit", [(20, 64), (10, 32)])
def test_units_of_64_and_32_entries(dev_map, scans, batch_full, n, unit):
    """The sparse launch packs 64 list entries into a wavefront when the batch lists at least 64 x 4 096 of them, 32 from 32 x 4 096,
    else 16 (KT_SPARSE_WAVES, ll_knn_kernels.hip).  Full scans from a guess so far off that nearly every query is listed in every
    iteration (~14.9 k per scan): 20 scans reach the first size, 10 the second (the batches above stay at 16 entries)."""
    poses = guesses(scans, n, "far", np.random.default_rng(6))
    sparse, dense, _ = (run(dev_map, batch_full, n, poses, kw) if k < 2 else None for k, kw in enumerate(modes(n)))
    same(sparse, dense)
    same_blocks(sparse, dense)
    per_iteration = sparse["listed"] / (ICP - SPARSE_FROM)
    print(f"n={n}: {per_iteration:.0f} entries listed per iteration")
    assert unit * 4096 <= per_iteration < 2 * unit * 4096


def test_scans_that_finish_early(dev_map, scans, batch):
    """force_all_iterations = 0: scans leave the loop at their own iteration -- before the records exist, between the record
    iteration and the first sparse one, or later -- and every launch skips them from then on"""
    n = 17
    poses = guesses(scans, n, "init", None)
    poses[1::2] = guesses(scans, n, "true", None)[1::2]
    sparse, dense, lane = (run(dev_map, batch, n, poses, kw, force=0) for kw in modes(n))
    same(sparse, dense)
    same(sparse, lane)
    same_blocks(sparse, dense)
    print("ICP iterations per scan:", sparse["iters"])
    assert min(sparse["iters"]) < ICP


def test_subsampling_switches_the_mode_off(dev_map, scans, batch):
    """a13 with a seed: the skipped features change from iteration to iteration, so a query's list changes without the query
    moving; the registrar searches every query in every iteration, whatever the switch says"""
    n = 17
    poses = guesses(scans, n, "init", None)
    sparse, dense, lane = (run(dev_map, batch, n, poses, kw, subsample=(3000, 11)) for kw in modes(n))
    assert sparse["listed"] == 0
    same(sparse, dense)
    same(sparse, lane)
    same_blocks(sparse, dense)
