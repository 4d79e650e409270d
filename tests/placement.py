"""Where the world sits: rigid placements of the test world far from the origin, stray points that coarsen the search grid, and the plain
restatement of the grid geometry (ll_map_kernels.hip map_grid_geometry).  A plain module shared by tests/test_placement_host.py (CPU tier) and
tests/test_gpu_placement.py (GPU tier).

synth.make_maps( 200_000 ) is axis-aligned rooms in [0, 90] x [0, 90] x [0, 4] m.  A placement P = (q, t) moves map and poses alike; the
placed map IS the test's input (rotated and translated in fp64, rounded to fp32 once), so device and oracle receive the same floats."""
import math

import numpy as np

from loam_livox_amd import synth

PLACEMENTS = {
    # every axis changes sign inside the map; axis-aligned on purpose, so walls and cell faces meet at 0
    "straddle": np.r_[synth.quat_from_rpy(0.0, 0.0, 0.0), [-45.0, -45.0, -2.0]],
    # kilometre coordinates, walls not parallel to the grid
    "km": np.r_[synth.quat_from_rpy(np.deg2rad(3.0), 0.0, np.deg2rad(37.0)), [-4321.0, 987.0, -55.0]],
    # one fp32 ulp is 4 mm
    "far": np.r_[synth.quat_from_rpy(np.deg2rad(3.0), 0.0, np.deg2rad(-115.0)), [52000.0, -31000.0, 120.0]],
}

# stray points (a range glitch carried into the map), appended BEHIND a cloud so that original indices do not move; with the 200 k-point
# surface map and cells of 1 m they give: cell edge 25.63 m, grid 7804 x 7808 x 1 / 129.7 m, 463 x 463 x 463 / 1.5 m, nx = 666 667
STRAYS = {
    "two_axes": np.array([[2e5, 45.0, 2.0], [45.0, -2e5, 2.0]], np.float32),
    "diagonal": np.array([[3e4, 3e4, 3e4], [-3e4, -3e4, -3e4]], np.float32),
    "wide_x": np.array([[1e6, 45.0, 2.0]], np.float32),
}


def place_points(P, xyz_or_xyzi):
    """the cloud moved by P: rotated and translated in fp64, rounded to fp32 ONCE; further columns (intensity) are kept"""
    a = np.asarray(xyz_or_xyzi)
    out = np.array(a, np.float32, copy=True)
    out[:, :3] = (a[:, :3].astype(np.float64) @ synth.quat_to_mat(P[:4]).T + P[4:]).astype(np.float32)
    return np.ascontiguousarray(out)


def place_pose(P, pose):
    return synth.pose_compose(P, np.asarray(pose, np.float64))


def with_strays(cloud, strays):
    """the strays appended behind the cloud's xyz columns"""
    return np.ascontiguousarray(np.concatenate([np.asarray(cloud, np.float32)[:, :3], strays]), np.float32)


def plain_geometry(mm, cell):
    """map_grid_geometry restated: float32 where the library computes in float, double where it computes in double"""
    f = np.float32
    mm = [f(x) for x in mm]
    if not (mm[0] <= mm[3]):
        mm = [f(0)] * 6
    h = f(cell)
    while True:
        dims = [math.floor(float(f(mm[3 + d] - mm[d])) / float(h)) + 1 for d in range(3)]
        if float(dims[0]) * dims[1] * dims[2] <= float(1 << 27):
            break
        h = f(h * f(1.5))
    ext = f(max(abs(x) for x in mm) + max(f(mm[3 + d] - mm[d]) for d in range(3)))
    slack = f(f(f(1e-3) * h) + f(f(2e-6) * ext))
    return tuple(int(d) for d in dims), h, slack


def coarsened_cell(points, cell):
    """(cell edge, (nx, ny, nz)) of the search grid the library builds over `points` when asked for cells of `cell` metres: the edge grows by
    1.5 until the dense table holds at most 2^27 cells"""
    p = np.asarray(points, np.float32)[:, :3]
    p = p[np.isfinite(p).all(axis=1)]
    mm = np.r_[p.min(axis=0), p.max(axis=0)] if len(p) else np.array([np.inf] * 3 + [-np.inf] * 3, np.float32)
    dims, h, _ = plain_geometry(mm, cell)
    return float(h), dims


def box_queries(points, n=200, margin=8.0, seed=3):
    """n points in the cloud's bounding box grown by `margin` metres, all of them OUTSIDE the box itself"""
    p = np.asarray(points, np.float32)[:, :3]
    lo, hi = p.min(axis=0).astype(np.float64), p.max(axis=0).astype(np.float64)
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        q = rng.uniform(lo - margin, hi + margin, (4 * n, 3))
        q = q[((q < lo) | (q > hi)).any(axis=1)]
        out.extend(q[:n - len(out)])
    return np.asarray(out, np.float64).astype(np.float32)


def stray_queries(strays):
    """0.3 m from each stray, and one point 1e5 m out on the x axis of the un-placed world"""
    s = np.asarray(strays, np.float64)
    return np.concatenate([s + np.array([0.3, 0.0, 0.0]), [[1e5, 44.0, 2.0]]]).astype(np.float32)


def search_queries(pose, features, cloud, seed=3):
    """the queries of the search tests: the features moved by `pose`, 200 points up to 8 m outside the cloud's bounding box, and 50 points of
    the cloud itself"""
    rng = np.random.default_rng(seed + 1)
    own = np.asarray(cloud, np.float32)[rng.choice(len(cloud), 50, replace=False), :3]
    return np.ascontiguousarray(np.concatenate([synth.transform_points(pose, np.asarray(features)[:, :3]), box_queries(cloud, 200, 8.0, seed), own]),
                                np.float32)


def knn_within(tree, q, max_d2):
    """the k-d tree's five neighbours as the grid searches report them: -1 / inf beyond the radius"""
    oi, od = tree.knn(q, 5)
    inside = od < max_d2
    return np.where(inside, oi, -1), np.where(inside, od, np.inf).astype(np.float32)
