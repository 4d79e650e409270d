"""What the map-refinement tests share (tests/test_map_refine_host.py, tests/test_gpu_map_refine.py): the numpy restatement of
refine_pts (ceres_pose_graph_3d.hpp:444-449), the ragged set of key-frame clouds, seeded poses, and the expected outputs -- the oracle's
VoxelGrid composed with the numpy move.  Nothing here reads the reference."""
import numpy as np

from oracle import orc

ADD_LEAF, RUN_LEAF = 0.5, 0.2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rotation_np(q):
    """Eigen's toRotationMatrix for {x, y, z, w} in float64, as it stands (no renormalisation)"""
    x, y, z, w = (np.float64(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]], np.float64)


def affine_np(ori7, opm7):
    """(R_aff float32[3, 3], T_aff float32[3]): R_aff = float( R_opm R_ori^T ), double products reduced ( e0 + e1 ) + e2;
    T_aff = float( double( R_aff ) ( -t_ori ) + t_opm )"""
    ori7, opm7 = np.asarray(ori7, np.float64), np.asarray(opm7, np.float64)
    Ro, Rp = rotation_np(ori7[:4]), rotation_np(opm7[:4])
    R = np.zeros((3, 3), np.float32)
    for r in range(3):
        for c in range(3):
            e = Rp[r] * Ro[c]
            R[r, c] = np.float32((e[0] + e[1]) + e[2])
    Rd, nt = R.astype(np.float64), -ori7[4:]
    T = np.zeros(3, np.float32)
    for r in range(3):
        e = Rd[r] * nt
        T[r] = np.float32(((e[0] + e[1]) + e[2]) + opm7[4 + r])
    return R, T


def move_np(R, T, xyz):
    """out_i = ( R_i0 x + ( R_i1 y + R_i2 z ) ) + T_i in float32, for xyz [n, >= 3]; returns [n, 4] with intensity 0"""
    p = np.ascontiguousarray(xyz, np.float32)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out = np.zeros((len(p), 4), np.float32)
    with np.errstate(all="ignore"):
        for i in range(3):
            out[:, i] = (R[i, 0] * x + (R[i, 1] * y + R[i, 2] * z)) + T[i]
    return out


def filtered(cloud, leaf):
    """(status, what pcl::VoxelGrid leaves of cloud): status 1 hands the input back, status 2 nothing"""
    cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
    if len(cloud) == 0:
        return 2, cloud
    st, out = orc.voxel_grid(cloud, leaf)
    if st == 1:
        return 1, cloud
    return st, out


def expected(stored, ori7, opm7, leaf=RUN_LEAF, transform_first=False):
    """(status, cloud) of one selection: mode 0 = filter, then move; mode 1 = move, then filter"""
    R, T = affine_np(ori7, opm7)
    if transform_first:
        return filtered(move_np(R, T, stored), leaf)
    st, f = filtered(stored, leaf)
    return st, move_np(R, T, f)


def poses(n, seed, far=0.0):
    """n seeded pose pairs: an original pose and a corrected one a few decimetres and degrees off it, `far` metres out along x and y"""
    rng = np.random.default_rng(seed)
    ori, opm = np.zeros((n, 7)), np.zeros((n, 7))
    for out, scale in ((ori, 1.0), (opm, 0.0)):
        q = rng.normal(0, 1, (n, 4)) if scale else ori[:, :4] + rng.normal(0, 0.02, (n, 4))
        out[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True)
        out[:, 4:] = (rng.uniform(-20, 20, (n, 3)) if scale else ori[:, 4:] + rng.normal(0, 0.3, (n, 3)))
    ori[:, 4:6] += far
    opm[:, 4:6] += far
    return ori, opm


SIZES = [0, 1, 3, 63, 64, 65, 255, 256, 257, 1000, 5000]


def raw_clouds(seed=5, centre=(0.0, 0.0, 0.0)):
    """[(name, raw cloud [n, 4], leaf of its add)]: the sizes of SIZES seeded in a 20 m box; 3000 points inside one 0.2 m voxel among 500
    others (added at 1 mm: 8001^3 > 2^31, the add hands the cloud back, and the 3000 lie on both sides of a 2048-point chunk boundary
    whatever their order);
    ten non-finite points; three corners of a 300 m cube (filtered at 0.5 m: 601^3 < 2^31, handed back at 0.2 m: 1501^3 > 2^31); three
    corners of a 700 m cube (handed back at the add: 1401^3 > 2^31)"""
    rng = np.random.default_rng(seed)
    c = np.array([*centre, 0.0], np.float32)
    out = []
    for n in SIZES:
        p = rng.uniform(-10, 10, (n, 4)).astype(np.float32)
        p[:, 3] = rng.uniform(0, 255, n)
        out.append((f"box{n}", p + c, ADD_LEAF))
    cluster = np.zeros((3500, 4), np.float32)
    cluster[:3000, :3] = rng.uniform(0.01, 0.19, (3000, 3)) + np.array([3.0, -2.0, 1.0])
    cluster[3000:, :3] = rng.uniform(-4, 4, (500, 3))
    cluster[:, 3] = rng.uniform(0, 255, 3500)
    out.append(("one_voxel", rng.permutation(cluster) + c, 0.001))
    out.append(("non_finite", np.full((10, 4), np.nan, np.float32), ADD_LEAF))
    cube = np.array([[0, 0, 0, 1], [300, 300, 300, 2], [300, 0, 300, 3]], np.float32)
    out.append(("cube300", cube + c, ADD_LEAF))
    out.append(("cube700", cube * np.array([7 / 3, 7 / 3, 7 / 3, 1], np.float32) + c, ADD_LEAF))
    return out


def stored_clouds(raw):
    """[(status of the add, the cloud the store holds)] of raw_clouds' entries"""
    return [filtered(p, leaf) for _, p, leaf in raw]
