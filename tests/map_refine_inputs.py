"""What the map-refinement tests share (tests/test_map_refine_host.py, tests/test_gpu_map_refine.py): the numpy restatement of
refine_pts (ceres_pose_graph_3d.hpp:444-449), the ragged set of key-frame clouds, the sets for the points where the device chain changes
form (many_selections, last_voxel_at_the_end), seeded poses, and the expected outputs -- the oracle's VoxelGrid composed with the numpy
move.  Nothing here reads the reference."""
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


IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])    # the pose whose pair gives R_aff = I and T_aff = 0 exactly
N_MANY, N_TINY = 600, 48
TINY_FEW = (1, 2, 3, 6, 7, 8)                                # tiny clouds of 1, 2, 3, 1, 2, 3 points
PACKED_AT = np.array([3.0, -2.0, 1.0], np.float32)           # lower corner of the 0.2 m voxel that rows 2040-2055 of a chunk-sized cloud fill
MANY_EMPTY, MANY_CUBE, MANY_NAN, MANY_2048, MANY_2049, MANY_4096 = (N_TINY + k for k in range(6))
MANY_CHUNK_AT = {60: MANY_2048, 330: MANY_2049, 599: MANY_4096}   # selection -> chunk-sized cloud, once each
MANY_FEW_AT = range(300, 316)                                # the stretch of 16 consecutive selections of 1-3 points


def many_selections(seed):
    """(store, ids, ori, opm): a store to go in through add_stored -- kept as given, non-finite rows included -- and N_MANY selections of it.
    Store: N_TINY clouds of 1-70 points in a 2 m box, every fifth with about 30 % of its rows non-finite in one coordinate (its first row
    stays finite) and those of TINY_FEW of 1-3 points; an empty cloud; three corners of a 300 m cube (1501^3 > 2^31 leaves at 0.2 m: handed
    back); nine all-NaN rows; clouds of exactly MR_CHUNK, MR_CHUNK + 1 and 2 MR_CHUNK finite points in a 20 m box, rows 2040-2055 of the
    last two inside the one voxel at PACKED_AT -- on both sides of a work-item bound.
    ids: tiny clouds drawn at random, duplicates wanted; 254-257 and 511-513 empty, all-NaN and handed-back entries with a handed-back one
    at 255 and at 512, the last slot of a 256-selection trip of mr_offsets_kernel and the first of the next -- there alone the trip's two
    carried sums differ; one more handed-back entry mid-trip at 100; MANY_FEW_AT; MANY_CHUNK_AT.  Poses: poses(N_MANY, seed)."""
    rng = np.random.default_rng(seed)
    store = []
    for k in range(N_TINY):
        n = 1 + TINY_FEW.index(k) % 3 if k in TINY_FEW else int(rng.integers(4, 71))
        p = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
        p[:, 3] = rng.uniform(0, 255, n)
        if k % 5 == 0:
            bad = rng.random(n) < 0.3
            bad[0], bad[-1] = False, True
            p[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        store.append(p)
    store.append(np.zeros((0, 4), np.float32))
    store.append(np.array([[0, 0, 0, 1], [300, 300, 300, 2], [300, 0, 300, 3]], np.float32))
    store.append(np.full((9, 4), np.nan, np.float32))
    for n in (2048, 2049, 4096):
        p = rng.uniform(-10, 10, (n, 4)).astype(np.float32)
        p[:, 3] = rng.uniform(0, 255, n)
        if n > 2048:
            p[2040:2056, :3] = PACKED_AT + rng.uniform(0.02, 0.18, (len(p[2040:2056]), 3)).astype(np.float32)
        store.append(p)
    ids = [int(i) for i in rng.integers(0, N_TINY, N_MANY)]
    for s, cid in zip((254, 255, 256, 257, 511, 512, 513, 100), (MANY_EMPTY, MANY_CUBE, MANY_NAN, MANY_EMPTY, MANY_NAN, MANY_CUBE, MANY_EMPTY, MANY_CUBE)):
        ids[s] = cid
    for k, s in enumerate(MANY_FEW_AT):
        ids[s] = TINY_FEW[k % len(TINY_FEW)]
    for s, cid in MANY_CHUNK_AT.items():
        ids[s] = cid
    ori, opm = poses(N_MANY, seed)
    return store, ids, ori, opm


def finite_count(cloud):
    return int(np.isfinite(np.asarray(cloud)[:, :3]).all(axis=1).sum())


def selections_in_a_wavefront(counts):
    """the most selections that one aligned window of 64 sorted positions holds points of, for selections of `counts` valid points laid
    end to end in selection order -- as the sort lays them"""
    at, seen = 0, {}
    for c in counts:
        if c > 0:
            for w in range(at // 64, (at + c - 1) // 64 + 1):
                seen[w] = seen.get(w, 0) + 1
        at += c
    return max(seen.values(), default=0)


def expected_run(store, ids, ori, opm, leaf=RUN_LEAF):
    """transform_first -> [(status, cloud) per selection] of a run, from the oracle"""
    return {tf: [expected(store[cid], ori[s], opm[s], leaf, tf) for s, cid in enumerate(ids)] for tf in (False, True)}


def many_conditions(store, ids, want):
    """What the many_selections tests rest on, asserted on the inputs and on the oracle's results `want` (one mode of expected_run) alone:
    a run that passes them cannot equal the oracle for the wrong reason.  Returns the figures."""
    st = [w[0] for w in want]
    assert len(ids) == N_MANY and set(st) == {0, 1, 2}
    assert [st[s] for s in (255, 512)] == [1, 1] and [st[s] for s in (254, 256, 257, 511, 513)] == [2] * 5
    assert st[258] == 0 and st[514] == 0 and len(want[258][1]) >= 1 and len(want[514][1]) >= 1
    # the sorted valid positions: the finite points of the status-0 selections, in selection order
    valid = [finite_count(store[cid]) if st[s] == 0 else 0 for s, cid in enumerate(ids)]
    in_window = selections_in_a_wavefront(valid)
    assert in_window >= 8
    mixed = sum(st[s] == 0 and 0 < finite_count(store[cid]) < len(store[cid]) for s, cid in enumerate(ids))
    assert mixed >= 20
    for s, cid in MANY_CHUNK_AT.items():
        assert ids[s] == cid and ids.count(cid) == 1 and st[s] == 0
    assert [len(store[c]) for c in (MANY_2048, MANY_2049, MANY_4096)] == [2048, 2049, 4096]
    return dict(status=[st.count(v) for v in (0, 1, 2)], in_window=in_window, mixed=mixed, points=sum(len(store[c]) for c in ids), valid=sum(valid))


def in_voxel(cloud, corner, leaf=RUN_LEAF):
    """the rows of cloud inside the voxel whose lower corner is `corner`"""
    d = np.asarray(cloud)[:, :3] - corner
    with np.errstate(invalid="ignore"):
        return np.all((d >= 0) & (d < leaf), axis=1)


def packed_voxel_is_one_point(store):
    """from the inputs and the oracle: rows 2040-2055 of the 2049- and 4096-point clouds lie in the voxel at PACKED_AT, on both sides of
    the work-item bound at MR_CHUNK, and the filter leaves one point of that voxel"""
    for cid in (MANY_2049, MANY_4096):
        packed = in_voxel(store[cid], PACKED_AT)
        assert packed[2040:min(2056, len(packed))].all() and packed[:2048].any() and packed[2048:].any()
        assert in_voxel(filtered(store[cid], RUN_LEAF)[1], PACKED_AT).sum() == 1


LAST_VOXEL_AT = np.array([5.0, 5.0, 5.0], np.float32)   # lower corner of the packed voxel of last_voxel_at_the_end: the box ends there


def last_voxel_at_the_end(cnt, seed=71):
    """a store of two all-finite clouds of a few hundred points in a 10 m box; the second holds cnt more points inside the one 0.2 m voxel
    at the box's maximum corner, anywhere among its rows.  That voxel has the highest leaf index of the second cloud, so in a run over
    [0, 1] that moves nothing, or filters first, its cnt keys are the last of the sorted keys: no sentinel follows them."""
    rng = np.random.default_rng(seed)
    store = []
    for n, extra in ((300, 0), (417, cnt)):
        p = rng.uniform(-5, 5, (n + extra, 4)).astype(np.float32)
        p[n:, :3] = LAST_VOXEL_AT + rng.uniform(0.02, 0.18, (extra, 3)).astype(np.float32)
        p[:, 3] = rng.uniform(0, 255, n + extra)
        store.append(rng.permutation(p))
    return store
