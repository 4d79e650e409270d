"""-m gpu: device VoxelGrid (through the C ABI) against the oracle -- bit-exact: the leaf of every point is integer
work, and the centroid sums run in the same (input) order in float."""
import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.api import Livox_laser, Map_buffer, Point_cloud_registration, VoxelGrid
from oracle import orc
from tests.conftest import oracle_features

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("n,span,leaf", [(24000, 30.0, 0.4), (24000, 30.0, 0.1), (5000, 8.0, (0.2, 0.4, 0.8)), (1, 1.0, 0.4),
                                         (100000, 200.0, 0.5), (7, 0.01, 1.0)])
def test_filter_bit_exact_vs_oracle(gpu_lib, n, span, leaf):
    rng = np.random.default_rng(n)
    p = rng.uniform(-span, span, (n, 4)).astype(np.float32)
    p[rng.random(n) < 0.01, rng.integers(0, 3)] = np.nan
    vg = VoxelGrid(max_points=100000)
    vg.setLeafSize(*np.broadcast_to(np.asarray(leaf, np.float32), (3,)))
    vg.setInputCloud(p)
    out = vg.filter()
    st, ref = orc.voxel_grid(p, leaf)
    assert vg.status == st == 0 and out.shape == ref.shape and np.array_equal(bits(out), bits(ref))
    vg.close()


def test_edge_cases(gpu_lib):
    vg = VoxelGrid(max_points=1000)
    vg.setLeafSize(1.0, 1.0, 1.0)
    # order-sensitive float sum, -0/+0, exact leaf boundaries
    a, b, c = np.float32(1e8), np.float32(-1e8), np.float32(0.3)
    p = np.array([[0.1, 0.1, 0.1, a], [0.2, 0.2, 0.2, b], [0.3, 0.3, 0.3, c], [1.0, 0, 0, 1], [0.99999994, 0, 0, 1], [-0.0, 0, 0, 5]], np.float32)
    for perm in ([0, 1, 2, 3, 4, 5], [2, 1, 0, 5, 4, 3]):
        vg.setInputCloud(p[perm])
        out = vg.filter()
        st, ref = orc.voxel_grid(p[perm], 1.0)
        assert np.array_equal(bits(out), bits(ref))
    # no finite point / empty input
    vg.setInputCloud(np.full((5, 4), np.nan, np.float32))
    assert vg.filter().shape == (0, 4) and vg.status == 2
    vg.setInputCloud(np.zeros((0, 4), np.float32))
    assert vg.filter().shape == (0, 4) and vg.status == 2
    # leaf too small for the extent: PCL copies the input
    rng = np.random.default_rng(1)
    q = rng.uniform(-100, 100, (50, 4)).astype(np.float32)
    q[3, 1] = np.nan
    vg.setLeafSize(0.01, 0.01, 0.01)
    vg.setInputCloud(q)
    out = vg.filter()
    assert vg.status == 1 and np.array_equal(bits(out), bits(q))
    # errors are reported, not fatal
    with pytest.raises(Exception):
        vg.setLeafSize(0.0, 1.0, 1.0); vg.filter()
    with pytest.raises(Exception):
        vg.setLeafSize(1.0, 1.0, 1.0); vg.setInputCloud(np.zeros((2000, 4), np.float32)); vg.filter()
    vg.close()


def test_batch_of_ragged_clouds(gpu_lib):
    rng = np.random.default_rng(5)
    B, stride = 7, 6000
    n = np.array([6000, 0, 1, 3333, 5999, 17, 6000], np.int32)
    clouds = rng.uniform(-15, 15, (B, stride, 4)).astype(np.float32)
    clouds[2, 0, 0] = np.nan          # its only point is invalid -> empty
    clouds[6] *= 1e4                  # 300 km extent at leaf 0.3: too many leafs -> pass-through
    vg = VoxelGrid(max_points=stride, max_clouds=B)
    vg.setLeafSize(0.3, 0.3, 0.3)
    out, n_out, st = vg.filter_batch(clouds, n)
    for b in range(B):
        s, ref = orc.voxel_grid(clouds[b, :n[b]], 0.3)
        assert st[b] == s and n_out[b] == len(ref)
        assert np.array_equal(bits(out[b, :n_out[b]]), bits(ref))
    assert list(st) == [0, 2, 2, 0, 0, 0, 1]
    # run to run identical
    out2, n_out2, _ = vg.filter_batch(clouds, n)
    assert np.array_equal(n_out, n_out2) and np.array_equal(bits(out), bits(out2))
    vg.close()


def test_one_workgroup_path_equals_the_kernel_pipeline(gpu_lib, monkeypatch):
    """up to 16 clouds of up to 24 576 points are filtered by one workgroup each (vox_block_kernel: block radix sort in LDS);
    everything else, and every cloud when LL_VOXEL_GENERAL_PATH is set at creation, by the multi-kernel pipeline: same bits"""
    rng = np.random.default_rng(9)
    cases = []
    for stride, B in ((300, 1), (4096, 3), (4097, 2), (8192, 16), (24000, 2), (24576, 1)):
        n = rng.integers(0, stride + 1, B).astype(np.int32)
        n[0] = stride
        clouds = rng.uniform(-20, 20, (B, stride, 4)).astype(np.float32)
        clouds[rng.random((B, stride)) < 0.01, 1] = np.inf
        cases.append((stride, B, n, clouds))
    # strides one past the 8-item and the 24-item instantiation (24 577: past the one-workgroup filter altogether), and one batch whose
    # sizes sit on either side of the bounds between the instantiations
    for stride, B, sizes in ((8193, 2, None), (24577, 1, None), (8193, 4, [4096, 4097, 8192, 8193])):
        n = rng.integers(0, stride + 1, B).astype(np.int32)
        n[0] = stride
        if sizes is not None:
            n = np.array(sizes, np.int32)
        clouds = rng.uniform(-20, 20, (B, stride, 4)).astype(np.float32)
        clouds[rng.random((B, stride)) < 0.01, 1] = np.inf
        cases.append((stride, B, n, clouds))
    outs = []
    for general in (False, True):
        if general:
            monkeypatch.setenv("LL_VOXEL_GENERAL_PATH", "1")
        res = []
        for stride, B, n, clouds in cases:
            vg = VoxelGrid(max_points=stride, max_clouds=B)
            vg.setLeafSize(0.35, 0.5, 0.35)
            out, n_out, st = vg.filter_batch(clouds, n)
            res.append((n_out.copy(), st.copy(), [bits(out[b, :n_out[b]]).copy() for b in range(B)]))
            vg.close()
        outs.append(res)
    for a, b_ in zip(*outs):
        assert np.array_equal(a[0], b_[0]) and np.array_equal(a[1], b_[1])
        assert all(np.array_equal(x, y) for x, y in zip(a[2], b_[2]))
    s, ref = orc.voxel_grid(cases[4][3][0, :cases[4][2][0]], (0.35, 0.5, 0.35))
    assert np.array_equal(outs[0][4][2][0], bits(ref))
    for k in (6, 7, 8):
        stride, B, n, clouds = cases[k]
        for b in range(B):
            s, ref = orc.voxel_grid(clouds[b, :n[b]], (0.35, 0.5, 0.35))
            for res in (outs[0][k], outs[1][k]):
                assert res[1][b] == s and np.array_equal(res[2][b], bits(ref)), (k, b)


def test_offsets_carry_past_256_clouds(gpu_lib, monkeypatch):
    """vox_offsets_kernel scans the voxel counts 256 clouds a trip and carries the sum into the next: 600 ragged clouds of stride 64
    through the multi-kernel pipeline (a spin batch with long lines gives it S x 16 or S x 51 clouds), with empty and all-NaN clouds
    and one passed through, every cloud against the oracle; the one-workgroup path gives the same bits"""
    rng = np.random.default_rng(17)
    B, stride = 600, 64
    n = rng.integers(1, stride + 1, B).astype(np.int32)
    clouds = rng.uniform(-3, 3, (B, stride, 4)).astype(np.float32)
    clouds[rng.random((B, stride)) < 0.02, 2] = np.nan
    n[[3, 254, 258, 300, 510, 513]] = 0             # empty, next to the trip bounds too
    clouds[[7, 253, 259, 400, 509, 514], :, 0] = np.nan   # no finite point
    clouds[100] *= 1e6                              # more leaves than an int indexes: passed through
    for b in (0, 255, 256, 257, 511, 512, 599):
        n[b] = stride - (b % 3)
        clouds[b] = rng.uniform(-3, 3, (stride, 4)).astype(np.float32)
    refs = [orc.voxel_grid(clouds[b, :n[b]], 0.5) for b in range(B)]
    assert {0, 1, 2} == {s for s, _ in refs} and all(refs[b][0] == 0 and len(refs[b][1]) > 8 for b in (255, 256, 257, 511, 512))
    got = []
    for general in (True, False):
        if general:
            monkeypatch.setenv("LL_VOXEL_GENERAL_PATH", "1")
        else:
            monkeypatch.delenv("LL_VOXEL_GENERAL_PATH")
        vg = VoxelGrid(max_points=stride, max_clouds=B)
        vg.setLeafSize(0.5, 0.5, 0.5)
        out, n_out, st = vg.filter_batch(clouds, n)
        vg.close()
        for b in range(B):
            s, ref = refs[b]
            assert st[b] == s and n_out[b] == len(ref), (general, b)
            assert np.array_equal(bits(out[b, :n_out[b]]), bits(ref)), (general, b)
        got.append((n_out.copy(), [bits(out[b, :n_out[b]]).copy() for b in range(B)]))
    assert np.array_equal(got[0][0], got[1][0]) and all(np.array_equal(x, y) for x, y in zip(got[0][1], got[1][1]))


def test_properties_at_map_scale(gpu_lib):
    """1 M points (a map refresh, LM:533-537): count conservation, centroids inside their leaf, ascending leaf order"""
    rng = np.random.default_rng(6)
    n = 1_000_000
    p = rng.uniform(-40, 40, (n, 4)).astype(np.float32)
    vg = VoxelGrid(max_points=n)
    vg.setLeafSize(0.4, 0.4, 0.4)
    vg.setInputCloud(p)
    out = vg.filter()
    inv = np.float32(1.0) / np.float32(0.4)
    mn = p[:, :3].min(0)
    min_b = np.floor(mn * inv).astype(np.int64)
    div = np.floor(p[:, :3].max(0) * inv).astype(np.int64) - min_b + 1
    ijk_in = (np.floor(p[:, :3] * inv) - min_b).astype(np.int64)
    idx_in = ijk_in[:, 0] + ijk_in[:, 1] * div[0] + ijk_in[:, 2] * div[0] * div[1]
    uniq, counts = np.unique(idx_in, return_counts=True)
    assert len(out) == len(uniq)
    # intensity-weighted conservation: sum(count * centroid) == sum(points) up to float rounding
    assert np.allclose((out * counts[:, None]).sum(0, dtype=np.float64), p.sum(0, dtype=np.float64), rtol=1e-4, atol=1.0)
    ijk_out = (np.floor(out[:, :3] * inv) - min_b).astype(np.int64)
    idx_out = ijk_out[:, 0] + ijk_out[:, 1] * div[0] + ijk_out[:, 2] * div[0] * div[1]
    assert (idx_out == uniq).mean() > 0.999   # a centroid can round onto a leaf wall, otherwise it stays in its leaf
    vg.close()


def test_downsampled_registration_matches_oracle(gpu_lib, small_world, scans):
    """m_if_input_downsample_mode (LM:1367-1373): extractor -> device VoxelGrid (line_res 0.1 / plane_res 0.4) -> registrar,
    against oracle extraction -> oracle VoxelGrid -> oracle registration"""
    B = 4
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, small_world["corner"])
    m.setInputCloud(Map_buffer.SURF, small_world["surf"])
    fe = Livox_laser(max_points=24000, max_scans=B, piecewise_number=1)
    fe.upload(np.stack([s.xyzi for s in scans]), np.full(B, 1.0))
    fe.extract_batch(B); fe.resolve(); fe.select_batch(B, -1, 0.0, 1.0)
    vc, vs = VoxelGrid(24000, B), VoxelGrid(24000, B)
    reg = Point_cloud_registration(max_scans=B, max_features=24000)
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = 10, 20, 1
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    init = np.stack([s.pose_init for s in scans])
    reg.enqueue_fe_downsampled(m, fe, vc, vs, 0.1, 0.4, B, init, init)
    res, pc, pi, reps = reg.collect(B)
    nc, _ = vc.counts(B)
    ns, _ = vs.counts(B)
    for b, sc in enumerate(scans):
        _, _, _, _, fc, fs = oracle_features(sc)
        _, fc_ds = orc.voxel_grid(fc, 0.1)
        _, fs_ds = orc.voxel_grid(fs, 0.4)
        assert nc[b] == len(fc_ds) and ns[b] == len(fs_ds) and len(fs_ds) < len(fs)
        prm = orc.RegParams.defaults(icp_iters=10, ceres_iters=20, force_all=1)
        ret, opc, opi, rep = orc.reg_solve(small_world["tree_c"], small_world["tree_s"], fc_ds, fs_ds, prm, sc.pose_init, sc.pose_init)
        dt, dr = synth.pose_error(pc[b], opc)
        assert res[b] == ret and dt < 1e-7 and dr < 1e-7
        assert reps[b].n_blocks_last == rep.n_blocks_last and reps[b].lm_iterations_total == rep.lm_iterations_total
    for h in (fe, vc, vs, reg, m):
        h.close()


def test_fp16_point_map_knn_is_exact_on_the_dequantised_cloud(gpu_lib, small_world):
    """BASELINE config C5: 8-byte fp16-in-cell records, fp32 distance accumulation.  The device returns the exact 5-NN of
    the cloud its records stand for (ll_map_dequantized), which differs from the input by at most 2^-11 cell sizes."""
    rng = np.random.default_rng(21)
    surf = small_world["surf"][:, :3].copy()
    surf[5] = surf[9]                       # an exact duplicate: ties by original index survive the quantisation
    surf[17, 1] = np.nan                    # dropped point
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
    assert err <= 0.6 * 2.0 ** -11 * 1.01 + 1e-5       # cell 0.6 m: <= 0.3 mm
    i16, d16 = m.nearestKSearch(Map_buffer.SURF, q, 50.0)
    tree = orc.KdTree(np.where(np.isfinite(deq), deq, 1e9).astype(np.float32))
    oi, od = tree.knn(q, 5)
    assert np.array_equal(oi, i16) and np.array_equal(bits(od), bits(d16))
    assert i16[0, 0] == 5 and i16[0, 1] == 9 and d16[0, 0] == d16[0, 1]
    # the quantisation moves points by less than a millimetre: the neighbour sets barely change
    assert (np.sort(i16, 1) == np.sort(i32, 1)).all(1).mean() > 0.95
    # the registrar refuses an fp16-point map
    reg = Point_cloud_registration(max_scans=1, max_features=1000)
    reg.params.current_frame_index, reg.params.mapping_init_accumulate_frames = 100, 50
    m.setInputCloud(Map_buffer.CORNER, small_world["corner"])
    with pytest.raises(Exception):
        reg.find_out_incremental_transfrom(m, small_world["corner"][:100], small_world["surf"][:500])
    reg.close(); m.close()
