"""Spinning-lidar scans behind the extractor, GPU tier: the device hand-off of a spin handle's clouds to the registrar, the history
and a device sub-map (ll_reg_enqueue_spin, ll_reg_enqueue_spin_downsampled, ll_history_add_spin, ll_cloud_transform_spin_device),
and Laser_mapping(lidar_type="velodyne").

 A  the hand-off gives the bits of the host round trip through ll_spin_cloud / ll_reg_upload_features (no tolerance);
 B  every slot agrees with the oracle registrar on the downloaded clouds (pose within 1e-7, equal accept / reject and counts);
 C  add_spin == add of the downloaded clouds; append_to_submap_device_spin == ll_cloud_transform of the downloaded cloud;
 D  the mapping loop against the test-side oracle loop of tests/test_spin_reg_host.py, with and without the prefetch;
 E  no synchronising call is needed between extract_batch and enqueue_spin;
 F  every refusal has its text and leaves the handles usable;
 G  the defaults still build the Livox path."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from loam_livox_amd import capi, synth
from loam_livox_amd.api import History_buffer, Livox_laser, Map_buffer, Point_cloud_registration, Spinning_laser, VoxelGrid
from oracle import orc
from tests import spin_inputs, spin_ref
from tests.test_spin_reg_host import MAP_ARGS, N_STATIC, make_sequence, run_oracle

pytestmark = pytest.mark.gpu
TOL = 1e-7
LINE_RES, PLANE_RES = 0.1, 0.4
ICP_ITERS, CERES_ITERS = 10, 20
LS, LF = spin_ref.TOPICS[2], spin_ref.TOPICS[4]
N_SLOTS = {16: 32, 64: 8}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def set_params(reg):
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations = ICP_ITERS, CERES_ITERS
    p.para_max_angular_rate, p.para_max_speed = 20.0, 0.3
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    return p


def oracle_params():
    return orc.RegParams.defaults(icp_iters=ICP_ITERS, ceres_iters=CERES_ITERS, force_all=0)


def report_tuple(rep):
    return tuple(getattr(rep, name) for name, _ in capi.RegReport._fields_)


def counts(rep):
    return (rep.n_blocks_last, rep.corner_avail, rep.surf_avail, rep.icp_iterations, rep.lm_iterations_total)


def same_solution(a, b):
    """(res, poses, increments, reports) of two collects: the same bits in every field"""
    return (np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
            and [report_tuple(r) for r in a[3]] == [report_tuple(r) for r in b[3]])


@pytest.fixture(scope="module")
def dev_map(gpu_lib, small_world):
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, small_world["corner"])
    m.setInputCloud(Map_buffer.SURF, small_world["surf"])
    yield m
    m.close()


class Batch:
    """ragged scans of one sensor (as tests/test_gpu_spin.py builds them), extracted and resolved on a handle that stays open, their
    downloaded clouds and perturbed initial poses"""

    def __init__(self, world, scan_line):
        B = self.B = N_SLOTS[scan_line]
        self.scan_line = scan_line
        if scan_line == 16:
            sc = [synth.make_spin_scan(world, k, scan_line=16, n_azimuth=int(900 + 37 * (k % 25)), p_nan=0.002 * (k % 3),
                                       range_sigma=0.0 if k % 7 == 0 else 0.01) for k in range(B)]
        else:
            sc = [synth.make_spin_scan(world, 300 + k, scan_line=64, n_azimuth=int(1400 + 23 * k)) for k in range(B)]
        self.scans = [s.xyzi for s in sc]
        self.truth = np.stack([s.pose_true for s in sc])
        rng = np.random.default_rng(9100 + scan_line)
        self.inits = np.stack([synth.pose_compose(s.pose_true, np.r_[synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.0, 0.01)),
                                                                    rng.uniform(-0.05, 0.05, 3)]) for s in sc])
        self.max_points = max(len(s) for s in self.scans)
        self.spin = Spinning_laser(scan_line=scan_line, max_points=self.max_points, max_scans=B, max_line_points=4096)
        self.clouds = self.spin.extract_batch(self.scans)
        self.counts, self.status = self.spin.counts(B)
        self.corners = [c[LS] for c in self.clouds]
        self.surfs = [c[LF] for c in self.clouds]

    def registrar(self):
        reg = Point_cloud_registration(max_scans=self.B, max_features=self.max_points)
        set_params(reg)
        return reg

    def voxels(self):
        return VoxelGrid(self.max_points, self.B), VoxelGrid(self.max_points, self.B)


@pytest.fixture(scope="module")
def batches(gpu_lib, small_world):
    out = {L: Batch(small_world["world"], L) for L in (16, 64)}
    yield out
    for b in out.values():
        b.spin.close()


def pad(clouds):
    n = np.array([len(c) for c in clouds], np.int32)
    buf = np.zeros((len(clouds), max(1, int(n.max())), 4), np.float32)
    for b, c in enumerate(clouds):
        buf[b, :len(c)] = c
    return buf, n


def device_route(bt, dev_map, downsample):
    reg = bt.registrar()
    if downsample:
        vc, vs = bt.voxels()
        reg.enqueue_spin_downsampled(dev_map, bt.spin, vc, vs, LINE_RES, PLANE_RES, bt.B, bt.inits, bt.inits)
    else:
        reg.enqueue_spin(dev_map, bt.spin, bt.B, bt.inits, bt.inits)
    out = reg.collect(bt.B)
    n = None
    if downsample:
        n = (vc.counts(bt.B)[0].copy(), vs.counts(bt.B)[0].copy())
        vc.close(), vs.close()
    reg.close()
    return out, n


def round_trip_route(bt, dev_map, downsample):
    """what the library offered before the hand-off: download (bt.corners / bt.surfs come from ll_spin_cloud), filter, upload"""
    corners, surfs = bt.corners, bt.surfs
    n = None
    if downsample:
        vc, vs = bt.voxels()
        vc.setLeafSize(LINE_RES, LINE_RES, LINE_RES)
        vs.setLeafSize(PLANE_RES, PLANE_RES, PLANE_RES)
        oc, nc, _ = vc.filter_batch(*pad(corners))
        os_, ns, _ = vs.filter_batch(*pad(surfs))
        corners = [oc[b, :nc[b]] for b in range(bt.B)]
        surfs = [os_[b, :ns[b]] for b in range(bt.B)]
        n = (nc.copy(), ns.copy())
        vc.close(), vs.close()
    reg = bt.registrar()
    reg.upload_features(corners, surfs)
    reg.enqueue_uploaded(dev_map, bt.B, bt.inits, bt.inits)
    out = reg.collect(bt.B)
    reg.close()
    return out, n


@pytest.fixture(scope="module")
def solved(batches, dev_map):
    """(device route, round trip) of every (sensor, down-sampling) case"""
    return {(L, ds): (device_route(batches[L], dev_map, ds), round_trip_route(batches[L], dev_map, ds)) for L in (16, 64) for ds in (0, 1)}


# ------------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("downsample", [0, 1])
@pytest.mark.parametrize("scan_line", [16, 64])
def test_handoff_equals_round_trip_bit_for_bit(batches, solved, scan_line, downsample):
    bt = batches[scan_line]
    assert np.all(bt.status == 0) and len({len(s) for s in bt.scans}) > 1  # ragged
    assert all(len(c) > 0 for c in bt.corners) and all(len(s) > 100 for s in bt.surfs)
    (dev, dn), (rt, rn) = solved[(scan_line, downsample)]
    assert not any(r.gated for r in dev[3]) and sum(int(r) for r in dev[0]) > 0
    if downsample:
        assert np.array_equal(dn[0], rn[0]) and np.array_equal(dn[1], rn[1])
    assert np.array_equal(dev[0], rt[0])
    assert dev[1].tobytes() == rt[1].tobytes() and dev[2].tobytes() == rt[2].tobytes()
    for b in range(bt.B):
        assert report_tuple(dev[3][b]) == report_tuple(rt[3][b]), b


# ------------------------------------------------------------------------------------------------------ B
def knife_edge_report(tc, ts, fc, fs, prm, init, pose, ret):
    runs = []
    for k in range(7):
        for d in (np.inf, -np.inf):
            p = np.array(init, np.float64).copy()
            p[k] = np.nextafter(p[k], d)
            runs.append(orc.reg_solve(tc, ts, fc, fs, prm, p, p))
    t = np.stack([r[1][4:] for r in runs])
    spread = float(np.max(np.linalg.norm(t[:, None, :] - t[None, :, :], axis=-1)))
    hit = any(r[0] == ret and max(synth.pose_error(pose, r[1])) < TOL for r in runs)
    return spread, hit


@pytest.mark.parametrize("downsample", [0, 1])
@pytest.mark.parametrize("scan_line", [16, 64])
def test_every_slot_against_the_oracle(batches, solved, small_world, scan_line, downsample):
    """No slot is exempt.  A slot that disagrees is printed with the oracle's own spread under one-ulp changes of its initial guess
    (the procedure of DESIGN section 3); a knife-edge found that way calls for another seed, not for an exemption."""
    bt = batches[scan_line]
    assert bt.B >= (32 if scan_line == 16 else 8)
    (res, pc, _, reps), _ = solved[(scan_line, downsample)][0]
    tc, ts, prm = small_world["tree_c"], small_world["tree_s"], oracle_params()

    def feats(b):
        fc, fs = bt.corners[b], bt.surfs[b]
        if downsample:
            fc, fs = orc.voxel_grid(fc, LINE_RES)[1], orc.voxel_grid(fs, PLANE_RES)[1]
        return fc, fs

    def solve(b):
        fc, fs = feats(b)
        return orc.reg_solve(tc, ts, fc, fs, prm, bt.inits[b], bt.inits[b])

    with ThreadPoolExecutor(16) as ex:
        ref = list(ex.map(solve, range(bt.B)))
    err = np.array([synth.pose_error(pc[b], ref[b][1]) for b in range(bt.B)])
    same = np.array([res[b] == ref[b][0] and counts(reps[b]) == counts(ref[b][3]) for b in range(bt.B)])
    off = np.flatnonzero(~same | (err.max(axis=1) >= TOL))
    true_err = np.array([synth.pose_error(pc[b], bt.truth[b]) for b in range(bt.B)])
    print(f"\nscan_line {scan_line} downsample {downsample}: {bt.B} slots, accepted {int(np.sum(res))}, max difference from the oracle "
          f"{err[:, 0].max():.3g} m / {err[:, 1].max():.3g} rad; distance from the true pose, median {np.median(true_err[:, 0]):.3g} m; "
          f"ICP iterations {sorted({r.icp_iterations for r in reps})}; slots off: {off.tolist()}")
    for b in off:
        spread, hit = knife_edge_report(tc, ts, *feats(b), prm, bt.inits[b], pc[b], res[b])
        print(f"  slot {b}: {err[b, 0]:.3g} m / {err[b, 1]:.3g} rad, device {counts(reps[b])} res {res[b]}, oracle {counts(ref[b][3])} "
              f"res {ref[b][0]}; oracle spread under 1-ulp perturbations {spread:.3g} m, device answer among them: {hit}")
    assert off.size == 0


# ------------------------------------------------------------------------------------------------------ C
def test_add_spin_equals_add_of_the_downloaded_clouds(batches):
    bt = batches[16]
    cap = max(max(len(s) for s in bt.surfs), max(len(c) for c in bt.corners))
    dev, host = History_buffer(3, cap, 0.2, 0.5), History_buffer(3, cap, 0.2, 0.5)
    md, mh = Map_buffer(), Map_buffer()
    for k, b in enumerate((0, 5, 17, 3, 31, 8)):
        pose = bt.truth[b]
        t_step, a_step = (0.0, 0.0) if k < 4 else (1000.0, 10.0)  # the last two frames are gated out by the add-frame rule
        a = dev.add_spin(bt.spin, b, pose, t_step, a_step)
        h = host.add(bt.corners[b], bt.surfs[b], pose, t_step, a_step)
        assert a == h == (k < 4) and len(dev) == len(host)
        assert dev.refresh(md) == host.refresh(mh)
        for kind in (0, 1):
            x, y = dev.map_cloud(kind), host.map_cloud(kind)
            assert len(x) > 0 and np.array_equal(bits(x), bits(y)), (k, kind)
    for h in (dev, host, md, mh):
        h.close()


def test_submap_device_spin_equals_cloud_transform(batches):
    import torch
    bt = batches[64]
    n = 5
    reg = Point_cloud_registration(max_scans=bt.B, max_features=bt.max_points)
    accept = np.array([1, 1, 0, 1, 1], np.int32)  # a rejected scan in the middle
    poses = bt.truth[:n]
    for which in (Spinning_laser.FULL, Spinning_laser.LESS_SHARP, Spinning_laser.LESS_FLAT):
        src = [bt.clouds[b][spin_ref.TOPICS[which]] for b in range(n)]
        expect = np.concatenate([reg.pointcloudAssociateToMap(src[b], poses[b]) for b in range(n) if accept[b]])
        lead = 7
        out = torch.full((lead + len(expect), 4), -1.0, dtype=torch.float32, device="cuda")
        used = reg.append_to_submap_device_spin(bt.spin, n, which, accept, poses, out, lead)
        assert used == lead + len(expect) and len(expect) > 0
        got = out.cpu().numpy()
        assert np.all(got[:lead] == -1.0) and np.array_equal(bits(got[lead:]), bits(expect)), which
        # one point short: refused, *n_points untouched, nothing reported as appended
        small = torch.zeros((lead + len(expect) - 1, 4), dtype=torch.float32, device="cuda")
        cnt = C.c_int64(lead)
        rc = reg.L.ll_cloud_transform_spin_device(reg.h, bt.spin.h, n, which, capi.ptr(accept), capi.ptr(np.ascontiguousarray(poses)),
                                                  C.c_void_p(small.data_ptr()), int(small.shape[0]), C.byref(cnt))
        assert rc != 0 and cnt.value == lead and b"device buffer too small" in reg.L.ll_last_error()
    reg.close()


@pytest.mark.parametrize("names,tight", [(("zigzag", "ring"), False), (("zigzag",), True), (("zigzag_jitter", "zigzag"), True)])
def test_crowded_scans_are_handed_over_whole(gpu_lib, names, tight):
    """scans with hundreds to thousands of less-sharp picks (tests/spin_inputs.py: sub-regions at the 200-pick bound; the scans above
    have a few dozen): the packed corner stack, bounded by pack_stride = min(1200 * scan_line, max_points), holds every pick.  The
    device sub-map append and the history add give the bits of the round trip through the downloaded clouds; `tight`: max_points
    below 1200 * scan_line, so that max_points is the bound."""
    import torch
    scans = [spin_inputs.family(k)[0] for k in names]
    refs = [spin_inputs.family(k)[1] for k in names]
    B = len(scans)
    max_points = max(len(x) for x in scans) + 1
    assert (max_points < 1200 * 16) == tight and all(len(r["less_sharp"]) > 900 for r in refs)
    sp = Spinning_laser(scan_line=16, max_points=max_points, max_scans=B, max_line_points=max_points)
    clouds = sp.extract_batch(scans)
    assert np.all(sp.counts(B)[1] == 0)
    for c, r in zip(clouds, refs):
        assert np.array_equal(c["less_sharp"], r["less_sharp"]) and np.array_equal(c[LS][:, :3], r["full"][r["less_sharp"], :3])
    rng = np.random.default_rng(31)
    poses = np.stack([np.r_[synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.1, 1.0)), rng.uniform(-5, 5, 3)] for _ in range(B)])
    reg = Point_cloud_registration(max_scans=B, max_features=max_points)
    accept = np.ones(B, np.int32)
    for which in (Spinning_laser.LESS_SHARP, Spinning_laser.SHARP, Spinning_laser.LESS_FLAT, Spinning_laser.FULL):  # (no flat points here)
        src = [clouds[b][spin_ref.TOPICS[which]] for b in range(B)]
        expect = np.concatenate([reg.pointcloudAssociateToMap(src[b], poses[b]) for b in range(B)])
        out = torch.full((3 + len(expect), 4), -1.0, dtype=torch.float32, device="cuda")
        used = reg.append_to_submap_device_spin(sp, B, which, accept, poses, out, 3)
        got = out.cpu().numpy()
        assert used == 3 + len(expect) and np.all(got[:3] == -1.0) and np.array_equal(bits(got[3:]), bits(expect)), which
    reg.close()
    # the corner stack of the hand-off itself (spin_handoff: what ll_reg_enqueue_spin and ll_history_add_spin read)
    cap = max(max(len(c[LS]) for c in clouds), max(len(c[LF]) for c in clouds))
    dev, host = History_buffer(3, cap, 0.2, 0.5), History_buffer(3, cap, 0.2, 0.5)
    md, mh = Map_buffer(), Map_buffer()
    for b in range(B):
        assert dev.add_spin(sp, b, poses[b], 0.0, 0.0) == host.add(clouds[b][LS], clouds[b][LF], poses[b], 0.0, 0.0)
        assert dev.refresh(md) == host.refresh(mh)
        for kind in (0, 1):
            x, y = dev.map_cloud(kind), host.map_cloud(kind)
            assert len(x) > 0 and np.array_equal(bits(x), bits(y)), (b, kind)
    for h in (dev, host, md, mh, sp):
        h.close()


# ------------------------------------------------------------------------------------------------------ D
def device_clouds_provider(scan_line, max_points):
    """xyzi -> the device extractor's downloaded (less-sharp, less-flat): the oracle loop on exactly the loop's input bits"""
    sp = Spinning_laser(scan_line=scan_line, max_points=max_points)

    def clouds(xyzi):
        c = sp.extract(xyzi)
        return c[LS], c[LF]
    return sp, clouds


@pytest.mark.parametrize("downsample", [1, 0])
@pytest.mark.parametrize("scan_line", [16, 64])
def test_spinning_mapping_loop_matches_oracle(gpu_lib, scan_line, downsample):
    """The device loop against the oracle loop on the host restatement's clouds: result, pose within 1e-7, map sizes, block counts, and
    x, y, z of the surface match buffer bit for bit (the restatement's intensities come from the host atan2f, the device's from the
    device's: within 1e-4, tests/test_gpu_spin.py).  Against the oracle loop on the device extractor's downloaded clouds every bit of
    the buffer, intensity included.  With and without the prefetch of the next scan: the same bits."""
    from loam_livox_amd.mapping import Laser_mapping
    scans, truth = make_sequence(scan_line)
    n_pts = max(len(s) for s in scans)
    ref = run_oracle(scans, scan_line, downsample)
    sp, provider = device_clouds_provider(scan_line, n_pts)
    ref_dev = run_oracle(scans, scan_line, downsample, clouds=provider)
    sp.close()
    runs = []
    for prefetch in (False, True):
        lm = Laser_mapping(scan_points=n_pts, input_downsample_mode=downsample, lidar_type="velodyne", scan_line=scan_line, **MAP_ARGS)
        assert isinstance(lm.fe, Spinning_laser)
        trace, compared = [], 0
        for k, o in enumerate(ref):
            nxt = scans[k + 1] if prefetch and k + 1 < len(scans) else None
            r = lm.process_new_scan(scans[k], next_xyzi=nxt)
            dt, dr = synth.pose_error(lm.pose, o[1])
            assert r == o[0] == 1 and dt < TOL and dr < TOL, (k, r, dt, dr)
            assert lm.map_sizes == (len(o[2][0]), len(o[2][1])), k
            assert lm.last_report.n_blocks_last == o[4] and lm.last_report.gated == o[3], k
            buf = [lm.history.map_cloud(0), lm.history.map_cloud(1)]
            if dt == 0.0 and dr == 0.0:  # identical poses -> identical transforms -> bit-identical match buffer
                compared += 1
                assert np.array_equal(bits(buf[1][:, :3]), bits(o[2][1][:, :3])), k
                assert np.allclose(buf[1][:, 3], o[2][1][:, 3], rtol=0, atol=1e-4), k
            od = ref_dev[k]
            if np.array_equal(lm.pose, od[1]):
                assert np.array_equal(bits(buf[1]), bits(od[2][1])) and np.array_equal(bits(buf[0]), bits(od[2][0])), k
            trace.append((r, lm.pose.copy(), buf))
        assert compared >= N_STATIC
        dt, dr = synth.pose_error(lm.pose, truth[len(ref) - 1])
        assert dt < 0.03 and dr < 0.006
        print(f"scan_line {scan_line} downsample {downsample} prefetch {prefetch}: match buffer compared on {compared} of {len(ref)} frames, "
              f"final drift {dt:.4f} m {dr:.5f} rad")
        if prefetch:
            assert lm._fe_pair[1] is not None  # the second handle was used
        runs.append(trace)
        lm.close()
    for a, b in zip(*runs):
        assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes()
        assert np.array_equal(bits(a[2][0]), bits(b[2][0])) and np.array_equal(bits(a[2][1]), bits(b[2][1]))


def test_spinning_mapping_refuses_what_it_does_not_run(gpu_lib):
    from loam_livox_amd.mapping import Laser_mapping
    for kw in (dict(matching_mode=1), dict(keep_cell_maps=True), dict(loop_closure_if_enable=1)):
        with pytest.raises(ValueError, match="history mode only"):
            Laser_mapping(scan_points=4000, lidar_type="velodyne", **kw)


# ------------------------------------------------------------------------------------------------------ E
def test_enqueue_spin_needs_no_synchronising_call(batches, dev_map):
    """extract_batch and enqueue_spin back to back on fresh handles: the registrar's stream waits for the extractor's (extraction and
    pack kernel) by an event, not the host"""
    bt = batches[16]
    B = 8
    scans, inits = bt.scans[:B], bt.inits[:B]
    cap = max(len(s) for s in scans)

    def run(sync, downsample):
        sp = Spinning_laser(scan_line=16, max_points=cap, max_scans=B, max_line_points=4096)
        reg = Point_cloud_registration(max_scans=B, max_features=cap)
        set_params(reg)
        vox = (VoxelGrid(cap, B), VoxelGrid(cap, B)) if downsample else ()
        sp.upload(scans)
        sp.extract_batch_async(B)
        if sync:
            sp.sync()
        if downsample:
            reg.enqueue_spin_downsampled(dev_map, sp, vox[0], vox[1], LINE_RES, PLANE_RES, B, inits, inits)
        else:
            reg.enqueue_spin(dev_map, sp, B, inits, inits)
        out = reg.collect(B)
        for h in (sp, reg) + vox:
            h.close()
        return out

    for downsample in (0, 1):
        ref = run(True, downsample)
        assert sum(int(r) for r in ref[0]) > 0
        for _ in range(4):
            assert same_solution(run(False, downsample), ref)


# ------------------------------------------------------------------------------------------------------ F
def test_refusals_have_their_text_and_leave_the_handles_usable(batches, dev_map, solved):
    bt = batches[16]
    L = capi.load()
    B = bt.B
    reg = bt.registrar()
    vc, vs = bt.voxels()
    pl = np.ascontiguousarray(bt.inits)
    prm = C.byref(reg.params)

    def refused(rc, text):
        msg = L.ll_last_error().decode()
        assert rc != 0 and text in msg, (rc, msg)

    def enq(r=reg.h, m=dev_map.h, sp=bt.spin.h, n=B, p=prm):
        return L.ll_reg_enqueue_spin(r, m, sp, n, p, capi.ptr(pl), capi.ptr(pl), None)

    def enq_ds(r=reg.h, sp=bt.spin.h, c=vc.h, s=vs.h, n=B, p=prm):
        return L.ll_reg_enqueue_spin_downsampled(r, dev_map.h, sp, c, s, LINE_RES, PLANE_RES, n, p, capi.ptr(pl), capi.ptr(pl), None)

    refused(enq(sp=None), "ll_reg_enqueue_spin: null handle")
    refused(enq(r=None), "ll_reg_enqueue_spin: null handle")
    refused(enq_ds(sp=None), "ll_reg_enqueue_spin_downsampled: null handle")
    refused(enq_ds(c=None), "ll_reg_enqueue_spin_downsampled: null handle")
    refused(enq(n=B + 1), "n_scans exceeds the extractor capacity")
    refused(enq_ds(n=B + 1), "n_scans exceeds the extractor capacity")
    refused(enq(n=0), "n_scans must be at least 1")
    small_reg = Point_cloud_registration(max_scans=B - 1, max_features=bt.max_points)
    refused(enq(r=small_reg.h), "n_scans exceeds the registrar capacity")
    small_reg.close()
    thin_reg = Point_cloud_registration(max_scans=B, max_features=bt.max_points - 1)
    refused(enq(r=thin_reg.h), "registrar feature capacity < extractor max_points")
    refused(enq_ds(r=thin_reg.h), "registrar feature capacity < extractor max_points")
    thin_reg.close()
    few, thin = VoxelGrid(bt.max_points, B - 1), VoxelGrid(bt.max_points - 1, B)
    refused(enq_ds(c=few.h), "voxel filter capacity too small")
    refused(enq_ds(s=thin.h), "voxel filter capacity too small")
    refused(enq_ds(s=vc.h), "corner and surface need their own voxel filter handle")
    few.close(), thin.close()
    deblur = capi.reg_default_params()
    C.memmove(C.byref(deblur), C.byref(reg.params), C.sizeof(deblur))
    deblur.if_motion_deblur = 1
    refused(enq(p=C.byref(deblur)), "if_motion_deblur must be 0")
    refused(enq_ds(p=C.byref(deblur)), "if_motion_deblur must be 0")
    assert "laser_feature_extractor.hpp:502" in L.ll_last_error().decode()
    n_dev = C.c_int(0)
    C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n_dev))
    if n_dev.value > 1:  # handles on two devices
        other = Point_cloud_registration(max_scans=B, max_features=bt.max_points, device=1)
        refused(enq(r=other.h), "extractor lives on another device")
        hist1 = History_buffer(3, bt.max_points, device=1)
        added = C.c_int32(0)
        refused(L.ll_history_add_spin(hist1.h, bt.spin.h, 0, capi.ptr(pl[0]), 0.0, 0.0, C.byref(added)), "extractor lives on another device")
        other.close(), hist1.close()
    # history and sub-map forms
    hist = History_buffer(3, bt.max_points)
    added = C.c_int32(0)
    refused(L.ll_history_add_spin(hist.h, None, 0, capi.ptr(pl[0]), 0.0, 0.0, C.byref(added)), "ll_history_add_spin: null argument")
    refused(L.ll_history_add_spin(hist.h, bt.spin.h, B, capi.ptr(pl[0]), 0.0, 0.0, C.byref(added)), "scan slot out of range")
    refused(L.ll_history_add_spin(hist.h, bt.spin.h, -1, capi.ptr(pl[0]), 0.0, 0.0, C.byref(added)), "scan slot out of range")
    assert len(hist) == 0
    import torch
    out = torch.zeros((16, 4), dtype=torch.float32, device="cuda")
    acc = np.ones(B, np.int32)
    cnt = C.c_int64(3)

    def xf(sp=bt.spin.h, n=1, which=Spinning_laser.LESS_SHARP):
        return L.ll_cloud_transform_spin_device(reg.h, sp, n, which, capi.ptr(acc), capi.ptr(pl), C.c_void_p(out.data_ptr()), 16, C.byref(cnt))

    refused(xf(sp=None), "ll_cloud_transform_spin_device: null argument")
    refused(xf(which=Spinning_laser.LESS_FLAT_PRE), "LL_SPIN_LESS_FLAT_PRE is a list of positions")
    refused(xf(which=6), "unknown cloud")
    refused(xf(which=-1), "unknown cloud")
    refused(xf(n=B + 1), "n_scans exceeds the extractor capacity")
    assert cnt.value == 3
    hist.close()
    # the handles still work: a valid call gives the bits of A
    assert enq() == 0
    assert same_solution(reg.collect(B), solved[(16, 0)][0][0])
    assert enq_ds() == 0
    assert same_solution(reg.collect(B), solved[(16, 1)][0][0])
    for h in (reg, vc, vs):
        h.close()


def test_line_overflow_is_handed_over_as_downloaded(gpu_lib, small_world, dev_map):
    """a scan whose lines overflow max_line_points: the status stays readable, and the hand-off registers the clouds a download returns"""
    sc = synth.make_spin_scan(small_world["world"], 2, scan_line=16, n_azimuth=1200)
    sp = Spinning_laser(scan_line=16, max_points=len(sc.xyzi), max_scans=1, max_line_points=64)
    clouds = sp.extract_batch([sc.xyzi])[0]
    assert sp.counts(1)[1][0] == 2  # LL_SPIN_STATUS_LINE_OVERFLOW
    reg = Point_cloud_registration(max_scans=1, max_features=len(sc.xyzi))
    set_params(reg)
    init = sc.pose_true[None]
    reg.enqueue_spin(dev_map, sp, 1, init, init)
    a = reg.collect(1)
    assert sp.counts(1)[1][0] == 2
    reg.upload_features([clouds[LS]], [clouds[LF]])
    reg.enqueue_uploaded(dev_map, 1, init, init)
    assert same_solution(a, reg.collect(1))
    sp.close(), reg.close()


# ------------------------------------------------------------------------------------------------------ G
def test_defaults_still_build_the_livox_path(gpu_lib):
    from loam_livox_amd.feature_node import Laser_feature
    from loam_livox_amd.mapping import Laser_mapping
    lm = Laser_mapping(scan_points=4000, maximum_history_size=3)
    assert lm.lidar_type == "livox" and isinstance(lm.fe, Livox_laser) and not lm._spin
    lm.close()
    lf = Laser_feature(max_points=4000)
    assert lf.m_lidar_type == 1 and lf.m_spin is None
