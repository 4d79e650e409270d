"""-m gpu: the spinning-lidar feature extraction on the device (ll_spin_*, api.Spinning_laser) against the host restatement
tests/spin_ref.c (hku-mars/loam_livox source/laser_feature_extractor.hpp:393-787) and the recorded goldens.
x, y, z and every index set are bit-exact; the intensity of laserCloud goes through the device atan2f: it is held to what a
few-ulp atan2f difference moves it by (2^-22, the relative time scaled by 0.1) plus the rounding of scanID + 0.1 * relTime."""
import glob
import os

import numpy as np
import pytest

from loam_livox_amd import capi, synth
from loam_livox_amd.api import Spinning_laser
from loam_livox_amd.feature_node import Laser_feature
from tests import spin_inputs, spin_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def intensity_tol(ref_int):
    return np.maximum(2.0 ** -22, 2 * np.spacing(np.abs(ref_int).astype(np.float32)))


@pytest.fixture(scope="module")
def world():
    return synth.make_world(4, 4)


def compare(dev: dict, ref: dict):
    """device clouds (Spinning_laser.clouds) == restatement (spin_ref.extract); returns the number of intensities that differ"""
    full = dev["/laser_points_2"]
    assert np.array_equal(dev["full_src"], ref["full_src"])
    assert np.array_equal(dev["line_n"], ref["line_n"])
    assert np.array_equal(full[:, :3], ref["full"][:, :3])
    d = np.abs(full[:, 3].astype(np.float64) - ref["full"][:, 3])
    assert np.all(d <= intensity_tol(ref["full"][:, 3])), float(d.max())
    for k in ("sharp", "less_sharp", "flat", "less_flat_pre"):
        assert np.array_equal(dev[k], ref[k]), k
    assert np.array_equal(dev["/laser_cloud_sharp"][:, :3], ref["full"][ref["sharp"], :3])
    assert np.array_equal(dev["/laser_cloud_flat"][:, :3], ref["full"][ref["flat"], :3])
    lf = dev["/laser_cloud_less_flat"]
    assert lf.shape == ref["less_flat"].shape
    assert np.array_equal(lf[:, :3], ref["less_flat"][:, :3])
    assert np.allclose(lf[:, 3], ref["less_flat"][:, 3], rtol=0, atol=1e-4)
    return int(np.count_nonzero(d))


@pytest.mark.parametrize("scan_line", [16, 64])
def test_one_message_matches_restatement(gpu_lib, world, scan_line):
    sc = synth.make_spin_scan(world, 1, scan_line=scan_line, p_nan=0.01, p_near=0.01)
    dev = Spinning_laser(scan_line=scan_line, max_points=140000)
    c = dev.extract(sc.xyzi)
    ref = spin_ref.extract(sc.xyzi, scan_line=scan_line)
    assert len(ref["sharp"]) > 0 and len(ref["flat"]) > 0 and len(ref["less_flat"]) > 0
    compare(c, ref)
    st, n = dev.lines(0)
    assert np.array_equal(n, ref["line_n"]) and np.array_equal(st, np.r_[0, np.cumsum(n)[:-1]])
    dev.close()


def test_batch_vlp16_256_distinct_scans(gpu_lib, world):
    scans = [synth.make_spin_scan(world, k, scan_line=16, n_azimuth=int(900 + 37 * (k % 25)), p_nan=0.002 * (k % 3),
                                  range_sigma=0.0 if k % 7 == 0 else 0.01).xyzi for k in range(256)]
    dev = Spinning_laser(scan_line=16, max_points=32768, max_scans=256, max_line_points=4096)
    out = dev.extract_batch(scans)
    counts, status = dev.counts(256)
    assert np.all(status == 0)
    differ = 0
    for b in range(256):
        ref = spin_ref.extract(scans[b], scan_line=16)
        differ += compare(out[b], ref)
        assert counts[b, 0] == len(ref["full"]) and counts[b, 4] == len(ref["less_flat"])
    print(f"intensities that differ from the host libm: {differ}")
    dev.close()


def test_batch_hdl64_64_distinct_scans(gpu_lib, world):
    scans = [synth.make_spin_scan(world, 300 + k, scan_line=64, n_azimuth=int(1400 + 23 * k)).xyzi for k in range(64)]
    dev = Spinning_laser(scan_line=64, max_points=max(len(s) for s in scans), max_scans=64, max_line_points=4096)
    out = dev.extract_batch(scans)
    for b in range(64):
        compare(out[b], spin_ref.extract(scans[b], scan_line=64))
    dev.close()


def test_edges_small_nan_near_empty(gpu_lib, world):
    dev = Spinning_laser(scan_line=16, max_points=32768)
    sc = synth.make_spin_scan(world, 7, scan_line=16, n_azimuth=200)
    for pts in (sc.xyzi[:10], sc.xyzi[:11], sc.xyzi[:40], sc.xyzi[:0], np.full((20, 4), np.nan, np.float32)):
        compare(dev.extract(pts), spin_ref.extract(pts, scan_line=16))
    x = sc.xyzi.copy()
    x[::13, :3] = np.nan
    x[5::17, :3] *= 1e-3  # closer than minimum_range
    x[0, :3] = np.nan     # startOri comes from the first surviving point
    compare(dev.extract(x), spin_ref.extract(x, scan_line=16))
    dev.close()


def test_first_extraction_of_fresh_handles(gpu_lib, world):
    """the handle's counters and line offsets are zeroed at creation on the handle's own stream: a zeroing that were not ordered before
    the first extraction's kernels could land after them and wipe the counts and line offsets they wrote (empty clouds, zero lines) --
    the first extraction right after ll_spin_create, on many fresh handles"""
    sc = synth.make_spin_scan(world, 7, scan_line=16, n_azimuth=200)
    ref = spin_ref.extract(sc.xyzi[:10], scan_line=16)
    ref_big = spin_ref.extract(sc.xyzi, scan_line=16)
    for k in range(24):
        dev = Spinning_laser(scan_line=16, max_points=32768, max_scans=1 + k % 3)
        compare(dev.extract(sc.xyzi[:10] if k % 2 == 0 else sc.xyzi), ref if k % 2 == 0 else ref_big)
        dev.close()


def test_walk_reaching_the_ends_of_the_cloud(gpu_lib):
    """a dense line of sharp points next to the cloud ends: the +-500 walks stop at the ends (the defined edge)"""
    t = np.linspace(0, 1, 400, dtype=np.float32)
    x = np.stack([10 + 0.01 * t, 1 + 0.01 * t, np.full_like(t, -0.524), np.ones_like(t)], 1).astype(np.float32)  # -3 deg: line 6
    x[9:380:9, 0] += 0.8  # spikes: walks break at them; the walks from the first and the last sharp points run to the cloud ends
    dev = Spinning_laser(scan_line=16)
    compare(dev.extract(x), spin_ref.extract(x, scan_line=16))
    dev.close()


@pytest.mark.parametrize("name", sorted(spin_inputs.FAMILIES))
def test_family_matches_restatement(gpu_lib, name):
    """the scans of tests/spin_inputs.py, which reach what tests/test_spin_host.py asserts of them: sub-regions on both sides of the
    LDS / rank sort switch with runs of tied curvatures, the 20 / 200 pick bounds and the stop at the 201st pick, picks several
    64-candidate chunks deep, walks of exactly 500 steps, cut at 499, to the ends of the cloud and across a line boundary, and lines
    of more than 24 576 points (max_line_points >= the line: the per-line VoxelGrid takes the multi-kernel pipeline, status 0)"""
    x, ref = spin_inputs.family(name)
    dev = Spinning_laser(scan_line=16, max_points=len(x) + 1, max_line_points=max(8192, int(ref["line_n"].max())))
    compare(dev.extract(x), ref)
    counts, status = dev.counts(1)
    assert status[0] == 0 and counts[0, 2] == len(ref["less_sharp"]) and counts[0, 4] == len(ref["less_flat"])
    dev.close()


def test_families_in_a_batch_next_to_a_world_scan(gpu_lib, world):
    """the ladder and the spiked ring in slots other than 0, between ordinary scans: per-slot offsets of the sort and the selection"""
    scans = [synth.make_spin_scan(world, 5, scan_line=16, n_azimuth=900).xyzi, spin_inputs.family("ladder")[0],
             spin_inputs.family("ring")[0], synth.make_spin_scan(world, 6, scan_line=16, n_azimuth=1100, range_sigma=0.0).xyzi]
    refs = [spin_ref.extract(scans[0], scan_line=16), spin_inputs.family("ladder")[1], spin_inputs.family("ring")[1],
            spin_ref.extract(scans[3], scan_line=16)]
    dev = Spinning_laser(scan_line=16, max_points=max(len(s) for s in scans), max_scans=4,
                         max_line_points=int(max(r["line_n"].max() for r in refs)))
    out = dev.extract_batch(scans)
    assert np.all(dev.counts(4)[1] == 0)
    for b in range(4):
        compare(out[b], refs[b])
    dev.close()


def test_overflow_is_an_error_and_the_handle_stays_usable(gpu_lib, world):
    sc = synth.make_spin_scan(world, 3, scan_line=16, n_azimuth=600)
    dev = Spinning_laser(scan_line=16, max_points=len(sc.xyzi) - 1)
    with pytest.raises(capi.LoamLivoxError):
        dev.extract(sc.xyzi)
    small = sc.xyzi[:5000]
    compare(dev.extract(small), spin_ref.extract(small, scan_line=16))
    dev.close()
    with pytest.raises(capi.LoamLivoxError):
        Spinning_laser(scan_line=32)


def test_forced_resolve_on_scan_id_boundaries_and_the_flip(gpu_lib, world):
    """points whose vertical angle sits on a scan-ID boundary (16: odd degrees; 64: 2 deg and the 1/3-deg bins) and whose
    orientation sits on startOri + pi: the kernels list them and ll_spin_resolve re-decides them with the host libm"""
    rng = np.random.default_rng(4)
    for scan_line, bounds in ((16, [-14.0, -12.0, -2.0, 2.0, 6.0, 14.0]), (64, [2.0, 1.5, -0.5, -8.5, -20.5])):
        sc = synth.make_spin_scan(world, 11, scan_line=scan_line, n_azimuth=600)
        x = sc.xyzi.copy()
        n = len(x)
        idx = rng.choice(np.arange(20, n - 20), 300, replace=False)
        for j, i in enumerate(idx):
            e = np.deg2rad(bounds[j % len(bounds)])
            r = float(np.hypot(x[i, 0], x[i, 1]))
            x[i, 2] = np.float32(r * np.tan(e))
        # orientation on the flip: first point at azimuth 0 (startOri = 0), some points at ori = +-pi within a few ulps
        x[0, :3] = (10.0, 0.0, 0.0)
        for j, i in enumerate(idx[:60]):
            r = float(np.hypot(x[i, 0], x[i, 1]))
            x[i, 0], x[i, 1] = -r, np.float32((j - 30) * 1e-7 * r)
        dev = Spinning_laser(scan_line=scan_line, max_points=n)
        c = dev.extract(x)
        compare(c, spin_ref.extract(x, scan_line=scan_line))
        dev.close()
        dev = Spinning_laser(scan_line=scan_line, max_points=n)
        dev.extract_batch([x])
        assert dev.n_ambiguous > 0
        dev.close()


def test_feature_node_velodyne_publishes_five_topics(gpu_lib, world):
    sc = synth.make_spin_scan(world, 2, scan_line=16)
    node = Laser_feature(max_points=32768, para_system_delay=2, lidar_type="velodyne", scan_line=16)
    assert node.laserCloudHandler(sc.xyzi, 0.0) is None  # the start-up delay (:258-267)
    out = node.laserCloudHandler(sc.xyzi, 0.1)
    assert sorted(out) == sorted(Spinning_laser.TOPICS)
    ref = spin_ref.clouds(spin_ref.extract(sc.xyzi, scan_line=16))
    for t in Spinning_laser.TOPICS:
        assert out[t].shape == ref[t].shape and np.array_equal(out[t][:, :3], ref[t][:, :3]), t
    node.close()


def test_feature_node_livox_default_unchanged(gpu_lib):
    from tests.test_feature_node import messages
    w, _, _ = synth.make_maps(60_000)
    msgs = messages(w, 3, lidars=1)
    a = Laser_feature(max_points=12000, para_system_delay=1, maximum_input_lidar_pointcloud=1)
    b = Laser_feature(max_points=12000, para_system_delay=1, maximum_input_lidar_pointcloud=1, lidar_type="livox", scan_line=64)
    assert a.m_spin is None and b.m_spin is None
    for m in msgs:
        oa, ob = a.laserCloudHandler(*m), b.laserCloudHandler(*m)
        assert isinstance(oa, list) and len(oa) == len(ob)
        for ta, tb in zip(oa, ob):
            for ca, cb in zip(ta, tb):
                assert np.array_equal(ca, cb, equal_nan=True)
    a.close()
    b.close()


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "ref_spin_*.npz"))))
def test_device_matches_goldens(gpu_lib, world, path):
    g = np.load(path)
    sc = synth.make_spin_scan(world, int(g["k"]), scan_line=int(g["scan_line"]), n_azimuth=int(g["n_azimuth"]),
                              range_sigma=float(g["range_sigma"]))
    dev = Spinning_laser(scan_line=int(g["scan_line"]), max_points=len(sc.xyzi))
    c = dev.extract(sc.xyzi)
    for k in ("full_src", "sharp", "less_sharp", "flat", "less_flat_pre"):
        assert np.array_equal(c[k], g[k]), k
    assert np.array_equal(c["/laser_cloud_less_flat"][:, :3], g["less_flat"][:, :3])
    assert np.all(np.abs(c["/laser_points_2"][:, 3].astype(np.float64) - g["intensity"]) <= intensity_tol(g["intensity"]))
    dev.close()
