"""Spinning-lidar scans behind the extractor, CPU tier: the C ABI of the device hand-off (ll_reg_enqueue_spin,
ll_reg_enqueue_spin_downsampled, ll_history_add_spin, ll_cloud_transform_spin_device) is declared, exported and bound; the synthetic
sequence of a level spinning sensor is reproducible and extractable; and a test-side oracle mapping loop -- oracle/orc_mapping.py's
LaserMapping with the Livox extractor replaced by the host restatement of the spinning one (tests/spin_ref.c) -- tracks it.  The loop
is the reference of the GPU tier (tests/test_gpu_spin_reg.py).

Cloud choice (a project decision): corner stack = /laser_cloud_less_sharp, surface stack = /laser_cloud_less_flat."""
import os
import re

import numpy as np
import pytest

from loam_livox_amd import capi, synth
from oracle import orc
from oracle.orc_mapping import LaserMapping
from tests import spin_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ll_reg_enqueue_spin", "ll_reg_enqueue_spin_downsampled", "ll_history_add_spin", "ll_cloud_transform_spin_device")
# the arguments of tests/test_mapping_sequence.py
MAP_ARGS = dict(maximum_history_size=5, init_accumulate_frames=2, line_res=0.1, plane_res=0.15, icp_max_iterations=6, ceres_max_iterations=20,
                max_allow_incre_R=20.0, max_allow_incre_T=0.3)
SEQ_SEED, N_FRAMES, N_STATIC = 77, 9, 3
SEQ_SHAPES = {16: 900, 64: 500}  # scan_line -> azimuth columns per revolution


def ref_clouds(xyzi, scan_line):
    """(less-sharp, less-flat) of the host restatement"""
    c = spin_ref.clouds(spin_ref.extract(xyzi, scan_line=scan_line))
    return c[spin_ref.TOPICS[2]], c[spin_ref.TOPICS[4]]


class SpinLaserMapping(LaserMapping):
    """oracle/orc_mapping.py LaserMapping::process_new_scan (history mode) fed the spinning extractor's clouds.  `clouds`: a callable
    xyzi -> (corner stack, surface stack); the default is the host restatement."""

    def __init__(self, scan_line=16, clouds=None, **kw):
        assert not kw.get("matching_mode", 0), "history mode only"
        super().__init__(**kw)
        self.clouds = clouds or (lambda xyzi: ref_clouds(xyzi, scan_line))

    def process_new_scan(self, xyzi, time_stamp=1.0):
        fc, fs = self.clouds(xyzi)
        if self.ds:                                                       # LM:1367-1373
            fc = orc.voxel_grid(fc, self.res[0])[1] if len(fc) else fc
            fs = orc.voxel_grid(fs, self.res[1])[1] if len(fs) else fs
        self.prm.current_frame_index = self.frame
        self.frame += 1
        ret, pc, _, rep = orc.reg_solve(self.trees[0], self.trees[1], fc, fs, self.prm, self.pose, self.pose)
        self.report = rep
        if not ret:
            return 0
        self.hist.add(fc, fs, pc, self.steps[0], self.steps[1], gate_pose=self.pose)
        self.pose = pc.copy()
        self.maps = self.hist.refresh()
        self.trees = [orc.KdTree(m) if len(m) else None for m in self.maps]
        return 1


def run_oracle(scans, scan_line, downsample, clouds=None):
    om = SpinLaserMapping(scan_line=scan_line, clouds=clouds, input_downsample_mode=downsample, **MAP_ARGS)
    out = []
    for xyzi in scans:
        r = om.process_new_scan(xyzi)
        out.append((r, om.pose.copy(), [m.copy() for m in om.maps], om.report.gated, om.report.n_blocks_last))
    return out


def make_sequence(scan_line):
    return synth.make_spin_sequence(synth.make_world(2, 2), N_FRAMES, N_STATIC, scan_line, SEQ_SHAPES[scan_line], seed=SEQ_SEED)


# ------------------------------------------------------------------------------------------------------ C ABI
def header_text():
    return open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()


def test_handoff_symbols_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    L = capi.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), f"{name} is not declared in include/loam_livox_hip.h"
        assert hasattr(L, name), f"{name} is not exported"
        assert name in capi.SYMBOLS, f"{name} has no ctypes prototype"
        assert getattr(L, name).argtypes == capi.SYMBOLS[name][1]
    # the _spin forms take the arguments of the _fe forms
    for spin, fe in (("ll_reg_enqueue_spin", "ll_reg_enqueue_fe"), ("ll_reg_enqueue_spin_downsampled", "ll_reg_enqueue_fe_downsampled"),
                     ("ll_history_add_spin", "ll_history_add_fe"), ("ll_cloud_transform_spin_device", "ll_cloud_transform_fe_device")):
        assert capi.SYMBOLS[spin] == capi.SYMBOLS[fe]


def test_python_surface_exists():
    from loam_livox_amd.api import History_buffer, Point_cloud_registration
    from loam_livox_amd.mapping import Laser_mapping
    import inspect
    for name in ("enqueue_spin", "enqueue_spin_downsampled", "append_to_submap_device_spin"):
        assert callable(getattr(Point_cloud_registration, name))
    assert callable(History_buffer.add_spin)
    sig = inspect.signature(Laser_mapping.__init__).parameters
    assert sig["lidar_type"].default == "livox" and sig["scan_line"].default == 16
    assert sig["minimum_range"].default == 0.1 and sig["mapping_plane_resolution"].default == 0.8


def test_header_documents_the_deblur_refusal_and_the_cloud_choice():
    text = " ".join(header_text().split())
    i = text.index("int ll_reg_enqueue_spin(")
    doc = text[text.rindex("/*", 0, i):i].replace(" * ", " ")
    assert "if_motion_deblur must be 0" in doc and "refused" in doc and "laser_feature_extractor.hpp:502" in doc
    assert "corner stack = LL_SPIN_LESS_SHARP" in doc and "surface stack = LL_SPIN_LESS_FLAT" in doc
    assert "ll_spin_resolve" in doc and "LL_SPIN_STATUS_LINE_OVERFLOW" in doc and "LL_SPIN_LESS_FLAT_PRE" in doc


# ------------------------------------------------------------------------------------------------------ the sequence
@pytest.mark.parametrize("scan_line", [16, 64])
def test_spin_sequence_is_deterministic_and_extractable(scan_line):
    a, pa = make_sequence(scan_line)
    b, pb = make_sequence(scan_line)
    assert len(a) == len(pa) == N_FRAMES
    assert all(x.dtype == np.float32 and x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert all(np.array_equal(p, q) for p, q in zip(pa, pb))
    c, _ = synth.make_spin_sequence(synth.make_world(2, 2), N_FRAMES, N_STATIC, scan_line, SEQ_SHAPES[scan_line], seed=SEQ_SEED + 1)
    assert a[0].tobytes() != c[0].tobytes()
    # static frames share the pose, the others move by 4 cm + 0.4 deg, level
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    for k in range(N_STATIC):
        assert synth.pose_error(pa[k], ident) == (0.0, 0.0) or max(synth.pose_error(pa[k], ident)) < 1e-12
    for k in range(N_STATIC, N_FRAMES):
        dt, dr = synth.pose_error(pa[k], pa[k - 1])
        assert abs(dt - np.hypot(0.04, 0.015)) < 1e-9 and abs(dr - np.deg2rad(0.4)) < 1e-9
        assert abs(pa[k][0]) < 1e-12 and abs(pa[k][1]) < 1e-12 and abs(pa[k][6]) < 1e-12
    for xyzi in a:
        r = spin_ref.extract(xyzi, scan_line=scan_line)
        assert len(r["full"]) > 0.5 * len(xyzi) and len(r["less_sharp"]) > 0 and len(r["less_flat"]) > 300
        assert len(r["less_sharp"]) <= 1200 * scan_line  # 200 picks x 6 sub-regions per line (laser_feature_extractor.hpp:667-676)


@pytest.mark.parametrize("downsample", [1, 0])
@pytest.mark.parametrize("scan_line", [16, 64])
def test_oracle_loop_tracks_the_spin_sequence(scan_line, downsample):
    scans, truth = make_sequence(scan_line)
    run = run_oracle(scans, scan_line, downsample)
    gated = [o[3] for o in run]
    assert gated[:N_STATIC] == [1] * N_STATIC and not any(gated[N_STATIC:])
    for k, (r, pose, maps, _, nb) in enumerate(run):
        assert r == 1, f"frame {k} rejected"
        dt, dr = synth.pose_error(pose, truth[k])
        assert dt < 0.03 and dr < 0.006, (k, dt, dr)  # the bound of tests/test_mapping_sequence.py
        if k >= N_STATIC:
            assert nb > 100
    dt, dr = synth.pose_error(run[-1][1], truth[-1])
    print(f"scan_line {scan_line} downsample {downsample}: final drift {dt:.4f} m {dr:.5f} rad")
