"""What bench.py feeds its figures, regenerated with bench.py's defaults for the -m gpu tests at the measured shapes
(tests/test_gpu_measured_shapes.py):

  * the 5 M-point map, synth.make_maps(5_000_000);
  * 256 distinct 24 000-point scans, seeds 0 .. 255, built by bench.make_scans (spawned workers, at most 16);
  * the headline's (Q-full) initial guesses, default_rng(4242), one per distinct scan;
  * the Q-pipe initial guesses, default_rng(777), drawn in the order q_pipe_figure draws them: slot b registers distinct scan b % 256;
  * the registrar parameters of make_registrar (10 forced ICP iterations, 20 LM iterations, max final cost 1000, ...), and the
    shipped cap of q_pipe_figure(shipped_cap=True) (maximum_residual_blocks = 200, sub-sampling seed 7).

CRCs pin the regenerated map and scans.  The oracle side (k-d trees, features, one registration per slot) runs on a thread pool of at
most 16 threads, never os.cpu_count(): the oracle's ctypes calls release the GIL.  A plain module the tests import, not a conftest."""
from __future__ import annotations

import functools
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from loam_livox_amd import synth

MAP_POINTS = 5_000_000
N_DISTINCT = 256
SCAN_POINTS = 24000
Q_PIPE_BATCH = 2048
ICP_ITERS, CERES_ITERS, MAX_FINAL_COST = 10, 20, 1000.0
LINE_RES, PLANE_RES = 0.1, 0.4  # the VoxelGrid leaves of the Q-pipe figure (laser_mapping.hpp:1367-1373)
SHIPPED_CAP, SHIPPED_SEED = 200, 7

# CRC-32 of the regenerated arrays: the synthetic world, and with it every figure bench.py reports, must not drift under the tests
CORNER_CRC, SURF_CRC = 3146051677, 1339491843
SCANS_CRC = 2475447720  # running CRC over the xyzi of the 256 scans, seed order


def host_threads() -> int:
    """size of every host thread pool: the cores this process may run on, at most 16"""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def crc(a) -> int:
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


@functools.lru_cache(maxsize=1)
def world():
    """(world model, corner map, surface map)"""
    w, corner, surf = synth.make_maps(MAP_POINTS)
    assert crc(corner) == CORNER_CRC and crc(surf) == SURF_CRC, "the synthetic 5 M-point map changed"
    return w, corner, surf


@functools.lru_cache(maxsize=1)
def scans():
    """the 256 distinct scans (synth.Scan), built the way bench.py builds them"""
    import bench
    sc = bench.make_scans(synth, world()[0], list(range(N_DISTINCT)), SCAN_POINTS)
    c = 0
    for s in sc:
        c = zlib.crc32(np.ascontiguousarray(s.xyzi).tobytes(), c)
    assert c == SCANS_CRC, "the synthetic scans changed"
    return sc


def _perturbed(rng, pose_true):
    # bench.py's expression, operand for operand: the draws happen in this order
    return synth.pose_compose(pose_true, np.r_[synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 1.0))),
                                               rng.uniform(-0.1, 0.1, 3)])


def qfull_inits() -> np.ndarray:
    """[256, 7] initial guesses of the headline batch (bench.py main: slot b registers distinct scan b)"""
    rng = np.random.default_rng(4242)
    return np.stack([_perturbed(rng, s.pose_true) for s in scans()])


def qpipe_slots(n: int = Q_PIPE_BATCH):
    """(distinct scan of every slot, [n, 7] initial guesses) of q_pipe_figure's batch of n scans"""
    idx = np.arange(n) % N_DISTINCT
    rng = np.random.default_rng(777)
    sc = scans()
    return idx, np.stack([_perturbed(rng, sc[i].pose_true) for i in idx])


def set_bench_params(reg, shipped_cap: bool = False):
    """make_registrar's parameters on a Point_cloud_registration (q_pipe_figure copies them; shipped_cap as q_pipe_figure(shipped_cap=True))"""
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = ICP_ITERS, CERES_ITERS, 1
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, MAX_FINAL_COST
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    p.maximum_allow_residual_block = SCAN_POINTS
    if shipped_cap:
        p.maximum_allow_residual_block, p.subsample_seed = SHIPPED_CAP, SHIPPED_SEED
    return p


def oracle_params(shipped_cap: bool = False):
    """the oracle's parameters for the same registrations (bench.py qpipe_oracle_audit / cpu_legs)"""
    from oracle import orc
    prm = orc.RegParams.defaults(icp_iters=ICP_ITERS, ceres_iters=CERES_ITERS, force_all=1)
    prm.max_final_cost = MAX_FINAL_COST
    if shipped_cap:
        prm.maximum_allow_residual_block, prm.subsample_seed = SHIPPED_CAP, SHIPPED_SEED
    return prm


@functools.lru_cache(maxsize=1)
def oracle_trees():
    from oracle import orc
    _, corner, surf = world()
    return orc.KdTree(corner), orc.KdTree(surf)


def _features(i: int, q_pipe: bool):
    from oracle import orc
    o = orc.fe_extract(scans()[i].xyzi, 1.0)
    ci, si, _ = orc.fe_get_features(o, 0.0, 1.0)
    fc, fs = orc.feature_cloud(o, ci), orc.feature_cloud(o, si)
    if q_pipe:
        fc, fs = orc.voxel_grid(fc, LINE_RES)[1], orc.voxel_grid(fs, PLANE_RES)[1]
    return fc, fs


@functools.lru_cache(maxsize=2)
def oracle_features(q_pipe: bool):
    """the oracle's feature clouds of the 256 distinct scans: (corner, surface) per scan, voxel-filtered for Q-pipe"""
    with ThreadPoolExecutor(host_threads()) as ex:
        return tuple(ex.map(lambda i: _features(i, q_pipe), range(N_DISTINCT)))


def oracle_solve(i: int, init, q_pipe: bool, prm):
    """one oracle registration of distinct scan i from init -> (ret, pose, report)"""
    from oracle import orc
    tc, ts = oracle_trees()
    fc, fs = oracle_features(q_pipe)[i]
    ret, pc, _, rep = orc.reg_solve(tc, ts, fc, fs, prm, init, init)
    return ret, pc, rep


def oracle_many(scan_idx, inits, q_pipe: bool, prm):
    """oracle_solve for every (scan, initial guess) pair, on host_threads() threads"""
    oracle_features(q_pipe)
    oracle_trees()
    with ThreadPoolExecutor(host_threads()) as ex:
        return list(ex.map(lambda b: oracle_solve(int(scan_idx[b]), inits[b], q_pipe, prm), range(len(scan_idx))))


def ulp_neighbours(pose) -> list:
    """the 14 poses one ulp away from `pose` in one component (each of the seven up and down)"""
    out = []
    for k in range(7):
        for d in (np.inf, -np.inf):
            p = np.array(pose, np.float64).copy()
            p[k] = np.nextafter(p[k], d)
            out.append(p)
    return out
