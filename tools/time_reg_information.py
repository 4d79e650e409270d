#!/usr/bin/env python3
"""Times what ll_reg_set_information costs a registration -- one more kernel behind the last ICP iteration, its records in the collect's copy --
on one device in one process, at three shapes: C2 Q-full at B = 256 (every feature a query), Q-pipe at 2 048 scans per batch (voxel-filtered
features, the small-scan solver), and one voxel-filtered scan (the mapping loop's shape).  The features are extracted once and stay on the
device; a repetition is enqueue -> collect with a device synchronise inside the timed region.  Registrations with the switch off and on
ALTERNATE, so that clock and thermal drift fall on both alike; every shape is warmed up, medians and ranges of the repetitions are reported
as milliseconds and as a share of the registration measured beside it, and the kernel's own time comes from ll_reg_information_time in a
profiled repetition of its own.  There is no bar on the enabled cost.  One JSON record per shape.  Needs a HIP device: no fall-back."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = (("C2 Q-full, B = 256", 256, False), ("Q-pipe, 2048 scans per batch", 2048, True), ("one voxel-filtered scan (mapping loop)", 1, True))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--map-points", type=int, default=5_000_000)
    ap.add_argument("--scan-points", type=int, default=24000)
    ap.add_argument("--icp-iters", type=int, default=10)
    ap.add_argument("--distinct-scans", type=int, default=32)
    ap.add_argument("--shapes", type=int, nargs="+", default=[0, 1, 2], help="indices into the three shapes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reg_information.json"))
    args = ap.parse_args()
    if args.reps < 11:
        ap.error("at least 11 repetitions")

    from loam_livox_amd import synth
    from loam_livox_amd.api import Livox_laser, Map_buffer, Point_cloud_registration, VoxelGrid
    from tools.build_id import build_id
    hip = ctypes.CDLL("libamdhip64.so")
    n_dev = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n_dev)) != 0 or n_dev.value < 1:
        sys.exit("no HIP device")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            sys.exit("hipDeviceSynchronize failed")

    N = args.scan_points
    world, corner, surf = synth.make_maps(args.map_points)
    base = [synth.make_scan(world, k, n=N) for k in range(args.distinct_scans)]
    rng = np.random.default_rng(4242)
    mp = Map_buffer()
    mp.setInputCloud(Map_buffer.CORNER, corner)
    mp.setInputCloud(Map_buffer.SURF, surf)
    records = []
    for name, B, q_pipe in (SHAPES[i] for i in args.shapes):
        scans = np.stack([base[b % len(base)].xyzi for b in range(B)])
        init = np.stack([synth.pose_compose(base[b % len(base)].pose_true,
                                            np.r_[synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 1.0))), rng.uniform(-0.1, 0.1, 3)])
                         for b in range(B)])
        fe = Livox_laser(max_points=N, max_scans=B, piecewise_number=1)
        fe.upload(scans, np.full(B, 1.0))
        fe.extract_batch(B)
        fe.resolve()
        fe.select_batch(B, -1, 0.0, 1.0)
        reg = Point_cloud_registration(max_scans=B, max_features=N)
        p = reg.params
        p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = args.icp_iters, 20, 1
        p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 1000.0
        p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
        p.maximum_allow_residual_block = N
        vox = (VoxelGrid(N, B), VoxelGrid(N, B)) if q_pipe else None

        def run(on):
            reg.set_information(on)
            sync()
            t0 = time.perf_counter()
            if vox:
                reg.enqueue_fe_downsampled(mp, fe, vox[0], vox[1], 0.1, 0.4, B, init, init)
            else:
                reg.enqueue_fe(mp, fe, B, init, init)
            out = reg.collect(B)
            sync()
            return time.perf_counter() - t0, out

        times = {False: [], True: []}
        poses = {}
        for rep in range(args.warmup + args.reps):
            for on in (False, True):  # alternating
                dt, out = run(on)
                if rep >= args.warmup:
                    times[on].append(dt)
                poses.setdefault(on, out[1].tobytes())
                assert out[1].tobytes() == poses[False], "the switch changed a pose, or a run differs from the first"
        infos = reg.information(B)
        reg.set_profiling(True)
        run(True)
        kernel_ms = reg.information_time()
        ms, launches = reg.kernel_times()
        reg.set_profiling(False)
        off, on = 1e3 * statistics.median(times[False]), 1e3 * statistics.median(times[True])
        blocks = [r["n_line"] + r["n_plane"] for r in infos]
        records.append(dict(what="enqueue -> collect of one batch, ll_reg_set_information off and on alternating", shape=name, scans=B, q_pipe=q_pipe,
                            icp_iterations=args.icp_iters, map_points=args.map_points, build=build_id(), reps=args.reps, warmup=args.warmup,
                            blocks_per_scan_median=statistics.median(blocks), computed=sum(r["status"] == 0 for r in infos),
                            off_median_ms=off, off_min_max_ms=[1e3 * min(times[False]), 1e3 * max(times[False])],
                            on_median_ms=on, on_min_max_ms=[1e3 * min(times[True]), 1e3 * max(times[True])],
                            enabled_cost_ms=on - off, enabled_cost_share_of_registration=(on - off) / off,
                            information_kernel_ms=kernel_ms, kernel_share_of_registration=kernel_ms / off,
                            registration_kernels_ms=[float(v) for v in ms], registration_launches=[int(v) for v in launches]))
        for h in (fe, reg) + (vox or ()):
            h.close()
    mp.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
