#!/usr/bin/env python3
"""Times the two routes by which the loop detector aligns a candidate pair of key frames (Scene_alignment::find_tranfrom_of_two_mappings,
scene_alignment.hpp:269-391), on one device in one process:

  host    loam_livox_amd.scene_alignment.Scene_alignment as Keyframe_assembly uses it by default: a fresh object per pair, both cell maps
          dumped, the line / plane points picked with numpy, every cloud through the VoxelGrid, the map and the registrar as host arrays;
  device  Scene_alignment( on_device=True ) kept across pairs, as Keyframe_assembly( device_alignment=True ) keeps it: ll_scene_align_run.

The key frames are synthetic scenes of planes, lines and blobs (3000 / 800 / 500 points each, a third of the objects of each kind) some
tens of metres from the origin; key frame b is a's scene under a small rigid motion with noise, each keeping 80 % of the points.  The
settings are the loop detector's (laser_mapping.hpp:700-706: 0.2 m, 2 ICP iterations, 0.35).  Both routes are warmed up, then timed
alternately with a device synchronise inside every timed region; the medians are reported, the two routes' thresholds and poses must be
equal bit for bit, and one JSON record per shape is written.  Needs a HIP device: there is no fall-back."""
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


def scene(n_objects: int, seed: int = 5):
    rng = np.random.default_rng(seed)
    half = 8.0 * (n_objects / 40.0) ** (1.0 / 3.0)     # (the density of the 40-object scene at every size)
    pts = []
    for i in range(n_objects):
        o = rng.uniform(-half, half, 3) + np.array([30.0, -20.0, 5.0])
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        u = np.cross(n, [0, 0, 1.0])
        u /= np.linalg.norm(u)
        v = np.cross(n, u)
        if i % 3 == 0:
            p = o + rng.uniform(-1.5, 1.5, (3000, 1)) * u + rng.uniform(-1.5, 1.5, (3000, 1)) * v + rng.normal(0, 0.01, (3000, 3))
        elif i % 3 == 1:
            p = o + rng.uniform(-2, 2, (800, 1)) * u + rng.normal(0, 0.01, (800, 3))
        else:
            p = o + rng.normal(0, 0.3, (500, 3))
        pts.append(p)
    return np.concatenate(pts)


def pair(n_objects: int, seed: int = 3):
    from loam_livox_amd import synth
    xyz = scene(n_objects)
    rng = np.random.default_rng(seed)
    T = np.r_[synth.quat_from_axis_angle(np.array([0.1, 0.2, 1.0]), np.deg2rad(1.5)), [0.35, -0.2, 0.1]]
    R = synth.quat_to_mat(T[:4])
    keep = rng.uniform(size=len(xyz)) < 0.8
    b = ((xyz[keep] - T[4:]) @ R) + rng.normal(0, 0.005, (int(keep.sum()), 3))
    a = xyz[rng.uniform(size=len(xyz)) < 0.8]
    z = lambda p: np.c_[p, np.zeros(len(p))].astype(np.float32)
    return z(a), z(b)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, nargs="+", default=[40, 400], help="objects per scene, one shape each (40: about 46 k points per key frame)")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_align.json"))
    args = ap.parse_args()
    if args.reps < 11:
        ap.error("at least 11 repetitions")

    from loam_livox_amd.api import Cell_map
    from loam_livox_amd.scene_alignment import Scene_alignment
    hip = ctypes.CDLL("libamdhip64.so")
    n_dev = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n_dev)) != 0 or n_dev.value < 1:
        sys.exit("no HIP device")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            sys.exit("hipDeviceSynchronize failed")

    settings = dict(line_res=0.2, plane_res=0.2, maximum_icp_iteration=2, accepted_threshold=0.35, maximum_residual_block=5000)
    records = []
    for n_objects in args.objects:
        a, b = pair(n_objects)
        da, db = Cell_map(len(a), 1.0), Cell_map(len(b), 1.0)
        da.append_cloud(a)
        db.append_cloud(b)
        kept = Scene_alignment(on_device=True, **settings)

        def host_route():
            sa = Scene_alignment(**settings)
            thr = sa.find_tranfrom_of_two_mappings(da, db)
            sync()
            return thr, sa.pose.copy(), len(sa.reports)

        def device_route():
            thr = kept.find_tranfrom_of_two_mappings(da, db)
            sync()
            return thr, kept.pose.copy(), len(kept.reports)

        h, d = host_route(), device_route()
        assert np.float64(h[0]).tobytes() == np.float64(d[0]).tobytes() and h[1].tobytes() == d[1].tobytes() and h[2] == d[2], "the two routes differ"
        t_host, t_dev = [], []
        for rep in range(args.warmup + args.reps):
            for route, into in ((host_route, t_host), (device_route, t_dev)):   # alternating: both see the same neighbours on the machine
                sync()
                t0 = time.perf_counter()
                route()
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    into.append(dt)
        work = kept._aligner.work()
        line_a, plane_a, _ = da.feature_clouds()
        line_b, plane_b, _ = db.feature_clouds()
        records.append(dict(what="scene alignment of one candidate pair: host route (a Scene_alignment per pair) against ll_scene_align_run (one handle kept)",
                            objects=n_objects, points_a=len(a), points_b=len(b), cells_a=da.stats()[0], cells_b=db.stats()[0],
                            line_plane_points_a=[len(line_a), len(plane_a)], line_plane_points_b=[len(line_b), len(plane_b)], settings=settings,
                            registrations=d[2], inlier_threshold=d[0], device_host_waits=int(work[1]), reps=args.reps, warmup=args.warmup,
                            host_route_median_ms=1e3 * statistics.median(t_host), device_route_median_ms=1e3 * statistics.median(t_dev),
                            host_route_min_max_ms=[1e3 * min(t_host), 1e3 * max(t_host)], device_route_min_max_ms=[1e3 * min(t_dev), 1e3 * max(t_dev)],
                            routes_bit_equal=True))
        kept.close()
        da.close()
        db.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
