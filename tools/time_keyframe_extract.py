#!/usr/bin/env python3
"""Times the two routes by which Keyframe_assembly turns a key frame's cell set into a cell map of its own, on one device in one process:

  host    Keyframe_assembly._materialize_host -- ll_cellmap_dump of the whole full map, numpy's isin and gather, a fresh Cell_map and
          append_cloud (radix sort, gather, scan, table build) -- followed by keyframe_images();
  device  Cell_map.extract_cells into a fresh Cell_map (ll_cellmap_extract_cells: mark, scan, table, gather) followed by keyframe_images().

The full map is built the way the mapping loop builds it: synthetic Mid-40 scans (loam_livox_amd.synth) taken along a path that goes out
and comes back inside the synthetic rooms, each moved into the map frame with its true pose and appended with append_cloud_touched.  The
key frame is the union of the touched-cell lists of the middle third of the scans.  Both routes are warmed up, then timed alternately
with a device synchronise inside every timed region; the medians are reported, the two routes' dumps and images must be equal bit for
bit, and one JSON record is written.  Needs a HIP device: there is no fall-back."""
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


def build_full_map(ka, n_scans: int, scan_points: int):
    from loam_livox_amd import synth
    world = synth.world_for_map_size(200_000)
    rng = np.random.default_rng(77)
    start = synth.sensor_pose_in_world(world, rng)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    step = np.r_[synth.quat_from_axis_angle(np.array([0.1, 0.2, 1.0]), np.deg2rad(0.4)), np.array([0.04, 0.015, 0.0])]
    back = synth.pose_inverse(step)
    leg = 21                                   # scans per leg: out, back, out, ... so that the sensor stays in its room
    cur, touched = start, []
    for k in range(n_scans):
        if k > 0:
            cur = synth.pose_compose(cur, step if (k // leg) % 2 == 0 else back)
        sc = synth.make_moving_scan(world, 500 + k, scan_points, inc_true=ident, pose_start=cur, t_phase=0.13 * k)
        pose = synth.pose_compose(synth.pose_inverse(start), cur)       # relative to scan 0 = the map frame
        cloud = np.c_[synth.transform_points(pose, sc.xyzi[:, :3]), np.zeros(len(sc.xyzi), np.float32)].astype(np.float32)
        touched.append(ka.add_scan(cloud, pose, k))
    return touched


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scans", type=int, default=84, help="scans appended to the full map (84 x 24000 points: about 2 M)")
    ap.add_argument("--scan-points", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_extract.json"))
    args = ap.parse_args()
    if args.reps < 11:
        ap.error("at least 11 repetitions")

    from loam_livox_amd import keyframes
    from loam_livox_amd.api import Cell_map
    hip = ctypes.CDLL("libamdhip64.so")
    n_dev = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n_dev)) != 0 or n_dev.value < 1:
        sys.exit("no HIP device")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            sys.exit("hipDeviceSynchronize failed")

    # (no key frame closes on its own here: the key frame under test is assembled below)
    ka = keyframes.Keyframe_assembly(scans_of_each_keyframe=1 << 30, scans_between_two_keyframe=1 << 30)
    touched = build_full_map(ka, args.scans, args.scan_points)
    full = ka.m_pt_cell_map_full
    kf = keyframes.Maps_keyframe()
    third = args.scans // 3
    for cells in touched[third:2 * third]:
        kf.add_cells(cells)
    want = keyframes._unpack_cells(np.fromiter(kf.m_set_cell, np.int64, len(kf.m_set_cell)))

    def host_route():
        km = ka._materialize_host(kf)
        img = km.keyframe_images()
        sync()
        return km, img

    def device_route():
        km = Cell_map(max(1024, len(want)), ka.m_pt_cell_resolution, device=ka.device)
        full.extract_cells(want, km)
        img = km.keyframe_images()
        sync()
        return km, img

    # equality first: the two routes' maps and images, bit for bit
    (ma, ia), (mb, ib) = host_route(), device_route()
    da, db = ma.dump(), mb.dump()
    assert all(same_bits(x, y) for x, y in zip(da, db)) and ma.stats() == mb.stats(), "the two routes' maps differ"
    assert sorted(ia) == sorted(ib) and all(same_bits(np.asarray(ia[k]), np.asarray(ib[k])) for k in ia), "the two routes' images differ"
    sel_cells, sel_points, _ = mb.stats()
    ma.close()
    mb.close()

    t_host, t_dev, t_call = [], [], []
    scratch = Cell_map(max(1024, sel_points), ka.m_pt_cell_resolution, device=ka.device)
    for rep in range(args.warmup + args.reps):
        for route, into in ((host_route, t_host), (device_route, t_dev)):   # alternating: both see the same neighbours on the machine
            sync()
            t0 = time.perf_counter()
            km, _ = route()
            dt = time.perf_counter() - t0
            km.close()
            if rep >= args.warmup:
                into.append(dt)
        sync()
        t0 = time.perf_counter()
        full.extract_cells(want, scratch)                                    # the extraction call alone, into a map that has the room
        sync()
        if rep >= args.warmup:
            t_call.append(time.perf_counter() - t0)
    scratch.close()
    n_cells, n_points, _ = full.stats()
    rec = dict(what="key frame out of the full map: host route (dump, isin, append) against ll_cellmap_extract_cells, each followed by keyframe_images()",
               map_points=n_points, map_cells=n_cells, scans=args.scans, listed_cells=len(want), selected_cells=sel_cells, selected_points=sel_points,
               reps=args.reps, warmup=args.warmup, host_route_median_ms=1e3 * statistics.median(t_host),
               device_route_median_ms=1e3 * statistics.median(t_dev), extract_call_median_ms=1e3 * statistics.median(t_call),
               host_route_min_max_ms=[1e3 * min(t_host), 1e3 * max(t_host)], device_route_min_max_ms=[1e3 * min(t_dev), 1e3 * max(t_dev)],
               routes_bit_equal=True)
    ka.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
