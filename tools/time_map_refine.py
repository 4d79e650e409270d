#!/usr/bin/env python3
"""Times the two routes from K stored key-frame clouds to their corrected, filtered clouds (refine_pointcloud( ..., if_save = 0 ),
ceres_pose_graph_3d.hpp:476-485), on one device in one process:

  per-cloud  one api.VoxelGrid.filter per cloud, host in and host out, and the move of refine_pts in numpy -- what the existing entry
             points allow;
  refine     ONE api.Map_refine.refine over all K clouds, which stay on the device; the outputs are fetched once.

The clouds are generated from a seed: a world of planes (a floor, walls) and edges (posts), sampled around K sensor positions and put
through the 0.5 m filter of the add, about 50 k points each.  Both routes are warmed up, then timed alternately with a device
synchronise inside every timed region; medians and ranges are reported, the two routes' floats must be equal bit for bit in every
repetition, and one JSON record per K is written.  --run-only K runs nothing but the adds and one refine of K clouds: the process a
kernel trace is taken of.  Needs a HIP device: there is no fall-back."""
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

ADD_LEAF, RUN_LEAF = 0.5, 0.2


def world_cloud(rng, centre, n_raw=80_000):
    """points of a floor, four walls and a dozen posts within 60 m of centre: planes and edges, as a key frame's accumulated cloud has them"""
    n_floor, n_wall, n_post = n_raw // 2, n_raw // 3, n_raw - n_raw // 2 - n_raw // 3
    floor = np.c_[rng.uniform(-60, 60, (n_floor, 2)), rng.normal(0, 0.02, n_floor)]
    side = rng.integers(0, 4, n_wall)
    along, up = rng.uniform(-60, 60, n_wall), rng.uniform(0, 12, n_wall)
    off = np.where(side < 2, -60.0, 60.0) + rng.normal(0, 0.02, n_wall)
    wall = np.where((side % 2 == 0)[:, None], np.c_[off, along, up], np.c_[along, off, up])
    posts = rng.uniform(-50, 50, (12, 2))
    which = rng.integers(0, 12, n_post)
    post = np.c_[posts[which] + rng.normal(0, 0.03, (n_post, 2)), rng.uniform(0, 8, n_post)]
    xyz = np.concatenate([floor, wall, post]) + np.asarray(centre)
    return np.c_[xyz, rng.uniform(0, 255, len(xyz))].astype(np.float32)


def poses(k, rng):
    ori, opm = np.zeros((k, 7)), np.zeros((k, 7))
    q = rng.normal(0, 1, (k, 4))
    ori[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    q = ori[:, :4] + rng.normal(0, 0.01, (k, 4))
    opm[:, :4] = q / np.linalg.norm(q, axis=1, keepdims=True)
    ori[:, 4:] = np.c_[np.arange(k) * 3.0, rng.uniform(-5, 5, (k, 2))]
    opm[:, 4:] = ori[:, 4:] + rng.normal(0, 0.3, (k, 3))
    return ori, opm


def move_np(R, T, xyz):
    """refine_pts' float move: out_i = ( R_i0 x + ( R_i1 y + R_i2 z ) ) + T_i, intensity 0"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.zeros((len(xyz), 4), np.float32)
    for i in range(3):
        out[:, i] = (R[i, 0] * x + (R[i, 1] * y + R[i, 2] * z)) + T[i]
    return out


def filled(k, seed=9):
    """(Map_refine with K clouds, the stored clouds on the host, poses)"""
    from loam_livox_amd.api import Map_refine
    rng = np.random.default_rng(seed)
    mr = Map_refine(initial_points=1 << 20)
    ori, opm = poses(k, rng)
    stored = []
    base = [world_cloud(rng, (0.0, 0.0, 0.0)) for _ in range(min(k, 4))]      # four worlds, shifted: the generation is not what is timed
    for j in range(k):
        c = base[j % len(base)].copy()
        c[:, :3] += np.float32(ori[j, 4:])
        cid, _, st = mr.add_cloud(c, ADD_LEAF)
        assert cid == j and st == 0
        stored.append(mr.cloud(cid))
    return mr, stored, ori, opm


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--keyframes", type=int, nargs="+", default=[1, 20, 200], help="stored key frames K, one record each")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_refine.json"))
    ap.add_argument("--run-only", type=int, default=0, metavar="K", help="the adds and ONE refine of K clouds, nothing else (for a kernel trace)")
    args = ap.parse_args()
    if args.reps < 11:
        ap.error("at least 11 repetitions")

    from loam_livox_amd.api import VoxelGrid, map_refine_affine
    from tools.build_id import build_id
    hip = ctypes.CDLL("libamdhip64.so")
    n_dev = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n_dev)) != 0 or n_dev.value < 1:
        sys.exit("no HIP device")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            sys.exit("hipDeviceSynchronize failed")

    if args.run_only:
        k = args.run_only
        mr, stored, ori, opm = filled(k)
        out = mr.refine(list(range(k)), ori, opm, RUN_LEAF)
        sync()
        print(json.dumps(dict(run_only=k, work=mr.work().tolist(), points_in=int(sum(len(c) for c in stored)), points_out=int(sum(len(c) for c in out)),
                              build=build_id())))
        mr.close()
        return

    records = []
    for k in args.keyframes:
        mr, stored, ori, opm = filled(k)
        ids = list(range(k))
        vg = VoxelGrid(max_points=max(len(c) for c in stored))
        vg.setLeafSize(RUN_LEAF, RUN_LEAF, RUN_LEAF)

        def per_cloud_route():
            out = []
            for j in ids:
                vg.setInputCloud(stored[j])
                f = vg.filter()
                R, T = map_refine_affine(ori[j], opm[j])
                out.append(move_np(R, T, f))
            sync()
            return out

        def refine_route():
            out = mr.refine(ids, ori, opm, RUN_LEAF)
            sync()
            return out

        t_per, t_ref = [], []
        for rep in range(args.warmup + args.reps):
            got = {}
            for name, route, into in (("per_cloud", per_cloud_route, t_per), ("refine", refine_route, t_ref)):   # alternating
                sync()
                t0 = time.perf_counter()
                got[name] = route()
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    into.append(dt)
            for a, b in zip(got["per_cloud"], got["refine"]):
                assert a.tobytes() == b.tobytes(), f"the two routes differ (K = {k}, repetition {rep})"
        med_per, med_ref = statistics.median(t_per), statistics.median(t_ref)
        rec = dict(what="K stored key-frame clouds filtered at 0.2 m and moved: K VoxelGrid.filter + numpy against one Map_refine.refine",
                   keyframes=k, points_in=int(sum(len(c) for c in stored)), points_out=int(sum(len(c) for c in got["refine"])), build=build_id(),
                   reps=args.reps, warmup=args.warmup, refine_work=mr.work().tolist(), per_cloud_median_ms=1e3 * med_per, refine_median_ms=1e3 * med_ref,
                   per_cloud_min_max_ms=[1e3 * min(t_per), 1e3 * max(t_per)], refine_min_max_ms=[1e3 * min(t_ref), 1e3 * max(t_ref)],
                   per_cloud_over_refine=med_per / med_ref, routes_bit_equal=True)
        if k == 1:
            # the condition at K = 1: the new route's median is not above the per-cloud median by more than that route's own range
            rec["k1_condition_holds"] = bool(med_ref <= med_per + (max(t_per) - min(t_per)))
        records.append(rec)
        vg.close()
        mr.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
