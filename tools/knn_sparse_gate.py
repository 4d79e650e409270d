#!/usr/bin/env python3
"""Per ICP iteration: how many surface queries of the headline batch (bench.py: C2 Q-full, B = 256) would keep their neighbour list.

The registrar runs in its `knn_tile_with_reuse` mode -- tile search at ICP iterations 0 and 1, reuse records and work lists afterwards --
once per iteration count K = 3 .. icp-iters, and the work-list counters of the LAST iteration (K - 1) are read back
(Point_cloud_registration.debug_worklists_by_kind): queries whose list provably holds in order (strong-stable: nothing to do), queries
whose set holds (re-sort) and queries that need a search.  Then the same loop with the default switches: how many queries the sparse
tile search of every late iteration was handed (a library without that mode reports none).  The batch, the initial guesses and the parameters are bench.py's.  One JSON
record.  Needs a HIP device: no fall-back."""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--map-points", type=int, default=5_000_000)
    ap.add_argument("--scan-points", type=int, default=24000)
    ap.add_argument("--icp-iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_sparse_gate.json"))
    args = ap.parse_args()

    import bench
    from loam_livox_amd import synth
    from loam_livox_amd.api import Livox_laser, Map_buffer, Point_cloud_registration
    from tools.build_id import build_id

    B, N = args.batch, args.scan_points
    world, corner, surf = synth.make_maps(args.map_points)
    base = bench.make_scans(synth, world, list(range(B)), N)
    rng = np.random.default_rng(4242)
    scans = np.stack([s.xyzi for s in base])
    init = np.stack([synth.pose_compose(base[b].pose_true,
                                        np.r_[synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 1.0))), rng.uniform(-0.1, 0.1, 3)])
                     for b in range(B)])
    mp = Map_buffer()
    mp.setInputCloud(Map_buffer.CORNER, corner)
    mp.setInputCloud(Map_buffer.SURF, surf)
    fe = Livox_laser(max_points=N, max_scans=B, piecewise_number=1)
    fe.upload(scans, np.full(B, 1.0))
    fe.extract_batch(B)
    fe.resolve()
    fe.select_batch(B, -1, 0.0, 1.0)
    reg = Point_cloud_registration(max_scans=B, max_features=N)
    p = reg.params
    p.ceres_max_iterations, p.force_all_iterations = 20, 1
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 1000.0
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    p.maximum_allow_residual_block = N
    reg.set_debug(False, knn_tile_with_reuse=True)
    n_surf = int(np.asarray(fe.counts(B)[1]).sum())
    rows = []
    for k in range(3, args.icp_iters + 1):
        p.icp_max_iterations = k
        reg.enqueue_fe(mp, fe, B, init, init)
        reg.collect(B)
        _, (searched, resorted) = reg.debug_worklists_by_kind(B)
        rows.append({"icp_iteration": k - 1, "search": searched, "resort": resorted, "strong_stable": n_surf - searched - resorted,
                     "unsettled_share": round((searched + resorted) / n_surf, 5)})
    # the mode that was built on this record (default switches): the registrar adds every sparse iteration's list lengths up
    # (ll_knn_kernels.hip, reg_knn_lane_kernel); the difference between K and K - 1 iterations is iteration K - 1's list
    reg.set_debug(False)
    listed, before = [], 0
    for k in range(1, args.icp_iters + 1):
        p.icp_max_iterations = k
        reg.enqueue_fe(mp, fe, B, init, init)
        reg.collect(B)
        total = reg.debug_worklists_by_kind(B)[0][1]
        listed.append({"icp_iteration": k - 1, "listed": total - before, "share": round((total - before) / n_surf, 5)})
        before = total
    rec = dict(listed_by_the_sparse_tile_search=[r for r in listed if r["listed"]], what="surface queries of the headline batch per ICP iteration by reuse class (knn_tile_with_reuse: records of the tile search at "
                    "iteration 1, of the list kernel afterwards; guard band 5 cm)", scans=B, scan_points=N, map_points=args.map_points,
               surface_queries=n_surf, per_iteration=rows, build=build_id())
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))
    for h in (fe, reg, mp):
        h.close()


if __name__ == "__main__":
    main()
