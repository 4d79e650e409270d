#!/usr/bin/env python3
"""Times api.Pose_graph.solve -- the pose-graph optimisation of an accepted loop, one workgroup per graph, the whole Levenberg-Marquardt
loop inside one launch -- on one device in one process: milliseconds per call for G = 1 and G = 64 copies of a detector-shaped graph
(tests/pose_graph_inputs.py: a drifted closed loop, chain constraints from the estimates, one loop constraint) of N = 33 and N = 300
poses, with the iterations a call ran.  Every configuration is warmed up, then timed with a device synchronise inside the timed region;
medians and ranges of the repetitions are reported and one JSON record per configuration is written.  There is no speed bar: one
sequential graph on one workgroup is not meant to beat a CPU sparse solver.  Needs a HIP device: there is no fall-back."""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", type=int, nargs="+", default=[33, 300], help="poses N of the graph, one record per N and G")
    ap.add_argument("--graphs", type=int, nargs="+", default=[1, 64], help="graphs G of a call")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_graph.json"))
    args = ap.parse_args()
    if args.reps < 11:
        ap.error("at least 11 repetitions")

    from loam_livox_amd.api import Pose_graph
    from tests.pose_graph_inputs import make_graph
    from tools.build_id import build_id
    hip = ctypes.CDLL("libamdhip64.so")
    n_dev = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n_dev)) != 0 or n_dev.value < 1:
        sys.exit("no HIP device")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            sys.exit("hipDeviceSynchronize failed")

    records = []
    for n in args.poses:
        g = make_graph(n, [(n - 1, 1)], seed=4)
        graph = dict(poses=g["poses"], ab=g["ab"], meas=g["meas"])
        for G in args.graphs:
            blocks = Pose_graph.envelope_blocks(n, g["ab"])
            handle = Pose_graph(max_graphs=G, max_poses=G * n, max_edges=G * len(g["ab"]), max_envelope_blocks=G * blocks)
            times, first = [], None
            for rep in range(args.warmup + args.reps):
                sync()
                t0 = time.perf_counter()
                poses, summaries = handle.solve([graph] * G)
                sync()
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    times.append(dt)
                first = first if first is not None else poses[0].tobytes()
                assert all(p.tobytes() == first for p in poses), "a graph's result depends on its slot or on the run"
            s = summaries[0]
            records.append(dict(what="Pose_graph.solve of G copies of a detector-shaped graph of N poses", poses=n, edges=len(g["ab"]), graphs=G,
                                envelope_blocks_per_graph=blocks, build=build_id(), reps=args.reps, warmup=args.warmup, work=handle.work().tolist(),
                                iterations=s["iterations"], successful_steps=s["successful_steps"], termination=s["termination"],
                                median_ms=1e3 * statistics.median(times), min_max_ms=[1e3 * min(times), 1e3 * max(times)]))
            handle.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
