#!/usr/bin/env python3
"""Times one round of key-frame adds in the lock-step loop with map refinement, on one device in one process: S key frames (one per
sequence), each the accumulated cloud of --scans logged scans of --points points, into the refine store at 0.5 m by

  add_logged  ONE api.Map_refine.add_logged over the S groups, device to device (one gather, one filter chain, one host wait);
  host        the route it replaces: per key frame History_buffer_batch.read_group (the host concatenation of its scans) and
              api.Map_refine.add_cloud.

Every repetition fills a fresh scan log (append_full + log_full per step, the same scans under a pose that moves with the step; not
timed as a whole), times the host route -- which leaves the groups alone -- and then add_logged, which consumes them, so the two
routes alternate within a repetition and always in that order; each timed region ends with a device synchronise, medians and ranges
are reported, and the stored clouds of the two routes must be equal bit for bit.  Beside that, per step of the fill: the wall time of the log_full call alone
(it enqueues and returns) and of the call with a device synchronise behind it.  One JSON record per S.  Needs a HIP device: there is no
fall-back."""
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

LEAF = 0.5


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sequences", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--scans", type=int, default=100, help="logged scans per key frame (maximum_history_size)")
    ap.add_argument("--points", type=int, default=24000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_refine_batch.json"))
    args = ap.parse_args()

    from loam_livox_amd import synth
    from loam_livox_amd.api import History_buffer_batch, Livox_laser, Map_refine
    from tools.build_id import build_id
    hip = ctypes.CDLL("libamdhip64.so")
    n_dev = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n_dev)) != 0 or n_dev.value < 1:
        sys.exit("no HIP device")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            sys.exit("hipDeviceSynchronize failed")

    world, _, _ = synth.make_maps(200_000)
    P = args.points
    records = []
    for S in args.sequences:
        fe = Livox_laser(max_points=P, max_scans=S, piecewise_number=1)
        base = [synth.make_scan(world, k % 8, n=P) for k in range(min(S, 8))]
        fe.upload(np.stack([np.ascontiguousarray(base[s % len(base)].xyzi, np.float32) for s in range(S)]), np.ones(S))
        fe.extract_batch(S)
        fe.resolve()
        fe.select_batch(S, -1, 0.0, 1.0)
        n_full = [len(fe.get_features(0.0, 1.0, scan=s)["full_idx"]) for s in range(min(S, 8))]
        t_log_call, t_log_sync = [], []

        def filled():
            """a fresh batch whose scan log holds args.scans scans per slot -> (batch, one group per slot)"""
            hb = History_buffer_batch(S, args.scans, P, 0.1, 0.4)
            hb.enable_full_maps(args.scans * P, 1.0, 5000)
            hb.enable_scan_log(args.scans, S * (args.scans + 1))
            poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (S, 1))
            for t in range(args.scans):
                poses[:, 4] = 0.05 * t
                hb.append_full(fe, poses, None, 3, lists=False)
                sync()
                t0 = time.perf_counter()
                hb.log_full(fe)
                t1 = time.perf_counter()
                sync()
                t_log_call.append(t1 - t0)
                t_log_sync.append(time.perf_counter() - t0)
            return hb, [hb.hand_over(s) for s in range(S)]

        mr_dev, mr_host = Map_refine(1 << 22), Map_refine(1 << 22)
        t_dev, t_host, points_in, work, equal = [], [], 0, None, True
        for rep in range(args.warmup + args.reps):
            hb, groups = filled()
            first = len(mr_dev)

            def host_route():
                for g in groups:
                    mr_host.add_cloud(hb.read_group(g), LEAF)
                sync()

            def device_route():
                mr_dev.add_logged(hb, [[g] for g in groups], LEAF)
                sync()

            sync()
            t0 = time.perf_counter()
            host_route()       # (reads the groups and leaves them; so it runs first, and the alternation is in which handle is warm)
            t1 = time.perf_counter()
            device_route()
            t2 = time.perf_counter()
            if rep >= args.warmup:
                t_host.append(t1 - t0)
                t_dev.append(t2 - t1)
            work = mr_dev.work().tolist()
            points_in = int(work[3])
            for k in (0, S - 1):
                equal = equal and mr_dev.cloud(first + k).tobytes() == mr_host.cloud(first + k).tobytes()
            hb.close()
        assert equal, "the two routes' stored clouds differ"
        med_dev, med_host = statistics.median(t_dev), statistics.median(t_host)
        med_call, med_sync = statistics.median(t_log_call), statistics.median(t_log_sync)
        log_bytes = 32.0 * S * statistics.mean(n_full)   # 16 B read + 16 B written per logged point
        records.append(dict(what="one round: S key frames of `scans` logged scans into the refine store at 0.5 m; add_logged against read_group + add_cloud per key frame",
                            sequences=S, scans=args.scans, points=P, full_selection_points=n_full, points_in=points_in, build=build_id(), reps=args.reps,
                            warmup=args.warmup, add_logged_median_ms=1e3 * med_dev, add_logged_min_max_ms=[1e3 * min(t_dev), 1e3 * max(t_dev)],
                            host_route_median_ms=1e3 * med_host, host_route_min_max_ms=[1e3 * min(t_host), 1e3 * max(t_host)],
                            host_over_add_logged=med_host / med_dev, add_logged_work=work, routes_bit_equal=True,
                            log_full_call_median_us=1e6 * med_call, log_full_call_and_sync_median_us=1e6 * med_sync,
                            log_full_bytes_per_step=log_bytes, log_full_GBps_of_call_and_sync=log_bytes / med_sync / 1e9))
        mr_dev.close()
        mr_host.close()
        fe.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
