#!/usr/bin/env python3
"""Spinning-lidar feature extraction on one MI355X (ll_spin_*, the lidar_type != "livox" branch of the feature node,
hku-mars/loam_livox source/laser_feature_extractor.hpp:393-787).  Prints one JSON line.

  vlp16  B = 256 VLP-16 scans (1800 azimuths x 16 beams = 28.8 k points), one batch at a time, scans resident in HBM;
  hdl64  B = 64 HDL-64-like scans (2000 azimuths x 64 beams, ~102 k points kept by the 0..50 scan-ID rule).
A timed step is ll_spin_extract_batch + ll_spin_resolve (which synchronises): the whole extraction of a resident batch, the
per-line VoxelGrid included.  scans/s = B / median step.  kernels_ms: the phases of the last step from HIP events on the
handle's stream.  latency_ms: one message through ll_spin_extract (upload, extract, resolve) and through the Python call that
also downloads the five clouds.  bytes: what the algorithm has to move per batch (inputs read once, every intermediate plane
written and read once, outputs written once), against the HBM bound (8 TB/s).  cpu_baseline: the host restatement
(tests/spin_ref.c + the oracle VoxelGrid) on one core.  parity: the last timed batch against the restatement -- index sets and
x, y, z must be identical (max_index_mismatch = scans with any difference), intensities are counted where they differ."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
HBM_GBS = 8000.0
# bytes per input point the pipeline has to move: assign (16 in, 8 out), lines (24 in, 20 out), curvature (16 in, 6 out),
# sort (4 in, 4 out), select (~25 in, 4 out), less-flat staging + VoxelGrid + gather (~16 in/out three times)
BYTES_PER_POINT = 16 + 8 + 24 + 20 + 16 + 6 + 4 + 4 + 25 + 4 + 48


def run_config(name, scan_line, B, n_azimuth, steps, warmup, world, parity):
    from loam_livox_amd import capi, synth
    from loam_livox_amd.api import Spinning_laser
    t0 = time.time()
    scans = [synth.make_spin_scan(world, 7000 + k, scan_line=scan_line, n_azimuth=n_azimuth).xyzi for k in range(B)]
    synth_s = time.time() - t0
    n_pts = np.array([len(s) for s in scans])
    dev = Spinning_laser(scan_line=scan_line, max_points=int(n_pts.max()), max_scans=B, max_line_points=4096)
    dev.upload(scans)
    L = dev.L
    times = []
    for it in range(warmup + steps):
        t = time.perf_counter()
        capi.check(L.ll_spin_extract_batch(dev.h, B), "extract_batch")
        n_amb = capi.check(L.ll_spin_resolve(dev.h), "resolve")
        dt = time.perf_counter() - t
        if it >= warmup:
            times.append(dt)
    kms = dev.kernel_times()
    counts, status = dev.counts(B)
    med = float(np.median(times))
    kept = int(counts[:, 0].sum())
    out = {"B": B, "points_in": int(n_pts.sum()), "points_kept": kept, "scans_per_s": B / med, "step_ms_median": med * 1e3,
           "step_ms_min": float(np.min(times)) * 1e3, "kernels_ms": dict(zip(["assign", "lines", "curvature", "sort", "select", "voxel_gather"],
                                                                              [round(float(x), 4) for x in kms])),
           "ambiguous_points": int(n_amb), "status_nonzero": int(np.count_nonzero(status)),
           "features_per_scan": {k: float(counts[:, i].mean()) for i, k in enumerate(["full", "sharp", "less_sharp", "flat", "less_flat"])}}
    moved = BYTES_PER_POINT * int(n_pts.sum())
    out["bytes"] = {"algorithmic_per_batch": moved, "hbm_bound_ms": moved / (HBM_GBS * 1e9) * 1e3,
                    "achieved_gbs": moved / med / 1e9, "fraction_of_bound": (moved / (HBM_GBS * 1e9)) / med}
    if parity:
        from tests import spin_ref
        mism, int_diff, worst = 0, 0, 0.0
        cpu_t = []
        for b in range(B):
            t = time.perf_counter()
            ref = spin_ref.extract(scans[b], scan_line=scan_line)
            cpu_t.append(time.perf_counter() - t)
            c = dev.clouds(b)
            ok = (np.array_equal(c["full_src"], ref["full_src"]) and np.array_equal(c["/laser_points_2"][:, :3], ref["full"][:, :3])
                  and all(np.array_equal(c[k], ref[k]) for k in ("sharp", "less_sharp", "flat", "less_flat_pre"))
                  and np.array_equal(c["/laser_cloud_less_flat"][:, :3], ref["less_flat"][:, :3]))
            mism += 0 if ok else 1
            if ok:
                d = np.abs(c["/laser_points_2"][:, 3].astype(np.float64) - ref["full"][:, 3])
                int_diff += int(np.count_nonzero(d))
                worst = max(worst, float(d.max()) if len(d) else 0.0)
        out["parity"] = {"scans_checked": B, "max_index_mismatch": mism, "intensity_differ": int_diff, "intensity_max_abs_diff": worst}
        out["cpu_baseline"] = {"scans_per_s_one_core": 1.0 / float(np.median(cpu_t)), "ms_per_scan_median": float(np.median(cpu_t)) * 1e3,
                               "what": "tests/spin_ref.c restatement (gcc -O2) + oracle VoxelGrid, one thread"}
        out["speedup_vs_one_core"] = out["scans_per_s"] / out["cpu_baseline"]["scans_per_s_one_core"]
    out["synth_s"] = round(synth_s, 2)
    if scan_line == 16:  # one-message latency
        one = Spinning_laser(scan_line=16, max_points=int(n_pts.max()))
        x = np.ascontiguousarray(scans[0])
        lat_c, lat_py = [], []
        for it in range(warmup + steps):
            t = time.perf_counter()
            capi.check(L.ll_spin_extract(one.h, x.ctypes.data_as(C.c_void_p), len(x)), "extract")
            t1 = time.perf_counter()
            one.extract(x)
            t2 = time.perf_counter()
            if it >= warmup:
                lat_c.append(t1 - t)
                lat_py.append(t2 - t1)
        out["latency_ms"] = {"ll_spin_extract": float(np.median(lat_c)) * 1e3, "python_extract_with_downloads": float(np.median(lat_py)) * 1e3}
        one.close()
    dev.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-parity", action="store_true")
    ap.add_argument("--only", default="", help="vlp16 or hdl64")
    a = ap.parse_args()
    from loam_livox_amd import synth
    world = synth.make_world(4, 4)
    res = {"bench": "spin", "device": "MI355X (gfx950)"}
    if a.only in ("", "vlp16"):
        res["vlp16"] = run_config("vlp16", 16, 256, 1800, a.steps, a.warmup, world, not a.no_parity)
    if a.only in ("", "hdl64"):
        res["hdl64"] = run_config("hdl64", 64, 64, 2000, a.steps, a.warmup, world, not a.no_parity)
    head = res.get("vlp16") or res.get("hdl64")
    res["metric"] = "scans_per_s_vlp16_b256" if "vlp16" in res else "scans_per_s_hdl64_b64"
    res["value"] = head["scans_per_s"]
    res["parity"] = {"max_index_mismatch": sum(res[k]["parity"]["max_index_mismatch"] for k in ("vlp16", "hdl64") if k in res and "parity" in res[k]),
                     "intensity_differ": sum(res[k]["parity"]["intensity_differ"] for k in ("vlp16", "hdl64") if k in res and "parity" in res[k])} \
        if not a.no_parity else "not measured"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
