"""Times the deskewed clouds on the device and writes profiles/undistort.json (DESIGN "Deskewed clouds").

  python tools/time_undistort.py [--reps 11] [--batch 256] [--out profiles/undistort.json]

Every figure is the median of `--reps` repetitions, the variants of a comparison alternating inside one repetition, after a warm-up of
every shape; a repetition is a host clock around calls that end in a device synchronise (each entry point synchronises its stream).
  history_add     a 24 k-point scan's History_buffer.add_fe with and without set_undistort (fresh frames into a full history)
  submap          B slots of 24 k-point scans: cloud_undistort_fe_device (full selection), append_to_submap_device on the same clouds
                  (kinds 0 + 1: it has no full selection), and the host round trip that was the only way to a deskewed sub-map before:
                  read the selections back, numpy restatement of PCR:641-646, upload
  kernel          cloud_undistort_kernel alone, on the surface selections: its time from a kernel trace taken in a run of its own
                  (`rocprofv3 --kernel-trace --stats ... -- python tools/time_undistort.py --trace-only`, handed over with
                  --kernel-stats), and the bytes it moves (32 per point) over that time against the guide's HBM figure.  The call with
                  every slot accepted minus the call with none is written beside it as a rough cross-check, no more: the calls'
                  synchronisations jitter by as much as the kernel takes
No GPU: the script fails (there is no other path)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.29e12   # bytes/s, float4 copy (MI355X microarchitecture guide)


def numpy_undistort(xyzi, it, b, pose_curr, min_ts, max_ts):
    """PCR:622-661 in float64 numpy (the restatement the tests use, inlined: tools do not import tests)"""
    def mat(q):
        x, y, z, w = q
        return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                         [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                         [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    with np.errstate(all="ignore"):
        s = (xyzi[:, 3] - np.float32(min_ts)) / (np.float32(max_ts) - np.float32(min_ts))
    s = np.where(~np.isfinite(s) | (s > 1), np.float32(1), s).astype(np.float64)
    p = xyzi[:, :3].astype(np.float64)
    hat, th = it["omega_hat"][b], it["theta"][b]
    R = np.eye(3)[None] + np.sin(s * th)[:, None, None] * hat[None] + (1 - np.cos(s * th))[:, None, None] * (hat @ hat)[None]
    inner = np.einsum("nij,nj->ni", R, p) + s[:, None] * it["pose_incre"][b][4:][None]
    out = inner @ mat(it["pose_last"][b][:4]).T + it["pose_last"][b][4:]
    end = s == 1.0
    out[end] = p[end] @ mat(pose_curr[:4]).T + pose_curr[4:]
    return np.c_[out.astype(np.float32), xyzi[:, 3]]


def kernel_stats_row(path, kernel):
    """the row of `kernel` in a rocprofv3 kernel_stats.csv (Name, Calls, TotalDurationNs, AverageNs, ..., MinNs, MaxNs)"""
    import csv
    import glob
    files = [path] if os.path.isfile(path) else sorted(glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True))
    for f in files:
        for row in csv.DictReader(open(f)):
            if kernel in row.get("Name", ""):
                return row
    raise SystemExit(f"time_undistort: no row of {kernel} under {path}")


def median_ms(samples):
    return {k: 1e3 * statistics.median(v) for k, v in samples.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--scan-points", type=int, default=24000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "undistort.json"))
    ap.add_argument("--trace-only", action="store_true", help="set up, launch the kernel on the batch's surface selections 20 times and leave: the "
                    "program of a `rocprofv3 --kernel-trace --stats` run")
    ap.add_argument("--kernel-stats", default=None, help="the kernel_stats.csv of such a run (a file, or a directory searched for one): the kernel's time")
    ap.add_argument("--no-deblur", action="store_true", help="with --trace-only: register with if_motion_deblur = 0, so that every point takes the "
                    "kernel's plain branch (no sin / cos): the same traffic without the fp64 transcendentals")
    ap.add_argument("--kernel-stats-plain", default=None, help="the kernel_stats.csv of a `--trace-only --no-deblur` run")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("time_undistort: no GPU")
    from loam_livox_amd import synth
    from loam_livox_amd.api import History_buffer, Livox_laser, Map_buffer, Point_cloud_registration

    N, B = a.scan_points, a.batch
    world, corner, surf = synth.make_maps(200_000)
    m = Map_buffer()
    m.setInputCloud(Map_buffer.CORNER, corner)
    m.setInputCloud(Map_buffer.SURF, surf)
    distinct = [synth.make_moving_scan(world, k, N) for k in range(8)]
    scans = np.stack([distinct[b % 8].xyzi for b in range(B)])
    poses = np.stack([distinct[b % 8].pose_init for b in range(B)])
    t0, dt = 0.5, 1e-5
    fe = Livox_laser(max_points=N, max_scans=B, piecewise_number=1)
    fe.upload(scans, np.full(B, t0))
    fe.extract_batch(B)
    fe.resolve()
    fe.select_batch(B, -1, 0.0, 1.0)
    nc, ns, nf, _ = fe.counts(B)
    reg = Point_cloud_registration(max_scans=B, max_features=N)
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations = 4, 20
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    p.if_motion_deblur, p.minimum_pt_time_stamp, p.maximum_pt_time_stamp = 0 if a.no_deblur else 1, t0, t0 + (N - 1) * dt
    res, pc, _, _ = reg.solve_batch_fe(m, fe, B, poses, poses)
    it = reg.interpolation(B)
    result = {"config": {"batch": B, "scan_points": N, "reps": a.reps, "device": torch.cuda.get_device_name(0),
                         "points": {"corner": int(nc.sum()), "surface": int(ns.sum()), "full": int(nf.sum())}, "accepted": int(res.sum())}}

    if a.trace_only:   # under a kernel trace, in a run of its own: the kernel is launched on the batch's surface selections and nowhere else
        out = torch.zeros((int(ns.sum()) + 8, 4), dtype=torch.float32, device="cuda")
        for _ in range(20):
            reg.cloud_undistort_fe_device(fe, B, 1, np.ones(B, np.int32), out, 0)
        return

    # ---- history add, single scan
    hist = History_buffer(5, N, 0.1, 0.4)
    step = [0]

    def next_pose():   # a millimetre further every time: a full history takes a frame only when the gate pose has moved (LM:1446-1448)
        step[0] += 1
        q = pc[0].copy()
        q[4] += 1e-3 * step[0]
        return q
    for _ in range(6):   # fill the history: every timed add pushes a frame and pops one
        assert hist.add_fe(fe, 0, next_pose())
    t = {"plain": [], "undistort": []}
    for r in range(a.reps + 2):
        for name in (("plain", "undistort") if r % 2 == 0 else ("undistort", "plain")):
            c0 = time.perf_counter()
            if name == "undistort":
                hist.set_undistort(reg, 0)
            assert hist.add_fe(fe, 0, next_pose())
            if r >= 2:
                t[name].append(time.perf_counter() - c0)
    result["history_add_ms"] = median_ms(t)

    # ---- sub-map of B slots
    acc, none = np.ones(B, np.int32), np.zeros(B, np.int32)
    out = torch.zeros((int(nf.sum()) + 8, 4), dtype=torch.float32, device="cuda")
    feats = [fe.get_features(scan=b) for b in range(min(B, 8))]   # the host round trip reads every slot back; 8 slots are timed and scaled

    def undistort_full():
        reg.cloud_undistort_fe_device(fe, B, 2, acc, out, 0)

    def undistort_surface():
        reg.cloud_undistort_fe_device(fe, B, 1, acc, out, 0)

    def undistort_none():
        reg.cloud_undistort_fe_device(fe, B, 1, none, out, 0)

    def undistort_features():
        n = reg.cloud_undistort_fe_device(fe, B, 0, acc, out, 0)
        reg.cloud_undistort_fe_device(fe, B, 1, acc, out, n)

    def transform_features():
        n = reg.append_to_submap_device(fe, B, 0, acc, pc, out, 0)
        reg.append_to_submap_device(fe, B, 1, acc, pc, out, n)

    def host_round_trip():
        k = len(feats)
        clouds = []
        for b in range(k):
            g = fe.get_features(scan=b)
            for c in (g["pc_corners"], g["pc_surface"]):
                clouds.append(numpy_undistort(c, it, b, pc[b], p.minimum_pt_time_stamp, p.maximum_pt_time_stamp))
        torch.from_numpy(np.concatenate(clouds)).cuda()
        torch.cuda.synchronize()

    variants = {"undistort_fe_device_full": undistort_full, "undistort_fe_device_surface": undistort_surface,
                "undistort_fe_device_none_accepted": undistort_none,
                "undistort_fe_device_features": undistort_features, "transform_fe_device_features": transform_features,
                "host_round_trip_8_slots": host_round_trip}
    t = {k: [] for k in variants}
    order = list(variants)
    for r in range(a.reps + 2):
        for name in (order if r % 2 == 0 else order[::-1]):
            torch.cuda.synchronize()
            c0 = time.perf_counter()
            variants[name]()
            if r >= 2:
                t[name].append(time.perf_counter() - c0)
    sub = median_ms(t)
    sub["host_round_trip_scaled_to_batch"] = sub["host_round_trip_8_slots"] * B / len(feats)
    result["submap_ms"] = sub
    # the kernel alone.  From a kernel trace when one is given; the difference of two host-clock medians is kept beside it as a rough
    # cross-check only: each call holds two stream synchronisations and a blocking read-back, whose jitter is of the kernel's own size
    moved = 32 * int(ns.sum())   # the surface selections: 16 bytes in, 16 out per point
    result["kernel"] = {"bytes": moved, "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE, "trace": "not measured",
                        "host_clock_difference_ms": sub["undistort_fe_device_surface"] - sub["undistort_fe_device_none_accepted"]}
    if a.kernel_stats_plain:
        row = kernel_stats_row(a.kernel_stats_plain, "cloud_undistort_kernel")
        ms = float(row["AverageNs"]) * 1e-6
        result["kernel"]["trace_plain_branch"] = {"source": "the same launches after a registration with if_motion_deblur = 0: no sin / cos", "launches": int(row["Calls"]),
                                                  "average_ms": ms, "min_ms": float(row["MinNs"]) * 1e-6, "bytes_per_s": moved / (ms * 1e-3),
                                                  "share_of_hbm": moved / (ms * 1e-3) / HBM_ACHIEVABLE}
    if a.kernel_stats:
        row = kernel_stats_row(a.kernel_stats, "cloud_undistort_kernel")
        ms = float(row["AverageNs"]) * 1e-6
        result["kernel"]["trace"] = {"source": "rocprofv3 --kernel-trace --stats of `--trace-only` (surface selections of the batch, one launch each)",
                                     "launches": int(row["Calls"]), "average_ms": ms, "min_ms": float(row["MinNs"]) * 1e-6,
                                     "bytes_per_s": moved / (ms * 1e-3), "share_of_hbm": moved / (ms * 1e-3) / HBM_ACHIEVABLE}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
