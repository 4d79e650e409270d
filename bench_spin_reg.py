#!/usr/bin/env python3
"""Spinning-lidar scans from the extractor into the registrar on one MI355X: the device hand-off (ll_reg_enqueue_spin,
ll_reg_enqueue_spin_downsampled) against the host round trip it replaces.  Prints one JSON line.

  vlp16  B = 256 VLP-16 scans (1800 azimuths x 16 beams), resident in HBM;
  hdl64  B = 64 HDL-64-like scans (2000 azimuths x 64 beams).
Both register against a synthetic map of bench.py's size (synth.make_maps(5 000 000)), 10 ICP iterations (all of them run), from initial
poses up to 5 cm / 0.01 rad off.  A timed step is extract + resolve + register + collect of one batch, a host clock around work that
ends in ll_reg_collect's synchronisation.  Three routes run in the same process on the same inputs, one step of each in turn, so that
they share the machine's noise:

  round_trip          what the library offered before the hand-off: per scan ll_spin_cloud of the less-sharp and the less-flat
                      cloud, then ll_reg_upload_features + ll_reg_enqueue_uploaded.  This is the baseline: existing code;
  device              ll_reg_enqueue_spin;
  device_downsampled  ll_reg_enqueue_spin_downsampled with leaf 0.1 / 0.4 (less work per scan: not comparable with the other two).

scans_per_s = B / median step: an end-to-end rate of the whole step, not any kernel's share of peak.  pack_kernel_ms: the hand-off's
one new kernel, from HIP events on the extractor's stream (last device step).  parity: the last batch of `device` against the last
batch of `round_trip`, and `device_downsampled` against VoxelGrid.filter_batch + upload -- poses, increments, results and every report
field must have the same bits (mismatch = slots with any difference)."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")  # as bench.py: before the first HIP call
MAP_POINTS = 5_000_000
LINE_RES, PLANE_RES = 0.1, 0.4
ROUTES = ("round_trip", "device", "device_downsampled")
_world = None


def _init_worker(map_points):
    global _world
    from loam_livox_amd import synth
    _world = synth.world_for_map_size(map_points)


def _make_scan(args):
    from loam_livox_amd import synth
    k, scan_line, n_azimuth = args
    s = synth.make_spin_scan(_world, k, scan_line=scan_line, n_azimuth=n_azimuth)
    return s.xyzi, s.pose_true


def report_tuple(rep):
    return tuple(getattr(rep, name) for name, _ in type(rep)._fields_)


def mismatches(a, b, B):
    return sum(0 if (a[0][s] == b[0][s] and a[1][s].tobytes() == b[1][s].tobytes() and a[2][s].tobytes() == b[2][s].tobytes()
                     and report_tuple(a[3][s]) == report_tuple(b[3][s])) else 1 for s in range(B))


def make_scans(pool, scan_line, B, n_azimuth, seed0):
    t0 = time.time()
    made = list(pool.map(_make_scan, [(seed0 + k, scan_line, n_azimuth) for k in range(B)]))
    return made, time.time() - t0


def run_config(made, synth_s, dev_map, scan_line, B, steps, warmup):
    from loam_livox_amd import capi, synth
    from loam_livox_amd.api import Point_cloud_registration, Spinning_laser, VoxelGrid
    scans = [m[0] for m in made]
    rng = np.random.default_rng(31000 + scan_line)
    inits = np.stack([synth.pose_compose(m[1], np.r_[synth.quat_from_axis_angle(rng.normal(size=3), rng.uniform(0.0, 0.01)),
                                                      rng.uniform(-0.05, 0.05, 3)]) for m in made])
    cap = max(len(s) for s in scans)
    spin = Spinning_laser(scan_line=scan_line, max_points=cap, max_scans=B, max_line_points=4096)
    spin.upload(scans)
    reg = Point_cloud_registration(max_scans=B, max_features=cap)
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = 10, 20, 1
    p.para_max_angular_rate, p.para_max_speed = 20.0, 0.3
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    vc, vs = VoxelGrid(cap, B), VoxelGrid(cap, B)
    L = spin.L
    cap_c = min(cap, 1200 * scan_line)
    cbuf, sbuf = np.zeros((B, cap_c, 4), np.float32), np.zeros((B, cap, 4), np.float32)
    nc, ns = np.zeros(B, np.int32), np.zeros(B, np.int32)
    n1 = C.c_int32(0)
    F4 = 16

    def step(route):
        t = time.perf_counter()
        capi.check(L.ll_spin_extract_batch(spin.h, B), "ll_spin_extract_batch")
        capi.check(L.ll_spin_resolve(spin.h), "ll_spin_resolve")
        if route == "round_trip":
            for b in range(B):
                capi.check(L.ll_spin_cloud(spin.h, b, Spinning_laser.LESS_SHARP, C.c_void_p(cbuf.ctypes.data + b * cap_c * F4), None, C.byref(n1)), "ll_spin_cloud")
                nc[b] = n1.value
                capi.check(L.ll_spin_cloud(spin.h, b, Spinning_laser.LESS_FLAT, C.c_void_p(sbuf.ctypes.data + b * cap * F4), None, C.byref(n1)), "ll_spin_cloud")
                ns[b] = n1.value
            capi.check(L.ll_reg_upload_features(reg.h, B, capi.ptr(cbuf), capi.ptr(nc), cap_c, capi.ptr(sbuf), capi.ptr(ns), cap), "ll_reg_upload_features")
            reg.enqueue_uploaded(dev_map, B, inits, inits)
        elif route == "device":
            reg.enqueue_spin(dev_map, spin, B, inits, inits)
        else:
            reg.enqueue_spin_downsampled(dev_map, spin, vc, vs, LINE_RES, PLANE_RES, B, inits, inits)
        out = reg.collect(B)
        return time.perf_counter() - t, out

    times = {r: [] for r in ROUTES}
    last = {}
    pack_ms = []
    for it in range(warmup + steps):  # every route (every shape that is timed) is warmed up; one step of each in turn
        for r in ROUTES:
            dt, out = step(r)
            if it >= warmup:
                times[r].append(dt)
                if r == "device":
                    pack_ms.append(spin.handoff_time())
            last[r] = out
    counts, status = spin.counts(B)
    res = {"B": B, "points_in": int(sum(len(s) for s in scans)), "steps": steps, "warmup": warmup,
           "features_per_scan": {"less_sharp": float(counts[:, 2].mean()), "less_flat": float(counts[:, 4].mean()),
                                 "less_sharp_max": int(counts[:, 2].max()), "less_flat_max": int(counts[:, 4].max())},
           "status_nonzero": int(np.count_nonzero(status)), "synth_s": round(synth_s, 1)}
    for r in ROUTES:
        t = np.array(times[r])
        res[r] = {"scans_per_s": B / float(np.median(t)), "step_ms_median": float(np.median(t)) * 1e3, "step_ms_min": float(t.min()) * 1e3,
                  "step_ms_p90": float(np.percentile(t, 90)) * 1e3, "timed_window_s": float(t.sum()),
                  "accepted": int(np.sum(last[r][0]))}
    res["device_over_round_trip_scans_per_s"] = res["device"]["scans_per_s"] / res["round_trip"]["scans_per_s"]
    res["pack_kernel_ms"] = {"median": float(np.median(pack_ms)), "max": float(np.max(pack_ms)), "source": "HIP events on the extractor's stream"}
    # parity of the last batch (the same extraction outputs: nothing was uploaded in between)
    hv = (VoxelGrid(cap, B), VoxelGrid(cap, B))
    hv[0].setLeafSize(LINE_RES, LINE_RES, LINE_RES)
    hv[1].setLeafSize(PLANE_RES, PLANE_RES, PLANE_RES)
    oc, onc, _ = hv[0].filter_batch(cbuf, nc)
    os_, ons, _ = hv[1].filter_batch(sbuf, ns)
    reg.upload_features([oc[b, :onc[b]] for b in range(B)], [os_[b, :ons[b]] for b in range(B)])
    reg.enqueue_uploaded(dev_map, B, inits, inits)
    ds_rt = reg.collect(B)
    res["parity"] = {"slots": B, "device_vs_round_trip_mismatch": mismatches(last["device"], last["round_trip"], B),
                     "device_downsampled_vs_filter_upload_mismatch": mismatches(last["device_downsampled"], ds_rt, B)}
    for h in (spin, reg, vc, vs) + hv:
        h.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--map-points", type=int, default=MAP_POINTS)
    ap.add_argument("--only", default="", help="vlp16 or hdl64")
    ap.add_argument("--workers", type=int, default=16, help="host processes that ray-cast the synthetic scans")
    a = ap.parse_args()
    # the scans are ray-cast by worker processes that never touch the GPU; they are gone before this process's first HIP call
    configs = [c for c in (("vlp16", 16, 256, 1800, 7000), ("hdl64", 64, 64, 2000, 7300)) if a.only in ("", c[0])]
    with ProcessPoolExecutor(a.workers, initializer=_init_worker, initargs=(a.map_points,)) as pool:
        made = {c[0]: make_scans(pool, c[1], c[2], c[3], c[4]) for c in configs}
    from loam_livox_amd import synth
    from loam_livox_amd.api import Map_buffer
    _, corner, surf = synth.make_maps(a.map_points)
    dev_map = Map_buffer()
    dev_map.setInputCloud(Map_buffer.CORNER, corner)
    dev_map.setInputCloud(Map_buffer.SURF, surf)
    res = {"bench": "spin_reg", "device": "MI355X (gfx950)", "map_points": int(len(corner) + len(surf)), "icp_iterations": 10,
           "timed_step": "ll_spin_extract_batch + ll_spin_resolve + route + ll_reg_collect", "baseline": "round_trip (existing entry points)"}
    for name, scan_line, B, _, _ in configs:
        res[name] = run_config(made[name][0], made[name][1], dev_map, scan_line, B, a.steps, a.warmup)
    head = "vlp16" if "vlp16" in res else "hdl64"
    res["metric"] = f"scans_per_s_{head}_device_handoff"
    res["value"] = res[head]["device"]["scans_per_s"]
    res["parity"] = {k: sum(res[c]["parity"][k] for c in ("vlp16", "hdl64") if c in res)
                     for k in ("device_vs_round_trip_mismatch", "device_downsampled_vs_filter_upload_mismatch")}
    dev_map.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
