#!/usr/bin/env python3
"""BASELINE config C4 on ONE GPU: S independent sub-sequences with local map growth, three ways in one process.

  one_by_one   S loam_livox_amd.mapping.Laser_mapping loops back to back, each with the prefetch of the next scan (bench_c4.py's loop):
               one scan per launch, what the sequential path offers;
  lockstep     loam_livox_amd.mapping.Laser_mapping_batch: frame k of all S sequences is one batch -- one batched extraction, one
               VoxelGrid pair, one registration with a map per slot (ll_reg_enqueue_fe_downsampled_maps) -- then S history adds and
               match-buffer refreshes on a small pool of host threads;
  lockstep_batched  the same loop with batched_history=True: the histories of all S sequences in one History_buffer_batch, one add and
               one refresh per step whose launches and host waits do not grow with S.

The sequences are bench_c4.py's with the sequence index where it has the rank (start-pose seed 9000 + s, scan seeds 7000 + 1000 s + k,
turn sign by parity), under its args_map without cell maps on both routes.  The routes alternate after all are warm; every timed loop
ends in a device synchronise.  Prints one JSON line per S: aggregate frames/s of the routes (best and all repeats), their ratios, the
host time per phase and the number of sequences whose poses differ in any bit between the routes (must be 0; for lockstep_batched:
from either other route).

--cell-maps measures what C4 hands over at its end, the two cell maps of every sequence: one_by_one runs Laser_mapping(keep_cell_maps=True),
lockstep_batched runs Laser_mapping_batch(batched_history=True, cell_maps=True), both with their sync() inside the timed region, and
lockstep_batched_plain is lockstep_batched without cell maps from the same call.  The line then also reports the number of
(sequence, kind) cell-map dumps that differ in any bit between the two routes that keep them (must be 0).

--cell-matching measures the cell ("cube") matching mode: one_by_one runs S Laser_mapping(matching_mode=1) loops, lockstep_batched runs
Laser_mapping_batch(batched_history=True, cell_maps=True, cell_matching=True); both register every frame against the cells of their
own map around the current pose (--fov, --search-range).  The line also reports the wall time of the refresh phase per step (for
one_by_one: summed over the S sequences) and the number of sequences whose poses differ in any bit (must be 0).

--full-maps [--key-frames] measures the map a user of offline map building receives, the un-filtered full cloud of every accepted scan
(m_pt_cell_map_full), and with --key-frames the key frames and the loop detector on top of it: one_by_one runs S
Laser_mapping(loop_closure_if_enable=1) loops (without --key-frames their key-frame length lies beyond the run), lockstep_batched runs
Laser_mapping_batch(batched_history=True, full_maps=True[, key_frames=True]).  Both routes read every sequence's full map once, at the
end, inside the timed region.  The line reports frames/s of both, the wall time of the full-map phase per step (for one_by_one: summed
over the S sequences), the number of sequences whose full-map dumps differ in any bit and, with --key-frames, whose key-frame states,
images or detector logs differ (both must be 0).

  python bench_c4_batch.py [--sequences 1,8,64] [--frames 200] [--distinct-frames 100] [--out profiles/bench_c4_batch.json]
  python bench_c4_batch.py --cell-maps --sequences 1,8,64 --out profiles/bench_c4_batch_cell_maps.json
  python bench_c4_batch.py --cell-matching --sequences 1,8,64 --out profiles/bench_c4_batch_cell_matching.json
  python bench_c4_batch.py --full-maps [--key-frames] --sequences 1,8,64 --frames 100 --out profiles/bench_c4_batch_full_maps.json
  python bench_c4_batch.py --routes lockstep_batched --sequences 8 --frames 12 --repeats 1   # one route alone, e.g. under a kernel trace"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")  # (bench_c4.py: every handle has a stream of its own)


def make_sequence(job):
    """bench_c4.py's generator for sequence s (there: rank): D distinct scans of an out-and-back trajectory of period 50"""
    s, n_scans, n_points = job
    from loam_livox_amd import synth
    world = synth.world_for_map_size(200_000)
    rng = np.random.default_rng(9000 + s)
    start = synth.sensor_pose_in_world(world, rng)
    sgn = 1.0 if s % 2 == 0 else -1.0
    step = np.r_[synth.quat_from_axis_angle(np.array([0.1, 0.2, 1.0]), np.deg2rad(0.2 * sgn)), np.array([-0.02, 0.01 * sgn, 0.0])]
    back = synth.pose_inverse(step)
    ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    scans, cur = [], start
    for k in range(n_scans):
        if k >= 3:
            cur = synth.pose_compose(cur, step if ((k - 3) // 25) % 2 == 0 else back)
        scans.append(synth.make_moving_scan(world, 7000 + 1000 * s + k, n_points, inc_true=ident, pose_start=cur, t_phase=0.13 * k).xyzi)
    return scans


def frame_scan(scans, k, D):
    """frame k of a sequence that replays D distinct scans (the trajectory has period 50 from frame 3 on)"""
    while k >= D + 3:
        k -= D
    return scans[k]


def keyframes_digest(kf):
    """everything the two routes must agree on about one sequence's key frames: the lists, every processed key frame's cell set, images
    and ratios, the detector's log and its loops"""
    def flat(rec):
        return [(k, np.asarray(rec[k]).tobytes()) for k in sorted(rec)]
    return [kf.state(), [(sorted(k.m_set_cell), k.m_ending_frame_idx, [(n, np.asarray(k.analysis[n]).tobytes()) for n in sorted(k.analysis)])
                         for k in kf.keyframe_vec], [flat(r) for r in kf.log], [flat(r) for r in kf.loops]]


def full_maps_line(args, S, seqs, routes, args_map):
    """--full-maps: one JSON line for S sequences"""
    import torch
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    F, D, N = args.frames, args.distinct_frames, args.scan_points
    kf_scans = args.keyframe_scans if args.key_frames else F + 1000
    closure = dict(scans_of_each_keyframe=kf_scans, scans_between_two_keyframe=max(1, kf_scans // 3), minimum_keyframe_differen=2,
                   map_alignment_maximum_icp_iteration=2, max_points=1 << 19)

    def dump_of(cell_map):
        return b"".join(np.ascontiguousarray(a).tobytes() for a in cell_map.dump())

    def one_by_one(frames):
        lms = [Laser_mapping(scan_points=N, loop_closure_if_enable=1, loop_closure=closure, **args_map) for _ in range(S)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses, dumps, accepted = [], [], 0
        for s, lm in enumerate(lms):
            ps = []
            for k in range(frames):
                nxt = frame_scan(seqs[s], k + 1, D) if k + 1 < frames else None
                accepted += lm.process_new_scan(frame_scan(seqs[s], k, D), next_xyzi=nxt)
                ps.append(lm.pose.copy())
            poses.append(np.stack(ps))
            dumps.append(dump_of(lm.keyframes.m_pt_cell_map_full))  # (the map is read once, at the end: inside the timed region)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = dict(dt=dt, poses=poses, accepted=accepted, dumps=dumps, full_s=sum(lm.full_map_s for lm in lms),
                   keyframes=[keyframes_digest(lm.keyframes) for lm in lms] if args.key_frames else None,
                   n_keyframes=sum(len(lm.keyframes.keyframe_vec) for lm in lms))
        for lm in lms:
            lm.close()
        return out

    def lockstep_batched(frames):
        lb = Laser_mapping_batch(S, scan_points=N, batched_history=True, full_maps=True, key_frames=args.key_frames, loop_closure=closure, **args_map)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        poses, accepted = [[] for _ in range(S)], 0
        for k in range(frames):
            out = lb.process_new_scans([frame_scan(seqs[s], k, D) for s in range(S)])
            accepted += int((out == 1).sum())
            for s in range(S):
                poses[s].append(lb.poses[s].copy())
        dumps = [dump_of(lb.full_map(s)) for s in range(S)]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = dict(dt=dt, poses=[np.stack(p) for p in poses], accepted=accepted, dumps=dumps, full_s=lb.full_map_s,
                   keyframes=[keyframes_digest(k) for k in lb.keyframes] if args.key_frames else None,
                   n_keyframes=sum(len(k.keyframe_vec) for k in lb.keyframes) if args.key_frames else 0,
                   work=lb.history_batch.full_map_work().tolist(), stored_points=sum(lb.full_map(s).stats()[1] for s in range(S)))
        lb.close()
        return out

    run = {"one_by_one": one_by_one, "lockstep_batched": lockstep_batched}
    assert set(routes) <= set(run), "--full-maps: routes one_by_one and lockstep_batched"
    for r in routes:
        run[r](min(6, F))  # warm-up
    times, last = {r: [] for r in routes}, {}
    for _ in range(args.repeats):
        for r in routes:
            last[r] = run[r](F)
            times[r].append(last[r]["dt"])
    n = S * F
    line = {"metric": "frames_per_s", "sequences": S, "frames_per_sequence": F, "scan_points": N, "full_maps": True, "key_frames": bool(args.key_frames)}
    for r in routes:
        line[r] = {"frames_per_s": round(n / min(times[r]), 1), "all_repeats": [round(n / t, 1) for t in times[r]], "accepted": last[r]["accepted"],
                   "full_map_phase_ms_per_step": round(1e3 * last[r]["full_s"] / F, 4), "key_frames_processed": last[r]["n_keyframes"]}
    if "lockstep_batched" in routes:
        b = last["lockstep_batched"]
        line["full_map_work_last_append"] = b["work"]
        line["full_map_points_stored"] = int(b["stored_points"])
        line["full_map_dump_bytes"] = sum(len(x) for x in b["dumps"])
    if len(routes) == 2:
        a, b = last["one_by_one"], last["lockstep_batched"]
        line["lockstep_batched_over_one_by_one"] = round(min(times["one_by_one"]) / min(times["lockstep_batched"]), 3)
        line["sequences_with_differing_poses"] = sum(0 if np.array_equal(a["poses"][s].view(np.uint64), b["poses"][s].view(np.uint64)) else 1 for s in range(S))
        line["sequences_with_differing_full_map_dumps"] = sum(a["dumps"][s] != b["dumps"][s] for s in range(S))
        if args.key_frames:
            line["sequences_with_differing_key_frames"] = sum(a["keyframes"][s] != b["keyframes"][s] for s in range(S))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", default="1,8,64")
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--distinct-frames", type=int, default=100, help="distinct scans per sequence (a multiple of 50, at least 100), replayed")
    ap.add_argument("--scan-points", type=int, default=24000)
    ap.add_argument("--history", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--refresh-threads", type=int, default=0, help="0 = Laser_mapping_batch's default")
    ap.add_argument("--workers", type=int, default=8, help="processes that generate the synthetic scans")
    ap.add_argument("--routes", default="one_by_one,lockstep,lockstep_batched", help="the routes to run (all three for the JSON line of record)")
    ap.add_argument("--cell-maps", action="store_true", help="keep every sequence's two cell maps: one_by_one, lockstep_batched and lockstep_batched_plain")
    ap.add_argument("--cell-map-points", type=int, default=1 << 19, help="with --cell-maps: cell_map_max_points of both routes (the maps grow from it)")
    ap.add_argument("--cell-matching", action="store_true", help="the cell matching mode: one_by_one (matching_mode=1) and lockstep_batched (cell_matching=True)")
    ap.add_argument("--fov", type=float, default=30.0, help="with --cell-matching: maximum_in_fov_angle")
    ap.add_argument("--search-range", type=float, default=100.0, help="with --cell-matching: maximum_search_range_corner and _surface")
    ap.add_argument("--full-maps", action="store_true", help="keep every sequence's full-cloud map: one_by_one (loop_closure_if_enable=1) and lockstep_batched")
    ap.add_argument("--key-frames", action="store_true", help="with --full-maps: the key frames and the loop detector on top of the full maps")
    ap.add_argument("--keyframe-scans", type=int, default=30, help="with --key-frames: scans_of_each_keyframe (a new key frame opens every third of it)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert not (args.cell_maps and args.cell_matching), "--cell-maps and --cell-matching are separate measurements"
    assert not (args.full_maps and (args.cell_maps or args.cell_matching)), "--full-maps is a measurement of its own"
    assert args.full_maps or not args.key_frames, "--key-frames needs --full-maps"
    S_list = [int(x) for x in args.sequences.split(",")]
    routes = args.routes.split(",")
    if args.cell_maps:  # (the threaded lockstep route keeps no cell maps; the plain batched loop joins the line of record)
        routes = [r for r in routes if r != "lockstep"] + (["lockstep_batched_plain"] if "lockstep_batched" in routes and "one_by_one" in routes else [])
    if args.cell_matching:  # (the threaded lockstep route has no cell mode; the plain batched loop would not match against cells)
        assert "lockstep_batched_plain" not in routes, "--cell-matching: routes one_by_one and lockstep_batched"
        routes = [r for r in routes if r != "lockstep"]
    if args.full_maps:  # (the threaded lockstep route keeps no full maps)
        routes = [r for r in routes if r != "lockstep"]
    assert routes and set(routes) <= {"one_by_one", "lockstep", "lockstep_batched", "lockstep_batched_plain"}, "--routes: one_by_one, lockstep, lockstep_batched"
    F, D, N = args.frames, args.distinct_frames, args.scan_points
    assert D >= F or (D % 50 == 0 and D >= 100), "--distinct-frames must be a multiple of 50 and at least 100"
    n_gen = min(F, D + 3)
    # the scans first, in worker processes started before this process touches the device
    from concurrent.futures import ProcessPoolExecutor
    jobs = [(s, n_gen, N) for s in range(max(S_list))]
    if args.workers > 1 and len(jobs) > 1:
        with ProcessPoolExecutor(max_workers=min(args.workers, 16, len(jobs))) as ex:
            seqs = list(ex.map(make_sequence, jobs))
    else:
        seqs = [make_sequence(j) for j in jobs]

    import torch
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    args_map = dict(maximum_history_size=args.history, init_accumulate_frames=2, line_res=0.1, plane_res=0.15, icp_max_iterations=10,
                    ceres_max_iterations=20, max_allow_incre_R=20.0, max_allow_incre_T=0.3, minimum_icp_R_diff=1e-3, minimum_icp_T_diff=1e-4)
    cell_mode = dict(maximum_search_range_corner=args.search_range, maximum_search_range_surface=args.search_range, maximum_in_fov_angle=args.fov,
                     cell_map_max_points=args.cell_map_points) if args.cell_matching else {}
    lines = []
    for S in S_list if args.full_maps else []:
        line = full_maps_line(args, S, seqs, routes, args_map)
        print(json.dumps(line), flush=True)
        lines.append(line)
    for S in [] if args.full_maps else S_list:
        def dumps_of(cell_map):
            """both dumps of one sequence as bytes"""
            return [b"".join(np.ascontiguousarray(a).tobytes() for a in cell_map(kind).dump()) for kind in (0, 1)]

        def one_by_one(frames):
            if args.cell_matching:
                lms = [Laser_mapping(scan_points=N, matching_mode=1, **cell_mode, **args_map) for _ in range(S)]
            else:
                lms = [Laser_mapping(scan_points=N, keep_cell_maps=args.cell_maps, cell_map_max_points=args.cell_map_points, **args_map) for _ in range(S)]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            poses, accepted = [], 0
            for s, lm in enumerate(lms):
                ps = []
                for k in range(frames):
                    nxt = frame_scan(seqs[s], k + 1, D) if k + 1 < frames else None
                    accepted += lm.process_new_scan(frame_scan(seqs[s], k, D), next_xyzi=nxt)
                    ps.append(lm.pose.copy())
                poses.append(np.stack(ps))
                lm.sync()  # (every frame is in the cell maps: inside the timed region)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            stage = np.sum([lm.stage_s for lm in lms], axis=0)
            dumps = [dumps_of(lm.history.cell_map) for lm in lms] if args.cell_maps else None
            for lm in lms:
                lm.close()
            return dt, poses, accepted, stage, None, dumps, [tuple(lm.map_sizes) for lm in lms]

        def lockstep(frames, batched_history=False, cell_maps=False, cell_matching=False):
            kw = dict(refresh_threads=args.refresh_threads) if args.refresh_threads else {}
            if batched_history:
                kw["batched_history"] = True
            if cell_matching:
                kw.update(cell_maps=True, cell_matching=True, **cell_mode)
            if cell_maps:
                kw.update(cell_maps=True, cell_map_max_points=args.cell_map_points)
            lb = Laser_mapping_batch(S, scan_points=N, **kw, **args_map)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            poses, accepted = [[] for _ in range(S)], 0
            for k in range(frames):
                out = lb.process_new_scans([frame_scan(seqs[s], k, D) for s in range(S)])
                accepted += int((out == 1).sum())
                for s in range(S):
                    poses[s].append(lb.poses[s].copy())
            if cell_maps:
                lb.sync()  # (the stores are in order, ready to be handed over: inside the timed region)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            stage, threads, sizes = lb.stage_s.copy(), lb.refresh_threads, [tuple(x) for x in lb.map_sizes]
            dumps = [dumps_of(lambda kind, s=s: lb.cell_map(s, kind)) for s in range(S)] if cell_maps else None
            lb.close()
            return dt, [np.stack(p) for p in poses], accepted, stage, threads, dumps, sizes

        run = {"one_by_one": one_by_one, "lockstep": lockstep, "lockstep_batched": lambda frames: lockstep(frames, True, args.cell_maps, args.cell_matching),
               "lockstep_batched_plain": lambda frames: lockstep(frames, True)}
        for r in routes:
            run[r](min(6, F))  # warm-up: code objects load lazily, the ICP kernels first run on frame 3
        times, last = {r: [] for r in routes}, {}
        for _ in range(args.repeats):
            for r in routes:
                last[r] = run[r](F)
                times[r].append(last[r][0])
        n = S * F

        def differing(x, y):
            return sum(0 if np.array_equal(last[x][1][s].view(np.uint64), last[y][1][s].view(np.uint64)) else 1 for s in range(S))

        def rate(r):
            return {"frames_per_s": round(n / min(times[r]), 1), "all_repeats": [round(n / t, 1) for t in times[r]], "accepted": last[r][2]}

        def wall(st):
            return {"extract_register": round(1e3 * float(st[0]) / F, 4), "history_add_and_refresh": round(1e3 * float(st[4]) / F, 4)}

        line = {"metric": "frames_per_s", "sequences": S, "frames_per_sequence": F, "scan_points": N, "cell_maps": bool(args.cell_maps)}
        if args.cell_matching:
            line.update(cell_matching=True, maximum_in_fov_angle=args.fov, maximum_search_range=args.search_range)
            if "one_by_one" in routes:
                line["refresh_ms_per_step_one_by_one"] = round(1e3 * float(last["one_by_one"][3][2]) / F, 4)
                line["match_buffer_points_last_frame_one_by_one"] = [int(x) for x in np.sum(last["one_by_one"][6], axis=0)]
            if "lockstep_batched" in routes:
                line["refresh_ms_per_step_lockstep_batched"] = round(1e3 * float(last["lockstep_batched"][3][2]) / F, 4)
                line["match_buffer_points_last_frame"] = [int(x) for x in np.sum(last["lockstep_batched"][6], axis=0)]
        if "one_by_one" in routes:
            line["one_by_one"] = dict(rate("one_by_one"), ms_per_frame_by_stage=dict(zip(("extract_register", "history_add", "match_buffer_refresh"),
                                                                                       [round(1e3 * float(v) / n, 4) for v in last["one_by_one"][3][:3]])))
        if "lockstep" in routes:
            st = last["lockstep"][3]
            line["lockstep"] = dict(rate("lockstep"), refresh_threads=last["lockstep"][4], ms_per_step_wall=wall(st),
                                    ms_per_frame_thread_time={"history_add": round(1e3 * float(st[1]) / n, 4), "match_buffer_refresh": round(1e3 * float(st[2]) / n, 4)})
        if "one_by_one" in routes and "lockstep" in routes:
            line["lockstep_over_one_by_one"] = round(min(times["one_by_one"]) / min(times["lockstep"]), 3)
            line["sequences_with_differing_poses"] = differing("one_by_one", "lockstep")
        if "lockstep_batched" in routes:
            st = last["lockstep_batched"][3]
            line["lockstep_batched"] = dict(rate("lockstep_batched"), ms_per_step_wall=wall(st),
                                            ms_per_step_by_stage={"history_add": round(1e3 * float(st[1]) / F, 4), "match_buffer_refresh": round(1e3 * float(st[2]) / F, 4)})
            if "lockstep" in routes:
                line["lockstep_batched_over_lockstep"] = round(min(times["lockstep"]) / min(times["lockstep_batched"]), 3)
            if "one_by_one" in routes:
                line["lockstep_batched_over_one_by_one"] = round(min(times["one_by_one"]) / min(times["lockstep_batched"]), 3)
            if "lockstep_batched_plain" in routes:  # the same loop without cell maps, from the same call
                line["lockstep_batched_plain"] = rate("lockstep_batched_plain")
                line["cell_maps_time_factor_lockstep_batched"] = round(min(times["lockstep_batched"]) / min(times["lockstep_batched_plain"]), 3)
            if args.cell_maps and "one_by_one" in routes:
                a, b = last["one_by_one"][5], last["lockstep_batched"][5]
                line["cell_map_dumps_differing"] = sum(a[s][kind] != b[s][kind] for s in range(S) for kind in (0, 1))
                line["cell_map_dumps_compared"] = 2 * S
                line["cell_map_dump_bytes"] = sum(len(x) for d in b for x in d)
            others = [r for r in ("one_by_one", "lockstep", "lockstep_batched_plain") if r in routes]
            if others:  # sequences whose poses differ in any bit from EITHER other route
                line["lockstep_batched_sequences_with_differing_poses"] = sum(
                    1 if any(not np.array_equal(last["lockstep_batched"][1][s].view(np.uint64), last[r][1][s].view(np.uint64)) for r in others) else 0
                    for s in range(S))
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
