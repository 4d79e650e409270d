"""Times the lock-step mapping loop with motion deblur and deskewed maps and writes profiles/deblur_batch.json (DESIGN "Deskewed
clouds", lock-step loop).

  python tools/time_deblur_batch.py [--sequences 1 8 64] [--frames 100] [--reps 3] [--out profiles/deblur_batch.json]

For every S: S sequences of 12 000-point scans (four distinct synthetic trajectories, reused with start stamps of their own), through
  alone          S Laser_mapping(if_motion_deblur=1, if_undistort=1) run back to back
  histories      Laser_mapping_batch(S, if_motion_deblur=1, if_undistort=1): a History_buffer per sequence, the refresh pool
  history_batch  the same with batched_history=True: one add and one refresh per step
alternating inside a repetition, after one warm-up pass of every variant at the smallest S.  Figures: the median over the repetitions
of frames per second (S x frames over the wall time of the loop's calls) and of the add and the refresh per step in milliseconds
(the loops' own stage clocks, summed over the sequences), and the frames the registrations accepted -- the add and the refresh run
for those only.  No GPU: the script fails (there is no other path)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P, DT, DISTINCT = 12000, 1e-5, 4
ARGS = dict(scan_points=P, maximum_history_size=20, init_accumulate_frames=5, if_motion_deblur=1, if_undistort=1)


def run_alone(mapping, seqs, S, frames):
    t_loop, add, ref, ok = 0.0, 0.0, 0.0, 0
    for s in range(S):
        lm = mapping.Laser_mapping(**ARGS)
        scans = seqs[s % DISTINCT]
        t0 = time.perf_counter()
        for k in range(frames):
            ok += int(lm.process_new_scan(scans[k], 1.0 + 0.37 * s + k * P * DT))
        t_loop += time.perf_counter() - t0
        add, ref = add + lm.stage_s[1], ref + lm.stage_s[2]
        lm.close()
    return t_loop, add / frames, ref / frames, ok   # (per step of all S sequences, to compare with the lock-step loop's step)


def run_batch(mapping, seqs, S, frames, batched_history):
    lb = mapping.Laser_mapping_batch(S, batched_history=batched_history, **ARGS)
    t0, ok = time.perf_counter(), 0
    for k in range(frames):
        ok += int((lb.process_new_scans([seqs[s % DISTINCT][k] for s in range(S)], [1.0 + 0.37 * s + k * P * DT for s in range(S)]) == 1).sum())
    t_loop = time.perf_counter() - t0
    # stage_s[1] / [2] are summed over the sequences (and over the pool's threads): per step, as run_alone reports them
    out = t_loop, lb.stage_s[1] / frames, lb.stage_s[2] / frames, ok
    lb.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deblur_batch.json"))
    a = ap.parse_args()
    from loam_livox_amd import mapping, synth
    world, _, _ = synth.make_maps(40_000)
    seqs = [synth.make_livox_sequence(world, 77 + i, n_frames=a.frames, n_static=3, n_points=P)[0] for i in range(DISTINCT)]
    variants = {"alone": lambda S: run_alone(mapping, seqs, S, a.frames), "histories": lambda S: run_batch(mapping, seqs, S, a.frames, False),
                "history_batch": lambda S: run_batch(mapping, seqs, S, a.frames, True)}
    for fn in variants.values():   # warm-up: every kernel and every allocation path once
        fn(min(a.sequences))
    rows = []
    for S in a.sequences:
        samples = {name: [] for name in variants}
        for _ in range(a.reps):
            for name, fn in variants.items():
                samples[name].append(fn(S))
        row = {"sequences": S, "frames": a.frames, "repetitions": a.reps}
        for name, v in samples.items():
            row[name] = {"frames_per_s": statistics.median(S * a.frames / v_[0] for v_ in v),
                         "add_ms_per_step": 1e3 * statistics.median(v_[1] for v_ in v),
                         "refresh_ms_per_step": 1e3 * statistics.median(v_[2] for v_ in v),
                         "accepted_frames": sorted(set(v_[3] for v_ in v)),   # (of S x frames; the add and the refresh run for these only)
                         "loop_s": [round(v_[0], 4) for v_ in v]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/time_deblur_batch.py", "scan_points": P, "distinct_trajectories": DISTINCT, "arguments": {k: v for k, v in ARGS.items()},
                   "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
