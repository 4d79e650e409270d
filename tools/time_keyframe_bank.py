#!/usr/bin/env python3
"""Times the two routes by which the loop detector compares a new key frame with N stored ones (service_loop_detection's walk,
laser_mapping.hpp:988-1057), on one device in one process:

  pairwise  2 N api.keyframe_similarity calls (plane image, then line image, per stored key frame), as Keyframe_assembly makes them by
            default: per call an allocation, two uploads, one workgroup, a download, a free;
  bank      ONE api.Keyframe_bank.match of the new key frame against the N stored ones, as Keyframe_assembly( device_bank=True ) makes it.

The images are random and positive (a uniform draw to the eighth power: mostly small, a few bins large, as a blurred direction histogram
is); the bank holds the N stored entries and the new one before anything is timed.  Both routes are warmed up, then timed alternately
with a device synchronise inside every timed region; medians and ranges are reported, the two routes' floats must be equal bit for bit
in every repetition, and one JSON record per N is written.  --match-only N runs nothing but the adds and one match of N pairs: the
process a kernel trace is taken of.  Needs a HIP device: there is no fall-back."""
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


def images(n: int, seed: int = 5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (n, 2, 60, 60)).astype(np.float32) ** 8


def filled_bank(n_stored: int):
    """(bank, images [n_stored + 1, 2, 60, 60]): entries 0 .. n_stored - 1 are the stored key frames, entry n_stored is the new one"""
    from loam_livox_amd.api import Keyframe_bank
    img = images(n_stored + 1)
    bank = Keyframe_bank(initial_entries=n_stored + 1)
    for e in range(n_stored + 1):
        assert bank.add_images(img[e, 0], img[e, 1]) == e
    return bank, img


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--stored", type=int, nargs="+", default=[1, 200, 1000], help="stored key frames N, one record each")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "keyframe_bank.json"))
    ap.add_argument("--match-only", type=int, default=0, metavar="N", help="the adds and ONE match of N pairs, nothing else (for a kernel trace)")
    args = ap.parse_args()
    if args.reps < 11:
        ap.error("at least 11 repetitions")

    from loam_livox_amd.api import keyframe_similarity
    from tools.build_id import build_id
    hip = ctypes.CDLL("libamdhip64.so")
    n_dev = ctypes.c_int(0)
    if hip.hipGetDeviceCount(ctypes.byref(n_dev)) != 0 or n_dev.value < 1:
        sys.exit("no HIP device")

    def sync():
        if hip.hipDeviceSynchronize() != 0:
            sys.exit("hipDeviceSynchronize failed")

    if args.match_only:
        n = args.match_only
        bank, _ = filled_bank(n)
        line, plane = bank.match([n] * n, list(range(n)))
        sync()
        print(json.dumps(dict(match_only=n, work=bank.work().tolist(), sim_line_0=float(line[0]), sim_plane_0=float(plane[0]), build=build_id())))
        bank.close()
        return

    records = []
    for n in args.stored:
        bank, img = filled_bank(n)
        ids_a, ids_b = [n] * n, list(range(n))

        def pairwise_route():
            plane = np.array([keyframe_similarity(img[n, 1], img[h, 1]) for h in range(n)], np.float32)   # (the walk asks plane, line per key frame;
            line = np.array([keyframe_similarity(img[n, 0], img[h, 0]) for h in range(n)], np.float32)    #  the order does not change the work)
            sync()
            return line, plane

        def bank_route():
            out = bank.match(ids_a, ids_b)
            sync()
            return out

        t_pair, t_bank = [], []
        for rep in range(args.warmup + args.reps):
            got = {}
            for name, route, into in (("pairwise", pairwise_route, t_pair), ("bank", bank_route, t_bank)):   # alternating: the same neighbours on the machine
                sync()
                t0 = time.perf_counter()
                got[name] = route()
                dt = time.perf_counter() - t0
                if rep >= args.warmup:
                    into.append(dt)
            for k in range(2):
                assert got["pairwise"][k].tobytes() == got["bank"][k].tobytes(), f"the two routes differ (N = {n}, repetition {rep})"
        work = bank.work().tolist()
        med_pair, med_bank = statistics.median(t_pair), statistics.median(t_bank)
        rec = dict(what="one new key frame against N stored ones: 2 N keyframe_similarity calls against one Keyframe_bank.match",
                   stored=n, pairs=n, build=build_id(), reps=args.reps, warmup=args.warmup, bank_work=work,
                   pairwise_median_ms=1e3 * med_pair, bank_median_ms=1e3 * med_bank,
                   pairwise_min_max_ms=[1e3 * min(t_pair), 1e3 * max(t_pair)], bank_min_max_ms=[1e3 * min(t_bank), 1e3 * max(t_bank)],
                   pairwise_over_bank=med_pair / med_bank, routes_bit_equal=True)
        if n == 1:
            # the condition at N = 1: the bank's median is not above the pairwise median by more than the pairwise route's own range
            rec["n1_condition_holds"] = bool(med_bank <= med_pair + (max(t_pair) - min(t_pair)))
        records.append(rec)
        bank.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(records, f, indent=1)
        f.write("\n")
    for rec in records:
        print(json.dumps(rec))


if __name__ == "__main__":
    main()
