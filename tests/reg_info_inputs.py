"""Inputs, driver and yardstick of the registration-information tests (tests/test_reg_information_host.py, tests/test_gpu_reg_information.py).

The driver is tests/reg_info_host.cpp: loam_livox_amd/csrc/ll_reg_info_core.h -- the text reg_information_kernel runs -- under g++.
The yardstick is the oracle: orc.make_block_line / make_block_plane from the same neighbour points, summed by orc.blocks_eval at the same
evaluation point, with the bound

    |v - v_orc| <= (1e-13 + n 2^-53) A        per entry of H, g and for the cost,

A = the sum over the blocks of that entry's absolute per-block contribution (blocks_eval on each block alone); 1e-13 is the project's
per-block agreement between its accumulate forms (tests/test_hostcheck.py), n 2^-53 the bound of summing n terms in another order."""
import os
import subprocess

import numpy as np

from loam_livox_amd import synth
from oracle import orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLK_LINE, BLK_PLANE, BLK_ACTIVE, BLK_AVAIL = 1, 2, 4, 8


def build_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", *extra, "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "reg_info_host.cpp")])
    return exe


def _run(exe, tmp, header, payload):
    pin, pout = os.path.join(tmp, "ri_in.bin"), os.path.join(tmp, "ri_out.bin")
    with open(pin, "wb") as f:
        f.write(np.array(header, np.int64).tobytes() + payload)
    done = subprocess.run([exe, pin, pout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stdout.decode(errors="replace"), done.stderr.decode(errors="replace"))
    return np.fromfile(pout, np.float64)


def run_info(exe, tmp, case, gated=0, aborted=0, icp_iters=1):
    """the driver on one scan -> dict(H, g, cost, n_line, n_plane, status)"""
    cap = case["cap_c"] + case["cap_s"]
    flag0 = np.zeros((cap + 7) // 8 * 8, np.uint8)
    flag0[:cap] = case["flag0"]
    head = [0, case["deblur"], case["n_corner"], case["n_surf"], case["cap_c"], case["cap_s"], len(case["map_c"]), len(case["map_s"]), 0,
            gated, aborted, icp_iters]
    d = np.r_[case["pose_last"], case["x"], case["huber_a"], case["min_ts"], case["max_ts"]].astype(np.float64)
    payload = (d.tobytes() + flag0.tobytes() + np.ascontiguousarray(case["nn"], np.int32).tobytes() +
               np.ascontiguousarray(case["corner"], np.float32).tobytes() + np.ascontiguousarray(case["surf"], np.float32).tobytes() +
               np.ascontiguousarray(case["map_c"], np.float32).tobytes() + np.ascontiguousarray(case["map_s"], np.float32).tobytes())
    raw = _run(exe, tmp, head, payload)
    assert raw.shape == (46,)
    return dict(H=raw[:36].reshape(6, 6), g=raw[36:42], cost=float(raw[42]), n_line=int(raw[43]), n_plane=int(raw[44]), status=int(raw[45]))


def run_eigen(exe, tmp, mats):
    """the adapter's symmetric_eigen6 on matrices [n, 6, 6] -> (w [n, 6], V [n, 6, 6] with the vectors in columns, sweeps [n])"""
    mats = np.ascontiguousarray(mats, np.float64).reshape(-1, 36)
    raw = _run(exe, tmp, [1, 0, 0, 0, 0, 0, 0, 0, len(mats), 0, 0, 0], mats.tobytes()).reshape(len(mats), 43)
    return raw[:, :6], raw[:, 6:42].reshape(-1, 6, 6), raw[:, 42].astype(int)


def run_pose_frame(exe, tmp, mats, poses):
    """the adapter's information_in_pose_frame -> [n, 6, 6]"""
    rows = np.concatenate([np.asarray(mats, np.float64).reshape(-1, 36), np.asarray(poses, np.float64).reshape(-1, 7)], axis=1)
    return _run(exe, tmp, [2, 0, 0, 0, 0, 0, 0, 0, len(rows), 0, 0, 0], np.ascontiguousarray(rows).tobytes()).reshape(-1, 6, 6)


def refine_blur(stamp, min_ts, max_ts):
    """point_cloud_registration.hpp:128-141 with if_motion_deblur = 1, in float arithmetic"""
    with np.errstate(all="ignore"):
        res = (np.float32(stamp) - np.float32(min_ts)) / (np.float32(max_ts) - np.float32(min_ts))
    return 1.0 if (not np.isfinite(res) or res > np.float32(1.0)) else float(res)


def make_case(seed, n_line, n_plane, deblur=0, inactive=False, wall=False):
    """One scan as the registrar leaves it in HBM after its last ICP iteration: feature clouds, map points, neighbour positions and
    pristine flags -- and the same blocks for the oracle, in candidate order.  inactive: candidates that must not enter are mixed in
    (non-finite features, candidates without five neighbours, a degenerate triple, a degenerate line).  wall: every map point has z == 0
    exactly and pose_last turns about z only.

    Conditioning.  A residual is a difference of coordinates, |r| out of |p|: the oracle forms it in the map frame
    (R_last (R_inc f + t_inc) + t_last - a), the device in the frame of pose_last, and each rounds it by a few eps |p| / |r| -- an error of
    the QUANTITY, which the bound's 1e-13 (the agreement of the accumulate forms' arithmetic) does not cover and which a single block
    cannot average out.  So the blocks here are built with their residual's size chosen, 0.05 .. 0.099 m (inside the Huber radius) or
    0.2 .. 0.5 m (every fourth, outside), and coordinates within ~1.2 m: |p| / |r| <= 25, a share below 3e-14."""
    rng = np.random.default_rng(seed)
    if wall:
        pose_last = np.r_[synth.quat_from_axis_angle(np.array([0.0, 0.0, 1.0]), 0.4), 1.5, -0.7, 1.2]
    else:
        pose_last = np.r_[synth.quat_from_axis_angle(rng.normal(size=3), 0.5), rng.uniform(-0.3, 0.3, 3)]
    x = np.r_[synth.quat_from_axis_angle(rng.normal(size=3), 0.02), rng.uniform(-0.05, 0.05, 3)]
    Rl, Ri = synth.quat_to_mat(pose_last[:4]), synth.quat_to_mat(x[:4])
    min_ts, max_ts = 0.25, 1.0
    feats, maps, nns, flags = ([], []), ([], []), ([], []), ([], [])
    blocks = []

    def add(kind, f, pts, flag, found=1, block=True):
        base = len(maps[kind])
        maps[kind].extend(pts)
        idx = [base + k for k in range(len(pts))] + [0x7fffffff] * (3 - len(pts))
        nns[kind].append(idx + [found])
        feats[kind].append(f)
        flags[kind].append(flag)
        if block:
            s = refine_blur(f[3], min_ts, max_ts) if deblur else 1.0
            p = [np.asarray(q[:3], np.float64) for q in pts]
            fd = np.asarray(f[:3], np.float64)
            blocks.append(orc.make_block_plane(fd, p[0], p[1], p[2], s) if kind else orc.make_block_line(fd, p[0], p[1], s))

    def point(v):
        return np.r_[np.asarray(v, np.float64), 0.0].astype(np.float32)

    def feature():
        f = np.r_[rng.uniform(-0.5, 0.5, 3), rng.uniform(0.0, 1.1)].astype(np.float32)  # stamp: some below min_ts, some above max_ts
        pw = Rl @ (Ri @ f[:3].astype(np.float64) + x[4:]) + pose_last[4:]
        return f, pw

    for kind, n in ((0, n_line), (1, n_plane)):
        for i in range(n):
            f, pw = feature()
            if wall:
                a = np.r_[pw[:2] + rng.normal(0, 0.3, 2), 0.0]
                pts = [point(a), point(a + np.r_[rng.uniform(0.5, 1.5), rng.uniform(-0.3, 0.3), 0.0]), point(a + np.r_[rng.uniform(-0.3, 0.3), rng.uniform(0.5, 1.5), 0.0])]
            else:
                d1, e = rng.normal(size=3), rng.normal(size=3)
                d1 /= np.linalg.norm(d1)
                e -= d1 * (d1 @ e)
                e /= np.linalg.norm(e)                       # the residual's direction: across the line / the plane's normal
                d2 = np.cross(e, d1) + 0.3 * d1              # (the plane's second direction: |ab^ x ac^| ~ 0.96)
                rho = rng.uniform(0.2, 0.5) if i % 4 == 3 else rng.uniform(0.05, 0.099)  # every fourth beyond the Huber radius
                a = pw - rho * e + rng.uniform(-0.2, 0.2) * d1
                pts = [point(a), point(a + d1 * rng.uniform(0.3, 0.6))]
                if kind:
                    pts.append(point(a + d2 * rng.uniform(0.3, 0.6)))
            add(kind, f, pts, (BLK_PLANE if kind else BLK_LINE) | BLK_ACTIVE | BLK_AVAIL)
            if inactive and i % 5 == 2:
                bad = np.array([np.nan, 1.0, np.inf, 0.5], np.float32)
                add(kind, bad, [], 0, found=0, block=False)                                # a non-finite feature: no search, no block
                add(kind, feature()[0], [], 0, found=0, block=False)                       # fewer than five neighbours in range
                p = point(pw)
                if kind:
                    add(1, f, [p, p.copy(), point(pw + 1.0)], BLK_PLANE | BLK_ACTIVE | BLK_AVAIL, block=False)   # degenerate triple (a == b)
                    add(1, feature()[0], [p, point(pw + 0.5), point(pw - 0.5)], BLK_AVAIL, block=False)          # counted available, not active
                else:
                    add(0, f, [p, point(pw + np.r_[5e-5, 0, 0])], BLK_LINE | BLK_ACTIVE | BLK_AVAIL, block=False)  # |a - b| < 1e-4 (PCR:302)
    nC, nS = len(feats[0]), len(feats[1])
    cap_c, cap_s = nC + 3, nS + 5
    flag0 = np.zeros(cap_c + cap_s, np.uint8)
    nn = np.full((cap_c + cap_s, 4), 0x7fffffff, np.int32)  # (slots beyond the scan: never read)
    nn[:, 3] = 1
    flag0[cap_c - 3:cap_c] = BLK_LINE | BLK_ACTIVE
    flag0[cap_c + nS:] = BLK_PLANE | BLK_ACTIVE
    if nC:
        flag0[:nC], nn[:nC] = flags[0], np.array(nns[0], np.int64).astype(np.int32)
    if nS:
        flag0[cap_c:cap_c + nS], nn[cap_c:cap_c + nS] = flags[1], np.array(nns[1], np.int64).astype(np.int32)
    arr = lambda v: np.array(v, np.float32).reshape(-1, 4)
    return dict(deblur=int(deblur), n_corner=nC, n_surf=nS, cap_c=cap_c, cap_s=cap_s, flag0=flag0, nn=nn, corner=arr(feats[0]), surf=arr(feats[1]),
                map_c=arr(maps[0]), map_s=arr(maps[1]), pose_last=pose_last, x=x, huber_a=0.1, min_ts=min_ts, max_ts=max_ts, blocks=blocks,
                n_line=n_line, n_plane=n_plane)


def oracle_record(blocks, pose_last, x, deblur=0, huber_a=0.1):
    """(cost, g, H) of the blocks by orc.blocks_eval, and the sums of the absolute per-block contributions (A_cost, A_g, A_H)"""
    if not blocks:
        return dict(cost=0.0, g=np.zeros(6), H=np.zeros((6, 6)), A_cost=0.0, A_g=np.zeros(6), A_H=np.zeros((6, 6)), n=0)
    cost, g, H = orc.blocks_eval(blocks, pose_last, x, deblur=deblur, huber_a=huber_a)
    A_cost, A_g, A_H = 0.0, np.zeros(6), np.zeros((6, 6))
    for b in blocks:
        c1, g1, H1 = orc.blocks_eval([b], pose_last, x, deblur=deblur, huber_a=huber_a)
        A_cost += abs(c1)
        A_g += np.abs(g1)
        A_H += np.abs(H1)
    return dict(cost=cost, g=g, H=H, A_cost=A_cost, A_g=A_g, A_H=A_H, n=len(blocks))


def worst_ratio(rec, orc_rec, rows=None):
    """the largest |v - v_orc| / ((1e-13 + n 2^-53) A) over H, g and the cost: the bound holds when this is <= 1
    (rows: only these rows and columns of H and entries of g)"""
    k = 1e-13 + orc_rec["n"] * 2.0 ** -53
    worst = 0.0
    sel = (lambda m: m) if rows is None else (lambda m: np.asarray(m)[np.ix_(rows, rows)] if np.ndim(m) == 2 else np.asarray(m)[rows])
    for got, want, A in ((sel(rec["H"]), sel(orc_rec["H"]), sel(orc_rec["A_H"])), (sel(rec["g"]), sel(orc_rec["g"]), sel(orc_rec["A_g"])),
                         (np.array([rec["cost"]]), np.array([orc_rec["cost"]]), np.array([orc_rec["A_cost"]]))):
        err, lim = np.abs(np.asarray(got) - np.asarray(want)).ravel(), (k * np.asarray(A)).ravel()
        for e, l in zip(err, lim):
            if e == 0.0:
                continue
            worst = max(worst, np.inf if l == 0.0 else e / l)
    return worst
