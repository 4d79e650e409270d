"""Builds and runs tests/pose_graph_host.cpp: loam_livox_amd/csrc/ll_pose_graph_core.h -- the text the kernel runs -- under g++."""
import os
import subprocess

import numpy as np

from tests import pose_graph_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "pose_graph_host.cpp")])
    return exe


def pack(graphs):
    """graphs: [dict(poses, ab, meas, information)] -> (pose_offsets, poses [P, 7], edge_offsets, ab [E, 2], meas [E, 7], information [E, 36] or None)"""
    po = np.cumsum([0] + [len(g["poses"]) for g in graphs]).astype(np.int64)
    eo = np.cumsum([0] + [len(g["ab"]) for g in graphs]).astype(np.int64)
    poses = np.concatenate([np.asarray(g["poses"], np.float64).reshape(-1, 7) for g in graphs]) if graphs else np.zeros((0, 7))
    ab = np.concatenate([np.asarray(g["ab"], np.int32).reshape(-1, 2) for g in graphs]) if graphs else np.zeros((0, 2), np.int32)
    meas = np.concatenate([np.asarray(g["meas"], np.float64).reshape(-1, 7) for g in graphs]) if graphs else np.zeros((0, 7))
    info = None
    if any(g.get("information") is not None for g in graphs):
        info = np.concatenate([np.asarray(g["information"], np.float64).reshape(-1, 36) if g.get("information") is not None
                               else np.tile(np.eye(6).ravel(), (len(g["ab"]), 1)) for g in graphs])
    return po, np.ascontiguousarray(poses), eo, np.ascontiguousarray(ab), np.ascontiguousarray(meas), info


PARAM_INTS = ("max_num_iterations", "max_num_consecutive_invalid_steps")
PARAM_DOUBLES = ("initial_trust_region_radius", "max_trust_region_radius", "min_trust_region_radius", "min_relative_decrease", "min_lm_diagonal",
                 "max_lm_diagonal", "function_tolerance", "gradient_tolerance", "parameter_tolerance")


def all_options(options):
    """pose_graph_ref.OPTIONS with `options` over them: the numbers the reference, the driver and the device are all given"""
    unknown = set(options or {}) - set(ref.OPTIONS)
    assert not unknown, unknown
    return dict(ref.OPTIONS, **(options or {}))


def params_block(options):
    """the driver's params block: the two ints as int64, the nine doubles, in ll_pose_graph_params' order"""
    o = all_options(options)
    return np.array([o[k] for k in PARAM_INTS], np.int64).tobytes() + np.array([o[k] for k in PARAM_DOUBLES], np.float64).tobytes()


def params_struct(options):
    """the same dict as a capi.PoseGraphParams (what api.Pose_graph( params=... ) takes)"""
    from loam_livox_amd import capi
    o = all_options(options)
    assert [k for k, _ in capi.PoseGraphParams._fields_] == list(PARAM_INTS + PARAM_DOUBLES)
    p = capi.PoseGraphParams()
    for k in PARAM_INTS:
        setattr(p, k, int(o[k]))
    for k in PARAM_DOUBLES:
        setattr(p, k, float(o[k]))
    return p


def run_driver(exe, tmp, graphs, mode=0, expect_refusal=False, options=None):
    """mode 0: (poses per graph, summaries); mode 1: the first linearisation of one graph; mode 2: envelope blocks per graph and of
    the call, as the plan counts them.  options: a dict keyed like pose_graph_ref.OPTIONS, or None for the driver's defaults."""
    po, poses, eo, ab, meas, info = pack(graphs)
    pin, pout = os.path.join(tmp, "pg_in.bin"), os.path.join(tmp, "pg_out.bin")
    with open(pin, "wb") as f:
        f.write(np.array([mode, len(graphs), len(poses), len(ab), 0 if info is None else 1, 0 if options is None else 1], np.int64).tobytes())
        if options is not None:
            f.write(params_block(options))
        f.write(po.tobytes() + eo.tobytes() + poses.tobytes() + ab.tobytes() + meas.tobytes())
        if info is not None:
            f.write(np.ascontiguousarray(info).tobytes())
    done = subprocess.run([exe, pin, pout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if expect_refusal:
        assert done.returncode == 3 and not done.stderr, (done.returncode, done.stderr.decode(errors="replace"))
        return done.stdout.decode().strip()
    assert done.returncode == 0 and not done.stderr, (done.returncode, done.stdout.decode(errors="replace"), done.stderr.decode(errors="replace"))
    raw = np.fromfile(pout, np.float64)
    if mode == 0:
        P, G = len(poses), len(graphs)
        out = raw[:7 * P].reshape(P, 7)
        rec = raw[7 * P:].reshape(G, 6)
        summaries = [dict(iterations=int(r[0]), successful_steps=int(r[1]), unsuccessful_steps=int(r[2]), termination=int(r[3]),
                          initial_cost=r[4], final_cost=r[5]) for r in rec]
        return [out[po[g]:po[g + 1]] for g in range(G)], summaries
    if mode == 2:
        return [int(b) for b in raw[:len(graphs)]], int(raw[len(graphs)])
    E = len(ab)
    J = raw[:72 * E].reshape(E, 2, 6, 6)
    n = int(raw[72 * E])
    rest = raw[72 * E + 1:]
    return dict(J=J, A=rest[:n * n].reshape(n, n), rhs=rest[n * n:n * n + n], y=rest[n * n + n:n * n + 2 * n], ok=bool(rest[n * n + 2 * n]))
