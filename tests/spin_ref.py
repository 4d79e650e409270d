"""ctypes binding of tests/spin_ref.c: the TEST-ONLY host restatement of the spinning-lidar feature extraction
(hku-mars/loam_livox source/laser_feature_extractor.hpp:393-787), plus the per-line VoxelGrid of :769-776 through the
oracle's PCL 1.9 VoxelGrid.  Built on first use with the host C compiler into tests/ (git-ignored)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
_SRC = os.path.join(_HERE, "spin_ref.c")
_LIB = os.path.join(_HERE, "libspinref.so")
MAX_POINTS = 400000
TOPICS = ("/laser_points_2", "/laser_cloud_sharp", "/laser_cloud_less_sharp", "/laser_cloud_flat", "/laser_cloud_less_flat")

_lib = None


def build() -> str:
    if not os.path.exists(_LIB) or os.path.getmtime(_SRC) > os.path.getmtime(_LIB):
        tmp = _LIB + f".{os.getpid()}.tmp"
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-shared", "-ffp-contract=off", "-o", tmp, _SRC, "-lm"])
        os.replace(tmp, _LIB)
    return _LIB


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.spin_ref.restype = C.c_int
        L.spin_ref.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double] + [C.c_void_p] * 15
        _lib = L
    return _lib


class SpinRefError(ValueError):
    pass


def _p(a):
    return a.ctypes.data if a is not None else None


def extract(xyzi, scan_line: int = 16, minimum_range: float = 0.1, plane_resolution: float = 0.8, voxel: bool = True) -> dict:
    """One message.  Returns full (n,4) float32, full_src, line_n, sharp / less_sharp / flat / less_flat_pre (positions in
    full), lf_line_n, curvature, picked0 and -- with voxel -- less_flat (the per-line VoxelGrid output, concatenated)."""
    pts = np.ascontiguousarray(xyzi, np.float32).reshape(-1, 4)
    n_in = pts.shape[0]
    cap = max(n_in, 1)
    full = np.zeros((cap, 4), np.float32)
    ints = {k: np.zeros(cap, np.int32) for k in ("full_src", "sharp", "less_sharp", "flat", "less_flat_pre", "picked0")}
    curv = np.zeros(cap, np.float32)
    line_n = np.zeros(64, np.int32)
    lf_line_n = np.zeros(64, np.int32)
    cnt = [C.c_int(0) for _ in range(5)]
    rc = lib().spin_ref(_p(pts), n_in, 4, int(scan_line), float(minimum_range), _p(full), _p(ints["full_src"]), C.byref(cnt[0]),
                        _p(line_n), _p(ints["sharp"]), C.byref(cnt[1]), _p(ints["less_sharp"]), C.byref(cnt[2]), _p(ints["flat"]),
                        C.byref(cnt[3]), _p(ints["less_flat_pre"]), _p(lf_line_n), C.byref(cnt[4]), _p(curv), _p(ints["picked0"]))
    if rc == -1:
        raise SpinRefError("only support velodyne with 16 or 64 scan line!")
    if rc == -2:
        raise SpinRefError(f"more than {MAX_POINTS} points")
    n = cnt[0].value
    out = {"full": full[:n].copy(), "full_src": ints["full_src"][:n].copy(), "line_n": line_n[:scan_line].copy(),
           "sharp": ints["sharp"][:cnt[1].value].copy(), "less_sharp": ints["less_sharp"][:cnt[2].value].copy(),
           "flat": ints["flat"][:cnt[3].value].copy(), "less_flat_pre": ints["less_flat_pre"][:cnt[4].value].copy(),
           "lf_line_n": lf_line_n[:scan_line].copy(), "curvature": curv[:n].copy(), "picked0": ints["picked0"][:n].copy()}
    if voxel:
        from oracle import orc
        leaf = np.float32(plane_resolution) / np.float32(2)  # m_plane_resolution / 2 in float (:192)
        parts, o = [], 0
        for c in out["lf_line_n"]:
            seg = out["full"][out["less_flat_pre"][o:o + c]]
            o += c
            if c:
                parts.append(orc.voxel_grid(seg, leaf)[1])
        out["less_flat"] = np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)
    return out


def clouds(r: dict) -> dict:
    """the five published clouds keyed by topic (:782-812)"""
    f = r["full"]
    return {TOPICS[0]: f, TOPICS[1]: f[r["sharp"]], TOPICS[2]: f[r["less_sharp"]], TOPICS[3]: f[r["flat"]], TOPICS[4]: r["less_flat"]}
