"""What the deskew tests share (tests/test_undistort_host.py, tests/test_gpu_undistort.py): a float64 numpy restatement of
point_cloud_registration.hpp:622-661 (pointAssociateToMap with if_undistore = 1) and :607-620 (compute_interpolatation_rodrigue), and the
rule the device's floats are held to against it.  The restatement itself is held to the reference's compiled class under the same rule
(tests/test_ref_undistort.py, tests/test_ref_undistort_golden.py).

The rule.  Both sides round a double to float.  The doubles differ by a few fp64 ulps (other sin / cos / atan2 implementations, a rotation
matrix here against Eigen's v + w uv + q x uv there), so the floats are equal unless the double lies within ~1e-15 relative of a rounding
boundary: expected about 1e-7 of the coordinates (2^-52 * a few / 2^-24 ulp spacing), and then they are neighbours.  Hence: every coordinate
within one fp32 ulp, at most 1 coordinate in 10 000 unequal."""
import numpy as np


def quat_to_mat(q):
    x, y, z, w = (float(v) for v in q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quat_from_rotvec(v):
    v = np.asarray(v, np.float64)
    a = np.linalg.norm(v)
    if a == 0.0:
        return np.array([0.0, 0.0, 0.0, 1.0])
    return np.r_[np.sin(a / 2) * v / a, np.cos(a / 2)]


def interp(q):
    """PCR:607-620: Eigen::AngleAxisd( q ) -> (theta, hat [3, 3]); hat_sq is hat @ hat"""
    q = np.asarray(q, np.float64)
    n = float(np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]))
    if n != 0.0:
        theta = 2.0 * np.arctan2(n, abs(q[3]))   # AngleAxis::operator=( QuaternionBase ): the angle first ...
        axis = q[:3] / (-n if q[3] < 0 else n)   # ... then n = -n for w < 0
    else:
        theta, axis = 0.0, np.array([1.0, 0.0, 0.0])
    axis = axis / np.linalg.norm(axis)
    hat = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return float(theta), hat


def blur_ratio(w, deblur, min_ts, max_ts):
    """refine_blur, PCR:128-141, in float arithmetic"""
    w = np.asarray(w, np.float32)
    if not deblur:
        return np.ones(w.shape, np.float32)
    with np.errstate(all="ignore"):
        res = (w - np.float32(min_ts)) / (np.float32(max_ts) - np.float32(min_ts))
    return np.where(~np.isfinite(res) | (res > np.float32(1.0)), np.float32(1.0), res).astype(np.float32)


def plain(pose, xyzi):
    """PCR:627-630: q p + t, as doubles"""
    p = np.asarray(xyzi, np.float32)[:, :3].astype(np.float64)
    pose = np.asarray(pose, np.float64)
    return p @ quat_to_mat(pose[:4]).T + pose[4:]


def undistort(xyzi, pose_last, pose_curr, pose_incre, theta, hat, deblur, min_ts, max_ts):
    """PCR:622-661 -> [n, 3] doubles (the caller rounds)"""
    xyzi = np.asarray(xyzi, np.float32).reshape(-1, 4)
    pose_last, pose_curr, pose_incre = (np.asarray(a, np.float64) for a in (pose_last, pose_curr, pose_incre))
    hat = np.asarray(hat, np.float64).reshape(3, 3)
    s = blur_ratio(xyzi[:, 3], deblur, min_ts, max_ts).astype(np.float64)
    out = plain(pose_curr, xyzi)
    mid = s != 1.0
    if deblur and mid.any():
        p = xyzi[mid, :3].astype(np.float64)
        sm = s[mid]
        R = np.eye(3)[None] + np.sin(sm * theta)[:, None, None] * hat[None] + (1.0 - np.cos(sm * theta))[:, None, None] * (hat @ hat)[None]  # :641-644
        inner = np.einsum("nij,nj->ni", R, p) + sm[:, None] * pose_incre[4:][None]                                                      # :645
        out[mid] = inner @ quat_to_mat(pose_last[:4]).T + pose_last[4:]                                                                  # :646
    return out


def check_rule(got, want64, what=""):
    """got: float32 [n, 3]; want64: the restatement's doubles.  Prints the count of unequal coordinates, then asserts the rule."""
    got = np.asarray(got, np.float32)
    want = np.asarray(want64, np.float64).astype(np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    if got.size == 0:
        return 0
    assert np.isfinite(got).all() and np.isfinite(want).all()
    unequal = got != want
    ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
    worst = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp))
    n_bad = int(unequal.sum())
    print(f"{what}: {n_bad} of {got.size} coordinates unequal, worst distance {worst:.3g} fp32 ulp")
    assert worst <= 1.0
    assert n_bad <= got.size // 10000
    return n_bad
