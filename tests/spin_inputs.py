"""Deterministic inputs that drive the spinning-lidar extraction (ll_spin_kernels.hip, tests/spin_ref.c) through its data-dependent
changes of form -- the LDS / rank sort switch at 4096 entries, the 20 / 200 pick bounds of the sharp pass, its 64-candidate chunks,
the 64-step ballots of the +-500 walks, walks across a line boundary, lines past the one-workgroup VoxelGrid -- and the helpers
that read, from the restatement's outputs, what an input reaches.  tests/test_spin_host.py asserts those figures on the CPU, so
that the device tests built on the same scans cannot be hollowed out by a later edit.

Geometry: a VLP-16 point of line l sits at elevation -15 + 2 l degrees (+0.02, off the scan-ID boundaries); the orientation
-atan2(y, x) grows with the azimuth.  A line of 11 + 6 m points has six sub-regions of exactly m points; 3 more points give
sub-regions alternating m and m + 1.  Every scan is in-domain: no NaN, nothing inside minimum_range."""
import numpy as np

WALK = 500          # steps of a sharp walk (5 * times, laser_feature_extractor.hpp:679)
GAP2 = 0.05         # squared gap that stops a walk
SHARP_CURV = 0.5    # sharp_point_threshold * 10
LADDER = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049, 4095, 4096, 4097, 5000)


def elevation(line, offset=0.02):
    return -15.0 + 2.0 * line + offset


def polar(r, az, el_deg):
    """horizontal range, azimuth, elevation (degrees) -> (n, 4) float32, intensity 1"""
    r, az = np.asarray(r, np.float64), np.asarray(az, np.float64)
    el = np.deg2rad(np.broadcast_to(np.asarray(el_deg, np.float64), r.shape))
    return np.stack([r * np.cos(az), -r * np.sin(az), r * np.tan(el), np.ones_like(r)], 1).astype(np.float32)


def line_points(m, extra=0):
    return 11 + 6 * m + extra


# ------------------------------------------------------------------------------------------------------ the families
def spiked_ring(m=4096, extra=3, line=6, radius=10.0, period=9, spike=0.8, noise=0.0, seed=0, az0=0.0, az1=2 * np.pi * 0.999):
    """One line, radius + spike at every period-th point.  noise: range noise as a random outward drift, increments uniform in
    [0, noise] -- it breaks the curvature ties; zero-mean noise would let the backward-occlusion rule (depth1 > depth2 wherever the
    curvature is above 0.1, which is everywhere here) pre-mark nearly every candidate."""
    n = line_points(m, extra)
    r = np.full(n, radius)
    if noise > 0:
        r += np.cumsum(np.random.default_rng(seed).uniform(0.0, noise, n))
    r[period::period] += spike
    return polar(r, np.linspace(az0, az1, n, endpoint=False), elevation(line))


def ladder(noise=0.0, seed=1, sizes=LADDER):
    """one scan, one spiked line per sub-region length of `sizes` (lines 0, 1, ...), the lines one after the other round one turn"""
    n = np.array([line_points(m) for m in sizes])
    edge = np.r_[0, np.cumsum(n)] / n.sum() * 2 * np.pi * 0.999
    return np.concatenate([spiked_ring(m, 0, line, noise=noise, seed=seed + line, az0=edge[line], az1=edge[line + 1])
                           for line, m in enumerate(sizes)])


def zigzag_line(m, line=6, r0=100.0, growth=0.05, az0=0.0, az_step=1e-4, jitter=0.0, seed=0, extra=0):
    """horizontal range r0 + growth * i, elevation alternating -+0.2 degrees round the line's (jitter: +- that many degrees more):
    every neighbour is more than the walk gap away, the depth grows monotonically (no backward occlusion mark)"""
    n = line_points(m, extra)
    i = np.arange(n)
    el = elevation(line, 0.0) + np.where(i % 2 == 0, -0.2, 0.2)
    if jitter > 0:
        el = el + np.random.default_rng(seed).uniform(-jitter, jitter, n)
    return polar(r0 + growth * i, az0 + az_step * i, el)


def zigzag(ms=(199, 200, 201), jitter=0.0, seed=3, first_line=6):
    """one zig-zag line per entry of ms on consecutive lines"""
    out, az0 = [], 0.0
    for k, m in enumerate(ms):
        out.append(zigzag_line(m, first_line + k, az0=az0, jitter=jitter, seed=seed + k))
        az0 += 1e-4 * len(out[-1])
    return np.concatenate(out)


def level(n, radius, drift=2e-5):
    """a ring that drifts outward by `drift` a point: many float ulps, so that depth1 > depth2 of the backward-occlusion rule is never
    decided by the rounding of two equal depths; a linear drift adds no curvature"""
    return radius + drift * np.arange(n)


def kink(r, a, c, rise=5):
    """A sharp candidate no rule pre-marks, at any range: the ring is level up to position a and rises by c metres a point over the
    next `rise` points, then stays out.  Curvature (15 c)^2 at a; the depth never falls (no backward occlusion mark), the gap behind
    a is an azimuth step (no parallel-beam mark of a), and gaps of c < 0.22 m stop no walk.  With c > 0.0142 r the parallel-beam rule
    pre-marks the points of the ramp itself, so a is the only candidate of the kink."""
    r[a + 1:a + 1 + rise] += c * np.arange(1, rise + 1)
    r[a + 1 + rise:] += c * rise


WALK_M = 2000                    # sub-region length of the long-walk line
WALK_A = 5 + WALK_M * 2 + 1000   # the walker: in sub-region 2, 1000 points from either of its ends, so its probes share the sub-region


def long_walks(case):
    """A level ring of 11 + 6 * 2000 points at 2 m with kinks.  The walker at WALK_A (0.2 m a point, curvature 9) is the first pick of
    its sub-region and walks 500 steps either way.  Probes are kinks of 0.06 m a point (curvature 0.81): picked if and only if no
    walk reached them.
      'limit'  probes at a - 500 and a + 500: reached by the last step of the eighth ballot round, not picked
      'past'   probes at a - 501 and a + 501: not reached, picked -- the walks are exactly 500 steps long
      'cut'    the ring steps by 0.45 m (a gap, curvature 5 next to it) between a + 499 and a + 500 and between a - 500 and a - 499:
               both walks stop after 499 steps, and the candidates beyond the gaps are picked
      'ends'   walkers 99 points from either end of the cloud: their walks stop at the first / the last point after 99 steps"""
    n = line_points(WALK_M)
    r = level(n, 2.0)
    az = np.linspace(0.0, 2 * np.pi * 0.999, n, endpoint=False)
    a = WALK_A
    if case == "ends":
        kink(r, 99, 0.1)
        kink(r, n - 100, 0.1)
    elif case in ("limit", "past"):
        d = WALK if case == "limit" else WALK + 1
        kink(r, a - d, 0.06)
        kink(r, a, 0.2)
        kink(r, a + d, 0.06)
    elif case == "cut":
        r[a - WALK + 1:] += 0.45
        kink(r, a, 0.2)
        r[a + WALK:] += 0.45
    else:
        raise ValueError(case)
    return polar(r, az, elevation(6))


BOUNDARY_M = 100


def line_boundary(far=False):
    """Two adjacent lines: line 7 starts at the azimuth where line 6 ends, 0.05 m above it.  The walker (a kink 20 points before the
    end of line 6) walks across the boundary over a probe kink 10 points into line 7, which is then not picked; with `far` line 7
    lies 1 m further out, the gap at the boundary stops the walk and the probe is picked.  Returns (scan, walker, probe)."""
    n = line_points(BOUNDARY_M)
    walker, probe = n - 20, n + 10
    r6 = level(n, 1.0)
    kink(r6, walker, 0.1)
    r7 = level(n, r6[-1] + (1.0 if far else 0.0))
    kink(r7, probe - n, 0.06)
    az = 2e-3 * np.arange(2 * n)
    return np.concatenate([polar(r6, az[:n], elevation(6)), polar(r7, az[n:], elevation(7))]), walker, probe


def long_line(n=30000, line=6, noise=2e-5, seed=11):
    """a spiked ring line of more than 24 576 points with a normal extent (the multi-kernel per-line VoxelGrid, filtered)"""
    return spiked_ring((n - 11) // 6, (n - 11) % 6, line, noise=noise, seed=seed)


def long_zigzag(n=25200, line=6):
    """a zig-zag line of more than 24 576 points swept over most of a turn: more leaves than PCL's VoxelGrid indexes, so the per-line
    filter passes the line through"""
    return zigzag_line((n - 11) // 6, line, growth=0.1, az_step=5.5 / n, extra=(n - 11) % 6)


# ------------------------------------------------------------------------------------------------------ what a scan reaches
def subregions(line_n):
    """[(line, j, sp, ep)] of the non-empty sub-regions (laser_feature_extractor.hpp:636-637)"""
    out, n = [], 0
    for line, c in enumerate(np.asarray(line_n, np.int64)):
        start, end = n + 5, n + int(c) - 6
        n += int(c)
        for j in range(6):
            sp = (start * (6 - j) + end * j) // 6
            ep = (start * (5 - j) + end * (j + 1)) // 6 - 1
            if ep >= sp and end >= start:
                out.append((line, j, sp, ep))
    return out


def reach(r):
    """per sub-region of a restatement result: size, candidates (curvature above the sharp bound), sharp and less-sharp picks, the
    rank of its deepest pick in the descending (curvature, position) order, and whether its picks are exactly the top of that order"""
    curv = r["curvature"]
    ls, sh = r["less_sharp"], r["sharp"]
    rows = []
    for line, j, sp, ep in subregions(r["line_n"]):
        pos = np.arange(sp, ep + 1)
        order = pos[np.lexsort((pos, curv[sp:ep + 1]))][::-1]  # highest (curvature, position) first
        picks = ls[(ls >= sp) & (ls <= ep)]
        rank_of = np.empty(len(pos), np.int64)
        rank_of[order - sp] = np.arange(len(pos))
        ranks = rank_of[picks - sp]
        rows.append(dict(line=line, j=j, sp=sp, ep=ep, size=ep - sp + 1, candidates=int(np.count_nonzero(curv[sp:ep + 1] > SHARP_CURV)),
                         sharp=int(np.count_nonzero((sh >= sp) & (sh <= ep))), less_sharp=len(picks),
                         deepest=int(ranks.max()) if len(ranks) else -1, in_order=bool(np.all(np.diff(ranks) > 0)),
                         top=bool(np.array_equal(picks, order[:len(picks)]))))
    return rows


def tied_curvatures(r):
    """positions inside sub-regions whose curvature equals another's of the same sub-region"""
    curv, tied = r["curvature"], 0
    for _, _, sp, ep in subregions(r["line_n"]):
        _, counts = np.unique(curv[sp:ep + 1], return_counts=True)
        tied += int(counts[counts > 1].sum())
    return tied


def walk_len(full, ind, direction, limit=WALK):
    """steps the walk from position ind marks (:679-710): up to the first gap, the limit or the end of the cloud"""
    p = full[:, :3].astype(np.float32)
    steps = 0
    for l in range(1, limit + 1):
        q = ind + direction * l
        if q < 0 or q > len(p) - 1:
            break
        d = p[q] - p[q - direction]
        if np.float32(d[0] * d[0] + d[1] * d[1]) + np.float32(d[2] * d[2]) > np.float32(GAP2):
            break
        steps += 1
    return steps


# ------------------------------------------------------------------------------------------------------ the scans the tests share
FAMILIES = {
    "ring": spiked_ring,
    "zigzag": zigzag,
    "zigzag_jitter": lambda: zigzag(jitter=0.05),
    "ladder": ladder,
    "ladder_noise": lambda: ladder(noise=2e-5),
    "walk_limit": lambda: long_walks("limit"),
    "walk_past": lambda: long_walks("past"),
    "walk_cut": lambda: long_walks("cut"),
    "walk_ends": lambda: long_walks("ends"),
    "boundary_near": lambda: line_boundary(False)[0],
    "boundary_far": lambda: line_boundary(True)[0],
    "long_line": long_line,
    "long_zigzag": long_zigzag,
}
_cache = {}


def family(name):
    """(scan, restatement result with the per-line VoxelGrid), computed once per process; callers leave both unchanged"""
    if name not in _cache:
        from tests import spin_ref
        x = FAMILIES[name]()
        _cache[name] = (x, spin_ref.extract(x, scan_line=16))
    return _cache[name]
