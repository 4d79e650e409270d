"""CPU tier of tests/test_gpu_solver_size_classes.py: the feature counts at which the registrar switches its solver form and its
neighbour-search form, the cases built on them and the inputs those cases are cut from.

The GPU module imports every number, case list and input from here.  The limits are compile-time constants of the library; this module
reads them out of the headers and holds them to the numbers the cases were written with, and it restates the choices the host makes from
them (launch_reg_solve, reg_enqueue, scan_is_compact), so that a moved limit fails here, loudly, instead of leaving the edge cases
somewhere in the middle of a range.  No device is needed."""
import functools
import os
import re

import numpy as np

from loam_livox_amd import synth
from oracle import orc
from tests.conftest import oracle_features

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "loam_livox_amd", "csrc")

# ---- the limits (name -> the value the cases below were written with, the header that defines it) ------------------------------------
LL_SMALL_MAX_BLOCKS = 2048        # reg_solve_small_kernel up to this many corner + surface features ...
SMALL_MAX_CORNER = 1024           # ... and this many corner features (a literal in reg_solve_small_eligible)
FAST_MAX_BLOCKS = 24576           # solve_fast3: 48 rounds of 512 blocks
LL_TABLE_MAX_BLOCKS = 61440       # solve_big: 120 rounds; beyond, solve_general
LL_KNN_TILE_SEG = 24576           # surface queries one sorting workgroup orders
LL_KNN_TILE_MAX_SURF = 98304      # four segments; beyond, no tile search
PT_SLOTS = 8192                   # hash slots of the plane table's build: more distinct triples than that get private entries
DD2_LIST = 2048                   # twice-contested L1 keys the inlier phase compares exactly
LIMITS = {"LL_SMALL_MAX_BLOCKS": "ll_device.h", "FAST_MAX_BLOCKS": "ll_reg_query.h", "LL_TABLE_MAX_BLOCKS": "ll_reg_query.h",
          "LL_KNN_TILE_SEG": "ll_device.h", "LL_KNN_TILE_MAX_SURF": "ll_device.h", "PT_SLOTS": "ll_reg_solve_fast.h",
          "DD2_LIST": "ll_reg_solve_fast.h"}
# what the choices below also depend on (not limits of a solver form; held to the headers all the same)
RS_THREADS = 512                  # threads of a solver workgroup: the plane blocks are padded to whole rounds of it
LL_GRP_MIN_BLOCKS = 6000          # a batch whose largest scan has fewer features keeps one workgroup per scan
LL_GRP_MAX_SCANS = 16             # larger batches too
LL_KNN_COOP_MAX_SCANS = 16        # batches up to this size take the tile search only with knn_tile_small_batches
LL_KNN_TILE_MIN_SURF = 1024
OTHERS = {"RS_THREADS": "ll_reg_query.h", "LL_GRP_MIN_BLOCKS": "ll_device.h", "LL_GRP_MAX_SCANS": "ll_device.h",
          "LL_KNN_COOP_MAX_SCANS": "ll_device.h", "LL_KNN_TILE_MIN_SURF": "ll_device.h"}

ICP, CERES = 3, 20
MAX_BLOCKS = 200000               # maximum_allow_residual_block on both sides (strict mode, subsample_seed 0, refuses larger scans)


def header_constant(name, header):
    """the value of `#define name <integer expression of literals and other defines of that header>`"""
    with open(os.path.join(CSRC, header)) as f:
        text = f.read()
    m = re.search(r"^[ \t]*#define[ \t]+%s[ \t]+(.+?)[ \t]*(?://.*)?$" % re.escape(name), text, re.M)
    assert m, f"{name} is not defined in {header}"
    expr = re.sub(r"[A-Za-z_]\w*", lambda t: str(header_constant(t.group(0), header)), m.group(1))
    assert re.fullmatch(r"[0-9 ()*+/-]+", expr), (name, expr)
    return int(eval(expr, {"__builtins__": {}}))  # noqa: S307 (digits, brackets and arithmetic signs only)


def padded_block_count(nc, ns):
    """ll_reg_query.h: the planes padded to whole rounds of a solver workgroup, then the lines"""
    return (ns + RS_THREADS - 1) // RS_THREADS * RS_THREADS + nc


def one_feature_fewer(scan):
    """the smaller padded block count of the scan without its last corner or its last surface feature: an "over" case is over by one"""
    nc, ns = scan
    return min(padded_block_count(nc - 1, ns) if nc else 1 << 30, padded_block_count(nc, ns - 1) if ns else 1 << 30)


def batch_kernel(scans, deblur=False, general=False, no_small=False):
    """launch_reg_solve: "small", "fast" or "big" for a batch of (nC, nS) pairs -- from the two maxima, which may come from different scans"""
    max_nc, max_ns = max(c for c, _ in scans), max(s for _, s in scans)
    plain = not deblur and not general
    if plain and not no_small and 0 < max_nc + max_ns <= LL_SMALL_MAX_BLOCKS and max_nc <= SMALL_MAX_CORNER:
        return "small"
    if plain and padded_block_count(max_nc, max_ns) <= FAST_MAX_BLOCKS:
        return "fast"
    return "big"


def scan_solver(scan, scans, deblur=False, general=False):
    """the solver one scan of the batch runs on: "small", "fast3", "big" or "general" (scan_is_compact, per scan, inside the big kernel)"""
    k = batch_kernel(scans, deblur, general)
    if k != "big":
        return {"small": "small", "fast": "fast3"}[k]
    return "big" if not general and padded_block_count(*scan) <= LL_TABLE_MAX_BLOCKS else "general"


def grouped(scans, deblur=False, general=False, no_groups=False):
    """reg_enqueue: a group of eight workgroups per scan (only reg_solve_kernel spreads a scan over it)"""
    max_nc, max_ns = max(c for c, _ in scans), max(s for _, s in scans)
    return not (no_groups or len(scans) > LL_GRP_MAX_SCANS or deblur or general or max_nc + max_ns < LL_GRP_MIN_BLOCKS)


def knn_form(scans, tile_small_batches=False):
    """reg_enqueue: (tile search: 0 none, 1 at ICP iterations 0 / 1 with the reuse lists behind it, 2 in every iteration; sorted segments)"""
    max_ns = max(s for _, s in scans)
    tile = 2
    if max_ns < LL_KNN_TILE_MIN_SURF or max_ns > LL_KNN_TILE_MAX_SURF or (len(scans) <= LL_KNN_COOP_MAX_SCANS and not tile_small_batches):
        tile = 0
    if tile == 2 and max_ns > LL_KNN_TILE_SEG:
        tile = 1
    return tile, (max_ns + LL_KNN_TILE_SEG - 1) // LL_KNN_TILE_SEG


# ---- the cases: (nC, nS) = the first nC corner and the first nS surface features of the concatenated cloud ---------------------------
SMALL_TO_FAST = [(0, 2048), (0, 2049), (1024, 1024), (1025, 1023)]
FAST_TOP = [(0, 24576), (512, 24064), (0, 24065)]          # the last pads to 24 576: 511 dead blocks in round 48
FAST_OVER = [(1, 24065), (513, 24064), (0, 24577)]
FILLERS = [(0, 1), (0, 513), (300, 4097)]                  # the other slots of a batch of 17
FILLERS_NO_CORNER = [(0, 1), (0, 513), (0, 4097)]          # ... and a set that leaves max_nc to the scan under test (see batch_of_17)
BIG_TOP = [(0, 61440), (512, 60928)]
BIG_OVER = [(513, 60928), (0, 61441)]
MIXED_B4 = [(513, 60928), (512, 60928), (0, 1), (100, 300)]
MIXED_B2 = [(1000, 23000), (10, 24064)]
FULL_REGIONS = [((0, 24576), 24576), ((0, 24065), 24065), ((512, 60928), 60928)]   # (scan, max_features of its registrar)
TILE_NC = 300
TILE_EDGES = [24576, 24577, 49153, 98304, 98305]
DUP_BASES = [(300, 20000), (300, 30000)]
DUP_TWICE, DUP_THRICE, DUP_SEED = 200, 50, 7
DUP_FEW = [(12, 4, 11), (12, 4, 12)]   # (twice, thrice, seed): two small sets for solve_fast3's list, see test_true_duplicates_... (GPU module)
HEAVY_NS = 12000


def batch_of_17(scan, fillers=FILLERS):
    """slot 0: the scan under test; the others cycled from the fillers.  launch_reg_solve sees the batch's two maxima: with a corner-free
    scan of 24 065 - 24 576 surface features in slot 0, the 300 corner features of the filler (300, 4097) push padded_block_count(max_nc,
    max_ns) over FAST_MAX_BLOCKS and the whole batch runs on reg_solve_big_kernel<0>.  That batch is kept (a top-of-fast scan inside
    solve_big, beside small ones); FILLERS_NO_CORNER gives the batch that stays on reg_solve_kernel."""
    return [scan] + [fillers[i % len(fillers)] for i in range(16)]


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def inputs():
    """the 40 k-point rooms map, six scans taken from scan 0's pose with their features concatenated into one cloud in one sensor
    frame, scan 0's own features, the start pose and the range of the time stamps (the features' fourth column)"""
    world, corner, surf = synth.make_maps(40_000)
    sc0 = synth.make_scan(world, 0)
    _, _, _, _, fc0, fs0 = oracle_features(sc0)
    fcs, fss = [], []
    for k in range(6):
        _, _, _, _, fc, fs = oracle_features(synth.make_scan(world, k, pose_true=sc0.pose_true))
        fcs.append(fc)
        fss.append(fs)
    fc, fs = np.ascontiguousarray(np.concatenate(fcs)), np.ascontiguousarray(np.concatenate(fss))
    stamps = np.concatenate([fc[:, 3], fs[:, 3]])
    for a in (corner, surf, fc, fs):
        a.setflags(write=False)
    return dict(world=world, corner=corner, surf=surf, fc=fc, fs=fs, fc0=fc0, fs0=fs0, pose=sc0.pose_init.copy(),
                tmin=float(stamps.min()), tmax=float(stamps.max()))


def random_cloud(inp):
    """the construction of the `noise` fixture of tests/test_gpu_solver_table_in_lds.py over all the surface features: nearly every query
    has a neighbour triple of its own"""
    rng = np.random.default_rng(5)
    q = synth.transform_points(inp["pose"], inp["fs"][:, :3])
    lo, hi = q.min(0) - 1.0, q.max(0) + 1.0
    corner = rng.uniform(lo, hi, (60000, 3)).astype(np.float32)
    surf = rng.uniform(lo, hi, (400000, 3)).astype(np.float32)
    return corner, surf


def spread(a, n):
    """n rows spread evenly over a (tests/test_gpu_solver_table_in_lds.py)"""
    return a[np.linspace(0, len(a) - 1, n).astype(np.int64)]


def repeated_rows(n, twice, thrice, seed):
    """`twice` row indices of an n-row surface cloud, drawn with a fixed seed, such that the rows and their appended copies (rows n ..
    n + twice + thrice - 1) all fall on different threads of a solver workgroup.  A surface feature's plane block has the feature's
    index (planes come first), and the inlier phase gives block j to thread j % RS_THREADS (ll_reg_solve_fast.h inlier_phase3: "block
    j = tid + k * RS_THREADS").  Every occurrence of a repeated value is a twice-contested key, and solve_fast3 takes its exact list
    only while no thread owns more than two of them (inlier_threshold_regs: `over`): one per thread leaves room for one natural
    twice-contested key beside it."""
    assert 2 * twice + thrice <= RS_THREADS and thrice <= twice
    taken = {(n + i) % RS_THREADS for i in range(twice + thrice)}
    rep = []
    for i in np.random.default_rng(seed).permutation(n):
        if len(rep) == twice:
            break
        if int(i) % RS_THREADS not in taken:
            taken.add(int(i) % RS_THREADS)
            rep.append(int(i))
    assert len(rep) == twice
    return np.array(rep, np.int64)


def listed_blocks_per_thread(n, rep, thrice):
    """how many blocks with a repeated value each of the RS_THREADS threads owns"""
    blocks = np.concatenate([rep, n + np.arange(len(rep) + thrice)])
    return np.bincount(blocks % RS_THREADS, minlength=RS_THREADS)


def with_true_duplicates(fs, twice=DUP_TWICE, thrice=DUP_THRICE, seed=DUP_SEED):
    """fs, then `twice` of its rows once more, then `thrice` of those a third time (fixed seed; one repeated block per thread at most):
    exact repeats of L1 values in a natural scan"""
    rep = repeated_rows(len(fs), twice, thrice, seed)
    return np.ascontiguousarray(np.concatenate([fs, fs[rep], fs[rep[:thrice]]]))


def heavy_duplicates(fc, fs):
    """the construction of test_duplicate_residuals_follow_std_set_semantics (tests/test_gpu_reg.py) on a scan thinned to 12 000 surface
    features: a third of them twice, a sixth three times, half the corner features twice"""
    fs = spread(fs, HEAVY_NS)
    rep = np.random.default_rng(3).choice(len(fs), len(fs) // 3, replace=False)
    return np.ascontiguousarray(np.concatenate([fc, fc[: len(fc) // 2]])), np.ascontiguousarray(np.concatenate([fs, fs[rep], fs[rep[: len(rep) // 2]]]))


def oracle_params(icp=ICP, deblur=0, tmin=0.0, tmax=1.0):
    prm = orc.RegParams.defaults(icp_iters=icp, ceres_iters=CERES, force_all=1, deblur=deblur)
    prm.maximum_allow_residual_block, prm.subsample_seed = MAX_BLOCKS, 0
    if deblur:
        prm.minimum_pt_time_stamp, prm.maximum_pt_time_stamp = tmin, tmax
    return prm


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
def test_limits_in_the_headers_are_the_numbers_the_cases_were_written_with():
    for name, header in {**LIMITS, **OTHERS}.items():
        assert header_constant(name, header) == globals()[name], (name, header)
    assert len(LIMITS) == 7
    # two limits the sources spell as literals
    with open(os.path.join(CSRC, "ll_reg_small_kernels.hip")) as f:
        assert re.search(r"max_nc \+ max_ns <= LL_SMALL_MAX_BLOCKS && max_nc <= %d;" % SMALL_MAX_CORNER, f.read())
    with open(os.path.join(CSRC, "ll_api_reg.hip")) as f:
        assert re.search(r"lim = d\.cap_s < %d \? d\.cap_s : %d;" % (LL_TABLE_MAX_BLOCKS, LL_TABLE_MAX_BLOCKS), f.read())
    with open(os.path.join(CSRC, "ll_reg_query.h")) as f:
        assert "return (nS + RS_THREADS - 1) / RS_THREADS * RS_THREADS + nC;" in f.read()   # what padded_block_count() above restates
    # the ranges the cases count on
    assert FAST_MAX_BLOCKS == 48 * RS_THREADS and LL_TABLE_MAX_BLOCKS == 120 * RS_THREADS and LL_KNN_TILE_MAX_SURF == 4 * LL_KNN_TILE_SEG
    assert LL_TABLE_MAX_BLOCKS - 1 < 0xFFFE   # the largest 16-bit plane id stays below the sentinels PT_INACTIVE / PT_PRIVATE


def test_every_case_lies_on_the_side_of_its_boundary_it_is_named_for():
    assert padded_block_count(0, 1) == 512 and padded_block_count(3, 512) == 515 and padded_block_count(0, 513) == 1024
    # 1. small to fast
    assert [scan_solver(s, [s]) for s in SMALL_TO_FAST] == ["small", "fast3", "small", "fast3"]
    assert sum(SMALL_TO_FAST[0]) == LL_SMALL_MAX_BLOCKS and sum(SMALL_TO_FAST[1]) == LL_SMALL_MAX_BLOCKS + 1
    assert SMALL_TO_FAST[2] == (SMALL_MAX_CORNER, LL_SMALL_MAX_BLOCKS - SMALL_MAX_CORNER) and SMALL_TO_FAST[3][0] == SMALL_MAX_CORNER + 1
    assert sum(SMALL_TO_FAST[3]) == LL_SMALL_MAX_BLOCKS
    assert not any(grouped([s]) for s in SMALL_TO_FAST)
    # 2. top of solve_fast3: exactly the limit, alone (grouped and not) and in the corner-free batch of 17; one block over: the big kernel
    for s in FAST_TOP:
        assert padded_block_count(*s) == FAST_MAX_BLOCKS and scan_solver(s, [s]) == "fast3" and scan_solver(s, [s], general=True) == "general"
        assert grouped([s]) and not grouped([s], no_groups=True)
        b = batch_of_17(s, FILLERS_NO_CORNER)
        assert len(b) == 17 and batch_kernel(b) == "fast" and not grouped(b)
        assert all(scan_solver(x, batch_of_17(s)) == ("fast3" if s[0] >= 300 else "big") for x in batch_of_17(s))
    assert FAST_TOP[2][1] % RS_THREADS == 1 and padded_block_count(*FAST_TOP[2]) - sum(FAST_TOP[2]) == RS_THREADS - 1   # 511 dead blocks
    for s in FAST_OVER:
        assert padded_block_count(*s) > FAST_MAX_BLOCKS and one_feature_fewer(s) <= FAST_MAX_BLOCKS and scan_solver(s, [s]) == "big"
        assert all(scan_solver(x, batch_of_17(s)) == "big" for x in batch_of_17(s))
    for s in FILLERS + FILLERS_NO_CORNER:
        assert scan_solver(s, [s, FAST_TOP[1]]) == "fast3"
    # 3. top of solve_big, without and with motion deblur; one over: solve_general
    for s in BIG_TOP:
        assert padded_block_count(*s) == LL_TABLE_MAX_BLOCKS
        assert scan_solver(s, [s]) == "big" and scan_solver(s, [s], deblur=True) == "big"
    for s in BIG_OVER:
        assert padded_block_count(*s) > LL_TABLE_MAX_BLOCKS and one_feature_fewer(s) <= LL_TABLE_MAX_BLOCKS and scan_solver(s, [s]) == "general"
    # 4. mixed launches
    assert [scan_solver(s, MIXED_B4) for s in MIXED_B4] == ["general", "big", "big", "big"]
    assert all(scan_solver(s, [s]) == "fast3" for s in MIXED_B2) and [scan_solver(s, MIXED_B2) for s in MIXED_B2] == ["big", "big"]
    assert padded_block_count(max(c for c, _ in MIXED_B2), max(s for _, s in MIXED_B2)) > FAST_MAX_BLOCKS
    # 5. full table regions: the scan's count is the registrar's capacity, whose table region is that rounded up to 4096 entries
    for s, cap in FULL_REGIONS:
        assert cap == s[1] and padded_block_count(*s) in (FAST_MAX_BLOCKS, LL_TABLE_MAX_BLOCKS) and scan_solver(s, [s]) in ("fast3", "big")
        assert s[1] <= (min(cap, LL_TABLE_MAX_BLOCKS) + 4095) // 4096 * 4096 <= LL_TABLE_MAX_BLOCKS   # tab_cap (ll_reg_create)
    assert FULL_REGIONS[1][1] % 4096 != 0 and FULL_REGIONS[2][1] % 4096 != 0
    # 6. segments of the tile search
    forms = [knn_form([(TILE_NC, n)], tile_small_batches=True) for n in TILE_EDGES]
    assert forms == [(2, 1), (1, 2), (1, 3), (1, 4), (0, 5)]
    assert TILE_EDGES[1] % LL_KNN_TILE_SEG == 1 and TILE_EDGES[2] % LL_KNN_TILE_SEG == 1   # a last segment of one query
    assert knn_form([(TILE_NC, TILE_EDGES[1])]) == (0, 2) and knn_form(batch_of_17((TILE_NC, TILE_EDGES[1]))) == (1, 2)
    # 7. / 8. duplicates: the solver each base reaches; no thread of the inlier phase owns more than one block with a repeated value
    for n in (DUP_BASES[0][1], DUP_BASES[1][1]):
        for twice, thrice, seed in [(DUP_TWICE, DUP_THRICE, DUP_SEED)] + DUP_FEW:
            rep = repeated_rows(n, twice, thrice, seed)
            per_thread = listed_blocks_per_thread(n, rep, thrice)
            assert len(np.unique(rep)) == twice and rep.max() < n
            assert per_thread.sum() == 2 * twice + thrice and per_thread.max() == 1, (n, twice, thrice, seed)
    heavy = np.random.default_rng(3).choice(HEAVY_NS, HEAVY_NS // 3, replace=False)
    assert listed_blocks_per_thread(HEAVY_NS, heavy, HEAVY_NS // 6).max() > 2 and HEAVY_NS + HEAVY_NS // 2 > DD2_LIST   # the fall-back, both ways
    extra = DUP_TWICE + DUP_THRICE
    assert scan_solver((DUP_BASES[0][0], DUP_BASES[0][1] + extra), [(DUP_BASES[0][0], DUP_BASES[0][1] + extra)]) == "fast3"
    big = (DUP_BASES[1][0], DUP_BASES[1][1] + extra)
    assert scan_solver(big, [big]) == "big" and scan_solver(big, [big], deblur=True) == "big"


def test_concatenated_features_and_the_oracle_on_the_smallest_and_largest_case():
    inp = inputs()
    fc, fs = inp["fc"], inp["fs"]
    print(f"concatenated cloud: {len(fc)} corner, {len(fs)} surface features; scan 0 alone {len(inp['fc0'])} / {len(inp['fs0'])}")
    assert len(fs) >= max(TILE_EDGES) and len(fs) >= LL_TABLE_MAX_BLOCKS + 1 and len(fc) >= SMALL_MAX_CORNER + 1
    assert np.all(np.isfinite(fc)) and np.all(np.isfinite(fs))
    assert len(np.unique(fs, axis=0)) == len(fs) and len(np.unique(fc, axis=0)) == len(fc)
    assert len(np.unique(fs[:, :3], axis=0)) == len(fs)   # distinct positions, not only distinct stamps
    assert len(inp["fs0"]) >= HEAVY_NS and inp["tmin"] < inp["tmax"]
    # test_duplicate_residuals_follow_std_set_semantics[general=False] (tests/test_gpu_reg.py) repeats scan 0's features of the 200 k map
    # of conftest.py; with its counts the batch leaves reg_solve_kernel, the thinned construction here stays on it
    fc2, fs2 = heavy_duplicates(inp["fc0"], inp["fs0"])
    assert scan_solver((len(fc2), len(fs2)), [(len(fc2), len(fs2))]) == "fast3" and len(fs2) == HEAVY_NS + HEAVY_NS // 3 + HEAVY_NS // 6
    tree_c, tree_s = orc.KdTree(inp["corner"]), orc.KdTree(inp["surf"])
    for (nc, ns), icp in (((0, 1), ICP), ((TILE_NC, max(TILE_EDGES)), 2)):
        ret, pc, _, rep = orc.reg_solve(tree_c, tree_s, fc[:nc], fs[:ns], oracle_params(icp), inp["pose"], inp["pose"])
        print(f"oracle ({nc}, {ns}): ret {ret}, blocks {rep.n_blocks_last}, surf_avail {rep.surf_avail}, LM iterations {rep.lm_iterations_total}")
        assert ret == 1 and np.all(np.isfinite(pc)) and rep.icp_iterations == icp and rep.surf_avail == ns


def test_random_cloud_gives_more_distinct_triples_than_hash_slots():
    """the first-iteration neighbour triples of the 24 576-feature case against the random cloud: more distinct ones than PT_SLOTS, so
    private table entries are certain"""
    inp = inputs()
    _, surf = random_cloud(inp)
    ns = FULL_REGIONS[0][0][1]
    oi, od = orc.KdTree(surf).knn(synth.transform_points(inp["pose"], inp["fs"][:ns, :3]), 5)
    found = od[:, 4] < 50.0
    distinct = len(np.unique(oi[found][:, [0, 2, 4]], axis=0))
    print(f"random cloud, {ns} queries: {int(found.sum())} with five neighbours, {distinct} distinct triples")
    assert distinct > PT_SLOTS
