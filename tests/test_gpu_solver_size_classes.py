"""-m gpu: the registrar at the feature counts where it switches its solver form and its neighbour-search form (the limits, the case
lists and the inputs come from tests/test_solver_size_classes_host.py, which holds the limits to the headers):

  reg_solve_small_kernel | reg_solve_kernel (solve_fast3)      2 048 features, 1 024 corner features
  solve_fast3 | reg_solve_big_kernel<0> (solve_big)            24 576 padded blocks: round 48, mask bit 47, the last slot register,
                                                               a group member's sixth trip
  solve_big | solve_general inside the same launch             61 440 padded blocks: round 120, bit 55 of the second mask word
  one sorting workgroup | segments | no tile search            24 576 / 98 304 surface queries

A case is the first nC corner and the first nS surface features of six scans' features concatenated in one sensor frame, registered
against the 40 k-point rooms map or against a uniform random cloud (nearly every block a plane of its own: full table regions, private
entries).  Every result is held to the oracle with the bounds of tests/test_gpu_reg.py; forms that group their sums differently agree
to 1e-9 with equal counts; inside one form a scan's pose does not depend on its slot, its batch or its neighbours, to the
bit.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.api import Map_buffer, Point_cloud_registration
from oracle import orc
from tests import test_solver_size_classes_host as H

pytestmark = pytest.mark.gpu
POSE_TOL_M, POSE_TOL_RAD = 1e-4, 1e-4   # BASELINE.json north_star (tests/test_gpu_reg.py)
ORACLE_TOL = 1e-7                       # "what we actually expect from identical algorithms in fp64" (tests/test_gpu_reg.py)
FORMS_TOL = 1e-9                        # forms that group their sums differently
ICP, CERES = H.ICP, H.CERES
FIGURES = {}                            # row of DESIGN 5's table -> largest (translation, rotation) difference to the oracle seen


class Case:
    """one scan's features, its start pose, and the oracle's answer"""

    def __init__(self, name, fc, fs, pose, ret, pc, rep):
        self.name, self.fc, self.fs, self.pose, self.ret, self.pc, self.rep = name, fc, fs, pose, ret, pc, rep


class World:
    """a map on the device, its k-d trees, and every oracle answer asked for so far: computed once, never changed"""

    def __init__(self, inp, corner, surf):
        self.inp, self.tree_c, self.tree_s, self.memo = inp, orc.KdTree(corner), orc.KdTree(surf), {}
        self.knn0 = None   # the surface tree's lists for the whole concatenated cloud at the start pose (check_knn_lists)
        self.map = Map_buffer()
        self.map.setInputCloud(Map_buffer.CORNER, corner)
        self.map.setInputCloud(Map_buffer.SURF, surf)

    def case(self, scan, icp=ICP, deblur=False, name=None, feats=None):
        """scan: (nC, nS) of the concatenated cloud, or with feats = (fc, fs) any cloud under `name`"""
        key = (name or scan, icp, bool(deblur))
        if key not in self.memo:
            inp = self.inp
            fc, fs = feats if feats is not None else (inp["fc"][:scan[0]], inp["fs"][:scan[1]])
            fc, fs = np.ascontiguousarray(fc), np.ascontiguousarray(fs)
            prm = H.oracle_params(icp, int(bool(deblur)), inp["tmin"], inp["tmax"])
            ret, pc, _, rep = orc.reg_solve(self.tree_c, self.tree_s, fc, fs, prm, inp["pose"], inp["pose"])
            pc.setflags(write=False)
            self.memo[key] = Case(str(name or scan), fc, fs, inp["pose"], ret, pc, rep)
        return self.memo[key]


@pytest.fixture(scope="module")
def rooms(gpu_lib):
    inp = H.inputs()
    w = World(inp, inp["corner"], inp["surf"])
    yield w
    w.map.close()
    for row, (dt, dr) in FIGURES.items():
        print(f"\nlargest pose difference to the oracle, {row}: {dt:.1e} m / {dr:.1e} rad")


@pytest.fixture(scope="module")
def cloud(gpu_lib):
    inp = H.inputs()
    corner, surf = H.random_cloud(inp)
    w = World(inp, corner, surf)
    yield w
    w.map.close()


def solve(w, cases, icp=ICP, deblur=False, max_features=None, debug=False, knn_iter=0, **switches):
    """one batch on a fresh registrar; returns (res, poses, reports, registrar or None): the registrar is kept open for its debug taps"""
    n = len(cases)
    if max_features is None:
        max_features = max(24000, max(max(len(c.fc), len(c.fs)) for c in cases))
    reg = Point_cloud_registration(max_scans=n, max_features=max_features)
    reg.set_debug(debug, **switches)
    if debug:
        reg.set_debug_knn_iteration(knn_iter)
    p = reg.params
    p.icp_max_iterations, p.ceres_max_iterations, p.force_all_iterations = icp, CERES, 1
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = 20.0, 0.3, 100.0
    p.current_frame_index, p.mapping_init_accumulate_frames = 100, 50
    p.maximum_allow_residual_block, p.subsample_seed = H.MAX_BLOCKS, 0
    if deblur:
        p.if_motion_deblur, p.minimum_pt_time_stamp, p.maximum_pt_time_stamp = 1, w.inp["tmin"], w.inp["tmax"]
    pl = np.stack([c.pose for c in cases])
    res, pc, _, reps = reg.solve_batch(w.map, [c.fc for c in cases], [c.fs for c in cases], pl, pl)
    if not debug:
        reg.close()
        reg = None
    return res, pc, reps, reg


def counts(r):
    return (r.icp_iterations, r.n_blocks_last, r.corner_avail, r.surf_avail, r.lm_iterations_total)


def check_oracle(tag, cases, res, pc, reps, row=None, row_slots=None):
    """row: the row of DESIGN 5's table the figures of the slots row_slots (default: all) go to"""
    fig = []
    for i, c in enumerate(cases):
        dt, dr = synth.pose_error(pc[i], c.pc)
        fig.append((dt, dr))
        print(f"{tag} scan {c.name:>14}: vs oracle {dt:.2e} m {dr:.2e} rad; blocks {reps[i].n_blocks_last} (oracle {c.rep.n_blocks_last}), "
              f"LM {reps[i].lm_iterations_total} ({c.rep.lm_iterations_total}), cost {reps[i].final_cost:.12g} ({c.rep.final_cost:.12g}), "
              f"threshold {reps[i].inlier_threshold:.12g} ({c.rep.inlier_threshold:.12g})")
        if row is not None and (row_slots is None or i in row_slots) and np.isfinite(dt) and np.isfinite(dr):
            old = FIGURES.get(row, (0.0, 0.0))
            FIGURES[row] = (max(old[0], dt), max(old[1], dr))
    for i, c in enumerate(cases):
        dt, dr = fig[i]
        g, o = reps[i], c.rep
        assert c.ret == 1, c.name                                        # the oracle accepts every case of this module
        assert res[i] == c.ret and np.all(np.isfinite(pc[i])), c.name
        assert dt <= POSE_TOL_M and dr <= POSE_TOL_RAD and dt < ORACLE_TOL and dr < ORACLE_TOL, (c.name, dt, dr)
        assert g.icp_iterations == o.icp_iterations and g.n_blocks_last == o.n_blocks_last, c.name
        assert g.corner_avail == o.corner_avail and g.surf_avail == o.surf_avail and g.lm_iterations_total == o.lm_iterations_total, c.name
        assert np.isclose(g.final_cost, o.final_cost, rtol=1e-8) and np.isclose(g.initial_cost, o.initial_cost, rtol=1e-8), c.name
        assert np.isclose(g.inlier_threshold, o.inlier_threshold, rtol=1e-8), c.name


def check_forms(tag, pose_a, rep_a, pose_b, rep_b):
    """two forms of the same scan: sums grouped differently, nothing else"""
    dt, dr = synth.pose_error(pose_a, pose_b)
    print(f"{tag}: {dt:.2e} m {dr:.2e} rad; counts {counts(rep_a)} / {counts(rep_b)}")
    assert dt < FORMS_TOL and dr < FORMS_TOL, (tag, dt, dr)
    assert counts(rep_a) == counts(rep_b), tag


def check_same_bits(tag, pose_a, pose_b):
    dt, dr = synth.pose_error(pose_a, pose_b)
    print(f"{tag}: bit-equal {np.array_equal(pose_a, pose_b)} ({dt:.2e} m {dr:.2e} rad)")
    assert np.array_equal(pose_a, pose_b), (tag, dt, dr)


# ---- 1. small to fast --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", H.SMALL_TO_FAST, ids=str)
def test_small_solver_to_fast3(rooms, scan):
    """2 048 features and 1 024 corner features are the small solver's last (W = 8), one more of either goes to solve_fast3 on one
    workgroup; the same scan with the small solver switched off is another form of it."""
    c = rooms.case(scan)
    res, pc, reps, _ = solve(rooms, [c])
    check_oracle(f"{H.scan_solver(scan, [scan])}", [c], res, pc, reps)
    res2, pc2, reps2, _ = solve(rooms, [c], no_small_solver=True)
    check_oracle("fast3 (no_small_solver)", [c], res2, pc2, reps2)
    if H.scan_solver(scan, [scan]) == "small":
        check_forms(f"{scan} small against fast3", pc[0], reps[0], pc2[0], reps2[0])
    else:
        check_same_bits(f"{scan} fast3 with and without the switch", pc[0], pc2[0])


# ---- 2. top of solve_fast3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan", H.FAST_TOP, ids=str)
def test_top_of_fast3(rooms, scan):
    """24 576 padded blocks: all 48 rounds, mask bit 47, the last of the 24 slot registers, a group member's sixth trip -- as a group
    of eight workgroups (B = 1), as one workgroup (no_solver_groups), and as slot 0 of batches of 17.  With the fillers (0, 1), (0, 513),
    (300, 4097) a corner-free scan's batch has padded_block_count(300, nS) > 24 576 and runs on reg_solve_big_kernel<0> (see
    tests/test_solver_size_classes_host.py batch_of_17); the corner-free fillers keep every scan's batch on reg_solve_kernel."""
    c = rooms.case(scan)
    assert H.scan_solver(scan, [scan]) == "fast3" and H.grouped([scan])
    res_g, pc_g, reps_g, _ = solve(rooms, [c])
    check_oracle("grouped", [c], res_g, pc_g, reps_g, row="top of fast")
    res_s, pc_s, reps_s, _ = solve(rooms, [c], no_solver_groups=True)
    check_oracle("single", [c], res_s, pc_s, reps_s, row="top of fast")
    check_forms(f"{scan} grouped against single", pc_g[0], reps_g[0], pc_s[0], reps_s[0])
    for fillers in (H.FILLERS, H.FILLERS_NO_CORNER):
        batch = H.batch_of_17(scan, fillers)
        form = H.scan_solver(scan, batch)
        cases = [rooms.case(s) for s in batch]
        res, pc, reps, _ = solve(rooms, cases)
        check_oracle(f"B=17 ({form})", cases, res, pc, reps, row="top of fast" if form == "fast3" else "top of big", row_slots=[0])
        for i in range(1, 14):   # the same filler in another slot
            check_same_bits(f"B=17 slots {i} / {i + 3}", pc[i], pc[i + 3])
        if form == "fast3":      # one workgroup per scan, like B = 1 with the groups off
            check_same_bits(f"{scan} slot 0 of 17 against B=1 single", pc[0], pc_s[0])
        else:
            check_forms(f"{scan} slot 0 of 17 (solve_big) against B=1 single", pc[0], reps[0], pc_s[0], reps_s[0])


@pytest.mark.parametrize("scan", H.FAST_OVER, ids=str)
def test_one_block_over_fast3_takes_solve_big(rooms, scan):
    """24 577 padded blocks (one corner feature, or one surface feature that opens round 49) leave reg_solve_kernel: solve_big, the
    first bit beyond the 64-bit masks' 48 -- alone and as slot 0 of a batch of 17 (one workgroup per scan both times)."""
    c = rooms.case(scan)
    assert H.scan_solver(scan, [scan]) == "big"
    res1, pc1, reps1, _ = solve(rooms, [c])
    check_oracle("B=1", [c], res1, pc1, reps1, row="top of big")
    cases = [rooms.case(s) for s in H.batch_of_17(scan)]
    res, pc, reps, _ = solve(rooms, cases)
    check_oracle("B=17", cases, res, pc, reps, row="top of big", row_slots=[0])
    check_same_bits(f"{scan} slot 0 of 17 against B=1", pc[0], pc1[0])
    for i in range(1, 14):
        check_same_bits(f"B=17 slots {i} / {i + 3}", pc[i], pc[i + 3])


# ---- 3. top of solve_big -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deblur", [False, True], ids=["plain", "deblur"])
@pytest.mark.parametrize("scan", H.BIG_TOP, ids=str)
def test_top_of_solve_big(rooms, scan, deblur):
    """61 440 padded blocks: round 120, the last bit the 128-bit masks use, the largest 16-bit plane id range -- reg_solve_big_kernel<0>
    and <1> (time stamps' range from the concatenated features); the same scan on solve_general is another form of it."""
    c = rooms.case(scan, deblur=deblur)
    assert H.scan_solver(scan, [scan], deblur=deblur) == "big"
    res, pc, reps, _ = solve(rooms, [c], deblur=deblur)
    check_oracle(f"solve_big<{int(deblur)}>", [c], res, pc, reps, row="top of big")
    res_g, pc_g, reps_g, _ = solve(rooms, [c], deblur=deblur, force_general_solver=True)
    check_oracle("solve_general (forced)", [c], res_g, pc_g, reps_g)
    check_forms(f"{scan} solve_big against solve_general", pc[0], reps[0], pc_g[0], reps_g[0])


@pytest.mark.parametrize("scan", H.BIG_OVER, ids=str)
def test_one_block_over_solve_big_takes_solve_general(rooms, scan):
    """61 441 padded blocks: solve_general in its natural range, by the scan's own count and not by the test switch"""
    c = rooms.case(scan)
    assert H.scan_solver(scan, [scan]) == "general"
    res, pc, reps, _ = solve(rooms, [c])
    check_oracle("solve_general", [c], res, pc, reps, row="general above 61 440")
    res_f, pc_f, _, _ = solve(rooms, [c], force_general_solver=True)
    check_same_bits(f"{scan} by its count against the force_general switch", pc[0], pc_f[0])


# ---- 4. mixed launches -------------------------------------------------------------------------------------------------------------------
def test_one_launch_runs_solve_general_beside_solve_big(rooms):
    """B = 4: slot 0 beyond 61 440 blocks (solve_general), slot 1 at 61 440 (solve_big), two small scans (solve_big) in one launch of
    reg_solve_big_kernel<0>.  A scan's answer does not depend on its slot or its neighbours: the two large scans, each
    alone on a fresh registrar, give the same bits."""
    batch = H.MIXED_B4
    assert [H.scan_solver(s, batch) for s in batch] == ["general", "big", "big", "big"]
    cases = [rooms.case(s) for s in batch]
    res, pc, reps, _ = solve(rooms, cases)
    check_oracle("B=4 slot 0", cases[:1], res[:1], pc[:1], reps[:1], row="general above 61 440")
    check_oracle("B=4", cases[1:], res[1:], pc[1:], reps[1:], row="top of big", row_slots=[0])
    for i, s in enumerate(batch):
        if H.padded_block_count(*s) > H.FAST_MAX_BLOCKS:
            _, pc1, _, _ = solve(rooms, [cases[i]])
            check_same_bits(f"{s} slot {i} of 4 against the scan alone", pc[i], pc1[0])


def test_maxima_of_two_scans_send_the_pair_to_the_big_kernel(rooms):
    """B = 2: (1000, 23000) and (10, 24064) each fit solve_fast3; padded_block_count(max_nc, max_ns) takes the 1 000 corner features of
    one and the 24 064 surface features of the other and sends the pair to reg_solve_big_kernel<0>.  Alone each takes solve_fast3 on a
    group of eight workgroups: another form."""
    batch = H.MIXED_B2
    assert H.batch_kernel(batch) == "big" and all(H.batch_kernel([s]) == "fast" for s in batch)
    cases = [rooms.case(s) for s in batch]
    res, pc, reps, _ = solve(rooms, cases)
    check_oracle("B=2", cases, res, pc, reps, row="top of big")
    for i, s in enumerate(batch):
        res1, pc1, reps1, _ = solve(rooms, [cases[i]])
        check_oracle("alone", [cases[i]], res1, pc1, reps1)
        check_forms(f"{s} in the pair (solve_big) against alone (solve_fast3)", pc[i], reps[i], pc1[0], reps1[0])


# ---- 5. full table regions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scan,cap,form", [(H.FULL_REGIONS[0][0], H.FULL_REGIONS[0][1], "grouped"), (H.FULL_REGIONS[0][0], H.FULL_REGIONS[0][1], "single"),
                                           (H.FULL_REGIONS[1][0], H.FULL_REGIONS[1][1], "grouped"), (H.FULL_REGIONS[1][0], H.FULL_REGIONS[1][1], "single"),
                                           (H.FULL_REGIONS[2][0], H.FULL_REGIONS[2][1], "big"),
                                           (H.FULL_REGIONS[2][0], H.FULL_REGIONS[2][1], "big-deblur")], ids=str)
def test_full_table_regions_against_a_random_cloud(cloud, scan, cap, form):
    """Against the random cloud nearly every surface block has a neighbour triple of its own, on a registrar whose max_features is
    exactly the scan's count (24 065 and 60 928 are no multiples of 4 096: the table region is the count rounded up).  Counted from the
    device's neighbour lists of the last ICP iteration: the blocks found, less every query that repeats another query's triple, is a
    lower bound of the scan's distinct active triples, and it exceeds the 8 192 hash slots.
    "single", "big", "big-deblur": one workgroup inserts all of them into one hash table, so thousands of blocks take private table
    entries, which count down from the top of the scan's region while the dense ids count up.
    "grouped": each of the eight members inserts only its own round of every eight (about 3 072 blocks) into a hash table of its own
    and practically never needs a private entry; what these cases fill is each member's region of tab_cap / 8 entries, one entry per
    block nearly everywhere.
    The same scan on solve_general builds no table."""
    deblur = form == "big-deblur"
    c = cloud.case(scan, icp=2, deblur=deblur)
    assert H.scan_solver(scan, [scan], deblur=deblur) == ("big" if form.startswith("big") else "fast3")
    res, pc, reps, reg = solve(cloud, [c], icp=2, deblur=deblur, max_features=cap, debug=True, knn_iter=1, no_solver_groups=(form == "single"))
    _, _, si, _ = reg.debug_knn(0, len(c.fc), len(c.fs))
    reg.close()
    triples = si[:, [0, 2, 4]]
    repeats = len(triples) - len(np.unique(triples, axis=0))
    print(f"{scan} {form}: surface blocks found {reps[0].surf_avail}, queries repeating a triple {repeats}")
    assert reps[0].surf_avail - repeats > H.PT_SLOTS
    check_oracle(form, [c], res, pc, reps, row="random cloud at full regions")
    res_g, pc_g, reps_g, _ = solve(cloud, [c], icp=2, deblur=deblur, max_features=cap, force_general_solver=True)
    check_oracle("solve_general (forced)", [c], res_g, pc_g, reps_g)
    check_forms(f"{scan} {form} against solve_general", pc[0], reps[0], pc_g[0], reps_g[0])


# ---- 6. segment edges of the tile search -------------------------------------------------------------------------------------------------
def check_knn_lists(w, reg, slot, c, pose, it):
    """the device's lists of one ICP iteration against the k-d trees at that iteration's pose: surface lists exactly (indices and
    squared distances), corner lists inside the match radius"""
    ci, _, si, sd = reg.debug_knn(slot, len(c.fc), len(c.fs))
    if it == 0:   # every case is a prefix of one cloud at one start pose: the tree is asked once
        if w.knn0 is None:
            w.knn0 = w.tree_s.knn(orc.cloud_transform(pose, w.inp["fs"][:max(H.TILE_EDGES)])[:, :3], 5)
        assert np.array_equal(c.fs, w.inp["fs"][:len(c.fs)]) and np.array_equal(pose, w.inp["pose"])
        oi, od = w.knn0[0][:len(c.fs)], w.knn0[1][:len(c.fs)]
    else:
        oi, od = w.tree_s.knn(orc.cloud_transform(pose, c.fs)[:, :3], 5)
    inside = od < 50.0
    bad = int((np.where(inside, oi, -1) != si).any(axis=1).sum()), int((np.where(inside, od, np.inf) != sd).any(axis=1).sum())
    print(f"{c.name} ICP iteration {it}: surface queries with another index list {bad[0]}, with other distances {bad[1]} of {len(c.fs)}")
    assert bad == (0, 0)
    oi, od = w.tree_c.knn(orc.cloud_transform(pose, c.fc)[:, :3], 5)
    assert np.array_equal(np.where(od < 2.0, oi, -1), ci)


def tile_edge_run(w, cases, **switches):
    """iteration 0's lists and the pose behind it from a registration of one ICP iteration, iteration 1's lists from one of two"""
    res1, pose1, _, reg = solve(w, cases, icp=1, debug=True, knn_iter=0, **switches)
    assert res1[0] == 1
    check_knn_lists(w, reg, 0, cases[0], cases[0].pose, 0)
    reg.close()
    res, pc, reps, reg = solve(w, cases, icp=2, debug=True, knn_iter=1, **switches)
    check_knn_lists(w, reg, 0, cases[0], pose1[0], 1)
    reg.close()
    return res, pc, reps


@pytest.mark.parametrize("ns", H.TILE_EDGES)
def test_tile_search_at_its_segment_edges(rooms, ns):
    """knn_tile_small_batches at B = 1: one sorting workgroup's last count (24 576), a second segment of one query (24 577), a third of
    one query (49 153), four full segments (98 304) and the first count without a tile search (98 305).  Beyond one segment the reuse
    lists run behind the tile search of ICP iterations 0 and 1: the lists of both iterations against the k-d tree, exactly."""
    scan = (H.TILE_NC, ns)
    assert H.knn_form([scan], tile_small_batches=True) == ((2 if ns <= H.LL_KNN_TILE_SEG else 1) if ns <= H.LL_KNN_TILE_MAX_SURF else 0, -(-ns // H.LL_KNN_TILE_SEG))
    c = rooms.case(scan, icp=2)
    res, pc, reps = tile_edge_run(rooms, [c], knn_tile_small_batches=True)
    check_oracle(f"tile edge {ns}", [c], res, pc, reps)


def test_tile_search_second_segment_of_one_query_in_a_batch_of_17(rooms):
    """the same 24 577 queries as slot 0 of a batch of 17, where the tile search is the default: two segments for slot 0, one short one
    for every other slot of the same launch"""
    batch = H.batch_of_17((H.TILE_NC, H.TILE_EDGES[1]))
    assert H.knn_form(batch) == (1, 2)
    cases = [rooms.case(s, icp=2) for s in batch]
    res, pc, reps = tile_edge_run(rooms, cases)
    check_oracle("tile edge, B=17", cases, res, pc, reps)


# ---- 7. / 8. duplicates ------------------------------------------------------------------------------------------------------------------
DUP_SET = (H.DUP_TWICE, H.DUP_THRICE, H.DUP_SEED)


@pytest.mark.parametrize("base,deblur,repeats", [(H.DUP_BASES[0], False, DUP_SET), (H.DUP_BASES[0], False, H.DUP_FEW[0]), (H.DUP_BASES[0], False, H.DUP_FEW[1]),
                                                 (H.DUP_BASES[1], False, DUP_SET), (H.DUP_BASES[1], True, DUP_SET)], ids=str)
def test_true_duplicates_on_the_exact_list(rooms, base, deblur, repeats):
    """compute_inlier_residual_threshold ranks the DISTINCT loss-corrected residuals (a std::set, PCR:155-160).  Surface features
    appended once more, some of them a third time (200 and 50; for solve_fast3 also two sets of 12 and 4), give exact repeats of L1
    values inside an otherwise natural scan: few enough for the exact list of twice-contested keys, where the list decides which
    occurrence of a value is the first.

    solve_big<0> and solve_big<1> (30 k features) take their list while it holds at most DD2_LIST (2 048) entries: the 450 entries of the
    repeated values plus the natural ones, about 600 - 700 at 41 - 50 k blocks by the estimate in ll_reg_big_path.h / DESIGN 4c.
    solve_fast3 (20 k features, grouped and single) takes its list only while, besides that, no thread owns more than two listed keys
    (inlier_threshold_regs: `over`).  Rows drawn freely put three to five repeated blocks on some threads and the scan on the fall-back
    that hashes every key, so the rows are drawn such that every repeated block has a thread of its own (H.repeated_rows; asserted in
    the CPU tier).  What remains open are the natural twice-contested keys (about 20 at 20 k blocks: ~1 500 keys contested in the first
    bitmap, squared over twice the second bitmap's 131 072 slots): a thread that owns two of them and a repeated block still overflows.
    With 450 repeated blocks that has a chance of about three in ten, with the 28 of a small set about one in fifty -- hence the two
    small sets.  Nobody has measured which route a scan took or how long its list was: no build makes either visible."""
    twice, thrice, seed = repeats
    fc, fs = rooms.inp["fc"][:base[0]], rooms.inp["fs"][:base[1]]
    fs2 = H.with_true_duplicates(fs, twice, thrice, seed)
    scan = (len(fc), len(fs2))
    fast = base == H.DUP_BASES[0]
    assert scan[1] == base[1] + twice + thrice and H.scan_solver(scan, [scan], deblur=deblur) == ("fast3" if fast else "big")
    c = rooms.case(scan, deblur=deblur, name=f"{base}+{twice}+{thrice} seed {seed}", feats=(fc, fs2))
    plain = rooms.case(base, deblur=deblur)
    print(f"oracle inlier threshold with the repeats {c.rep.inlier_threshold!r}, without {plain.rep.inlier_threshold!r}")
    assert c.rep.inlier_threshold != plain.rep.inlier_threshold   # the repeats do matter
    res, pc, reps, _ = solve(rooms, [c], deblur=deblur)
    check_oracle(H.scan_solver(scan, [scan], deblur=deblur) + (" grouped" if fast else ""), [c], res, pc, reps)
    res_g, pc_g, reps_g, _ = solve(rooms, [c], deblur=deblur, force_general_solver=True)
    check_oracle("solve_general (forced)", [c], res_g, pc_g, reps_g)
    check_forms(f"{scan} against solve_general", pc[0], reps[0], pc_g[0], reps_g[0])
    if fast:
        assert H.grouped([scan])
        res_s, pc_s, reps_s, _ = solve(rooms, [c], no_solver_groups=True)
        check_oracle("fast3 single", [c], res_s, pc_s, reps_s)
        check_forms(f"{scan} grouped against single", pc[0], reps[0], pc_s[0], reps_s[0])


@pytest.mark.parametrize("groups", [True, False], ids=["grouped", "single"])
def test_heavy_duplicates_inside_the_fast_range(rooms, groups):
    """The construction of test_duplicate_residuals_follow_std_set_semantics (tests/test_gpu_reg.py) on scan 0 thinned to 12 000 surface
    features -- a third of them twice, a sixth three times, 18 000 in all, so the batch stays on reg_solve_kernel: thousands of
    twice-contested keys, more than DD2_LIST and many per thread, either of which sends solve_fast3's inlier phase to its fall-back of
    hashing every key."""
    inp = rooms.inp
    fc2, fs2 = H.heavy_duplicates(inp["fc0"], inp["fs0"])
    scan = (len(fc2), len(fs2))
    assert H.scan_solver(scan, [scan]) == "fast3" and H.grouped([scan])
    c = rooms.case(scan, name="scan 0 heavy repeats", feats=(fc2, fs2))
    plain = rooms.case(scan, name="scan 0 thinned", feats=(inp["fc0"], H.spread(inp["fs0"], H.HEAVY_NS)))
    print(f"oracle inlier threshold with the repeats {c.rep.inlier_threshold!r}, without {plain.rep.inlier_threshold!r}")
    assert c.rep.inlier_threshold != plain.rep.inlier_threshold
    res, pc, reps, _ = solve(rooms, [c], no_solver_groups=not groups)
    check_oracle("fast3", [c], res, pc, reps)
    res_g, pc_g, reps_g, _ = solve(rooms, [c], force_general_solver=True)
    check_forms(f"{scan} against solve_general", pc[0], reps[0], pc_g[0], reps_g[0])
