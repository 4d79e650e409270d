"""-m gpu: the key-frame map refinement on the device (api.Map_refine over ll_map_refine_*) against the oracle's VoxelGrid composed with
the numpy move of tests/map_refine_inputs.py -- float bits, counts and status, no tolerance.  Reads nothing of the reference.
The ragged set runs the chain at up to 40 selections of filtered clouds; mi.many_selections and mi.last_voxel_at_the_end, stored as
given, run it past the 256-selection trips of mr_offsets_kernel, with wavefronts of mr_head_kernel over many selections, at the
selection counts where the sort width changes, at the MR_CHUNK bounds, with non-finite rows inside filtered selections and with no
sentinel behind the last voxel."""
import numpy as np
import pytest

from loam_livox_amd.api import Map_refine
from tests import map_refine_inputs as mi
from tests.map_refine_inputs import bits

pytestmark = pytest.mark.gpu


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def filled(raw, **kw):
    """a handle with raw_clouds' entries added in order -> (handle, [(status, stored cloud)] as the oracle has them)"""
    mr = Map_refine(**kw)
    stored = mi.stored_clouds(raw)
    for k, ((name, cloud, leaf), (st, want)) in enumerate(zip(raw, stored)):
        cid, kept, status = mr.add_cloud(cloud, leaf)
        assert (cid, kept, status) == (k, len(want), st), name
    return mr, stored


@pytest.fixture(scope="module")
def ragged(gpu_lib):
    """the ragged set on the device, its oracle copies, and one scrambled selection with duplicates: made once, shared, not changed"""
    raw = mi.raw_clouds()
    mr, stored = filled(raw, initial_points=1 << 16)
    ids = [int(i) for i in np.random.default_rng(3).permutation(len(raw))] + [10, 3, 11, 11]
    ori, opm = mi.poses(len(ids), 23)
    yield dict(mr=mr, names=[n for n, _, _ in raw], stored=stored, ids=ids, ori=ori, opm=opm)
    mr.close()


def test_the_adds_store_what_the_oracle_filters(ragged):
    mr, names = ragged["mr"], ragged["names"]
    assert len(mr) == len(names)
    for k, (st, want) in enumerate(ragged["stored"]):
        assert same(mr.cloud(k), want), names[k]
    sts = {n: st for n, (st, _) in zip(names, ragged["stored"])}
    assert sts["non_finite"] == 2 and sts["box0"] == 2 and sts["cube300"] == 0 and sts["cube700"] == 1 and sts["one_voxel"] == 1 and sts["box5000"] == 0


@pytest.mark.parametrize("transform_first", [False, True])
def test_ragged_batch_in_one_run(ragged, transform_first):
    mr, names, ids, ori, opm = (ragged[k] for k in ("mr", "names", "ids", "ori", "opm"))
    clouds = mr.refine(ids, ori, opm, mi.RUN_LEAF, transform_first)
    work = mr.work()
    seen = set()
    for s, cid in enumerate(ids):
        st, want = mi.expected(ragged["stored"][cid][1], ori[s], opm[s], mi.RUN_LEAF, transform_first)
        assert mr.status[s] == st and same(clouds[s], want), (names[cid], s)
        assert not clouds[s][:, 3].any()                                # the output intensity is 0 everywhere
        seen.add(st)
    assert seen == {0, 1, 2}
    one = names.index("one_voxel")
    if not transform_first:                                            # 3000 points of one voxel, across a chunk boundary, are one point
        assert len(ragged["stored"][one][1]) == 3500 and len(clouds[ids.index(one)]) <= 501
    # one chain, one wait for the offsets, one more copy and wait for the fetch -- over the sum of the selections' points
    assert work[0] == 15 and work[1] == 2 and work[3] == sum(len(ragged["stored"][c][1]) for c in ids)
    # merge: VoxelGrid over the concatenated outputs, taken as one cloud
    flat = np.concatenate(clouds)
    st, want = mi.filtered(flat, mi.RUN_LEAF)
    assert same(mr.merge(mi.RUN_LEAF), want) and mr.merge_status == st


def test_merge_of_nearby_clouds_filters(ragged):
    mr, names, stored = ragged["mr"], ragged["names"], ragged["stored"]
    ids = [k for k, n in enumerate(names) if n.startswith("box") or n == "one_voxel"]
    ori, opm = mi.poses(len(ids), 29)
    for transform_first in (False, True):
        flat = np.concatenate(mr.refine(ids, ori, opm, mi.RUN_LEAF, transform_first))
        st, want = mi.filtered(flat, mi.RUN_LEAF)
        assert st == 0 and 0 < len(want) < len(flat) and same(mr.merge(mi.RUN_LEAF), want) and mr.merge_status == 0


def test_a_selections_output_does_not_depend_on_its_slot_or_the_run(ragged):
    mr, names = ragged["mr"], ragged["names"]
    me = names.index("box5000")
    ori, opm = mi.poses(40, 31)
    for transform_first in (False, True):
        alone = mr.refine([me], ori[37:38], opm[37:38], mi.RUN_LEAF, transform_first)[0]
        work_1 = mr.work()
        again = mr.refine([me], ori[37:38], opm[37:38], mi.RUN_LEAF, transform_first)[0]
        first = mr.refine([me] + [3, 9, 11, 9], np.concatenate([ori[37:38], ori[:4]]), np.concatenate([opm[37:38], opm[:4]]), mi.RUN_LEAF, transform_first)[0]
        around = [int(i) for i in np.random.default_rng(7).integers(0, len(names), 40)]
        around[37] = me
        inside = mr.refine(around, ori, opm, mi.RUN_LEAF, transform_first)[37]
        work_40 = mr.work()
        assert len(alone) > 1000 and same(again, alone) and same(first, alone) and same(inside, alone)
        # the launches and the waits do not depend on n_sel (the bytes and the points do)
        assert work_1[0] == work_40[0] == 15 and work_1[1] == work_40[1] == 2 and work_40[2] > work_1[2] and work_40[3] > work_1[3]


def test_growth_keeps_the_earlier_clouds(gpu_lib):
    rng = np.random.default_rng(41)
    mr = Map_refine(initial_points=1024)
    raws, kept = [], []
    for n in (700, 900, 1500, 3000, 257, 6000):                          # 1024 -> 2048 -> 4096 -> 8192 -> 16384: past three doublings
        p = rng.uniform(-30, 30, (n, 4)).astype(np.float32)
        cid, n_kept, st = mr.add_cloud(p, mi.ADD_LEAF)
        raws.append(p)
        kept.append(mr.cloud(cid))
        assert st == 0 and cid == len(raws) - 1
        for k, (raw, before) in enumerate(zip(raws, kept)):              # every earlier cloud, after every add
            now = mr.cloud(k)
            assert same(now, before) and same(now, orc_filtered(raw)), (n, k)
    assert sum(len(c) for c in kept) > 8 * 1024
    mr.close()


def orc_filtered(raw):
    return mi.filtered(raw, mi.ADD_LEAF)[1]


def test_selection_order_is_output_order_and_an_empty_run_launches_nothing(ragged):
    mr, stored = ragged["mr"], ragged["stored"]
    ids = [9, 4, 9, 1, 12, 8]
    ori, opm = mi.poses(len(ids), 37)
    fwd = mr.refine(ids, ori, opm)
    rev = mr.refine(ids[::-1], ori[::-1], opm[::-1])
    for s in range(len(ids)):
        assert same(fwd[s], rev[len(ids) - 1 - s]) and same(fwd[s], mi.expected(stored[ids[s]][1], ori[s], opm[s])[1]), s
    offsets, status = mr.run([], np.zeros((0, 7)), np.zeros((0, 7)))
    assert offsets.tolist() == [0] and len(status) == 0 and mr.work().tolist() == [0, 0, 0, 0]
    assert mr.refine([], np.zeros((0, 7)), np.zeros((0, 7))) == []
    # a run of empty clouds alone has nothing to sort either
    offsets, status = mr.run([0, 12, 0], *mi.poses(3, 1))
    assert offsets.tolist() == [0, 0, 0, 0] and status.tolist() == [2, 2, 2] and mr.work()[0] == 0


def test_refusals_leave_the_store_and_the_last_outputs(ragged):
    from loam_livox_amd.capi import LoamLivoxError
    mr = ragged["mr"]
    ori, opm = mi.poses(2, 43)
    before = mr.refine([10, 5], ori, opm)
    n_clouds = len(mr)
    nan_pose = ori.copy()
    nan_pose[1, 2] = np.nan
    for args, text in [(([10, len(mr)], ori, opm), "id out of range"), (([-1, 5], ori, opm), "id out of range"),
                       (([10, 5], ori, opm, 0.0), "positive and finite"), (([10, 5], ori, opm, float("inf")), "positive and finite"),
                       (([10, 5], nan_pose, opm), "a pose is not finite"), (([10, 5], ori, nan_pose), "a pose is not finite")]:
        with pytest.raises(LoamLivoxError, match=text):
            mr.run(*args)
    with pytest.raises(LoamLivoxError, match="positive and finite"):
        mr.add_cloud(np.zeros((3, 4), np.float32), -1.0)
    with pytest.raises(LoamLivoxError, match="id out of range"):
        mr.cloud(n_clouds)
    with pytest.raises(LoamLivoxError, match="capacity below"):
        flat = np.zeros((1, 4), np.float32)
        from loam_livox_amd.capi import check, ptr
        check(mr.L.ll_map_refine_fetch(mr.h, ptr(flat), 1), "ll_map_refine_fetch")
    assert len(mr) == n_clouds
    flat = np.zeros((sum(len(c) for c in before), 4), np.float32)     # the last outputs are still there to fetch
    assert mr.L.ll_map_refine_fetch(mr.h, flat.ctypes.data, len(flat)) == 0 and same(flat, np.concatenate(before))


def test_far_from_the_origin(gpu_lib):
    raw = mi.raw_clouds(seed=47, centre=(5000.0, 5000.0, 0.0))[7:12]      # box256 .. box5000 and the one-voxel cloud, 5 km out
    mr, stored = filled(raw, initial_points=1 << 15)
    ids = [4, 0, 3, 2, 1]
    ori, opm = mi.poses(len(ids), 53, far=5000.0)
    for transform_first in (False, True):
        clouds = mr.refine(ids, ori, opm, mi.RUN_LEAF, transform_first)
        for s, cid in enumerate(ids):
            st, want = mi.expected(stored[cid][1], ori[s], opm[s], mi.RUN_LEAF, transform_first)
            assert mr.status[s] == st == 0 and same(clouds[s], want), (raw[cid][0], transform_first)
            assert np.abs(clouds[s][:, :2]).min() > 4900.0
    mr.close()


# ---- where the chain changes form: trips of mr_offsets_kernel, wavefronts of many selections, sort widths, chunk bounds, the keys' end ------
def stored(store, **kw):
    """a handle that holds `store` as given (add_stored): id = position"""
    mr = Map_refine(**kw)
    for k, cloud in enumerate(store):
        assert mr.add_stored(cloud) == k
        assert mr.work().tolist() == ([1, 1, 16 * len(cloud), len(cloud)] if len(cloud) else [0, 0, 0, 0])
    return mr


def assert_run(mr, ids, ori, opm, want, transform_first, what=()):
    """a run over ids equals want = [(status, cloud)] in bits; -> the clouds"""
    clouds = mr.refine(ids, ori, opm, mi.RUN_LEAF, transform_first)
    assert len(clouds) == len(want)
    for s, (st, cloud) in enumerate(want):
        assert mr.status[s] == st and same(clouds[s], cloud), (*what, transform_first, s, ids[s])
    return clouds


@pytest.fixture(scope="module")
def many(gpu_lib):
    """mi.many_selections, the oracle's results of the 600 in both modes and the conditions they meet -- all before the device is touched --
    then the set on a handle: made once, shared, not changed"""
    store, ids, ori, opm = mi.many_selections(83)
    want = mi.expected_run(store, ids, ori, opm)
    figures = {tf: mi.many_conditions(store, ids, want[tf]) for tf in (False, True)}
    mr = stored(store, initial_points=1 << 12)
    for k, cloud in enumerate(store):                                    # kept as given, non-finite rows included
        assert same(mr.cloud(k), cloud), k
    yield dict(mr=mr, store=store, ids=ids, ori=ori, opm=opm, want=want, figures=figures)
    mr.close()


@pytest.mark.parametrize("transform_first", [False, True])
def test_600_selections_in_one_run(many, transform_first):
    mr, store, ids, ori, opm = (many[k] for k in ("mr", "store", "ids", "ori", "opm"))
    print("many_selections:", many["figures"][transform_first])
    clouds = assert_run(mr, ids, ori, opm, many["want"][transform_first], transform_first)
    work = mr.work()
    assert work[0] == 15 and work[1] == 2 and work[3] == sum(len(store[c]) for c in ids)
    st, want = mi.filtered(np.concatenate(clouds), mi.RUN_LEAF)
    assert same(mr.merge(mi.RUN_LEAF), want) and mr.merge_status == st


@pytest.mark.parametrize("n_sel", [2, 3, 4, 7, 8, 255, 256, 257, 511, 512, 513])
def test_selection_counts_where_the_sort_width_changes(many, n_sel):
    """32 + sel_bits key bits are sorted, 2^sel_bits >= n_sel + 1: at 3, 7, 255 and 511 selections the sentinel's low bits are n_sel itself"""
    mr, ids, ori, opm = (many[k] for k in ("mr", "ids", "ori", "opm"))
    for transform_first in (False, True):
        assert_run(mr, ids[:n_sel], ori[:n_sel], opm[:n_sel], many["want"][transform_first][:n_sel], transform_first, (n_sel,))


def test_shrinking_back_after_growth_leaves_nothing_behind(many):
    store, ids, ori, opm = (many[k] for k in ("store", "ids", "ori", "opm"))
    mr, fresh = stored(store, initial_points=1 << 10), stored(store, initial_points=1 << 10)
    few = [mi.MANY_2049, 5, mi.MANY_CUBE, mi.MANY_NAN, 0]               # two work items, finite and non-finite rows, handed back, empty
    for transform_first in (False, True):
        want5 = [mi.expected(store[c], ori[s], opm[s], mi.RUN_LEAF, transform_first) for s, c in enumerate(few)]
        assert [st for st, _ in want5] == [0, 0, 1, 2, 0]
        first = assert_run(mr, few, ori[:5], opm[:5], want5, transform_first, ("before",))
        grown = assert_run(mr, ids, ori, opm, many["want"][transform_first], transform_first, ("grown",))
        third = assert_run(mr, few, ori[:5], opm[:5], want5, transform_first, ("after",))
        alone = fresh.refine(ids, ori, opm, mi.RUN_LEAF, transform_first)
        assert all(same(a, b) for a, b in zip(first, third)) and all(same(a, b) for a, b in zip(grown, alone))
        assert np.array_equal(mr.status, [st for st, _ in want5])
    mr.close()
    fresh.close()


def test_selections_of_one_two_and_four_chunks(many):
    mr, store, ids, ori, opm = (many[k] for k in ("mr", "store", "ids", "ori", "opm"))
    at = sorted(mi.MANY_CHUNK_AT)                                        # the selections that hold the 2048-, 2049- and 4096-point clouds
    mi.packed_voxel_is_one_point(store)                                  # from the oracle: the voxel across the work-item bound is one point
    for transform_first in (False, True):
        want = many["want"][transform_first]
        for s in at:
            assert want[s][0] == 0 and 0 < len(want[s][1]) <= len(store[ids[s]])
            assert_run(mr, [ids[s]], ori[s:s + 1], opm[s:s + 1], [want[s]], transform_first, ("alone",))
            assert mr.work()[3] == len(store[ids[s]])
        assert_run(mr, [ids[s] for s in at], ori[at], opm[at], [want[s] for s in at], transform_first, ("together",))


@pytest.mark.parametrize("cnt", [1, 7, 8, 9, 16])
def test_last_voxel_ends_at_the_last_key(gpu_lib, cnt):
    """mr_centroid reads keys eight at a time up to `total`: here the last voxel's cnt keys are the last keys of the chain"""
    store = mi.last_voxel_at_the_end(cnt)
    n_finite = sum(mi.finite_count(c) for c in store)
    assert n_finite == sum(len(c) for c in store) and all(len(c) > 0 for c in store)     # no point is a sentinel ...
    mr = stored(store, initial_points=1 << 10)
    for ori, opm in (mi.poses(2, 89), (np.stack([mi.IDENTITY] * 2),) * 2):
        want = mi.expected_run(store, [0, 1], ori, opm)
        assert all(st == 0 for tf in want for st, _ in want[tf])                        # ... and no selection is empty or handed back
        for transform_first in (False, True):
            assert_run(mr, [0, 1], ori, opm, want[transform_first], transform_first, (cnt,))
            assert mr.work()[3] == n_finite
    packed = mi.in_voxel(store[1], mi.LAST_VOXEL_AT)
    for transform_first in (False, True):                               # under the identity pair the last output row is the packed voxel
        last = want[transform_first][1][1][-1:]
        assert packed.sum() == cnt and mi.in_voxel(last, mi.LAST_VOXEL_AT).all()
        assert np.array_equal(bits(last[:, :3]), bits(mi.filtered(store[1][packed], mi.RUN_LEAF)[1][:, :3]))
    mr.close()


def test_add_cloud_hands_back_non_finite_rows_and_a_run_filters_them(gpu_lib):
    rng = np.random.default_rng(97)
    cloud = rng.uniform(-15, 15, (60, 4)).astype(np.float32)
    cloud[0, :3], cloud[1, :3] = -15.0, 15.0                             # a 30 m extent: 30001^3 > 2^31 leaves of 1 mm
    bad = np.arange(60) % 7 == 3
    cloud[bad, rng.integers(0, 3, int(bad.sum()))] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    assert 0 < mi.finite_count(cloud) < 60 and mi.filtered(cloud, 0.001)[0] == 1
    mr = Map_refine(initial_points=1 << 10)
    assert mr.add_cloud(np.ones((5, 4), np.float32), mi.ADD_LEAF) == (0, 1, 0)
    assert mr.add_cloud(cloud, 0.001) == (1, 60, 1)
    assert same(mr.cloud(1), cloud)
    ori, opm = mi.poses(2, 101)
    want = mi.expected_run([np.ones((1, 4), np.float32), cloud], [1, 0], ori, opm)
    for transform_first in (False, True):
        assert want[transform_first][0][0] == 0 and 0 < len(want[transform_first][0][1]) <= mi.finite_count(cloud)
        assert_run(mr, [1, 0], ori, opm, want[transform_first], transform_first)
    mr.close()


def test_assembly_end_to_end(gpu_lib):
    """Keyframe_assembly( pose_graph=True, map_refinement=True ) on the device -- the full cell map, the key frames' analysis, the pose
    graph and the refinement are the real ones: a sensor walks out along a line and its scans are accumulated into overlapping key frames;
    an accepted loop between the last and the first key frame is closed.  refined holds ids K - 1, K - 3, ...; every cloud equals the
    FIFO rule replayed here, then the oracle's VoxelGrid at 0.5 and at 0.2, then the numpy move with the assembly's own poses_ori /
    poses_opm; loops, log and state() equal those of the same walk with map_refinement=False.
    (The out-and-back scenario of tests/test_keyframes.py closes a key frame every time it opens one, scans_of_each_keyframe =
    scans_between_two_keyframe: there the open list runs empty, no key frame is ever the back one at :1545, and nothing is accumulated;
    the walk here keeps two key frames open.)"""
    from loam_livox_amd.keyframes import Keyframe_assembly
    each, between, history, n_scans = 12, 6, 4, 60
    rng = np.random.default_rng(61)
    scans, poses, added = [], [], rng.random(n_scans) < 0.75
    for k in range(n_scans):
        pose = np.array([0, 0, np.sin(0.01 * k), np.cos(0.01 * k), 0.5 * k, 0.1 * k, 0.0])
        p = rng.uniform(-15, 15, (1500, 4)).astype(np.float32)
        p[:, 2] /= 30.0                                                    # (a slab a metre thick: cells that a scan fills with three points and more)
        p[:, :3] += pose[4:].astype(np.float32)
        scans.append(p)
        poses.append(pose)
    outcome = {}
    for on in (False, True):
        ka = Keyframe_assembly(scans_of_each_keyframe=each, scans_between_two_keyframe=between, maximum_history_size=history,
                               minimum_keyframe_differen=10 ** 6, max_points=1 << 18, pose_graph=True, map_refinement=on)
        for k in range(n_scans):
            ka.add_scan(scans[k], poses[k], k + 1, history_added=bool(added[k]))
            ka.process_waiting()
        K = len(ka.keyframe_vec)
        loop = dict(his=0, last=K - 1, inlier_threshold=0.1, icp_q=np.array([0, 0, np.sin(0.002), np.cos(0.002)]), icp_t=np.array([0.3, -0.2, 0.05]))
        ka.close_loop(loop)
        outcome[on] = (ka.state(), list(ka.log), list(ka.loops), ka.if_end, K, ka.poses_opm.copy())
        if on:
            refined, ori, opm = ka.refined, ka.poses_ori.copy(), ka.poses_opm.copy()
            assert ka.refined_mapping().shape[1] == 4
        else:
            assert ka.refined is None
        ka.close()
    assert outcome[True][:5] == outcome[False][:5] and np.array_equal(outcome[True][5], outcome[False][5])
    K = outcome[True][4]
    assert K == (n_scans - each) // between + 1 and [i for i, _ in refined] == list(range(K - 1, -1, -2))
    assert not np.array_equal(ori, opm)
    # the FIFO rule, replayed: key frame j is the back one when scan 6 ( j + 1 ) - 1 has been added, and takes what the FIFO holds then
    fifo, acc = [], []
    for k in range(n_scans):
        if added[k]:
            fifo.append(k)
        if len(fifo) > history:
            fifo.pop(0)
        if (k + 1) % between == 0:
            acc.append(fifo)
            fifo = []
    for pc_idx, cloud in refined:
        raw = np.concatenate([scans[k] for k in acc[pc_idx]]) if acc[pc_idx] else np.zeros((0, 4), np.float32)
        stored = mi.filtered(raw, 0.5)[1]
        st, want = mi.expected(stored, ori[pc_idx], opm[pc_idx], 0.2, False)
        assert same(cloud, want), pc_idx
    assert sum(len(c) for _, c in refined) > 5000


def test_mapping_loop_refines_the_map_when_its_detector_accepts_a_loop(gpu_lib):
    """Laser_mapping( loop_closure = dict( pose_graph=True, map_refinement=True ) ) end to end, with nothing stubbed: the history's add
    rule rejects scans (history_add_t_step and history_add_angle_step above the steps of the walk, once the history is full), the mapping loop hands that answer and
    its maximum_history_size to the assembly, key frames close and are processed, the DETECTOR accepts a loop between two key frames
    of the one place (process_waiting -> close_loop -> refine_map).  Every stored cloud equals the FIFO rule replayed over what add_scan
    was given, through the oracle's 0.5 m VoxelGrid; refined holds K - 1, K - 3, ... and equals the oracle at 0.2 m composed with the
    numpy move under the assembly's poses; poses, loops, log and state() equal those of the same run with map_refinement off."""
    from loam_livox_amd import synth
    from loam_livox_amd.mapping import Laser_mapping
    from tests.test_mapping_sequence import MAP_ARGS, N_PTS, make_sequence
    world = synth.world_for_map_size(200_000)
    scans, _ = make_sequence(world, n_frames=26)
    # out and back over the same scans: on the way out every newer key frame holds FEWER cells than the older ones (121, 120, 107, 102,
    # 92 were counted), and the detector skips such a pair (:1030); the key frames of the way back grow again and meet their places
    scans = scans + scans[-2::-1]
    each, between = 8, 4
    outcome = {}
    for on in (False, True):
        lc = dict(scans_of_each_keyframe=each, scans_between_two_keyframe=between, maximum_keyframe_in_waiting_list=3, minimum_keyframe_differen=1,
                  max_points=1 << 18, avail_ratio_plane=0.0, avail_ratio_line=0.0, map_alignment_maximum_icp_iteration=2, minimum_similarity_linear=0.4,
                  minimum_similarity_planar=0.5, pose_graph=True, map_refinement=on)   # (8 scans per key frame: emptier images than the node's 300)
        lm = Laser_mapping(scan_points=N_PTS, loop_closure_if_enable=1, loop_closure=lc, history_add_t_step=0.1, history_add_angle_step=0.05, **MAP_ARGS)
        ka, given = lm.keyframes, []
        inner = ka.add_scan

        def spy(cloud, pose, index, history_added=True, inner=inner, given=given):
            given.append((np.array(cloud, np.float32), bool(history_added)))
            return inner(cloud, pose, index, history_added=history_added)
        ka.add_scan = spy
        for xyzi in scans:
            lm.process_new_scan(xyzi)
        log = [{k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in ka.log + ka.loops]
        outcome[on] = (ka.state(), log, ka.if_end, len(ka.keyframe_vec), lm.pose.copy(), None if ka.poses_opm is None else ka.poses_opm.copy())
        if on:
            assert ka.m_maximum_history_size == MAP_ARGS["maximum_history_size"]
            flags = [a for _, a in given]
            assert 3 < sum(flags) < len(flags) - 3, flags                           # the add rule let some scans in and kept some out
            fifo, acc = [], []
            for k, (cloud, added) in enumerate(given):                              # the FIFO rule over what add_scan was given
                if added:
                    fifo.append(cloud)
                if len(fifo) > MAP_ARGS["maximum_history_size"]:
                    fifo.pop(0)
                if (k + 1) % between == 0:
                    acc.append(np.concatenate(fifo) if fifo else np.zeros((0, 4), np.float32))
                    fifo = []
            K = len(ka.keyframe_vec)
            store = ka.rounds.map_refine()
            stored = [mi.filtered(acc[j], 0.5)[1] for j in range(K)]
            for j, kf in enumerate(ka.keyframe_vec):
                assert kf.cloud_id == j and same(store.cloud(j), stored[j]), j
            assert len(ka.loops) >= 1 and ka.if_end and ka.poses_opm is not None, ([len(kf.m_set_cell) for kf in ka.keyframe_vec], [(r["last"], r["his"], round(r.get("sim_line", -1), 2), round(r.get("sim_plane", -1), 2), r.get("inlier_threshold")) for r in ka.log])   # the detector accepted a loop
            assert [i for i, _ in ka.refined] == list(range(K - 1, -1, -2)) and len(ka.poses_ori) == K
            for pc_idx, cloud in ka.refined:
                assert same(cloud, mi.expected(stored[pc_idx], ka.poses_ori[pc_idx], ka.poses_opm[pc_idx], 0.2, False)[1]), pc_idx
            # (a key frame of this walk covers about a hundred 1 m cells, and a 0.2 m voxel lies inside one: a refined cloud of a
            #  key frame that was given any scan holds points by the hundred, not by the thousand)
            assert sum(len(c) for _, c in ka.refined) > 100 and sum(len(c) > 0 for _, c in ka.refined) >= 2
        lm.close()
    a, b = outcome[False], outcome[True]
    assert a[:4] == b[:4] and np.array_equal(a[4], b[4]) and np.array_equal(a[5], b[5])
