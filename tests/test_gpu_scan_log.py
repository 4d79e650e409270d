"""-m gpu: the scan log of the batched match buffer (ll_history_batch_enable_scan_log .. _scan_log_work, api.History_buffer_batch.log_full /
hand_over / drop_groups / read_group), the device-to-device add into the refine store (ll_map_refine_add_logged, api.Map_refine.add_logged)
and the lock-step loop with loop_closure map_refinement on top of them.

Every yardstick is the per-sequence route: pointcloudAssociateToMap( scan[full_idx], pose ) through the host, as
Laser_mapping._keyframe_step makes it, under the FIFO rule of laser_mapping.hpp:1456, 1480-1486, 1545-1558 replayed in numpy; a second
Map_refine fed by add_cloud; Laser_mapping(loop_closure_if_enable=1) run alone.  The log copies floats and the filter is fp32 work in a
fixed order, so every comparison is equality of bits.  The step sequence is the CPU tier's (tests/test_scan_log_host.py): full selections
of 300, 257, 256, 1 and 0 points, an idle slot, two scans the add rule kept out, a hand-over every four steps, one group dropped."""
import numpy as np
import pytest

from loam_livox_amd import synth
from loam_livox_amd.capi import LoamLivoxError
from tests.test_gpu_multimap import MAP_ARGS, N_PTS, report_tuple
from tests.test_scan_log_host import HISTORY, SIZES, T

pytestmark = pytest.mark.gpu

CELL_RES, THR = 1.0, 5000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cropped(gpu_lib, small_world):
    """target size -> a scan whose full selection holds exactly that many points (a real scan cut short), and a pose per step"""
    from loam_livox_amd.api import Livox_laser
    scans, poses = synth.make_livox_sequence(small_world["world"], 77)
    fe = Livox_laser(max_points=N_PTS, max_scans=1, piecewise_number=1)
    out = {}
    for k, n in enumerate(x for x in SIZES if x >= 0):
        scan, m = np.ascontiguousarray(scans[k % len(scans)], np.float32), n
        for _ in range(30):
            fe.upload(scan[:m][None], np.ones(1))
            fe.extract_batch(1)
            fe.resolve()
            fe.select_batch(1, -1, 0.0, 1.0)
            got = len(fe.get_features(0.0, 1.0, scan=0)["full_idx"])
            if got == n:
                break
            m += n - got
        assert got == n, (n, got)
        out[n] = scan[:m].copy()
    fe.close()
    return out, [np.array(p, np.float64) for p in poses]


class Rig:
    def __init__(self, S, initial_scans):
        from loam_livox_amd.api import History_buffer_batch, Livox_laser, Point_cloud_registration
        self.S = S
        self.fe = Livox_laser(max_points=N_PTS, max_scans=S, piecewise_number=1)
        self.reg = Point_cloud_registration(max_scans=1, max_features=N_PTS)
        self.hb = History_buffer_batch(S, MAP_ARGS["maximum_history_size"], N_PTS, MAP_ARGS["line_res"], MAP_ARGS["plane_res"])
        self.hb.enable_full_maps(N_PTS, CELL_RES, THR)
        self.hb.enable_scan_log(HISTORY, initial_scans)
        self.fifo = [[] for _ in range(S)]     # the FIFO rule, replayed over the host route's clouds
        self.markers = 0

    def close(self):
        for h in (self.fe, self.reg, self.hb):
            h.close()

    def step(self, scans, poses, named):
        """scans[s]: (n, 4) or None (idle); named[s]: the add rule let the scan in.  append_full, log_full, and the host route's FIFO."""
        S = self.S
        on = np.array([x is not None for x in scans])
        for s in range(S):
            self.fe.upload((scans[s] if on[s] else np.zeros((0, 4), np.float32))[None], np.ones(1), first_scan=s)
        self.fe.extract_batch(S)
        self.fe.resolve()
        self.fe.select_batch(S, -1, 0.0, 1.0)
        self.hb.append_full(self.fe, poses, on, 3, lists=False)
        self.hb.log_full(self.fe, np.asarray(named, bool) & on)
        for s in range(S):
            if not on[s]:
                continue
            if named[s]:
                full = scans[s][self.fe.get_features(0.0, 1.0, scan=s)["full_idx"]]
                ok = np.isfinite(full[:, :3]).all(axis=1)   # (Laser_mapping._keyframe_step)
                self.markers += int((~ok).sum())
                full = full[ok]
                self.fifo[s].append(self.reg.pointcloudAssociateToMap(full, poses[s]) if len(full) else full.reshape(0, 4))
            if len(self.fifo[s]) > HISTORY:
                self.fifo[s].pop(0)

    def hand_over(self, s):
        gid, want = self.hb.hand_over(s), self.fifo[s]
        self.fifo[s] = []
        return gid, want


def cat(scans):
    return np.concatenate(scans) if scans else np.zeros((0, 4), np.float32)


def finite_rows(cloud):
    return cloud[np.isfinite(cloud[:, :3]).all(axis=1)]


def run_schedule(cropped, S, initial_scans):
    """the CPU tier's twelve steps on S slots -> (rig, [(group id, the host route's scans)] in hand-over order, work taps per step)"""
    scans_of, poses = cropped
    rig, groups, taps = Rig(S, initial_scans), [], []
    for t in range(T):
        sizes = [SIZES[(t + 2 * s) % len(SIZES)] for s in range(S)]
        named = [n >= 0 and not (t == 6 and s == 0) and not (t == 9 and s == 2) for s, n in enumerate(sizes)]
        pose = np.stack([poses[(t + s) % len(poses)] for s in range(S)])
        rig.step([scans_of[n] if n >= 0 else None for n in sizes], pose, named)
        taps.append(rig.hb.scan_log_work().tolist() + [max([n for n, a in zip(sizes, named) if a], default=0)])
        if t % 4 == 3:
            groups += [rig.hand_over(s) for s in range(S)]
        if t == 8 and S > 1:
            rig.hb.drop_groups([groups[1][0]])
            groups[1] = (groups[1][0], None)
    return rig, groups, taps


@pytest.fixture(scope="module")
def runs(cropped):
    """(S, initial_scans) -> (rig, groups, taps, every live group read back), made once and shared"""
    made = {}

    def get(S, initial_scans):
        key = (S, initial_scans)
        if key not in made:
            rig, groups, taps = run_schedule(cropped, S, initial_scans)
            made[key] = (rig, groups, taps, [None if want is None else rig.hb.read_group(gid) for gid, want in groups])
        return made[key]
    yield get
    for run in made.values():
        run[0].close()


def test_groups_equal_the_fifo_rule_over_the_host_route(gpu_lib, runs):
    rig, groups, taps, read = runs(3, 64)
    assert len(groups) == 9
    n_markers = 0
    for k, ((gid, want), got) in enumerate(zip(groups, read)):
        if want is None:
            with pytest.raises(LoamLivoxError, match="unknown or consumed"):
                rig.hb.read_group(gid)
            continue
        assert len(want) <= HISTORY
        n_markers += len(got) - len(finite_rows(got))
        assert np.array_equal(bits(finite_rows(got)), bits(cat(want))), (k, "group in bits")
    assert max(len(w) for _, w in groups if w is not None) == HISTORY              # a FIFO was trimmed
    assert n_markers <= rig.markers                                               # (markers of scans that were trimmed away are gone)
    assert any(np.any(cat(w)[:, 3] != 0) for _, w in groups if w)                  # the intensity is the scan's, not the gather's 0
    # blocks in use: what the FIFOs hold (nothing after the last hand-over) and the live groups
    assert rig.hb.scan_log_work()[2] == sum(len(w) for _, w in groups if w is not None)


def test_a_log_call_is_four_enqueues_and_no_wait_for_one_slot_and_for_three(gpu_lib, runs):
    three, one = runs(3, 64)[2], runs(1, 64)[2]
    for taps in (three, one):
        for enq, waits, _, _, max_n in taps:
            assert waits == 0 and enq == (4 if max_n > 0 else 0), taps
    assert {t[0] for t in three} == {4} and {t[0] for t in one} == {0, 4}          # (one slot alone meets its empty and its idle step)


def test_growth_by_chunks_gives_the_groups_of_a_handle_created_large(gpu_lib, runs):
    small, large = runs(3, 2), runs(3, 64)
    assert small[2][-1][3] > 2 and small[2][-1][3] % 2 == 0 and large[2][-1][3] == 64   # it grew, by chunks of two; the large one never did
    assert [t[2] for t in small[2]] == [t[2] for t in large[2]]                    # blocks in use, step by step
    for a, b in zip(small[3], large[3]):
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())


def test_add_logged_equals_add_cloud_of_the_host_concatenation(gpu_lib, runs):
    from loam_livox_amd.api import Map_refine
    rig, groups, _, _ = runs(3, 16)   # (a run of its own: its groups are consumed here)
    live = [k for k, (_, w) in enumerate(groups) if w is not None]
    one, two = [live[0]], [live[1], live[2]]
    empty_gid = rig.hb.hand_over(0)                                                # the FIFO was handed over at the last step: an empty group
    assert len(rig.hb.read_group(empty_gid)) == 0
    requests = [[groups[k][0] for k in one], [groups[k][0] for k in two], [empty_gid]]
    wants = [cat([sc for k in one for sc in groups[k][1]]), cat([sc for k in two for sc in groups[k][1]]), np.zeros((0, 4), np.float32)]
    assert len(wants[0]) > 0 and len(wants[1]) > 0
    mr, ref = Map_refine(1 << 12), Map_refine(1 << 12)                             # (small: the store grows inside the call)
    ref.add_cloud(np.ones((5, 4), np.float32), 0.5)
    mr.add_cloud(np.ones((5, 4), np.float32), 0.5)                                 # a cloud in the store already: the ids go on behind it
    in_use = int(rig.hb.scan_log_work()[2])
    ids, kept, status = mr.add_logged(rig.hb, requests, 0.5)
    work3 = mr.work().tolist()
    for r, w in enumerate(wants):
        cid, n_kept, st = ref.add_cloud(w, 0.5)
        assert (int(ids[r]), int(kept[r]), int(status[r])) == (cid, n_kept, st), r
        assert np.array_equal(bits(mr.cloud(int(ids[r]))), bits(ref.cloud(cid))), (r, "stored cloud in bits")
    assert ids.tolist() == [1, 2, 3] and kept[0] > 0 and kept[1] > 0 and kept[2] == 0 and len(mr) == 4
    assert work3[1] == 1                                                           # one host wait whatever n_req is
    # the groups are gone, their blocks free
    assert rig.hb.scan_log_work()[2] == in_use - sum(len(groups[k][1]) for k in one + two)
    for gid in [g for r in requests for g in r]:
        with pytest.raises(LoamLivoxError, match="unknown or consumed"):
            rig.hb.read_group(gid)
    # one request: the same number of enqueue calls, one wait
    k = live[3]
    ids1, _, _ = mr.add_logged(rig.hb, [[groups[k][0]]], 0.5)
    work1 = mr.work().tolist()
    assert work1[:2] == work3[:2] and ids1.tolist() == [4]
    assert np.array_equal(bits(mr.cloud(4)), bits(ref.cloud(ref.add_cloud(cat(groups[k][1]), 0.5)[0])))
    mr.close()
    ref.close()


def test_add_logged_past_256_requests(gpu_lib, runs):
    """300 requests are 300 selections of one MR_FILTER_ONLY chain: mr_offsets_kernel makes two trips, and the requests that hold points
    sit at the chain's first and last selection and on both sides of the trip bound"""
    from loam_livox_amd.api import Map_refine
    rig, groups, _, _ = runs(3, 32)   # (a run of its own: its groups are consumed here)
    live = [k for k, (_, w) in enumerate(groups) if w is not None]
    named = {0: live[:1], 255: live[1:3], 256: live[3:4], 299: live[4:6]}
    requests = [[groups[k][0] for k in named.get(r, [])] for r in range(300)]
    wants = [cat([sc for k in named.get(r, []) for sc in groups[k][1]]) for r in range(300)]
    assert all(len(wants[r]) > 0 for r in named) and sum(len(w) > 0 for w in wants) == 4
    mr, ref = Map_refine(1 << 12), Map_refine(1 << 12)
    in_use = int(rig.hb.scan_log_work()[2])
    ids, kept, status = mr.add_logged(rig.hb, requests, 0.5)
    work = mr.work().tolist()
    assert ids.tolist() == list(range(300)) and len(mr) == 300
    for r, w in enumerate(wants):
        cid, n_kept, st = ref.add_cloud(w, 0.5)
        assert (int(ids[r]), int(kept[r]), int(status[r])) == (cid, n_kept, st), r
        assert (n_kept > 0 and st == 0) if r in named else (n_kept == 0 and st == 2), r
        assert np.array_equal(bits(mr.cloud(r)), bits(ref.cloud(cid))), (r, "stored cloud in bits")
    assert work[1] == 1                                                            # one host wait whatever n_req is
    assert rig.hb.scan_log_work()[2] == in_use - sum(len(groups[k][1]) for ks in named.values() for k in ks)
    mr.close()
    ref.close()


def test_refusals_leave_both_handles_usable(gpu_lib, cropped):
    from loam_livox_amd.api import History_buffer, History_buffer_batch, Map_refine
    scans_of, poses = cropped
    rig = Rig(2, 4)
    hb, mr = rig.hb, Map_refine(1 << 12)
    pose = np.stack([poses[0], poses[1]])
    with pytest.raises(LoamLivoxError, match="no ll_history_batch_append_full_fe to log"):   # a log without an append
        hb.log_full(rig.fe)
    rig.step([scans_of[300], scans_of[257]], pose, [True, True])
    with pytest.raises(LoamLivoxError, match="no ll_history_batch_append_full_fe to log"):   # a log twice
        hb.log_full(rig.fe)
    assert hb.scan_log_work()[2] == 2
    with pytest.raises(LoamLivoxError, match="already enabled"):
        hb.enable_scan_log(3, 4)
    with pytest.raises(LoamLivoxError, match="sequence out of range"):
        hb.hand_over(2)
    g0, want0 = rig.hand_over(0)
    g1, want1 = rig.hand_over(1)
    size = len(mr)
    for bad, words in (([[g0 + 1000]], "unknown or consumed"), ([[g0], [g0]], "named twice"), ([[g0, g1, g0]], "named twice")):
        with pytest.raises(LoamLivoxError, match=words):
            mr.add_logged(hb, bad, 0.5)
    with pytest.raises(LoamLivoxError, match="leaf"):
        mr.add_logged(hb, [[g0]], 0.0)
    with pytest.raises(LoamLivoxError, match="unknown or consumed"):
        hb.drop_groups([g0, 12345])
    assert len(mr) == size and hb.scan_log_work()[2] == 2                          # store and log untouched
    # a handle of the wrong kind: not a batched match buffer; a batched match buffer without a scan log
    single = History_buffer(3, N_PTS)
    with pytest.raises(TypeError):
        mr.add_logged(single, [[g0]], 0.5)
    single.close()
    bare = History_buffer_batch(2, 3, N_PTS)
    with pytest.raises(LoamLivoxError, match="not enabled"):
        mr.add_logged(bare, [[g0]], 0.5)
    with pytest.raises(LoamLivoxError, match="full maps are not enabled"):
        bare.enable_scan_log(3, 4)
    with pytest.raises(LoamLivoxError, match="not enabled"):
        bare.hand_over(0)
    bare.close()
    # both handles still work: the groups are there and go in; a consumed group is refused afterwards
    ids, _, _ = mr.add_logged(hb, [[g0], [g1]], 0.5)
    ref = Map_refine(1 << 12)
    for cid, want in zip(ids, (want0, want1)):
        assert np.array_equal(bits(mr.cloud(int(cid))), bits(ref.cloud(ref.add_cloud(cat(want), 0.5)[0])))
    with pytest.raises(LoamLivoxError, match="unknown or consumed"):
        mr.add_logged(hb, [[g0]], 0.5)
    assert hb.scan_log_work()[2] == 0
    rig.step([scans_of[1], None], pose, [True, True])
    assert hb.scan_log_work()[2] == 1
    for h in (mr, ref, rig):
        h.close()


def test_blocks_are_reused_over_forty_steps(gpu_lib, cropped):
    from loam_livox_amd.api import Map_refine
    scans_of, poses = cropped
    rig, mr = Rig(3, 3), Map_refine(1 << 12)
    allocated, pending = [], []
    for t in range(40):
        pose = np.stack([poses[(t + s) % len(poses)] for s in range(3)])
        rig.step([scans_of[300], scans_of[257], scans_of[256] if t % 5 else None], pose, [True, t % 3 != 1, True])
        if t % 4 == 3:
            got = [rig.hand_over(s)[0] for s in range(3)]
            if (t // 4) % 2:
                mr.add_logged(rig.hb, [got[:2], got[2:]], 0.5)                    # consumed ...
            else:
                rig.hb.drop_groups(got)                                           # ... or dropped
        work = rig.hb.scan_log_work()
        assert work[2] == sum(len(f) for f in rig.fifo), t                        # blocks in use = the FIFOs' sum
        allocated.append(int(work[3]))
    assert len(set(allocated[8:])) == 1 and allocated[-1] <= 3 * (HISTORY + 1) + 3  # no growth after the first cycle
    mr.close()
    rig.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_loop_with_map_refinement_equals_the_sequences_run_alone(gpu_lib):
    """S = 3, ragged by step - s % 3, on the out-and-back walk of tests/test_gpu_map_refine.py, on which the solo route closes a loop
    and its add rule lets some scans in and keeps some out (asserted on the solo side).  Every slot's stored clouds and `refined` are
    the solo run's in bits, the key frames are the solo run's, and poses and reports are those of the same batched run with
    map_refinement off."""
    from loam_livox_amd.mapping import Laser_mapping, Laser_mapping_batch
    from tests.test_gpu_fullmap_batch import assert_same_keyframes
    from tests.test_mapping_sequence import MAP_ARGS as SEQ_ARGS, N_PTS as SEQ_PTS, make_sequence
    world = synth.world_for_map_size(200_000)
    scans, _ = make_sequence(world, n_frames=26)
    scans = scans + scans[-2::-1]
    S, n = 3, len(scans)

    def settings(on):
        return dict(scans_of_each_keyframe=8, scans_between_two_keyframe=4, maximum_keyframe_in_waiting_list=3, minimum_keyframe_differen=1,
                    max_points=1 << 18, avail_ratio_plane=0.0, avail_ratio_line=0.0, map_alignment_maximum_icp_iteration=2, minimum_similarity_linear=0.4,
                    minimum_similarity_planar=0.5, pose_graph=True, map_refinement=on)
    common = dict(scan_points=SEQ_PTS, history_add_t_step=0.1, history_add_angle_step=0.05, **SEQ_ARGS)
    # the solo route (the three slots walk the same walk, shifted: one solo run is the yardstick of all of them)
    lm = Laser_mapping(loop_closure_if_enable=1, loop_closure=settings(True), **common)
    flags, inner = [], lm.keyframes.add_scan

    def spy(cloud, pose, index, history_added=True):
        flags.append(bool(history_added))
        return inner(cloud, pose, index, history_added=history_added)
    lm.keyframes.add_scan = spy
    for xyzi in scans:
        lm.process_new_scan(xyzi)
    solo = lm.keyframes
    assert len(solo.loops) >= 1 and solo.if_end and solo.refined is not None       # the solo route closes a loop
    assert 3 < sum(flags) < len(flags) - 3, flags                                  # the add rule let some scans in and kept some out
    lb = Laser_mapping_batch(S, batched_history=True, full_maps=True, key_frames=True, loop_closure=settings(True), **common)
    off = Laser_mapping_batch(S, batched_history=True, full_maps=True, key_frames=True, loop_closure=settings(False), **common)
    for step in range(n + 2):
        frame = [step - s % 3 for s in range(S)]
        batch = [scans[f] if 0 <= f < n else None for f in frame]
        out, out_off = lb.process_new_scans(batch), off.process_new_scans(batch)
        assert np.array_equal(out, out_off), step
        assert lb.poses.tobytes() == off.poses.tobytes(), (step, "poses")
        assert [None if r is None else report_tuple(r) for r in lb.last_reports] == [None if r is None else report_tuple(r) for r in off.last_reports], step
    store = solo.rounds.map_refine()
    for s in range(S):
        ka = lb.keyframes[s]
        assert_same_keyframes(ka, solo, s)
        assert_same_keyframes(off.keyframes[s], solo, (s, "off"))
        assert off.keyframes[s].refined is None and np.array_equal(ka.poses_opm, solo.poses_opm) and np.array_equal(ka.poses_opm, off.keyframes[s].poses_opm)
        assert len(ka.keyframe_vec) == len(solo.keyframe_vec)
        for j, (g, w) in enumerate(zip(ka.keyframe_vec, solo.keyframe_vec)):
            assert g.cloud_id is not None and g.m_accumulated_point_cloud == []
            assert np.array_equal(bits(lb.map_refine.cloud(g.cloud_id)), bits(store.cloud(w.cloud_id))), (s, j, "stored cloud")
        assert [i for i, _ in ka.refined] == [i for i, _ in solo.refined]
        for (i, g), (_, w) in zip(ka.refined, solo.refined):
            assert np.array_equal(bits(g), bits(w)), (s, i, "refined")
    assert sum(len(store.cloud(kf.cloud_id)) for kf in solo.keyframe_vec) > 100
    assert len({kf.cloud_id for ka in lb.keyframes for kf in ka.keyframe_vec}) == S * len(solo.keyframe_vec)   # one store, an id each
    merged = lb.keyframes[1].refined_mapping()                                     # refined_mapping() of an assembly keeps working
    assert np.array_equal(bits(merged), bits(solo.refined_mapping()))
    lb.close()
    off.close()
    lm.close()
