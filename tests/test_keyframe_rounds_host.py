"""CPU tier of keyframes.Keyframe_rounds, the one driver of a key-frame round, over stubs only (no device, no library).

Every valid combination of its services at once -- bank x pose graph x map refinement, map refinement only with the pose graph: six --
on three scripted sequences: the driver over three assemblies gives what three assemblies give that each run their own
process_waiting, and makes at most one call of each shared service per round.  A failing extraction and a failing solve leave no
half-round behind."""
import numpy as np
import pytest

from loam_livox_amd import keyframes as kfm
from tests import test_keyframe_bank_host as kb
from tests.test_keyframes_accumulate import StubRefine
from tests.test_pose_graph_host import StubPoseGraph, key_frame_poses

S, MIN_DIFF = 3, 2
SEEDS = (2, 3, 2)          # slots 0 and 2 walk the same script and accept their loop in the same round; slot 1 never accepts one
COMBINATIONS = [(bank, pose_graph, refine) for bank in (False, True) for pose_graph, refine in ((False, False), (True, False), (True, True))]


class Batch:
    """stands in for the History_buffer_batch: the store the key frames' cells come out of, and the owner of the scan log"""

    def __init__(self, events, fail=False):
        self.events, self.fail = events, fail

    def extract_cells(self, kind, sequences, cell_lists, dsts):
        assert kind == 2 and len(sequences) == len(cell_lists) == len(dsts) > 0
        self.events.append(("extract", list(sequences), list(dsts)))
        if self.fail:
            raise RuntimeError("extraction failed")


class LogSlot:
    def __init__(self, batch):
        self.batch = batch

    def drop(self, ids):
        pass


class Refine(StubRefine):
    """... with the scan-log route: a key frame's stored cloud carries its group ids"""

    def __init__(self, events):
        super().__init__()
        self.events = events

    def add_logged(self, batch, groups_per_request, leaf=0.5):
        self.events.append(("add_logged", len(groups_per_request)))
        first = len(self.clouds)
        for groups in groups_per_request:
            self.add_cloud(np.array([[g, 0, 0, g] for g in groups], np.float32).reshape(-1, 4), leaf)
        n = len(groups_per_request)
        return np.arange(first, first + n), np.ones(n, np.int64), np.zeros(n, np.int32)

    def refine(self, ids, poses_ori, poses_opm, leaf=0.2, transform_first=False):
        self.events.append(("refine", len(ids)))
        return super().refine(ids, poses_ori, poses_opm, leaf, transform_first)


class Bank(kb.StubBank):
    def __init__(self, events):
        super().__init__()
        self.events = events

    def match(self, ids_a, ids_b):
        self.events.append(("match", len(ids_a)))
        return super().match(ids_a, ids_b)


class Solver(StubPoseGraph):
    def __init__(self, events, fail=0):
        super().__init__()
        self.events, self.fail = events, fail

    def solve(self, graphs):
        self.events.append(("solve", len(graphs)))
        if self.fail:
            self.fail -= 1
            raise RuntimeError("solve failed")
        return super().solve(graphs)


def assemblies(monkeypatch, scripts, events, batch, bank, pose_graph, refine, shared):
    """three stub assemblies with the services named: one handle of each for all (shared) or one per assembly"""
    out = []
    for sc in scripts:
        if not out or not shared:
            handles = dict(bank=Bank(events) if bank else None, pose_graph=Solver(events) if pose_graph else False,
                           map_refinement=Refine(events) if refine else False)
        ka = kb.stub_assembly(monkeypatch, sc, MIN_DIFF, [], scan_log=LogSlot(batch) if refine else None, **handles)
        ka.handles = handles

        def walk(sims=None, _ka=ka, _real=ka.walk_front):      # without a bank the walk asks the module's function: this assembly's script
            monkeypatch.setattr(kfm, "keyframe_similarity", _ka.similarity)
            return _real(sims)
        ka.walk_front = walk
        out.append(ka)
    return out


def waiting_keyframe(sc, s, k, poses):
    kf = kb.waiting_keyframe(sc, k)
    kf.m_pose_q, kf.m_pose_t = poses[k][:4].copy(), poses[k][4:7].copy()
    kf.m_accumulated_point_cloud = [1000 * s + 2 * k, 1000 * s + 2 * k + 1]     # its groups in the scan log (read with map refinement alone)
    return kf


def plain(records):
    return [{key: (v.tolist() if isinstance(v, np.ndarray) else v) for key, v in r.items()} for r in records]


@pytest.fixture(scope="module")
def world():
    """the scripts and key-frame poses of the three slots -- made once, shared, not changed"""
    return [kb.script(seed) for seed in SEEDS], [key_frame_poses(seed, kb.K) for seed in (12, 13, 14)]


@pytest.mark.parametrize("bank,pose_graph,refine", COMBINATIONS)
def test_driver_over_three_assemblies_equals_three_assemblies_run_alone(monkeypatch, world, bank, pose_graph, refine):
    scripts, poses = world
    ev_alone, ev = [], []
    alone = assemblies(monkeypatch, scripts, ev_alone, Batch(ev_alone), bank, pose_graph, refine, shared=False)
    batch = Batch(ev)
    slots = assemblies(monkeypatch, scripts, ev, batch, bank, pose_graph, refine, shared=True)
    rounds = kfm.Keyframe_rounds(slots, store=batch, **slots[0].handles)
    assert all(ka.rounds is rounds for ka in slots) and all(ka.rounds is not rounds and ka.rounds.assemblies == [ka] for ka in alone)
    found_alone, found = [[] for _ in range(S)], [[] for _ in range(S)]
    rounds_of_step_7 = None
    for k in range(kb.K):
        nxt = [len(a.keyframe_vec) + len(a.m_keyframe_need_precession_list) for a in alone]
        for s in range(S):
            for j in range(2 if (k == 7 and s == 1) else 1):                       # slot 1 closes two key frames in one step
                if nxt[s] + j < kb.K:
                    for ka in (alone[s], slots[s]):
                        ka.m_keyframe_need_precession_list.append(waiting_keyframe(scripts[s], s, nxt[s] + j, poses[s]))
        for s in range(S):
            found_alone[s] += alone[s].process_waiting()
        at = len(ev)
        for s, loops in enumerate(rounds.run(list(range(S)))):
            found[s] += loops
        if k == 7:
            rounds_of_step_7 = sum(e[0] == "extract" for e in ev[at:])
    assert rounds_of_step_7 == 2
    for s in range(S):
        g, w = slots[s], alone[s]
        assert kb.outcome(g) == kb.outcome(w) and plain(g.log) == plain(w.log) and plain(g.loops) == plain(w.loops), s
        assert plain(found[s]) == plain(found_alone[s]) == plain(w.loops), s
        assert (g.poses_opm is None) == (w.poses_opm is None) == (not (pose_graph and w.loops)), s
        if g.poses_opm is not None:
            assert g.poses_opm.tobytes() == w.poses_opm.tobytes() and g.poses_ori.tobytes() == w.poses_ori.tobytes(), s
        assert (g.refined is None) == (w.refined is None) == (not (refine and w.loops)), s
        if g.refined is not None:
            assert [i for i, _ in g.refined] == [i for i, _ in w.refined] == list(range(len(g.poses_ori) - 1, -1, -2)), s
            assert all(np.array_equal(a, b) and len(a) == 2 for (_, a), (_, b) in zip(g.refined, w.refined)), s
        if refine:          # every processed key frame's stored cloud, whatever id the shared store gave it
            assert all(np.array_equal(g.handles["map_refinement"].clouds[a.cloud_id], w.handles["map_refinement"].clouds[b.cloud_id])
                       and a.m_accumulated_point_cloud == [] for a, b in zip(g.keyframe_vec, w.keyframe_vec)), s
        assert not g.pending_loops and not w.pending_loops
    assert [bool(a.loops) for a in alone] == [True, False, True] and [a.if_end for a in alone] == [True, False, True]
    assert len(alone[1].keyframe_vec) == kb.K
    # a round begins with its one extraction; behind it at most one call of each shared service
    cuts = [i for i, e in enumerate(ev) if e[0] == "extract"] + [len(ev)]
    assert cuts[0] == 0
    for a, b in zip(cuts, cuts[1:]):
        names = [e[0] for e in ev[a + 1:b]]
        assert all(names.count(n) <= 1 for n in ("match", "add_logged", "solve", "refine")), names
        assert names.count("add_logged") == int(refine) and (not refine or ev[a + 1:b][names.index("add_logged")][1] == len(ev[a][1]))
    # slots 0 and 2 accepted their loops in the same round: ONE solve of two graphs and ONE refine of both selections
    assert [e for e in ev if e[0] == "solve"] == ([("solve", 2)] if pose_graph else [])
    assert [e for e in ev if e[0] == "refine"] == ([("refine", 2 * len(slots[0].refined))] if refine else [])
    assert [e[1] for e in ev_alone if e[0] == "solve"] == ([1, 1] if pose_graph else [])
    if bank:
        assert max(e[1] for e in ev if e[0] == "match") > max(e[1] for e in ev_alone if e[0] == "match")   # a match carries several slots' pairs


class Destination:
    def __init__(self, made):
        self.closed = 0
        made.append(self)

    def close(self):
        self.closed += 1


def test_a_failing_extraction_closes_its_destinations_and_leaves_the_key_frames_waiting(monkeypatch, world):
    scripts, poses = world
    ev, made = [], []
    batch = Batch(ev, fail=True)
    slots = assemblies(monkeypatch, scripts, ev, batch, True, True, True, shared=True)
    rounds = kfm.Keyframe_rounds(slots, store=batch, **slots[0].handles)
    for s, ka in enumerate(slots):
        ka.new_keyframe_map = lambda n_cells: Destination(made)
        for k in range(2 if s == 1 else 1):
            ka.m_keyframe_need_precession_list.append(waiting_keyframe(scripts[s], s, k, poses[s]))
    before = [list(ka.m_keyframe_need_precession_list) for ka in slots]
    with pytest.raises(RuntimeError, match="extraction failed"):
        rounds.run([0, 1, 2])
    assert len(made) == 3 and ev == [("extract", [0, 1, 2], made)] and all(d.closed == 1 for d in made)
    assert [list(ka.m_keyframe_need_precession_list) for ka in slots] == before
    assert all(not ka.keyframe_vec and not ka.log and ka._front is None and ka._prefetched is None for ka in slots)
    assert not slots[0].handles["bank"].entries and not slots[0].handles["map_refinement"].clouds      # no service was reached


def test_a_failing_solve_keeps_the_accepted_loops_for_the_next_run(monkeypatch, world):
    """What the lock-step loop did before the driver (read from Laser_mapping_batch._close_loops and the first pass of
    _process_keyframes, which ran for slots with nothing waiting): a solve that raises leaves the round's accepted loops in
    pending_loops -- logged, in `loops`, if_end set -- and the next run solves them again: it closes them, or raises again and still
    holds them.  An accepted loop is never dropped."""
    scripts, poses = world
    ev = []
    batch = Batch(ev)
    slots = assemblies(monkeypatch, scripts, ev, batch, True, True, True, shared=True)
    solver = slots[0].handles["pose_graph"]
    rounds = kfm.Keyframe_rounds(slots, store=batch, **slots[0].handles)
    solver.fail = 2
    failed_at = None
    for k in range(kb.K):
        for s in (0, 2):
            slots[s].m_keyframe_need_precession_list.append(waiting_keyframe(scripts[s], s, k, poses[s]))
        try:
            rounds.run([0, 2])
        except RuntimeError as e:
            assert str(e) == "solve failed"
            failed_at = k
            break
    assert failed_at == kb.K - 5

    def held():
        return all(len(ka.loops) == 1 and ka.pending_loops == ka.loops and ka.if_end and ka.poses_opm is None and ka.refined is None for ka in (slots[0], slots[2]))
    assert held() and [e for e in ev if e[0] == "refine"] == []
    with pytest.raises(RuntimeError, match="solve failed"):       # raises again: the loops are still held
        rounds.run([0, 2])
    assert held() and [e for e in ev if e[0] == "solve"] == [("solve", 2), ("solve", 2)]
    extractions = sum(e[0] == "extract" for e in ev)
    assert rounds.run([0, 2]) == [[], []]                          # closes them: nothing new is found, nothing is extracted or analysed
    assert sum(e[0] == "extract" for e in ev) == extractions and ev[-2:] == [("solve", 2), ("refine", 2 * len(slots[0].refined))]
    for ka in (slots[0], slots[2]):
        assert not ka.pending_loops and len(ka.loops) == 1 and ka.poses_opm is not None and [i for i, _ in ka.refined][0] == len(ka.keyframe_vec) - 1
    assert rounds.run([0, 2]) == [[], []] and len(solver.calls) == 1
