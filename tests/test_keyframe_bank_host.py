"""CPU tier of the key-frame descriptor bank (tests/test_gpu_keyframe_bank.py is the GPU tier).

Arithmetic: the tile body of loam_livox_amd/csrc/ll_keyframe_bank_core.h -- the text kb_corr_kernel runs -- compiled with g++
(tests/keyframe_bank_host.cpp) gives, bit for bit, the sums of the straight double loop of cm_kf_similarity_kernel's definition; the
maximum over 60 x 60 shifts is the maximum over 61 x 61; the similarity agrees with the oracle and, where it is built, with the
reference's own max_similiarity_of_two_image; the driver runs clean under the address and undefined-behaviour sanitizers.
Symbols: the new entry points are declared, exported and bound and refuse null handles and bad arguments without a device.
Bookkeeping: Keyframe_assembly( device_bank=True ) over a stub bank, on the scripted walks of tests/test_keyframes.py, gives the
state, log, loops and if_end of device_bank=False, asks for exactly the pairs that pass the three gates, once per processed key frame;
a Keyframe_rounds over stub assemblies and handles makes one match per round for all its slots."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from loam_livox_amd import capi
from tests.test_keyframes import ScriptedMap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = 3600
RECORD = 2 * BINS + 5


def build_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", os.path.join(ROOT, "loam_livox_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "keyframe_bank_host.cpp")])
    return exe


def run_driver(exe, tmp, pairs):
    """pairs: [(a, b)] of 60 x 60 float32 images -> per pair dict(tiled [60, 60], plain [60, 60], max60, max61, A, B, sim)"""
    pin, pout = os.path.join(tmp, "kb_in.bin"), os.path.join(tmp, "kb_out.bin")
    with open(pin, "wb") as f:
        f.write(np.int32(len(pairs)).tobytes())
        for a, b in pairs:
            f.write(np.ascontiguousarray(a, np.float32).tobytes() + np.ascontiguousarray(b, np.float32).tobytes())
    done = subprocess.run([exe, pin, pout], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert done.returncode == 0 and not done.stderr, done.stderr.decode(errors="replace")
    raw = np.fromfile(pout, np.float64).reshape(len(pairs), RECORD)
    return [dict(tiled=r[:BINS].reshape(60, 60), plain=r[BINS:2 * BINS].reshape(60, 60), max60=r[2 * BINS], max61=r[2 * BINS + 1],
                 A=r[2 * BINS + 2], B=r[2 * BINS + 3], sim=np.float32(r[2 * BINS + 4])) for r in raw]


def images():
    """name -> 60 x 60 float32: sparse positive images (as a blurred histogram is), one of both signs, single non-zero bins, zero, shifts"""
    rng = np.random.default_rng(11)
    out = {"r0": rng.uniform(0, 1, (60, 60)).astype(np.float32) ** 8, "r1": rng.uniform(0, 1, (60, 60)).astype(np.float32) ** 8,
           "signed": rng.normal(0, 1, (60, 60)).astype(np.float32), "zero": np.zeros((60, 60), np.float32)}
    for name, (i, j, v) in {"bin00": (0, 0, 3.0), "bin59_17": (59, 17, 0.7), "bin29_30": (29, 30, 1.0)}.items():
        out[name] = np.zeros((60, 60), np.float32)
        out[name][i, j] = v
    out["r0_shift_7_-20"] = np.roll(out["r0"], (7, -20), (0, 1))
    out["r0_shift_30_30"] = np.roll(out["r0"], (30, 30), (0, 1))
    return out


PAIRS = [("r0", "r1"), ("r1", "r0"), ("signed", "r0"), ("r0", "signed"), ("bin00", "bin59_17"), ("bin59_17", "bin29_30"), ("bin29_30", "r0"),
         ("r0", "bin00"), ("r0", "zero"), ("zero", "zero"), ("r0", "r0"), ("r0", "r0_shift_7_-20"), ("r0", "r0_shift_30_30")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(str(tmp_path_factory.mktemp("keyframe_bank") / "keyframe_bank_host"))


@pytest.fixture(scope="module")
def results(driver, tmp_path_factory):
    """the driver's record of every pair -- computed once, shared, not changed"""
    img = images()
    got = run_driver(driver, str(tmp_path_factory.mktemp("keyframe_bank_run")), [(img[a], img[b]) for a, b in PAIRS])
    return img, dict(zip(PAIRS, got))


def test_tiled_sums_equal_the_straight_sums_bit_for_bit(results):
    _, res = results
    for pair, r in res.items():
        assert np.array_equal(r["tiled"].view(np.uint64), r["plain"].view(np.uint64)), pair
    # a single bin against a single bin: exactly one shift sees the product, and it is where the definition puts it
    s = res[("bin00", "bin59_17")]["tiled"]
    assert np.count_nonzero(s) == 1 and s[(59 + 30) % 60, (17 + 30) % 60] == np.float64(np.float32(3.0)) * np.float64(np.float32(0.7))
    # ... and the sums are the definition's (in exact arithmetic: numpy's order differs)
    img, _ = results
    a, b = img["r0"].astype(np.float64), img["r1"].astype(np.float64)
    for Y, X in [(0, 0), (59, 59), (30, 30), (7, 41), (19, 20), (40, 39)]:
        want = (a * np.roll(b, (30 - Y, 30 - X), (0, 1))).sum()
        assert abs(res[("r0", "r1")]["tiled"][Y, X] - want) < 1e-9 * max(1.0, abs(want)), (Y, X)


def test_maximum_over_60x60_equals_the_maximum_over_61x61(results):
    for pair, r in results[1].items():
        assert np.float64(r["max60"]).tobytes() == np.float64(r["max61"]).tobytes(), pair
        assert r["max60"] == r["tiled"].max(), pair


def test_similarity_agrees_with_the_oracle(results):
    from oracle.orc_cellmap import CellMap
    img, res = results
    for (a, b), r in res.items():
        assert abs(float(r["sim"]) - CellMap.max_similarity(img[a], img[b])) < 1e-5, (a, b)     # the bound of tests/test_cellmap.py:423
        assert abs(r["A"] - (img[a].astype(np.float64) ** 2).sum()) <= 1e-12 * max(1.0, r["A"]), a


def test_similarity_agrees_with_the_reference_build(results):
    from oracle import ref_cells as rc
    if not rc.available():
        pytest.skip("oracle/_ref/libll_ref_cells.so is not built here")
    img, res = results
    for (a, b), r in res.items():
        assert abs(float(r["sim"]) - rc.max_similarity(img[a], img[b])) < 2e-6, (a, b)             # the bound of tests/test_ref_cells.py


def test_fixed_values(results):
    _, res = results
    assert res[("r0", "zero")]["sim"] == 0.0 and res[("zero", "zero")]["sim"] == 0.0
    ulp = 2.0 ** -23
    for pair in [("r0", "r0"), ("r0", "r0_shift_7_-20"), ("r0", "r0_shift_30_30")]:
        assert abs(float(res[pair]["sim"]) - 1.0) <= ulp, pair
    # roles matter only in the rounding: the same maximum, the norms exchanged
    ab, ba = res[("r0", "r1")], res[("r1", "r0")]
    assert ab["A"] == ba["B"] and ab["B"] == ba["A"] and abs(float(ab["sim"]) - float(ba["sim"])) <= ulp


def test_driver_runs_clean_under_the_sanitizers(tmp_path, results):
    img, res = results
    exe = build_driver(str(tmp_path / "keyframe_bank_host_san"), ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])
    pairs = [("signed", "r0"), ("bin59_17", "bin29_30")]
    got = run_driver(exe, str(tmp_path), [(img[a], img[b]) for a, b in pairs])      # (asserts exit status 0 and an empty stderr)
    for pair, r in zip(pairs, got):
        assert np.array_equal(r["tiled"].view(np.uint64), res[pair]["tiled"].view(np.uint64)) and r["sim"] == res[pair]["sim"]


# ------------------------------------------------------------------------------------------------ entry points without a device
NEW = {"ll_keyframe_bank_create": 3, "ll_keyframe_bank_destroy": 1, "ll_keyframe_bank_add_cellmap": 9, "ll_keyframe_bank_add_images": 4,
       "ll_keyframe_bank_images": 4, "ll_keyframe_bank_size": 1, "ll_keyframe_bank_match": 6, "ll_keyframe_bank_debug_surface": 5,
       "ll_keyframe_bank_work": 2}


def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "loam_livox_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    L = capi.load()
    for name, n_args in NEW.items():
        decl = re.search(r"\b(int|void|int64_t)\s+" + name + r"\s*\(([^;]*)\);", header)
        assert decl and name in capi.SYMBOLS, name
        fn = getattr(L, name)
        assert len(decl.group(2).split(",")) == len(fn.argtypes) == n_args, name
        assert fn.restype is {"int": C.c_int32, "void": None, "int64_t": C.c_int64}[decl.group(1)], name
    import inspect
    from loam_livox_amd.api import Keyframe_bank
    from loam_livox_amd.keyframes import Keyframe_assembly
    for method in ("add_cell_map", "add_images", "match", "surface", "work", "close"):
        assert callable(getattr(Keyframe_bank, method)), method
    p = inspect.signature(Keyframe_assembly.__init__).parameters
    assert p["device_bank"].default is False and p["bank"].default is None
    assert callable(Keyframe_assembly.analyse_front) and callable(Keyframe_assembly.walk_front)


def test_null_handles_and_bad_arguments_are_refused_without_a_device():
    L = capi.load()
    h, eid = C.c_void_p(), C.c_int64(-7)
    img, ids, sims, work = np.zeros((60, 60), np.float32), np.zeros(1, np.int64), np.zeros(1, np.float32), np.zeros(4, np.int64)
    assert L.ll_keyframe_bank_create(0, 16, None) < 0 and b"ll_keyframe_bank_create: null" in L.ll_last_error()
    assert L.ll_keyframe_bank_create(0, 0, C.byref(h)) < 0 and b"initial_entries out of range" in L.ll_last_error() and not h.value
    assert L.ll_keyframe_bank_create(0, -3, C.byref(h)) < 0 and b"initial_entries out of range" in L.ll_last_error() and not h.value
    # 2^31 / (2 * 3600) = 298 261.6: entry 298 262 would pass 2^31 image floats
    assert L.ll_keyframe_bank_create(0, 298262, C.byref(h)) < 0 and b"would pass 2^31 image floats" in L.ll_last_error() and not h.value
    assert L.ll_keyframe_bank_add_cellmap(None, None, 0.9, None, None, None, None, None, C.byref(eid)) < 0
    assert b"ll_keyframe_bank_add_cellmap: null" in L.ll_last_error() and eid.value == -7
    assert L.ll_keyframe_bank_add_images(None, capi.ptr(img), capi.ptr(img), C.byref(eid)) < 0
    assert b"ll_keyframe_bank_add_images: null" in L.ll_last_error() and eid.value == -7
    assert L.ll_keyframe_bank_images(None, 0, capi.ptr(img), capi.ptr(img)) < 0 and b"ll_keyframe_bank_images: null" in L.ll_last_error()
    assert L.ll_keyframe_bank_size(None) < 0 and b"ll_keyframe_bank_size: null" in L.ll_last_error()
    assert L.ll_keyframe_bank_match(None, 1, capi.ptr(ids), capi.ptr(ids), capi.ptr(sims), capi.ptr(sims)) < 0
    assert b"ll_keyframe_bank_match: null" in L.ll_last_error()
    assert L.ll_keyframe_bank_debug_surface(None, 0, 0, 0, None) < 0 and b"ll_keyframe_bank_debug_surface: null" in L.ll_last_error()
    assert L.ll_keyframe_bank_work(None, capi.ptr(work)) < 0 and b"ll_keyframe_bank_work: null" in L.ll_last_error()
    L.ll_keyframe_bank_destroy(None)


# ------------------------------------------------------------------------------------------------ bookkeeping against stubs
K = 40
AVAIL_P, AVAIL_L, SIM_LIN, SIM_PLAN, INLIER = 0.05, 0.03, 0.65, 0.95, 0.35
WALKS = [(1, 3), (2, 1), (3, 6), (4, 2), (5, 4), (6, 2)]       # (seed, minimum_keyframe_differen) of tests/test_keyframes.py's walks


def script(seed):
    """the scripted key frames, similarities and alignment results of tests/test_keyframes.py
    test_loop_detector_walk_equals_the_reference_text, value for value (that test builds them inline)"""
    rng = np.random.default_rng(seed)
    ratio_p, ratio_l = rng.uniform(0.0, 0.12, K).astype(np.float32), rng.uniform(0.0, 0.07, K).astype(np.float32)
    roi = rng.uniform(4.0, 13.0, K).astype(np.float32)
    n_cells = rng.integers(900, 1100, K)
    sim_p = rng.uniform(0.85, 1.0, (K, K)).astype(np.float32)
    sim_l = rng.uniform(0.4, 0.9, (K, K)).astype(np.float32)
    thr = rng.uniform(0.36 if seed % 2 else 0.2, 1.0, (K, K)).astype(np.float32)
    if seed % 2 == 0:
        thr[thr < 0.35] += 0.2
        thr[K - 5, :] = 0.1
        sim_p[K - 5, :] = 0.99
        roi[K - 5] = roi[: K - 5].mean()
        n_cells[K - 5] = 1200
    return dict(ratio_p=ratio_p, ratio_l=ratio_l, roi=roi, n_cells=n_cells, sim_p=sim_p, sim_l=sim_l, thr=thr)


class StubMap:
    def __init__(self, sc, k, events=None):
        self.sc, self.k, self.events = sc, k, events

    def keyframe_images(self):
        img = np.zeros((4, 1, 1), np.float32)
        img[:, 0, 0] = self.k
        return dict(images=img, ratio_nonzero=np.array([self.sc["ratio_l"][self.k], self.sc["ratio_p"][self.k], 0, 0], np.float32),
                    roi_range=float(self.sc["roi"][self.k]))

    def close(self):
        pass


class StubBank:
    """stands in for api.Keyframe_bank: an entry remembers the stub map it was added from; match answers from the scripts"""

    def __init__(self):
        self.entries, self.calls = [], []

    def add_cell_map(self, cm, roi_ratio=0.9):
        self.entries.append(cm)
        return cm.keyframe_images(), len(self.entries) - 1

    def match(self, ids_a, ids_b):
        assert len(ids_a) == len(ids_b) > 0
        self.calls.append((list(ids_a), list(ids_b)))
        a, b = [self.entries[i] for i in ids_a], [self.entries[i] for i in ids_b]
        assert all(x.sc is y.sc for x, y in zip(a, b))                 # a pair never crosses sequences
        return (np.array([x.sc["sim_l"][x.k, y.k] for x, y in zip(a, b)], np.float32),
                np.array([x.sc["sim_p"][x.k, y.k] for x, y in zip(a, b)], np.float32))

    def close(self):
        pass


class StubAlignment:
    def __init__(self, *a, **k):
        self.pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)

    def find_tranfrom_of_two_mappings(self, a, b):
        a.events.append(f"A {a.k} {b.k}")      # (into the list of the assembly whose key frames these are)
        return float(a.sc["thr"][a.k, b.k])


def stub_assembly(monkeypatch, sc, min_diff, events, **kw):
    from loam_livox_amd import keyframes as kfm

    def similarity(a, b, device=0):
        ka, kb = int(a[0, 0]), int(b[0, 0])
        plane = similarity.calls % 2 == 0      # the plane image first, then the line image (:1009-1010)
        similarity.calls += 1
        return float((similarity.sc["sim_p"] if plane else similarity.sc["sim_l"])[ka, kb])
    similarity.calls, similarity.sc = 0, sc
    monkeypatch.setattr(kfm, "Scene_alignment", StubAlignment)
    ka = kfm.Keyframe_assembly(full_cell_map=ScriptedMap([]), minimum_keyframe_differen=min_diff, minimum_similarity_linear=SIM_LIN,
                               minimum_similarity_planar=SIM_PLAN, map_alignment_inlier_threshold=INLIER, avail_ratio_plane=AVAIL_P,
                               avail_ratio_line=AVAIL_L, **kw)
    ka.materialize = lambda kf: StubMap(sc, kf.k, events)
    ka.new_keyframe_map = lambda n_cells: StubMap(sc, -1)
    ka.similarity = similarity
    return ka


def waiting_keyframe(sc, k):
    from loam_livox_amd import keyframes as kfm
    kf = kfm.Maps_keyframe()
    kf.k = k
    kf.m_set_cell = set(range(int(sc["n_cells"][k])))
    return kf


def gated(sc, k, min_diff):
    """the earlier key frames that pass :994, :1001 and :1004 when key frame k is the new one (it is the k + 1-th of the vector)"""
    return [his for his in range(k) if (k + 1) - his >= min_diff and not (sc["ratio_p"][his] < AVAIL_P and sc["ratio_l"][his] < AVAIL_L)
            and not abs(float(sc["roi"][his]) - float(sc["roi"][k])) > 5.0]


def outcome(ka):
    log = [{key: (v.tolist() if isinstance(v, np.ndarray) else v) for key, v in r.items()} for r in ka.log + ka.loops]
    return ka.state(), log, ka.if_end, len(ka.keyframe_vec)


@pytest.mark.parametrize("seed,min_diff", WALKS)
def test_device_bank_over_a_stub_gives_the_walk_of_the_pairwise_route(monkeypatch, seed, min_diff):
    from loam_livox_amd import keyframes as kfm
    sc = script(seed)
    ev_off, ev_on = [], []
    off = stub_assembly(monkeypatch, sc, min_diff, ev_off)
    monkeypatch.setattr(kfm, "keyframe_similarity", off.similarity)
    bank = StubBank()
    on = stub_assembly(monkeypatch, sc, min_diff, ev_on, device_bank=True, bank=bank)
    found, want_calls = ([], []), []
    for k in range(K):
        for ka, loops in zip((off, on), found):
            ka.m_keyframe_need_precession_list.append(waiting_keyframe(sc, k))
        processed = not off.if_end
        found[0].extend(off.process_waiting())
        found[1].extend(on.process_waiting())
        if processed and gated(sc, k, min_diff):
            want_calls.append(([k] * len(gated(sc, k, min_diff)), gated(sc, k, min_diff)))
    assert outcome(on) == outcome(off) and ev_on == ev_off
    assert [{key: (v.tolist() if isinstance(v, np.ndarray) else v) for key, v in r.items()} for r in found[1]] == \
        [{key: (v.tolist() if isinstance(v, np.ndarray) else v) for key, v in r.items()} for r in found[0]]
    # one match per processed key frame with candidates, over exactly the gated pairs (entry id = key-frame index: one sequence, one bank)
    assert bank.calls == want_calls
    assert len(off.log) > 10 and sum(e.startswith("A ") for e in ev_off) > 3 and (seed % 2 == 1 or (off.if_end and len(off.loops) == 1))
    assert off.similarity.calls == 2 * len([r for r in off.log if "sim_plane" in r])
    if seed % 2 == 1:
        assert sum(len(a) for a, _ in bank.calls) > len(on.log)        # similarities of candidates the walk skipped were computed, and never seen
    assert on.rounds.bank.handle is bank and not on.rounds.bank.own
    on.close()
    assert bank.entries                                                # a bank handed in is not closed by the assembly


def test_batched_loop_makes_one_match_per_round_over_all_slots(monkeypatch):
    from loam_livox_amd import keyframes as kfm
    S, min_diff = 3, 2
    scripts = [script(seed) for seed in (2, 3, 6)]
    alone = [stub_assembly(monkeypatch, sc, min_diff, []) for sc in scripts]
    bank = StubBank()
    slots = [stub_assembly(monkeypatch, sc, min_diff, [], device_bank=True, bank=bank) for sc in scripts]

    class Store:
        calls = 0

        def extract_cells(self, kind, sequences, cell_lists, dsts):
            Store.calls += 1
            assert kind == 2 and len(sequences) == len(cell_lists) == len(dsts)

    rounds_of_the_loop, loops = kfm.Keyframe_rounds(slots, store=Store(), bank=bank), [[] for _ in range(S)]
    rounds = 0
    for k in range(K):
        busy = [s for s in range(S) if not alone[s].if_end]
        n_new = {s: 2 if (k == 7 and s == 1) else 1 for s in range(S)}          # slot 1 closes two key frames in one step: two rounds
        nxt = [len(a.keyframe_vec) + len(a.m_keyframe_need_precession_list) for a in alone]
        for s in range(S):
            for j in range(n_new[s]):
                if nxt[s] + j < K:
                    for ka in (alone[s], slots[s]):
                        ka.m_keyframe_need_precession_list.append(waiting_keyframe(scripts[s], nxt[s] + j))
        before, stores = len(bank.calls), Store.calls
        for s in range(S):
            monkeypatch.setattr(kfm, "keyframe_similarity", alone[s].similarity)
            alone[s].process_waiting()
        for s, found in enumerate(rounds_of_the_loop.run(list(range(S)))):
            loops[s] += found
        step_rounds = Store.calls - stores                                        # one extraction per round
        assert len(bank.calls) - before <= step_rounds
        if k == 7 and 1 in busy:
            assert step_rounds == 2
        rounds += step_rounds
    for s in range(S):
        assert outcome(slots[s]) == outcome(alone[s]), s
        assert [dict(r, icp_q=None, icp_t=None) for r in loops[s]] == [dict(r, icp_q=None, icp_t=None) for r in alone[s].loops], s
    assert any(a.if_end for a in alone) and not all(a.if_end for a in alone)
    # a round's match carries the pairs of all its slots: some call holds entries of more than one sequence, and there are far fewer
    # matches than processed key frames with candidates
    per_call = [len({id(bank.entries[i].sc) for i in a}) for a, _ in bank.calls]
    assert max(per_call) == S and len(bank.calls) <= rounds
    assert len(bank.calls) < sum(1 for s in range(S) for k in range(len(alone[s].keyframe_vec)) if gated(scripts[s], k, min_diff))
