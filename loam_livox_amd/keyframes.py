"""Key-frame assembly of the mapping loop and the front half of loop detection, on top of the C ABI.

Mirrors hku-mars/loam_livox source/laser_mapping.hpp:
  :626          one open key frame from the start (m_keyframe_of_updating_list);
  :1524-1562    per accepted scan: append the scan's full cloud (map frame) to the full cell map and collect the cells it touched
                (Points_cloud_map::append_cloud( pts, &cell_vec ), cell_map_keyframe.hpp:619-672: >= 3 points of the scan, every cell on an
                empty map), add them to every open key frame (Maps_keyframe::add_cells, cell_map_keyframe.hpp:1243-1261), close the oldest
                key frame after scans_of_each_keyframe scans, open another every scans_between_two_keyframe scans, keep at most
                maximum_keyframe_in_waiting_list closed ones waiting;
  :919-1060     service_loop_detection's body for one waiting key frame: update_features_of_each_cells + analyze (the four direction images),
                then against every earlier key frame: the distance-in-time gate, the non-zero ratio gate, the ROI range gate, the image
                similarities, the cell-count gate, and Scene_alignment::find_tranfrom_of_two_mappings; a pair whose inlier threshold
                ends below map_alignment_inlier_threshold is reported as a loop with the alignment's transform (:1054-1068).
pose_graph=True adds what the node does with an accepted loop (:948-960, 1058-1089): the chain constraints over pose3d_vec plus the one
loop constraint, optimised on the device (api.Pose_graph); close_loop keeps poses_ori, poses_opm, constraints and pose_graph_summary.
map_refinement=True (it needs pose_graph) adds the corrected map behind that (:943-946, 1091-1100): every key frame's accumulated cloud
goes through api.Map_refine.add_cloud when the key frame is processed (VoxelGrid at surround_pointcloud_resolution; the host copy is
dropped, the key frame keeps the id -- its index in keyframe_vec, as map_id_pc.size() is, when the store is the assembly's own; a
shared handle gives whatever id comes next, and refine_map goes through the key frames' ids), and refine_map() re-projects every
second one, newest first, with R_opm R_ori^T after a VoxelGrid at map_refinement_resolution: self.refined holds the
/pc_aft_loop_closure messages.  The file dumps behind the pose graph (:1069-1110) are out of scope.

A key frame is a SET OF CELLS of the full cell map, not a copy: the reference's key frames hold shared pointers to the map's cells, so
what a key frame is analysed with is whatever those cells contain when it is processed (earlier and later scans included).  Here a key
frame keeps the cell indices; `materialize` copies those cells out of the device-resident full map into a cell map of its own
(ll_cellmap_extract_cells, on the device), in the map's (cell, insertion) order, which is the order determine_feature's float sums run in.

Memory (the shipped loop_closure settings keep a few hundred key frames before any pair is old enough to be compared,
minimum_keyframe_differen = 200): a processed key frame keeps its direction images, its cell set and the compacted points it was analysed
with (12 bytes per point, host memory) -- NOT a device cell map; `cell_map_of` builds one again from those points (same order, so the same
cells, features and clouds) for the pairs that pass the similarity gates, and it is closed after the alignment.  The full map starts at
max_points and doubles (ll_cellmap_reserve) when a scan would not fit, as the reference's heap-allocated cells grow.

Differences from the node, by design: everything runs synchronously (the node's service thread polls every millisecond);
m_accumulated_point_cloud (only consumed by the map refinement) is kept with map_refinement=True alone: the full clouds of the scans the
history's add rule let in wait in a host FIFO (m_laser_cloud_full_history, :1456, trimmed to maximum_history_size, :1480-1486), and the
whole FIFO is appended to the BACK key frame at the moment the next one is opened, then cleared (:1545-1558).  With scan_log= (slot s
of a History_buffer_batch's scan log, handed in by the lock-step loop) that FIFO lives on the device: the owner of the batch pushes
for all slots (log_full), the flush is a hand_over whose group id the back key frame keeps, a key frame's stored cloud comes from
Map_refine.add_logged, and the groups of a key frame nobody will process are dropped.

device_bank=True keeps the line and plane image of every processed key frame in a device-resident api.Keyframe_bank and asks for the
similarities of a new key frame against ALL earlier key frames that pass the three scalar gates in one Keyframe_bank.match, instead of
two keyframe_similarity calls per pair inside the walk; the floats are the same to the bit, and so are log, loops and if_end.

One pass over a waiting key frame -- analyse_front (materialise, analyse, gate, store its cloud), one match, walk_front, close and refine
an accepted loop -- is written once, in Keyframe_rounds, for any number of assemblies that share the services: process_waiting is that
driver over the assembly alone, and the lock-step loop runs it over all its slots."""
from __future__ import annotations

from collections import deque

import numpy as np

from . import api
from .api import Cell_map, keyframe_similarity
from .scene_alignment import Scene_alignment


class Maps_keyframe:
    """cell_map_keyframe.hpp:1003-1261, the members the assembly and the detector touch."""

    def __init__(self):
        self.m_set_cell = set()          # cell indices (i, j, k) of the full map
        self.m_accumulate_frames = 0
        self.m_ending_frame_idx = 0
        self.m_pose_q = np.array([0, 0, 0, 1], np.float64)
        self.m_pose_t = np.zeros(3, np.float64)
        self.m_accumulated_point_cloud = []   # full clouds [n, 4] appended at :1552 (map_refinement); emptied once the cloud is on the device
        self.cloud_id = None             # its id in the api.Map_refine store, once processed
        self.points = None               # xyz of its cells as they were when it was processed, in the full map's (cell, insertion) order
        self.analysis = None             # Cell_map.keyframe_images() of those cells

    def add_cells(self, cell_ijk: np.ndarray) -> None:   # :1243-1261
        self.m_set_cell.update(_pack_cells(cell_ijk).tolist())
        self.m_accumulate_frames += 1

    # what service_loop_detection reads
    @property
    def m_ratio_nonzero_line(self):
        return float(self.analysis["ratio_nonzero"][0])

    @property
    def m_ratio_nonzero_plane(self):
        return float(self.analysis["ratio_nonzero"][1])

    @property
    def m_roi_range(self):
        return float(self.analysis["roi_range"])

    @property
    def m_feature_img_line(self):
        return self.analysis["images"][0]

    @property
    def m_feature_img_plane(self):
        return self.analysis["images"][1]


class Keyframe_assembly:
    def __init__(self, device: int = 0, cell_resolution: float = 1.0, threshold_cell_revisit: int = 5000, max_points: int = 1 << 22,
                 scans_of_each_keyframe: int = 300, scans_between_two_keyframe: int = 100, maximum_keyframe_in_waiting_list: int = 3,
                 minimum_keyframe_differen: int = 200, minimum_similarity_linear: float = 0.65, minimum_similarity_planar: float = 0.95,
                 map_alignment_resolution: float = 0.2, map_alignment_inlier_threshold: float = 0.35,
                 map_alignment_maximum_icp_iteration: int = 2, scene_alignments_maximum_residual_block: int = 5000,
                 keyframe_max_points: int = 1 << 20, full_cell_map=None, avail_ratio_plane: float = 0.05, avail_ratio_line: float = 0.03,
                 device_alignment: bool = False, device_bank: bool = False, bank=None, pose_graph=False,
                 map_refinement=False, surround_pointcloud_resolution: float = 0.5, map_refinement_resolution: float = 0.2,
                 maximum_history_size: int = 100, scan_log=None):
        # parameter names and defaults: laser_mapping.hpp:698-710 (loop_closure/*), :686-687 (mapping/pt_cell_resolution, threshold_cell_revisit)
        self.device = device
        self.m_pt_cell_resolution = cell_resolution
        # (full_cell_map: anything with append_cloud_touched / dump / close -- tests drive the bookkeeping without a device, and the
        #  lock-step loop hands in api.Full_map_slot, slot s of the batched full-cloud store: its append_cloud_touched answers with the
        #  cells the step's one batched append listed for the slot, so add_scan is given an empty cloud there)
        self.m_pt_cell_map_full = full_cell_map if full_cell_map is not None else \
            Cell_map(max_points, cell_resolution, threshold_cell_revisit, device=device)   # :616-617
        self.m_para_scans_of_each_keyframe = scans_of_each_keyframe
        self.m_para_scans_between_two_keyframe = scans_between_two_keyframe
        self.m_loop_closure_maximum_keyframe_in_wating_list = maximum_keyframe_in_waiting_list
        self.m_loop_closure_minimum_keyframe_differen = minimum_keyframe_differen
        self.m_loop_closure_minimum_similarity_linear = minimum_similarity_linear
        self.m_loop_closure_minimum_similarity_planar = minimum_similarity_planar
        self.m_loop_closure_map_alignment_resolution = map_alignment_resolution
        self.m_loop_closure_map_alignment_inlier_threshold = map_alignment_inlier_threshold
        self.m_loop_closure_map_alignment_maximum_icp_iteration = map_alignment_maximum_icp_iteration
        self.m_para_scene_alignments_maximum_residual_block = scene_alignments_maximum_residual_block
        self.keyframe_max_points = keyframe_max_points
        # locals of service_loop_detection (laser_mapping.hpp:887-888: "0.05 for 300 scans, 0.15 for 1000 scans"): a key frame whose direction
        # images are emptier than this is not compared against
        self.avail_ratio_plane, self.avail_ratio_line = avail_ratio_plane, avail_ratio_line
        self.m_keyframe_of_updating_list = deque([Maps_keyframe()])   # :626
        self.m_keyframe_need_precession_list = deque()
        self.keyframe_vec = []          # service_loop_detection's keyframe_vec
        self.pose3d_vec = []            # ... and the poses it pairs with them
        self.loops = []                 # detected loops: dict(his, last, inlier_threshold, icp_q, icp_t)
        self.if_end = False
        self.log = []                   # one record per compared pair (what the node writes to loop_closure.log)
        self._prefetched = None         # (key frame, its cell map) handed over in advance (prefetch)
        # device_alignment: candidate pairs are aligned without a host hop (Scene_alignment( on_device=True )) by ONE object, whose
        # handle -- registrar, map, voxel filter -- serves every pair; off, every pair gets a Scene_alignment of its own, as before
        self.device_alignment = device_alignment
        self._scene_alignment = None
        self._front = None              # (key frame, candidates) between analyse_front and walk_front
        # The three services of the detector's back end, each off, this assembly's own (created on first use) or a handle to share, whose
        # owner closes it (Keyframe_rounds has the rule):
        #   device_bank=True / bank=: the key frames' line and plane images stay on the device (api.Keyframe_bank; anything with
        #     add_cell_map / match) and a new key frame is compared against all gated earlier ones in one match;
        #   pose_graph=True or a handle (api.Pose_graph; anything with solve( graphs )): an accepted loop is closed, close_loop;
        #   map_refinement=True or a handle (api.Map_refine; anything with add_cloud / refine / merge -- "on" whatever its truth value: an
        #     empty api.Map_refine has length 0).  surround_pointcloud_resolution: :696, the leaf of the add; map_refinement_resolution:
        #     :903, Mapping_refine's leaf.
        # self.rounds is the driver that serves this assembly: its own over [self], until an owner of many assemblies builds one over them.
        self.rounds = self._own_rounds = Keyframe_rounds([self], bank=bank if bank is not None else bool(device_bank), pose_graph=pose_graph,
                                                         map_refinement=map_refinement)
        self.device_bank, self.pose_graph, self.map_refinement = self.rounds.bank.on, self.rounds.pose_graph.on, self.rounds.map_refine.on
        if self.map_refinement and not self.pose_graph:
            raise ValueError("map_refinement needs pose_graph: the corrected map is made from the optimised poses")
        self.pending_loops = []         # accepted loops not yet closed: the round's one solve takes them; a solve that raised leaves them
        self.poses_ori, self.poses_opm, self.constraints, self.pose_graph_summary = None, None, None, None
        self.surround_pointcloud_resolution, self.map_refinement_resolution = surround_pointcloud_resolution, map_refinement_resolution
        self.m_maximum_history_size = maximum_history_size
        self.m_laser_cloud_full_history = deque()   # :1456
        self.refined = None             # [(pc_idx, cloud [n, 4])] of the last refine_map: the /pc_aft_loop_closure messages, in their order
        # scan_log: slot s of a batched match buffer's scan log (api.Scan_log_slot; anything with hand_over() / drop( ids ) and, for the
        # assembly's own add, a .batch), in the manner of full_cell_map=.  With it m_laser_cloud_full_history lives on the device and the
        # owner of the batch makes the push for all slots (History_buffer_batch.log_full): add_scan keeps no host arrays, the flush is a
        # hand_over, and a key frame's m_accumulated_point_cloud holds group ids, which Map_refine.add_logged turns into its stored cloud.
        self.scan_log = scan_log

    def state(self) -> str:
        """the lists as tests/verbatim_build.py's harness prints them: open key frames frames:cells, waiting ones frames:cells:ending-index"""
        u = " ".join(f"{kf.m_accumulate_frames}:{len(kf.m_set_cell)}" for kf in self.m_keyframe_of_updating_list)
        w = " ".join(f"{kf.m_accumulate_frames}:{len(kf.m_set_cell)}:{kf.m_ending_frame_idx}" for kf in self.m_keyframe_need_precession_list)
        return ("U " + u).rstrip() + " W" + (" " + w if w else "")

    def close(self):
        if self.scan_log is not None:   # the groups nobody will read any more: open and waiting key frames, and one analysed but not yet stored
            orphans = []
            for kf in list(self.m_keyframe_of_updating_list) + list(self.m_keyframe_need_precession_list) + self.keyframe_vec[-1:]:
                orphans += kf.m_accumulated_point_cloud
                kf.m_accumulated_point_cloud = []
            self.scan_log.drop(orphans)
            self.scan_log = None
        if self.m_pt_cell_map_full is not None:
            self.m_pt_cell_map_full.close()
            self.m_pt_cell_map_full = None
        if self._scene_alignment is not None:
            self._scene_alignment.close()
            self._scene_alignment = None
        self._own_rounds.close()

    # ---- laser_mapping.hpp:1524-1562 ------------------------------------------------------------------------------------------------
    def add_scan(self, full_cloud_map_frame: np.ndarray, pose: np.ndarray, current_frame_index: int, history_added: bool = True) -> np.ndarray:
        """One accepted scan.  full_cloud_map_frame: current_laser_cloud_full after pointcloudAssociateToMap; pose: m_q_w_curr /
        m_t_w_curr as {qx, qy, qz, qw, tx, ty, tz}; history_added: whether the history's add rule let the scan in (:1446-1448), which is
        what puts its full cloud into m_laser_cloud_full_history (read with map_refinement alone).  Returns the touched cells (cell_vec)."""
        if self.map_refinement and self.scan_log is None:   # :1456, :1480-1486 -- before the key-frame step of the same scan
            if history_added:
                self.m_laser_cloud_full_history.append(np.array(full_cloud_map_frame, np.float32).reshape(-1, 4))
            if len(self.m_laser_cloud_full_history) > self.m_maximum_history_size:
                self.m_laser_cloud_full_history.popleft()
        full = self.m_pt_cell_map_full
        if hasattr(full, "reserve"):  # the reference's map grows on the heap: double the device map's capacity when this scan would not fit
            need = full.stats()[1] + len(full_cloud_map_frame)
            if need > full.max_points:
                full.reserve(max(2 * full.max_points, need))
        cell_vec = full.append_cloud_touched(full_cloud_map_frame, 3)
        for kf in self.m_keyframe_of_updating_list:
            kf.add_cells(cell_vec)
        front = self.m_keyframe_of_updating_list[0]
        if front.m_accumulate_frames >= self.m_para_scans_of_each_keyframe:
            front.m_ending_frame_idx = current_frame_index
            front.m_pose_q = np.array(pose[:4], np.float64)
            front.m_pose_t = np.array(pose[4:7], np.float64)
            self.m_keyframe_need_precession_list.append(front)
            self.m_keyframe_of_updating_list.popleft()
        # (with scans_of_each_keyframe <= scans_between_two_keyframe the list can run empty here; the node would dereference back() of
        #  an empty list -- the shipped 300 / 100 never does; a new key frame is opened instead)
        if not self.m_keyframe_of_updating_list:
            self.m_keyframe_of_updating_list.append(Maps_keyframe())
        elif self.m_keyframe_of_updating_list[-1].m_accumulate_frames >= self.m_para_scans_between_two_keyframe:
            if self.map_refinement and self.scan_log is not None:   # the same on the device: the slot's FIFO becomes a group
                self.m_keyframe_of_updating_list[-1].m_accumulated_point_cloud.append(self.scan_log.hand_over())
            elif self.map_refinement:   # :1550-1553, 1558: the whole FIFO to the back key frame, then cleared
                self.m_keyframe_of_updating_list[-1].m_accumulated_point_cloud.extend(self.m_laser_cloud_full_history)
                self.m_laser_cloud_full_history.clear()
            if len(self.m_keyframe_need_precession_list) > self.m_loop_closure_maximum_keyframe_in_wating_list:
                out = self.m_keyframe_need_precession_list.popleft()
                if self.scan_log is not None:   # its groups are orphans
                    self.scan_log.drop(out.m_accumulated_point_cloud)
                    out.m_accumulated_point_cloud = []
            self.m_keyframe_of_updating_list.append(Maps_keyframe())
        return cell_vec

    # ---- the key frame's view of the shared cells ------------------------------------------------------------------------------------
    def prefetch(self, kf: Maps_keyframe, cell_map) -> None:
        """hand over, in advance, the cell map materialize( kf ) is to return: an owner of many assemblies extracts the key frames they
        close in the same step in one call (History_buffer_batch.extract_cells).  Consumed by the next materialize of that key frame."""
        self._prefetched = (kf, cell_map)

    def wanted_cells(self, kf: Maps_keyframe) -> np.ndarray:
        """the key frame's cells as {i, j, k} [n, 3]"""
        return _unpack_cells(np.fromiter(kf.m_set_cell, np.int64, len(kf.m_set_cell)))

    def materialize(self, kf: Maps_keyframe) -> Cell_map:
        """the key frame's cells as a cell map of their own (the caller closes it): the one handed over in advance for this key frame
        (prefetch), else copied on the device when the full map offers it (Cell_map.extract_cells, or a batch slot's
        extract_cells_into: no sort, nothing but the cell list crosses to the device), through the host otherwise (test stubs).  All
        give the same map: the cells in key order, every cell's points in the full map's stored order."""
        ready, self._prefetched = self._prefetched, None
        if ready is not None:
            if ready[0] is kf:
                return ready[1]
            _close(ready[1])
        full = self.m_pt_cell_map_full
        route = getattr(full, "extract_cells", None) or getattr(full, "extract_cells_into", None)
        if route is None:
            return self._materialize_host(kf)
        want = self.wanted_cells(kf)
        km = self.new_keyframe_map(len(want))
        route(want, km)
        return km

    def new_keyframe_map(self, n_cells: int) -> Cell_map:
        """an empty cell map for a key frame of n_cells cells to be extracted into (it grows to the points the cells hold)"""
        return Cell_map(max(1024, n_cells), self.m_pt_cell_resolution, device=self.device)

    def _materialize_host(self, kf: Maps_keyframe) -> Cell_map:
        xyz, ijk, start, _ = self.m_pt_cell_map_full.dump()
        want = np.fromiter(kf.m_set_cell, np.int64, len(kf.m_set_cell))
        sel = np.flatnonzero(np.isin(_pack_cells(ijk), want))
        start = np.asarray(start, np.int64)
        lens = start[sel + 1] - start[sel]
        # the points of the selected cells, cell after cell: position p of the output lies in selected cell c(p) at offset p - first(c)
        first = np.cumsum(lens) - lens
        idx = np.repeat(start[sel] - first, lens) + np.arange(int(lens.sum()), dtype=np.int64)
        return self._cell_map_from_points(xyz[idx])

    def _cell_map_from_points(self, xyz: np.ndarray) -> Cell_map:
        km = Cell_map(max(1024, len(xyz) + 1), self.m_pt_cell_resolution, device=self.device)
        if len(xyz):
            km.append_cloud(np.c_[xyz, np.zeros(len(xyz), np.float32)].astype(np.float32))
        return km

    def cell_map_of(self, kf: Maps_keyframe):
        """a device cell map of a processed key frame, rebuilt from the points it was analysed with (the caller closes it); a key frame
        that kept no points (test stubs) is read out of the full map again"""
        return self._cell_map_from_points(kf.points) if kf.points is not None else self.materialize(kf)

    # ---- laser_mapping.hpp:919-1060 --------------------------------------------------------------------------------------------------
    def process_waiting(self, limit: int | None = None):
        """Every waiting key frame (the first `limit` of them, when given) through one pass of service_loop_detection's loop body: the
        rounds of Keyframe_rounds.run over this assembly alone.  Returns the loops found in this call."""
        return self.rounds.run([self.rounds.assemblies.index(self)], limit)[0]

    def analyse_front(self) -> list:
        """The analysis half of one pass: the first waiting key frame leaves the list, is materialised and analysed (through the bank
        with device_bank=True: the same dict, and its line and plane image stay on the device), its accumulated cloud goes into the
        map-refinement store, and it joins keyframe_vec.  Returns the earlier key frames `his` that pass the gates of :994, :1001 and
        :1004 -- the only ones whose similarities the walk can ask for."""
        return self.rounds.analyse([self])[0]

    def _analyse(self) -> list:
        """analyse_front without the stored cloud of the scan-log route, which the driver adds for all key frames of a round at once"""
        last = self.m_keyframe_need_precession_list.popleft()
        cm = self.materialize(last)                     # update_features_of_each_cells + analyze read the cells as they are now
        if self.rounds.bank.on:
            last.analysis, last.bank_id = self.rounds.bank().add_cell_map(cm)
        else:
            last.analysis = cm.keyframe_images()
        last.points = cm.dump()[0] if hasattr(cm, "dump") else None
        _close(cm)
        if self.map_refinement and self.scan_log is None:   # :943-946: down_sample_filter over the accumulated cloud; map_id_pc's key is its size
            acc = np.concatenate(last.m_accumulated_point_cloud) if last.m_accumulated_point_cloud else np.zeros((0, 4), np.float32)
            last.cloud_id = self.rounds.map_refine().add_cloud(acc, self.surround_pointcloud_resolution)[0]
            last.m_accumulated_point_cloud = []
        self.keyframe_vec.append(last)
        self.pose3d_vec.append((last.m_pose_q.copy(), last.m_pose_t.copy()))
        n_kf = len(self.keyframe_vec)
        candidates = [his for his in range(n_kf - 1) if self._passes_gates(n_kf, his, last)]
        self._front = (last, candidates)
        return candidates

    def front_pairs(self):
        """(ids_a, ids_b) of the bank entries of analyse_front's candidates: a = the new key frame, b = the old one, as the detector
        calls max_similiarity_of_two_image (:1009-1010)"""
        last, candidates = self._front
        return [last.bank_id] * len(candidates), [self.keyframe_vec[his].bank_id for his in candidates]

    def _passes_gates(self, n_kf: int, his: int, last: Maps_keyframe) -> bool:
        """the three scalar gates in front of the image comparison"""
        old = self.keyframe_vec[his]
        if n_kf - his < self.m_loop_closure_minimum_keyframe_differen:   # :994
            return False
        if old.m_ratio_nonzero_plane < self.avail_ratio_plane and old.m_ratio_nonzero_line < self.avail_ratio_line:   # :1001, :887-888
            return False
        if abs(old.m_roi_range - last.m_roi_range) > 5.0:   # :1004
            return False
        return True

    # ---- laser_mapping.hpp:948-960, 1058-1089 -------------------------------------------------------------------------------------
    def loop_graph(self, loop) -> dict:
        """The graph the node optimises when it accepts `loop` (a record of self.loops): pose3d_vec as the poses; constrain_vec -- the
        chain constraint k -> k + 1 of every two consecutive key-frame poses, built from those poses (:951-960) -- and behind them the
        loop constraint last -> his from the alignment's inverted transform (:1058-1078, add_constrain_of_loop)."""
        from .api import loop_constraint, relative_constraint
        poses = np.array([_pose7(q, t) for q, t in self.pose3d_vec], np.float64).reshape(-1, 7)
        last, his = loop["last"], loop["his"]
        ab = [(k, k + 1) for k in range(len(poses) - 1)]
        meas = [relative_constraint(poses[k], poses[k + 1]) for k in range(len(poses) - 1)]
        s_idx, t_idx, m = loop_constraint(last, his, poses[his], poses[last], loop["icp_q"], loop["icp_t"])
        ab.append((s_idx, t_idx))
        meas.append(m)
        return dict(poses=poses, ab=np.array(ab, np.int32).reshape(-1, 2), meas=np.array(meas, np.float64).reshape(-1, 7))

    def take_solution(self, graph: dict, poses_opm: np.ndarray, summary: dict) -> None:
        """keeps what close_loop keeps, from a solve its caller made, and refines the map behind it with map_refinement"""
        self._keep_solution(graph, poses_opm, summary)
        if self.map_refinement:
            self.refine_map()

    def _keep_solution(self, graph: dict, poses_opm: np.ndarray, summary: dict) -> None:
        self.poses_ori, self.poses_opm = graph["poses"].copy(), np.asarray(poses_opm, np.float64).reshape(-1, 7).copy()   # pose3d_map_ori, temp_pose_3d_map
        self.constraints = dict(ab=graph["ab"].copy(), meas=graph["meas"].copy())                                           # constrain_vec_temp
        self.pose_graph_summary = dict(summary)

    # ---- laser_mapping.hpp:1091-1100; ceres_pose_graph_3d.hpp:368-538 -------------------------------------------------------------------
    def refine_map(self) -> list:
        """The node's loop at :1091-1100: refine_pointcloud( map_id_pc, pose3d_map_ori, temp_pose_3d_map, pc_idx, 0 ) for pc_idx = K - 1,
        K - 3, ... >= 0 -- one run on the device for all of them.  Keeps and returns self.refined = [(pc_idx, cloud)]."""
        if not self.map_refinement or self.poses_opm is None:
            raise ValueError("refine_map needs map_refinement=True and a closed loop (close_loop / take_solution)")
        self.rounds.refine([self])
        return self.refined

    def refined_mapping(self) -> np.ndarray:
        """Mapping_refine::refine_mapping's in-memory overload over ALL key frames of the closed loop (move, then VoxelGrid,
        ceres_pose_graph_3d.hpp:511-533), concatenated and filtered once more (:577-578): the single corrected map [n, 4]"""
        if not self.map_refinement or self.poses_opm is None:
            raise ValueError("refined_mapping needs map_refinement=True and a closed loop (close_loop / take_solution)")
        ids = list(range(len(self.poses_ori)))
        h = self.rounds.map_refine()
        h.refine([self.keyframe_vec[k].cloud_id for k in ids], self.poses_ori, self.poses_opm, self.map_refinement_resolution, True)
        return h.merge(self.map_refinement_resolution)

    def close_loop(self, loop) -> np.ndarray:
        """Pose-graph optimisation of an accepted loop: builds loop_graph( loop ), solves it on the device and keeps poses_ori,
        poses_opm, constraints and pose_graph_summary; with map_refinement, refine_map behind it.  loops, log, if_end and state() are
        not touched.  Returns poses_opm."""
        self.rounds.close_loops([(self, loop)])
        return self.poses_opm

    def walk_front(self, sims=None):
        """The walk half of one pass (laser_mapping.hpp:988-1057) for the key frame analyse_front added.  sims: (sim_line, sim_plane)
        of analyse_front's candidates, in their order (one Keyframe_bank.match); None: every pair that reaches the comparison asks
        keyframe_similarity itself.  A similarity of a candidate the walk skips (his += 11, += 6, the loop that ends the search) is
        never read.  Returns the loops found."""
        found = []
        last, candidates = self._front
        self._front = None
        where = {his: k for k, his in enumerate(candidates)} if sims is not None else None
        n_kf = len(self.keyframe_vec)
        his = 0
        while his < n_kf - 1:
            if self.if_end:
                break
            old = self.keyframe_vec[his]
            rec = dict(last=n_kf - 1, his=his)
            if not self._passes_gates(n_kf, his, last):
                his += 1
                continue
            if sims is not None:
                sim_plane, sim_line = float(sims[1][where[his]]), float(sims[0][where[his]])
            else:
                sim_plane = keyframe_similarity(last.m_feature_img_plane, old.m_feature_img_plane, self.device)   # :1009-1010
                sim_line = keyframe_similarity(last.m_feature_img_line, old.m_feature_img_line, self.device)
            rec.update(sim_plane=sim_plane, sim_line=sim_line)
            self.log.append(rec)
            if (sim_line > self.m_loop_closure_minimum_similarity_linear and sim_plane > 0.92) or \
                    sim_plane > self.m_loop_closure_minimum_similarity_planar:   # :1012-1013
                # :1030  ( a - b ) / ( a + b ) * 0.1 in size_t arithmetic: zero unless a < b, where a - b wraps around
                if len(last.m_set_cell) < len(old.m_set_cell):
                    his += 1
                    continue
                sa = self._scene_alignment
                if sa is None:
                    sa = Scene_alignment(self.m_loop_closure_map_alignment_resolution, self.m_loop_closure_map_alignment_resolution,   # :1034
                                         self.m_loop_closure_map_alignment_maximum_icp_iteration, self.m_loop_closure_map_alignment_inlier_threshold,
                                         self.m_para_scene_alignments_maximum_residual_block, device=self.device,   # :897-898, 1035
                                         on_device=self.device_alignment)
                    if self.device_alignment:
                        self._scene_alignment = sa
                cm_last, cm_old = self.cell_map_of(last), self.cell_map_of(old)
                thr = sa.find_tranfrom_of_two_mappings(cm_last, cm_old)   # :1036
                _close(cm_last)
                _close(cm_old)
                rec.update(inlier_threshold=thr, pose=sa.pose.copy())
                if thr > self.m_loop_closure_map_alignment_inlier_threshold * 2:   # :1048-1052
                    his += 10 + 1
                    continue
                if thr < self.m_loop_closure_map_alignment_inlier_threshold:   # :1054: "I believe this is true loop."
                    q, t = sa.pose[:4], sa.pose[4:7]
                    qi = np.array([-q[0], -q[1], -q[2], q[3]])                # :1064-1065  ICP_t = ICP_q^-1 * (-ICP_t); ICP_q = ICP_q^-1
                    ti = _quat_rot(qi, -t)
                    loop = dict(his=his, last=n_kf - 1, inlier_threshold=thr, icp_q=qi, icp_t=ti, sim_plane=sim_plane, sim_line=sim_line)
                    self.loops.append(loop)
                    found.append(loop)
                    if self.pose_graph:      # :1058-1089, in the round's one solve (Keyframe_rounds.close_loops)
                        self.pending_loops.append(loop)
                    self.if_end = True   # :1108 (the dumps in between are out of scope)
                    break
                his += 5 + 1   # :1111-1114
                continue
            his += 1
        return found


class _Service:
    """One shared device handle of a Keyframe_rounds: off, handed in (its owner closes it), or created on first use and closed here.
    how: None / False / 0 (off), True (an api.<kind> of the driver's own) or the handle to share."""

    def __init__(self, kind: str, how, device: int):
        own = how is None or isinstance(how, (bool, int))
        self.kind, self.device, self.on, self.handle, self.own = kind, device, bool(how) or not own, None if own else how, False

    def __call__(self):
        if self.handle is None:
            self.handle, self.own = getattr(api, self.kind)(device=self.device), True
        return self.handle

    def close(self):
        if self.own and self.handle is not None:
            self.handle.close()
        self.handle = None


class Keyframe_rounds:
    """The detector's loop body for many assemblies at once: Keyframe_assembly.process_waiting is this over [itself], and the lock-step
    loop (mapping.Laser_mapping_batch) runs it once per step over the slots that accepted a scan.  Slot s gives, bit for bit, what
    assembly s gives run alone -- log, loops, poses_opm, stored clouds and `refined` -- because alone is the same text with one slot.

    It owns the assemblies' shared services (bank, pose_graph, map_refine: _Service each; an assembly reaches them through its
    `rounds`) and, optionally, the batched full-cloud store the key frames' cells are read from (store: anything with
    extract_cells( kind, sequences, cell_lists, dsts ), slot s of this driver being its sequence s).

    One round takes the first waiting key frame of every named slot that has one and has not ended:
      1. extraction: with a store, ONE extract_cells into maps handed to the assemblies in advance (prefetch); no append happens
         between that and the analysis, so the cells are read as they are now (cell_map_keyframe.hpp:1243-1261).  Without a store
         every assembly reads its own full map (materialize);
      2. the analysis half of every slot (through the bank when there is one), and with a scan log ONE Map_refine.add_logged for the
         key frames just analysed, at surround_pointcloud_resolution: stored ids are consecutive in slot order (on the host-FIFO
         route the analysis itself makes an add_cloud per key frame);
      3. with a bank, ONE Keyframe_bank.match over all slots' gated pairs;
      4. the walk half of every slot;
      5. ONE Pose_graph.solve over the loops the round accepted, then ONE Map_refine.refine over all their selections (every second
         key frame, newest first, at map_refinement_resolution), split back into each assembly's `refined`.
    A solve that raises leaves its loops in the assemblies' pending_loops; the next run solves them first."""

    def __init__(self, assemblies, bank=False, pose_graph=False, map_refinement=False, store=None):
        self.assemblies, self.store = list(assemblies), store
        device = self.assemblies[0].device
        self.bank, self.pose_graph = _Service("Keyframe_bank", bank, device), _Service("Pose_graph", pose_graph, device)
        self.map_refine = _Service("Map_refine", map_refinement, device)
        for ka in self.assemblies:
            ka.rounds = self

    def close(self):
        for service in (self.bank, self.pose_graph, self.map_refine):
            service.close()

    def run(self, slots, limit: int | None = None) -> list:
        """rounds while a named slot has a key frame waiting and has not ended (at most `limit` of them, when given).  Returns the
        loops found, a list per named slot."""
        found = [[] for _ in slots]
        while True:
            todo = [k for k, s in enumerate(slots) if self.assemblies[s].m_keyframe_need_precession_list and not self.assemblies[s].if_end
                    and (limit is None or limit > 0)]
            kas = [self.assemblies[slots[k]] for k in todo]
            if kas and self.store is not None:
                self.extract([slots[k] for k in todo])
            self.analyse(kas)
            for k, ka, sims in zip(todo, kas, self.match(kas)):
                found[k] += ka.walk_front(sims)
            pending = [(self.assemblies[s], loop) for s in slots for loop in self.assemblies[s].pending_loops]
            self.close_loops(pending)
            for ka, _ in pending:
                ka.pending_loops.clear()
            if not todo:
                return found
            limit = None if limit is None else limit - 1

    def extract(self, slots) -> None:
        """the first waiting key frame of every slot out of the store in one call, each handed to its assembly for its next materialize"""
        kas = [self.assemblies[s] for s in slots]
        fronts = [ka.m_keyframe_need_precession_list[0] for ka in kas]
        wants = [ka.wanted_cells(kf) for ka, kf in zip(kas, fronts)]
        dsts = [ka.new_keyframe_map(len(w)) for ka, w in zip(kas, wants)]
        try:
            self.store.extract_cells(2, list(slots), wants, dsts)
        except Exception:
            for km in dsts:
                km.close()
            raise
        for ka, kf, km in zip(kas, fronts, dsts):
            ka.prefetch(kf, km)

    def analyse(self, kas) -> list:
        """the analysis half for every assembly named, and their key frames' accumulated clouds out of the scan log into the store in one
        add_logged (laser_mapping.hpp:943-946 for each).  Returns every assembly's candidates."""
        candidates = [ka._analyse() for ka in kas]
        logged = [ka for ka in kas if ka.map_refinement and ka.scan_log is not None]
        if logged:
            fronts = [ka._front[0] for ka in logged]
            ids, _, _ = self.map_refine().add_logged(logged[0].scan_log.batch, [kf.m_accumulated_point_cloud for kf in fronts],
                                                     logged[0].surround_pointcloud_resolution)
            for kf, cloud_id in zip(fronts, ids):
                kf.cloud_id, kf.m_accumulated_point_cloud = int(cloud_id), []
        return candidates

    def match(self, kas) -> list:
        """(sim_line, sim_plane) of every assembly's candidates out of one Keyframe_bank.match; None for an assembly without candidates,
        and for all without a bank (the walk then asks keyframe_similarity per pair)"""
        if not self.bank.on:
            return [None] * len(kas)
        pairs = [ka.front_pairs() for ka in kas]
        cut = np.cumsum([0] + [len(a) for a, _ in pairs])
        line, plane = self.bank().match([i for a, _ in pairs for i in a], [i for _, b in pairs for i in b]) if cut[-1] else ((), ())
        return [(line[cut[k]:cut[k + 1]], plane[cut[k]:cut[k + 1]]) if pairs[k][0] else None for k in range(len(kas))]

    def close_loops(self, todo) -> None:
        """todo: [(assembly, accepted loop)].  Their pose graphs optimised in one solve (:1058-1089), every assembly keeping its
        solution, and with map_refinement the maps behind them refined in one run (:1091-1100)."""
        if not todo:
            return
        graphs = [ka.loop_graph(loop) for ka, loop in todo]
        poses, summaries = self.pose_graph().solve(graphs)
        for (ka, _), graph, x, summary in zip(todo, graphs, poses, summaries):
            ka._keep_solution(graph, x, summary)
        self.refine([ka for ka, _ in todo if ka.map_refinement])

    def refine(self, kas) -> None:
        """Keyframe_assembly.refine_map for every assembly named, in one Map_refine.refine: key frames K - 1, K - 3, ... >= 0 of each"""
        if not kas:
            return
        ids = [list(range(len(ka.poses_ori) - 1, -1, -2)) for ka in kas]
        clouds = self.map_refine().refine([ka.keyframe_vec[k].cloud_id for ka, sel in zip(kas, ids) for k in sel],
                                          np.concatenate([ka.poses_ori[sel] for ka, sel in zip(kas, ids)]),
                                          np.concatenate([ka.poses_opm[sel] for ka, sel in zip(kas, ids)]), kas[0].map_refinement_resolution, False)
        cut = np.cumsum([0] + [len(sel) for sel in ids])
        for k, (ka, sel) in enumerate(zip(kas, ids)):
            ka.refined = list(zip(sel, clouds[cut[k]:cut[k + 1]]))


def _pose7(q, t) -> np.ndarray:
    return np.concatenate([np.asarray(q, np.float64).reshape(4), np.asarray(t, np.float64).reshape(3)])


def _pack_cells(cell_ijk) -> np.ndarray:
    """(i, j, k) cell indices -> one int64 per cell (21 bits per axis, like the device's cell key)"""
    c = np.asarray(cell_ijk, np.int64).reshape(-1, 3) + (1 << 20)
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def _unpack_cells(packed) -> np.ndarray:
    """_pack_cells' int64 form -> (i, j, k) int32 [n, 3]"""
    p = np.asarray(packed, np.int64).reshape(-1)
    return (np.stack([p, p >> 21, p >> 42], axis=1) & 0x1fffff).astype(np.int32) - (1 << 20)


def _close(cm) -> None:
    if hasattr(cm, "close"):
        cm.close()


def _quat_rot(q, v):
    """rotate v by the unit quaternion q = {x, y, z, w}"""
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R @ np.asarray(v, np.float64)
