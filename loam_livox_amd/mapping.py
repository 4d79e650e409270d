"""Host-side mirror of Laser_mapping::process_new_scan for both match modes (m_matching_mode == 0: history,
1: cell map), hku-mars/loam_livox source/laser_mapping.hpp:1311-1520, on top of the C ABI: extractor -> (VoxelGrid)
-> registrar -> history / cell maps -> match-buffer refresh, everything resident on one device.

This is the unit of BASELINE config C4 (one sequence per GPU, local map growth).  Differences from the node, by design:
  * the match buffer is refreshed synchronously after every accepted frame; the node refreshes it on a service thread
    and registers against whichever buffer is newest (laser_mapping.hpp:568-594, 1395-1403), which makes its output
    depend on thread timing;
  * no ROS or logging; the full-cloud cell map, the key frames and the front half of loop detection are optional
    (loop_closure_if_enable, keyframes.py), with loop_closure["pose_graph"] the pose-graph optimisation of an accepted loop and
    loop_closure["map_refinement"] the corrected key-frame clouds behind it (keyframes.refined); the file dumps are out of scope.
"""
from __future__ import annotations

import numpy as np

from .api import (History_buffer, History_buffer_batch, Livox_laser, Map_buffer, Point_cloud_registration, Spinning_laser, VoxelGrid,
                  information_in_pose_frame)


def _set_registrar_params(p, *, scan_points, icp_max_iterations, ceres_max_iterations, max_allow_incre_R, max_allow_incre_T, max_allow_final_cost,
                          init_accumulate_frames, minimum_icp_R_diff, minimum_icp_T_diff, maximum_residual_blocks, subsample_seed, **others) -> None:
    """the registrar's parameters from the arguments of Laser_mapping of the same names (others: the arguments the registrar does not take)"""
    p.icp_max_iterations, p.ceres_max_iterations = icp_max_iterations, ceres_max_iterations
    p.para_max_angular_rate, p.para_max_speed, p.max_final_cost = max_allow_incre_R, max_allow_incre_T, max_allow_final_cost
    p.mapping_init_accumulate_frames = init_accumulate_frames
    p.minimum_icp_R_diff, p.minimum_icp_T_diff = minimum_icp_R_diff, minimum_icp_T_diff  # PCR:94-95
    # optimization/maximum_residual_blocks (200 in the shipped configs): sub-sampling on a reproducible stream; 0 = keep all
    p.maximum_allow_residual_block = maximum_residual_blocks if maximum_residual_blocks > 0 else scan_points
    p.subsample_seed = subsample_seed if maximum_residual_blocks > 0 else 0


def _with_pose_frame(info: dict, pose_last) -> dict:
    """a registrar's information record plus H_pose: H in the frame of the pose the registration started from (translation, then rotation vector)"""
    info = dict(info)
    info["H_pose"] = information_in_pose_frame(info["H"], pose_last)
    return info


def _degenerate_directions(info: dict, min_eigenvalue: float) -> np.ndarray:
    weak = info["eigenvalues"] < float(min_eigenvalue)
    return np.ascontiguousarray(info["eigenvectors"][:, weak].T)


def _point_time_stamp(current_time: float, idx, time_internal_pts: float):
    """the extractor's stamp of point idx (livox_feature_extractor.hpp:482; ll_fe_core.h point_time_stamp), operation for operation;
    idx: one position or an array of them -> float32"""
    return (np.float64(current_time) + (np.asarray(idx).astype(np.float32) * np.float32(time_internal_pts)).astype(np.float64)).astype(np.float32)


class Laser_mapping:
    """lidar_type (common/lidar_type of the feature node, laser_feature_extractor.hpp:831-851): "livox" (default) runs the Livox
    extractor; any other value runs the spinning-lidar one (scan_line 16 or 64, minimum_range, mapping_plane_resolution: the feature
    node's parameters) and hands its less-sharp / less-flat clouds to the registrar and the history on the device
    (Point_cloud_registration.enqueue_spin, History_buffer.add_spin): extract -> resolve -> register -> history -> refresh, with the
    same prefetch of the next scan on a second handle.  The reference's mapping node has no spinning input; the cloud choice is the
    project's.  Spinning lidars run in history mode (matching_mode 0) only: cell-map matching, keep_cell_maps and
    loop closure are refused at construction with a ValueError, and process_clouds stays the Livox node path."""

    def __init__(self, scan_points: int = 24000, device: int = 0, maximum_history_size: int = 100, line_res: float = 0.1,
                 plane_res: float = 0.4, init_accumulate_frames: int = 50, input_downsample_mode: int = 1, icp_max_iterations: int = 20,
                 ceres_max_iterations: int = 100, max_allow_incre_R: float = 200.0 / 50.0, max_allow_incre_T: float = 100.0 / 50.0,
                 max_allow_final_cost: float = 100.0, history_add_t_step: float = 0.0, history_add_angle_step: float = 0.0,
                 minimum_icp_R_diff: float = 0.01, minimum_icp_T_diff: float = 0.01, maximum_residual_blocks: int = 0,
                 subsample_seed: int = 1, matching_mode: int = 0, cell_resolution: float = 1.0, threshold_cell_revisit: int = 5000,
                 maximum_search_range_corner: float = 100.0, maximum_search_range_surface: float = 100.0,
                 maximum_in_fov_angle: float = 30.0, down_sample_replace: int = 1, cell_map_max_points: int = 1 << 21,
                 loop_closure_if_enable: int = 0, loop_closure: dict | None = None, keep_cell_maps: bool = False,
                 lidar_type: str = "livox", scan_line: int = 16, minimum_range: float = 0.1, mapping_plane_resolution: float = 0.8,
                 information: bool = False, if_motion_deblur: int = 0, if_undistort: int = 0):
        self.lidar_type = lidar_type
        self._spin = lidar_type != "livox"
        # if_motion_deblur: the registrar's switch and the frame's time range (laser_mapping.hpp:1336-1347).  if_undistort: g_if_undistore --
        # the history frames, the full cloud and the published clouds move with the pose interpolated at every point's time stamp
        # (:1424,1430,1442).  Both 0: the loop makes exactly the calls it makes without them.
        self.if_motion_deblur, self.if_undistort = int(bool(if_motion_deblur)), int(bool(if_undistort))
        if self._spin and (self.if_motion_deblur or self.if_undistort):
            raise ValueError(f'lidar_type "{lidar_type}" (spinning lidar): if_motion_deblur and if_undistort must be 0 -- the spinning extractor\'s '
                             "intensity is scanID + scanPeriod * relTime (laser_feature_extractor.hpp:502), no time stamp")
        if self._spin:
            if matching_mode or keep_cell_maps or loop_closure_if_enable:
                raise ValueError(f'lidar_type "{lidar_type}" (spinning lidar) runs in history mode only: matching_mode, keep_cell_maps and '
                                 "loop_closure_if_enable must be 0")
            self._spin_args = dict(scan_line=scan_line, minimum_range=minimum_range, plane_resolution=mapping_plane_resolution,
                                   max_points=scan_points, max_scans=1, max_line_points=min(scan_points, 8192), device=device)
        self.fe = self._new_extractor(scan_points, device)
        # The feature node and the mapping node are separate processes in the reference: scan k + 1 is extracted while scan k is
        # registered.  process_new_scan( scan, next_xyzi = ... ) does the same with a second extractor handle (own stream): the next
        # scan's upload, extraction and selection are issued between this scan's enqueue and its collect.
        self._fe_pair = [self.fe, None]
        self._prefetched = None  # (the array object that was prefetched, its time stamp, handle)
        self._scan_points, self._device = scan_points, device
        self.reg = Point_cloud_registration(max_scans=1, max_features=scan_points, device=device)
        # information: every frame's registration also leaves the Gauss-Newton matrix of its last linearisation (last_information:
        # Point_cloud_registration.information()'s dict plus H_pose, the same in the pose's own frame); poses are the same bits either way
        self._information = bool(information)
        self.last_information = None
        if self._information:
            self.reg.set_information(True)
        self.map = Map_buffer(device=device)
        self.vox = (VoxelGrid(scan_points, 1, device=device), VoxelGrid(scan_points, 1, device=device))
        self.history = History_buffer(maximum_history_size, scan_points, line_res, plane_res, device=device)
        self.line_res, self.plane_res = line_res, plane_res
        # mapping/matching_mode (laser_mapping.hpp:689; 0 in the shipped configs): 1 = match against the cell maps
        self.m_matching_mode = matching_mode
        self.m_maximum_search_range = (maximum_search_range_corner, maximum_search_range_surface)  # :694-695
        self.m_maximum_in_fov_angle = maximum_in_fov_angle                                           # :691
        self.m_down_sample_replace = down_sample_replace                                             # :277
        # m_pt_cell_map_corners / m_pt_cell_map_planes receive every registered frame in BOTH match modes (:1492-1493); only mode 1 reads
        # them per frame.  keep_cell_maps: maintain them in mode 0 too -- the sub-map a batched map-building job hands over at its end
        # (BASELINE config C4, bench_c4.py); they grow with the sequence (ll_cellmap_reserve)
        self.keep_cell_maps = bool(matching_mode or keep_cell_maps)
        if self.keep_cell_maps:
            self.history.enable_cell_map(cell_map_max_points, cell_resolution, threshold_cell_revisit)  # :620-624
            if not matching_mode:  # nothing reads them between frames: fed by the handle's service thread, beside the loop
                self.history.set_cell_map_async(True)
        self.m_if_input_downsample_mode = input_downsample_mode
        self.history_add_t_step, self.history_add_angle_step = history_add_t_step, history_add_angle_step
        _set_registrar_params(self.reg.params, scan_points=scan_points, icp_max_iterations=icp_max_iterations, ceres_max_iterations=ceres_max_iterations,
                              max_allow_incre_R=max_allow_incre_R, max_allow_incre_T=max_allow_incre_T, max_allow_final_cost=max_allow_final_cost,
                              init_accumulate_frames=init_accumulate_frames, minimum_icp_R_diff=minimum_icp_R_diff,
                              minimum_icp_T_diff=minimum_icp_T_diff, maximum_residual_blocks=maximum_residual_blocks, subsample_seed=subsample_seed)
        if self.if_motion_deblur:
            self.reg.params.if_motion_deblur = 1
        self.m_current_frame_index = 0
        self.pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)  # m_q_w_curr / m_t_w_curr
        self.map_sizes = (0, 0)
        self.last_report = None
        self.aborted_solves = 0     # registrations abandoned by the grouped solver and repeated on one workgroup (ll_reg_report.aborted)
        self.stage_s = np.zeros(4)  # cumulative wall time: extract+register, history add, match-buffer refresh, frames
        self.m_last_time_stamp = 0.0
        self._host_vox = None
        # loop_closure/if_enable_loop_closure (laser_mapping.hpp:698; 0 in the shipped Mid-40 configs): the full-cloud cell map, the key frames
        # and the front half of loop detection (keyframes.py; laser_mapping.hpp:626, 1524-1562, 919-1060)
        # (loop_closure: Keyframe_assembly's settings as they are, device_alignment=True -- candidate pairs aligned without a host hop -- and
        #  device_bank=True -- the key frames' images kept on the device, one similarity call per closed key frame -- among them)
        self.keyframes = None
        self.loops = []
        self.full_map_s = 0.0  # cumulative wall time of the full-map and key-frame part of the frames (part of stage_s[1])
        if loop_closure_if_enable:
            from .keyframes import Keyframe_assembly
            self.keyframes = Keyframe_assembly(device=device, cell_resolution=cell_resolution, threshold_cell_revisit=threshold_cell_revisit,
                                               **{"maximum_history_size": maximum_history_size, **(loop_closure or {})})

    def close(self):
        for h in tuple(f for f in self._fe_pair if f is not None) + (self.reg, self.map, self.vox[0], self.vox[1], self.history):
            h.close()
        if self.keyframes is not None:
            self.keyframes.close()

    def _keyframe_step(self, full_xyzi: np.ndarray, history_added: bool = True) -> None:
        """laser_mapping.hpp:1442 + 1524-1562 (+ the detector's loop body for whatever key frame that closed): the scan's full cloud,
        moved into the map frame with the accepted pose, goes into the full cell map and the open key frames.  history_added: what the
        history's add answered for this scan (:1446-1448) -- the scan's full cloud joins m_laser_cloud_full_history with it (:1456)"""
        full = np.ascontiguousarray(full_xyzi, np.float32)
        full = full[np.isfinite(full[:, :3]).all(axis=1)]
        if self.if_undistort:  # :1442, pointcloudAssociateToMap( full, full_out, g_if_undistore )
            cloud = self.reg.pointcloudAssociateToMap(full, self.pose, if_undistore=1) if len(full) else full
        else:
            cloud = self.reg.pointcloudAssociateToMap(full, self.pose) if len(full) else full
        self.keyframes.add_scan(cloud, self.pose, self.m_current_frame_index, history_added=history_added)
        self.loops += self.keyframes.process_waiting()

    def _read_information(self, pose_last) -> None:
        """the record of the registration just collected, with H in the frame of the pose it started from"""
        if self._information:
            self.last_information = _with_pose_frame(self.reg.information(1)[0], pose_last)

    def degenerate_directions(self, min_eigenvalue: float) -> np.ndarray:
        """The eigenvectors [k, 6] of the last frame's H (solver tangent [d_rot; d_t]) whose eigenvalue lies below min_eigenvalue: the
        directions the frame's registration left unconstrained.  The caller names the value: rotation and translation rows carry
        different units, so any built-in threshold would be a guess."""
        if self.last_information is None:
            raise RuntimeError("degenerate_directions needs information=True and a registered frame")
        return _degenerate_directions(self.last_information, min_eigenvalue)

    def sync(self) -> None:
        """every frame handed to the cell maps' service thread has been appended (keep_cell_maps in matching mode 0)"""
        if self.keep_cell_maps:
            self.history.sync_cell_maps()

    def _new_extractor(self, scan_points, device):
        if self._spin:
            return Spinning_laser(**self._spin_args)
        return Livox_laser(max_points=scan_points, max_scans=1, device=device, piecewise_number=1)

    def _extract(self, fe, xyzi, time_stamp):
        if self._spin:  # laserCloudHandler :393-776; the time stamp plays no part in this branch
            fe.upload([xyzi])
            fe.extract_batch_async(1)
            fe.resolve()
            return
        fe.upload(xyzi[None], np.full(1, time_stamp))
        fe.extract_batch(1)
        fe.resolve()
        fe.select_batch(1, -1, 0.0, 1.0)

    def _enqueue(self, fe, pose):
        reg = self.reg
        if self._spin:
            if self.m_if_input_downsample_mode:  # :1367-1373
                reg.enqueue_spin_downsampled(self.map, fe, self.vox[0], self.vox[1], self.line_res, self.plane_res, 1, pose, pose)
            else:
                reg.enqueue_spin(self.map, fe, 1, pose, pose)
        elif self.m_if_input_downsample_mode:  # :1367-1373
            reg.enqueue_fe_downsampled(self.map, fe, self.vox[0], self.vox[1], self.line_res, self.plane_res, 1, pose, pose)
        else:
            reg.enqueue_fe(self.map, fe, 1, pose, pose)

    def process_new_scan(self, xyzi: np.ndarray, time_stamp: float = 1.0, next_xyzi: np.ndarray | None = None, next_time_stamp: float = 1.0,
                         scan_id=None, next_scan_id=None) -> int:
        """One frame (laser_mapping.hpp:1311-1520).  Returns the registration result (1 accepted, 0 rejected).
        next_xyzi: the scan that will be passed next, extracted on the second handle while this one registers.  The prefetched extraction
        is used by the next call only if it is recognisably the same scan: the caller's token (scan_id of that call == next_scan_id of
        this one) when tokens are given -- the contract for callers that refill one buffer in place, e.g. a ring filled by a driver thread
        -- otherwise the same array OBJECT with the same time stamp, which the caller must then not have rewritten in between."""
        try:
            return self._process_new_scan(xyzi, time_stamp, next_xyzi, next_time_stamp, scan_id, next_scan_id)
        except Exception:
            self._prefetched = None  # (a failure between the prefetch and its use must not leave a stale extraction behind)
            raise

    def _process_new_scan(self, xyzi, time_stamp, next_xyzi, next_time_stamp, scan_id, next_scan_id) -> int:
        import time
        t0 = time.perf_counter()
        reg = self.reg
        pf = self._prefetched
        self._prefetched = None
        hit = pf is not None and pf[1] == time_stamp and ((scan_id is not None and pf[3] is not None and pf[3] == scan_id) or
                                                           (scan_id is None and pf[3] is None and pf[0] is xyzi))
        if hit:
            fe = pf[2]
        else:
            fe = self._fe_pair[0]
            self._extract(fe, xyzi, time_stamp)
        self.fe = fe  # the handle that holds this frame's features (history add, key frames)
        if self.if_motion_deblur:  # find_min_max_intensity( full ), :1336-1347: from the previous frame's last stamp to this frame's
            full_idx = fe.full_selection(0)  # (ascending: the last one carries the largest stamp)
            max_t = float(_point_time_stamp(time_stamp, int(full_idx[-1]), fe.params.time_internal_pts)) if len(full_idx) else 0.0
            reg.params.minimum_pt_time_stamp, reg.params.maximum_pt_time_stamp = self.m_last_time_stamp, max_t
            self.m_last_time_stamp = max_t
        reg.params.current_frame_index = self.m_current_frame_index  # init_pointcloud_registration runs before the increment
        self.m_current_frame_index += 1
        pose = self.pose[None]
        self._enqueue(fe, pose)
        if next_xyzi is not None:  # the next frame's extraction runs beside this frame's ICP kernels
            other = 1 if fe is self._fe_pair[0] else 0
            if self._fe_pair[other] is None:
                self._fe_pair[other] = self._new_extractor(self._scan_points, self._device)
            self._extract(self._fe_pair[other], next_xyzi, next_time_stamp)
            self._prefetched = (next_xyzi, next_time_stamp, self._fe_pair[other], next_scan_id)
        res, pc, _, reps = reg.collect(1)
        self._read_information(self.pose)
        flags = getattr(reg, "debug_flags", 0)
        if reps[0].aborted:
            self.aborted_solves += 1
        if reps[0].aborted and not (flags & 32):
            # not a rejection the reference would have made: a bounded wait of the grouped solver ran out (the device was oversubscribed,
            # e.g. by the prefetched extraction beside it).  Counted apart, and the scan is registered once more on one workgroup -- with
            # the caller's other debug / A-B flags left as they are.  (An abort with the groups already off has another cause -- the small
            # solver could not hold the scan -- which a repeat would not cure: the scan stays rejected.)
            reg.set_debug_flags(flags | 32)
            self._enqueue(fe, pose)
            res, pc, _, reps = reg.collect(1)
            self._read_information(self.pose)  # the repeat's record replaces the aborted one
            reg.set_debug_flags(flags)
        self.last_report = reps[0]
        t1 = time.perf_counter()
        self.stage_s[0] += t1 - t0
        self.stage_s[3] += 1
        if not res[0]:  # :1413-1416
            return 0
        self.history.set_gate_pose(self.pose)  # m_q_w_curr is still the pre-registration pose at LM:1439-1451
        if self.if_undistort:
            self.history.set_undistort(reg, 0)  # :1424,1430
        if self.m_if_input_downsample_mode:
            added = self.history.add_voxel(self.vox[0], self.vox[1], 0, pc[0], self.history_add_t_step, self.history_add_angle_step)
        elif self._spin:
            added = self.history.add_spin(fe, 0, pc[0], self.history_add_t_step, self.history_add_angle_step)
        else:
            added = self.history.add_fe(fe, 0, pc[0], self.history_add_t_step, self.history_add_angle_step)
        self.pose = pc[0].copy()  # :1496-1500
        if self.keyframes is not None:
            tk = time.perf_counter()
            full_idx = fe.get_features(0.0, 1.0)["full_idx"]
            full = np.asarray(xyzi, np.float32)[full_idx]  # /pc2_full of this scan
            if self.if_undistort:  # the feature node publishes it with intensity := time stamp (LFE:246,255), which the deskew reads
                full = full.copy()
                full[:, 3] = _point_time_stamp(time_stamp, full_idx, fe.params.time_internal_pts)
            self._keyframe_step(full, bool(added))
            self.full_map_s += time.perf_counter() - tk
        t2 = time.perf_counter()
        if self.m_matching_mode:  # update_buff_for_matching (service thread in the node), synchronous here
            self.map_sizes = self.history.refresh_cells(self.map, self.pose, self.m_maximum_search_range[0], self.m_maximum_search_range[1],
                                                        self.m_maximum_in_fov_angle, self.m_down_sample_replace)
        else:
            self.map_sizes = self.history.refresh(self.map)
        t3 = time.perf_counter()
        self.stage_s[1] += t2 - t1
        self.stage_s[2] += t3 - t2
        return 1

    def process_clouds(self, full: np.ndarray, surface: np.ndarray, corners: np.ndarray) -> int:
        """process_new_scan as the mapping NODE runs it (laser_mapping.hpp:1316-1520): from the three clouds the
        feature node published (/pc2_full, /pc2_surface, /pc2_corners; feature_node.Laser_feature.laserCloudHandler),
        host clouds in, through the same C-ABI entry points tools/ll_node.cpp reaches through the adapter."""
        reg = self.reg
        max_t = float(np.max(full[:, 3])) if len(full) else 0.0  # find_min_max_intensity( full ), :1336
        reg.params.minimum_pt_time_stamp, reg.params.maximum_pt_time_stamp = self.m_last_time_stamp, max_t  # :1345-1346
        self.m_last_time_stamp = max_t
        reg.params.current_frame_index = self.m_current_frame_index
        self.m_current_frame_index += 1
        if self.m_if_input_downsample_mode:  # :1367-1373
            if self._host_vox is None:
                cap = int(self.fe.params.max_points)
                self._host_vox = (VoxelGrid(cap, 1), VoxelGrid(cap, 1))
                self._host_vox[0].setLeafSize(*([self.line_res] * 3))
                self._host_vox[1].setLeafSize(*([self.plane_res] * 3))
            stacks = []
            for vg, cloud in zip(self._host_vox, (corners, surface)):
                if len(cloud):
                    vg.setInputCloud(cloud)
                    cloud = vg.filter()
                stacks.append(cloud)
            corner_stack, surf_stack = stacks
        else:
            corner_stack, surf_stack = corners, surface
        self.stack_sizes = (len(corner_stack), len(surf_stack))
        reg.m_pose_w_last = self.pose.copy()
        reg.m_pose_w_curr = self.pose.copy()
        reg.m_para_buffer_incremental = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)  # a fresh Point_cloud_registration per scan (:1348)
        res = reg.find_out_incremental_transfrom(self.map, corner_stack, surf_stack)
        self._read_information(self.pose)
        self.last_report = reg.report
        if not res:  # :1413-1416
            return 0
        self.history.set_gate_pose(self.pose)  # m_q_w_curr is still the pre-registration pose at LM:1439-1451
        self.pose = np.array(reg.m_pose_w_curr, np.float64)
        if self.if_undistort:
            self.history.set_undistort(reg, 0)  # :1424,1430
        added = self.history.add(corner_stack, surf_stack, self.pose, self.history_add_t_step, self.history_add_angle_step)
        if self.keyframes is not None:
            self._keyframe_step(full, bool(added))
        self.map_sizes = self.history.refresh(self.map)
        return 1


class _History_slot:
    """slot s of a History_buffer_batch, read the way a History_buffer is: len() and map_cloud(kind)"""

    def __init__(self, batch: "History_buffer_batch", sequence: int):
        self.batch, self.sequence = batch, sequence

    def __len__(self):
        return self.batch.size(self.sequence)

    def map_cloud(self, kind: int) -> np.ndarray:
        return self.batch.map_cloud(self.sequence, kind)


class Laser_mapping_batch:
    """n_sequences independent Laser_mapping loops advanced in lock step (BASELINE config C4: batched offline map building from
    independent sub-sequences with local map growth).  Frame k of all sequences is ONE batch: one batched extraction, one VoxelGrid
    pair over all slots, one registration in which slot s is searched and solved against sequence s's own match buffer
    (Point_cloud_registration.enqueue_fe[_downsampled]_maps), then per sequence the history add and the match-buffer refresh --
    those on a small pool of host threads (refresh_threads; every history has its own stream), because a refresh drains its stream
    four times and S of them on one thread would serialise.

    Per sequence this is Laser_mapping._process_new_scan line for line -- the frame index handed to the gate, the gate pose of the
    add rule, the repeat of an aborted grouped solve on one workgroup -- and gives the same bits as a Laser_mapping run alone on that
    sequence.  Takes the arguments of Laser_mapping; Livox scans only, in history mode unless cell_matching=True (below): lidar_type
    other than "livox", matching_mode, loop_closure_if_enable and keep_cell_maps raise ValueError.

    if_motion_deblur=1 registers every sequence with the reference's *_mb problem over its own time range -- from its previous frame's
    last stamp to this frame's (m_last_time_stamp[s]; one Livox_laser.selection_last and one Point_cloud_registration.set_time_ranges per
    enqueue) -- and if_undistort=1 builds every sequence's match buffer from deskewed clouds (History_buffer.set_undistort per sequence,
    or one History_buffer_batch.set_undistort): Laser_mapping(if_motion_deblur=1, if_undistort=1) per sequence, bit for bit.
    if_undistort=1 with full_maps=True raises ValueError.

    batched_history=True keeps all histories in ONE History_buffer_batch: the slots a step accepted go through one add and one
    refresh, whose launches and host waits do not grow with n_sequences (no thread pool, no per-sequence handles; refresh_threads is
    ignored).  Same bits per sequence; histories[s] is then a view of slot s that offers len() and map_cloud(kind).

    cell_maps=True (with batched_history=True only) keeps the two cell maps of every sequence on the History_buffer_batch -- the
    sub-map a sequence hands over at its end, what Laser_mapping(keep_cell_maps=True) keeps for one sequence -- under
    cell_map_max_points (the points per map the store starts with, 2^18 unless given; it grows), cell_resolution and threshold_cell_revisit.  Every
    accepted frame is appended; poses and results do not change by a bit.  sync() puts the stores in order, cell_map(s, kind) reads
    one (stats(), dump(), device_view(device) as api.Cell_map has them).  keep_cell_maps itself stays refused: it names
    Laser_mapping's per-sequence maps and their service thread.

    cell_matching=True (with cell_maps=True only) registers against those cell maps: the step's one refresh becomes one refresh_cells
    at the accepted slots' new poses -- the cells within maximum_search_range_corner / _surface and maximum_in_fov_angle, each through
    the VoxelGrid, replaced by their leaves with down_sample_replace -- which is Laser_mapping(matching_mode=1) per sequence, bit for
    bit.  matching_mode itself stays refused: it names Laser_mapping's per-sequence route.

    full_maps=True (with batched_history=True only) keeps the full-cloud map of every sequence -- m_pt_cell_map_full, the un-filtered
    cloud of every accepted scan in the map frame (laser_mapping.hpp:1442, 1527), what Laser_mapping(loop_closure_if_enable=1) keeps
    for one sequence -- on the History_buffer_batch: one append_full per step for the accepted slots at their new poses, after the
    add.  The store starts at loop_closure["max_points"] points per map (2^18 unless given; it grows) under cell_resolution and
    threshold_cell_revisit; full_map(s) reads slot s (stats(), dump()).  key_frames=True (with full_maps=True only) also owns one
    keyframes.Keyframe_assembly per sequence, built with the rest of loop_closure, on top of its slot: per accepted slot add_scan with
    the new pose and the slot's frame index after the increment, as Laser_mapping._keyframe_step does; then ONE keyframes.Keyframe_rounds
    (rounds) over the S assemblies processes the key frames the slots closed, a round at a time, out of the batched store; keyframes[s]
    and loops[s] are those of Laser_mapping run alone on sequence s.  Nothing of the registration reads the full maps: poses and reports
    do not change by a bit.  loop_closure_if_enable itself stays refused: it names Laser_mapping's per-sequence map.  The options of
    loop_closure below are off by default, and what each does in a round is told in Keyframe_rounds:
    loop_closure["device_bank"]=True: ONE api.Keyframe_bank (keyframe_bank) for the S assemblies, one match per round.
    loop_closure["pose_graph"]=True: ONE api.Pose_graph (pose_graph) for the S assemblies, one solve per round.
    loop_closure["map_refinement"]=True (with batched_history, full_maps, key_frames and loop_closure["pose_graph"] only -- every other
    configuration raises ValueError): ONE api.Map_refine (map_refine) for the S assemblies and a scan log on the History_buffer_batch
    (enable_scan_log: m_laser_cloud_full_history of every slot, laser_mapping.hpp:1456, in device blocks), so that no full cloud reaches
    the host.  A step is then append_full, ONE log_full for the accepted slots whose history add let the scan in (:1456 before :1524),
    the slots' add_scan -- whose flush is a hand-over of the slot's FIFO -- and the rounds: one add_logged and one refine each."""

    def __init__(self, n_sequences: int, refresh_threads: int | None = None, batched_history: bool = False, cell_maps: bool = False,
                 cell_matching: bool = False, full_maps: bool = False, key_frames: bool = False, **kw):
        import inspect
        sig = inspect.signature(Laser_mapping.__init__)
        unknown = set(kw) - set(sig.parameters)
        if unknown:
            raise TypeError(f"unexpected argument(s) {sorted(unknown)}: Laser_mapping_batch takes the arguments of Laser_mapping")
        a = {k: p.default for k, p in sig.parameters.items() if k != "self"}
        a.update(kw)
        if n_sequences < 1:
            raise ValueError("n_sequences must be at least 1")
        if a["lidar_type"] != "livox":
            raise ValueError(f'lidar_type "{a["lidar_type"]}": the batched loop takes Livox scans only')
        if a["matching_mode"]:
            raise ValueError("matching_mode is not offered by the batched loop (cell_maps=True, cell_matching=True matches against the cell "
                             "maps on the batched history)")
        if a["loop_closure_if_enable"]:
            raise ValueError("loop_closure_if_enable must be 0 in the batched loop")
        if (a["loop_closure"] or {}).get("map_refinement") and not (batched_history and full_maps and key_frames and a["loop_closure"].get("pose_graph")):
            raise ValueError("map_refinement is not available in the batched loop without batched_history=True, full_maps=True, "
                             "key_frames=True and loop_closure pose_graph: its full clouds never reach the host, they wait in the "
                             "scan log of the History_buffer_batch")
        if a["keep_cell_maps"]:
            raise ValueError("keep_cell_maps is not offered by the batched loop (cell_maps=True keeps them on the batched history)")
        if cell_maps and not batched_history:
            raise ValueError("cell_maps=True needs batched_history=True: the cell maps live on the History_buffer_batch")
        if cell_matching and not cell_maps:
            raise ValueError("cell_matching=True needs cell_maps=True: the cell mode matches against the cell maps of the History_buffer_batch")
        if full_maps and not batched_history:
            raise ValueError("full_maps=True needs batched_history=True: the full-cloud maps live on the History_buffer_batch")
        if key_frames and not full_maps:
            raise ValueError("key_frames=True needs full_maps=True: a key frame is a set of cells of the sequence's full-cloud map")
        # if_motion_deblur / if_undistort: Laser_mapping's switches per sequence (class docstring).  Both 0: the loop makes exactly the
        # calls it makes without them.
        self.if_motion_deblur, self.if_undistort = int(bool(a["if_motion_deblur"])), int(bool(a["if_undistort"]))
        if self.if_undistort and full_maps:
            raise ValueError("if_undistort=1 is not available with full_maps=True (and so not with key frames, loop closure or map "
                             "refinement) in the batched loop: the append of the full selections and the scan log would need the full "
                             "cloud with intensity := time stamp on the device; if_motion_deblur=1 alone is")
        if refresh_threads is None:
            refresh_threads = min(4, n_sequences)
        if not 1 <= int(refresh_threads) <= 16:
            raise ValueError("refresh_threads must be between 1 and 16")
        S, scan_points, device = int(n_sequences), a["scan_points"], a["device"]
        self.n_sequences, self.refresh_threads = S, int(refresh_threads)
        self._scan_points = scan_points
        self.fe = Livox_laser(max_points=scan_points, max_scans=S, device=device, piecewise_number=1)
        self.reg = Point_cloud_registration(max_scans=S, max_features=scan_points, device=device)
        self._information = bool(a["information"])  # Laser_mapping's: last_information[s] is slot s's record of its last frame
        self.last_information = [None] * S
        if self._information:
            self.reg.set_information(True)
        self.vox = (VoxelGrid(scan_points, S, device=device), VoxelGrid(scan_points, S, device=device))
        self.maps = [Map_buffer(device=device) for _ in range(S)]
        self.batched_history, self.cell_maps, self.cell_matching = bool(batched_history), bool(cell_maps), bool(cell_matching)
        self.full_maps, self.key_frames = bool(full_maps), bool(key_frames)
        self.keyframes, self.loops, self.rounds, self.keyframe_bank, self.pose_graph, self.map_refine = None, None, None, None, None, None
        self.full_map_s = 0.0  # cumulative wall time of the full-map phase (append_full, and the key-frame steps with key_frames)
        self.m_maximum_search_range = (a["maximum_search_range_corner"], a["maximum_search_range_surface"])
        self.m_maximum_in_fov_angle, self.m_down_sample_replace = a["maximum_in_fov_angle"], a["down_sample_replace"]
        if self.batched_history:
            self.history_batch = History_buffer_batch(S, a["maximum_history_size"], scan_points, a["line_res"], a["plane_res"], device=device)
            self.histories = [_History_slot(self.history_batch, s) for s in range(S)]
            if cell_maps:  # laser_mapping.hpp:620-624
                # the stores grow: they start at the points per map the caller names, a quarter of a million otherwise
                first = max(int(kw.get("cell_map_max_points", 1 << 18)), int(scan_points))
                self.history_batch.enable_cell_maps(first, a["cell_resolution"], a["threshold_cell_revisit"])
            if full_maps:  # laser_mapping.hpp:616-617, 626
                lc = dict(a["loop_closure"] or {})
                first = max(int(lc.pop("max_points", 1 << 18)), int(scan_points))
                self.history_batch.enable_full_maps(first, a["cell_resolution"], a["threshold_cell_revisit"])
                if key_frames:
                    from .keyframes import Keyframe_assembly, Keyframe_rounds
                    # the services named in loop_closure are the driver's, ONE of each for the S assemblies, closed with it
                    on = {k: bool(lc.get(k)) for k in ("device_bank", "pose_graph", "map_refinement")}
                    lc.update({k: True for k in on if on[k]})
                    logs = [{}] * S
                    if on["map_refinement"]:  # the full clouds wait in the scan log on the batch
                        lc.setdefault("maximum_history_size", a["maximum_history_size"])  # (as Laser_mapping hands it on)
                        self.history_batch.enable_scan_log(lc["maximum_history_size"])
                        logs = [dict(scan_log=self.history_batch.scan_log(s)) for s in range(S)]
                    self.keyframes = [Keyframe_assembly(device=device, cell_resolution=a["cell_resolution"],
                                                        threshold_cell_revisit=a["threshold_cell_revisit"],
                                                        full_cell_map=self.history_batch.full_map(s), **lc, **logs[s]) for s in range(S)]
                    self.rounds = Keyframe_rounds(self.keyframes, store=self.history_batch, bank=on["device_bank"],
                                                  pose_graph=on["pose_graph"], map_refinement=on["map_refinement"])
                    self.keyframe_bank = self.rounds.bank() if on["device_bank"] else None
                    self.pose_graph = self.rounds.pose_graph() if on["pose_graph"] else None
                    self.map_refine = self.rounds.map_refine() if on["map_refinement"] else None
                    self.loops = [[] for _ in range(S)]
        else:
            self.history_batch = None
            self.histories = [History_buffer(a["maximum_history_size"], scan_points, a["line_res"], a["plane_res"], device=device) for _ in range(S)]
        self.line_res, self.plane_res = a["line_res"], a["plane_res"]
        self.m_if_input_downsample_mode = a["input_downsample_mode"]
        self.history_add_t_step, self.history_add_angle_step = a["history_add_t_step"], a["history_add_angle_step"]
        _set_registrar_params(self.reg.params, **a)
        if self.if_motion_deblur:
            self.reg.params.if_motion_deblur = 1
        self.m_last_time_stamp = np.zeros(S, np.float64)  # m_last_time_stamp of every sequence (laser_mapping.hpp:1345-1347)
        self._ranges = None                               # this step's (minimum, maximum) time stamps per slot, with if_motion_deblur
        self.frame_index = np.zeros(S, np.int32)                                  # m_current_frame_index of every sequence
        self.poses = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (S, 1))  # m_q_w_curr / m_t_w_curr
        self.map_sizes = [(0, 0)] * S
        self.last_reports = [None] * S
        self.aborted_solves = 0
        # cumulative host time: extract + register (wall), history add and refresh (summed over the pool's threads), steps, and the
        # wall time of the add + refresh phase
        self.stage_s = np.zeros(5)
        self._pool = None
        if self.refresh_threads > 1 and not self.batched_history:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.refresh_threads)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        for kf in self.keyframes or []:
            kf.close()
        if self.rounds is not None:
            self.rounds.close()
        for h in [self.fe, self.reg, self.vox[0], self.vox[1]] + self.maps + ([self.history_batch] if self.batched_history else self.histories):
            h.close()

    def degenerate_directions(self, sequence: int, min_eigenvalue: float) -> np.ndarray:
        """Laser_mapping.degenerate_directions for one sequence's last frame"""
        if self.last_information[sequence] is None:
            raise RuntimeError("degenerate_directions needs information=True and a registered frame of that sequence")
        return _degenerate_directions(self.last_information[sequence], min_eigenvalue)

    def sync(self) -> None:
        """every accepted frame is in the cell maps and their stores are in order (cell_maps=True; otherwise nothing to wait for)"""
        if self.cell_maps:
            self.history_batch.sync_cell_maps()

    def cell_map(self, sequence: int, kind: int):
        if not self.cell_maps:
            raise ValueError("no cell maps: create the loop with batched_history=True, cell_maps=True")
        return self.history_batch.cell_map(sequence, kind)

    def full_map(self, sequence: int):
        if not self.full_maps:
            raise ValueError("no full maps: create the loop with batched_history=True, full_maps=True")
        return self.history_batch.full_map(sequence)

    def _full_step(self, jobs, on, new, added=None) -> None:
        """laser_mapping.hpp:1442 + 1524-1562 for the accepted slots: their scans' full clouds into the full-cloud maps in one append,
        then per slot the key-frame bookkeeping on the cells that scan touched.  With loop_closure map_refinement the scans the
        history's add let in (`added`) join the scan log in between, in one call (:1456 comes before :1524)."""
        import time
        t0 = time.perf_counter()
        self.history_batch.append_full(self.fe, new, on, 3, lists=False)  # (a key frame reads its slot's list through its view)
        logging = self.map_refine is not None
        if logging:
            self.history_batch.log_full(self.fe, np.asarray(on, bool) & np.asarray(added, bool))
        if self.key_frames:
            none = np.zeros((0, 4), np.float32)  # (the slot view answers with the append's list; the cloud itself stays on the device)
            for s, _, pose_new in jobs:
                if logging:
                    self.keyframes[s].add_scan(none, pose_new, int(self.frame_index[s]), history_added=bool(added[s]))
                else:
                    self.keyframes[s].add_scan(none, pose_new, int(self.frame_index[s]))
            slots = [s for s, _, _ in jobs]
            for s, found in zip(slots, self.rounds.run(slots)):
                self.loops[s] += found
        self.full_map_s += time.perf_counter() - t0

    def _upload(self, scans, stamps, active):
        S = self.n_sequences
        arrs = [None if scans[s] is None else np.ascontiguousarray(scans[s], np.float32) for s in range(S)]
        if all(active) and len({x.shape for x in arrs}) == 1:
            self.fe.upload(np.stack(arrs), stamps)
            return
        empty = np.zeros((1, 0, 4), np.float32)
        for s in range(S):  # an idle slot holds an empty scan: nothing is extracted for it
            self.fe.upload(arrs[s][None] if active[s] else empty, stamps[s:s + 1], first_scan=s)

    def _time_ranges(self, stamps, active) -> None:
        """find_min_max_intensity( full ) per sequence (laser_mapping.hpp:1336-1347): slot s runs from its previous frame's last stamp to
        this frame's, whatever becomes of the registration; an idle slot keeps its stamp.  One selection_last for all slots."""
        last = self.fe.selection_last(self.n_sequences, 2)  # (ascending: the last position carries the largest stamp)
        lo, hi = self.m_last_time_stamp.copy(), self.m_last_time_stamp.copy()
        for s in range(self.n_sequences):
            if active[s]:
                hi[s] = float(_point_time_stamp(stamps[s], int(last[s]), self.fe.params.time_internal_pts)) if last[s] >= 0 else 0.0
                self.m_last_time_stamp[s] = hi[s]
        self._ranges = (lo, hi)

    def _enqueue(self, maps, fi):
        S = self.n_sequences
        if self.if_motion_deblur:  # one-shot: in front of every enqueue, the repeat of an aborted solve included
            self.reg.set_time_ranges(*self._ranges)
        if self.m_if_input_downsample_mode:  # laser_mapping.hpp:1367-1373
            self.reg.enqueue_fe_downsampled_maps(maps, self.fe, self.vox[0], self.vox[1], self.line_res, self.plane_res, S, self.poses, self.poses, fi)
        else:
            self.reg.enqueue_fe_maps(maps, self.fe, S, self.poses, self.poses, fi)

    def _add_and_refresh(self, s, pose_before, pose_new):
        """(with if_undistort the caller has handed sequence s's deskew record to histories[s] already, on its own thread: the copies
        go through the one registrar, which the pool's threads must not share)"""
        import time
        t0 = time.perf_counter()
        h = self.histories[s]
        h.set_gate_pose(pose_before)  # m_q_w_curr is still the pre-registration pose at LM:1439-1451
        if self.m_if_input_downsample_mode:
            h.add_voxel(self.vox[0], self.vox[1], s, pose_new, self.history_add_t_step, self.history_add_angle_step)
        else:
            h.add_fe(self.fe, s, pose_new, self.history_add_t_step, self.history_add_angle_step)
        t1 = time.perf_counter()
        sizes = h.refresh(self.maps[s])
        return s, sizes, t1 - t0, time.perf_counter() - t1

    def _add_and_refresh_batched(self, jobs, undistort=False):
        """the accepted slots of a step through one add and one refresh; rejected and idle slots are inactive"""
        import time
        S = self.n_sequences
        t0 = time.perf_counter()
        on = np.zeros(S, bool)
        gate, new = self.poses.copy(), self.poses.copy()
        for s, pose_before, pose_new in jobs:
            on[s] = True
            gate[s], new[s] = pose_before, pose_new  # m_q_w_curr is still the pre-registration pose at LM:1439-1451
        hb = self.history_batch
        if undistort:
            hb.set_undistort(self.reg)  # :1424,1430 for every slot
        if self.m_if_input_downsample_mode:
            added = hb.add_voxel(self.vox[0], self.vox[1], new, gate, on, self.history_add_t_step, self.history_add_angle_step)
        else:
            added = hb.add_fe(self.fe, new, gate, on, self.history_add_t_step, self.history_add_angle_step)
        t1 = time.perf_counter()
        t_full = self.full_map_s
        if self.full_maps:
            self._full_step(jobs, on, new, added)
        t_full = self.full_map_s - t_full  # (its own figure: neither the add's nor the refresh's)
        maps = [self.maps[s] if on[s] else None for s in range(S)]
        if self.cell_matching:  # update_buff_for_matching with m_matching_mode == 1, at the poses the step just accepted
            nc, ns = hb.refresh_cells(maps, new, on, self.m_maximum_search_range[0], self.m_maximum_search_range[1], self.m_maximum_in_fov_angle,
                                      self.m_down_sample_replace)
        else:
            nc, ns = hb.refresh(maps, on)
        t2 = time.perf_counter()
        k = max(len(jobs), 1)
        return [(s, (int(nc[s]), int(ns[s])), (t1 - t0) / k, (t2 - t1 - t_full) / k) for s, _, _ in jobs]

    def process_new_scans(self, scans, time_stamps=None) -> np.ndarray:
        """One step of every sequence: scans[s] is sequence s's next scan, or None when it has none this step.  Returns an int array:
        -1 idle, 0 rejected, 1 accepted (laser_mapping.hpp:1311-1520 per sequence)."""
        import time
        S = self.n_sequences
        if len(scans) != S:
            raise ValueError(f"{len(scans)} scans for {S} sequences")
        t0 = time.perf_counter()
        active = [x is not None for x in scans]
        out = np.full(S, -1, np.int32)
        if not any(active):
            return out
        stamps = np.ones(S, np.float64) if time_stamps is None else np.ascontiguousarray(time_stamps, np.float64).reshape(S)
        fe, reg = self.fe, self.reg
        self._upload(scans, stamps, active)
        fe.extract_batch(S)
        fe.resolve()
        fe.select_batch(S, -1, 0.0, 1.0)
        if self.if_motion_deblur:
            self._time_ranges(stamps, active)
        fi = self.frame_index.copy()  # init_pointcloud_registration runs before the increment
        self.frame_index[active] += 1
        maps = [self.maps[s] if active[s] else None for s in range(S)]
        self._enqueue(maps, fi)
        res, pc, _, reps = reg.collect(S)
        infos = reg.information(S) if self._information else None
        flags = getattr(reg, "debug_flags", 0)
        again = [s for s in range(S) if active[s] and reps[s].aborted]
        self.aborted_solves += len(again)
        repeated = bool(again and not (flags & 32))
        if repeated:
            # Laser_mapping's repeat of a registration the grouped solver abandoned: those slots once more on one workgroup each,
            # the others idle.  With if_motion_deblur the repeat overwrites the deskew records of the slots it leaves idle, so all
            # active slots repeat: every slot runs solve_big on one workgroup either way, the same bits.  (No solve is abandoned there
            # today -- the grouped solver is not used -- but the repeat, its ranges included, is part of the loop's contract.)
            if self.if_motion_deblur:
                again = [s for s in range(S) if active[s]]
            reg.set_debug_flags(flags | 32)
            self._enqueue([self.maps[s] if s in again else None for s in range(S)], fi)
            res2, pc2, _, reps2 = reg.collect(S)
            infos2 = reg.information(S) if self._information else None
            reg.set_debug_flags(flags)
            for s in again:
                res[s], pc[s], reps[s] = res2[s], pc2[s], reps2[s]
                if infos is not None:
                    infos[s] = infos2[s]  # the repeat's record replaces the aborted one
        t1 = time.perf_counter()
        jobs = []
        for s in range(S):
            if not active[s]:
                continue
            self.last_reports[s] = reps[s]
            if infos is not None:
                self.last_information[s] = _with_pose_frame(infos[s], self.poses[s])
            out[s] = 1 if res[s] else 0
            if res[s]:  # :1413-1416
                jobs.append((s, self.poses[s].copy(), pc[s].copy()))
        # if_undistort: the adds move their clouds with the registration's records (:1424,1430).  Without motion deblur a record is the
        # plain transform with the pose the add receives, bit for bit, so the one step in which a repeat has overwritten the other
        # slots' records goes without them.
        undistort = bool(self.if_undistort and jobs and (self.if_motion_deblur or not repeated))
        if undistort and not self.batched_history:
            for s, _, _ in jobs:  # on this thread, before the pool starts: the copies go through the one registrar
                self.histories[s].set_undistort(reg, s)
        if self.batched_history:
            done = self._add_and_refresh_batched(jobs, undistort) if jobs else []
        elif self._pool is not None and len(jobs) > 1:
            done = list(self._pool.map(lambda j: self._add_and_refresh(*j), jobs))
        else:
            done = [self._add_and_refresh(*j) for j in jobs]
        for (s, sizes, t_add, t_ref), j in zip(done, jobs):
            self.map_sizes[s] = sizes
            self.poses[s] = j[2]  # :1496-1500
            self.stage_s[1] += t_add
            self.stage_s[2] += t_ref
        t2 = time.perf_counter()
        self.stage_s[0] += t1 - t0
        self.stage_s[3] += 1
        self.stage_s[4] += t2 - t1
        return out
