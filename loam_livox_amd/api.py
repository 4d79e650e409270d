"""Host-side mirror of the reference's call surface for the hot path, on top of the C ABI.

Class and method names follow hku-mars/loam_livox so that parity tests read like calls into the reference:

  Livox_laser               source/livox_feature_extractor.hpp:77     (extract_laser_features :722, get_features :219)
  Point_cloud_registration  source/point_cloud_registration.hpp:38    (find_out_incremental_transfrom :163/:585,
                                                                       pointcloudAssociateToMap :673)
  Map_buffer                the (cloud, KdTreeFLANN) pairs of source/laser_mapping.hpp:539-546
  Spinning_laser            the lidar_type != "livox" branch of Laser_feature::laserCloudHandler,
                            source/laser_feature_extractor.hpp:393-787

Poses are numpy float64[7] = (qx,qy,qz,qw,tx,ty,tz).  PyTorch is not needed here: device memory and streams are
owned by the library.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from .capi import FeParams, RegParams, RegReport, check, ptr


class _Handle:
    """A class that owns one device handle: L is the library, h the handle (a c_void_p, None once closed), _destroy the name of the
    entry point that frees it.  close() may be called any number of times and destroys the handle once; an object whose constructor
    raised before or inside its ll_*_create holds no handle (no h at all, or a null one) and never destroys; __del__ closes and swallows
    whatever that raises."""

    _destroy = None

    def __init__(self):
        self.L = capi.load()
        self.h = C.c_void_p()

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, self._destroy)(self.h)
        self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _call(self, name: str, *args) -> int:
        """check( ll_<name>( h, args... ) ), for the bodies that several entry points share"""
        return check(getattr(self.L, name)(self.h, *args), name)

    def _tap(self, name: str, *lead, n: int = 4) -> np.ndarray:
        """a test tap: the entry point fills int64[n] behind its leading arguments"""
        out = np.zeros(n, np.int64)
        self._call(name, *lead, ptr(out))
        return out

    def _read_cloud(self, name: str, key: int) -> np.ndarray:
        """size, then fill, with the count through the last argument: the points [n, 4] an entry point keeps under `key`"""
        n = C.c_int64(0)
        self._call(name, int(key), None, 0, C.byref(n))
        out = np.zeros((int(n.value), 4), np.float32)
        self._call(name, int(key), ptr(out), len(out), C.byref(n))
        return out

    def _read_counted_cloud(self, name: str, *lead) -> np.ndarray:
        """size, then fill, with the count returned (negative: the library's error): the match cloud [n, 4] of a history"""
        n = self._call(name, *lead, None, 0)
        out = np.zeros((n, 4), np.float32)
        if n > 0:
            check(min(0, getattr(self.L, name)(self.h, *lead, ptr(out), n)), name)
        return out


def _active_mask(active, S: int):
    """the slots a batched call serves as int32[S], None for all of them"""
    return None if active is None else np.ascontiguousarray(np.asarray(active).astype(bool), np.int32).reshape(S)


def _handle_table(objs):
    """the handles of a list of objects as a C array of pointers; None stays a null entry (an idle slot)"""
    return (C.c_void_p * max(len(objs), 1))(*[None if o is None else o.h for o in objs])


def _poses(x, n: int) -> np.ndarray:
    """n poses as a contiguous float64[n, 7] block (n = -1: as many as x holds)"""
    return np.ascontiguousarray(x, np.float64).reshape(n, 7)


def _keyframe_outputs():
    """the five output arrays of Maps_keyframe::analyze: images [4, 60, 60], ratio_nonzero [4], eigen_R [2, 3, 3], n_vectors [4],
    (centre, roi_range) [4]"""
    return np.zeros((4, 60, 60), np.float32), np.zeros(4, np.float32), np.zeros((2, 3, 3), np.float32), np.zeros(4, np.int32), np.zeros(4, np.float32)


def _keyframe_result(img, ratio, R, nv, cr) -> dict:
    return dict(images=img, ratio_nonzero=ratio, eigen_R=R, n_vectors=nv, centre=cr[:3].copy(), roi_range=float(cr[3]))


class Livox_laser(_Handle):
    """Device-backed Livox_laser.  Tunables are the public fields of the reference class
    (livox_feature_extractor.hpp:143-167); they are fixed at construction."""

    _destroy = "ll_fe_destroy"

    def __init__(self, max_points: int = 24000, max_scans: int = 1, device: int = 0, piecewise_number: int = 3, **tunables):
        super().__init__()
        p = capi.fe_default_params()
        p.max_points, p.max_scans, p.device, p.piecewise_number = max_points, max_scans, device, piecewise_number
        for k, v in tunables.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        self.params = p
        check(self.L.ll_fe_create(C.byref(p), C.byref(self.h)), "ll_fe_create")
        self.m_input_points_size = 0
        self._n = [0] * max_scans

    # -- per-message path (laser_feature_extractor.hpp:285) ---------------------------------------------------
    def extract_laser_features(self, xyzi: np.ndarray, time_stamp: float) -> int:
        """Returns laserCloudScans.size() (number of surviving petal clouds)."""
        xyzi = capi.as_f32(xyzi, 4)
        n = xyzi.shape[0]
        npc = C.c_int32(0)
        check(self.L.ll_fe_extract(self.h, ptr(xyzi), n, float(time_stamp), C.byref(npc)), "ll_fe_extract")
        self.m_input_points_size = n
        self._n[0] = n
        return npc.value

    def get_features(self, minimum_blur: float = 0.0, maximum_blur: float = 0.3, scan: int | None = None):
        """Returns dict(corner_idx, surf_idx, full_idx, pc_corners, pc_surface) for scan slot 0; with `scan` given: the selection
        select_batch() left in that slot (the blur window is then the one select_batch was called with)."""
        n = self.params.max_points
        ci, si, fi = (np.zeros(n, np.int32) for _ in range(3))
        cc, sc = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
        nc, ns, nf = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        if scan is None:
            check(self.L.ll_fe_select(self.h, minimum_blur, maximum_blur, ptr(ci), C.byref(nc), ptr(si), C.byref(ns), ptr(fi),
                                      C.byref(nf), ptr(cc), ptr(sc)), "ll_fe_select")
        else:
            check(self.L.ll_fe_selection(self.h, int(scan), ptr(ci), C.byref(nc), ptr(si), C.byref(ns), ptr(fi), C.byref(nf), ptr(cc), ptr(sc)),
                  "ll_fe_selection")
        return dict(corner_idx=ci[:nc.value].copy(), surf_idx=si[:ns.value].copy(), full_idx=fi[:nf.value].copy(),
                    pc_corners=cc[:nc.value].copy(), pc_surface=sc[:ns.value].copy())

    def full_selection(self, scan: int = 0) -> np.ndarray:
        """the positions of the full cloud select_batch() left in slot `scan` (ascending), and nothing else: one count and one index array
        cross the bus (ll_fe_selection with its other outputs NULL)"""
        fi = np.zeros(self.params.max_points, np.int32)
        nf = C.c_int32(0)
        check(self.L.ll_fe_selection(self.h, int(scan), None, None, None, None, ptr(fi), C.byref(nf), None, None), "ll_fe_selection")
        return fi[:nf.value].copy()

    def selection_last(self, n_scans: int, kind: int = 2) -> np.ndarray:
        """the last (largest) position of every slot's selection of `kind` (0 corner, 1 surface, 2 full) after select_batch(), int32
        [n_scans], -1 where the selection is empty (ll_fe_selection_last: one small launch, n_scans ints across the bus)"""
        last = np.zeros(int(n_scans), np.int32)
        check(self.L.ll_fe_selection_last(self.h, int(n_scans), int(kind), ptr(last)), "ll_fe_selection_last")
        return last

    def pts_info(self, scan: int = 0):
        """m_pts_info_vec as a dict of arrays."""
        n = self._n[scan]
        out = dict(pt_type=np.zeros(n, np.int32), pt_label=np.zeros(n, np.int32), depth_sq2=np.zeros(n, np.float32),
                   polar_dis_sq2=np.zeros(n, np.float32), curvature=np.zeros(n, np.float32),
                   view_angle=np.zeros(n, np.float32), time_stamp=np.zeros(n, np.float32),
                   polar_angle=np.zeros(n, np.float32))
        check(self.L.ll_fe_labels(self.h, scan, ptr(out["pt_type"]), ptr(out["pt_label"]), ptr(out["depth_sq2"]),
                                  ptr(out["polar_dis_sq2"]), ptr(out["curvature"]), ptr(out["view_angle"]),
                                  ptr(out["time_stamp"]), ptr(out["polar_angle"])), "ll_fe_labels")
        return out

    def splits(self, scan: int = 0):
        cap = self.params.max_points // 50 + 8
        split = np.zeros(cap, np.int32)
        first, last = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        ps, pe = np.zeros(8, np.float32), np.zeros(8, np.float32)
        ns, cl, npc = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(self.L.ll_fe_splits(self.h, scan, ptr(split), C.byref(ns), C.byref(cl), C.byref(npc), ptr(first), ptr(last),
                                  ptr(ps), ptr(pe)), "ll_fe_splits")
        P = self.params.piecewise_number
        return dict(split_idx=split[:ns.value].copy(), clutter_size=cl.value, n_petal_clouds=npc.value,
                    first_idx=first[:npc.value].copy(), last_idx=last[:npc.value].copy(), piece_start=ps[:P].copy(),
                    piece_end=pe[:P].copy())

    # -- batched, device-resident path ------------------------------------------------------------------------
    def upload(self, scans: np.ndarray, current_time: np.ndarray, first_scan: int = 0, wait: bool = True):
        """wait=False: ll_fe_upload_async -- the arrays are kept referenced on the object until the next upload / sync and
        should be page-locked (e.g. views of torch pinned tensors) for the copy to overlap other work."""
        assert scans.dtype == np.float32 and scans.flags["C_CONTIGUOUS"] if not wait else True
        scans = np.ascontiguousarray(scans, np.float32)
        assert scans.ndim == 3 and scans.shape[2] == 4
        ct = np.ascontiguousarray(current_time, np.float64)
        fn = self.L.ll_fe_upload if wait else self.L.ll_fe_upload_async
        check(fn(self.h, first_scan, scans.shape[0], ptr(scans), scans.shape[1], ptr(ct)), "ll_fe_upload")
        self._pending_upload = None if wait else (scans, ct)
        for i in range(scans.shape[0]):
            self._n[first_scan + i] = scans.shape[1]

    def extract_batch(self, n_scans: int):
        check(self.L.ll_fe_extract_batch(self.h, n_scans), "ll_fe_extract_batch")

    def resolve(self) -> int:
        return check(self.L.ll_fe_resolve(self.h), "ll_fe_resolve")

    def select_batch(self, n_scans: int, piece: int = -1, minimum_blur: float = 0.0, maximum_blur: float = 1.0):
        check(self.L.ll_fe_select_batch(self.h, n_scans, piece, minimum_blur, maximum_blur), "ll_fe_select_batch")

    def counts(self, n_scans: int):
        nc, ns, nf = (np.zeros(n_scans, np.int32) for _ in range(3))
        na = np.zeros(1, np.int32)
        check(self.L.ll_fe_counts(self.h, n_scans, ptr(nc), ptr(ns), ptr(nf), ptr(na)), "ll_fe_counts")
        return nc, ns, nf, int(na[0])

    def sync(self):
        check(self.L.ll_fe_sync(self.h), "ll_fe_sync")


class Spinning_laser(_Handle):
    """The spinning-lidar branch of Laser_feature::laserCloudHandler (lidar_type != "livox",
    source/laser_feature_extractor.hpp:393-787) on the device: one message in, the five published clouds out
    (include/loam_livox_hip.h, ll_spin_*).  `extract` is the one-message call, `extract_batch` the batched one."""

    _destroy = "ll_spin_destroy"

    TOPICS = ("/laser_points_2", "/laser_cloud_sharp", "/laser_cloud_less_sharp", "/laser_cloud_flat", "/laser_cloud_less_flat")
    FULL, SHARP, LESS_SHARP, FLAT, LESS_FLAT, LESS_FLAT_PRE = range(6)

    def __init__(self, scan_line: int = 16, minimum_range: float = 0.1, plane_resolution: float = 0.8, max_points: int = 32768,
                 max_scans: int = 1, max_line_points: int = 8192, device: int = 0):
        super().__init__()
        p = capi.spin_default_params()
        p.scan_line, p.minimum_range, p.plane_resolution = scan_line, minimum_range, plane_resolution
        p.max_points, p.max_scans, p.max_line_points, p.device = max_points, max_scans, max_line_points, device
        self.params = p
        check(self.L.ll_spin_create(C.byref(p), C.byref(self.h)), "ll_spin_create")
        self.n_ambiguous = 0

    def upload(self, scans, first_scan: int = 0):
        """scans: a list of (n_b, 4) clouds"""
        n = np.array([len(c) for c in scans], np.int32)
        stride = max(1, int(n.max()) if len(n) else 1)
        buf = np.zeros((len(scans), stride, 4), np.float32)
        for b, c in enumerate(scans):
            buf[b, :len(c)] = capi.as_f32(c, 4)
        check(self.L.ll_spin_upload(self.h, first_scan, len(scans), ptr(buf), ptr(n), stride), "ll_spin_upload")

    def extract_batch(self, scans) -> list:
        """Uploads, extracts, resolves; returns one dict of clouds per scan (see `clouds`)."""
        self.upload(scans)
        B = len(scans)
        check(self.L.ll_spin_extract_batch(self.h, B), "ll_spin_extract_batch")
        self.n_ambiguous = check(self.L.ll_spin_resolve(self.h), "ll_spin_resolve")
        return [self.clouds(b) for b in range(B)]

    def extract_batch_async(self, n_scans: int):
        """ll_spin_extract_batch on the slots already uploaded: asynchronous, nothing is downloaded (the device hand-offs
        Point_cloud_registration.enqueue_spin / History_buffer.add_spin take the clouds where they are)"""
        check(self.L.ll_spin_extract_batch(self.h, int(n_scans)), "ll_spin_extract_batch")

    def resolve(self) -> int:
        self.n_ambiguous = check(self.L.ll_spin_resolve(self.h), "ll_spin_resolve")
        return self.n_ambiguous

    def sync(self):
        check(self.L.ll_spin_sync(self.h), "ll_spin_sync")

    def extract(self, xyzi) -> dict:
        """One message (laserCloudHandler :393-787 without the publishes)."""
        pts = capi.as_f32(xyzi, 4)
        if len(pts) == 0:
            pts = np.zeros((0, 4), np.float32)
        buf = pts if len(pts) else np.zeros((1, 4), np.float32)
        st = check(self.L.ll_spin_extract(self.h, ptr(buf), len(pts)), "ll_spin_extract")
        if st != 0:
            raise capi.LoamLivoxError(f"ll_spin_extract: status {st} (a line holds more less-flat points than max_line_points)")
        return self.clouds(0)

    def counts(self, n_scans: int):
        c = np.zeros((n_scans, 5), np.int32)
        st = np.zeros(n_scans, np.int32)
        check(self.L.ll_spin_counts(self.h, n_scans, ptr(c), ptr(st)), "ll_spin_counts")
        return c, st

    def cloud(self, scan: int, which: int, with_idx: bool = True):
        cap = self.params.max_points
        xyzi = np.zeros((cap, 4), np.float32)
        idx = np.zeros(cap, np.int32) if with_idx and which != self.LESS_FLAT else None
        n = C.c_int32(0)
        check(self.L.ll_spin_cloud(self.h, scan, which, ptr(xyzi), ptr(idx), C.byref(n)), "ll_spin_cloud")
        return xyzi[:n.value].copy(), (idx[:n.value].copy() if idx is not None else None)

    def lines(self, scan: int = 0):
        L = self.params.scan_line
        st, n = np.zeros(L, np.int32), np.zeros(L, np.int32)
        check(self.L.ll_spin_lines(self.h, scan, ptr(st), ptr(n)), "ll_spin_lines")
        return st, n

    def clouds(self, scan: int = 0) -> dict:
        """The five published clouds keyed by topic, plus index arrays: full_src (input index of each laserCloud point),
        sharp / less_sharp / flat / less_flat_pre (positions in laserCloud), line_start / line_n (laserCloudScans)."""
        out = {}
        full, src = self.cloud(scan, self.FULL)
        out[self.TOPICS[0]], out["full_src"] = full, src
        for which, key in ((self.SHARP, "sharp"), (self.LESS_SHARP, "less_sharp"), (self.FLAT, "flat"), (self.LESS_FLAT_PRE, "less_flat_pre")):
            xyzi, idx = self.cloud(scan, which)
            out[key] = idx
            if which != self.LESS_FLAT_PRE:
                out[self.TOPICS[which]] = xyzi
        out[self.TOPICS[4]] = self.cloud(scan, self.LESS_FLAT, with_idx=False)[0]
        out["line_start"], out["line_n"] = self.lines(scan)
        return out

    def handoff_time(self) -> float:
        """milliseconds of the pack kernel of the last device hand-off (ll_spin_handoff_time)"""
        ms = C.c_float(0.0)
        check(self.L.ll_spin_handoff_time(self.h, C.byref(ms)), "ll_spin_handoff_time")
        return float(ms.value)

    def kernel_times(self):
        """milliseconds of the phases of the last batch: assign, lines, curvature, sort, select, VoxelGrid + gather"""
        ms = np.zeros(6, np.float32)
        check(self.L.ll_spin_kernel_times(self.h, ptr(ms)), "ll_spin_kernel_times")
        return ms


class VoxelGrid(_Handle):
    """pcl::VoxelGrid<pcl::PointXYZI> as the reference uses it (setLeafSize / setInputCloud / filter:
    laser_feature_extractor.hpp:192-193,372-381; laser_mapping.hpp:742-743,1367-1373,1434-1437,533-537),
    PCL 1.9 semantics with a deterministic in-leaf order (include/loam_livox_hip.h)."""

    _destroy = "ll_voxel_destroy"

    def __init__(self, max_points: int = 100000, max_clouds: int = 1, device: int = 0):
        super().__init__()
        self.max_points, self.max_clouds = max_points, max_clouds
        check(self.L.ll_voxel_create(device, max_clouds, max_points, C.byref(self.h)), "ll_voxel_create")
        self.leaf = np.array([0.4, 0.4, 0.4], np.float32)
        self._cloud = None
        self.status = 0

    def setLeafSize(self, lx: float, ly: float, lz: float):
        self.leaf = np.array([lx, ly, lz], np.float32)

    def setInputCloud(self, cloud: np.ndarray):
        self._cloud = capi.as_f32(cloud, 4)

    def filter(self) -> np.ndarray:
        """Returns the filtered cloud (n_out x 4); self.status: 0 filtered, 1 leaf too small (copy of the input), 2 empty."""
        out, n_out, st = self.filter_batch(self._cloud[None], np.array([self._cloud.shape[0]], np.int32))
        self.status = int(st[0])
        return out[0, :n_out[0]].copy()

    def filter_batch(self, clouds: np.ndarray, n_points: np.ndarray):
        """clouds [B][stride][4], n_points [B] -> (out [B][stride][4], n_out [B], status [B])."""
        clouds = np.ascontiguousarray(clouds, np.float32)
        B, stride = clouds.shape[0], clouds.shape[1]
        n_points = np.ascontiguousarray(n_points, np.int32)
        if stride == 0:
            return np.zeros_like(clouds), np.zeros(B, np.int32), np.full(B, 2, np.int32)
        out = np.zeros_like(clouds)
        n_out = np.zeros(B, np.int32)
        st = np.zeros(B, np.int32)
        check(self.L.ll_voxel_filter(self.h, B, ptr(clouds), ptr(n_points), stride, ptr(self.leaf), ptr(out), ptr(n_out), ptr(st)),
              "ll_voxel_filter")
        return out, n_out, st

    def counts(self, n_clouds: int):
        n_out, st = np.zeros(n_clouds, np.int32), np.zeros(n_clouds, np.int32)
        check(self.L.ll_voxel_counts(self.h, n_clouds, ptr(n_out), ptr(st)), "ll_voxel_counts")
        return n_out, st


class History_buffer(_Handle):
    """m_laser_cloud_{corner,surface}_history + update_buff_for_matching (history mode), laser_mapping.hpp:1417-1478,
    517-546, resident on the device (include/loam_livox_hip.h, ll_history_*)."""

    _destroy = "ll_history_destroy"

    def __init__(self, maximum_history_size: int = 100, max_points_per_frame: int = 24000, line_res: float = 0.1,
                 plane_res: float = 0.4, device: int = 0):
        super().__init__()
        self.device = device
        check(self.L.ll_history_create(device, maximum_history_size, max_points_per_frame, line_res, plane_res, C.byref(self.h)),
              "ll_history_create")

    def __len__(self):
        return int(self.L.ll_history_size(self.h))

    def _add(self, name: str, source, pose, t_step: float, angle_step: float) -> bool:
        """the four adds: the entry point's own arguments (`source`), then the pose, the two steps of the add rule and the added flag"""
        pose = np.ascontiguousarray(pose, np.float64)
        added = C.c_int32(0)
        self._call(name, *source, ptr(pose), t_step, angle_step, C.byref(added))
        return bool(added.value)

    def add(self, corner, surf, pose, history_add_t_step: float = 0.0, history_add_angle_step: float = 0.0) -> bool:
        corner, surf = capi.as_f32(corner, 4), capi.as_f32(surf, 4)
        return self._add("ll_history_add", (ptr(corner), corner.shape[0], ptr(surf), surf.shape[0]), pose, history_add_t_step, history_add_angle_step)

    def add_fe(self, fe: "Livox_laser", scan: int, pose, history_add_t_step: float = 0.0, history_add_angle_step: float = 0.0) -> bool:
        return self._add("ll_history_add_fe", (fe.h, scan), pose, history_add_t_step, history_add_angle_step)

    def add_spin(self, spin: "Spinning_laser", scan: int, pose, history_add_t_step: float = 0.0, history_add_angle_step: float = 0.0) -> bool:
        """add_fe for a spinning-lidar handle: the less-sharp and the less-flat cloud of slot `scan`, device to device"""
        return self._add("ll_history_add_spin", (spin.h, scan), pose, history_add_t_step, history_add_angle_step)

    def add_voxel(self, vox_corner: "VoxelGrid", vox_surf: "VoxelGrid", cloud: int, pose, history_add_t_step: float = 0.0,
                  history_add_angle_step: float = 0.0) -> bool:
        return self._add("ll_history_add_voxel", (vox_corner.h, vox_surf.h, cloud), pose, history_add_t_step, history_add_angle_step)

    def refresh(self, map_buffer: "Map_buffer"):
        nc, ns = C.c_int64(0), C.c_int64(0)
        check(self.L.ll_history_refresh(self.h, map_buffer.h, C.byref(nc), C.byref(ns)), "ll_history_refresh")
        return nc.value, ns.value

    def enable_cell_map(self, max_points: int = 1 << 20, cell_resolution: float = 1.0, threshold_cell_revisit: int = 5000) -> None:
        """m_pt_cell_map_corners / m_pt_cell_map_planes (laser_mapping.hpp:274-275, 617-624): fed by every add*()."""
        check(self.L.ll_history_enable_cell_map(self.h, max_points, cell_resolution, threshold_cell_revisit), "ll_history_enable_cell_map")
        self._cell_resolution = cell_resolution

    def set_cell_map_async(self, enable: bool = True) -> None:
        """feed the cell maps through the handle's service thread, beside the caller (matching mode 0: nothing reads them per frame)"""
        check(self.L.ll_history_set_cell_map_async(self.h, int(bool(enable))), "ll_history_set_cell_map_async")

    def sync_cell_maps(self) -> None:
        check(self.L.ll_history_sync_cell_maps(self.h), "ll_history_sync_cell_maps")

    def cell_map(self, kind: int) -> "Cell_map":
        h = self.L.ll_history_cell_map(self.h, kind)
        if not h:  # not enabled, or the service thread failed: the library says which
            msg = self.L.ll_last_error()
            raise capi.LoamLivoxError(f"ll_history_cell_map: {msg.decode() if msg else 'error'}")
        return Cell_map(resolution=self._cell_resolution, _borrowed=h)

    def refresh_cells(self, map_buffer: "Map_buffer", pose, maximum_search_range_corner: float = 100.0,
                      maximum_search_range_surface: float = 100.0, maximum_in_fov_angle: float = 30.0, down_sample_replace: int = 1):
        """update_buff_for_matching with m_matching_mode == 1 (laser_mapping.hpp:471-546)."""
        pose = np.ascontiguousarray(pose, np.float64)
        nc, ns = C.c_int64(0), C.c_int64(0)
        check(self.L.ll_history_refresh_cells(self.h, map_buffer.h, ptr(pose), maximum_search_range_corner, maximum_search_range_surface,
                                              maximum_in_fov_angle, int(down_sample_replace), C.byref(nc), C.byref(ns)),
              "ll_history_refresh_cells")
        return nc.value, ns.value

    def set_gate_pose(self, pose) -> None:
        """the node's pose before the registration whose result the next add() receives (laser_mapping.hpp:1439-1451)"""
        p = np.ascontiguousarray(pose, np.float64)
        check(self.L.ll_history_set_gate_pose(self.h, ptr(p)), "ll_history_set_gate_pose")

    def set_undistort(self, reg: "Point_cloud_registration", slot: int = 0) -> None:
        """g_if_undistore = 1 for the next add() / add_fe() / add_voxel() only (laser_mapping.hpp:1424,1430): that add moves its clouds with the
        pose interpolated at every point's time stamp, from the state slot `slot` of reg's last collected registration left"""
        check(self.L.ll_history_set_undistort(self.h, reg.h, int(slot)), "ll_history_set_undistort")

    def map_cloud(self, kind: int) -> np.ndarray:
        return self._read_counted_cloud("ll_history_map_cloud", kind)

    def map_cloud_device(self, kind: int):
        """The same cloud as a torch tensor (n, 4) float32 ON THE DEVICE, copied device-to-device out of the handle's
        buffer (which the next refresh overwrites): the input of the multi-GPU sub-map gather, no host hop."""
        import torch
        p, n = C.c_void_p(), C.c_int64(0)
        check(self.L.ll_history_map_cloud_device(self.h, kind, C.byref(p), C.byref(n)), "ll_history_map_cloud_device")
        if n.value == 0:
            return torch.zeros((0, 4), dtype=torch.float32, device=f"cuda:{self.device}")
        return torch.as_tensor(_DeviceView(p.value, n.value), device=f"cuda:{self.device}").clone()


class History_buffer_batch(_Handle):
    """The match buffers of n_sequences sequences in one handle (include/loam_livox_hip.h, ll_history_batch_*): slot s is a
    History_buffer in every result -- add rule with the gate pose, FIFO, concatenation, VoxelGrid, the snapshots published into
    maps[s] -- while one add_voxel / add_fe and one refresh serve all slots with a fixed number of launches and host waits."""

    _destroy = "ll_history_batch_destroy"

    def __init__(self, n_sequences: int, maximum_history_size: int = 100, max_points_per_frame: int = 24000, line_res: float = 0.1,
                 plane_res: float = 0.4, device: int = 0):
        super().__init__()
        self.device, self.n_sequences = device, int(n_sequences)
        check(self.L.ll_history_batch_create(device, n_sequences, maximum_history_size, max_points_per_frame, line_res, plane_res,
                                             C.byref(self.h)), "ll_history_batch_create")

    def _slots(self, active, poses, gate_poses):
        S = self.n_sequences
        act = _active_mask(active, S)
        return act, _poses(poses, S), None if gate_poses is None else _poses(gate_poses, S), np.zeros(S, np.int32)

    def _maps(self, maps, active):
        """(handle table of maps, active mask, two int64[S] for the sizes) of a refresh: a map per slot, None for an inactive one"""
        S = self.n_sequences
        if len(maps) != S:
            raise ValueError(f"{len(maps)} maps for {S} sequences")
        return _handle_table(maps), _active_mask(active, S), np.zeros(S, np.int64), np.zeros(S, np.int64)

    def add_voxel(self, vox_corner: "VoxelGrid", vox_surf: "VoxelGrid", poses, gate_poses=None, active=None, history_add_t_step: float = 0.0,
                  history_add_angle_step: float = 0.0) -> np.ndarray:
        """slot s takes cloud s of the two filters; returns the added flags [S] (bool)"""
        act, poses, gate, added = self._slots(active, poses, gate_poses)
        check(self.L.ll_history_batch_add_voxel(self.h, vox_corner.h, vox_surf.h, ptr(act), ptr(poses), ptr(gate), history_add_t_step,
                                                history_add_angle_step, ptr(added)), "ll_history_batch_add_voxel")
        return added.astype(bool)

    def add_fe(self, fe: "Livox_laser", poses, gate_poses=None, active=None, history_add_t_step: float = 0.0,
               history_add_angle_step: float = 0.0) -> np.ndarray:
        """slot s takes the features selected for scan s of the extractor; returns the added flags [S] (bool)"""
        act, poses, gate, added = self._slots(active, poses, gate_poses)
        check(self.L.ll_history_batch_add_fe(self.h, fe.h, ptr(act), ptr(poses), ptr(gate), history_add_t_step, history_add_angle_step,
                                             ptr(added)), "ll_history_batch_add_fe")
        return added.astype(bool)

    def set_undistort(self, reg: "Point_cloud_registration") -> None:
        """g_if_undistore = 1 for the next add_voxel() / add_fe() only (History_buffer.set_undistort for all slots): active slot s moves its
        clouds with the state slot s of reg's last collected registration left; poses / gate_poses still serve the add rule"""
        check(self.L.ll_history_batch_set_undistort(self.h, reg.h), "ll_history_batch_set_undistort")

    def refresh(self, maps, active=None):
        """maps: n_sequences Map_buffer (None allowed for an inactive slot).  Returns (n_corner [S], n_surf [S]) of the match buffers."""
        arr, act, nc, ns = self._maps(maps, active)
        check(self.L.ll_history_batch_refresh(self.h, arr, ptr(act), ptr(nc), ptr(ns)), "ll_history_batch_refresh")
        return nc, ns

    def refresh_cells(self, maps, poses, active=None, maximum_search_range_corner: float = 100.0, maximum_search_range_surface: float = 100.0,
                      maximum_in_fov_angle: float = 30.0, down_sample_replace: int = 1):
        """update_buff_for_matching in the cell mode (m_matching_mode == 1) for every active slot, at poses [S][7]: the cells in range
        and in the field of view, each through the VoxelGrid (and replaced by its leaves with down_sample_replace), concatenated,
        filtered, published into maps[s].  Needs enable_cell_maps.  Returns (n_corner [S], n_surf [S])."""
        arr, act, nc, ns = self._maps(maps, active)
        poses = None if poses is None else _poses(poses, self.n_sequences)
        check(self.L.ll_history_batch_refresh_cells(self.h, arr, ptr(act), ptr(poses), maximum_search_range_corner, maximum_search_range_surface,
                                                    maximum_in_fov_angle, int(down_sample_replace), ptr(nc), ptr(ns)), "ll_history_batch_refresh_cells")
        return nc, ns

    def cell_match_work(self) -> np.ndarray:
        """test tap (ll_history_batch_cell_match_work): enqueues and host waits of the last refresh_cells, compactions so far, log and live
        entries of the corner and of the surface stores, candidates of the last refresh"""
        return self._tap("ll_history_batch_cell_match_work", n=8)

    def size(self, sequence: int) -> int:
        return int(self.L.ll_history_batch_size(self.h, sequence))

    def map_cloud(self, sequence: int, kind: int) -> np.ndarray:
        return self._read_counted_cloud("ll_history_batch_map_cloud", sequence, kind)

    def enable_cell_maps(self, initial_points_per_map: int = 1 << 20, cell_resolution: float = 1.0, threshold_cell_revisit: int = 5000) -> None:
        """the two cell maps of every slot (laser_mapping.hpp:274-275, 617-624): fed by every active slot of add_voxel / add_fe, put in
        order when read; the stores grow from n_sequences * initial_points_per_map points per kind"""
        check(self.L.ll_history_batch_enable_cell_maps(self.h, int(initial_points_per_map), cell_resolution, int(threshold_cell_revisit)),
              "ll_history_batch_enable_cell_maps")
        self._cell_resolution = cell_resolution

    def sync_cell_maps(self) -> None:
        """put the stored points of all slots in order now (every reader does so itself when an add came since the last time)"""
        check(self.L.ll_history_batch_sync_cell_maps(self.h), "ll_history_batch_sync_cell_maps")

    def cell_map(self, sequence: int, kind: int) -> "Cell_map_slot":
        return Cell_map_slot(self, int(sequence), int(kind))

    def cell_map_work(self) -> np.ndarray:
        """test tap (ll_history_batch_cell_map_work): points appended, points sorted or gathered inside adds, materialisations, launches of
        the cell-map part of the last add"""
        return self._tap("ll_history_batch_cell_map_work")

    def enable_full_maps(self, initial_points_per_map: int = 1 << 20, cell_resolution: float = 1.0, threshold_cell_revisit: int = 5000) -> None:
        """the full-cloud map of every slot (m_pt_cell_map_full, laser_mapping.hpp:1442, 1527), independent of enable_cell_maps: fed by
        append_full, read as cell_map(s, 2) / full_map(s); the store grows from n_sequences * initial_points_per_map points"""
        check(self.L.ll_history_batch_enable_full_maps(self.h, int(initial_points_per_map), cell_resolution, int(threshold_cell_revisit)),
              "ll_history_batch_enable_full_maps")
        self._full_resolution = cell_resolution
        self._full_min_points = None

    def append_full(self, fe: "Livox_laser", poses, active=None, min_points: int = 3, lists: bool = True):
        """every active slot appends the full selection of scan s of the extractor, moved with poses[s], to its full-cloud map; returns
        per slot the cells [n, 3] its last appended scan touched (Cell_map.append_cloud_touched's list; an inactive slot keeps its own),
        with lists=False only their numbers [S] (full_touched(s) reads a list later)"""
        S = self.n_sequences
        act = _active_mask(active, S)
        poses = _poses(poses, S)
        n = np.zeros(S, np.int64)
        check(self.L.ll_history_batch_append_full_fe(self.h, fe.h, ptr(act), ptr(poses), int(min_points), ptr(n)), "ll_history_batch_append_full_fe")
        self._full_min_points = int(min_points)
        if not lists:
            return n
        return [self.full_touched(s, int(n[s])) for s in range(S)]

    def full_touched(self, sequence: int, n: int | None = None) -> np.ndarray:
        """the cells [n, 3] the last scan appended to slot `sequence`'s full-cloud map touched, in ascending cell order"""
        if n is None:
            c = C.c_int64(0)
            check(self.L.ll_history_batch_full_touched(self.h, int(sequence), None, 0, C.byref(c)), "ll_history_batch_full_touched")
            n = c.value
        ijk = np.zeros((max(1, n), 3), np.int32)
        c = C.c_int64(0)
        check(self.L.ll_history_batch_full_touched(self.h, int(sequence), ptr(ijk), ijk.shape[0], C.byref(c)), "ll_history_batch_full_touched")
        return ijk[:c.value].copy()

    def full_map(self, sequence: int) -> "Full_map_slot":
        return Full_map_slot(self, int(sequence))

    def extract_cells(self, kind: int, sequences, cell_lists, dsts):
        """Key frames' views of the shared cells for several slots in one call (include/loam_livox_hip.h,
        ll_history_batch_extract_cells): request r copies the cells of slot sequences[r]'s map of `kind` (0 corner, 1 surface, 2 full
        cloud) named in cell_lists[r] [n, 3] into the Cell_map dsts[r], on the device, as Cell_map.extract_cells would out of a map
        of the slot's own.  A slot and a destination appear at most once.  Returns [(cells found, points)] per request."""
        R = len(sequences)
        if len(cell_lists) != R or len(dsts) != R:
            raise ValueError(f"{R} sequences, {len(cell_lists)} cell lists, {len(dsts)} destinations")
        seq = np.ascontiguousarray(sequences, np.int32).reshape(R)
        lists = [np.ascontiguousarray(c, np.int32).reshape(-1, 3) for c in cell_lists]
        off = np.zeros(R + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in lists])
        ijk = np.ascontiguousarray(np.concatenate(lists)) if R and off[-1] else None
        arr = _handle_table(dsts)
        nc, npts = np.zeros(max(R, 1), np.int64), np.zeros(max(R, 1), np.int64)
        check(self.L.ll_history_batch_extract_cells(self.h, int(kind), R, ptr(seq), ptr(off), ptr(ijk), arr, ptr(nc), ptr(npts)),
              "ll_history_batch_extract_cells")
        for d, n in zip(dsts, npts):
            d.max_points = max(d.max_points, int(n))
        return [(int(a), int(b)) for a, b in zip(nc[:R], npts[:R])]

    def extract_work(self) -> np.ndarray:
        """test tap (ll_history_batch_extract_work): enqueues and host waits of the last extract_cells, stored points sorted or moved
        by extractions (stays 0), materialisations extractions caused"""
        return self._tap("ll_history_batch_extract_work")

    def full_map_work(self) -> np.ndarray:
        """test tap (ll_history_batch_full_map_work): enqueues and host waits of the last append_full, stored points sorted or gathered
        inside append_full calls, materialisations of the full store"""
        return self._tap("ll_history_batch_full_map_work")

    def enable_scan_log(self, maximum_history_size: int = 100, initial_scans: int | None = None) -> None:
        """the scan log of every slot (m_laser_cloud_full_history, laser_mapping.hpp:1456, kept on the device): fed by log_full behind
        every append_full, trimmed to maximum_history_size scans per slot; it needs enable_full_maps.  The pool of one-scan blocks
        starts with initial_scans of them (n_sequences unless given) and grows by as many"""
        first = self.n_sequences if initial_scans is None else int(initial_scans)
        check(self.L.ll_history_batch_enable_scan_log(self.h, int(maximum_history_size), first), "ll_history_batch_enable_scan_log")

    def log_full(self, fe: "Livox_laser", active=None) -> None:
        """behind the append_full of the same step: the full cloud of every slot named in `active` (all, when None) that the append took
        joins the slot's FIFO, and every FIFO of the append's slots is trimmed (:1456, 1480-1486).  One launch, no host wait."""
        S = self.n_sequences
        act = _active_mask(active, S)
        check(self.L.ll_history_batch_log_full_fe(self.h, fe.h, ptr(act)), "ll_history_batch_log_full_fe")

    def hand_over(self, sequence: int) -> int:
        """the slot's whole FIFO as a group (its id); the FIFO is empty afterwards (:1550-1553, 1558).  Host work only."""
        gid = C.c_int64(0)
        check(self.L.ll_history_batch_scan_log_hand_over(self.h, int(sequence), C.byref(gid)), "ll_history_batch_scan_log_hand_over")
        return int(gid.value)

    def drop_groups(self, group_ids) -> None:
        """the groups' blocks back to the free list"""
        ids = np.ascontiguousarray(group_ids, np.int64).reshape(-1)
        check(self.L.ll_history_batch_scan_log_drop(self.h, len(ids), ptr(ids) if len(ids) else None), "ll_history_batch_scan_log_drop")

    def read_group(self, group_id: int) -> np.ndarray:
        """test tap and debug read: the group's points [n, 4], scan after scan"""
        return self._read_cloud("ll_history_batch_scan_log_read", group_id)

    def scan_log_work(self) -> np.ndarray:
        """test tap (ll_history_batch_scan_log_work): enqueue calls and host waits of the last log_full, blocks in use, blocks allocated"""
        return self._tap("ll_history_batch_scan_log_work")

    def scan_log(self, sequence: int) -> "Scan_log_slot":
        return Scan_log_slot(self, int(sequence))


class Scan_log_slot:
    """Slot s of a History_buffer_batch's scan log, as a Keyframe_assembly sees it (scan_log=): the FIFO lives in the log and the
    owner of the batch makes the push for all slots, so the view only hands the FIFO over and drops the groups nobody will read."""

    def __init__(self, batch: "History_buffer_batch", sequence: int):
        self.batch, self.sequence = batch, sequence

    def hand_over(self) -> int:
        return self.batch.hand_over(self.sequence)

    def drop(self, group_ids) -> None:
        if len(group_ids):
            self.batch.drop_groups(group_ids)


class _Cell_map_readers:
    """stats(), dump() and device_view() of a cell map, for Cell_map (ll_cellmap_*) and for the view of a History_buffer_batch's slot
    (ll_history_batch_cell_map_*): the two families take the same arguments behind what names the map.  A class says in _map() where
    its map is: (library, prefix of the entry points, leading arguments)."""

    def stats(self):
        """(cells, points, m_current_frame_idx)"""
        L, prefix, lead = self._map()
        nc, npts, fr = C.c_int64(0), C.c_int64(0), C.c_int32(0)
        check(getattr(L, prefix + "stats")(*lead, C.byref(nc), C.byref(npts), C.byref(fr)), prefix + "stats")
        return nc.value, npts.value, fr.value

    def dump(self):
        """(xyz [n,3] in (cell, insertion) order, cell indices [c,3], first point of each cell [c+1], last-update frame [c])"""
        L, prefix, lead = self._map()
        nc, npts, _ = self.stats()
        xyzi = np.zeros((max(npts, 1), 4), np.float32)
        ijk = np.zeros((max(nc, 1), 3), np.int32)
        start = np.zeros(nc + 1, np.int32)
        last = np.zeros(max(nc, 1), np.int32)
        check(getattr(L, prefix + "dump")(*lead, ptr(xyzi), xyzi.shape[0], ptr(ijk), ptr(start), ptr(last), ijk.shape[0]), prefix + "dump")
        return xyzi[:npts, :3].copy(), ijk[:nc].copy(), start, last[:nc].copy()

    def device_view(self, device: int = 0):
        """(points (n, 4) float32, cell keys (n,) int64) as torch DEVICE tensors, copied device-to-device out of the handle's arrays
        (which the next append rewrites; a batch's store, which the next add writes behind and may move): the input of
        multigpu.gather_cell_maps, no host hop"""
        import torch
        L, prefix, lead = self._map()
        p, k, n, nc = C.c_void_p(), C.c_void_p(), C.c_int64(0), C.c_int64(0)
        check(getattr(L, prefix + "device_view")(*lead, C.byref(p), C.byref(k), C.byref(n), C.byref(nc)), prefix + "device_view")
        if n.value == 0:
            return torch.zeros((0, 4), dtype=torch.float32, device=f"cuda:{device}"), torch.zeros(0, dtype=torch.int64, device=f"cuda:{device}")
        pts = torch.as_tensor(_DeviceView(p.value, n.value), device=f"cuda:{device}").clone()
        keys = torch.as_tensor(_DeviceView64(k.value, n.value), device=f"cuda:{device}").clone()
        return pts, keys


class Cell_map_slot(_Cell_map_readers):
    """One cell map of one slot of a History_buffer_batch, read the way a Cell_map is: stats(), dump() and device_view(device) have
    Cell_map's return shapes, so what gathers a Cell_map (multigpu.gather_cell_maps) takes a slot's view unchanged."""

    def __init__(self, batch: "History_buffer_batch", sequence: int, kind: int):
        self.batch, self.sequence, self.kind = batch, sequence, kind
        self.resolution = getattr(batch, "_full_resolution" if kind == 2 else "_cell_resolution", None)

    def _map(self):
        return self.batch.L, "ll_history_batch_cell_map_", (self.batch.h, self.sequence, self.kind)

    def extract_cells_into(self, cell_ijk, dst: "Cell_map"):
        """Cell_map.extract_cells for this slot: the one-request form of History_buffer_batch.extract_cells.  (Not named extract_cells:
        a consumer that holds many slots batches its requests; Keyframe_assembly.materialize falls back to this.)"""
        return self.batch.extract_cells(self.kind, [self.sequence], [cell_ijk], [dst])[0]


class Full_map_slot(Cell_map_slot):
    """The full-cloud map of one slot of a History_buffer_batch (kind 2), in the place of the Cell_map a Keyframe_assembly owns:
    stats() and dump() read the slot; append_cloud_touched does NOT append -- the step's one append_full has done that for all slots --
    it answers with the list that append left for this slot; close() leaves the batch alone."""

    def __init__(self, batch: "History_buffer_batch", sequence: int):
        super().__init__(batch, sequence, 2)

    def append_cloud_touched(self, cloud=None, min_points: int = 3) -> np.ndarray:
        used = getattr(self.batch, "_full_min_points", None)
        if used is None:
            raise ValueError("no append_full on the batch yet: there is no list to answer with")
        if int(min_points) != used:
            raise ValueError(f"the batch's append_full listed the cells with min_points={used}, not {min_points}")
        return self.batch.full_touched(self.sequence)

    def close(self):
        pass


def map_grid_geometry(bbox_min_max, cell_size: float):
    """ll_map_grid_geometry (host arithmetic): ((nx, ny, nz), cell, slack) of the search grid over a bounding box"""
    bb = np.ascontiguousarray(bbox_min_max, np.float32).reshape(6)
    dims = np.zeros(3, np.int32)
    h, slack = C.c_float(0), C.c_float(0)
    check(capi.load().ll_map_grid_geometry(ptr(bb), cell_size, ptr(dims), C.byref(h), C.byref(slack)), "ll_map_grid_geometry")
    return (int(dims[0]), int(dims[1]), int(dims[2])), h.value, slack.value


class _DeviceView:
    """(n, 4) float32 at a raw device address, for torch.as_tensor (zero copy)"""

    def __init__(self, address: int, n: int):
        self.__cuda_array_interface__ = {"shape": (int(n), 4), "typestr": "<f4", "data": (int(address), False), "version": 2}


class _DeviceView64:
    """(n,) int64 at a raw device address"""

    def __init__(self, address: int, n: int):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i8", "data": (int(address), False), "version": 2}


class Cell_map(_Handle, _Cell_map_readers):
    """Points_cloud_map<float> (cell_map_keyframe.hpp:477-790) as used by the "cube" matching mode, resident on the
    device (include/loam_livox_hip.h, ll_cellmap_*): append_cloud, find_cells_in_radius + if_pt_in_fov + per-cell
    VoxelGrid (laser_mapping.hpp:475-513)."""

    _destroy = "ll_cellmap_destroy"

    def __init__(self, max_points: int = 1 << 20, resolution: float = 1.0, minimum_revisit_threshold: int = 2**31 - 1, device: int = 0,
                 _borrowed=None):
        super().__init__()
        self.owned = _borrowed is None
        self.resolution = resolution
        self.max_points = int(max_points)
        if self.owned:
            check(self.L.ll_cellmap_create(device, max_points, resolution, minimum_revisit_threshold, C.byref(self.h)), "ll_cellmap_create")
        else:
            self.h = C.c_void_p(_borrowed)

    def close(self):
        if not getattr(self, "owned", True):
            self.h = None   # borrowed (History_buffer.cell_map): the history destroys it
        super().close()

    def _map(self):
        return self.L, "ll_cellmap_", (self.h,)

    def reserve(self, max_points: int) -> None:
        """room for max_points points (no-op when not larger); content, revisit stamps and frame counter are kept"""
        check(self.L.ll_cellmap_reserve(self.h, int(max_points)), "ll_cellmap_reserve")
        self.max_points = max(self.max_points, int(max_points))

    def append_cloud(self, cloud) -> None:
        cloud = capi.as_f32(cloud, 4)
        check(self.L.ll_cellmap_append(self.h, ptr(cloud), cloud.shape[0]), "ll_cellmap_append")

    def extract_cells(self, cell_ijk, dst: "Cell_map"):
        """The cells of this map named in cell_ijk [n, 3], copied on the device into dst (another Cell_map of the same resolution on the
        same device, whose previous content goes and whose capacity grows when the selection does not fit): a key frame's view of the
        shared cells (Maps_keyframe::add_cells keeps pointers to the map's cells and reads them as they are now,
        cell_map_keyframe.hpp:1243-1261).  The list is a set -- order and repeats do not matter, cells the map does not hold are skipped;
        dst ends with the selected cells in cell order, every point in its stored order under the key it had here, and the
        bookkeeping of a fresh map after one append of those points (include/loam_livox_hip.h, ll_cellmap_extract_cells).  Returns
        (cells found, points)."""
        ijk = np.ascontiguousarray(cell_ijk, np.int32).reshape(-1, 3)
        nc, npts = C.c_int64(0), C.c_int64(0)
        check(self.L.ll_cellmap_extract_cells(self.h, ptr(ijk) if len(ijk) else None, len(ijk), dst.h, C.byref(nc), C.byref(npts)),
              "ll_cellmap_extract_cells")
        dst.max_points = max(dst.max_points, npts.value)
        return nc.value, npts.value

    def append_cloud_touched(self, cloud, min_points: int = 3) -> np.ndarray:
        """append_cloud( pts, &cell_vec ) (cell_map_keyframe.hpp:619-672): the append, and the indices [n,3] of the cells that received
        at least min_points of this cloud's points (every touched cell on an empty map)."""
        cloud = capi.as_f32(cloud, 4)
        cap = max(1, cloud.shape[0])
        ijk = np.zeros((cap, 3), np.int32)
        n = C.c_int64(0)
        check(self.L.ll_cellmap_append_touched(self.h, ptr(cloud), cloud.shape[0], int(min_points), ptr(ijk), cap, C.byref(n)),
              "ll_cellmap_append_touched")
        return ijk[:n.value].copy()

    def query_filter(self, pose, radius: float, maximum_in_fov_angle: float, leaf: float, down_sample_replace: int = 1):
        """Returns (concatenated per-cell filtered cloud [n,4], number of selected cells)."""
        pose = np.ascontiguousarray(pose, np.float64)
        nsel, nout = C.c_int64(0), C.c_int64(0)
        check(self.L.ll_cellmap_query_filter(self.h, ptr(pose), radius, maximum_in_fov_angle, leaf, int(down_sample_replace), C.byref(nsel),
                                             C.byref(nout)), "ll_cellmap_query_filter")
        out = np.zeros((nout.value, 4), np.float32)
        if nout.value > 0:
            check(min(0, self.L.ll_cellmap_result(self.h, ptr(out), nout.value)), "ll_cellmap_result")
        return out, nsel.value

    def features(self):
        """determine_feature for every cell (cell_map_keyframe.hpp:436-473), in the cell order of dump():
        dict(type [c] (0 sphere, 1 line, 2 plane), vector [c,3], mean [c,3], cov [c,6], eigen_val [c,3])."""
        nc = self.stats()[0]
        out = dict(type=np.zeros(nc, np.int32), vector=np.zeros((nc, 3), np.float32), mean=np.zeros((nc, 3), np.float32),
                   cov=np.zeros((nc, 6), np.float32), eigen_val=np.zeros((nc, 3), np.float32))
        if nc > 0:
            check(self.L.ll_cellmap_features(self.h, ptr(out["type"]), ptr(out["vector"]), ptr(out["mean"]), ptr(out["cov"]),
                                             ptr(out["eigen_val"]), nc), "ll_cellmap_features")
        return out

    def feature_clouds(self):
        """extract_specify_points( e_feature_line ), ( e_feature_plane ) and get_center() (cell_map_keyframe.hpp:1263-1301), selected on
        the device (ll_cellmap_feature_clouds): (line xyzi [n, 4], plane xyzi [m, 4], centre float32[3]); cells in cell order, every
        cell's points in stored order, intensity 0."""
        line = np.zeros((max(1, self.stats()[1]), 4), np.float32)   # (either cloud holds at most the map's points)
        plane = np.zeros_like(line)
        nl, npl, centre = C.c_int64(0), C.c_int64(0), np.zeros(3, np.float32)
        check(self.L.ll_cellmap_feature_clouds(self.h, ptr(line), line.shape[0], C.byref(nl), ptr(plane), plane.shape[0], C.byref(npl), ptr(centre)),
              "ll_cellmap_feature_clouds")
        return line[:nl.value].copy(), plane[:npl.value].copy(), centre

    def keyframe_images(self, roi_ratio: float = 0.9):
        """Maps_keyframe::analyze over the cells of this map (cell_map_keyframe.hpp:1385-1493): dict(images [4,60,60] =
        line, plane, line_roi, plane_roi; ratio_nonzero [4]; eigen_R [2,3,3]; n_vectors [4]; centre [3]; roi_range)."""
        out = _keyframe_outputs()
        check(self.L.ll_cellmap_keyframe_images(self.h, roi_ratio, *map(ptr, out)), "ll_cellmap_keyframe_images")
        return _keyframe_result(*out)


class Scene_aligner(_Handle):
    """The device route of Scene_alignment::find_tranfrom_of_two_mappings (scene_alignment.hpp:269-391; ll_scene_align_*): one registrar,
    one map, one voxel filter, the selected clouds and their filtered forms, kept between calls and grown from initial_points.  No point of either key
    frame crosses to the host."""

    _destroy = "ll_scene_align_destroy"

    def __init__(self, initial_points: int = 1 << 16, device: int = 0):
        super().__init__()
        check(self.L.ll_scene_align_create(device, int(initial_points), C.byref(self.h)), "ll_scene_align_create")
        self.params = capi.scene_align_default_params()

    def run(self, keyframe_a: "Cell_map", keyframe_b: "Cell_map"):
        """(pose float64[7] = m_q_w_curr, m_t_w_curr; m_inlier_threshold; the reports of the registrations run)"""
        pose, thr, n = np.zeros(7, np.float64), C.c_double(0.0), C.c_int32(0)
        reports = (RegReport * 3)()
        check(self.L.ll_scene_align_run(self.h, keyframe_a.h, keyframe_b.h, C.byref(self.params), ptr(pose), C.byref(thr), reports, C.byref(n)),
              "ll_scene_align_run")
        out = []
        for i in range(n.value):   # (copies: the array goes with this call)
            r = RegReport()
            C.memmove(C.byref(r), C.byref(reports[i]), C.sizeof(RegReport))
            out.append(r)
        return pose, float(thr.value), out

    def work(self) -> np.ndarray:
        """test tap (ll_scene_align_work) on the last run: bytes of point data copied between host and device, host waits,
        registrations run, enqueues of the selection step"""
        return self._tap("ll_scene_align_work")


class Keyframe_bank(_Handle):
    """The key-frame descriptor bank (ll_keyframe_bank_*): the line and plane direction image of every processed key frame stay on the
    device with their norms; match answers "these (new, old) pairs" in one launch chain and one host wait, with keyframe_similarity's
    floats bit for bit.  An entry's id is its position in the order of the adds; the capacity doubles on demand."""

    _destroy = "ll_keyframe_bank_destroy"

    def __init__(self, initial_entries: int = 256, device: int = 0):
        super().__init__()
        check(self.L.ll_keyframe_bank_create(device, int(initial_entries), C.byref(self.h)), "ll_keyframe_bank_create")

    def __len__(self):
        return int(check(self.L.ll_keyframe_bank_size(self.h), "ll_keyframe_bank_size"))

    def add_cell_map(self, cell_map: "Cell_map", roi_ratio: float = 0.9):
        """(Cell_map.keyframe_images( roi_ratio ) of the map, the id of the new entry): images 0 and 1 go into the bank device to device"""
        out, eid = _keyframe_outputs(), C.c_int64(-1)
        check(self.L.ll_keyframe_bank_add_cellmap(self.h, cell_map.h, roi_ratio, *map(ptr, out), C.byref(eid)), "ll_keyframe_bank_add_cellmap")
        return _keyframe_result(*out), int(eid.value)

    def add_images(self, img_line, img_plane) -> int:
        """an entry from two 60 x 60 host images; returns its id"""
        a, b = np.ascontiguousarray(img_line, np.float32), np.ascontiguousarray(img_plane, np.float32)
        if a.shape != (60, 60) or b.shape != (60, 60):
            raise ValueError("direction images are 60 x 60")
        eid = C.c_int64(-1)
        check(self.L.ll_keyframe_bank_add_images(self.h, ptr(a), ptr(b), C.byref(eid)), "ll_keyframe_bank_add_images")
        return int(eid.value)

    def images(self, entry: int):
        """(line image, plane image) of an entry, read back"""
        a, b = np.zeros((60, 60), np.float32), np.zeros((60, 60), np.float32)
        check(self.L.ll_keyframe_bank_images(self.h, int(entry), ptr(a), ptr(b)), "ll_keyframe_bank_images")
        return a, b

    def match(self, ids_a, ids_b):
        """(sim_line float32[n], sim_plane float32[n]) of the ordered pairs ( ids_a[p], ids_b[p] ): a is the new key frame, b the old one"""
        a, b = np.ascontiguousarray(ids_a, np.int64).reshape(-1), np.ascontiguousarray(ids_b, np.int64).reshape(-1)
        if len(a) != len(b):
            raise ValueError("ids_a and ids_b differ in length")
        line, plane = np.zeros(len(a), np.float32), np.zeros(len(a), np.float32)
        check(self.L.ll_keyframe_bank_match(self.h, len(a), ptr(a), ptr(b), ptr(line), ptr(plane)), "ll_keyframe_bank_match")
        return line, plane

    def surface(self, id_a: int, id_b: int, kind: int) -> np.ndarray:
        """test tap (ll_keyframe_bank_debug_surface): the correlation sums of one pair and kind (0 line, 1 plane) over all 60 x 60 shifts"""
        out = np.zeros((60, 60), np.float64)
        check(self.L.ll_keyframe_bank_debug_surface(self.h, int(id_a), int(id_b), int(kind), ptr(out)), "ll_keyframe_bank_debug_surface")
        return out

    def work(self) -> np.ndarray:
        """test tap (ll_keyframe_bank_work) on the last match: enqueues, host waits, image bytes copied between host and device, pairs"""
        return self._tap("ll_keyframe_bank_work")


def map_refine_affine(pose_ori, pose_opm):
    """(R_aff float32[3, 3], T_aff float32[3]) of refine_pts (ceres_pose_graph_3d.hpp:444-445) from two poses {qx, qy, qz, qw, tx, ty, tz};
    host arithmetic only (ll_map_refine_affine)"""
    a, b = np.ascontiguousarray(pose_ori, np.float64).reshape(7), np.ascontiguousarray(pose_opm, np.float64).reshape(7)
    R, T = np.zeros((3, 3), np.float32), np.zeros(3, np.float32)
    check(capi.load().ll_map_refine_affine(ptr(a), ptr(b), ptr(R), ptr(T)), "ll_map_refine_affine")
    return R, T


class Map_refine(_Handle):
    """The key-frame map refinement (ll_map_refine_*): Mapping_refine of ceres_pose_graph_3d.hpp:368-538 over key-frame clouds that stay
    on the device.  add_cloud filters an accumulated cloud into the store and returns its id (its position in the order of the adds);
    refine moves and filters any selection of them in one launch chain and one host wait; merge filters the last outputs as one cloud."""

    _destroy = "ll_map_refine_destroy"

    def __init__(self, initial_points: int = 1 << 20, device: int = 0):
        super().__init__()
        check(self.L.ll_map_refine_create(device, int(initial_points), C.byref(self.h)), "ll_map_refine_create")

    def __len__(self):
        return int(check(self.L.ll_map_refine_size(self.h), "ll_map_refine_size"))

    def add_cloud(self, cloud, leaf: float = 0.5):
        """(id, points kept, status) of a cloud [n, 4] filtered with `leaf` (surround_pointcloud_resolution, laser_mapping.hpp:943-946)"""
        c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        cid, kept, st = C.c_int64(-1), C.c_int64(0), C.c_int32(0)
        check(self.L.ll_map_refine_add_cloud(self.h, ptr(c), len(c), leaf, C.byref(cid), C.byref(kept), C.byref(st)), "ll_map_refine_add_cloud")
        return int(cid.value), int(kept.value), int(st.value)

    def add_logged(self, batch: "History_buffer_batch", groups_per_request, leaf: float = 0.5):
        """add_cloud for several key frames at once, device to device: request r is the concatenation of the logged scans of the groups
        groups_per_request[r] (ids of batch.hand_over) -- one gather, one filter chain, one host wait for all of them.  The groups are
        consumed.  Returns (ids [R], points kept [R], status [R]); bit for bit what add_cloud gives for the same points."""
        if not isinstance(batch, History_buffer_batch):
            raise TypeError("add_logged reads the scan log of a History_buffer_batch")
        lists = [np.ascontiguousarray(g, np.int64).reshape(-1) for g in groups_per_request]
        R = len(lists)
        off = np.zeros(R + 1, np.int64)
        off[1:] = np.cumsum([len(g) for g in lists])
        gids = np.ascontiguousarray(np.concatenate(lists)) if R and off[-1] else None
        ids, kept, st = np.zeros(max(R, 1), np.int64), np.zeros(max(R, 1), np.int64), np.zeros(max(R, 1), np.int32)
        check(self.L.ll_map_refine_add_logged(self.h, batch.h, R, ptr(off), ptr(gids), leaf, ptr(ids), ptr(kept), ptr(st)), "ll_map_refine_add_logged")
        return ids[:R], kept[:R], st[:R]

    def add_stored(self, cloud) -> int:
        """the id of a cloud [n, 4] stored as it is: one that is filtered already (a map_id_pc entry kept on the host)"""
        c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        cid = C.c_int64(-1)
        check(self.L.ll_map_refine_add_stored(self.h, ptr(c), len(c), C.byref(cid)), "ll_map_refine_add_stored")
        return int(cid.value)

    def cloud(self, cloud_id: int) -> np.ndarray:
        """a stored cloud [n, 4], read back"""
        return self._read_cloud("ll_map_refine_cloud", cloud_id)

    def run(self, ids, poses_ori, poses_opm, leaf: float = 0.2, transform_first: bool = False):
        """(offsets int64[n_sel + 1], status int32[n_sel]) of a run whose outputs stay on the device"""
        ids = np.ascontiguousarray(ids, np.int64).reshape(-1)
        a, b = _poses(poses_ori, -1), _poses(poses_opm, -1)
        if len(a) != len(ids) or len(b) != len(ids):
            raise ValueError("a pose pair per selected id")
        offsets, status = np.zeros(len(ids) + 1, np.int64), np.zeros(len(ids), np.int32)
        check(self.L.ll_map_refine_run(self.h, 1 if transform_first else 0, len(ids), ptr(ids), ptr(a), ptr(b), leaf, ptr(offsets), ptr(status)),
              "ll_map_refine_run")
        self.status = status
        return offsets, status

    def refine(self, ids, poses_ori, poses_opm, leaf: float = 0.2, transform_first: bool = False) -> list:
        """the corrected clouds [n, 4] (intensity 0) of the selected ids, in selection order: refine_pointcloud( ..., if_save = 0 ) per id,
        or with transform_first refine_mapping's move-then-filter.  The status values of the run are left in self.status."""
        offsets, _ = self.run(ids, poses_ori, poses_opm, leaf, transform_first)
        flat = np.zeros((int(offsets[-1]), 4), np.float32)
        check(self.L.ll_map_refine_fetch(self.h, ptr(flat), len(flat)), "ll_map_refine_fetch")
        return [flat[offsets[s]:offsets[s + 1]].copy() for s in range(len(offsets) - 1)]

    def merge(self, leaf: float = 0.2) -> np.ndarray:
        """VoxelGrid over the last run's concatenated outputs (ceres_pose_graph_3d.hpp:577-578): the single corrected map [n, 4]"""
        n, st = C.c_int64(0), C.c_int32(0)
        check(self.L.ll_map_refine_merge(self.h, leaf, C.byref(n), C.byref(st)), "ll_map_refine_merge")
        out = np.zeros((int(n.value), 4), np.float32)
        check(self.L.ll_map_refine_fetch_merged(self.h, ptr(out), len(out)), "ll_map_refine_fetch_merged")
        self.merge_status = int(st.value)
        return out

    def work(self) -> np.ndarray:
        """test tap (ll_map_refine_work) on the last add / run / merge and its fetch: the host's enqueue calls (the sort and the scan one
        each), host waits, bytes between host and device, points of the chain"""
        return self._tap("ll_map_refine_work")


class Pose_graph(_Handle):
    """The pose-graph optimiser (ll_pose_graph_*): Ceres_pose_graph_3d::pose_graph_optimization (ceres_pose_graph_3d.hpp:336-352) for
    any number of independent graphs in one launch and one host wait.  A graph is a dict: poses [N, 7] {qx, qy, qz, qw, tx, ty, tz}
    (pose 0 is held constant), ab [E, 2] pose ids of every edge, meas [E, 7] in the pose layout, and optionally information [E, 36].
    The handle's capacities grow on demand (the handle is created again, larger: it keeps nothing between calls)."""

    _destroy = "ll_pose_graph_destroy"

    def __init__(self, max_graphs: int = 16, max_poses: int = 4096, max_edges: int = 8192, max_envelope_blocks: int = 1 << 16, device: int = 0,
                 params=None):
        super().__init__()
        self.device = device
        self.params = params if params is not None else capi.pose_graph_default_params()
        self._create([int(max_graphs), int(max_poses), int(max_edges), int(max_envelope_blocks)])

    def _create(self, capacity):
        self.close()
        h = C.c_void_p()
        check(self.L.ll_pose_graph_create(self.device, *capacity, C.byref(h)), "ll_pose_graph_create")
        self.h, self.capacity = h, list(capacity)

    @staticmethod
    def envelope_blocks(n_poses: int, ab) -> int:
        """6 x 6 blocks of the block envelope of a graph's normal matrix: row f (pose f + 1) reaches back to the lowest free pose an
        edge joins it to"""
        first = np.arange(max(n_poses - 1, 0), dtype=np.int64)
        ab = np.asarray(ab, np.int64).reshape(-1, 2)
        if len(ab) == 0 or len(first) == 0:
            return len(first)
        lo, hi = ab.min(axis=1) - 1, ab.max(axis=1) - 1
        ok = (lo >= 0) & (hi < len(first))
        np.minimum.at(first, hi[ok], lo[ok])
        return int(np.sum(np.arange(len(first)) - first + 1))

    def solve(self, graphs):
        """-> (poses: one [N, 7] array per graph, summaries: one dict per graph with iterations, successful_steps, unsuccessful_steps,
        initial_cost, final_cost, termination (a name of capi.POSE_GRAPH_TERMINATION)).  The inputs are not modified."""
        graphs = list(graphs)
        G = len(graphs)
        poses = [np.array(g["poses"], np.float64).reshape(-1, 7) for g in graphs]
        abs_ = [np.ascontiguousarray(g["ab"], np.int32).reshape(-1, 2) for g in graphs]
        meas = [np.ascontiguousarray(g["meas"], np.float64).reshape(-1, 7) for g in graphs]
        for p, a, m in zip(poses, abs_, meas):
            if len(a) != len(m):
                raise ValueError("a graph's ab and meas differ in length")
        info = None
        if any(g.get("information") is not None for g in graphs):
            info = [np.asarray(g["information"], np.float64).reshape(-1, 36) if g.get("information") is not None
                    else np.tile(np.eye(6).ravel(), (len(a), 1)) for g, a in zip(graphs, abs_)]
            for i, a in zip(info, abs_):
                if len(i) != len(a):
                    raise ValueError("a graph's ab and information differ in length")
            info = np.ascontiguousarray(np.concatenate(info)) if G else None
        po = np.cumsum([0] + [len(p) for p in poses]).astype(np.int64)
        eo = np.cumsum([0] + [len(a) for a in abs_]).astype(np.int64)
        x = np.ascontiguousarray(np.concatenate(poses)) if G else np.zeros((0, 7))
        ab = np.ascontiguousarray(np.concatenate(abs_)) if G else np.zeros((0, 2), np.int32)
        ms = np.ascontiguousarray(np.concatenate(meas)) if G else np.zeros((0, 7))
        need = [G, len(x), len(ab), sum(self.envelope_blocks(len(p), a) for p, a in zip(poses, abs_))]
        if any(n > c for n, c in zip(need, self.capacity)):
            self._create([max(c, 2 * n if n > c else 1) for n, c in zip(need, self.capacity)])
        summary = (capi.PoseGraphSummary * max(G, 1))()
        check(self.L.ll_pose_graph_solve(self.h, C.byref(self.params), G, ptr(po), ptr(x), ptr(eo), ptr(ab), ptr(ms), ptr(info), summary),
              "ll_pose_graph_solve")
        out = [dict(iterations=s.iterations, successful_steps=s.successful_steps, unsuccessful_steps=s.unsuccessful_steps,
                    initial_cost=s.initial_cost, final_cost=s.final_cost, termination=capi.POSE_GRAPH_TERMINATION[s.termination])
               for s in summary[:G]]
        return [x[po[g]:po[g + 1]].copy() for g in range(G)], out

    def work(self) -> np.ndarray:
        """test tap (ll_pose_graph_work) on the last solve: enqueues, host waits, envelope blocks, graphs"""
        return self._tap("ll_pose_graph_work")


def _q_mul(a, b):
    """Eigen's quaternion product on {x, y, z, w}, term for term"""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], np.float64)


def _q_inverse(q):
    """Eigen's inverse(): the conjugate over the squared norm"""
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2], np.float64)


def _q_rotate(q, v):
    """Eigen's quaternion * vector: uv = 2 (u x v); v + w uv + u x uv"""
    u = q[:3]
    uv = np.cross(u, v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(u, uv)


def relative_constraint(pose_prev, pose_curr) -> np.ndarray:
    """The chain constraint of two consecutive key-frame poses (laser_mapping.hpp:954-958) as a measurement {q, t}:
    relative_Q = q_prev^-1 q_curr, relative_T = q_prev^-1 ( t_curr - t_prev ).  fp64, on the host."""
    a, b = np.asarray(pose_prev, np.float64).reshape(7), np.asarray(pose_curr, np.float64).reshape(7)
    qi = _q_inverse(a[:4])
    return np.concatenate([_q_mul(qi, b[:4]), _q_rotate(qi, b[4:7] - a[4:7])])


def loop_constraint(s_idx: int, t_idx: int, pose_a, pose_b, icp_q, icp_t):
    """Scene_alignment::add_constrain_of_loop (scene_alignment.hpp:97-129): (s_idx, t_idx, measurement {q, t}) with
    q_res = q_b^-1 icp_q^-1 q_a and t_res = q_b^-1 ( icp_q^-1 ( t_a - icp_t ) - t_b ).  The detector calls it with s_idx the new key
    frame, t_idx the old one, pose_a the OLD key frame's pose and pose_b the new one's (laser_mapping.hpp:1058-1078)."""
    a, b = np.asarray(pose_a, np.float64).reshape(7), np.asarray(pose_b, np.float64).reshape(7)
    iq, it = np.asarray(icp_q, np.float64).reshape(4), np.asarray(icp_t, np.float64).reshape(3)
    qbi, qii = _q_inverse(b[:4]), _q_inverse(iq)
    q_res = _q_mul(_q_mul(qbi, qii), a[:4])
    t_res = _q_rotate(qbi, _q_rotate(qii, a[4:7] - it) - b[4:7])
    return int(s_idx), int(t_idx), np.concatenate([q_res, t_res])


def keyframe_similarity(img_a, img_b, device: int = 0) -> float:
    """Maps_keyframe::max_similiarity_of_two_image (cell_map_keyframe.hpp:1155-1224) of two 60 x 60 direction images."""
    a, b = np.ascontiguousarray(img_a, np.float32), np.ascontiguousarray(img_b, np.float32)
    if a.shape != (60, 60) or b.shape != (60, 60):
        raise ValueError("direction images are 60 x 60")
    out = C.c_float(0)
    check(capi.load().ll_keyframe_similarity(device, ptr(a), ptr(b), C.byref(out)), "ll_keyframe_similarity")
    return float(out.value)


class Map_buffer(_Handle):
    """m_laser_cloud_{corner,surf}_from_map + their kd-trees (laser_mapping.hpp:539-546) as device grids."""

    _destroy = "ll_map_destroy"

    CORNER, SURF = 0, 1

    def __init__(self, device: int = 0):
        super().__init__()
        check(self.L.ll_map_create(device, C.byref(self.h)), "ll_map_create")

    def setInputCloud(self, kind: int, cloud: np.ndarray, cell_size: float = 0.0):
        cloud = np.ascontiguousarray(cloud, np.float32)
        assert cloud.ndim == 2 and cloud.shape[1] >= 3
        check(self.L.ll_map_upload(self.h, kind, ptr(cloud), cloud.shape[1], cloud.shape[0], cell_size), "ll_map_upload")

    def size(self, kind: int) -> int:
        return int(self.L.ll_map_size(self.h, kind))

    def cells(self, kind: int) -> int:
        return int(self.L.ll_map_cells(self.h, kind))

    def to_f16(self, kind: int):
        """fp16-point records for this kind (BASELINE config C5); the registrar cannot use the map afterwards"""
        check(self.L.ll_map_to_f16(self.h, kind), "ll_map_to_f16")

    def dequantized(self, kind: int) -> np.ndarray:
        n = self.size(kind)
        out = np.zeros((n, 3), np.float32)
        check(self.L.ll_map_dequantized(self.h, kind, ptr(out), n), "ll_map_dequantized")
        return out

    def nearestKSearch(self, kind: int, queries: np.ndarray, max_sq_dis: float):
        q = capi.as_f32(queries, 3)
        idx = np.zeros((q.shape[0], 5), np.int32)
        d2 = np.zeros((q.shape[0], 5), np.float32)
        check(self.L.ll_map_knn5(self.h, kind, ptr(q), q.shape[0], max_sq_dis, ptr(idx), ptr(d2)), "ll_map_knn5")
        return idx, d2


    def nearestKSearch_device(self, kind: int, queries, max_sq_dis: float, idx_out, d2_out) -> float:
        """The same search on torch DEVICE tensors (queries (n, 3) float32, idx_out (n, 5) int32, d2_out (n, 5) float32, contiguous):
        nothing crosses PCIe.  Returns the search kernel's duration in ms (HIP events on the map's stream)."""
        n = int(queries.shape[0])
        assert queries.is_contiguous() and idx_out.is_contiguous() and d2_out.is_contiguous() and queries.shape[1] == 3
        ms = C.c_float(0)
        check(self.L.ll_map_knn5_device(self.h, kind, C.c_void_p(queries.data_ptr()), n, max_sq_dis, C.c_void_p(idx_out.data_ptr()),
                                        C.c_void_p(d2_out.data_ptr()), C.byref(ms)), "ll_map_knn5_device")
        return float(ms.value)


class Point_cloud_registration(_Handle):
    """Device-backed Point_cloud_registration.  Configuration fields keep the reference names
    (point_cloud_registration.hpp:45-103); poses are the m_q_w_*/m_t_w_* pairs packed as float64[7]."""

    _destroy = "ll_reg_destroy"

    def __init__(self, max_scans: int = 1, max_features: int = 24000, device: int = 0):
        super().__init__()
        check(self.L.ll_reg_create(device, max_scans, max_features, C.byref(self.h)), "ll_reg_create")
        self.params = capi.reg_default_params()
        self.max_scans = max_scans
        ident = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
        self.m_pose_w_last = ident.copy()   # m_q_w_last, m_t_w_last
        self.m_pose_w_curr = ident.copy()   # m_q_w_curr, m_t_w_curr
        self.m_para_buffer_incremental = ident.copy()
        self.report = RegReport()
        self.m_inlier_threshold = 0.0

    def find_out_incremental_transfrom(self, map_buffer: Map_buffer, laserCloudCornerStack: np.ndarray,
                                       laserCloudSurfStack: np.ndarray) -> int:
        c = capi.as_f32(laserCloudCornerStack, 4)
        s = capi.as_f32(laserCloudSurfStack, 4)
        pl = np.ascontiguousarray(self.m_pose_w_last, np.float64)
        pc = np.ascontiguousarray(self.m_pose_w_curr, np.float64).copy()
        pi = np.ascontiguousarray(self.m_para_buffer_incremental, np.float64).copy()
        rep = RegReport()
        ret = check(self.L.ll_reg_solve(self.h, map_buffer.h, ptr(c), c.shape[0], ptr(s), s.shape[0], C.byref(self.params),
                                        ptr(pl), ptr(pc), ptr(pi), C.byref(rep)), "ll_reg_solve")
        self.m_pose_w_curr, self.m_para_buffer_incremental, self.report = pc, pi, rep
        self.m_inlier_threshold = rep.inlier_threshold
        return ret

    @staticmethod
    def _pack_features(corners: list, surfs: list):
        """ragged feature clouds as the library takes them: (n, corner [n, stride, 4], counts [n], stride, and the same of the surfaces)"""
        n = len(corners)
        nc = np.array([len(c) for c in corners], np.int32)
        ns = np.array([len(s) for s in surfs], np.int32)
        sc, ss = max(1, int(nc.max())), max(1, int(ns.max()))
        cbuf = np.zeros((n, sc, 4), np.float32)
        sbuf = np.zeros((n, ss, 4), np.float32)
        for i in range(n):
            cbuf[i, :nc[i]] = corners[i]
            sbuf[i, :ns[i]] = surfs[i]
        return n, cbuf, nc, sc, sbuf, ns, ss

    def solve_batch(self, map_buffer: Map_buffer, corners: list, surfs: list, poses_last: np.ndarray, poses_curr: np.ndarray):
        n, cbuf, nc, sc, sbuf, ns, ss = self._pack_features(corners, surfs)
        pl = _poses(poses_last, n)
        pc = _poses(poses_curr, n).copy()
        pi = np.tile(np.array([0, 0, 0, 1, 0, 0, 0], np.float64), (n, 1))
        reps = (RegReport * n)()
        res = np.zeros(n, np.int32)
        check(self.L.ll_reg_solve_batch(self.h, map_buffer.h, n, ptr(cbuf), ptr(nc), sc, ptr(sbuf), ptr(ns), ss,
                                        C.byref(self.params), ptr(pl), ptr(pc), ptr(pi), reps, ptr(res)), "ll_reg_solve_batch")
        return res, pc, pi, list(reps)

    def upload_features(self, corners: list, surfs: list):
        """Host feature clouds -> the registrar's HBM buffers (the upload half of solve_batch)."""
        n, cbuf, nc, sc, sbuf, ns, ss = self._pack_features(corners, surfs)
        check(self.L.ll_reg_upload_features(self.h, n, ptr(cbuf), ptr(nc), sc, ptr(sbuf), ptr(ns), ss), "ll_reg_upload_features")
        return n

    def _enqueue(self, name: str, sources, n_scans: int, poses_last, poses_curr, heads=(), frame_index=()):
        """the eight enqueues: the entry point's own handles and settings (`sources`: the map or the table of maps, the extractor, the
        filters), the number of scans (and the heads of a merged scan), the parameters (and the frame indices of a map per slot), the
        two pose blocks; no completion flag"""
        pl, pc = _poses(poses_last, n_scans), _poses(poses_curr, n_scans)
        self._call(name, *sources, n_scans, *heads, C.byref(self.params), *frame_index, ptr(pl), ptr(pc), None)

    def enqueue_uploaded(self, map_buffer: Map_buffer, n_scans: int, poses_last, poses_curr):
        self._enqueue("ll_reg_enqueue_uploaded", (map_buffer.h,), n_scans, poses_last, poses_curr)

    def enqueue_fe(self, map_buffer: Map_buffer, fe: Livox_laser, n_scans: int, poses_last, poses_curr):
        self._enqueue("ll_reg_enqueue_fe", (map_buffer.h, fe.h), n_scans, poses_last, poses_curr)

    def enqueue_fe_merged(self, map_buffer: Map_buffer, fe: Livox_laser, n_scans: int, heads: int, poses_last, poses_curr):
        """Mid-100 (laser_feature_extractor.hpp:348-358): registrar scan b = the selected features of extractor slots
        b * heads ... b * heads + heads - 1, concatenated on the device (corner clouds together, surface clouds together)."""
        self._enqueue("ll_reg_enqueue_fe_merged", (map_buffer.h, fe.h), n_scans, poses_last, poses_curr, heads=(int(heads),))

    def enqueue_fe_downsampled(self, map_buffer: Map_buffer, fe: Livox_laser, vox_corner: "VoxelGrid", vox_surf: "VoxelGrid",
                               line_res: float, plane_res: float, n_scans: int, poses_last, poses_curr):
        """m_if_input_downsample_mode (laser_mapping.hpp:1367-1373): voxel-filter the selected features on the device, then
        register them."""
        self._enqueue("ll_reg_enqueue_fe_downsampled", (map_buffer.h, fe.h, vox_corner.h, vox_surf.h, line_res, plane_res), n_scans, poses_last, poses_curr)

    def set_time_ranges(self, min_ts, max_ts) -> None:
        """ll_reg_set_time_ranges: a time range per scan for the NEXT enqueue_fe_maps / enqueue_fe_downsampled_maps only -- slot b runs
        over (min_ts[b], max_ts[b]) wherever a registration reads params.minimum_pt_time_stamp / maximum_pt_time_stamp, which is what
        params.if_motion_deblur = 1 needs with a map per slot.  A single-map enqueue with a table pending is refused."""
        lo, hi = np.ascontiguousarray(min_ts, np.float32).reshape(-1), np.ascontiguousarray(max_ts, np.float32).reshape(-1)
        if len(lo) != len(hi):
            raise ValueError(f"{len(lo)} minimum and {len(hi)} maximum time stamps")
        check(self.L.ll_reg_set_time_ranges(self.h, ptr(lo), ptr(hi), len(lo)), "ll_reg_set_time_ranges")

    def _maps_args(self, maps, n_scans: int, frame_index):
        """the handle table and the frame indices of a map-per-slot enqueue (None in maps = an idle slot)"""
        if len(maps) != n_scans:
            raise ValueError(f"maps has {len(maps)} entries for {n_scans} scans")
        fi = None
        if frame_index is not None:
            fi = np.ascontiguousarray(frame_index, np.int32).reshape(n_scans)
        return _handle_table(maps), (ptr(fi),)

    def enqueue_fe_maps(self, maps, fe: Livox_laser, n_scans: int, poses_last, poses_curr, frame_index=None):
        """enqueue_fe with a map per slot (ll_reg_enqueue_fe_maps): scan b is registered against maps[b] (a Map_buffer, or None for an
        idle slot) with frame_index[b] (None: params.current_frame_index for every slot); the start-up gate is decided per slot."""
        tab, fi = self._maps_args(maps, n_scans, frame_index)
        self._enqueue("ll_reg_enqueue_fe_maps", (tab, fe.h), n_scans, poses_last, poses_curr, frame_index=fi)

    def enqueue_fe_downsampled_maps(self, maps, fe: Livox_laser, vox_corner: "VoxelGrid", vox_surf: "VoxelGrid", line_res: float, plane_res: float,
                                    n_scans: int, poses_last, poses_curr, frame_index=None):
        """enqueue_fe_downsampled with a map per slot (ll_reg_enqueue_fe_downsampled_maps)"""
        tab, fi = self._maps_args(maps, n_scans, frame_index)
        self._enqueue("ll_reg_enqueue_fe_downsampled_maps", (tab, fe.h, vox_corner.h, vox_surf.h, line_res, plane_res), n_scans, poses_last, poses_curr,
                      frame_index=fi)

    def enqueue_spin(self, map_buffer: Map_buffer, spin: "Spinning_laser", n_scans: int, poses_last, poses_curr):
        """enqueue_fe for a spinning-lidar handle: corner stack = its less-sharp cloud, surface stack = its less-flat cloud, read where
        the extractor left them (ll_reg_enqueue_spin).  params.if_motion_deblur must be 0."""
        self._enqueue("ll_reg_enqueue_spin", (map_buffer.h, spin.h), n_scans, poses_last, poses_curr)

    def enqueue_spin_downsampled(self, map_buffer: Map_buffer, spin: "Spinning_laser", vox_corner: "VoxelGrid", vox_surf: "VoxelGrid",
                                 line_res: float, plane_res: float, n_scans: int, poses_last, poses_curr):
        """enqueue_fe_downsampled for a spinning-lidar handle (m_if_input_downsample_mode, laser_mapping.hpp:1367-1373)"""
        self._enqueue("ll_reg_enqueue_spin_downsampled", (map_buffer.h, spin.h, vox_corner.h, vox_surf.h, line_res, plane_res), n_scans, poses_last,
                      poses_curr)

    def collect(self, n_scans: int):
        pc = np.zeros((n_scans, 7), np.float64)
        pi = np.zeros((n_scans, 7), np.float64)
        reps = (RegReport * n_scans)()
        res = np.zeros(n_scans, np.int32)
        check(self.L.ll_reg_collect(self.h, n_scans, ptr(pc), ptr(pi), reps, ptr(res)), "ll_reg_collect")
        return res, pc, pi, list(reps)

    def solve_batch_fe(self, map_buffer: Map_buffer, fe: Livox_laser, n_scans: int, poses_last, poses_curr):
        self.enqueue_fe(map_buffer, fe, n_scans, poses_last, poses_curr)
        return self.collect(n_scans)

    def set_debug(self, enable: bool = True, force_general_solver: bool = False, no_knn_reuse: bool = False,
                  reuse_from_iter1: bool = False, no_solver_groups: bool = False,
                  test_group_abort: bool = False, no_knn_coop: bool = False, no_knn_tile: bool = False,
                  knn_tile_with_reuse: bool = False, knn_tile_small_batches: bool = False, no_line_cache: bool = False,
                  no_small_solver: bool = False, small_solver_waves: int = 0, no_solve_order: bool = False, no_knn_sparse: bool = False):
        flags = (int(bool(enable)) | (2 if force_general_solver else 0) | (4 if no_knn_reuse else 0) | (8 if reuse_from_iter1 else 0)
                 | (32 if no_solver_groups else 0)
                 | (128 if test_group_abort else 0) | (256 if no_knn_coop else 0) | (512 if no_knn_tile else 0)
                 | (1024 if knn_tile_with_reuse else 0) | (2048 if knn_tile_small_batches else 0) | (4096 if no_line_cache else 0)
                 | (32768 if no_small_solver else 0) | {0: 0, 1: 65536, 4: 131072, 2: 65536 | 131072}[int(small_solver_waves)] | (262144 if no_solve_order else 0)
                 | (524288 if no_knn_sparse else 0))
        self.set_debug_flags(flags)

    def set_debug_flags(self, flags: int):
        """ll_reg_set_debug with the raw flag word (kept in self.debug_flags, so a caller can add a bit and put the word back)"""
        check(self.L.ll_reg_set_debug(self.h, int(flags)), "ll_reg_set_debug")
        self.debug_flags = int(flags)

    def set_debug_knn_iteration(self, icp_iteration: int):
        """the ICP iteration whose neighbour lists debug_knn() returns (default 0)"""
        check(self.L.ll_reg_set_debug_knn_iteration(self.h, int(icp_iteration)), "ll_reg_set_debug_knn_iteration")

    def debug_knn(self, scan: int, n_corner: int, n_surf: int):
        ci, cd = np.zeros((n_corner, 5), np.int32), np.zeros((n_corner, 5), np.float32)
        si, sd = np.zeros((n_surf, 5), np.int32), np.zeros((n_surf, 5), np.float32)
        check(self.L.ll_reg_debug_knn(self.h, scan, ptr(ci), ptr(cd), ptr(si), ptr(sd)), "ll_reg_debug_knn")
        return ci, cd, si, sd

    def debug_blocks(self, scan: int, n_corner: int, n_surf: int):
        """what the solver reads of a scan after a registration: (corner nn [n, 4], corner flag [n], surface nn, surface flag) -- the
        neighbour positions + found flag and the block flag as built, whichever ICP iteration established them"""
        cn, cf = np.zeros((n_corner, 4), np.int32), np.zeros(n_corner, np.uint8)
        sn, sf = np.zeros((n_surf, 4), np.int32), np.zeros(n_surf, np.uint8)
        check(self.L.ll_reg_debug_blocks(self.h, scan, ptr(cn), ptr(cf), ptr(sn), ptr(sf)), "ll_reg_debug_blocks")
        return cn, cf, sn, sf

    def set_profiling(self, enable: bool = True):
        check(self.L.ll_reg_set_profiling(self.h, int(enable)), "ll_reg_set_profiling")

    def set_information(self, enable: bool = True):
        """ll_reg_set_information: from the next enqueue on, every registration also leaves the Gauss-Newton matrix of its last
        linearisation per scan (information()); off by default, and nothing is launched, allocated or copied while it is off"""
        check(self.L.ll_reg_set_information(self.h, int(bool(enable))), "ll_reg_set_information")

    def information(self, n_scans: int = 1) -> list:
        """The records of the last collected enqueue (made with set_information on), one dict per scan: H [6, 6] = sum rho' J^T J, g [6]
        and cost of the scan's last linearisation in the solver's tangent [d_rot(3); d_t(3)] (R_inc+ = Exp(2 d_rot) R_inc), n_line /
        n_plane blocks summed, status (0 computed, 1 gated / no iteration / empty scan, 2 aborted solve: H zero), and the
        eigenvalues (ascending) and eigenvectors (columns) of H.  No device work: ll_reg_collect brought the records back."""
        recs = (capi.RegInformation * n_scans)()
        check(self.L.ll_reg_information(self.h, int(n_scans), recs), "ll_reg_information")
        out = []
        for r in recs:
            H = np.array(r.H, np.float64).reshape(6, 6)
            w, v = np.linalg.eigh(H)
            out.append({"H": H, "g": np.array(r.g, np.float64), "cost": float(r.cost), "n_line": int(r.n_line), "n_plane": int(r.n_plane),
                        "status": int(r.status), "eigenvalues": w, "eigenvectors": v})
        return out

    def information_time(self) -> float:
        """with set_profiling: milliseconds of the information kernel in the last collected enqueue (0.0 when it did not run)"""
        ms = C.c_float(0.0)
        check(self.L.ll_reg_information_time(self.h, C.byref(ms)), "ll_reg_information_time")
        return float(ms.value)

    def debug_worklists(self, n_scans=1):
        out = self._tap("ll_reg_debug_worklists", int(n_scans))
        return int(out[0] + out[2]), int(out[1] + out[3])

    def debug_worklists_by_kind(self, n_scans=1):
        """((corner searched, corner re-sorted), (surface searched, surface re-sorted)) of the last ICP iteration"""
        out = self._tap("ll_reg_debug_worklists", int(n_scans))
        return (int(out[0]), int(out[1])), (int(out[2]), int(out[3]))

    def debug_cycles(self, scan: int = 0):
        return self._tap("ll_reg_debug_cycles", scan, n=16)

    def kernel_times(self):
        ms = np.zeros(3, np.float32)
        n = np.zeros(3, np.int32)
        check(self.L.ll_reg_kernel_times(self.h, ptr(ms), ptr(n)), "ll_reg_kernel_times")
        return ms, n

    def append_to_submap_device(self, fe: "Livox_laser", n_scans: int, kind: int, accept: np.ndarray, poses: np.ndarray, out, n_used: int) -> int:
        """pointcloudAssociateToMap over an extractor's resident batch, device to device: the selected `kind` features
        of every accepted scan, moved to the map frame with its pose, are appended to the torch DEVICE tensor `out`
        ((capacity, 4) float32, contiguous) from row n_used on.  Returns the new row count."""
        acc = np.ascontiguousarray(accept, np.int32)
        ps = _poses(poses, -1)
        assert out.is_contiguous() and out.shape[1] == 4 and acc.shape[0] >= n_scans and ps.shape[0] >= n_scans
        n = C.c_int64(int(n_used))
        check(self.L.ll_cloud_transform_fe_device(self.h, fe.h, int(n_scans), int(kind), ptr(acc), ptr(ps), C.c_void_p(out.data_ptr()),
                                                  int(out.shape[0]), C.byref(n)), "ll_cloud_transform_fe_device")
        return int(n.value)

    def append_to_submap_device_spin(self, spin: "Spinning_laser", n_scans: int, which: int, accept: np.ndarray, poses: np.ndarray, out,
                                     n_used: int) -> int:
        """append_to_submap_device for a spinning-lidar handle: cloud `which` (Spinning_laser.FULL .. LESS_FLAT) of every accepted scan"""
        acc = np.ascontiguousarray(accept, np.int32)
        ps = _poses(poses, -1)
        assert out.is_contiguous() and out.shape[1] == 4 and acc.shape[0] >= n_scans and ps.shape[0] >= n_scans
        n = C.c_int64(int(n_used))
        check(self.L.ll_cloud_transform_spin_device(self.h, spin.h, int(n_scans), int(which), ptr(acc), ptr(ps), C.c_void_p(out.data_ptr()),
                                                    int(out.shape[0]), C.byref(n)), "ll_cloud_transform_spin_device")
        return int(n.value)

    def interpolation(self, n_scans: int = 1) -> dict:
        """ll_reg_interpolation: what compute_interpolatation_rodrigue (PCR:607-620) left in the slots of the last collected registration:
        dict(theta [n], omega_hat [n, 3, 3], pose_last [n, 7], pose_incre [n, 7]).  A gated slot: theta 0, zero matrix, identity increment."""
        n = int(n_scans)
        th, hat, pl, pi = np.zeros(n), np.zeros((n, 3, 3)), np.zeros((n, 7)), np.zeros((n, 7))
        check(self.L.ll_reg_interpolation(self.h, n, ptr(th), ptr(hat), ptr(pl), ptr(pi)), "ll_reg_interpolation")
        return {"theta": th, "omega_hat": hat, "pose_last": pl, "pose_incre": pi}

    def cloud_undistort_fe_device(self, fe: "Livox_laser", n_scans: int, kind: int, accept: np.ndarray, out, n_used: int) -> int:
        """append_to_submap_device with if_undistore = 1: the `kind` selection (0 corner, 1 surface, 2 full) of every accepted slot moves with
        that slot's state of the last collected registration (no poses argument).  Returns the new row count."""
        acc = np.ascontiguousarray(accept, np.int32)
        assert out.is_contiguous() and out.shape[1] == 4 and acc.shape[0] >= n_scans
        n = C.c_int64(int(n_used))
        check(self.L.ll_cloud_undistort_fe_device(self.h, fe.h, int(n_scans), int(kind), ptr(acc), C.c_void_p(out.data_ptr()), int(out.shape[0]),
                                                  C.byref(n)), "ll_cloud_undistort_fe_device")
        return int(n.value)

    def pointcloudAssociateToMap(self, pc_in: np.ndarray, pose: np.ndarray | None = None, if_undistore: int = 0, slot: int = 0) -> np.ndarray:
        """PCR:673-685.  if_undistore = 1: every point with the pose interpolated at its time stamp, from slot `slot` of the last collected
        registration (`pose` is not used)."""
        pc_in = capi.as_f32(pc_in, 4)
        out = np.empty_like(pc_in)
        if if_undistore:
            check(self.L.ll_cloud_undistort(self.h, int(slot), ptr(pc_in), ptr(out), pc_in.shape[0]), "ll_cloud_undistort")
            return out
        p = np.ascontiguousarray(self.m_pose_w_curr if pose is None else pose, np.float64)
        check(self.L.ll_cloud_transform(self.h, ptr(pc_in), ptr(out), pc_in.shape[0], ptr(p)), "ll_cloud_transform")
        return out


def information_in_pose_frame(H, pose_last) -> np.ndarray:
    """Point_cloud_registration.information()'s H, given in the solver's tangent d = [d_rot; d_t] of the increment, as the information of
    the scan's POSE in the map frame, ordered translation then rotation vector (radians): the order of the pose graph's residual.
    With R = R(pose_last), a step d moves the pose by xi = [dt_map; theta_map] = T d, T = [[0, R], [2 R, 0]] (R_curr+ = Exp(2 R d_rot) R_curr,
    t_curr+ = t_curr + R d_t), hence H_pose = T^-T H T^-1 with T^-1 = [[0, R^T / 2], [R^T, 0]].  36 numbers: host arithmetic."""
    H = np.asarray(H, np.float64).reshape(6, 6)
    x, y, z, w = (float(v) for v in np.asarray(pose_last, np.float64).reshape(7)[:4])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    Ti = np.zeros((6, 6))
    Ti[0:3, 3:6] = 0.5 * R.T
    Ti[3:6, 0:3] = R.T
    return Ti.T @ H @ Ti
