"""The key frames' accumulated clouds (Keyframe_assembly( map_refinement=True )), without a device: a stub full map and a stub refine
handle that records add_cloud.  Which scans' full clouds land in which key frame is held to the reference's own text
(laser_mapping.hpp:1443-1487 and :1524-1562, extracted at test time and compiled in a harness of its own; skipped where the reference is
absent) and to a plain restatement kept here; refine_map's id order and poses are checked with a stub solver; the ValueError paths."""
import os
import subprocess

import numpy as np
import pytest

from loam_livox_amd.keyframes import Keyframe_assembly
from tests.verbatim_build import REF

REF_HPP = os.path.join(REF, "source", "laser_mapping.hpp")
N_SCANS, EACH, BETWEEN, HISTORY = 350, 30, 10, 7


def added_pattern():
    """which scans the history's add rule lets in: seeded, with runs of rejections longer than the FIFO and of acceptances longer than it"""
    rng = np.random.default_rng(8)
    added = rng.random(N_SCANS) < 0.7
    added[40:55] = False
    added[100:125] = True
    added[200:212] = False
    return added


class StubFullMap:
    def append_cloud_touched(self, cloud, min_points=3):
        return np.array([[int(cloud[0, 3]) % 5, 0, 0]], np.int32)           # (a cell or two per key frame: the bookkeeping alone)

    def close(self):
        pass


class StubCellMap:
    def keyframe_images(self):
        return dict(images=np.zeros((4, 60, 60), np.float32), ratio_nonzero=np.zeros(4, np.float32), roi_range=1.0)

    def close(self):
        pass


class StubRefine:
    """stands in for api.Map_refine: records the clouds as they are added; refine hands back the stored clouds and records the call"""

    def __init__(self):
        self.clouds, self.leaves, self.calls, self.closed = [], [], [], False

    def add_cloud(self, cloud, leaf=0.5):
        self.clouds.append(np.array(cloud, np.float32).reshape(-1, 4))
        self.leaves.append(leaf)
        return len(self.clouds) - 1, len(cloud), 0

    def refine(self, ids, poses_ori, poses_opm, leaf=0.2, transform_first=False):
        self.calls.append(dict(ids=list(ids), ori=np.array(poses_ori), opm=np.array(poses_opm), leaf=leaf, transform_first=transform_first))
        return [self.clouds[i] for i in ids]

    def merge(self, leaf=0.2):
        self.calls.append(dict(merge=leaf))
        return np.concatenate([self.clouds[i] for i in self.calls[-2]["ids"]])

    def close(self):
        self.closed = True


class StubSolver:
    def solve(self, graphs):
        out = []
        for g in graphs:
            p = g["poses"].copy()
            p[:, 4:] += 0.25 * np.arange(len(p))[:, None]                  # a "corrected" pose per key frame, different for each
            out.append(p)
        return out, [dict(iterations=1, termination=3) for _ in graphs]

    def close(self):
        pass


def scan_cloud(k):
    """the full cloud of scan k: two points that carry k in their intensity"""
    return np.array([[k, 0, 0, k], [k, 1, 0, k]], np.float32)


def drive(**kw):
    """350 scans through an assembly over the stubs -> (assembly, refine stub); every closed key frame is processed at once"""
    refine = StubRefine()
    ka = Keyframe_assembly(full_cell_map=StubFullMap(), scans_of_each_keyframe=EACH, scans_between_two_keyframe=BETWEEN,
                           maximum_history_size=HISTORY, minimum_keyframe_differen=10 ** 6, pose_graph=StubSolver(), map_refinement=refine, **kw)
    ka.materialize = lambda kf: StubCellMap()
    added = added_pattern()
    for k in range(N_SCANS):
        pose = np.array([0, 0, 0, 1, k, 0.5 * k, 0], np.float64)
        ka.add_scan(scan_cloud(k), pose, k + 1, history_added=bool(added[k]))
        ka.process_waiting()
    return ka, refine


def restated():
    """the scan indices of every processed key frame's accumulated cloud, in order: the rule, stated plainly"""
    added = added_pattern()
    fifo, open_kfs, done = [], [dict(frames=0, acc=[])], []
    for k in range(N_SCANS):
        if added[k]:
            fifo.append(k)
        if len(fifo) > HISTORY:
            fifo.pop(0)
        for kf in open_kfs:
            kf["frames"] += 1
        if open_kfs[0]["frames"] >= EACH:
            done.append(open_kfs.pop(0))
        if open_kfs[-1]["frames"] >= BETWEEN:
            open_kfs[-1]["acc"] += fifo
            fifo = []
            open_kfs.append(dict(frames=0, acc=[]))
    return [kf["acc"] for kf in done]


REF_HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <list>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <vector>
using namespace std;
static std::ostringstream screen_out;
static void screen_printf( const char *, ... ) {}
struct PointType {};
struct Cloud {                                  // a point cloud is the list of the scans whose points it holds
    std::vector< int > scans;
    std::shared_ptr< Cloud > makeShared() const { return std::make_shared< Cloud >( *this ); }
    Cloud &operator+=( const Cloud &o ) { scans.insert( scans.end(), o.scans.begin(), o.scans.end() ); return *this; }
    void clear() { scans.clear(); }
};
namespace PCL_TOOLS { template < class T, class P > int pcl_pts_to_eigen_pts( std::shared_ptr< Cloud > ) { return 0; } }
template < typename T > struct Points_cloud_map {
    typedef int Mapping_cell_ptr;
    void append_cloud( int, std::set< Mapping_cell_ptr > *cells ) { cells->insert( 1 ); }
    int get_cells_size() { return 0; }
};
template < typename T > struct Maps_keyframe {
    size_t m_accumulate_frames = 0;
    int m_ending_frame_idx = 0;
    int m_pose_q = 0, m_pose_t = 0;
    Cloud m_accumulated_point_cloud;
    void add_cells( const std::set< int > & ) { m_accumulate_frames++; }
};
struct Reg { float m_inlier_threshold = 0; };
int main( int argc, char **argv )
{
    const int n_scans = atoi( argv[ 1 ] ), m_para_scans_of_each_keyframe = atoi( argv[ 2 ] ), m_para_scans_between_two_keyframe = atoi( argv[ 3 ] ),
              m_maximum_history_size = atoi( argv[ 4 ] );
    const char *pattern = argv[ 5 ];
    struct { void lock() {} } m_mutex_mapping;   // ( locked at :1444, released behind the excerpt )
    std::mutex m_mutex_dump_full_history, m_mutex_keyframe;
    std::list< Cloud > m_laser_cloud_corner_history, m_laser_cloud_surface_history, m_laser_cloud_full_history;
    std::list< float > m_his_reg_error;
    std::list< std::shared_ptr< Maps_keyframe< float > > > m_keyframe_of_updating_list, m_keyframe_need_precession_list;
    m_keyframe_of_updating_list.push_back( std::make_shared< Maps_keyframe< float > >() );   // :626
    Points_cloud_map< float > m_pt_cell_map_full, m_pt_cell_map_corners, m_pt_cell_map_planes;
    size_t m_loop_closure_maximum_keyframe_in_wating_list = 3;
    int m_loop_closure_if_enable = 1, m_current_frame_index = 0, m_q_w_curr = 0, m_t_w_curr = 0, m_last_his_add_q = 0, m_last_his_add_t = 0;
    Reg pc_reg;
    const float history_add_t_step = 1.f, history_add_angle_step = 1.f;
    // the corner history is full from the start, so the add rule is the pattern's alone (the first clause of :1446 never holds)
    for ( int i = 0; i < m_maximum_history_size; i++ ) m_laser_cloud_corner_history.push_back( Cloud() );
    for ( int k = 0; k < n_scans; k++ )
    {
        m_current_frame_index = k + 1;
        Cloud current_laser_cloud_full, corners, surface;
        current_laser_cloud_full.scans.push_back( k );
        Cloud *pc_new_feature_corners = &corners, *pc_new_feature_surface = &surface;
        const float t_diff = pattern[ k ] == '1' ? 2.f : 0.f, r_diff = 0.f;
        {
%s
        }
        {
%s
                }   // ( :1563 )
            }       // ( if ( m_loop_closure_if_enable ) )
        }
        while ( !m_keyframe_need_precession_list.empty() )   // the detector takes every waiting key frame at once
        {
            printf( "K" );
            for ( int s : m_keyframe_need_precession_list.front()->m_accumulated_point_cloud.scans ) printf( " %%d", s );
            printf( "\n" );
            m_keyframe_need_precession_list.pop_front();
        }
    }
    return 0;
}
"""


def test_accumulated_scans_equal_the_restatement_and_the_rule_is_exercised():
    ka, refine = drive()
    got = [sorted(set(int(v) for v in c[:, 3])) if len(c) else [] for c in refine.clouds]
    in_order = [[int(v) for v in c[::2, 3]] for c in refine.clouds]
    want = restated()
    assert in_order == want and got == [sorted(w) for w in want]
    assert len(want) == len(ka.keyframe_vec) == (N_SCANS - EACH) // BETWEEN + 1
    assert [kf.cloud_id for kf in ka.keyframe_vec] == list(range(len(want)))       # the index in keyframe_vec is the id
    assert all(kf.m_accumulated_point_cloud == [] for kf in ka.keyframe_vec)       # the host copies are dropped
    assert set(refine.leaves) == {0.5}
    sizes = [len(w) for w in want]
    added = added_pattern()
    # the FIFO is trimmed (a full 7 after ten accepted scans), runs dry (a key frame opened after ten rejections gets nothing), and a scan
    # lands in at most one key frame; a rejected scan in none
    assert max(sizes) == HISTORY and min(sizes) == 0 and 0 < sorted(sizes)[len(sizes) // 2] <= HISTORY
    flat = [s for w in want for s in w]
    assert len(flat) == len(set(flat)) and all(added[s] for s in flat) and len(flat) < added.sum()
    ka.close()
    assert not refine.closed                                                       # a handle handed in is not closed by the assembly


def test_accumulated_scans_equal_the_reference_text(tmp_path):
    if not os.path.exists(REF_HPP):
        pytest.skip("the reference is not on this machine")
    lines = open(REF_HPP).read().split("\n")
    first, second = lines[1443:1487], lines[1523:1562]                             # :1444-1487 (1443 is blank), :1524-1562
    assert "m_mutex_mapping.lock();" in first[0] and "m_his_reg_error.pop_front();" in first[-3]
    assert "if ( m_loop_closure_if_enable )" in second[0] and "Number of keyframes in update lists" in second[-1]
    src, exe = str(tmp_path / "accumulate_ref.cpp"), str(tmp_path / "accumulate_ref")
    with open(src, "w") as f:
        f.write(REF_HARNESS % ("\n".join(first), "\n".join(second)))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, src])
    pattern = "".join("1" if a else "0" for a in added_pattern())
    out = subprocess.run([exe, str(N_SCANS), str(EACH), str(BETWEEN), str(HISTORY), pattern], stdout=subprocess.PIPE, check=True, timeout=60).stdout.decode()
    ref = [[int(v) for v in line.split()[1:]] for line in out.strip().split("\n")]
    _, refine = drive()
    assert [[int(v) for v in c[::2, 3]] for c in refine.clouds] == ref == restated()


def test_refine_map_runs_every_second_key_frame_newest_first():
    ka, refine = drive()
    K = len(ka.keyframe_vec)
    loop = dict(his=2, last=K - 1, inlier_threshold=0.1, icp_q=np.array([0, 0, 0, 1.0]), icp_t=np.zeros(3))
    before = (ka.state(), list(ka.log), list(ka.loops), ka.if_end)
    ka.close_loop(loop)
    want_ids = list(range(K - 1, -1, -2))
    call = refine.calls[-1]
    assert call["ids"] == want_ids and call["leaf"] == 0.2 and call["transform_first"] is False
    assert np.array_equal(call["ori"], ka.poses_ori[want_ids]) and np.array_equal(call["opm"], ka.poses_opm[want_ids])
    assert not np.array_equal(ka.poses_ori, ka.poses_opm)
    assert [i for i, _ in ka.refined] == want_ids and all(c is refine.clouds[i] for i, c in ka.refined)
    assert (ka.state(), ka.log, ka.loops, ka.if_end) == before
    merged = ka.refined_mapping()
    assert refine.calls[-2]["ids"] == list(range(K)) and refine.calls[-2]["transform_first"] is True and refine.calls[-1] == dict(merge=0.2)
    assert len(merged) == sum(len(c) for c in refine.clouds)
    # take_solution, the route of an owner that solves for many assemblies, refines as well
    ka.refined = None
    ka.take_solution(ka.loop_graph(loop), ka.poses_opm, dict(iterations=0))
    assert [i for i, _ in ka.refined] == want_ids


def test_value_errors():
    with pytest.raises(ValueError, match="needs pose_graph"):
        Keyframe_assembly(full_cell_map=StubFullMap(), map_refinement=True)
    with pytest.raises(ValueError, match="needs pose_graph"):
        Keyframe_assembly(full_cell_map=StubFullMap(), map_refinement=StubRefine(), pose_graph=False)
    ka = Keyframe_assembly(full_cell_map=StubFullMap(), pose_graph=StubSolver(), map_refinement=StubRefine())
    with pytest.raises(ValueError, match="a closed loop"):
        ka.refine_map()
    with pytest.raises(ValueError, match="a closed loop"):
        ka.refined_mapping()
    off = Keyframe_assembly(full_cell_map=StubFullMap(), pose_graph=StubSolver())
    with pytest.raises(ValueError, match="map_refinement=True"):
        off.refine_map()
    assert off.map_refinement is False and off.refined is None and len(off.m_laser_cloud_full_history) == 0
    off.add_scan(scan_cloud(0), np.array([0, 0, 0, 1, 0, 0, 0.0]), 1, history_added=True)
    assert len(off.m_laser_cloud_full_history) == 0                                # off: the FIFO is not kept
    from loam_livox_amd.mapping import Laser_mapping_batch
    with pytest.raises(ValueError, match="map_refinement is not available in the batched loop"):
        Laser_mapping_batch(2, loop_closure=dict(pose_graph=True, map_refinement=True))
