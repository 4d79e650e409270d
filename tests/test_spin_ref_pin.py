"""CPU tier, where the reference sources are present: pins the host restatement tests/spin_ref.c to the reference's own text.

The spinning-lidar branch of Laser_feature::laserCloudHandler (source/laser_feature_extractor.hpp:393-811, through the five
publishes) and removeClosedPointCloud (:211-240) are extracted by line range, wrapped in a harness that supplies what the excerpt
reads (the member arrays, publishers that capture, removeNaNFromPointCloud, ROS_BREAK) and compiled against oracle/ref_stubs
into a temporary directory: nothing compiled from the reference lands in the tree.  The harness's own compilation decides which
atan / atan2 / sqrt overloads the text resolves to.  On scans inside the defined domain (nothing filtered) the five published
clouds must be bit-identical to the restatement's, intensities included (both sides call the host libm)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from loam_livox_amd import synth
from tests import spin_inputs, spin_ref, verbatim_build

REF = verbatim_build.REF
ROOT = verbatim_build.ROOT
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "source", "laser_feature_extractor.hpp")),
                                reason="needs the reference sources")

HARNESS = r'''
namespace pcl
{
template <class C> void removeNaNFromPointCloud( const C &in, C &out, std::vector<int> &index )
{
    C tmp;  // the node passes the same cloud in and out
    index.clear();
    for ( size_t i = 0; i < in.points.size(); i++ )
        if ( std::isfinite( in.points[ i ].x ) && std::isfinite( in.points[ i ].y ) && std::isfinite( in.points[ i ].z ) )
        {
            tmp.points.push_back( in.points[ i ] );
            index.push_back( ( int ) i );
        }
    out.points = tmp.points;
}
} // namespace pcl
#define ROS_BREAK() abort()

class Spin_harness
{
  public:
    const double m_para_scanPeriod = 0.1;   // laser_feature_extractor.hpp:68
    float       m_pc_curvature[ 400000 ];   // :75-78
    int         m_pc_sort_idx[ 400000 ];
    int         m_pc_neighbor_picked[ 400000 ];
    int         m_pc_cloud_label[ 400000 ];
    bool        m_if_pub_each_line = false; // :88
    int         m_lidar_type = 0;           // :89
    int         m_laser_scan_number = 16;
    double      m_minimum_range = 0.1;
    float       m_plane_resolution = 0.8f;
    Livox_laser m_livox;
    Voxel_t     m_voxel_filter_for_surface;
    Capture_pub m_pub_laser_pc, m_pub_pc_sharp_corner, m_pub_pc_less_sharp_corner, m_pub_pc_surface_flat, m_pub_pc_surface_less_flat;
    std::vector<Capture_pub> m_pub_each_scan;
    std::vector<pcl::PointCloud<PointType>> out;

// ---- verbatim: laser_feature_extractor.hpp:211-240
@CLOSED@
// ---- end of excerpt

    void handler( const sensor_msgs::PointCloud2ConstPtr &laserCloudMsg )
    {
        std::vector<pcl::PointCloud<PointType>> laserCloudScans( m_laser_scan_number );   // :257
        std::vector<int> scanStartInd( 1000, 0 );                                         // :270-271
        std::vector<int> scanEndInd( 1000, 0 );
        pcl::PointCloud<pcl::PointXYZI> laserCloudIn;                                     // :273-274
        pcl::fromROSMsg( *laserCloudMsg, laserCloudIn );
        size_t cloudSize = laserCloudIn.points.size();                                    // :280
        if ( m_lidar_type )
        {
            return;
        }
// ---- verbatim: laser_feature_extractor.hpp:393-811
@HANDLER@
// ---- end of excerpt
    }
};

// argv: msgs.bin out.bin scan_line minimum_range plane_resolution
// msgs.bin: int32 n_msgs, then per message int32 n_points and the xyzi cloud; out.bin: per message five clouds as int32 n + n x xyzi
int main( int argc, char **argv )
{
    if ( argc < 6 ) return 2;
    FILE *f = fopen( argv[ 1 ], "rb" ), *o = fopen( argv[ 2 ], "wb" );
    if ( !f || !o ) return 3;
    Spin_harness *node = new Spin_harness();
    node->m_laser_scan_number = atoi( argv[ 3 ] );
    node->m_minimum_range = atof( argv[ 4 ] );
    node->m_plane_resolution = ( float ) atof( argv[ 5 ] );
    node->m_voxel_filter_for_surface.setLeafSize( node->m_plane_resolution / 2, node->m_plane_resolution / 2, node->m_plane_resolution / 2 );  // :192
    Capture_pub *pubs[ 5 ] = { &node->m_pub_laser_pc, &node->m_pub_pc_sharp_corner, &node->m_pub_pc_less_sharp_corner, &node->m_pub_pc_surface_flat,
                               &node->m_pub_pc_surface_less_flat };
    for ( Capture_pub *p : pubs ) p->sink = &node->out;
    int n_msgs = 0;
    if ( fread( &n_msgs, 4, 1, f ) != 1 ) return 4;
    for ( int m = 0; m < n_msgs; m++ )
    {
        int n = 0;
        if ( fread( &n, 4, 1, f ) != 1 ) return 4;
        auto msg = std::make_shared<sensor_msgs::PointCloud2>();
        msg->cloud.points.resize( n );
        for ( int i = 0; i < n; i++ )
        {
            float v[ 4 ];
            if ( fread( v, 4, 4, f ) != 4 ) return 4;
            msg->cloud.points[ i ].x = v[ 0 ];
            msg->cloud.points[ i ].y = v[ 1 ];
            msg->cloud.points[ i ].z = v[ 2 ];
            msg->cloud.points[ i ].intensity = v[ 3 ];
        }
        node->out.clear();
        node->handler( msg );
        if ( node->out.size() != 5 ) return 5;
        for ( auto &c : node->out )
        {
            int k = ( int ) c.points.size();
            fwrite( &k, 4, 1, o );
            for ( auto &p : c.points )
            {
                float v[ 4 ] = { p.x, p.y, p.z, p.intensity };
                fwrite( v, 4, 4, o );
            }
        }
    }
    fclose( o );
    return 0;
}
'''


@pytest.fixture(scope="module")
def pin_exe(tmp_path_factory):
    td = tmp_path_factory.mktemp("spin_pin")
    # the stand-in PointCloud of oracle/ref_stubs carries no header: the one header copy of removeClosedPointCloud (on a branch the node
    # never takes, it filters a cloud into itself) is the only text changed
    closed = verbatim_build._lines("source/laser_feature_extractor.hpp", 211, 240)
    assert closed.count("cloud_out.header = cloud_in.header;") == 1
    closed = closed.replace("cloud_out.header = cloud_in.header;", ";")
    tu = verbatim_build.FEAT_HEAD + HARNESS.replace("@CLOSED@", closed) \
        .replace("@HANDLER@", verbatim_build._lines("source/laser_feature_extractor.hpp", 393, 811))
    src = td / "spin_pin.cpp"
    src.write_text(tu)
    exe = td / "spin_pin"
    stubs = os.path.join(ROOT, "oracle", "ref_stubs")
    inc = ["-I", os.path.join(stubs, "override"), "-I-", "-I", stubs, "-I", os.path.join(REF, "source"), "-I", os.path.join(REF, "include"),
           "-I", os.path.join(REF, "include", "tools")]
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-fno-fast-math", "-w"] + inc + [str(src), "-o", str(exe), "-lpthread"])
    return exe


def run_pin(exe, tmp_path, clouds, scan_line, minimum_range=0.1, plane_resolution=0.8):
    msgs, outp = tmp_path / f"msgs{scan_line}.bin", tmp_path / f"out{scan_line}.bin"
    with open(msgs, "wb") as f:
        f.write(struct.pack("i", len(clouds)))
        for c in clouds:
            c = np.ascontiguousarray(c, np.float32)
            f.write(struct.pack("i", len(c)))
            f.write(c.tobytes())
    subprocess.check_call([str(exe), str(msgs), str(outp), str(scan_line), repr(minimum_range), repr(plane_resolution)], timeout=600)
    data = outp.read_bytes()
    res, o = [], 0
    for _ in clouds:
        five = []
        for _ in range(5):
            (n,) = struct.unpack_from("i", data, o)
            o += 4
            five.append(np.frombuffer(data, np.float32, 4 * n, o).reshape(n, 4))
            o += 16 * n
        res.append(five)
    return res


def pin_scans(scan_line):
    """>= 8 in-domain scans (no NaN, nothing inside minimum_range): full revolutions (the halfPassed flip), noise-free ones (exact
    curvature ties), rooms with pillars (occlusions), coarse and fine azimuth steps (walks across sub-regions and lines), short and
    empty lines (a scan of a few azimuths: lines of fewer than 12 points have empty sub-regions); for 16 lines also the families of
    tests/spin_inputs.py: crowded sub-regions (the 20 / 200 pick bounds, sub-regions of more than 4096 points, runs of tied curvatures),
    walks of 500 steps, to the ends of the cloud and across a line boundary"""
    w = synth.make_world(4, 4)
    out = []
    for k, (n_az, sigma) in enumerate([(1800, 0.01), (1800, 0.0), (900, 0.02), (600, 0.0), (1200, 0.01), (300, 0.01), (8, 0.0), (20, 0.01)]):
        out.append(synth.make_spin_scan(w, 40 + k, scan_line=scan_line, n_azimuth=n_az if scan_line == 16 else n_az * 2 // 3,
                                        range_sigma=sigma).xyzi)
    if scan_line == 16:
        out += [spin_inputs.family(name)[0] for name in sorted(spin_inputs.FAMILIES)]
    return out


@pytest.mark.parametrize("scan_line", [16, 64])
def test_restatement_is_the_reference(pin_exe, tmp_path, scan_line):
    clouds = pin_scans(scan_line)
    got = run_pin(pin_exe, tmp_path, clouds, scan_line)
    n_flip = n_dropped = n_short = n_capped = 0
    for c, five in zip(clouds, got):
        r = spin_ref.extract(c, scan_line=scan_line)
        n_capped += sum(w["less_sharp"] == 200 for w in spin_inputs.reach(r))
        assert len(r["full"]) + np.count_nonzero(~np.isin(np.arange(len(c)), r["full_src"])) == len(c)
        ref5 = spin_ref.clouds(r)
        for topic, mine in zip(spin_ref.TOPICS, five):
            assert mine.shape == ref5[topic].shape, topic
            assert np.array_equal(mine, ref5[topic]), topic  # bit-identical, intensities included
        n_dropped += len(c) - len(r["full"])
        n_short += int(np.count_nonzero((r["line_n"] > 0) & (r["line_n"] < 12)))
        rel = r["full"][:, 3] - np.floor(r["full"][:, 3])
        n_flip += int(rel.max() > 0.05) if len(rel) else 0
    assert n_flip >= 4          # orientations past startOri + pi: the halfPassed branch ran
    assert n_short >= 1
    assert n_capped >= (20 if scan_line == 16 else 0)  # sub-regions stopped at the 201st pick
    if scan_line == 64:
        assert n_dropped > 0    # beams outside the 0..50 scan-ID rule
