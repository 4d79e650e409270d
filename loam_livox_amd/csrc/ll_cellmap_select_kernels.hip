// ll_cellmap_select_kernels.hip -- a cell map's line cloud and plane cloud on the device: the points of the cells that
// determine_feature labels e_feature_line / e_feature_plane, as Maps_keyframe::extract_specify_points hands them to the scene alignment
// (source/cell_map_keyframe.hpp:1263-1281, source/scene_alignment.hpp:283-290).
//
// The map is ordered by (cell key, insertion order) and both clouds come out in that order -- cells ascending, every cell's points as
// stored, every point {x, y, z, 0} -- so nothing is sorted:
//   flag     one thread per cell table entry (and one behind the table): the cell's points, counted in the low half of a 64-bit word
//            for a line cell and in the high half for a plane cell (ll_cellmap_select_core.h select_word);
//   scan     ONE exclusive sum of those words over n_cells + 1 entries: the low half of entry c is the first position of cell c in the
//            line cloud, the high half its first position in the plane cloud, and entry n_cells holds {plane points, line points};
//   gather   one lane per STORED point, one pass over the point store for both kinds.  Cell sizes are badly skewed (thousands of points
//            in a wall cell, one in a stray cell), so the work is divided by point, not by cell: a lane finds its cell in the table's
//            offsets (select_cell_of), reads the cell's label and 16 bytes of point, and a lane of a line or plane cell writes them to
//            its cloud; consecutive lanes read consecutive addresses and, inside a cell run, write consecutive addresses.  The first
//            lane also leaves the two totals as ints where a voxel filter reads its input count.
// No kernel waits for another thread: the test-only host build drives the same launches (tests/cellmap_feature_clouds_host.cpp).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include "ll_cellmap.h"
#include "ll_cellmap_select_core.h"

namespace ll {

typedef unsigned long long u64;
typedef unsigned int u32;

#define CSCHK(x)                              \
    do {                                      \
        hipError_t e_ = (x);                  \
        if (e_ != hipSuccess) {               \
            *err = hipGetErrorString(e_);     \
            return -1;                        \
        }                                     \
    } while (0)

static inline unsigned int cs_blocks(int n) { return (unsigned int)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1); }

__global__ __launch_bounds__(256) void cs_flag_kernel(const CellStats *stats, const int *cstart, int n_cells, u64 *word)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c > n_cells) return;
    word[c] = c < n_cells ? select_word(stats[c].type, cstart[c + 1] - cstart[c]) : 0ull;
}

// pos[0 .. n_cells]: the scanned words.  n_pts threads (at least one: the totals are written for an empty map too).
__global__ __launch_bounds__(256) void cs_gather_kernel(const float4 *pts, const int *cstart, const CellStats *stats, const u64 *pos, int n_cells,
                                                        int n_pts, float4 *line, float4 *plane, int *n_line, int *n_plane)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        const u64 totals = pos[n_cells];
        *n_line = (int)(u32)totals;
        *n_plane = (int)(totals >> 32);
    }
    if (i >= n_pts) return;
    const int c = select_cell_of(cstart, n_cells, i);
    const int type = stats[c].type;
    if (type != LL_FEATURE_LINE && type != LL_FEATURE_PLANE) return;
    const u64 p = pos[c];
    const float4 v = pts[i];
    const int within = i - cstart[c];
    if (type == LL_FEATURE_LINE)
        line[(int)(u32)p + within] = make_float4(v.x, v.y, v.z, 0.0f);
    else
        plane[(int)(p >> 32) + within] = make_float4(v.x, v.y, v.z, 0.0f);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
// Temporary storage the scan over n_cells + 1 words asks for.  A map's scratch is sized for its sorts and its 32-bit scans, which on a
// map of a few points is less than a 64-bit scan wants: the caller raises m.tmp to this before cellmap_select_features.
size_t cellmap_select_scratch(const CellMapDev &m)
{
    size_t need = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, need, m.skey, m.skey2, m.n_cells + 1) != hipSuccess) return 0;
    return need;
}

// d_stats: cellmap_stats' result for m as it is now.  d_line / d_plane: room for m.n_pts points each (the two clouds together hold at
// most m.n_pts).  d_n_line / d_n_plane: one int each, on the device.  Uses the map's scratch between queries -- skey (words), skey2
// (scanned), tmp -- and leaves the cells, the points and the result of the last query alone.  Three enqueues, no host wait.
int cellmap_select_features(CellMapDev &m, const CellStats *d_stats, float4 *d_line, float4 *d_plane, int *d_n_line, int *d_n_plane, hipStream_t s,
                            const char **err)
{
    const int nc = m.n_cells, np = nc > 0 ? m.n_pts : 0;
    hipLaunchKernelGGL(cs_flag_kernel, dim3(cs_blocks(nc + 1)), dim3(256), 0, s, d_stats, m.cstart, nc, m.skey);
    size_t need = 0;
    CSCHK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, m.skey, m.skey2, nc + 1));
    if (need > m.tmp_bytes) {
        *err = "cell map scratch too small for the scan";
        return -1;
    }
    size_t tb = m.tmp_bytes;
    CSCHK(hipcub::DeviceScan::ExclusiveSum(m.tmp, tb, m.skey, m.skey2, nc + 1, s));
    hipLaunchKernelGGL(cs_gather_kernel, dim3(cs_blocks(np)), dim3(256), 0, s, m.pts, m.cstart, d_stats, m.skey2, nc, np, d_line, d_plane, d_n_line,
                       d_n_plane);
    CSCHK(hipGetLastError());
    return 0;
}

}  // namespace ll
