// ll_reg_query_kernels.hip -- the registrar's per-query kernels (gfx950, wave64) and the host-side choice of search form:
// launch_reg_knn_build (one map for the batch) and launch_reg_knn_build_maps (a map per slot), declared in ll_device.h and called
// from ll_api_reg.hip once per ICP iteration.  Per query: transform with the current pose (pointAssociateToMap,
// point_cloud_registration.hpp:622-661), exact 5-NN on the cell grid (:249,351), match-radius tests (:254,353), line / plane block
// constants (:300-323, :416-423; ceres_icp.hpp:255-256, 328-334).  The per-query device code itself is ll_reg_query.h (shared with
// the tile search, ll_knn_kernels.hip); the solvers that consume the blocks are ll_reg_solve_kernels.hip and its neighbours.
//
// Corner and surface queries share every launch (blockIdx.z = kind).
//
//   ICP iterations 0 and 1 (and every iteration when neighbour reuse is disabled):
//       reg_transform_kernel -> reg_knn_kernel (all queries) -> reg_build_kernel (all queries)
//   ICP iteration >= 2:
//       reg_requery_kernel    : transform + displacement test of every query against its reuse record (ll_knn_core.h):
//                                 stable  -> nothing to do: same neighbours, same order, same residual block;
//                                 re-sort -> the same five neighbours re-evaluated at the new position, slot appended
//                                            to the chunk's re-sort list;
//                                 search  -> slot appended to the chunk's search list
//       reg_list_kernel       : full exact search of the search list + block constants of everything searched or re-sorted
// The two work lists are dense per scan and kind: every re-query workgroup reserves its share of the scan-and-kind's
// segment with one atomicAdd per list (work_cnt; ~94 workgroups per counter -- a single batch-wide counter cost 280 us
// of contention per launch), and the list kernel walks all segments as one dense index space (prefix sums of the 2 B
// counters in LDS, binary search per entry): a small grid of full wavefronts.  Round 1 kept one list segment per
// 256-query chunk and launched one workgroup per chunk: in the late iterations a chunk holds ~3 searches, the launch was
// 48 k workgroups with three busy lanes each, and its ~110 us floor (186 us average) was the cost of scheduling them.
// The order of the entries depends on the order of the atomics; every entry is processed independently, so results do not.
#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "ll_reg_query.h"

namespace ll {

#define RQ_THREADS 256  // queries per requery workgroup = work-list segment size
#define RQ_WAVES (RQ_THREADS / 64)

// K6t: pose transform of every query (pointAssociateToMap, fp64 math -> fp32 store like the reference).  A
// kernel of its own so that the double-precision sin/cos of the motion-deblur branch does not set the register
// footprint of the k-NN kernel.
__global__ __launch_bounds__(KB_THREADS) void reg_transform_kernel(RegDev rd, RegConst rc, int skip_kinds)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    if ((skip_kinds >> kind) & 1) return;  // (the tile kernel transforms its own queries)
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    const int q = blockIdx.x * KB_THREADS + threadIdx.x;
    if (q >= n) return;
    const int slot = (kind ? rd.cap_c : 0) + q;
    float pw[3];
    transform_query(st, rc, load_feature(rd, b, kind, q), pw);
    // a13: a skipped feature is handed on as a non-finite query -- no neighbours, no block (PCR:232-238, 339-345)
    if (subsample_skip_feature(rc.subsample_seed, kind, st->icp_iters, q, n, rc.max_blocks)) pw[0] = pw[1] = pw[2] = NAN;
    rd.qw[(size_t)b * rd.cap + slot] = make_float4(pw[0], pw[1], pw[2], 0.f);
}

// K6a: one lane per query: exact 5-NN of the transformed point (fp32 only -> small register footprint, so
// occupancy hides the gather latency).  Output per query: positions (cell-sorted order) of the neighbours the
// block needs + "5 found" flag, and the reuse record for the next ICP iteration.
#ifndef KNN_WAVES_PER_EU
#define KNN_WAVES_PER_EU 4
#endif
__global__ __launch_bounds__(KB_THREADS) __attribute__((amdgpu_waves_per_eu(KNN_WAVES_PER_EU, 8)))
void reg_knn_kernel(RegDev rd, RegConst rc, Grid gc, Grid gs, int iter, int skip_kinds)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    if ((skip_kinds >> kind) & 1) return;  // reg_knn_coop_kernel has them
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    const int q = blockIdx.x * KB_THREADS + threadIdx.x;
    if (q >= n) return;
    knn_one(rd, rc, gc, gs, b, (kind ? rd.cap_c : 0) + q, iter);
}

// K6a for small batches: one query per wavefront -- the corner queries (a few hundred per scan, a quarter of them searching
// rings of the sparse corner map: per lane the longest dependent chain of the launch, header of ll_knn_coop.h), and the
// surface queries too when a scan has few of them (voxel-filtered clouds against a sparse local map: the sequential mapping
// loop, where every search walks rings).  kinds: bit k set = kind k is searched here.
#define KC_THREADS 256
__global__ __launch_bounds__(KC_THREADS) void reg_knn_coop_kernel(RegDev rd, RegConst rc, Grid gc, Grid gs, int iter, int kinds)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    if (!((kinds >> kind) & 1)) return;
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int q = (int)((blockIdx.x * KC_THREADS + threadIdx.x) >> 6);
    if (q >= (kind ? rd.n_surf[b] : rd.n_corner[b])) return;  // (whole wavefronts)
    knn_one_coop(rd, rc, gc, gs, b, (kind ? rd.cap_c : 0) + q, iter);
}

// K6r: transform + reuse test (ICP iteration >= 1)

// One workgroup per chunk of RQ_PER x RQ_THREADS consecutive queries (round 3: four queries per thread -- their eight record loads
// are in flight together, and a workgroup pays its two barriers and two list reservations once per 1024 queries instead of once per
// 256; round 2: 73 us per B = 256 launch for 141 MB of records).  Unstable queries are appended to the dense per-(scan, kind) work
// lists: every thread with state 1 (re-sort) or 2 (search) gets a distinct position in its list; the workgroup reserves one
// contiguous range per list with one round of ballots per query slice, one barrier pair and two independent atomicAdds issued back
// to back.  (Within a list the entries of a workgroup are ordered by slice, then wavefront, then lane; nothing depends on the order.)
#define RQ_PER 4
__global__ __launch_bounds__(RQ_THREADS) void reg_requery_kernel(RegDev rd, RegConst rc, Grid gc, Grid gs, int iter)
{
    const int chunk = blockIdx.x, b = blockIdx.y, kind = blockIdx.z;
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    if (chunk * RQ_PER * RQ_THREADS >= n) return;
    const size_t sb = (size_t)b * rd.cap;
    const int koff = kind ? rd.cap_c : 0;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ int s_cnt[2][RQ_PER * RQ_WAVES];  // [list][slice * RQ_WAVES + wave]
    __shared__ int s_base[2];
    float4 ft[RQ_PER], rq[RQ_PER];
    int qq[RQ_PER];  // the query of this thread's u-th place (-1: beyond the scan's queries)
#pragma unroll
    for (int u = 0; u < RQ_PER; u++) {
        const int place = (chunk * RQ_PER + u) * RQ_THREADS + tid;
        qq[u] = place < n ? place : -1;
    }
#pragma unroll
    for (int u = 0; u < RQ_PER; u++) {
        const int qc = qq[u] >= 0 ? qq[u] : 0;
        ft[u] = load_feature(rd, b, kind, qc);
        rq[u] = rd.ref_q[sb + koff + qc];
    }
    int state[RQ_PER];  // 0 = stable or out of range, 1 = re-sorted, 2 = needs a search
    unsigned long long m1[RQ_PER], m2[RQ_PER];
#pragma unroll
    for (int u = 0; u < RQ_PER; u++) {
        const int q = qq[u];
        const int slot = koff + q;
        state[u] = 0;
        if (q >= 0) {
            float pw[3];
            transform_query(st, rc, ft[u], pw);
            KnnRef ref;
            ref.qx = rq[u].x;
            ref.qy = rq[u].y;
            ref.qz = rq[u].z;
            ref.m_strong = rq[u].w;
            const float delta = knn5_ref_delta(ref, pw[0], pw[1], pw[2]);  // NaN for a non-finite query -> search
            if (!(delta < ref.m_strong)) {  // else: same neighbours, same order: nn and the block are unchanged
                const float2 rs = rd.ref_s[sb + slot];
                ref.m_set = rs.y;
                // Both kinds of work are left to the list kernel: the five gathers and the stores of a re-sort in here kept
                // nearly every wavefront alive for three more dependent round trips (73 % of them hold at least one such lane)
                rd.qw[sb + slot] = make_float4(pw[0], pw[1], pw[2], 0.f);
                state[u] = (delta < ref.m_set) ? 1 : 2;
            }
        }
        m1[u] = __ballot(state[u] == 1);
        m2[u] = __ballot(state[u] == 2);
        if (lane == 0) {
            s_cnt[0][u * RQ_WAVES + wave] = __popcll(m1[u]);
            s_cnt[1][u * RQ_WAVES + wave] = __popcll(m2[u]);
        }
    }
    __syncthreads();
    int off1[RQ_PER], off2[RQ_PER], tot1 = 0, tot2 = 0;
#pragma unroll
    for (int u = 0; u < RQ_PER; u++) {
        off1[u] = off2[u] = 0;
        for (int w = 0; w < RQ_WAVES; w++) {
            const int c1 = s_cnt[0][u * RQ_WAVES + w], c2 = s_cnt[1][u * RQ_WAVES + w];
            if (w < wave) off1[u] += c1, off2[u] += c2;
            tot1 += c1, tot2 += c2;
        }
    }
    // (offsets of slice u: everything in the slices before it, then the earlier wavefronts of its own)
    int pre1 = 0, pre2 = 0;
#pragma unroll
    for (int u = 0; u < RQ_PER; u++) {
        int s1 = 0, s2 = 0;
        for (int w = 0; w < RQ_WAVES; w++) s1 += s_cnt[0][u * RQ_WAVES + w], s2 += s_cnt[1][u * RQ_WAVES + w];
        off1[u] += pre1;
        off2[u] += pre2;
        pre1 += s1;
        pre2 += s2;
    }
    int *cnt = rd.work_cnt + ((size_t)b * 2 + kind) * 2;  // [0] search, [1] re-sort
    if (tid == 0) {
        const int b1 = tot1 > 0 ? atomicAdd(cnt + 1, tot1) : 0;
        const int b2 = tot2 > 0 ? atomicAdd(cnt + 0, tot2) : 0;
        s_base[0] = b1;
        s_base[1] = b2;
    }
    __syncthreads();
    const size_t seg = sb + koff;  // the scan-and-kind's own segment of the work arrays
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int u = 0; u < RQ_PER; u++) {
        const int slot = koff + qq[u];
        if (state[u] == 1) rd.work_build[seg + s_base[0] + off1[u] + __popcll(m1[u] & below)] = (int)sb + slot;
        if (state[u] == 2) rd.work_search[seg + s_base[1] + off2[u] + __popcll(m2[u] & below)] = (int)sb + slot;
    }
}

__global__ __launch_bounds__(KB_THREADS) void reg_build_kernel(RegDev rd, RegConst rc, Grid gc, Grid gs, int skip_kinds)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    if ((skip_kinds >> kind) & 1) return;  // (the tile kernel builds the blocks of its own slots)
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    const int q = blockIdx.x * KB_THREADS + threadIdx.x;
    if (q >= n) return;
    build_one(rd, rc, gc, gs, b, (kind ? rd.cap_c : 0) + q);
}

// ICP iteration >= 2: exact search of the dense search list followed at once by the block constants of the same slot
// (the lane still holds the neighbours), then the block constants of the re-sorted slots.  Grid-stride over the lists.
#define RL_THREADS 128
#define RL_BLOCKS 2048  // x 128 threads; 4096 (every wavefront slot at 64 VGPRs) measured the same, the lists are bound by dependent misses
#define RL_MAX_SEG 2048  // scan-and-kind segments of one offsets table (max_scans <= 1024); larger batches run in slices
#define RL_LOCAL_SEG 64  // up to this many segments (32 scans) the list kernel builds the offsets itself
// exclusive prefix sums of the per-segment list lengths (segment = scan * 2 + kind) -> work_off[list][0 .. n_seg]; one workgroup
__global__ __launch_bounds__(1024) void reg_list_offsets_kernel(RegDev rd, int seg0, int n_seg)
{
    __shared__ int s_wave[3][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sg0 = 2 * tid, sg1 = 2 * tid + 1;  // two segments per thread (n_seg <= 2048): a scan's corner and surface segment
    for (int w = 0; w < 3; w++) {
        // (w = 2: the search list again with every surface segment -- odd: segment = scan * 2 + kind -- counted as empty)
        const int c0 = sg0 < n_seg ? rd.work_cnt[(size_t)(seg0 + sg0) * 2 + (w & 1)] : 0;
        const int c1 = (sg1 < n_seg && w < 2) ? rd.work_cnt[(size_t)(seg0 + sg1) * 2 + w] : 0;
        int incl = c0 + c1;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int y = __shfl_up(incl, off);
            if (lane >= off) incl += y;
        }
        if (lane == 63) s_wave[w][wave] = incl;
        __syncthreads();
        int base = 0;
        for (int k = 0; k < wave; k++) base += s_wave[w][k];
        const int excl = base + incl - (c0 + c1);
        int *off_w = rd.work_off + (size_t)w * (RL_MAX_SEG + 1);
        if (sg0 < n_seg) off_w[sg0] = excl;
        if (sg1 < n_seg) off_w[sg1] = excl + c0;
        if (tid == 1023) off_w[n_seg] = base + incl;  // its segments lie beyond n_seg or are the last ones: the grand total
        __syncthreads();
    }
}

// LOCAL: the offsets tables are built in LDS by every workgroup (small batches); a template constant so that the large-batch
// form keeps plain global loads in its binary searches
template <bool LOCAL>
__global__ __launch_bounds__(RL_THREADS) __attribute__((amdgpu_waves_per_eu(4, 8))) void reg_list_kernel(RegDev rd, RegConst rc, Grid gc, Grid gs, int iter, int seg0, int n_seg)
{
    // The offsets table (<= 16 KB) is searched where it lies: it stays in L1 / L2, and a copy in LDS would cap the
    // occupancy of this latency-bound kernel (16 KB per 128-thread workgroup: 36 -> 99 us per late iteration at B = 256).
    const int tid = threadIdx.x;
    const int stride = gridDim.x * RL_THREADS;
    // Corner searches first, one per WAVEFRONT while there are few of them (round 3): a late iteration searches a handful of
    // corner queries per scan, each a chain of 100+ dependent loads for a single lane -- the floor of this launch (~100 us at
    // B = 256 for ~1.5 k of them beside 75 k surface searches of ~15 round trips each; 49 us for a single scan).
    // With few searches altogether (a single scan, a small batch, voxel-filtered clouds) every search goes that way.
    // Small batches (<= RL_LOCAL_SEG segments) skip the offsets kernel: every workgroup sums the few counters itself
    // (one launch and one kernel boundary less per ICP iteration: ~6 us of a single scan's ~40 per iteration).
    __shared__ int s_cnt[2][LOCAL ? RL_LOCAL_SEG : 1];
    __shared__ int s_off[3][LOCAL ? RL_LOCAL_SEG + 1 : 1];
    if (LOCAL) {
        if (tid < n_seg) {
            s_cnt[0][tid] = rd.work_cnt[(size_t)(seg0 + tid) * 2 + 0];
            s_cnt[1][tid] = rd.work_cnt[(size_t)(seg0 + tid) * 2 + 1];
        }
        __syncthreads();
        if (tid < 3) {  // (as reg_list_offsets_kernel: searches, re-sorts, the searches of the corner segments alone)
            int acc = 0;
            for (int sg = 0; sg < n_seg; sg++) {
                s_off[tid][sg] = acc;
                acc += tid == 2 ? ((sg & 1) ? 0 : s_cnt[0][sg]) : s_cnt[tid][sg];
            }
            s_off[tid][n_seg] = acc;
        }
        __syncthreads();
    }
    const int *off_s = LOCAL ? s_off[0] : rd.work_off;
    const int *off_c = LOCAL ? s_off[2] : rd.work_off + (size_t)2 * (RL_MAX_SEG + 1);
    const bool coop_all = rc.knn_coop && off_s[n_seg] <= LL_KNN_COOP_MAX_QUERIES;
    const bool coop = rc.knn_coop && off_c[n_seg] <= LL_KNN_COOP_MAX_QUERIES;  // the corner ones at least
    if (coop_all || coop) {
        // (handed out from the LAST wavefront of the grid backwards: the per-lane lists below fill the grid from the front, so
        // with short lists a wavefront has either a cooperative search or per-lane entries and the two chains overlap)
        const int *off_w = coop_all ? off_s : off_c;
        const int total_w = off_w[n_seg];
        const int n_waves = stride >> 6;
        for (int t = n_waves - 1 - (int)((blockIdx.x * RL_THREADS + tid) >> 6); t < total_w; t += n_waves) {
            int lo = 0, hi = n_seg;  // largest segment with off_w[segment] <= t (in off_c the empty surface segments tie with their successor)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off_w[mid] <= t) lo = mid; else hi = mid;
            }
            const int sgg = seg0 + lo, b = sgg >> 1, kind = sgg & 1;
            const int e = rd.work_search[(size_t)b * rd.cap + (kind ? rd.cap_c : 0) + (t - off_w[lo])];
            const int slot = e - b * rd.cap;
            knn_one_coop(rd, rc, gc, gs, b, slot, iter);
            if ((tid & 63) == 0) build_one(rd, rc, gc, gs, b, slot);
        }
    }
    // (one index space over both lists, so that a lane never runs a re-sort after a search, brought the floor from 113 back
    // to 99 us but cost 25 % at the long early lists -- profiles/r02 runs U / V -- and was dropped)
    for (int w = coop_all ? 1 : 0; w < 2; w++) {
        const int *off = LOCAL ? s_off[w] : rd.work_off + (size_t)w * (RL_MAX_SEG + 1);
        const int total = off[n_seg];
        const int *list = w == 0 ? rd.work_search : rd.work_build;
        for (int t = blockIdx.x * RL_THREADS + tid; t < total; t += stride) {
            int lo = 0, hi = n_seg;  // largest segment with off[segment] <= t
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (off[mid] <= t) lo = mid; else hi = mid;
            }
            const int sgg = seg0 + lo, b = sgg >> 1, kind = sgg & 1;
            if (w == 0 && coop && kind == 0) continue;  // done above
            const int e = list[(size_t)b * rd.cap + (kind ? rd.cap_c : 0) + (t - off[lo])];
            const int slot = e - b * rd.cap;
            if (w == 0) knn_one(rd, rc, gc, gs, b, slot, iter);
            else resort_one(rd, rc, gc, gs, b, slot, iter);
            build_one(rd, rc, gc, gs, b, slot);
        }
    }
}

// ---- a map per slot (ll_reg_enqueue_fe_maps) --------------------------------------------------------------------------------------
// Scan b is searched against map_tab[2 b] (corner) / map_tab[2 b + 1] (surface); its solver is reg_solve_maps_kernel
// (ll_reg_maps_kernels.hip).  The scan is uniform per workgroup (blockIdx.y), so a workgroup reads its two grids once through
// scalar loads and then runs the same knn_one / build_one as the single-map kernels above.  A slot that does not run (gated,
// idle) has st->done set by the host and zeroed table entries that nobody reads.
__global__ __launch_bounds__(KB_THREADS) __attribute__((amdgpu_waves_per_eu(KNN_WAVES_PER_EU, 8)))
void reg_knn_maps_kernel(RegDev rd, RegConst rc, const Grid *__restrict__ map_tab, int iter, int skip_kinds)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    if ((skip_kinds >> kind) & 1) return;  // reg_knn_coop_maps_kernel has them
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    const int q = blockIdx.x * KB_THREADS + threadIdx.x;
    if (q >= n) return;
    const Grid gc = map_tab[2 * b], gs = map_tab[2 * b + 1];
    knn_one(rd, rc, gc, gs, b, (kind ? rd.cap_c : 0) + q, iter);
}

__global__ __launch_bounds__(KC_THREADS) void reg_knn_coop_maps_kernel(RegDev rd, RegConst rc, const Grid *__restrict__ map_tab, int iter, int kinds)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    if (!((kinds >> kind) & 1)) return;
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int q = (int)((blockIdx.x * KC_THREADS + threadIdx.x) >> 6);
    if (q >= (kind ? rd.n_surf[b] : rd.n_corner[b])) return;  // (whole wavefronts)
    const Grid gc = map_tab[2 * b], gs = map_tab[2 * b + 1];
    knn_one_coop(rd, rc, gc, gs, b, (kind ? rd.cap_c : 0) + q, iter);
}

__global__ __launch_bounds__(KB_THREADS) void reg_build_maps_kernel(RegDev rd, RegConst rc, const Grid *__restrict__ map_tab)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    const int q = blockIdx.x * KB_THREADS + threadIdx.x;
    if (q >= n) return;
    const Grid gc = map_tab[2 * b], gs = map_tab[2 * b + 1];
    build_one(rd, rc, gc, gs, b, (kind ? rd.cap_c : 0) + q);
}

// Motion deblur with a map per slot (ll_reg_set_time_ranges): the two per-query steps that read the time range -- the transform
// (transform_query -> point_to_map_undistort) and the blur ratio of the block constants (build_one's sblur) -- with scan b's own pair
// from ts_tab[b] in place of rc.min_ts / rc.max_ts.  The scan is uniform per workgroup, so the pair arrives through a scalar load
// and lands in a copy of the constants; the arithmetic is transform_query's and build_one's, and the searches in between do not read
// the range.  Kernels of their own: reg_transform_kernel and reg_build_maps_kernel keep their argument lists and their code.
__global__ __launch_bounds__(KB_THREADS) void reg_transform_ranges_kernel(RegDev rd, RegConst rc, const float2 *__restrict__ ts_tab)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    const int q = blockIdx.x * KB_THREADS + threadIdx.x;
    if (q >= n) return;
    const float2 ts = ts_tab[b];
    rc.min_ts = ts.x;
    rc.max_ts = ts.y;
    const int slot = (kind ? rd.cap_c : 0) + q;
    float pw[3];
    transform_query(st, rc, load_feature(rd, b, kind, q), pw);
    if (subsample_skip_feature(rc.subsample_seed, kind, st->icp_iters, q, n, rc.max_blocks)) pw[0] = pw[1] = pw[2] = NAN;  // (as reg_transform_kernel)
    rd.qw[(size_t)b * rd.cap + slot] = make_float4(pw[0], pw[1], pw[2], 0.f);
}

__global__ __launch_bounds__(KB_THREADS) void reg_build_ranges_kernel(RegDev rd, RegConst rc, const Grid *__restrict__ map_tab, const float2 *__restrict__ ts_tab)
{
    const int b = blockIdx.y, kind = blockIdx.z;
    const RegState *st = rd.state + b;
    if (st->done) return;
    const int n = kind ? rd.n_surf[b] : rd.n_corner[b];
    const int q = blockIdx.x * KB_THREADS + threadIdx.x;
    if (q >= n) return;
    const Grid gc = map_tab[2 * b], gs = map_tab[2 * b + 1];
    const float2 ts = ts_tab[b];
    rc.min_ts = ts.x;
    rc.max_ts = ts.y;
    build_one(rd, rc, gc, gs, b, (kind ? rd.cap_c : 0) + q);
}

// ---- launch wrappers -------------------------------------------------------------------------------------------
void launch_reg_knn_build(const RegDev &rd, const RegConst &rc, const Grid &gc, const Grid &gs, int n_scans, int iter,
                          int max_nc, int max_ns, hipStream_t s)
{
    if (iter >= rc.knn_reuse_from && rc.knn_reuse) {
        if (max_nc + max_ns <= 0) return;
        const int mx = max_nc > max_ns ? max_nc : max_ns;
        dim3 cgrid((mx + RQ_PER * RQ_THREADS - 1) / (RQ_PER * RQ_THREADS), n_scans, 2);
        (void)hipMemsetAsync(rd.work_cnt, 0, (size_t)n_scans * 4 * sizeof(int), s);
        hipLaunchKernelGGL(reg_requery_kernel, cgrid, dim3(RQ_THREADS), 0, s, rd, rc, gc, gs, iter);
        for (int seg0 = 0; seg0 < 2 * n_scans; seg0 += RL_MAX_SEG) {
            const int n_seg = 2 * n_scans - seg0 < RL_MAX_SEG ? 2 * n_scans - seg0 : RL_MAX_SEG;
            static const int local_seg = getenv("LL_LIST_NO_LOCAL_OFFSETS") ? 0 : RL_LOCAL_SEG;  // (A/B switch)
            if (n_seg <= local_seg) {
                hipLaunchKernelGGL(reg_list_kernel<true>, dim3(256), dim3(RL_THREADS), 0, s, rd, rc, gc, gs, iter, seg0, n_seg);
            } else {
                hipLaunchKernelGGL(reg_list_offsets_kernel, dim3(1), dim3(1024), 0, s, rd, seg0, n_seg);
                hipLaunchKernelGGL(reg_list_kernel<false>, dim3(n_scans >= 64 ? RL_BLOCKS : 256), dim3(RL_THREADS), 0, s, rd, rc, gc, gs, iter, seg0, n_seg);
            }
        }
        return;
    }
    // corner and surface queries share every launch (blockIdx.z = kind): the few hundred corner queries of a scan
    // are latency-bound on their own and would otherwise serialise three more launches per iteration
    const int mx = max_nc > max_ns ? max_nc : max_ns;
    if (mx <= 0) return;
    dim3 grid((mx + KB_THREADS - 1) / KB_THREADS, n_scans, 2);
    // large scans: the surface queries go to the tile kernel (ll_knn_kernels.hip) in the order of the map cells they fall into (sorted at
    // ICP iterations 0 and 1: the first pose update moves the queries by a good part of a cell, the later ones by centimetres); it also
    // builds their blocks and, without motion deblur, transforms them itself
    const bool tile = rc.knn_tile && max_ns >= LL_KNN_TILE_MIN_SURF && max_ns <= LL_KNN_TILE_MAX_SURF;
    const bool fused = tile && !rc.if_motion_deblur;
    // small batches: the corner queries one per wavefront, and the surface queries too when the scans are small
    int coop_kinds = 0;
    if (rc.knn_coop && n_scans <= LL_KNN_COOP_MAX_SCANS) {
        if (max_nc > 0) coop_kinds |= 1;
        if (max_ns > 0 && max_ns <= LL_KNN_COOP_MAX_SURF && !tile) coop_kinds |= 2;
    }
    const bool corner_in_tile = tile && max_nc > 0 && !(coop_kinds & 1);  // ... otherwise they ride in the tile launch
    {
        const int skip = fused ? (corner_in_tile ? 3 : 2) : 0;
        if (skip != 3 && (skip == 0 || max_nc > 0)) {
            const int mt = skip == 2 ? max_nc : mx;
            hipLaunchKernelGGL(reg_transform_kernel, dim3((mt + KB_THREADS - 1) / KB_THREADS, n_scans, 2), dim3(KB_THREADS), 0, s, rd, rc, skip);
        }
    }
    if (tile && iter <= rc.knn_tile_last_sort) launch_reg_qsort(rd, rc, gc, gs, n_scans, corner_in_tile ? max_nc : 0, max_ns, fused, s);
    if (coop_kinds) {
        const int mq = (coop_kinds & 2) ? mx : max_nc;
        hipLaunchKernelGGL(reg_knn_coop_kernel, dim3((mq * 64 + KC_THREADS - 1) / KC_THREADS, n_scans, 2), dim3(KC_THREADS), 0, s, rd, rc, gc, gs, iter, coop_kinds);
    }
    const int done_kinds = coop_kinds | (tile ? 2 : 0) | (corner_in_tile ? 1 : 0);  // kinds that do not need the per-lane kernel
    if ((max_nc > 0 && !(done_kinds & 1)) || (max_ns > 0 && !(done_kinds & 2))) {
        const int mk = (done_kinds & 2) ? max_nc : ((done_kinds & 1) ? max_ns : mx);
        hipLaunchKernelGGL(reg_knn_kernel, dim3((mk + KB_THREADS - 1) / KB_THREADS, n_scans, 2), dim3(KB_THREADS), 0, s, rd, rc, gc, gs, iter, done_kinds);
    }
    if (tile) {
        launch_reg_knn_tile(rd, rc, gc, gs, n_scans, iter, corner_in_tile ? max_nc : 0, max_ns, fused, s);
        if (max_nc > 0 && !corner_in_tile)
            hipLaunchKernelGGL(reg_build_kernel, dim3((max_nc + KB_THREADS - 1) / KB_THREADS, n_scans, 2), dim3(KB_THREADS), 0, s, rd, rc, gc, gs, 2);
    } else {
        hipLaunchKernelGGL(reg_build_kernel, grid, dim3(KB_THREADS), 0, s, rd, rc, gc, gs, 0);
    }
}
// A map per slot: every query of every running scan is searched in every ICP iteration -- per lane (reg_knn_maps_kernel), or per
// wavefront for the batches the single-map launcher serves that way -- and every block is rebuilt.  The tile search and the reuse
// lists have no table form (their work items are not bound to one scan per workgroup); the caller clears rc.knn_tile and
// rc.knn_reuse.  Every search form returns the same neighbour lists, so a slot gets the bits of its single-map registration.
void launch_reg_knn_build_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, int n_scans, int iter, int max_nc, int max_ns, hipStream_t s,
                               const float2 *ts_tab)
{
    (void)iter;
    const int mx = max_nc > max_ns ? max_nc : max_ns;
    if (mx <= 0) return;
    const dim3 grid((mx + KB_THREADS - 1) / KB_THREADS, n_scans, 2);
    if (ts_tab)
        hipLaunchKernelGGL(reg_transform_ranges_kernel, grid, dim3(KB_THREADS), 0, s, rd, rc, ts_tab);
    else
        hipLaunchKernelGGL(reg_transform_kernel, grid, dim3(KB_THREADS), 0, s, rd, rc, 0);
    int coop_kinds = 0;
    if (rc.knn_coop && n_scans <= LL_KNN_COOP_MAX_SCANS) {
        if (max_nc > 0) coop_kinds |= 1;
        if (max_ns > 0 && max_ns <= LL_KNN_COOP_MAX_SURF) coop_kinds |= 2;
    }
    if (coop_kinds) {
        const int mq = (coop_kinds & 2) ? mx : max_nc;
        hipLaunchKernelGGL(reg_knn_coop_maps_kernel, dim3((mq * 64 + KC_THREADS - 1) / KC_THREADS, n_scans, 2), dim3(KC_THREADS), 0, s, rd, rc, map_tab, iter,
                           coop_kinds);
    }
    if ((max_nc > 0 && !(coop_kinds & 1)) || (max_ns > 0 && !(coop_kinds & 2))) {
        const int mk = (coop_kinds & 2) ? max_nc : ((coop_kinds & 1) ? max_ns : mx);
        hipLaunchKernelGGL(reg_knn_maps_kernel, dim3((mk + KB_THREADS - 1) / KB_THREADS, n_scans, 2), dim3(KB_THREADS), 0, s, rd, rc, map_tab, iter,
                           coop_kinds);
    }
    if (ts_tab)
        hipLaunchKernelGGL(reg_build_ranges_kernel, grid, dim3(KB_THREADS), 0, s, rd, rc, map_tab, ts_tab);
    else
        hipLaunchKernelGGL(reg_build_maps_kernel, grid, dim3(KB_THREADS), 0, s, rd, rc, map_tab);
}

}  // namespace ll
