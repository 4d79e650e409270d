// ll_reg_small_kernels.hip -- the solver for SMALL scans (gfx950, wave64): the reference's real operating point.
//
// laser_mapping.hpp:1367-1373 voxel-filters the feature clouds before every registration (input_downsample_mode, leaf 0.1 / 0.4 m) and
// config/performance_*.yaml caps a problem at maximum_residual_blocks = 200: a registration then has a few hundred residual blocks, not
// the 17 000 of an unfiltered Mid-40 sweep.  reg_solve_kernel (ll_reg_solve_kernels.hip) gives every scan a 512-thread workgroup, 158 KB of LDS
// and therefore a whole CU; on such a scan its eight wavefronts hold two blocks per lane, a third of the launch clears and scans fixed-size
// tables, and a batch lasts as long as its slowest scan's Levenberg-Marquardt controller while 250 CUs idle (profiles/r04c_qpipe_*:
// 772 us per launch of 256 scans).
//
// Here a scan is ONE wavefront (batches of >= LL_SMALL_W1_MIN_SCANS scans: many scans per CU -- the controller of one overlaps the
// evaluations of the others; throughput) or FOUR wavefronts (smaller batches: one scan per CU anyway, so the evaluations are spread over
// its four SIMDs; latency), and everything a registration's inner loop (point_cloud_registration.hpp:460-531) touches more than once lives in
// a few KB of LDS:
//   census    the scan's candidate blocks in the reference's order (corner queries, then surface queries): flags -> active / available
//             counts (PCR:325, 425), the reproducible sub-sampling of PCR:438-458 (ll_reg_core.h subsample_drop_block), and a dense
//             numbering of the kept blocks (ballot + popcount prefix: lines first, then planes);
//   build     line blocks are copied from the 65-byte records the k-NN stage wrote (ll_reg_query.h build_one); a plane block's {n', c}
//             is computed here from its neighbour triple with block_plane() -- the arithmetic of every other path, so the same bits --
//             instead of through a de-duplicating plane table (a few hundred blocks share almost no triples);
//             LDS, structure of arrays: f (3 x fp32), v' (3 x fp64), a0 (a'.x of a line / c of a plane), and a'.y, a'.z for lines:
//             44 B per block + 16 B per line block;
//   solve     cost evaluations read the blocks from LDS (one round ahead), 28 accumulators per lane -> the butterfly reduction of
//             ll_reg_solve_common.h -> the controller lane (the same lm_* code as every other path, the line-search fit on its
//             wavefront);
//   inliers   loss-corrected L1 values in registers; std::set de-duplication (PCR:155-160) and the rank select by a bitonic sort of
//             the 64-bit keys across the registers of a wavefront (no table, no LDS): equal keys end up adjacent, the distinct values are
//             counted and the wanted rank picked by a prefix sum;
//   epilogue  pose composition and the convergence test (solve_epilogue).
// Sums are grouped differently from the 512-thread forms, so results agree with them to rounding (poses ~1e-12, equal block / iteration
// counts: tests/test_gpu_small.py), not bit for bit; a scan's answer does not depend on its slot or on the batch size within one form.
#include <hip/hip_runtime.h>

#include "ll_reg_query.h"
#include "ll_reg_solve_common.h"

namespace ll {

// R_inc / t_inc of the evaluation point x = {q, t}
#define LL_CTX_DECL_SMALL(x)                                   \
    double R_[9], t_[3];                                        \
    {                                                           \
        const double q_[4] = {(x)[0], (x)[1], (x)[2], (x)[3]};  \
        quat_to_mat(q_, R_);                                    \
        t_[0] = (x)[4];                                         \
        t_[1] = (x)[5];                                         \
        t_[2] = (x)[6];                                         \
    }

#ifdef LL_SOLVE_TIMING
#define SM_T0(var) long long var = clock64()
#define SM_TACC(slot, var)                                      \
    do {                                                        \
        if (threadIdx.x == 0) sh.tcyc[slot] += clock64() - var; \
    } while (0)
#else
#define SM_T0(var)
#define SM_TACC(slot, var)
#endif

struct SmallShared {
    long long tcyc[16];  // LL_SOLVE_TIMING builds: evaluations, controller, L1 pass, sort + select, -, total, census, prune, build (RegState::dbg_cycles)
    LmCtl ctl;
    double red[8][LL_NACC];  // per-wavefront sums of an evaluation (W <= 8)
    double sum[LL_NACC];
    double fit[10];
    double thr;
    double x_start[7];
    int need, n_active, n_corner_avail, n_surf_avail;
    int nL, nA;              // kept line blocks, kept blocks (lines first)
    int n_eval;              // cost evaluations of this launch
    int cnt[16][8];          // census: active blocks per (round, wavefront)
    int isum[8];
    unsigned long long lsum[8];
    int hist[256];           // W >= 4: digit histogram of the radix select
    int sel_digit, sel_rank;
};

// what the kernel reads of the registrar's buffers (ll_device.h RegDev holds ~50 pointers: passed whole, the ones a phase keeps live
// crowd the scalar registers of a kernel that already spills them)
struct SmallArgs {
    RegState *state;
    const int *n_corner, *n_surf;
    const int *order;              // scan of workgroup i (longest first, reg_solve_order_kernel), or nullptr
    const unsigned char *blk_flag0;
    const float4 *blk_f;
    const double *blk_av;
    const int4 *nn;
    const float4 *surf_feat;
    const f4 *map_surf;
    int cap_all, cap_c, feat_stride_s;  // RegDev::cap, cap_c, feat_stride_s
    int cap, capl;                      // LDS capacity in blocks / line blocks
};

// the LDS arrays of one scan (dynamic shared memory): see the header
struct SmallBlocks {
    LL_AS_LDS double *v0, *v1, *v2, *a0, *a1, *a2;
    LL_AS_LDS float *fx, *fy, *fz;
};

template <int W>
__device__ __forceinline__ unsigned long long small_sum_u64(unsigned long long v, SmallShared &sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += (unsigned long long)__shfl_xor((long long)v, off);
    if (W == 1) return v;
    if (lane == 0) sh.lsum[wave] = v;
    __syncthreads();
    unsigned long long s = 0;
#pragma unroll
    for (int w = 0; w < W; w++) s += sh.lsum[w];
    __syncthreads();
    return s;
}

// compare-exchange of two keys held by the same lane
__device__ __forceinline__ void cx_local(unsigned long long &a, unsigned long long &b, bool up)
{
    const bool sw = (b < a) == up;  // (equal keys: swapping them or not is the same)
    const unsigned long long lo = sw ? b : a, hi = sw ? a : b;
    a = lo;
    b = hi;
}

// Bitonic sort (ascending) of 64 * K keys held K per lane, element g = lane * K + r.  Every step is a fixed data-parallel pattern: pairs
// closer than K live in one lane's registers, the others are exchanged through the crossbar.
template <int K>
__device__ __forceinline__ void wave_bitonic_sort(unsigned long long (&key)[K], int lane)
{
    static_assert(K == 1 || K == 2 || K == 4 || K == 8 || K == 16, "keys per lane: a power of two");
    constexpr int N = 64 * K;
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j >= 1; j >>= 1) {
            if (j >= K) {
                const int lj = j / K;  // partner lane = lane ^ lj, same register
                const bool lower = (lane & lj) == 0;
#pragma unroll
                for (int r = 0; r < K; r++) {
                    const int g = lane * K + r;
                    const bool up = (g & k) == 0;
                    const unsigned long long mine = key[r];
                    const unsigned long long other = (unsigned long long)__shfl_xor((long long)mine, lj);
                    const bool keep_min = lower == up;
                    const bool take = (other < mine) == keep_min;  // one compare, no branch (equal keys: taking the partner's is the same)
                    key[r] = take ? other : mine;
                }
            } else {
#pragma unroll
                for (int r = 0; r < K; r++) {
                    if ((r & j) == 0) {
                        const int g = lane * K + r;
                        const bool up = (g & k) == 0;
                        cx_local(key[r], key[r | j], up);
                    }
                }
            }
        }
    }
}

// workgroup evaluation of cost / g / H at x over the active blocks -> sh.sum
template <int W>
__device__ __forceinline__ void small_eval(const SmallBlocks &B, const double *x, double huber_a, unsigned int act, int nL, int nA, SmallShared &sh)
{
    constexpr int DEBLUR = 0;
    constexpr int NT = 64 * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    LL_CTX_DECL_SMALL(x)
    double acc[LL_NACC];
#pragma unroll
    for (int i = 0; i < LL_NACC; i++) acc[i] = 0.0;
    if (nA > 0) {
        // one round ahead: the next block's ten values are fetched from LDS (clamped index, unconditional) while this one is evaluated
        int idx = tid < nA ? tid : nA - 1;
        float nfx = B.fx[idx], nfy = B.fy[idx], nfz = B.fz[idx];
        double nv0 = B.v0[idx], nv1 = B.v1[idx], nv2 = B.v2[idx], na0 = B.a0[idx];
        int il = idx < nL ? idx : 0;
        double na1 = B.a1[il], na2 = B.a2[il];
        for (int r = 0; r * NT < nA; r++) {
            const int cur = r * NT + tid;
            const double f[3] = {(double)nfx, (double)nfy, (double)nfz};
            const double v[3] = {nv0, nv1, nv2};
            const double a[3] = {na0, na1, na2};
            {
                const int nx = cur + NT;
                idx = nx < nA ? nx : nA - 1;
                nfx = B.fx[idx], nfy = B.fy[idx], nfz = B.fz[idx];
                nv0 = B.v0[idx], nv1 = B.v1[idx], nv2 = B.v2[idx], na0 = B.a0[idx];
                il = idx < nL ? idx : 0;
                na1 = B.a1[il], na2 = B.a2[il];
            }
            if (cur < nA && ((act >> r) & 1u)) {
                if (cur < nL) {
                    block_accumulate(BLK_LINE, R_, t_, f, a, v, huber_a, acc);  // ICP:238-380
                } else {
                    const double ap[3] = {a[0], 0.0, 0.0};
                    block_accumulate(BLK_PLANE, R_, t_, f, ap, v, huber_a, acc);
                }
            }
        }
    }
    wave_sum_acc(acc, sh.red[wave], lane);
    __syncthreads();
    if (tid < LL_NACC) {
        double s = sh.red[0][tid];
#pragma unroll
        for (int w = 1; w < W; w++) s += sh.red[w][tid];
        sh.sum[tid] = s;
    }
    __syncthreads();
}

// one ceres::Solve: starts at x0, leaves the result in sh.ctl
template <int W>
__device__ __forceinline__ void small_lm(const SmallBlocks &B, const RegConst &rc, const double *x0, int max_iter, unsigned int act, SmallShared &sh)
{
    const int tid = threadIdx.x;
    if (tid == 0) lm_begin(sh.ctl, x0, max_iter, rc.bound);
    __syncthreads();
    {
        SM_T0(t0);
        small_eval<W>(B, sh.ctl.x, rc.huber_a, act, sh.nL, sh.nA, sh);
        SM_TACC(0, t0);
    }
    {
        SM_T0(t1);
        if (tid < 64) {  // the controller's wavefront
            const int need = lm_init_wave(sh.ctl, sh.sum, sh.n_active, tid);
            if (tid == 0) sh.need = need;
        }
        __syncthreads();
        SM_TACC(1, t1);
    }
    while (sh.need) {
        SM_T0(t0);
        small_eval<W>(B, sh.ctl.cand, rc.huber_a, act, sh.nL, sh.nA, sh);
        SM_TACC(0, t0);
        SM_T0(t1);
        if (tid < 64) {  // the controller's wavefront steps the controller (ll_lm_wave.h); lane 0 has the answer
            const int need = lm_update_wave(sh.ctl, sh.sum, sh.fit, tid, sh.tcyc + 14);
            if (tid == 0) {
                sh.need = need;
                sh.n_eval++;
            }
        }
        __syncthreads();
        SM_TACC(1, t1);
#ifdef LL_SOLVE_TIMING
        if (tid == 0) sh.tcyc[9] += 1;  // evaluations beyond the first of a solve
#endif
    }
}

// W wavefronts per scan, at most M candidate blocks per thread (64 * W * M >= n_corner + n_surf of every scan of the batch)
#define LL_SMALL_KERNEL reg_solve_small_kernel
#define LL_SMALL_MORE_ARGS
#define LL_SMALL_BIND_MAP
#include "ll_reg_small_solve.h"
#undef LL_SMALL_KERNEL
#undef LL_SMALL_MORE_ARGS
#undef LL_SMALL_BIND_MAP

// a map per slot (ll_reg_enqueue_fe_maps): the surface map of scan b is entry 2 b + 1 of the table (one scalar load per workgroup)
#define LL_SMALL_KERNEL reg_solve_small_maps_kernel
#define LL_SMALL_MORE_ARGS , const Grid *map_tab, int cls
#define LL_SMALL_BIND_MAP                                                         \
    if (reg_maps_class(rc, rd.n_corner[b], rd.n_surf[b], 0x7fffffff) != cls) return; /* (another launch has this scan) */ \
    map_surf = map_tab[2 * b + 1].pts;
#include "ll_reg_small_solve.h"
#undef LL_SMALL_KERNEL
#undef LL_SMALL_MORE_ARGS
#undef LL_SMALL_BIND_MAP

// Longest first: the scans of a batch differ five-fold in the work of a launch (the ones whose step runs into the bound on t_inc contract a
// line search: dozens of extra evaluations), a launch of more scans than the device holds at once ends when its last scan does, and a
// scan's work changes little from one ICP iteration to the next.  One workgroup orders the scans by the evaluations of their previous
// launch, descending (counting sort: the first launch of a registration runs in scan order).  Only the order of dispatch depends on it, no result does.
#define SO_THREADS 1024
#define SO_BINS 256
__global__ __launch_bounds__(SO_THREADS) void reg_solve_order_kernel(const RegState *state, int n_scans, int *order)
{
    __shared__ int hist[SO_BINS], start[SO_BINS];
    const int tid = threadIdx.x;
    for (int e = tid; e < SO_BINS; e += SO_THREADS) hist[e] = 0;
    __syncthreads();
    for (int b = tid; b < n_scans; b += SO_THREADS) {
        int w = state[b].last_work;
        w = w < 0 ? 0 : (w > SO_BINS - 1 ? SO_BINS - 1 : w);
        atomicAdd(&hist[SO_BINS - 1 - w], 1);  // bin 0 = the most work
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int e = 0; e < SO_BINS; e++) {
            start[e] = run;
            run += hist[e];
        }
    }
    __syncthreads();
    for (int b = tid; b < n_scans; b += SO_THREADS) {  // (the order inside a bin is whatever the atomics hand out: it decides nothing but timing)
        int w = state[b].last_work;
        w = w < 0 ? 0 : (w > SO_BINS - 1 ? SO_BINS - 1 : w);
        order[atomicAdd(&start[SO_BINS - 1 - w], 1)] = b;
    }
}

// dynamic LDS of one scan
static size_t small_lds_bytes(int W, int M, int cap, int capl)
{
    const int keys = M * 64 * W;
    const int ns = W <= 2 ? 0 : (keys <= 256 ? 256 : (keys <= 512 ? 512 : (keys <= 1024 ? 1024 : 2048)));  // (NS of the kernel)
    return (size_t)cap * (4 * 8 + 3 * 4) + (size_t)capl * 16 + (size_t)ns * 16;  // (W >= 4: a hash table of 2 NS slots)
}

template <int W, int M, bool MAPS>
static void launch_small(const SmallArgs &a, const RegConst &rc, const Grid *map_tab, int maps_cls, int n_scans, hipStream_t s)
{
    const size_t lds = small_lds_bytes(W, M, a.cap, a.capl);
    const void *fn = MAPS ? (const void *)reg_solve_small_maps_kernel<W, M> : (const void *)reg_solve_small_kernel<W, M>;
    static bool attr_set = false;
    if (!attr_set) {  // dynamic LDS beyond the default 64 KB: everything the CU has left beside the kernel's static block
        hipFuncAttributes fa;
        int room = 160 * 1024 - 8 * 1024;
        if (hipFuncGetAttributes(&fa, fn) == hipSuccess) room = 160 * 1024 - (int)fa.sharedSizeBytes;
        if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, room) != hipSuccess)
            (void)hipGetLastError();  // (not sticky: a launch that needs more than the default then fails on its own)
        attr_set = true;
    }
    if (MAPS)
        hipLaunchKernelGGL((reg_solve_small_maps_kernel<W, M>), dim3(n_scans), dim3(64 * W), lds, s, a, rc, map_tab, maps_cls);
    else
        hipLaunchKernelGGL((reg_solve_small_kernel<W, M>), dim3(n_scans), dim3(64 * W), lds, s, a, rc);
}

bool reg_solve_small_eligible(const RegConst &rc, int max_nc, int max_ns)
{
    return !rc.if_motion_deblur && !rc.force_general && !rc.no_small_solver && max_nc + max_ns > 0 &&
           max_nc + max_ns <= LL_SMALL_MAX_BLOCKS && max_nc <= 1024;  // (line blocks take 16 B more of LDS each)
}

// wavefronts per scan: four for batches that leave CUs idle anyway (latency); for large batches as many as keep two wavefronts per SIMD
// busy at the number of scans whose blocks fit a CU's LDS together (256 VGPRs per wavefront: eight wavefronts per CU)
int reg_solve_small_waves(const RegConst &rc, int n_scans, int max_nc, int max_ns)
{
    const int total = max_nc + max_ns;
    if (total > 1024) return 8;  // (the only form that holds them)
    if (rc.small_waves) return rc.small_waves;
    if (n_scans < LL_SMALL_W1_MIN_SCANS) return 4;
    const int cap = (total + 63) / 64 * 64, capl = (max_nc + 63) / 64 * 64 + 64;
    const size_t per_scan = small_lds_bytes(1, 1, cap, capl) + sizeof(SmallShared) + 512;
    const int per_cu = (int)((size_t)(160 * 1024) / per_scan);
    return per_cu >= 8 ? 1 : (per_cu >= 4 ? 2 : 4);
}

template <bool MAPS>
static void launch_reg_solve_small_any(const RegDev &rd, const RegConst &rc, const f4 *map_surf, const Grid *map_tab, int maps_cls, int n_scans, int max_nc, int max_ns, int iter, hipStream_t s)
{
    const int total = max_nc + max_ns;
    SmallArgs a;
    a.state = rd.state, a.n_corner = rd.n_corner, a.n_surf = rd.n_surf, a.blk_flag0 = rd.blk_flag0, a.blk_f = rd.blk_f, a.blk_av = rd.blk_av;
    a.nn = rd.nn, a.surf_feat = rd.surf_feat, a.map_surf = map_surf, a.cap_all = rd.cap, a.cap_c = rd.cap_c, a.feat_stride_s = rd.feat_stride_s;
    a.cap = (total + 63) / 64 * 64, a.capl = (max_nc + 63) / 64 * 64 + 64;  // (+64: the clamped line index of a scan without lines stays inside)
    // (a map per slot: the wavefronts the scan would get ALONE -- the one- and two-wavefront forms of large batches group their sums
    //  differently, and a slot must give the bits of its own registration whatever the batch size)
    const int W = reg_solve_small_waves(rc, MAPS ? 1 : n_scans, max_nc, max_ns);
    // more scans than the device runs at once: longest first (from the second launch of a registration on)
    a.order = nullptr;
    if (rd.solve_order && !rc.no_solve_order && n_scans >= LL_SMALL_ORDER_MIN_SCANS && n_scans <= LL_SMALL_ORDER_MAX_SCANS && iter > 0) {
        hipLaunchKernelGGL(reg_solve_order_kernel, dim3(1), dim3(SO_THREADS), 0, s, rd.state, n_scans, rd.solve_order);
        a.order = rd.solve_order;
    }
    const int cls = total <= 256 ? 0 : (total <= 512 ? 1 : 2);  // 64 * W * M >= total (more than 1024: eight wavefronts, M = 4)
    if (W == 1) {
        if (cls == 0) launch_small<1, 4, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
        else if (cls == 1) launch_small<1, 8, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
        else launch_small<1, 16, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
    } else if (W == 2) {
        if (cls == 0) launch_small<2, 2, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
        else if (cls == 1) launch_small<2, 4, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
        else launch_small<2, 8, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
    } else if (W == 4) {
        if (cls == 0) launch_small<4, 1, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
        else if (cls == 1) launch_small<4, 2, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
        else launch_small<4, 4, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
    } else {
        launch_small<8, 4, MAPS>(a, rc, map_tab, maps_cls, n_scans, s);
    }
}
void launch_reg_solve_small(const RegDev &rd, const RegConst &rc, const Grid &gs, int n_scans, int max_nc, int max_ns, int iter, hipStream_t s)
{
    launch_reg_solve_small_any<false>(rd, rc, gs.pts, nullptr, 0, n_scans, max_nc, max_ns, iter, s);
}
// (cls, max_nc, max_ns: the class of reg_maps_class this launch serves and the largest scan of that class)
void launch_reg_solve_small_maps(const RegDev &rd, const RegConst &rc, const Grid *map_tab, int n_scans, int cls, int max_nc, int max_ns, int iter, hipStream_t s)
{
    launch_reg_solve_small_any<true>(rd, rc, nullptr, map_tab, cls, n_scans, max_nc, max_ns, iter, s);
}

}  // namespace ll
