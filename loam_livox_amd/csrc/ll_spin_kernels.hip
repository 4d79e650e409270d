// ll_spin_kernels.hip -- HIP kernels (gfx950, wave64) of the spinning-lidar feature extraction, the branch of
// Laser_feature::laserCloudHandler for lidar_type != "livox" (hku-mars/loam_livox source/laser_feature_extractor.hpp:393-787).
// B scans resident in HBM, one slot of `stride` points each.
//
//   spin_assign_kernel  : per input point: NaN / minimum-range filter, scan ID, raw orientation, and the list of points whose
//                         atanf / atan2f result lies within SPIN_BAND_ULP ulps of a decision (re-decided by ll_spin_resolve)
//   spin_lines_kernel   : one workgroup per scan: the halfPassed flip (first point whose unwrapped orientation passes
//                         startOri + pi, a min-index reduction), then a stable counting sort of the kept points by scan ID
//                         that writes laserCloud (:513-521) with the final orientation and intensity (:470-502)
//   spin_curv_kernel    : per position: the 11-point curvature and the backward-occlusion / parallel-beam flags (:524-597)
//   spin_sort_kernel    : one workgroup per sub-region: stable sort by curvature = sort of (curvature bits, position) keys
//                         (non-negative floats order as their bit patterns); bitonic in LDS, rank sort for huge sub-regions
//   spin_select_kernel  : one wavefront per scan, sub-regions in reference order (:631-767): candidates are consumed 64 at a
//                         time with ballots against a picked bitmap in LDS; the neighbour walks run 64 steps per ballot
//   spin_gather_kernel  : concatenates the per-line VoxelGrid outputs (:769-776; the filter is ll_voxel_kernels.hip's)
//   spin_pack_kernel    : hand-off: a list of positions (sharp / less-sharp / flat) -> a packed cloud + the [S] count arrays
#include <hip/hip_runtime.h>

#include "ll_spin.h"

namespace ll {

__global__ __launch_bounds__(256) void spin_assign_kernel(SpinDev d, int scan_line)
{
    const int s = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= d.n_in[s]) return;
    const size_t o = (size_t)s * d.stride + i;
    const float4 p = d.in[o];
    int sid = -1;
    float ori = 0.f;
    const float thres = d.thres;
    if (ll_isfinite(p.x) && ll_isfinite(p.y) && ll_isfinite(p.z) && !(p.x * p.x + p.y * p.y + p.z * p.z < thres * thres)) {
        const float angle = spin_angle(p.x, p.y, p.z);
        sid = spin_scan_id(angle, scan_line);
        int amb = spin_angle_ambiguous(angle, scan_line);
        if (sid >= 0 || amb) {
            ori = spin_ori(p.x, p.y);
            const float2 se = d.ori_se[s];
            amb |= spin_ori_ambiguous(ori, se.x, se.y);
        }
        if (amb) {
            const int k = atomicAdd(d.n_ambig, 1);
            if (k < d.ambig_cap) d.ambig[k] = make_int2(s, i);
        }
    }
    d.raw_sid[o] = sid;
    d.raw_ori[o] = ori;
}

#define SPIN_LT 128  // threads of spin_lines_kernel; the counting sort keeps [64 lines][SPIN_LT] counters in LDS (32 KB)

__global__ __launch_bounds__(SPIN_LT) void spin_lines_kernel(SpinDev d, int scan_line)
{
    const int s = blockIdx.x;
    const int t = threadIdx.x;
    const int n_in = d.n_in[s];
    const size_t base = (size_t)s * d.stride;
    const float2 se = d.ori_se[s];
    __shared__ unsigned int cnt[SPIN_MAX_LINES * SPIN_LT];
    __shared__ int s_flip;
    __shared__ unsigned int s_line[SPIN_MAX_LINES + 1];
    if (t == 0) s_flip = 0x7fffffff;
    for (int k = t; k < SPIN_MAX_LINES * SPIN_LT; k += SPIN_LT) cnt[k] = 0;
    __syncthreads();
    // the flip point: halfPassed is false up to and including it
    int flip = 0x7fffffff;
    for (int i = t; i < n_in; i += SPIN_LT) {
        if (d.raw_sid[base + i] < 0) continue;
        int w, f;
        (void)spin_unwrap_pre(d.raw_ori[base + i], se.x, &w, &f);
        if (f) {
            flip = i;
            break;
        }
    }
    atomicMin(&s_flip, flip);
    // stable counting sort: thread t owns the contiguous input range [lo, hi)
    const int seg = (n_in + SPIN_LT - 1) / SPIN_LT;
    const int lo = min(n_in, t * seg), hi = min(n_in, lo + seg);
    for (int i = lo; i < hi; i++) {
        const int sid = d.raw_sid[base + i];
        if (sid >= 0) cnt[sid * SPIN_LT + t]++;
    }
    __syncthreads();
    if (t < scan_line) {  // exclusive prefix along the threads of line t
        unsigned int acc = 0;
        for (int k = 0; k < SPIN_LT; k++) {
            const unsigned int c = cnt[t * SPIN_LT + k];
            cnt[t * SPIN_LT + k] = acc;
            acc += c;
        }
        s_line[t] = acc;
    }
    __syncthreads();
    if (t == 0) {
        unsigned int acc = 0;
        for (int l = 0; l < scan_line; l++) {
            const unsigned int c = s_line[l];
            s_line[l] = acc;
            acc += c;
        }
        s_line[scan_line] = acc;
    }
    __syncthreads();
    if (t <= scan_line) d.line_off[s * (SPIN_MAX_LINES + 1) + t] = (int)s_line[t];
    if (t == 0) {
        d.cnt[s * SPIN_NCNT + SPIN_C_FULL] = (int)s_line[scan_line];
        d.cnt[s * SPIN_NCNT + SPIN_C_STATUS] = 0;
    }
    flip = s_flip;
    for (int i = lo; i < hi; i++) {
        const int sid = d.raw_sid[base + i];
        if (sid < 0) continue;
        float ori = d.raw_ori[base + i];
        int w, f;
        if (i <= flip)
            ori = spin_unwrap_pre(ori, se.x, &w, &f);
        else
            ori = spin_unwrap_post(ori, se.y, &w);
        const float4 p = d.in[base + i];
        const unsigned int k = s_line[sid] + cnt[sid * SPIN_LT + t]++;
        d.full[base + k] = make_float4(p.x, p.y, p.z, spin_intensity(sid, ori, se.x, se.y));
        d.full_src[base + k] = i;
    }
}

__global__ __launch_bounds__(256) void spin_curv_kernel(SpinDev d)
{
    const int s = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = d.cnt[s * SPIN_NCNT + SPIN_C_FULL];
    if (i >= n) return;
    const size_t base = (size_t)s * d.stride;
    const float4 *p = d.full + base;
    float c = 0.f;
    unsigned char fl = 0;
    if (n > 10 && i >= 5 && i < n - 5) {
        c = spin_curvature(p, i);
        fl = (unsigned char)(spin_occlusion_back(p, i, c) | (spin_parallel(p, i, c) << 1));
    }
    d.curv[base + i] = c;
    d.flags[base + i] = fl;
    d.label[base + i] = 0;
}

#define SPIN_ST 256
#define SPIN_SORT_LDS 4096  // sub-regions up to this size sort in LDS; larger ones (a line of > ~24 k points) rank-sort in HBM

__device__ __forceinline__ unsigned long long spin_key(const float *curv, int k)
{
    return ((unsigned long long)__float_as_uint(curv[k]) << 32) | (unsigned int)k;
}

__global__ __launch_bounds__(SPIN_ST) void spin_sort_kernel(SpinDev d, int scan_line)
{
    const int s = blockIdx.y;
    const int line = blockIdx.x / 6, j = blockIdx.x % 6;
    if (line >= scan_line) return;
    const int *lo = d.line_off + s * (SPIN_MAX_LINES + 1);
    const int start = lo[line] + 5, end = lo[line + 1] - 6;
    int sp, ep;
    spin_subregion(start, end, j, &sp, &ep);
    const int m = ep - sp + 1;
    if (m <= 0) return;
    const size_t base = (size_t)s * d.stride;
    const float *curv = d.curv + base;
    int *order = d.order + base;
    const int t = threadIdx.x;
    if (m > SPIN_SORT_LDS) {
        for (int a = sp + t; a <= ep; a += SPIN_ST) {
            const unsigned long long ka = spin_key(curv, a);
            int r = 0;
            for (int b = sp; b <= ep; b++) r += spin_key(curv, b) < ka;
            order[sp + r] = a;
        }
        return;
    }
    __shared__ unsigned long long key[SPIN_SORT_LDS];
    int m2 = 1;
    while (m2 < m) m2 <<= 1;
    for (int k = t; k < m2; k += SPIN_ST) key[k] = k < m ? spin_key(curv, sp + k) : ~0ull;
    __syncthreads();
    for (int size = 2; size <= m2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int k = t; k < m2; k += SPIN_ST) {
                const int q = k ^ stride;
                if (q > k) {
                    const bool up = (k & size) == 0;
                    const unsigned long long a = key[k], b = key[q];
                    if ((a > b) == up) {
                        key[k] = b;
                        key[q] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
    for (int k = t; k < m; k += SPIN_ST) order[sp + k] = (int)(unsigned int)key[k];
}

// picked bitmap in LDS (dynamic, one bit per position of the scan)
__device__ __forceinline__ bool bm_get(const unsigned int *bm, int k) { return (bm[k >> 5] >> (k & 31)) & 1u; }
__device__ __forceinline__ void bm_set(unsigned int *bm, int k) { atomicOr(&bm[k >> 5], 1u << (k & 31)); }

// the walk of :679-710 / :725-756 from `ind` in direction dir (+1 / -1), at most `len` steps, stopping at the ends of the cloud
__device__ void spin_walk(const float4 *p, unsigned int *bm, int n, int ind, int dir, int len, int lane)
{
    for (int w0 = 1; w0 <= len; w0 += 64) {
        const int l = w0 + lane;
        const int q = ind + dir * l;
        bool brk = true;
        if (l <= len && q >= 0 && q <= n - 1) brk = spin_walk_breaks(p, q, q - dir);
        const unsigned long long bmask = __ballot(brk);
        const int stop = bmask ? (int)__ffsll((long long)bmask) - 1 : 64;  // first lane that breaks
        if (lane < stop) bm_set(bm, q);
        if (stop < 64) return;
    }
}

__global__ __launch_bounds__(64) void spin_select_kernel(SpinDev d, int scan_line, int n_vlines)
{
    extern __shared__ unsigned int bm[];
    const int s = blockIdx.x;
    const int lane = threadIdx.x;
    const size_t base = (size_t)s * d.stride;
    int *cnt = d.cnt + s * SPIN_NCNT;
    const int n = cnt[SPIN_C_FULL];
    const float4 *p = d.full + base;
    const float *curv = d.curv + base;
    const unsigned char *fl = d.flags + base;
    const int *order = d.order + base;
    signed char *label = d.label + base;
    int *o_sharp = d.sharp + base, *o_less_sharp = d.less_sharp + base, *o_flat = d.flat + base, *o_lf = d.lf_pos + base;
    const int words = (n + 31) >> 5;
    // initial picked flags: the parallel-beam mark of i and the backward occlusion marks of i .. i+5 (see ll_spin_core.h)
    for (int w = lane; w < words; w += 64) {
        unsigned int v = 0;
        for (int b = 0; b < 32; b++) {
            const int i = w * 32 + b;
            if (i < 5 || i > n - 6 || n <= 10) continue;
            bool pk = (fl[i] & 2) != 0;
            for (int k = 0; k <= 5 && i + k <= n - 6; k++) pk |= (fl[i + k] & 1) != 0;
            if (pk) v |= 1u << b;
        }
        bm[w] = v;
    }
    __syncthreads();
    const float sharp_point_threshold = 0.05f;
    const float thr_sharp = sharp_point_threshold * 10;
    int n_sharp = 0, n_less_sharp = 0, n_flat = 0, n_lf = 0, status = 0;
    const int *lo = d.line_off + s * (SPIN_MAX_LINES + 1);
    for (int line = 0; line < scan_line; line++) {
        const int start = lo[line] + 5, end = lo[line + 1] - 6;
        int lf_line = 0;
        float4 *vin = line < n_vlines ? d.vox_in + ((size_t)s * n_vlines + line) * d.line_cap : nullptr;
        for (int j = 0; j < 6; j++) {
            int sp, ep;
            spin_subregion(start, end, j, &sp, &ep);
            if (ep < sp) continue;
            // sharp pass: highest (curvature, position) first
            int picked_num = 0;
            bool done = false;
            for (int k0 = ep; k0 >= sp && !done; k0 -= 64) {
                const int k = k0 - lane;
                const bool valid = k >= sp;
                const int ind = valid ? order[k] : 0;
                const bool cand = valid && curv[ind] > thr_sharp;
                unsigned long long mask = __ballot(cand && !bm_get(bm, ind));
                while (mask) {
                    const int f = (int)__ffsll((long long)mask) - 1;
                    const int pi = __shfl(ind, f);
                    picked_num++;
                    if (picked_num > 200) {
                        done = true;
                        break;
                    }
                    if (lane == 0) {
                        label[pi] = picked_num <= 20 ? 2 : 1;
                        if (picked_num <= 20) o_sharp[n_sharp] = pi;
                        o_less_sharp[n_less_sharp] = pi;
                    }
                    if (picked_num <= 20) n_sharp++;
                    n_less_sharp++;
                    if (lane == 0) bm_set(bm, pi);
                    spin_walk(p, bm, n, pi, 1, 500, lane);
                    spin_walk(p, bm, n, pi, -1, 500, lane);
                    mask = __ballot(cand && lane > f && !bm_get(bm, ind));
                }
            }
            // flat pass: lowest (curvature, position) first; the 5th pick is not marked (:733-737)
            int small_num = 0;
            done = false;
            for (int k0 = sp; k0 <= ep && !done; k0 += 64) {
                const int k = k0 + lane;
                const bool valid = k <= ep;
                const int ind = valid ? order[k] : 0;
                const bool cand = valid && curv[ind] < sharp_point_threshold;
                unsigned long long mask = __ballot(cand && !bm_get(bm, ind));
                while (mask) {
                    const int f = (int)__ffsll((long long)mask) - 1;
                    const int pi = __shfl(ind, f);
                    if (lane == 0) {
                        label[pi] = -1;
                        o_flat[n_flat] = pi;
                    }
                    n_flat++;
                    small_num++;
                    if (small_num >= 5) {
                        done = true;
                        break;
                    }
                    if (lane == 0) bm_set(bm, pi);
                    spin_walk(p, bm, n, pi, 1, 5, lane);
                    spin_walk(p, bm, n, pi, -1, 5, lane);
                    mask = __ballot(cand && lane > f && !bm_get(bm, ind));
                }
            }
            __threadfence_block();  // the labels lane 0 wrote are read by every lane below
            // less flat: every position of the sub-region with label <= 0, in position order (:760-766)
            for (int k0 = sp; k0 <= ep; k0 += 64) {
                const int k = k0 + lane;
                const bool keep = k <= ep && label[k] <= 0;
                const unsigned long long m = __ballot(keep);
                const int before = __popcll(m & ((1ull << lane) - 1ull));
                if (keep) {
                    o_lf[n_lf + before] = k;
                    if (vin && lf_line + before < d.line_cap) vin[lf_line + before] = p[k];
                }
                n_lf += __popcll(m);
                lf_line += __popcll(m);
            }
        }
        if (lf_line > d.line_cap) status = SPIN_STATUS_LINE_OVERFLOW;
        if (line < n_vlines && lane == 0) d.vox_n[s * n_vlines + line] = min(lf_line, d.line_cap);
    }
    if (lane == 0) {
        cnt[SPIN_C_SHARP] = n_sharp;
        cnt[SPIN_C_LESS_SHARP] = n_less_sharp;
        cnt[SPIN_C_FLAT] = n_flat;
        cnt[SPIN_C_LF_PRE] = n_lf;
        cnt[SPIN_C_STATUS] = status;
    }
}

// concatenation of the per-line VoxelGrid outputs (surfPointsLessFlat += surfPointsLessFlatScanDS, :776)
__global__ __launch_bounds__(256) void spin_gather_kernel(SpinDev d, const float4 *vout, const int *vn, int out_stride, int n_vlines)
{
    const int s = blockIdx.x;
    __shared__ int s_off[SPIN_MAX_LINES + 1];
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int l = 0; l < n_vlines; l++) {
            s_off[l] = acc;
            acc += vn[s * n_vlines + l];
        }
        s_off[n_vlines] = acc;
        d.cnt[s * SPIN_NCNT + SPIN_C_LESS_FLAT] = acc;
    }
    __syncthreads();
    float4 *dst = d.less_flat + (size_t)s * d.stride;
    for (int l = 0; l < n_vlines; l++) {
        const int c = s_off[l + 1] - s_off[l];
        const float4 *src = vout + ((size_t)s * n_vlines + l) * out_stride;
        for (int k = threadIdx.x; k < c; k += 256) dst[s_off[l] + k] = src[k];
    }
}

// hand-off to the registrar: out[s][i] = full[s][list[s][i]], one lane per output point (16-byte stores, contiguous per scan); the
// sizes leave cnt[][] for the [S] arrays the registrar reads.  blockIdx.y strides over the points of a scan.
__global__ __launch_bounds__(256) void spin_pack_kernel(SpinDev d, const int *list, int cnt_slot, float4 *out, int out_stride, int *n_out, int *n_surf)
{
    const int s = blockIdx.x;
    const int *cnt = d.cnt + s * SPIN_NCNT;
    const int n = min(min(cnt[cnt_slot], out_stride), d.stride);
    const size_t base = (size_t)s * d.stride;
    const float4 *full = d.full + base;
    const int *pos = list + base;
    float4 *dst = out + (size_t)s * out_stride;
    for (int i = blockIdx.y * 256 + threadIdx.x; i < n; i += 256 * gridDim.y) {
        const int p = pos[i];
        dst[i] = (unsigned)p < (unsigned)d.stride ? full[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        n_out[s] = n;
        if (n_surf) n_surf[s] = min(cnt[SPIN_C_LESS_FLAT], d.stride);
    }
}

__global__ __launch_bounds__(256) void spin_ambig_kernel(SpinDev d, int n, int patch)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int2 a = d.ambig[k];
    const size_t o = (size_t)a.x * d.stride + a.y;
    if (patch) {
        d.raw_sid[o] = d.ambig_sid[k];
        d.raw_ori[o] = d.ambig_ori[k];
    } else {
        d.ambig_p[k] = d.in[o];
        d.ambig_sid[k] = d.raw_sid[o];
        d.ambig_ori[k] = d.raw_ori[o];
    }
}

void spin_launch_pack(const SpinDev &d, const int *list, int cnt_slot, float4 *out, int out_stride, int *n_out, int *n_surf, int n_scans,
                      hipStream_t st)
{
    // the clouds are a few hundred points (up to out_stride): two workgroups per scan keep short batches on enough CUs
    hipLaunchKernelGGL(spin_pack_kernel, dim3(n_scans, 2), dim3(256), 0, st, d, list, cnt_slot, out, out_stride, n_out, n_surf);
}

void spin_launch_ambig(const SpinDev &d, int n, bool patch, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(spin_ambig_kernel, dim3((n + 255) / 256), dim3(256), 0, st, d, n, patch ? 1 : 0);
}

void spin_launch_assign(const SpinDev &d, int n_scans, int scan_line, int max_n, hipStream_t st)
{
    if (max_n > 0) hipLaunchKernelGGL(spin_assign_kernel, dim3((max_n + 255) / 256, n_scans), dim3(256), 0, st, d, scan_line);
}

void spin_launch_lines(const SpinDev &d, int n_scans, int scan_line, hipStream_t st)
{
    hipLaunchKernelGGL(spin_lines_kernel, dim3(n_scans), dim3(SPIN_LT), 0, st, d, scan_line);
}

void spin_launch_curv(const SpinDev &d, int n_scans, int max_n, hipStream_t st)
{
    if (max_n > 0) hipLaunchKernelGGL(spin_curv_kernel, dim3((max_n + 255) / 256, n_scans), dim3(256), 0, st, d);
}

void spin_launch_sort(const SpinDev &d, int n_scans, int scan_line, hipStream_t st)
{
    hipLaunchKernelGGL(spin_sort_kernel, dim3(scan_line * 6, n_scans), dim3(SPIN_ST), 0, st, d, scan_line);
}

void spin_launch_select(const SpinDev &d, int n_scans, int scan_line, int n_vlines, hipStream_t st)
{
    const size_t lds = (size_t)((d.stride + 31) / 32) * sizeof(unsigned int);
    hipLaunchKernelGGL(spin_select_kernel, dim3(n_scans), dim3(64), lds, st, d, scan_line, n_vlines);
}

void spin_launch_gather(const SpinDev &d, const float4 *vout, const int *vn, int out_stride, int n_scans, int n_vlines, hipStream_t st)
{
    hipLaunchKernelGGL(spin_gather_kernel, dim3(n_scans), dim3(256), 0, st, d, vout, vn, out_stride, n_vlines);
}

}  // namespace ll
