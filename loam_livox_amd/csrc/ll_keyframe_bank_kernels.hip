// ll_keyframe_bank_kernels.hip -- the key-frame descriptor bank's three kernels: the correlation of (new key frame, old key frame)
// pairs over all circular shifts, the finish (maximum over tiles, quotient, cast), and the norms of an entry.  The arithmetic is
// ll_keyframe_bank_core.h's; the results are cm_kf_similarity_kernel's bit for bit.  No atomics, no spin-waits, no scratch.
#include <hip/hip_runtime.h>

#include "ll_keyframe_bank.h"
#include "ll_keyframe_bank_core.h"

namespace ll {

#define KB_THREADS LL_KB_THREADS  // two wavefronts: lane = Y (60 of 64 used), wavefront = which ten X of the tile's twenty

// One workgroup per (tile of 60 Y x 20 X shifts, kind, pair); workgroups do not communicate.  a's image and the tile's wrap-padded
// rows of b's are staged in LDS (33 840 bytes) from 16-byte loads; then kb_item.  SURFACE: every sum of ONE pair and kind is
// written to surface[Y * 60 + X] instead of the tile's maximum (the test tap).
template <bool SURFACE>
__global__ __launch_bounds__(KB_THREADS) void kb_corr_kernel(const float *__restrict__ img, const int2 *__restrict__ pairs, int kind_only,
                                                             double *__restrict__ partial, double *__restrict__ surface)
{
    __shared__ __attribute__((aligned(16))) float s_a[LL_KB_BINS];
    __shared__ float s_pad[LL_KB_PAD_FLOATS];
    __shared__ double s_best[KB_THREADS / 64];
    const int tid = threadIdx.x;
    const int tile = blockIdx.x % LL_KB_TILES;
    const int kind = SURFACE ? kind_only : (blockIdx.x / LL_KB_TILES) % 2;
    const int pair = SURFACE ? 0 : blockIdx.x / (2 * LL_KB_TILES);
    const int2 ab = pairs[pair];
    const float4 *ga = (const float4 *)(img + (size_t)ab.x * LL_KB_ENTRY + (size_t)kind * LL_KB_BINS);
    const float4 *gb = (const float4 *)(img + (size_t)ab.y * LL_KB_ENTRY + (size_t)kind * LL_KB_BINS);
    for (int q = tid; q < LL_KB_BINS / 4; q += KB_THREADS) {
        const float4 va = ga[q], vb = gb[q];
        ((float4 *)s_a)[q] = va;
        kb_pad_element(vb.x, 4 * q + 0, tile, s_pad);
        kb_pad_element(vb.y, 4 * q + 1, tile, s_pad);
        kb_pad_element(vb.z, 4 * q + 2, tile, s_pad);
        kb_pad_element(vb.w, 4 * q + 3, tile, s_pad);
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6;
    double best = -1.0e300;
    if (lane < LL_KB_RES) {
        double acc[LL_KB_R];
        const int Y = kb_item_y(tid), x0 = kb_item_x0(tid);
        kb_item(s_a, s_pad, Y, x0, acc);
#pragma unroll
        for (int r = 0; r < LL_KB_R; r++) {
            if (SURFACE) surface[Y * LL_KB_RES + tile * LL_KB_TILE_X + x0 + r] = acc[r];
            best = acc[r] > best ? acc[r] : best;
        }
    }
    if (SURFACE) return;
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_down(best, off);
        best = o > best ? o : best;
    }
    if (lane == 0) s_best[wave] = best;
    __syncthreads();
    if (tid == 0) {
        double m = s_best[0];
        for (int w = 1; w < KB_THREADS / 64; w++) m = s_best[w] > m ? s_best[w] : m;
        partial[blockIdx.x] = m;  // [pair][kind][tile]
    }
}

// one thread per (pair, kind): sim[kind * n_pairs + pair]
__global__ __launch_bounds__(256) void kb_finish_kernel(const int2 *__restrict__ pairs, int n_pairs, const double *__restrict__ partial,
                                                        const double *__restrict__ norm, float *__restrict__ sim)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= 2 * n_pairs) return;
    const int pair = t >> 1, kind = t & 1;
    const double *p = partial + (size_t)t * LL_KB_TILES;
    double M = p[0];
    for (int k = 1; k < LL_KB_TILES; k++) M = p[k] > M ? p[k] : M;
    const int2 ab = pairs[pair];
    sim[(size_t)kind * n_pairs + pair] = kb_quotient(norm[2 * (size_t)ab.x + kind], norm[2 * (size_t)ab.y + kind], M);
}

// the norms of one entry: block 0 the line image, block 1 the plane image, in cm_kf_similarity_kernel's order
__global__ __launch_bounds__(1024) void kb_norm_kernel(const float *__restrict__ entry, double *__restrict__ norm2)
{
    __shared__ double s_w[1024 / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double n = kf_wave_sum(kf_block_norm_partial(entry + (size_t)blockIdx.x * LL_KB_BINS, tid));
    if (lane == 0) s_w[wave] = n;
    __syncthreads();
    if (tid == 0) {
        double A = 0.0;
        for (int w = 0; w < 1024 / 64; w++) A += s_w[w];
        norm2[blockIdx.x] = A;
    }
}

#define KBCHK(call)                       \
    do {                                  \
        hipError_t e_ = (call);           \
        if (e_ != hipSuccess) {           \
            *err = hipGetErrorString(e_); \
            return -1;                    \
        }                                 \
    } while (0)

int keyframe_bank_norms(const float *d_entry, double *d_norm2, hipStream_t s, const char **err)
{
    hipLaunchKernelGGL(kb_norm_kernel, dim3(2), dim3(1024), 0, s, d_entry, d_norm2);
    KBCHK(hipGetLastError());
    return 0;
}

int keyframe_bank_match(const float *d_img, const double *d_norm, const int2 *d_pairs, int n_pairs, double *d_partial, float *d_sim,
                        hipStream_t s, const char **err)
{
    hipLaunchKernelGGL(kb_corr_kernel<false>, dim3((unsigned)n_pairs * 2 * LL_KB_TILES), dim3(KB_THREADS), 0, s, d_img, d_pairs, 0, d_partial,
                       (double *)nullptr);
    hipLaunchKernelGGL(kb_finish_kernel, dim3((2 * n_pairs + 255) / 256), dim3(256), 0, s, d_pairs, n_pairs, d_partial, d_norm, d_sim);
    KBCHK(hipGetLastError());
    return 0;
}

int keyframe_bank_surface(const float *d_img, const int2 *d_pair, int kind, double *d_surface, hipStream_t s, const char **err)
{
    hipLaunchKernelGGL(kb_corr_kernel<true>, dim3(LL_KB_TILES), dim3(KB_THREADS), 0, s, d_img, d_pair, kind, (double *)nullptr, d_surface);
    KBCHK(hipGetLastError());
    return 0;
}

}  // namespace ll
