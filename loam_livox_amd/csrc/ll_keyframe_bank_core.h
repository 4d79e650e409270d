// ll_keyframe_bank_core.h -- the arithmetic of the key-frame descriptor bank (ll_keyframe_bank_kernels.hip), written once for the
// device and for a host compiler: tests/keyframe_bank_host.cpp runs the text below with g++.
//
// The definition is cm_kf_similarity_kernel's (ll_cellmap_kernels.hip; Maps_keyframe::max_similiarity_of_two_image, CMK:1155-1224):
//     num( Y, X ) = sum_i sum_j (double)a[i][j] * (double)b[(Y + i - 30) mod 60][(X + j - 30) mod 60]     one accumulator, i outer, j inner
//     M = max over Y, X in 0 .. 60 of num( Y, X ),   A = sum a^2,   B = sum b^2,   t = sqrt( A * B ),   result = t > 0 ? (float)( M / t ) : 0
//
// Two facts keep the bank's results equal to that kernel's to the bit.
//
// 1.  The product of two floats is exact in a double (24 + 24 significand bits <= 53), so  num + (double)a * (double)b  rounds once,
//     whether the multiply-add is fused or not: fma() below gives the bits of the unfused form the library is compiled to
//     (-ffp-contract=off).
//
// 2.  60 x 60 shifts are enough.  Shift index 60 addresses row (60 + i - 30 + 60) mod 60 = (i + 30) mod 60 for term i, and shift index 0
//     addresses (0 + i - 30 + 60) mod 60 = (i + 30) mod 60: the same row for every i, hence the same elements in the same order; the
//     same holds for the columns.  So num( 60, X ) is num( 0, X ), num( Y, 60 ) is num( Y, 0 ) and num( 60, 60 ) is num( 0, 0 ), each as
//     the same sequence of the same roundings: the 61 x 61 values are the 60 x 60 values with some of them listed twice, and a
//     maximum does not change when an element is repeated.  (No sum is NaN for finite images, and none is -0.0: an accumulator starts
//     at +0.0 and x + (-0.0) is never -0.0 for x = +0.0; so the maximum does not depend on the order it is taken in either.)
//
// The norms are NOT restated here: their summation order is the device's (a stride of 1 024 threads, a shuffle tree, sixteen
// wavefronts in sequence; kf_block_norm_partial and kf_wave_sum below, device only), and the host driver writes that order out for itself.
#pragma once
#include <math.h>

#ifndef LL_HD
#if defined(__HIPCC__)
#define LL_HD __host__ __device__ __forceinline__
#else
#define LL_HD inline
#endif
#endif

namespace ll {

#define LL_KB_RES 60                                  // LL_KF_RES
#define LL_KB_BINS (LL_KB_RES * LL_KB_RES)            // floats of one image: 14 400 bytes, a multiple of 16
#define LL_KB_ENTRY (2 * LL_KB_BINS)                  // floats of one entry: the line image, then the plane image
#define LL_KB_R 10                                    // consecutive X of one work item
#define LL_KB_TILE_X 20                               // X of one tile: two work items per Y
#define LL_KB_TILES (LL_KB_RES / LL_KB_TILE_X)        // 3
#define LL_KB_THREADS (64 * LL_KB_TILE_X / LL_KB_R)   // 128: lane = Y (60 of 64 used), wavefront = which ten X of the tile's twenty
// b's rows as a tile reads them: column c of a row holds b[row][(X0 + c - 30) mod 60], c = 0 .. 78 (X - X0 + j), so that the inner
// loop has no modulo.  79 columns; the stride is 81 floats because 81 mod 32 = 17 is odd: the lanes of a wavefront read consecutive
// rows (mod 60) at one column, and 32 consecutive rows then lie on 32 different banks of a 4-byte read.
#define LL_KB_PAD_COLS (LL_KB_TILE_X + LL_KB_RES - 1)
#define LL_KB_PAD_STRIDE 81
#define LL_KB_PAD_FLOATS (LL_KB_RES * LL_KB_PAD_STRIDE)

// the wrap-padded rows of tile `tile` from b's image; element e of the image goes to one or two columns of its row
LL_HD void kb_pad_element(const float v, int e, int tile, float *pad)
{
    const int row = e / LL_KB_RES, x = e % LL_KB_RES;
    int c = x - tile * LL_KB_TILE_X + LL_KB_RES / 2;  // (X0 + c - 30) mod 60 == x
    if (c < 0) c += LL_KB_RES;
    if (c >= LL_KB_RES) c -= LL_KB_RES;
    pad[row * LL_KB_PAD_STRIDE + c] = v;
    if (c + LL_KB_RES < LL_KB_PAD_COLS) pad[row * LL_KB_PAD_STRIDE + c + LL_KB_RES] = v;
}

// One work item: the LL_KB_R sums num( Y, X0 + x0 .. X0 + x0 + R - 1 ) of a tile, X0 the tile's first X and x0 = 0 or 10.
// a: the image [60][60]; pad: the tile's wrap-padded rows of b.  One accumulator per shift, i outer, j inner, in sequence; a window
// of b's row slides through registers, so a step costs one new element of b and R multiply-adds; a[i][j] is the same for every item.
// On the device the row loop stays a loop and the column loop is unrolled by two chunks of R: half the window's moves become register
// names (measured: 6 % faster than no unrolling; unrolling it fully costs more registers than it saves moves).
LL_HD void kb_item(const float *a, const float *pad, int Y, int x0, double acc[LL_KB_R])
{
    for (int r = 0; r < LL_KB_R; r++) acc[r] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int i = 0; i < LL_KB_RES; i++) {
        int bi = Y + i - LL_KB_RES / 2;
        if (bi < 0) bi += LL_KB_RES;
        if (bi >= LL_KB_RES) bi -= LL_KB_RES;
        const float *rb = pad + bi * LL_KB_PAD_STRIDE + x0;
        const float *ra = a + i * LL_KB_RES;
        double w[2 * LL_KB_R - 1];
        for (int k = 0; k < LL_KB_R - 1; k++) w[k] = (double)rb[k];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 2
#endif
        for (int j0 = 0; j0 < LL_KB_RES; j0 += LL_KB_R) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < LL_KB_R; k++) w[LL_KB_R - 1 + k] = (double)rb[j0 + LL_KB_R - 1 + k];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int jj = 0; jj < LL_KB_R; jj++) {
                const double av = (double)ra[j0 + jj];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
                for (int r = 0; r < LL_KB_R; r++) acc[r] = fma(av, w[jj + r], acc[r]);
            }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int k = 0; k < LL_KB_R - 1; k++) w[k] = w[k + LL_KB_R];
        }
    }
}

// work item t of a tile (t < LL_KB_THREADS as lane + 64 * wavefront, lanes 60 .. 63 idle): its Y and its first X within the tile
LL_HD int kb_item_y(int t) { return t & 63; }
LL_HD int kb_item_x0(int t) { return (t >> 6) * LL_KB_R; }

// cm_kf_similarity_kernel's last line
LL_HD float kb_quotient(double A, double B, double M)
{
    const double t = sqrt(A * B);
    return t > 0.0 ? (float)(M / t) : 0.0f;
}

#if defined(__HIPCC__)
// cm_kf_similarity_kernel's norm of one image, in its own order, by a workgroup of 1 024 threads: the thread-strided partial sum and
// the shuffle tree within a wavefront; the caller then adds wavefronts 0 .. 15 in sequence, starting from 0.0.
__device__ inline double kf_block_norm_partial(const float *img, int tid)
{
    double n = 0.0;
    for (int e = tid; e < LL_KB_BINS; e += 1024) n += (double)img[e] * (double)img[e];
    return n;
}
__device__ inline double kf_wave_sum(double x)
{
    for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off);
    return x;
}
#endif

}  // namespace ll
