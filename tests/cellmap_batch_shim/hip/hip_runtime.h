#pragma once
// Test-only stand-in for <hip/hip_runtime.h> (tests/cellmap_batch_kernels_host.cpp): just enough to compile
// loam_livox_amd/csrc/ll_cellmap_batch_kernels.hip with g++ and run its launch chains on the CPU.  A launch runs the kernel once per
// thread of the grid, one after the other, the threads of a block in DESCENDING order -- any fixed order is one legal schedule of
// kernels whose threads do not wait for each other, and this one is not the order a sequential restatement would take.
#include <string.h>
#include <stdint.h>
#include <algorithm>
#include <vector>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
struct float4 { float x, y, z, w; };
static inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
static dim3 blockIdx, threadIdx, gridDim, blockDim;
typedef int hipError_t;
typedef void *hipStream_t;
#define hipSuccess 0
static inline const char *hipGetErrorString(int) { return "err"; }
static inline int hipGetLastError() { return 0; }
static inline int hipMemsetAsync(void *p, int v, size_t n, hipStream_t) { memset(p, v, n); return 0; }
static inline int atomicExch(int *p, int v) { int o = *p; *p = v; return o; }
#define hipLaunchKernelGGL(k, g, b, sh, st, ...)                                  \
    do {                                                                            \
        dim3 g_ = (g), b_ = (b);                                                    \
        gridDim = g_; blockDim = b_;                                                \
        for (unsigned bz = 0; bz < g_.z; bz++) for (unsigned by = 0; by < g_.y; by++) for (unsigned bx = 0; bx < g_.x; bx++) \
            for (int tx = (int)b_.x - 1; tx >= 0; tx--) { /* reverse thread order: not the sequential order */ \
                blockIdx = dim3(bx, by, bz); threadIdx = dim3((unsigned)tx, 0, 0);  \
                k(__VA_ARGS__);                                                     \
            }                                                                       \
    } while (0)
