// ll_ordered_float.h -- floats as unsigned integers that compare the way the floats do, so that a minimum or a maximum over
// floats can be an integer atomic, whose result does not depend on the order (ll_voxel_kernels.hip, ll_map_refine_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ll {

__device__ __forceinline__ unsigned int f2ord(float f)
{
    const unsigned int b = (unsigned int)__float_as_int(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ord2f(unsigned int o)
{
    const unsigned int b = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __int_as_float((int)b);
}

}  // namespace ll
