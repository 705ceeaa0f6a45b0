// The sort keys of [~, indx] = sort(abs(vec(S)), 'descend') (plot_errorVSsnr.m:143), ONE expression for the trial builder's
// indx_S (csrc/inputgen.hip) and jstsp_support_order_c32 / _f64 (csrc/support.hip): the key of an entry is ~bits(|z|^2), so that
// an ASCENDING unsigned key is a DESCENDING magnitude (|z|^2 >= +0 or NaN: the bit pattern of a non-negative float orders as its
// value).  A NaN takes key 0 whatever its sign and payload: every NaN ties with every other and sorts before +Inf (key
// ~bits(+Inf) > 0), as MATLAB's descending sort places them.  Ties are broken by the index the caller puts below the key.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace {

// |z|^2 = x*x + y*y in fp32
__device__ __forceinline__ uint32_t support_key(float2 z)
{
    const float m2 = z.x * z.x + z.y * z.y;
    return m2 != m2 ? 0u : ~__float_as_uint(m2);
}

// |z|^2 = x*x + y*y in float64
__device__ __forceinline__ uint64_t support_key(double2 z)
{
    const double m2 = z.x * z.x + z.y * z.y;
    return m2 != m2 ? 0ull : ~(uint64_t)__double_as_longlong(m2);
}

}  // namespace
