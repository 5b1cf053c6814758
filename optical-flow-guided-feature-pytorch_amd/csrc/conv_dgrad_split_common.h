// What only the two split-fp32 data gradients of the fusion convs share (conv_dgrad_s2_split.hip: stride 2, four phases;
// conv_dgrad_split.hip: stride 1, one phase): the pre-pass that cuts g into channels-last bf16 plane images, under the name the stride-2
// file gave it, and the scratch rounding.  The cut and the MFMA are split_common.h's.  Internal linkage: one copy per translation unit.
#pragma once
#include "split_common.h"

namespace offk {
namespace {

// g (the caller's channel-sliced view, M pixels) -> three channels-last bf16 plane images [plane][M][Co]: the B operand of (pixel, 8 co)
// is one aligned 16-byte read.  One thread = eight consecutive co of one pixel, all three planes
__global__ __launch_bounds__(256) void conv_s2_gcut_split_kernel(const float* __restrict__ g, int g_cs, int g_coff, spu4* __restrict__ dst, int M,
                                                                 int Co) {
  const int c8 = Co >> 3;
  const size_t total = (size_t)M * c8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / c8;
    const int o = (int)(i - m * c8);
    const float4* s = reinterpret_cast<const float4*>(g + m * g_cs + g_coff + 8 * o);
    const float4 u0 = s[0], u1 = s[1];
    const float v[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    spu4 a, b, c;
    sp_cut8(v, a, b, c);
    dst[i] = a; dst[total + i] = b; dst[2 * total + i] = c;
  }
}

inline size_t ds_round256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
}  // namespace offk
