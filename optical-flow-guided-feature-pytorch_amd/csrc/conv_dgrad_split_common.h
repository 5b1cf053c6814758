// What the two split-fp32 data gradients of the fusion convs share (conv_dgrad_s2_split.hip: stride 2, four phases; conv_dgrad_split.hip:
// stride 1, one phase): the truncating three-plane cut of eight values into MFMA operand pieces, the pre-pass that cuts g into
// channels-last bf16 plane images, and the MFMA.  Everything here has internal linkage: each translation unit gets its own copy, under
// the names the stride-2 file gave them.
#pragma once
#include "offk_common.h"

namespace offk {
namespace {

typedef float dsf4 __attribute__((ext_vector_type(4)));
typedef unsigned dsu4 __attribute__((ext_vector_type(4)));

// the truncating three-plane cut (synth.cut3): h, m in the upper 16 bits of the returned words, l's plane is the upper 16 bits of its word
__device__ __forceinline__ void ds_cut(float x, unsigned& h, unsigned& m, unsigned& l) {
  h = __float_as_uint(x) & 0xFFFF0000u;
  const float r = x - __uint_as_float(h);
  m = __float_as_uint(r) & 0xFFFF0000u;
  l = __float_as_uint(r - __uint_as_float(m));
}
// the upper halves of two words as one: `lo` in bits 0..15 (the lower k)
__device__ __forceinline__ unsigned ds_pair(unsigned lo, unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302); }

__device__ __forceinline__ void ds_cut8(const float (&v)[8], dsu4& ph, dsu4& pm, dsu4& pl) {
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) ds_cut(v[e], h[e], m[e], l[e]);
  ph = dsu4{ds_pair(h[0], h[1]), ds_pair(h[2], h[3]), ds_pair(h[4], h[5]), ds_pair(h[6], h[7])};
  pm = dsu4{ds_pair(m[0], m[1]), ds_pair(m[2], m[3]), ds_pair(m[4], m[5]), ds_pair(m[6], m[7])};
  pl = dsu4{ds_pair(l[0], l[1]), ds_pair(l[2], l[3]), ds_pair(l[4], l[5]), ds_pair(l[6], l[7])};
}

// g (the caller's channel-sliced view, M pixels) -> three channels-last bf16 plane images [plane][M][Co]: the B operand of (pixel, 8 co)
// is one aligned 16-byte read.  One thread = eight consecutive co of one pixel, all three planes
__global__ __launch_bounds__(256) void conv_s2_gcut_split_kernel(const float* __restrict__ g, int g_cs, int g_coff, dsu4* __restrict__ dst, int M,
                                                                 int Co) {
  const int c8 = Co >> 3;
  const size_t total = (size_t)M * c8;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t m = i / c8;
    const int o = (int)(i - m * c8);
    const float4* s = reinterpret_cast<const float4*>(g + m * g_cs + g_coff + 8 * o);
    const float4 u0 = s[0], u1 = s[1];
    const float v[8] = {u0.x, u0.y, u0.z, u0.w, u1.x, u1.y, u1.z, u1.w};
    dsu4 a, b, c;
    ds_cut8(v, a, b, c);
    dst[i] = a; dst[total + i] = b; dst[2 * total + i] = c;
  }
}

__device__ __forceinline__ void ds_mfma(dsf4& c, const dsu4& a, const dsu4& b) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

inline size_t ds_round256(size_t b) { return (b + 255) & ~(size_t)255; }

}  // namespace
}  // namespace offk
