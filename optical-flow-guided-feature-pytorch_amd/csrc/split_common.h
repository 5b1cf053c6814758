// The device side of split-fp32 arithmetic on the bf16 matrix pipe, defined once (the CPU model is synth.py; every error bound of
// include/offk.h rests on these): the truncating three-plane cut, the pack of two planes' words into one MFMA operand word, the
// v_mfma_f32_16x16x32_bf16 wrapper, the store of four k of a row into plane images and the six-product issue block.  Everything here has
// internal linkage and is inlined: each translation unit gets its own copy.  A new split kernel includes this header.
#pragma once
#include "offk_common.h"

namespace offk {
namespace {

typedef float spf4 __attribute__((ext_vector_type(4)));
typedef unsigned spu4 __attribute__((ext_vector_type(4)));
typedef unsigned spu2 __attribute__((ext_vector_type(2)));

// the truncating three-plane cut (synth.cut3): h, m in the upper 16 bits of the returned words, l's plane is the upper 16 bits of its word
__device__ __forceinline__ void sp_cut(float x, unsigned& h, unsigned& m, unsigned& l) {
  h = __float_as_uint(x) & 0xFFFF0000u;
  const float r = x - __uint_as_float(h);
  m = __float_as_uint(r) & 0xFFFF0000u;
  l = __float_as_uint(r - __uint_as_float(m));
}
// the upper halves of two words as one: `lo` in bits 0..15 (the lower k)
__device__ __forceinline__ unsigned sp_pair(unsigned lo, unsigned hi) { return __builtin_amdgcn_perm(hi, lo, 0x07060302); }

__device__ __forceinline__ void sp_mfma(spf4& c, const spu4& a, const spu4& b) {
  c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// eight consecutive k of one row -> one 16-byte MFMA operand per plane
__device__ __forceinline__ void sp_cut8(const float (&v)[8], spu4& ph, spu4& pm, spu4& pl) {
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sp_cut(v[e], h[e], m[e], l[e]);
  ph = spu4{sp_pair(h[0], h[1]), sp_pair(h[2], h[3]), sp_pair(h[4], h[5]), sp_pair(h[6], h[7])};
  pm = spu4{sp_pair(m[0], m[1]), sp_pair(m[2], m[3]), sp_pair(m[4], m[5]), sp_pair(m[6], m[7])};
  pl = spu4{sp_pair(l[0], l[1]), sp_pair(l[2], l[3]), sp_pair(l[4], l[5]), sp_pair(l[6], l[7])};
}

// four consecutive k of one row, already cut (h, m, l point at the first of the four) -> 8 bytes in each of the first NPL plane images
template <int NPL>
__device__ __forceinline__ void sp_store_quad(char* dst, int plane_bytes, const unsigned* h, const unsigned* m, const unsigned* l) {
  *reinterpret_cast<spu2*>(dst) = spu2{sp_pair(h[0], h[1]), sp_pair(h[2], h[3])};
  if constexpr (NPL > 1) *reinterpret_cast<spu2*>(dst + plane_bytes) = spu2{sp_pair(m[0], m[1]), sp_pair(m[2], m[3])};
  if constexpr (NPL > 2) *reinterpret_cast<spu2*>(dst + 2 * plane_bytes) = spu2{sp_pair(l[0], l[1]), sp_pair(l[2], l[3])};
}
// the same from the four values
template <int NPL>
__device__ __forceinline__ void sp_store_quad(char* dst, int plane_bytes, float v0, float v1, float v2, float v3) {
  unsigned h[4], m[4], l[4];
  sp_cut(v0, h[0], m[0], l[0]); sp_cut(v1, h[1], m[1], l[1]); sp_cut(v2, h[2], m[2], l[2]); sp_cut(v3, h[3], m[3], l[3]);
  sp_store_quad<NPL>(dst, plane_bytes, h, m, l);
}

// One 32-k step of an MT x NT block of 16 x 16 tiles, w[mt][plane] against x[nt][plane] (plane 0 = h, 1 = m, 2 = l): six of the nine plane
// products in synth.SPLIT_PRODUCTS order (w plane, x plane) -- (2, 0), (0, 2), (1, 1), (1, 0), (0, 1) into A2, then (0, 0) into A1 --
// product-major over the tiles.  This is the order of synth.emulate_split_dot(form="units"); the caller adds A1 + A2 once, behind its K loop.
template <int MT, int NT>
__device__ __forceinline__ void sp_issue6(spf4 (&a1)[MT][NT], spf4 (&a2)[MT][NT], const spu4 (&w)[MT][3], const spu4 (&x)[NT][3]) {
  constexpr int WP[6] = {2, 0, 1, 1, 0, 0}, XP[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
  for (int p = 0; p < 6; ++p)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) sp_mfma(p < 5 ? a2[mt][nt] : a1[mt][nt], w[mt][WP[p]], x[nt][XP[p]]);
}

// The bias partial of the conv weight gradients: every g loader thread holds the fp32 sum `bs` of its position quad pq (0 .. 7) for the
// four channels 4 cq .. + 3; the eight quads of a channel go through LDS (red: [8 quads][64 channels]) and threads 0 .. 63 sum them in
// quad order into db[at + channel].  The caller has a barrier between the last reader of `red`'s memory and this.
__device__ __forceinline__ void sp_db_quads(float* red, bool is_g, int pq, int cq, const float4& bs, int tid, float* db, size_t at) {
  if (is_g) {
    red[pq * 64 + 4 * cq] = bs.x; red[pq * 64 + 4 * cq + 1] = bs.y; red[pq * 64 + 4 * cq + 2] = bs.z; red[pq * 64 + 4 * cq + 3] = bs.w;
  }
  __syncthreads();
  if (tid < 64) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) s += red[i * 64 + tid];
    db[at + tid] = s;
  }
}

}  // namespace
}  // namespace offk
