// The fused units kernel of split-fp32 handles for 16-bit NCHW feature maps (ABI v10, additive: offk_forward_typed and its siblings).
// The block body -- arithmetic, geometry, LDS stages, epilogue -- is pw_tdiff_staged.h's; this file is its loader for NCHW maps of
// bf16 (one plane) or fp16 (two planes) elements.
//
// A thread gathers eight k rows of one pixel pair (two pixels of a 4-byte load; the 7x7 sites, whose HW is odd, one pixel of a 2-byte
// load), cuts fp16 into (x_h, x_m) in registers and writes 16 B per plane and pixel, pixel p of a tile at pixel slot p.  An item is
// (frame, k group, pixel pair) -- 448, one per thread -- or (frame, k group, pixel) for odd HW -- 896, two per thread; lanes of one
// (frame, k group) take consecutive pixels.
#include "pw_tdiff_staged.h"

namespace offk {

namespace {
using namespace staged;

// F16: fp16 maps (two planes), else bf16 (one)
template <bool F16>
struct Feat16Loader {
  static constexpr int NPL = F16 ? 2 : 1;

  bool pairs;                                                // 28x28, 14x14 (even HW): a pixel pair never straddles two clips
  int HW, tid;
  int it_f[2], it_g[2], it_p[2], it_fr[2], it_px[2];         // (frame, k group, first pixel of the tile), (clip frame b L + t0 + f, pixel)
  bool it_ok[2];
  unsigned mv[2][8];                                         // pairs: 4-byte loads (two pixels); else 2-byte loads (one pixel)

  __device__ __forceinline__ Feat16Loader(const PtSite&, const BlockGeom& b) : pairs((b.HW & 1) == 0), HW(b.HW), tid(b.tid) {
    const int nit = pairs ? 1 : 2;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int item = tid + r * kThreads;
      int f, g, pp;
      if (pairs) { f = item >> 6; g = (item >> 4) & 3; pp = 2 * (item & 15); }
      else { f = item >> 7; g = (item >> 5) & 3; pp = item & 31; }
      const int gp = b.px0 + pp;
      const bool ok = r < nit && f < b.nf && gp < b.npx;
      const int clip = ok ? gp / HW : 0;
      it_f[r] = f; it_g[r] = g; it_p[r] = pp; it_ok[r] = ok;
      it_fr[r] = clip * b.L + b.t0 + f; it_px[r] = ok ? gp - clip * HW : 0;
    }
  }

  __device__ __forceinline__ void load(const PtSite& S, int kt) {
    const PartK k = part_of_ktile(S, kt);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (it_ok[r]) {
        const unsigned short* src = reinterpret_cast<const unsigned short*>(k.xb) + ((size_t)it_fr[r] * k.cpart + k.kl + 8 * it_g[r]) * HW + it_px[r];
        // (r == 0: a second item exists for odd HW only -- it_ok[1] implies !pairs, which the compiler does not derive from the
        // members; left to it, the step carries eight more 4-byte loads that never run)
        if (r == 0 && pairs) {
#pragma unroll
          for (int e = 0; e < 8; ++e) mv[r][e] = *reinterpret_cast<const unsigned*>(src + (size_t)e * HW);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) mv[r][e] = src[(size_t)e * HW];
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) mv[r][e] = 0u;
      }
    }
  }

  // bf16 as it is, fp16 cut into two planes
  __device__ __forceinline__ void store(char* xs) const {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int item = tid + r * kThreads;
      if (item >= (pairs ? 448 : 896)) continue;
      const int f = it_f[r], g = it_g[r], pp = it_p[r];
      unsigned v0[8], v1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { v0[e] = mv[r][e] & 0xffffu; v1[e] = mv[r][e] >> 16; }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 1 && !pairs) break;
        const int px = pp + s;
        const unsigned (&v)[8] = s == 0 ? v0 : v1;
        char* dst = xs + (f * 2 + (px >> 4)) * NPL * kPlane + g * 256 + (px & 15) * 16;
        if constexpr (F16) {
          spu4 ph, pm;
          cut2(v, ph, pm);
          *reinterpret_cast<spu4*>(dst) = ph;
          *reinterpret_cast<spu4*>(dst + kPlane) = pm;
        } else {
          *reinterpret_cast<spu4*>(dst) = spu4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
        }
      }
    }
  }

  static __device__ __forceinline__ int slot(int li, int) { return li; }
};
}  // namespace

template <bool F16>
__global__ __launch_bounds__(kThreads, 1) void pw_tdiff_feat16_kernel(PtParams p) {
  units_block<Feat16Loader<F16>::NPL, Feat16Loader<F16>>(p);
}

// xp[]: NCHW parts of 16-bit elements
hipError_t pw_tdiff_feat16_launch(const PtParams& p, int feat_dtype, hipStream_t st) {
  if (feat_dtype == kFeatF16) return launch<2>(pw_tdiff_feat16_kernel<true>, p, st);
  return launch<1>(pw_tdiff_feat16_kernel<false>, p, st);
}

}  // namespace offk
