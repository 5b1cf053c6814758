// The fused units kernel of split-fp32 handles for channels-last feature maps (ABI v10, additive: offk_forward_cl and its siblings).
// Every map (part) is physically [B * L * HW][c_part], elements fp32 / bf16 / fp16.  The block body -- arithmetic, geometry, LDS
// stages, epilogue -- is pw_tdiff_staged.h's; this file is its loader for channels-last maps.
//
// An item is (frame, pixel, k group) -- 896 per K-tile, two per thread: the eight k of a lane's B operand are 16 (16-bit maps) or 32
// (fp32) contiguous bytes of the map, fetched with one or two 16-byte loads; the four lanes of a pixel cover one 64- / 128-byte line.
// bf16 goes to LDS as loaded, fp16 is widened and cut into two planes, fp32 into three.  All sites take this one form (no pixel
// pairs, no 2-byte loads for the odd-HW 7x7 sites).
// LDS writes: a 16-byte ds_write is banked per eight contiguous lanes over 128 B, and eight loader lanes are two pixels x four k groups,
// whose entries [g][pixel] x 16 B would all fall on two 16-byte slots (4-way).  So the entry of (k group g, pixel p) sits at pixel slot
// p ^ g, and the loader's lane -> pixel map swaps pixel bits 0 and 2: the eight lanes then hold pixels p, p + 4 and write the eight
// slots {p .. p + 3} ^ g, {p + 4 .. p + 7} ^ g -- conflict-free.  The XOR touches slot bits 0 - 1 only, which keeps every 16-lane group
// of the MFMA side's ds_read_b128 ({0-3, 12-15} of one k group, {4-11} of the next) on sixteen distinct slots.
#include "pw_tdiff_staged.h"

namespace offk {

namespace {
using namespace staged;

// FEAT: kFeatF32 (three planes), kFeatBf16 (one), kFeatF16 (two)
template <int FEAT>
struct ClLoader {
  static constexpr int NPL = FEAT == kFeatF32 ? 3 : FEAT == kFeatF16 ? 2 : 1;
  static constexpr int ES = FEAT == kFeatF32 ? 4 : 2;                      // bytes per map element
  static constexpr int NLD = FEAT == kFeatF32 ? 2 : 1;                     // 16-byte loads per item
  static constexpr int kItems = kFrames * kPixels * 4;                     // (frame, pixel, k group): 896

  int it_dst[2];                                             // byte offset of the item's plane 0 entry in a stage's map area
  size_t it_row[2];                                          // (clip frame b L + t0 + f) HW + pixel: the item's row of the map
  int it_g8[2];
  bool it_ok[2];
  int tid;
  spu4 mv[2][NLD];

  // the four lanes of a pixel take its four k groups (one line of the map); pixel bits 0 and 2 swapped against the lane order
  __device__ __forceinline__ ClLoader(const PtSite&, const BlockGeom& b) : tid(b.tid) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int item = b.tid + r * kThreads;
      const int g = item & 3, q = (item >> 2) & 31, f = item >> 7;
      const int pp = (q & ~5) | ((q & 1) << 2) | ((q >> 2) & 1);
      const int gp = b.px0 + pp;
      const bool ok = item < kItems && f < b.nf && gp < b.npx;
      const int clip = ok ? gp / b.HW : 0;
      it_ok[r] = ok; it_g8[r] = 8 * g;
      it_row[r] = ok ? (size_t)(clip * b.L + b.t0 + f) * b.HW + (gp - clip * b.HW) : 0;
      it_dst[r] = (f * 2 + (pp >> 4)) * NPL * kPlane + g * 256 + (((pp & 15) ^ g) << 4);
    }
  }

  __device__ __forceinline__ void load(const PtSite& S, int kt) {
    const PartK k = part_of_ktile(S, kt);
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (it_ok[r]) {
        const spu4* src = reinterpret_cast<const spu4*>(reinterpret_cast<const char*>(k.xb) + (it_row[r] * k.cpart + k.kl + it_g8[r]) * ES);
#pragma unroll
        for (int n = 0; n < NLD; ++n) mv[r][n] = src[n];
      } else {
#pragma unroll
        for (int n = 0; n < NLD; ++n) mv[r][n] = spu4{0u, 0u, 0u, 0u};
      }
    }
  }

  __device__ __forceinline__ void store(char* xs) const {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (tid + r * kThreads >= kItems) continue;
      char* const dst = xs + it_dst[r];
      if constexpr (FEAT == kFeatBf16) {
        *reinterpret_cast<spu4*>(dst) = mv[r][0];
      } else if constexpr (FEAT == kFeatF16) {
        unsigned v[8];                                       // element e in the e & 1 half of word e >> 1
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (e & 1) ? mv[r][0][e >> 1] >> 16 : mv[r][0][e >> 1] & 0xffffu;
        spu4 ph, pm;
        cut2(v, ph, pm);
        *reinterpret_cast<spu4*>(dst) = ph;
        *reinterpret_cast<spu4*>(dst + kPlane) = pm;
      } else {
        const unsigned v[8] = {mv[r][0].x, mv[r][0].y, mv[r][0].z, mv[r][0].w, mv[r][NLD - 1].x, mv[r][NLD - 1].y, mv[r][NLD - 1].z, mv[r][NLD - 1].w};
        spu4 ph, pm, pl;
        cut3(v, ph, pm, pl);
        *reinterpret_cast<spu4*>(dst) = ph;
        *reinterpret_cast<spu4*>(dst + kPlane) = pm;
        *reinterpret_cast<spu4*>(dst + 2 * kPlane) = pl;
      }
    }
  }

  static __device__ __forceinline__ int slot(int li, int lg) { return li ^ lg; }
};
}  // namespace

template <int FEAT>
__global__ __launch_bounds__(kThreads, 1) void pw_tdiff_cl_kernel(PtParams p) {
  units_block<ClLoader<FEAT>::NPL, ClLoader<FEAT>>(p);
}

// xp[]: channels-last parts of feat_dtype elements
hipError_t pw_tdiff_cl_launch(const PtParams& p, int feat_dtype, hipStream_t st) {
  if (feat_dtype == kFeatF16) return launch<2>(pw_tdiff_cl_kernel<kFeatF16>, p, st);
  if (feat_dtype == kFeatBf16) return launch<1>(pw_tdiff_cl_kernel<kFeatBf16>, p, st);
  return launch<3>(pw_tdiff_cl_kernel<kFeatF32>, p, st);
}

}  // namespace offk
