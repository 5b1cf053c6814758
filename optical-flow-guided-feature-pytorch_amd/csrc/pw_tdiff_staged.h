// The block body shared by the fused units kernels of split-fp32 handles that stage their feature maps through registers into LDS:
// pw_tdiff_feat16_kernel (16-bit NCHW maps, pw_tdiff_f16.hip) and pw_tdiff_cl_kernel (channels-last maps, pw_tdiff_cl.hip).  Both
// write what pw_tdiff_split_kernel writes -- T into fusion_<28|14|7>, D_<site> -- and the S-blocks launch runs after them unchanged.
// A kernel is this body plus a Loader (below): how a thread fetches the eight k of a pixel and where their plane entries go.
//
// Arithmetic: equal values, not a new tolerance.  pw_tdiff_split_kernel cuts a map value x into three bf16 planes (h = the upper 16
// bits, m = the upper 16 bits of x - h, l = x - h - m) and issues per output tile and 32-k group, into A2: w_l x_h, w_h x_l, w_m x_m,
// w_m x_h, w_h x_m, then into A1: w_h x_h.  A bf16 map value is exactly its own leading plane (x_m = x_l = +0); an fp16 value has 11
// significant bits, so it is exactly two bf16 planes (x_l = +0; an fp16 subnormal is a normal number in fp32 and bf16).  The products
// of a +0 plane are all +-0 and may be left out: with NPL = 1 (bf16) the body issues w_l x_h, w_m x_h | w_h x_h (3 MFMAs), with
// NPL = 2 (fp16) w_l x_h, w_m x_m, w_m x_h, w_h x_m | w_h x_h (5), with NPL = 3 (fp32) all six -- the same k (K-tile kt, lane group g,
// element e <-> channel 32 kt + 8 g + e of the part that holds it) in the same operand slots, in the same order, into the same two
// accumulators, from the same weight plane image (pw_pack_split16_kernel), and ends in the same epilogue.  So for finite maps it
// returns pw_tdiff_split_kernel's values on the fp32 NCHW copy of the same logical tensor (tests/test_gpu_feat16.py,
// tests/test_gpu_feat_cl.py: torch.equal).
//
// Geometry.  One block = 512 threads = eight waves = (site, temporal group, 32 pixels of the site's stream of B * HW (clip, pixel)
// pairs) x seven frames x 160 channels; waves w and w + 4 take pixel tiles 0 and 1 with the channel work of pw_tdiff_split_kernel's
// wave w & 3 (gen channels 32 (w & 3) .. + 31 in two 16-channel tiles, down tile w & 1 of frames ((w & 3) >> 1) + 2 i).  A pixel's
// result does not depend on the other columns of its MFMA, so the stream order (which packs the 7x7 and 14x14 leftovers without a
// layout of their own) changes no value.  Per K-tile the block stages in LDS
//   * the K-tile's weight plane image, 30 KB, copied as it lies ([slab 5][ct 2][plane 3][lane 64] x 16 B): the eight waves read it with
//     conflict-free ds_read_b128, so each weight byte crosses the L1 once per 32 pixels (pw_tdiff_split_kernel: every wave loads its
//     own slab straight into registers, once per 16 pixels -- 5.2 of the 7.2 GB its launch pulls through the L1s);
//   * the maps as plane images [frame 7][pixel tile 2][plane NPL][k group 4][pixel slot 16] x 16 B (8 bf16 = k 8g .. 8g + 7), the B
//     operand of the fp32 kernel's layout; the Loader writes them and names the slot a pixel's entry sits in;
// double-buffered through registers (the loads of K-tile k + 1 are in flight during the gen MFMAs of K-tile k and go to LDS between
// its gen and down MFMAs), one barrier per K-tile.
// LDS: 2 x (30 KB + 7 x 2 x NPL KB) = 88 | 116 | 144 KB: one block (eight waves) per CU.  Compiler-scheduled: no counted waits.
#pragma once
#include "units_common.h"
#include "split_common.h"

namespace offk {
namespace staged {

constexpr int kFrames = 7;                       // frames per block (as pw_tdiff_split_kernel: temporal groups of pt_tgroups)
constexpr int kPixels = 32;                      // pixels per block: two MFMA pixel tiles
constexpr int kThreads = 512;
constexpr int kWImg = 5 * 2 * 3 * 1024;          // one K-tile of the weight plane image: 30 KB
constexpr int kWChunks = kWImg / 16;             // 1920 16-byte pieces
constexpr int kPlane = 1024;                     // [k group 4][pixel slot 16] x 16 B

template <int NPL>
struct Lds {
  static constexpr int kXFrame = 2 * NPL * kPlane;              // both pixel tiles of one frame
  static constexpr int kXStage = kFrames * kXFrame;
  static constexpr int kStage = kWImg + kXStage;
  static constexpr int kBytes = 2 * kStage;
};

// what a Loader is built from: the block's site and its window of the site's pixel stream and frames
struct BlockGeom {
  int HW, L;
  int px0, npx;                                  // first stream pixel of the block, pixels of the stream (B * HW)
  int t0, nf;                                    // first frame of the temporal group, frames it holds (<= kFrames)
  int tid;
};

__device__ __forceinline__ spu4 pack_hi(const unsigned (&v)[8]) {         // the upper halves of eight words, element e at bits 16 e
  return spu4{sp_pair(v[0], v[1]), sp_pair(v[2], v[3]), sp_pair(v[4], v[5]), sp_pair(v[6], v[7])};
}

// eight fp32 values -> the three bf16 planes, cut as pw_tdiff_split_kernel cuts (l has at most 8 significant bits: its low half is zero)
__device__ __forceinline__ void cut3(const unsigned (&v)[8], spu4& ph, spu4& pm, spu4& pl) {
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sp_cut(__uint_as_float(v[e]), h[e], m[e], l[e]);
  ph = pack_hi(h); pm = pack_hi(m); pl = pack_hi(l);
}

// eight fp16 bit patterns (the low halves of v) -> two planes, cut like pw_tdiff_split_kernel cuts x.float(): h = the upper 16 bits,
// m = the upper 16 bits of x - h (x - h - m = +0 for every finite fp16)
__device__ __forceinline__ void cut2(const unsigned (&v)[8], spu4& ph, spu4& pm) {
  unsigned h[8], m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = widen16<kFeatF16>(v[e] & 0xffffu);
    h[e] = __float_as_uint(x) & 0xffff0000u;
    m[e] = __float_as_uint(x - __uint_as_float(h[e])) & 0xffff0000u;
  }
  ph = pack_hi(h); pm = pack_hi(m);
}

// the part (channel group) of the site's map that holds K-tile kt: its base, its channels, the K-tile's first channel in it (scalar)
using PartK = Part;
__device__ __forceinline__ PartK part_of_ktile(const PtSite& S, int kt) { return part_at(S, kt * BK); }

// One block of a staged units kernel.  Loader:
//   Loader(S, geom)       sets up the thread's items of a K-tile's maps
//   load(S, kt)           global -> registers, zeros for what lies outside the block's frames and pixels
//   store(xs)             registers -> the plane entries in a stage's map area xs
//   static slot(li, lg)   the pixel slot the entry of (pixel li of a tile, k group lg) sits in
template <int NPL, class Loader>
__device__ __forceinline__ void units_block(const PtParams& p) {
  using L_ = Lds<NPL>;
  extern __shared__ __attribute__((aligned(16))) char lds[];        // [stage 2] { weight image 30 KB | maps [frame][tile][plane] }

  OFFK_SITE_INDEX(si, p, (int)blockIdx.x)
  const PtSite& S = p.s[si];
  const int nblk_site = OFFK_SITE_BLOCKS(p, si, S);
  const int C = S.C, HW = S.HW, L = p.L;
  int local = xcd_contiguous((int)blockIdx.x - S.blk_begin, nblk_site);
  const int tg = local % p.tgroups;
  const int px0 = (local / p.tgroups) * kPixels;             // first stream pixel of the block
  const int npx = p.B * HW;
  const int t0 = tg * (kFrames - 1);
  const int nf = min(kFrames, L - t0);
  const bool last_group = tg == p.tgroups - 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pt = wave >> 2, wl = wave & 3;
  const int li = lane & 15, lg = lane >> 4;

  Loader ld(S, BlockGeom{HW, L, px0, npx, t0, nf, tid});
  spu4 wv[4] = {};
  auto load_tile = [&](int kt) {
    const spu4* wsrc = reinterpret_cast<const spu4*>(static_cast<const char*>(S.wt16s) + (size_t)kt * kWImg);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = tid + r * kThreads;
      if (c < kWChunks) wv[r] = wsrc[c];
    }
    ld.load(S, kt);
  };
  auto store_tile = [&](int stage) {
    char* const sb = lds + stage * L_::kStage;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = tid + r * kThreads;
      if (c < kWChunks) *reinterpret_cast<spu4*>(sb + 16 * c) = wv[r];
    }
    ld.store(sb + kWImg);
  };

  spf4 a1[kFrames][2], a2[kFrames][2], d1[4], d2[4];        // as pw_tdiff_split_kernel: A1 = sum w_h x_h, A2 = the small products
#pragma unroll
  for (int j = 0; j < kFrames; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c) { a1[j][c] = spf4{0.f, 0.f, 0.f, 0.f}; a2[j][c] = spf4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int i = 0; i < 4; ++i) { d1[i] = spf4{0.f, 0.f, 0.f, 0.f}; d2[i] = spf4{0.f, 0.f, 0.f, 0.f}; }
  const int ctd = wl & 1, fd0 = wl >> 1;

  const int nkt = C / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nkt) load_tile(kt + 1);
    const char* const sb = lds + st * L_::kStage;
    spu4 w0[3], w1[3], wd[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      w0[q] = *reinterpret_cast<const spu4*>(sb + ((wl * 2 + 0) * 3 + q) * 1024 + lane * 16);
      w1[q] = *reinterpret_cast<const spu4*>(sb + ((wl * 2 + 1) * 3 + q) * 1024 + lane * 16);
      wd[q] = *reinterpret_cast<const spu4*>(sb + ((4 * 2 + ctd) * 3 + q) * 1024 + lane * 16);
    }
    const char* const xrd = sb + kWImg + pt * NPL * kPlane + lg * 256 + (Loader::slot(li, lg) << 4);
    auto rdx = [&](spu4 (&x)[3], int f) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (q < NPL) x[q] = *reinterpret_cast<const spu4*>(xrd + f * L_::kXFrame + q * kPlane);
        else x[q] = spu4{0u, 0u, 0u, 0u};
      }
    };
    // gen: per frame and channel tile pw_tdiff_split_kernel's sequence (planes 0 = h, 1 = m, 2 = l) without the products of +0 planes
#pragma unroll
    for (int j = 0; j < kFrames; ++j) {
      spu4 x[3];
      rdx(x, j);
      sp_mfma(a2[j][0], w0[2], x[0]);
      sp_mfma(a2[j][1], w1[2], x[0]);
      if constexpr (NPL > 2) {
        sp_mfma(a2[j][0], w0[0], x[2]);
        sp_mfma(a2[j][1], w1[0], x[2]);
      }
      if constexpr (NPL > 1) {
        sp_mfma(a2[j][0], w0[1], x[1]);
        sp_mfma(a2[j][1], w1[1], x[1]);
      }
      sp_mfma(a2[j][0], w0[1], x[0]);
      sp_mfma(a2[j][1], w1[1], x[0]);
      if constexpr (NPL > 1) {
        sp_mfma(a2[j][0], w0[0], x[1]);
        sp_mfma(a2[j][1], w1[0], x[1]);
      }
      sp_mfma(a1[j][0], w0[0], x[0]);
      sp_mfma(a1[j][1], w1[0], x[0]);
    }
    // the next K-tile into the other stage (read by nobody since the last barrier) between the gen and the down MFMAs: the cut's
    // vector work of one wave overlaps the MFMAs of the SIMD's other wave
    if (kt + 1 < nkt) store_tile(st ^ 1);
    // down: frames fd0 + 2 i (frame slot 7 of waves 2, 3 holds no frame: skipped -- its tile is never stored)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (fd0 + 2 * i >= kFrames) continue;
      spu4 x[3];
      rdx(x, fd0 + 2 * i);
      sp_mfma(d2[i], wd[2], x[0]);
      if constexpr (NPL > 2) sp_mfma(d2[i], wd[0], x[2]);
      sp_mfma(d1[i], wd[0], x[0]);
      if constexpr (NPL > 1) sp_mfma(d2[i], wd[1], x[1]);
      sp_mfma(d2[i], wd[1], x[0]);
      if constexpr (NPL > 1) sp_mfma(d2[i], wd[0], x[1]);
    }
    __syncthreads();
  }

  // ---- epilogue (pw_tdiff_split_kernel's): lane = (pixel li, channels 4 kq .. + 3 of a channel tile) ----
  const int kq_e = lg;
  const int gp = px0 + pt * 16 + li;
  const bool pix_ok = gp < npx;
  const int bl = pix_ok ? gp / HW : 0, pixl = pix_ok ? gp - bl * HW : 0;
  const size_t pair0 = (size_t)bl * (L - 1) + t0;
#pragma unroll
  for (int ct = 0; ct < 2; ++ct) {
    const spf4 bg = *reinterpret_cast<const spf4*>(S.bias + wl * 32 + 16 * ct + 4 * kq_e);
#pragma unroll
    for (int j = 0; j < kFrames; ++j) {
      const spf4 v = (a1[j][ct] + a2[j][ct]) + bg;
      a1[j][ct] = spf4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
    }
  }
#pragma unroll
  for (int j = 0; j + 1 < kFrames; ++j)
    if (j + 1 < nf && pix_ok) {
      float* const trow = S.M + ((pair0 + j) * HW + pixl) * S.m_cs + S.m_coff + kDownCh + wl * 32 + 4 * kq_e;
      *reinterpret_cast<spf4*>(trow) = a1[j + 1][0] - a1[j][0];
      *reinterpret_cast<spf4*>(trow + 16) = a1[j + 1][1] - a1[j][1];
    }
  {
    const spf4 bd = *reinterpret_cast<const spf4*>(S.bias_down + 16 * ctd + 4 * kq_e);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = fd0 + 2 * i;
      if (j < nf && (last_group || j < kFrames - 1) && pix_ok) {
        const int dr = down_row(bl, t0 + j, L, p.P, p.slice_mode);
        if (dr >= 0) *reinterpret_cast<spf4*>(S.D + ((size_t)dr * HW + pixl) * kDownCh + 16 * ctd + 4 * kq_e) = (d1[i] + d2[i]) + bd;
      }
    }
  }
}

// ---- host: the block plan of these kernels (a site's stream of B * HW pixels in blocks of 32, times the temporal groups) and the launch
inline void plan_blocks(PtParams& p) {
  int blk = 0;
  for (int i = 0; i < p.nsites; ++i) {
    PtSite& o = p.s[i];
    o.chunks = o.nrem = o.rsh = o.qpc = 0;
    o.blk_begin = blk;
    blk += ((p.B * o.HW + kPixels - 1) / kPixels) * p.tgroups;
  }
  p.total_blocks = blk;
}

// p: the fused units' sites as run_off_units_fused fills them (wt16s: the split plane image)
template <int NPL>
hipError_t launch(void (*kernel)(PtParams), const PtParams& p_in, hipStream_t st) {
  PtParams p = p_in;
  if (p.nsites <= 0 || p.B <= 0) return hipSuccess;
  plan_blocks(p);
  hipError_t er = lds_attr_once(reinterpret_cast<const void*>(kernel), Lds<NPL>::kBytes);
  if (er != hipSuccess) return er;
  hipLaunchKernelGGL(kernel, dim3(p.total_blocks), dim3(kThreads), Lds<NPL>::kBytes, st, p);
  return hipGetLastError();
}

}  // namespace staged
}  // namespace offk
