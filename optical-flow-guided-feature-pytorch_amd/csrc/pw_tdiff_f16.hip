// The fused units kernel of split-fp32 handles for 16-bit feature maps (ABI v10, additive: offk_forward_typed and its siblings).  It
// writes what pw_tdiff_split_kernel writes -- T into fusion_<28|14|7>, D_<site> -- and the S-blocks launch runs after it unchanged.
//
// Arithmetic: equal values, not a new tolerance.  A bf16 map value is exactly its own leading plane (x_m = x_l = +0); an fp16 value
// has 11 significant bits, so it is exactly two bf16 planes (x_l = +0; an fp16 subnormal is a normal number in fp32 and bf16).  The
// fp32-map kernel issues per output tile and 32-k group, into A2: w_l x_h, w_h x_l, w_m x_m, w_m x_h, w_h x_m, then into A1: w_h x_h;
// the products of a +0 plane are all +-0.  This kernel issues the remaining MFMAs -- bf16: w_l x_h, w_m x_h | w_h x_h (3), fp16: w_l x_h,
// w_m x_m, w_m x_h, w_h x_m | w_h x_h (5) -- with the same k in the same operand slots, in the same order, into the same two accumulators,
// from the same weight plane image (pw_pack_split16_kernel), and ends in the same epilogue, so for finite maps it returns
// pw_tdiff_split_kernel's values on x.float() (tests/test_gpu_feat16.py: torch.equal).
//
// Geometry.  One block = 512 threads = eight waves = (site, temporal group, 32 pixels of the site's stream of B * HW (clip, pixel)
// pairs) x seven frames x 160 channels; waves w and w + 4 take pixel tiles 0 and 1 with the channel work of pw_tdiff_split_kernel's
// wave w & 3 (gen channels 32 (w & 3) .. + 31 in two 16-channel tiles, down tile w & 1 of frames ((w & 3) >> 1) + 2 i).  A pixel's
// result does not depend on the other columns of its MFMA, so the stream order (which packs the 7x7 and 14x14 leftovers without a
// layout of their own) changes no value.  Per K-tile the block stages in LDS
//   * the K-tile's weight plane image, 30 KB, copied as it lies ([slab 5][ct 2][plane 3][lane 64] x 16 B): the eight waves read it with
//     conflict-free ds_read_b128, so each weight byte crosses the L1 once per 32 pixels (pw_tdiff_split_kernel: every wave loads its
//     own slab straight into registers, once per 16 pixels -- 5.2 of the 7.2 GB its launch pulls through the L1s);
//   * the maps as plane images [frame 7][pixel tile 2][plane 1 | 2][k group 4][pixel 16] x 16 B (8 bf16 = k 8g .. 8g + 7), the B
//     operand of the fp32 kernel's layout: a thread gathers eight k rows of one pixel pair (two pixels of a 4-byte load; the 7x7 sites,
//     whose HW is odd, one pixel of a 2-byte load), cuts fp16 into (x_h, x_m) in registers and writes 16 B per plane and pixel;
// double-buffered through registers (the loads of K-tile k + 1 are in flight during the gen MFMAs of K-tile k and go to LDS between
// its gen and down MFMAs), one barrier per K-tile.
// LDS: 2 x (30 KB + 7 x 2 x 1 | 2 KB) = 88 | 116 KB: one block (eight waves) per CU.  Compiler-scheduled: no counted waits.
#include <cstdio>
#include <cstdlib>

#include "offk_common.h"
#include "offk_internal.h"

namespace offk {

namespace {
constexpr int FH_FT = 7;                         // frames per block (as pw_tdiff_split_kernel: temporal groups of pt_tgroups)
constexpr int FH_PX = 32;                        // pixels per block: two MFMA pixel tiles
constexpr int FH_THREADS = 512;
constexpr int FH_WIMG = 5 * 2 * 3 * 1024;        // one K-tile of the weight plane image: 30 KB
constexpr int FH_WCHUNKS = FH_WIMG / 16;         // 1920 16-byte pieces
constexpr int FH_PLANE = 1024;                   // [k group 4][pixel 16] x 16 B

template <int NPL>
struct FhLds {
  static constexpr int kXFrame = 2 * NPL * FH_PLANE;            // both pixel tiles of one frame
  static constexpr int kXStage = FH_FT * kXFrame;
  static constexpr int kStage = FH_WIMG + kXStage;
  static constexpr int kBytes = 2 * kStage;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int fh_down_row(int b, int t, int L, int P, int slice_mode) {
  if (slice_mode == 0) { const int f = b * L + t; return f < P ? f : -1; }
  return t < L - 1 ? b * (L - 1) + t : -1;
}

// eight 16-bit k values of one pixel (element e = k 8g + e) -> the 16-byte plane entries: bf16 as they are; fp16 cut like
// pw_tdiff_split_kernel cuts x.float(): h = the upper 16 bits, m = the upper 16 bits of x - h (x - h - m = +0 for every finite fp16)
template <bool F16>
__device__ __forceinline__ void fh_cut8(const unsigned (&v)[8], u32x4& ph, u32x4& pm) {
  if constexpr (!F16) {
    ph = u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
    pm = u32x4{0u, 0u, 0u, 0u};
  } else {
    unsigned h[8], m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float x = (float)__builtin_bit_cast(_Float16, (unsigned short)v[e]);
      h[e] = __float_as_uint(x) & 0xffff0000u;
      m[e] = __float_as_uint(x - __uint_as_float(h[e])) & 0xffff0000u;
    }
    ph = u32x4{__builtin_amdgcn_perm(h[1], h[0], 0x07060302), __builtin_amdgcn_perm(h[3], h[2], 0x07060302),
               __builtin_amdgcn_perm(h[5], h[4], 0x07060302), __builtin_amdgcn_perm(h[7], h[6], 0x07060302)};
    pm = u32x4{__builtin_amdgcn_perm(m[1], m[0], 0x07060302), __builtin_amdgcn_perm(m[3], m[2], 0x07060302),
               __builtin_amdgcn_perm(m[5], m[4], 0x07060302), __builtin_amdgcn_perm(m[7], m[6], 0x07060302)};
  }
}
}  // namespace

// F16: fp16 maps (two planes, five MFMAs per tile and k group), else bf16 (one plane, three)
template <bool F16>
__global__ __launch_bounds__(FH_THREADS, 1) void pw_tdiff_feat16_kernel(PtParams p) {
  constexpr int NPL = F16 ? 2 : 1;
  using Lds = FhLds<NPL>;
  extern __shared__ __attribute__((aligned(16))) char lds[];        // [stage 2] { weight image 30 KB | maps [frame][tile][plane] }

  int si = 0;
#pragma unroll
  for (int i = 1; i < kNumSites; ++i)
    if (i < p.nsites && (int)blockIdx.x >= p.s[i].blk_begin) si = i;
  si = __builtin_amdgcn_readfirstlane(si);
  const PtSite& S = p.s[si];
  const int nblk_site = (si + 1 < p.nsites ? p.s[si + 1].blk_begin : p.total_blocks) - S.blk_begin;
  const int C = S.C, HW = S.HW, L = p.L;
  int local = xcd_contiguous((int)blockIdx.x - S.blk_begin, nblk_site);
  const int tg = local % p.tgroups;
  const int px0 = (local / p.tgroups) * FH_PX;               // first stream pixel of the block
  const int npx = p.B * HW;
  const int t0 = tg * (FH_FT - 1);
  const int nf = min(FH_FT, L - t0);
  const bool last_group = tg == p.tgroups - 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pt = wave >> 2, wl = wave & 3;
  const int li = lane & 15, lg = lane >> 4;
  const bool pairs = (HW & 1) == 0;                          // 28x28, 14x14: a pixel pair never straddles two clips

  // ---- loader: item = (frame, k group, pixel pair) -- 448 items, one per thread -- or (frame, k group, pixel) for odd HW -- 896, two
  //      per thread; lanes of one (frame, k group) take consecutive pixels ----
  const int nit = pairs ? 1 : 2;
  int it_f[2], it_g[2], it_p[2], it_fr[2], it_px[2];        // (frame, k group, first pixel of the tile), (clip frame b L + t0 + f, pixel)
  bool it_ok[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int item = tid + r * FH_THREADS;
    int f, g, pp;
    if (pairs) { f = item >> 6; g = (item >> 4) & 3; pp = 2 * (item & 15); }
    else { f = item >> 7; g = (item >> 5) & 3; pp = item & 31; }
    const int gp = px0 + pp;
    const bool ok = r < nit && f < nf && gp < npx;
    const int b = ok ? gp / HW : 0;
    it_f[r] = f; it_g[r] = g; it_p[r] = pp; it_ok[r] = ok;
    it_fr[r] = b * L + t0 + f; it_px[r] = ok ? gp - b * HW : 0;
  }
  // per K-tile: part pick (scalar) and the element offset of each item's first k row
  auto map_src = [&](int kt, int r) -> const unsigned short* {
    const float* xb = S.xp[0]; int cpart = S.cp[0], kl = kt * BK;
    if (S.nparts > 1 && kl >= S.cp[0]) {
      kl -= S.cp[0]; xb = S.xp[1]; cpart = S.cp[1];
      if (S.nparts > 2 && kl >= S.cp[1]) {
        kl -= S.cp[1]; xb = S.xp[2]; cpart = S.cp[2];
        if (S.nparts > 3 && kl >= S.cp[2]) { kl -= S.cp[2]; xb = S.xp[3]; cpart = S.cp[3]; }
      }
    }
    return reinterpret_cast<const unsigned short*>(xb) + ((size_t)it_fr[r] * cpart + kl + 8 * it_g[r]) * HW + it_px[r];
  };
  unsigned mv[2][8];                                         // pairs: 4-byte loads (two pixels); else 2-byte loads (one pixel)
  u32x4 wv[4] = {};
  auto load_tile = [&](int kt) {
    const u32x4* wsrc = reinterpret_cast<const u32x4*>(static_cast<const char*>(S.wt16s) + (size_t)kt * FH_WIMG);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = tid + r * FH_THREADS;
      if (c < FH_WCHUNKS) wv[r] = wsrc[c];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (it_ok[r]) {
        const unsigned short* src = map_src(kt, r);
        if (pairs) {
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
  };
  auto store_tile = [&](int stage) {
    char* const sb = lds + stage * Lds::kStage;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = tid + r * FH_THREADS;
      if (c < FH_WCHUNKS) *reinterpret_cast<u32x4*>(sb + 16 * c) = wv[r];
    }
    char* const xs = sb + FH_WIMG;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int item = tid + r * FH_THREADS;
      if (item >= (pairs ? 448 : 896)) continue;
      const int f = it_f[r], g = it_g[r], pp = it_p[r];
      unsigned v0[8], v1[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { v0[e] = mv[r][e] & 0xffffu; v1[e] = mv[r][e] >> 16; }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (s == 1 && !pairs) break;
        const int px = pp + s;
        u32x4 ph, pm;
        fh_cut8<F16>(s == 0 ? v0 : v1, ph, pm);
        char* dst = xs + (f * 2 + (px >> 4)) * NPL * FH_PLANE + g * 256 + (px & 15) * 16;
        *reinterpret_cast<u32x4*>(dst) = ph;
        if constexpr (F16) *reinterpret_cast<u32x4*>(dst + FH_PLANE) = pm;
      }
    }
  };

  f32x4 a1[FH_FT][2], a2[FH_FT][2], d1[4], d2[4];            // as pw_tdiff_split_kernel: A1 = sum w_h x_h, A2 = the small products
#pragma unroll
  for (int j = 0; j < FH_FT; ++j)
#pragma unroll
    for (int c = 0; c < 2; ++c) { a1[j][c] = f32x4{0.f, 0.f, 0.f, 0.f}; a2[j][c] = f32x4{0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int i = 0; i < 4; ++i) { d1[i] = f32x4{0.f, 0.f, 0.f, 0.f}; d2[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  auto mf = [&](f32x4& c, const u32x4& a, const u32x4& bb) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, bb), c, 0, 0, 0);
  };
  const int ctd = wl & 1, fd0 = wl >> 1;

  const int nkt = C / BK;
  load_tile(0);
  store_tile(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
    const int st = kt & 1;
    if (kt + 1 < nkt) load_tile(kt + 1);
    const char* const sb = lds + st * Lds::kStage;
    u32x4 w0[3], w1[3], wd[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      w0[q] = *reinterpret_cast<const u32x4*>(sb + ((wl * 2 + 0) * 3 + q) * 1024 + lane * 16);
      w1[q] = *reinterpret_cast<const u32x4*>(sb + ((wl * 2 + 1) * 3 + q) * 1024 + lane * 16);
      wd[q] = *reinterpret_cast<const u32x4*>(sb + ((4 * 2 + ctd) * 3 + q) * 1024 + lane * 16);
    }
    const char* const xrd = sb + FH_WIMG + pt * NPL * FH_PLANE + lg * 256 + li * 16;
    auto rdx = [&](u32x4 (&x)[2], int f) {
      x[0] = *reinterpret_cast<const u32x4*>(xrd + f * Lds::kXFrame);
      if constexpr (F16) x[1] = *reinterpret_cast<const u32x4*>(xrd + f * Lds::kXFrame + FH_PLANE);
      else x[1] = u32x4{0u, 0u, 0u, 0u};
    };
    // gen: per frame and channel tile the fp32-map kernel's sequence without the products of +0 planes
#pragma unroll
    for (int j = 0; j < FH_FT; ++j) {
      u32x4 x[2];
      rdx(x, j);
      mf(a2[j][0], w0[2], x[0]);
      mf(a2[j][1], w1[2], x[0]);
      if constexpr (F16) {
        mf(a2[j][0], w0[1], x[1]);
        mf(a2[j][1], w1[1], x[1]);
      }
      mf(a2[j][0], w0[1], x[0]);
      mf(a2[j][1], w1[1], x[0]);
      if constexpr (F16) {
        mf(a2[j][0], w0[0], x[1]);
        mf(a2[j][1], w1[0], x[1]);
      }
      mf(a1[j][0], w0[0], x[0]);
      mf(a1[j][1], w1[0], x[0]);
    }
    // the next K-tile into the other stage (read by nobody since the last barrier) between the gen and the down MFMAs: the cut's
    // vector work of one wave overlaps the MFMAs of the SIMD's other wave
    if (kt + 1 < nkt) store_tile(st ^ 1);
    // down: frames fd0 + 2 i (frame slot 7 of waves 2, 3 holds no frame: skipped -- its tile is never stored)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (fd0 + 2 * i >= FH_FT) continue;
      u32x4 x[2];
      rdx(x, fd0 + 2 * i);
      mf(d2[i], wd[2], x[0]);
      mf(d1[i], wd[0], x[0]);
      if constexpr (F16) mf(d2[i], wd[1], x[1]);
      mf(d2[i], wd[1], x[0]);
      if constexpr (F16) mf(d2[i], wd[0], x[1]);
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
    const f32x4 bg = *reinterpret_cast<const f32x4*>(S.bias + wl * 32 + 16 * ct + 4 * kq_e);
#pragma unroll
    for (int j = 0; j < FH_FT; ++j) {
      const f32x4 v = (a1[j][ct] + a2[j][ct]) + bg;
      a1[j][ct] = f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
    }
  }
#pragma unroll
  for (int j = 0; j + 1 < FH_FT; ++j)
    if (j + 1 < nf && pix_ok) {
      float* const trow = S.M + ((pair0 + j) * HW + pixl) * S.m_cs + S.m_coff + kDownCh + wl * 32 + 4 * kq_e;
      *reinterpret_cast<f32x4*>(trow) = a1[j + 1][0] - a1[j][0];
      *reinterpret_cast<f32x4*>(trow + 16) = a1[j + 1][1] - a1[j][1];
    }
  {
    const f32x4 bd = *reinterpret_cast<const f32x4*>(S.bias_down + 16 * ctd + 4 * kq_e);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int j = fd0 + 2 * i;
      if (j < nf && (last_group || j < FH_FT - 1) && pix_ok) {
        const int dr = fh_down_row(bl, t0 + j, L, p.P, p.slice_mode);
        if (dr >= 0) *reinterpret_cast<f32x4*>(S.D + ((size_t)dr * HW + pixl) * kDownCh + 16 * ctd + 4 * kq_e) = (d1[i] + d2[i]) + bd;
      }
    }
  }
}

// p: the fused units' sites as run_off_units_fused fills them (wt16s: the split plane image); the block layout is this kernel's own
hipError_t pw_tdiff_feat16_launch(const PtParams& p_in, int feat_dtype, hipStream_t st) {
  PtParams p = p_in;
  if (p.nsites <= 0 || p.B <= 0) return hipSuccess;
  int blk = 0;
  for (int i = 0; i < p.nsites; ++i) {
    PtSite& o = p.s[i];
    o.chunks = o.nrem = o.rsh = o.qpc = 0;
    o.blk_begin = blk;
    blk += ((p.B * o.HW + FH_PX - 1) / FH_PX) * p.tgroups;
  }
  p.total_blocks = blk;
  const void* k = feat_dtype == 2 ? reinterpret_cast<const void*>(pw_tdiff_feat16_kernel<true>)
                                  : reinterpret_cast<const void*>(pw_tdiff_feat16_kernel<false>);
  const int bytes = feat_dtype == 2 ? FhLds<2>::kBytes : FhLds<1>::kBytes;
  hipError_t er = lds_attr_once(k, bytes);
  if (er != hipSuccess) return er;
  if (feat_dtype == 2) hipLaunchKernelGGL(pw_tdiff_feat16_kernel<true>, dim3(p.total_blocks), dim3(FH_THREADS), bytes, st, p);
  else hipLaunchKernelGGL(pw_tdiff_feat16_kernel<false>, dim3(p.total_blocks), dim3(FH_THREADS), bytes, st, p);
  return hipGetLastError();
}

}  // namespace offk
