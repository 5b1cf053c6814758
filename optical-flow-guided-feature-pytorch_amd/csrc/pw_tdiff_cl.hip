// The fused units kernel of split-fp32 handles for channels-last feature maps (ABI v10, additive: offk_forward_cl and its siblings).
// Every map (part) is physically [B * L * HW][c_part], elements fp32 / bf16 / fp16.  It writes what pw_tdiff_split_kernel writes -- T
// into fusion_<28|14|7>, D_<site> -- and the S-blocks launch runs after it unchanged.
//
// Arithmetic: equal values, not a new tolerance.  The k -> operand slot mapping (K-tile kt, lane group g, element e <-> channel
// 32 kt + 8 g + e of the part that holds it), the weight plane image (pw_pack_split16_kernel), the cut (h = the upper 16 bits, m = the
// upper 16 bits of x - h, l = x - h - m), the order of the plane products into the two accumulators and the epilogue are those of
// pw_tdiff_split_kernel (fp32 maps: six MFMAs per tile and k group) and of pw_tdiff_feat16_kernel (bf16: three, fp16: five -- the
// products of a +0 plane left out), so for finite maps the outputs are torch.equal to what those kernels compute from the NCHW copy of
// the same logical tensor (tests/test_gpu_feat_cl.py).
//
// Geometry: pw_tdiff_feat16_kernel's.  One block = 512 threads = eight waves = (site, temporal group, 32 pixels of the site's stream of
// B * HW (clip, pixel) pairs) x seven frames x 160 channels; waves w and w + 4 take pixel tiles 0 and 1 with the channel work of
// pw_tdiff_split_kernel's wave w & 3.  Per K-tile the block stages in LDS
//   * the K-tile's weight plane image, 30 KB, copied as it lies;
//   * the maps as plane images [frame 7][pixel tile 2][plane 1 | 2 | 3][k group 4][pixel slot 16] x 16 B (8 bf16 = k 8g .. 8g + 7).
// The loader is what the layout changes.  An item is (frame, pixel, k group) -- 896 per K-tile, two per thread: the eight k of a lane's
// B operand are 16 (16-bit maps) or 32 (fp32) contiguous bytes of the map, fetched with one or two 16-byte loads; the four lanes of a
// pixel cover one 64- / 128-byte line.  bf16 goes to LDS as loaded, fp16 is widened and cut into two planes, fp32 into three.  All
// sites take this one form (no pixel pairs, no 2-byte loads for the odd-HW 7x7 sites).
// LDS writes: a 16-byte ds_write is banked per eight contiguous lanes over 128 B, and eight loader lanes are two pixels x four k groups,
// whose entries [g][pixel] x 16 B would all fall on two 16-byte slots (4-way).  So the entry of (k group g, pixel p) sits at pixel slot
// p ^ g, and the loader's lane -> pixel map swaps pixel bits 0 and 2: the eight lanes then hold pixels p, p + 4 and write the eight
// slots {p .. p + 3} ^ g, {p + 4 .. p + 7} ^ g -- conflict-free.  The XOR touches slot bits 0 - 1 only, which keeps every 16-lane group
// of the MFMA side's ds_read_b128 ({0-3, 12-15} of one k group, {4-11} of the next) on sixteen distinct slots.
// Double-buffered through registers, one barrier per K-tile.  LDS: 2 x (30 KB + 7 x 2 x (1 | 2 | 3) KB) = 88 | 116 | 144 KB: one
// block (eight waves) per CU.  Compiler-scheduled: no counted waits.
#include <cstdio>
#include <cstdlib>

#include "offk_common.h"
#include "offk_internal.h"

namespace offk {

namespace {
constexpr int CL_FT = 7;                         // frames per block (temporal groups of pt_tgroups)
constexpr int CL_PX = 32;                        // pixels per block: two MFMA pixel tiles
constexpr int CL_THREADS = 512;
constexpr int CL_WIMG = 5 * 2 * 3 * 1024;        // one K-tile of the weight plane image: 30 KB
constexpr int CL_WCHUNKS = CL_WIMG / 16;         // 1920 16-byte pieces
constexpr int CL_PLANE = 1024;                   // [k group 4][pixel slot 16] x 16 B
constexpr int CL_ITEMS = CL_FT * CL_PX * 4;      // (frame, pixel, k group): 896

template <int NPL>
struct ClLds {
  static constexpr int kXFrame = 2 * NPL * CL_PLANE;            // both pixel tiles of one frame
  static constexpr int kXStage = CL_FT * kXFrame;
  static constexpr int kStage = CL_WIMG + kXStage;
  static constexpr int kBytes = 2 * kStage;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int cl_down_row(int b, int t, int L, int P, int slice_mode) {
  if (slice_mode == 0) { const int f = b * L + t; return f < P ? f : -1; }
  return t < L - 1 ? b * (L - 1) + t : -1;
}

__device__ __forceinline__ u32x4 cl_pack_hi(const unsigned (&v)[8]) {      // the upper halves of eight words, element e at bits 16 e
  return u32x4{__builtin_amdgcn_perm(v[1], v[0], 0x07060302), __builtin_amdgcn_perm(v[3], v[2], 0x07060302),
               __builtin_amdgcn_perm(v[5], v[4], 0x07060302), __builtin_amdgcn_perm(v[7], v[6], 0x07060302)};
}

// eight fp32 values -> the three bf16 planes, cut as pw_tdiff_split_kernel cuts (l has at most 8 significant bits: its low half is zero)
__device__ __forceinline__ void cl_cut3(const unsigned (&v)[8], u32x4& ph, u32x4& pm, u32x4& pl) {
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    h[e] = v[e] & 0xffff0000u;
    const float r = __uint_as_float(v[e]) - __uint_as_float(h[e]);
    m[e] = __float_as_uint(r) & 0xffff0000u;
    l[e] = __float_as_uint(r - __uint_as_float(m[e]));
  }
  ph = cl_pack_hi(h); pm = cl_pack_hi(m); pl = cl_pack_hi(l);
}

// eight fp16 values (two per word, element e in the e & 1 half of word e >> 1) -> two planes, cut as pw_tdiff_feat16_kernel cuts
__device__ __forceinline__ void cl_cut2(const u32x4& v, u32x4& ph, u32x4& pm) {
  unsigned h[8], m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const unsigned word = v[e >> 1];
    const float x = (float)__builtin_bit_cast(_Float16, (unsigned short)((e & 1) ? word >> 16 : word & 0xffffu));
    h[e] = __float_as_uint(x) & 0xffff0000u;
    m[e] = __float_as_uint(x - __uint_as_float(h[e])) & 0xffff0000u;
  }
  ph = cl_pack_hi(h); pm = cl_pack_hi(m);
}
}  // namespace

// FEAT: kFeatF32 (three planes, six MFMAs per tile and k group), kFeatBf16 (one, three), kFeatF16 (two, five)
template <int FEAT>
__global__ __launch_bounds__(CL_THREADS, 1) void pw_tdiff_cl_kernel(PtParams p) {
  constexpr int NPL = FEAT == kFeatF32 ? 3 : FEAT == kFeatF16 ? 2 : 1;
  constexpr int ES = FEAT == kFeatF32 ? 4 : 2;                      // bytes per map element
  constexpr int NLD = FEAT == kFeatF32 ? 2 : 1;                     // 16-byte loads per item
  using Lds = ClLds<NPL>;
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
  const int px0 = (local / p.tgroups) * CL_PX;               // first stream pixel of the block
  const int npx = p.B * HW;
  const int t0 = tg * (CL_FT - 1);
  const int nf = min(CL_FT, L - t0);
  const bool last_group = tg == p.tgroups - 1;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pt = wave >> 2, wl = wave & 3;
  const int li = lane & 15, lg = lane >> 4;

  // ---- loader: item = (frame, pixel, k group), 896, two per thread; the four lanes of a pixel take its four k groups (one line of the
  //      map); pixel bits 0 and 2 swapped against the lane order (the LDS write banking, above) ----
  int it_dst[2];                                             // byte offset of the item's plane 0 entry in a stage's map area
  size_t it_row[2];                                          // (clip frame b L + t0 + f) HW + pixel: the item's row of the map
  int it_g8[2];
  bool it_ok[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int item = tid + r * CL_THREADS;
    const int g = item & 3, q = (item >> 2) & 31, f = item >> 7;
    const int pp = (q & ~5) | ((q & 1) << 2) | ((q >> 2) & 1);
    const int gp = px0 + pp;
    const bool ok = item < CL_ITEMS && f < nf && gp < npx;
    const int b = ok ? gp / HW : 0;
    it_ok[r] = ok; it_g8[r] = 8 * g;
    it_row[r] = ok ? (size_t)(b * L + t0 + f) * HW + (gp - b * HW) : 0;
    it_dst[r] = (f * 2 + (pp >> 4)) * NPL * CL_PLANE + g * 256 + (((pp & 15) ^ g) << 4);
  }
  // per K-tile: part pick (scalar) and the address of each item's eight k
  auto map_src = [&](int kt, int r) -> const u32x4* {
    const float* xb = S.xp[0]; int cpart = S.cp[0], kl = kt * BK;
    if (S.nparts > 1 && kl >= S.cp[0]) {
      kl -= S.cp[0]; xb = S.xp[1]; cpart = S.cp[1];
      if (S.nparts > 2 && kl >= S.cp[1]) {
        kl -= S.cp[1]; xb = S.xp[2]; cpart = S.cp[2];
        if (S.nparts > 3 && kl >= S.cp[2]) { kl -= S.cp[2]; xb = S.xp[3]; cpart = S.cp[3]; }
      }
    }
    return reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(xb) + (it_row[r] * cpart + kl + it_g8[r]) * ES);
  };
  u32x4 mv[2][NLD];
  u32x4 wv[4] = {};
  auto load_tile = [&](int kt) {
    const u32x4* wsrc = reinterpret_cast<const u32x4*>(static_cast<const char*>(S.wt16s) + (size_t)kt * CL_WIMG);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = tid + r * CL_THREADS;
      if (c < CL_WCHUNKS) wv[r] = wsrc[c];
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (it_ok[r]) {
        const u32x4* src = map_src(kt, r);
#pragma unroll
        for (int n = 0; n < NLD; ++n) mv[r][n] = src[n];
      } else {
#pragma unroll
        for (int n = 0; n < NLD; ++n) mv[r][n] = u32x4{0u, 0u, 0u, 0u};
      }
    }
  };
  auto store_tile = [&](int stage) {
    char* const sb = lds + stage * Lds::kStage;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = tid + r * CL_THREADS;
      if (c < CL_WCHUNKS) *reinterpret_cast<u32x4*>(sb + 16 * c) = wv[r];
    }
    char* const xs = sb + CL_WIMG;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (tid + r * CL_THREADS >= CL_ITEMS) continue;
      char* const dst = xs + it_dst[r];
      if constexpr (FEAT == kFeatBf16) {
        *reinterpret_cast<u32x4*>(dst) = mv[r][0];
      } else if constexpr (FEAT == kFeatF16) {
        u32x4 ph, pm;
        cl_cut2(mv[r][0], ph, pm);
        *reinterpret_cast<u32x4*>(dst) = ph;
        *reinterpret_cast<u32x4*>(dst + CL_PLANE) = pm;
      } else {
        const unsigned v[8] = {mv[r][0].x, mv[r][0].y, mv[r][0].z, mv[r][0].w, mv[r][NLD - 1].x, mv[r][NLD - 1].y, mv[r][NLD - 1].z, mv[r][NLD - 1].w};
        u32x4 ph, pm, pl;
        cl_cut3(v, ph, pm, pl);
        *reinterpret_cast<u32x4*>(dst) = ph;
        *reinterpret_cast<u32x4*>(dst + CL_PLANE) = pm;
        *reinterpret_cast<u32x4*>(dst + 2 * CL_PLANE) = pl;
      }
    }
  };

  f32x4 a1[CL_FT][2], a2[CL_FT][2], d1[4], d2[4];            // as pw_tdiff_split_kernel: A1 = sum w_h x_h, A2 = the small products
#pragma unroll
  for (int j = 0; j < CL_FT; ++j)
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
    const char* const xrd = sb + CL_WIMG + pt * NPL * CL_PLANE + lg * 256 + ((li ^ lg) << 4);
    auto rdx = [&](u32x4 (&x)[3], int f) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        if (q < NPL) x[q] = *reinterpret_cast<const u32x4*>(xrd + f * Lds::kXFrame + q * CL_PLANE);
        else x[q] = u32x4{0u, 0u, 0u, 0u};
      }
    };
    // gen: per frame and channel tile pw_tdiff_split_kernel's sequence (planes 0 = h, 1 = m, 2 = l) without the products of +0 planes
#pragma unroll
    for (int j = 0; j < CL_FT; ++j) {
      u32x4 x[3];
      rdx(x, j);
      mf(a2[j][0], w0[2], x[0]);
      mf(a2[j][1], w1[2], x[0]);
      if constexpr (NPL > 2) {
        mf(a2[j][0], w0[0], x[2]);
        mf(a2[j][1], w1[0], x[2]);
      }
      if constexpr (NPL > 1) {
        mf(a2[j][0], w0[1], x[1]);
        mf(a2[j][1], w1[1], x[1]);
      }
      mf(a2[j][0], w0[1], x[0]);
      mf(a2[j][1], w1[1], x[0]);
      if constexpr (NPL > 1) {
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
      if (fd0 + 2 * i >= CL_FT) continue;
      u32x4 x[3];
      rdx(x, fd0 + 2 * i);
      mf(d2[i], wd[2], x[0]);
      if constexpr (NPL > 2) mf(d2[i], wd[0], x[2]);
      mf(d1[i], wd[0], x[0]);
      if constexpr (NPL > 1) mf(d2[i], wd[1], x[1]);
      mf(d2[i], wd[1], x[0]);
      if constexpr (NPL > 1) mf(d2[i], wd[0], x[1]);
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
    for (int j = 0; j < CL_FT; ++j) {
      const f32x4 v = (a1[j][ct] + a2[j][ct]) + bg;
      a1[j][ct] = f32x4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
    }
  }
#pragma unroll
  for (int j = 0; j + 1 < CL_FT; ++j)
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
      if (j < nf && (last_group || j < CL_FT - 1) && pix_ok) {
        const int dr = cl_down_row(bl, t0 + j, L, p.P, p.slice_mode);
        if (dr >= 0) *reinterpret_cast<f32x4*>(S.D + ((size_t)dr * HW + pixl) * kDownCh + 16 * ctd + 4 * kq_e) = (d1[i] + d2[i]) + bd;
      }
    }
  }
}

// p: the fused units' sites as run_off_units_fused fills them (wt16s: the split plane image; xp[]: channels-last parts of feat_dtype
// elements); the block layout is this kernel's own
hipError_t pw_tdiff_cl_launch(const PtParams& p_in, int feat_dtype, hipStream_t st) {
  PtParams p = p_in;
  if (p.nsites <= 0 || p.B <= 0) return hipSuccess;
  int blk = 0;
  for (int i = 0; i < p.nsites; ++i) {
    PtSite& o = p.s[i];
    o.chunks = o.nrem = o.rsh = o.qpc = 0;
    o.blk_begin = blk;
    blk += ((p.B * o.HW + CL_PX - 1) / CL_PX) * p.tgroups;
  }
  p.total_blocks = blk;
  const void* k = feat_dtype == kFeatF16    ? reinterpret_cast<const void*>(pw_tdiff_cl_kernel<kFeatF16>)
                  : feat_dtype == kFeatBf16 ? reinterpret_cast<const void*>(pw_tdiff_cl_kernel<kFeatBf16>)
                                            : reinterpret_cast<const void*>(pw_tdiff_cl_kernel<kFeatF32>);
  const int bytes = feat_dtype == kFeatF16 ? ClLds<2>::kBytes : feat_dtype == kFeatBf16 ? ClLds<1>::kBytes : ClLds<3>::kBytes;
  hipError_t er = lds_attr_once(k, bytes);
  if (er != hipSuccess) return er;
  if (feat_dtype == kFeatF16) hipLaunchKernelGGL(pw_tdiff_cl_kernel<kFeatF16>, dim3(p.total_blocks), dim3(CL_THREADS), bytes, st, p);
  else if (feat_dtype == kFeatBf16) hipLaunchKernelGGL(pw_tdiff_cl_kernel<kFeatBf16>, dim3(p.total_blocks), dim3(CL_THREADS), bytes, st, p);
  else hipLaunchKernelGGL(pw_tdiff_cl_kernel<kFeatF32>, dim3(p.total_blocks), dim3(CL_THREADS), bytes, st, p);
  return hipGetLastError();
}

}  // namespace offk
