// K1 in split-fp32 arithmetic (offk_off_units_train_split): the stacked 1x1 reduces of pw_reduce.hip,
//   G[N*HW][128] = relu(Wg X + bg) on all frames,   D[P*HW][32] = Wd X + bd on the frames of the spatial slice,
// on the bf16 matrix pipe, DESIGN.md 5.1.  Both operands are cut into THREE bf16 planes by truncation (synth.cut3); a k step is 32
// consecutive channels, the steps run in increasing channel order over the whole C (concat order across parts), channel 32 kt + 8 g + e
// sits in lane group g, element e of step kt.  Per step six of the nine plane products are issued on v_mfma_f32_16x16x32_bf16 in
// synth.SPLIT_PRODUCTS order, the weights in the first operand slot as in pw_tdiff_split_kernel: w_l x_h, w_h x_l, w_m x_m, w_m x_h, w_h x_m
// into accumulator A2, w_h x_h into A1; no split-K, no atomics; v = (A1 + A2) + bias, G = max(v, 0), D = v.  That is what
// pw_tdiff_split_kernel computes in front of its temporal difference (synth.emulate_split_dot(form="units")).  A bf16 map IS its leading
// plane (three products, nothing dropped), an fp16 map is two planes (five products, only w_l x_m dropped): compile-time forms that leave
// out MFMAs which would add +-0, so their results equal the fp32 form's on the widened maps.
//
// Two launches.  The pre-pass (units_fwd_split_pack_kernel) cuts [Wg ; Wd] -- bound or set, as they are when it runs -- into the handle's
// plane image in operand order: one 16-byte item per (k step, 16-channel tile ct 0..9, plane, lane): plane q of
// W[16 ct + (lane & 15)][32 kt + 8 (lane >> 4) + 0..7], pw_pack_split16_kernel's layout.  The GEMM keeps K1's launch plan: the grouped grid,
// the block -> 128 rows mapping, down_row for both slice modes (quirk Q1), rows past M.  Threads 0..255 run K1's map loader thread for thread
// (mode 0: NCHW pixel quads, mode 1: NCHW single pixels of the 7x7 sites, mode 2: channels-last; plain guarded loads, a row past M
// reads nothing and counts as zeros) and cut on the way into the LDS plane images ([16-row tile 8][k group 4][16 rows] x 16 B per plane,
// rows swizzled by the k group as in units_wgrad_split.hip); all 512 threads copy the step's 30720 B of weight operands from the image
// into LDS as they lie.  Eight waves: wave w owns rows 32 (w >> 1) .. + 31 x channels 80 (w & 1) .. + 79: 2 x 5 tiles x (A1, A2) = 80
// accumulator registers, one weight fetch serves 128 output rows.  One block per CU, the step images double-buffered (110592 B on fp32
// maps) and TWO steps in flight in registers: a step takes over the operands of step kt + 1 (loaded a whole step earlier; the one wait
// for the loads in flight stands there, at the top), issues the loads of step kt + 2, runs the MFMAs of step kt and cuts step kt + 1 into
// the other buffer behind them with no wait of its own; ONE barrier per step.  (With the loads of step kt + 1 issued in the same step and
// waited for in front of the cut the train forward was 0.03 - 0.18 ms slower)  build.py refuses a form of this kernel
// that spills or keeps anything in scratch memory (REGISTER_RESIDENT_KERNELS).
#include "units_common.h"
#include "split_common.h"

namespace offk {
namespace {

constexpr int FS_BM = 128, FS_THREADS = 512;
constexpr int FS_PIECE = 1024;                       // one 16-row tile of one plane: 4 k groups x 16 rows x 16 B
constexpr int FS_CT = kUnitCh / 16;                  // 10 channel tiles
constexpr int FS_WTILE = FS_CT * 3 * FS_PIECE;       // 30720: the weight operands of one k step
constexpr int FS_WITEMS = FS_WTILE / 16;             // 1920 16-byte items
constexpr int FS_XPLANE = (FS_BM / 16) * FS_PIECE;   // 8192
constexpr int FS_WCT = FS_CT / 2;                    // channel tiles of one wave

template <int V> struct FsMode { static constexpr int value = V; };   // a loader mode known at compile time

}  // namespace

// The pre-pass: one thread per 16-byte item of a site's image (the three planes of the item's eight weights).
__global__ __launch_bounds__(256) void units_fwd_split_pack_kernel(UfsParams p) {
  const float* wg = p.s[0].wg; const float* wd = p.s[0].wd; uint4* img = static_cast<uint4*>(p.s[0].wimg);
  int C = p.s[0].C, begin = p.s[0].pack_begin;
#pragma unroll
  for (int i = 1; i < kNumSites; ++i)
    if (i < p.nsites && (int)blockIdx.x >= p.s[i].pack_begin) {
      wg = p.s[i].wg; wd = p.s[i].wd; img = static_cast<uint4*>(p.s[i].wimg); C = p.s[i].C; begin = p.s[i].pack_begin;
    }
  const int item = ((int)blockIdx.x - begin) * 256 + (int)threadIdx.x;
  if (item >= (C / BK) * FS_CT * 64) return;
  const int lane = item & 63, ct = (item >> 6) % FS_CT, kt = (item >> 6) / FS_CT;
  const int row = 16 * ct + (lane & 15), g = lane >> 4;
  const float* src = (row < kGenCh ? wg + (size_t)row * C : wd + (size_t)(row - kGenCh) * C) + kt * BK + 8 * g;
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) sp_cut(src[e], h[e], m[e], l[e]);
  uint4* dst = img + (size_t)(kt * FS_CT + ct) * 3 * 64 + lane;
  dst[0] = make_uint4(sp_pair(h[0], h[1]), sp_pair(h[2], h[3]), sp_pair(h[4], h[5]), sp_pair(h[6], h[7]));
  dst[64] = make_uint4(sp_pair(m[0], m[1]), sp_pair(m[2], m[3]), sp_pair(m[4], m[5]), sp_pair(m[6], m[7]));
  dst[128] = make_uint4(sp_pair(l[0], l[1]), sp_pair(l[2], l[3]), sp_pair(l[4], l[5]), sp_pair(l[6], l[7]));
}

// FEAT: element type of the feature map (kFeatF32 / kFeatBf16 / kFeatF16), | kFeatCl: channels-last maps.  NPX: the planes such a map has.
template <int FEAT>
__global__ __launch_bounds__(FS_THREADS, 1) void units_fwd_split_kernel(UfsParams p) {
  constexpr bool CL = (FEAT & kFeatCl) != 0;
  constexpr int FT = FEAT & ~kFeatCl;   // the element type alone
  constexpr int NPX = FT == kFeatBf16 ? 1 : (FT == kFeatF16 ? 2 : 3);
  constexpr int BUF_BYTES = FS_WTILE + NPX * FS_XPLANE;   // one k step: the weight operands as the image has them, then the plane images of X
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];   // two such buffers

  // block -> site: a uniform index into the by-value table, as pw_tdiff_split_kernel (the field-wise select chain of K1 over nine
  // entries of this size left scalar registers spilt); then the members this kernel reads, one by one (`S = p.s[si]` copies the whole
  // entry through vector registers: 60 fewer v_mov, other branches -- not the parent's code)
  OFFK_SITE_INDEX(si, p, (int)blockIdx.x)
  const UfsSite& S0 = p.s[si];
  UfsSite S;
  S.wimg = S0.wimg; S.bias = S0.bias; S.bias_down = S0.bias_down; S.G = S0.G; S.D = S0.D;
  S.C = S0.C; S.HW = S0.HW; S.M = S0.M; S.blk_begin = S0.blk_begin; S.nparts = S0.nparts;
#pragma unroll
  for (int q = 0; q < 4; ++q) { S.xp[q] = S0.xp[q]; S.cp[q] = S0.cp[q]; }
  const int nblk_site = OFFK_SITE_BLOCKS(p, si, S);
  const int C = S.C, HW = S.HW, M = S.M;
  const int m0 = xcd_contiguous((int)blockIdx.x - S.blk_begin, nblk_site) * FS_BM;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = tid >> 6;   // (kept in a vector register: the scalar form left scalar registers spilt)
  const bool xl = wave < 4;   // the map loader's role: K1's 256 threads
  const int lt = tid & 255;   // the thread's index in K1's loader

  // is any row of this block a source frame of the spatial branch?  K1 asks down_row for every frame the block touches; in closed form:
  // flat slice: the first frame is below P; per-clip slice: not every frame is a clip's last one (two neighbours never both are)
  bool down_active;
  {
    const int f_first = m0 / HW, f_last = (min(m0 + FS_BM, M) - 1) / HW;
    if (p.slice_mode == 0) down_active = f_first < p.P;
    else down_active = p.L > 1 && (f_last > f_first || f_first % p.L != p.L - 1);
  }

  // ---- the map loader: K1's three modes, thread for thread (pw_reduce.hip) ----
  // mode 0: NCHW, HW % 4 == 0 : thread = (k quad lt & 7, pixel quad lt >> 3);  mode 1: NCHW, any HW: thread = (pixel lt & 127, k quads
  // (lt >> 7) + 2 r);  mode 2: channels-last: thread = (rows (lt >> 3) + 32 r, k quad lt & 7)
  const int mode = CL ? 2 : ((HW & 3) == 0 ? 0 : 1);
  int fr = 0, pix = 0;
  bool row_ok = true;
  if (mode != 2) {
    const int m = m0 + (mode == 0 ? 4 * (lt >> 3) : (lt & 127));
    row_ok = m < M;                       // mode 0: M % 4 == 0, so the quad is all-in or all-out
    const int mm = row_ok ? m : 0;
    fr = mm / HW; pix = mm - fr * HW;
  }
  const int koff = mode == 1 ? 4 * (lt >> 7) : 4 * (lt & 7);

  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  typedef unsigned u2u __attribute__((ext_vector_type(2), aligned(4)));
  // TWO steps in flight: rgN / wrN receive the loads of step kt + 2 while rg / wr (step kt + 1, taken over at the top of the step, where the
  // one wait for everything in flight stands) are cut behind the MFMAs of step kt without any wait of their own
  float4 rg[4], rgN[4];   // the map elements: fp32 values, or 16-bit elements as loaded (bit patterns, widened by the store)
  spu4 wr[4], wrN[4];     // the thread's items of the step's weight operands
  auto load_x = [&](int k0, auto MT) {
    constexpr int MODE = decltype(MT)::value;
    if (!xl) return;
    const float* xb; int cpart, kl;
    part_at(S, k0, xb, cpart, kl);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (FT == kFeatF32) {
      if constexpr (MODE == 0) {
        const float* base = xb + ((size_t)fr * cpart + kl + koff) * HW + pix;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          rgN[j] = z;
          if (row_ok) { const f4u v = *reinterpret_cast<const f4u*>(base + (size_t)j * HW); rgN[j] = make_float4(v.x, v.y, v.z, v.w); }
        }
      } else if constexpr (MODE == 1) {
        const float* base = xb + ((size_t)fr * cpart + kl + koff) * HW + pix;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float* q = base + (size_t)(8 * r) * HW;
          rgN[r] = z;
          if (row_ok) rgN[r] = make_float4(q[0], q[HW], q[2 * (size_t)HW], q[3 * (size_t)HW]);
        }
      } else {
        const float* base = xb + (size_t)(m0 + (lt >> 3)) * cpart + kl + koff;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          rgN[r] = z;
          if (m0 + (lt >> 3) + 32 * r < M) { const f4u v = *reinterpret_cast<const f4u*>(base + (size_t)32 * r * cpart); rgN[r] = make_float4(v.x, v.y, v.z, v.w); }
        }
      }
    } else {
      const unsigned short* xs = reinterpret_cast<const unsigned short*>(xb);
      if constexpr (MODE == 0) {
        const unsigned short* base = xs + ((size_t)fr * cpart + kl + koff) * HW + pix;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          rgN[j] = z;
          if (row_ok) { const u2u v = *reinterpret_cast<const u2u*>(base + (size_t)j * HW); rgN[j].x = __uint_as_float(v.x); rgN[j].y = __uint_as_float(v.y); }
        }
      } else if constexpr (MODE == 1) {
        const unsigned short* base = xs + ((size_t)fr * cpart + kl + koff) * HW + pix;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned short* q = base + (size_t)(8 * r) * HW;
          rgN[r] = z;
          if (row_ok) rgN[r] = make_float4(__uint_as_float(q[0]), __uint_as_float(q[HW]), __uint_as_float(q[2 * (size_t)HW]), __uint_as_float(q[3 * (size_t)HW]));
        }
      } else {
        const unsigned short* base = xs + (size_t)(m0 + (lt >> 3)) * cpart + kl + koff;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          rgN[r] = z;
          if (m0 + (lt >> 3) + 32 * r < M) { const u2u v = *reinterpret_cast<const u2u*>(base + (size_t)32 * r * cpart); rgN[r].x = __uint_as_float(v.x); rgN[r].y = __uint_as_float(v.y); }
        }
      }
    }
  };
  auto load_w = [&](int kt) {
    const spu4* src = reinterpret_cast<const spu4*>(static_cast<const char*>(S.wimg) + (size_t)kt * FS_WTILE);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (tid + FS_THREADS * j < FS_WITEMS) wrN[j] = src[tid + FS_THREADS * j];
  };
  auto take = [&]() {   // the loads in flight have landed HERE (the asm reads their registers), not in front of the cut
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      asm volatile("" : "+v"(rgN[j].x), "+v"(rgN[j].y), "+v"(rgN[j].z), "+v"(rgN[j].w), "+v"(wrN[j]));
      rg[j] = rgN[j]; wr[j] = wrN[j];
    }
  };
  auto widen4 = [](const float4& v) { return widen16x4<FT>(__float_as_uint(v.x), __float_as_uint(v.y)); };   // four consecutive 16-bit elements in v.x, v.y
  // where the 8 bytes of (row, k quad kq) lie in a plane image.  Inside a (tile, k group) piece row r sits at r ^ (kg << sh): sh = 0 where
  // a thread stores four rows of one k quad (mode 0), 1 where it stores one row (modes 1, 2), as in units_wgrad_split.hip
  const int sh = mode == 0 ? 0 : 1;
  auto quad_at = [&](char* img, int row, int kq) {
    const int kg = kq >> 1;
    return img + (row >> 4) * FS_PIECE + kg * 256 + (((row & 15) ^ (kg << sh)) << 4) + (kq & 1) * 8;
  };
  // the step held in rg[] / wr[] -> buffer `buf`
  auto store_tile = [&](char* buf, auto MT) {
    constexpr int MODE = decltype(MT)::value;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (tid + FS_THREADS * j < FS_WITEMS) *reinterpret_cast<spu4*>(buf + (tid + FS_THREADS * j) * 16) = wr[j];
    if (!xl) return;
    char* const Xp = buf + FS_WTILE;
    if constexpr (MODE == 0) {
      float4 w[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) w[j] = FT == kFeatF32 ? rg[j] : widen4(rg[j]);
      // k row j's four pixels -> pixel i's four k, as K1 transposes them
      const int row = 4 * (lt >> 3), kq = lt & 7;
      sp_store_quad<NPX>(quad_at(Xp, row, kq), FS_XPLANE, w[0].x, w[1].x, w[2].x, w[3].x);
      sp_store_quad<NPX>(quad_at(Xp, row + 1, kq), FS_XPLANE, w[0].y, w[1].y, w[2].y, w[3].y);
      sp_store_quad<NPX>(quad_at(Xp, row + 2, kq), FS_XPLANE, w[0].z, w[1].z, w[2].z, w[3].z);
      sp_store_quad<NPX>(quad_at(Xp, row + 3, kq), FS_XPLANE, w[0].w, w[1].w, w[2].w, w[3].w);
    } else if constexpr (MODE == 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float4 v = rg[r];
        if constexpr (FT != kFeatF32)
          v = make_float4(widen16<FT>(__float_as_uint(v.x)), widen16<FT>(__float_as_uint(v.y)), widen16<FT>(__float_as_uint(v.z)), widen16<FT>(__float_as_uint(v.w)));
        sp_store_quad<NPX>(quad_at(Xp, lt & 127, (lt >> 7) + 2 * r), FS_XPLANE, v.x, v.y, v.z, v.w);
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 v = FT == kFeatF32 ? rg[r] : widen4(rg[r]);
        sp_store_quad<NPX>(quad_at(Xp, (lt >> 3) + 32 * r, lt & 7), FS_XPLANE, v.x, v.y, v.z, v.w);
      }
    }
  };

  // accumulators [channel tile][row tile]: A1 = sum w_h x_h, A2 = the small products
  spf4 a1[FS_WCT][2], a2[FS_WCT][2];
#pragma unroll
  for (int ct = 0; ct < FS_WCT; ++ct)
#pragma unroll
    for (int j = 0; j < 2; ++j) { a1[ct][j] = spf4{0.f, 0.f, 0.f, 0.f}; a2[ct][j] = spf4{0.f, 0.f, 0.f, 0.f}; }

  const int lr16 = lane & 15, lq = lane >> 4;
  const int wrow = wave >> 1, wch = wave & 1;   // MFMA role: rows 32 wrow .. + 31, channel tiles 5 wch .. + 4
  // the down tiles (8, 9: the last two of the upper half) are left out where no row of the block is in the spatial slice, as K1 does
  const int nct = (wch == 1 && !down_active) ? FS_WCT - 2 : FS_WCT;
  const int woff = wch * FS_WCT * 3 * FS_PIECE + lane * 16;                                           // + ct * 3 * FS_PIECE + plane * FS_PIECE
  const int xoff = FS_WTILE + 2 * wrow * FS_PIECE + lq * 256 + ((lr16 ^ (lq << sh)) << 4);            // + j * FS_PIECE + plane * FS_XPLANE

  auto mma_tile = [&](const char* buf) {
    spu4 xb[2][NPX];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < NPX; ++q) xb[j][q] = *reinterpret_cast<const spu4*>(buf + xoff + j * FS_PIECE + q * FS_XPLANE);
    // the weight operands of channel tile ct + 1 are read BEFORE the MFMAs of tile ct (two register sets, a scheduling barrier pins the order)
    spu4 wb[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) wb[0][q] = *reinterpret_cast<const spu4*>(buf + woff + q * FS_PIECE);
#pragma unroll
    for (int ct = 0; ct < FS_WCT; ++ct) {
      if (ct >= nct) break;
      spu4 (&w)[3] = wb[ct & 1];
      if (ct + 1 < FS_WCT) {
#pragma unroll
        for (int q = 0; q < 3; ++q) wb[(ct + 1) & 1][q] = *reinterpret_cast<const spu4*>(buf + woff + (ct + 1) * 3 * FS_PIECE + q * FS_PIECE);
      }
      __builtin_amdgcn_sched_barrier(0);
      // synth.SPLIT_PRODUCTS order (w plane, x plane): (2, 0), (0, 2), (1, 1), (1, 0), (0, 1) -> A2; (0, 0) -> A1.  A product with a plane
      // the map's type does not have is not issued (it would add +-0)
#pragma unroll
      for (int j = 0; j < 2; ++j) sp_mfma(a2[ct][j], w[2], xb[j][0]);
      if constexpr (NPX > 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[ct][j], w[0], xb[j][NPX > 2 ? 2 : 0]);
      }
      if constexpr (NPX > 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[ct][j], w[1], xb[j][NPX > 1 ? 1 : 0]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) sp_mfma(a2[ct][j], w[1], xb[j][0]);
      if constexpr (NPX > 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[ct][j], w[0], xb[j][NPX > 1 ? 1 : 0]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) sp_mfma(a1[ct][j], w[0], xb[j][0]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // Step kt lives in buffer kt & 1.  A step: take over the operands of step kt + 1 from the load registers (everything in flight has landed:
  // it was issued a whole step ago), issue the global loads of step kt + 2, the MFMAs of step kt, the cut of step kt + 1 into the other
  // buffer -- whose last readers (the MFMAs of step kt - 1) are behind the barrier that ended the previous step -- and one barrier.
  const int nkt = C / BK;
  auto k_loop = [&](auto MT) {
    load_x(0, MT);
    load_w(0);
    take();
    if (nkt > 1) { load_x(BK, MT); load_w(1); }
    store_tile(lds_raw, MT);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {      // (every condition here is block-uniform)
      const int cur = kt & 1;
      take();                                // step kt + 1
      if (kt + 2 < nkt) { load_x((kt + 2) * BK, MT); load_w(kt + 2); }
      __builtin_amdgcn_sched_barrier(0);
      mma_tile(lds_raw + cur * BUF_BYTES);
      if (kt + 1 < nkt) store_tile(lds_raw + (cur ^ 1) * BUF_BYTES, MT);
      __syncthreads();
    }
  };
  // one K loop per loader mode (a block-uniform choice), as K1's 16-bit forms
  if constexpr (CL) k_loop(FsMode<2>());
  else if (mode == 0) k_loop(FsMode<0>());
  else k_loop(FsMode<1>());

  // ---- epilogue: (a1 + a2)[ct][j][i] = channel 16 (5 wch + ct) + 4 lq + i of row m0 + 32 wrow + 16 j + lr16 ----
#pragma unroll
  for (int ct = 0; ct < FS_WCT; ++ct) {
    if (ct >= nct) break;
    const int c = 16 * (wch * FS_WCT + ct) + 4 * lq;     // tiles 0..7: gen channels, 8, 9: down channels (wave-uniform per ct)
    const bool gen = wch * FS_WCT + ct < kGenCh / 16;
    const float* bp = gen ? S.bias + c : S.bias_down + (c - kGenCh);
    const spf4 bv = spf4{bp[0], bp[1], bp[2], bp[3]};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int m = m0 + 32 * wrow + 16 * j + lr16;
      spf4 v = (a1[ct][j] + a2[ct][j]) + bv;
      if (m >= M) continue;
      if (gen) {
        v = spf4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)};
        *reinterpret_cast<spf4*>(S.G + (size_t)m * kGenCh + c) = v;
      } else {
        const int f = m / HW, px = m - f * HW;
        const int dr = down_row(f, p.L, p.P, p.slice_mode);
        if (dr >= 0) *reinterpret_cast<spf4*>(S.D + ((size_t)dr * HW + px) * kDownCh + (c - kGenCh)) = v;
      }
    }
  }
}

template <int FEAT>
static hipError_t fs_launch(const UfsParams& p, hipStream_t st) {
  constexpr int FT = FEAT & ~kFeatCl;
  constexpr int lds = 2 * (FS_WTILE + (FT == kFeatBf16 ? 1 : (FT == kFeatF16 ? 2 : 3)) * FS_XPLANE);
  hipError_t e = lds_attr_once(reinterpret_cast<const void*>(units_fwd_split_kernel<FEAT>), lds);
  if (e != hipSuccess) return e;                                 // nothing enqueued yet
  hipLaunchKernelGGL(units_fwd_split_kernel<FEAT>, dim3(p.total_blocks), dim3(FS_THREADS), lds, st, p);
  return hipGetLastError();
}

int units_fwd_split_pack_blocks(int C) { return ((C / BK) * FS_CT * 64 + 255) / 256; }
size_t units_fwd_split_image_bytes(int C) { return (size_t)kUnitCh * C * 6; }

hipError_t units_fwd_split_pack_launch(const UfsParams& p, hipStream_t st) {
  if (p.pack_blocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(units_fwd_split_pack_kernel, dim3(p.pack_blocks), dim3(256), 0, st, p);
  return hipGetLastError();
}

// feat_dtype: kFeatF32 / kFeatBf16 / kFeatF16; cl: channels-last maps (xp[] as pw_reduce_cl16_launch wants them, else as pw_reduce_launch /
// pw_reduce_feat16_launch do)
hipError_t units_fwd_split_launch(const UfsParams& p, int feat_dtype, bool cl, hipStream_t st) {
  if (p.total_blocks <= 0) return hipSuccess;
  switch (feat_dtype) {
    case kFeatF32: return cl ? fs_launch<kFeatF32 | kFeatCl>(p, st) : fs_launch<kFeatF32>(p, st);
    case kFeatBf16: return cl ? fs_launch<kFeatBf16 | kFeatCl>(p, st) : fs_launch<kFeatBf16>(p, st);
    case kFeatF16: return cl ? fs_launch<kFeatF16 | kFeatCl>(p, st) : fs_launch<kFeatF16>(p, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace offk
