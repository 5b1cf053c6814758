// The weight gradient of the stacked 1x1 reduce convs in split-fp32 arithmetic (offk_off_units_backward_split): K1b's GEMM (units_bwd.hip)
//   dW[m][c] = sum over (frame f, pixel q) a[(f,q)][m] X[f][c][q],   a = [dGpre (m 0..127) | dD at row r(f) (m 128..159), zeros outside the slice]
// on the bf16 matrix pipe, DESIGN.md 5.1: both operands are cut into THREE bf16 planes by truncation (synth.cut3; sp_cut of split_common.h)
// and per 32-k step -- one K-tile: 32 pixels of one frame, pad pixels zeros, exactly K1b's tiles -- six of the nine plane
// products are issued on v_mfma_f32_16x16x32_bf16 in synth.SPLIT_PRODUCTS order with a in the role of w: a_l x_h, a_h x_l, a_m x_m, a_m x_h,
// a_h x_m into accumulator A2, a_h x_h into A1; steps in increasing K-tile order, the block's partial tile is A1 + A2, added once.  That is
// synth.emulate_split_dot(form="units") over the block's chunk of K-tiles; the slabs are then summed in chunk order by the unchanged
// wgrad_reduce_kernel.  A bf16 map IS its leading plane (three products, nothing dropped), an fp16 map is two planes (five products, a_l x_m
// dropped): compile-time forms that leave out MFMAs which would add +-0, so their results equal the fp32 form's on the widened maps.
//
// The launch plan is K1b's: the block -> (site, chunk, channel tile) mapping of WgParams, kt_per_blk, the slab layout [chunk][160][ntiles 128],
// the bias partials.  The loaders are K1b's too, thread for thread: threads 0..255 run its A-side loader (dGpre, dD) with the same loads and
// the same bs_g / bs_d sums in the same order, so the bias partials keep K1b's bits; threads 256..511 run its X loader (the three NCHW forms,
// the channels-last transposing one) with the same widening.  What store_tile writes is the cut: per K-tile three plane images of a ([16-row
// tile 10][k group of 8: 4][16 rows] x 16 B = 10240 B each) and one, two or three of X (8 tiles: 8192 B each), 55296 B for fp32 maps.  A
// lane's ds_read_b128 of (tile, k group l >> 4, row l & 15) is the MFMA operand as it lies.  Inside a (tile, k group) piece row r sits at
// r ^ swz(kg): swz = kg where a thread stores four rows of one pixel quad (a, channels-last X), 2 kg where it stores one row (NCHW X) -- the
// sixteen lanes of a ds_write_b64 group then hit sixteen different 8-byte slots of the 128-byte bank row, and the reads stay conflict-free
// (an XOR below 8 permutes rows inside the aligned quads the read groups are made of).
// Geometry: 160 x 128 per block as K1b, but EIGHT waves: wave w owns rows 80 (w >> 2) .. + 79 x channels 32 (w & 3) .. + 31, 5 x 2 tiles x
// (A1, A2) = 80 accumulator registers (four waves of 160 x 32 need 160 and spilt at two blocks per CU).  One block per CU (two waves per SIMD,
// 256 registers each) with the K-tile images DOUBLE-BUFFERED in LDS (110592 B = 87 granules of 1280 B) and THREE K-tiles in flight in K1b's
// prefetch registers (WS_DEPTH sets): a step issues the global loads of K-tile kt + 3, the MFMAs of K-tile kt from one buffer (60 per wave
// on fp32 maps behind 21 ds_read_b128, the a operands read one row tile ahead), cuts K-tile kt + 1 into the other buffer and meets ONE
// barrier.  What made the prefetch work was not its depth but its SHAPE: as long as the two loader roles were two branches (and the last
// steps' loads conditional), hipcc had to wait for every load in flight before a cut -- 1.31 ms at B = 64 x 7 on fp32 maps and 1.38 - 1.44 ms
// on bf16 maps, whose steps have half the MFMAs, at depth one and at depth three alike; with the role-free, unconditional load sequence
// of load_tile the waits leave the ten newest loads in flight (DESIGN.md section 8 has the times).  build.py refuses a form of this kernel
// that spills or keeps anything in scratch memory (REGISTER_RESIDENT_KERNELS).
#include "units_common.h"
#include "split_common.h"

namespace offk {
namespace {

constexpr int WS_BM = 160, WS_BN = 128, WS_THREADS = 512, WS_MT = WS_BM / 32;   // WS_MT: row tiles of one wave
constexpr int WS_DEPTH = 3;                          // K-tiles in flight in registers (2 or 3)
constexpr int WS_PIECE = 1024;                       // one 16-row tile of one plane: 4 k groups x 16 rows x 16 B
constexpr int WS_APLANE = (WS_BM / 16) * WS_PIECE;   // 10240
constexpr int WS_XPLANE = (WS_BN / 16) * WS_PIECE;   // 8192

template <int V> struct WsVec { static constexpr int value = V; };   // X loader form known at compile time (-1: the runtime `vec`)

}  // namespace

// FEAT: as pw_wgrad_kernel's (element type of X, | kFeatCl: channels-last X).  NPX: the planes a map of that type has.
template <int FEAT>
__global__ __launch_bounds__(WS_THREADS, 1) void pw_wgrad_split_kernel(WgParams p) {
  constexpr bool CL = (FEAT & kFeatCl) != 0;
  constexpr int FT = FEAT & ~kFeatCl;   // the element type alone
  constexpr int NPX = FT == kFeatBf16 ? 1 : (FT == kFeatF16 ? 2 : 3);
  constexpr int BUF_BYTES = 3 * WS_APLANE + NPX * WS_XPLANE;   // one K-tile: plane images of a (rows = stacked output channel, k = pixel),
  static_assert(BUF_BYTES >= (8 * kGenCh + 32 * kDownCh) * 4, "bias reduction reuses the tile memory");   // then of X (rows = input channel)
  extern __shared__ __attribute__((aligned(16))) char lds_raw[];   // two such buffers

  // XCD-aware order, as K1b
  const unsigned bid = xcd_strided(blockIdx.x, (unsigned)p.total_blocks);
  OFFK_PICK_SITE(S, p, (int)bid >= p.s[i].blk_begin)
  const int C = S.C, HW = S.HW;
  const int local = (int)bid - S.blk_begin;
  const int chunk = local / S.ntiles, nt = local - chunk * S.ntiles;
  const int kt0 = chunk * p.kt_per_blk, kt1 = min(kt0 + p.kt_per_blk, S.kt_total);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wc = wave & 3;   // MFMA role: row half, 32-channel group.  Loader role: waves 0-3 a, waves 4-7 X (group wc)
  const bool is_a = wave < 4;
  const int lt = tid & 255;                  // the thread's index in K1b's loader
  const bool vec = (HW & 3) == 0;

  // ---- the loaders: K1b's, thread for thread (units_bwd.hip) ----
  const float* xrow[4];   // block-uniform: first row of the 32-channel group inside its part
  int xfs[4];             // frame stride of the part, in elements
  bool xok[4];
  const int rowoff = (lt >> 3) * HW;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int cb = nt * WS_BN + 32 * r;
    const auto [xb, cpart, kl] = part_at(S, cb);
    xok[r] = cb < C;
    xrow[r] = FEAT == kFeatF32 ? xb + (size_t)kl * HW
                               : reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(xb) + (size_t)kl * HW);
    xfs[r] = cpart * HW;
  }
  const bool wave_on = nt * WS_BN + 32 * wc < C;   // as an X loader (channels-last) and as an MFMA wave: the same 32-channel group
  const float* xcl = nullptr;
  int xcs = 0;
  if constexpr (CL) {
    const auto [xb, cpart, kl] = part_at(S, nt * WS_BN + 32 * wc);
    xcl = FT == kFeatF32 ? xb + kl : reinterpret_cast<const float*>(reinterpret_cast<const unsigned short*>(xb) + kl);
    xcs = cpart;
  }

  const int pq = lt & 7, cq = lt >> 3;     // gen A loader (and channels-last X loader): pixel quad, channel quad
  const int dpx = lt >> 3, dcq = lt & 7;   // down A loader: pixel, channel quad
  // WS_DEPTH K-tiles in flight, one register set each.  a loader: 0-3 gen pixels, 4 down.  X loader: 0-3 X rows (K1b's rg[5..8]); one role per wave
  // (separate objects, picked by a constant: one array of sets stayed in scratch memory in one of the six forms)
  struct TileRegs {
    float4 rg[5];
    unsigned long long rx[4];              // 16-bit maps: the X quads as loaded
    int kin;                               // k offset of the tile the set holds
  } t0, t1, t2;
  auto regs = [&](auto SET) -> TileRegs& {
    if constexpr (decltype(SET)::value == 0) return t0;
    else if constexpr (decltype(SET)::value == 1) return t1;
    else return t2;
  };
  float4 bs_g = make_float4(0.f, 0.f, 0.f, 0.f), bs_d = make_float4(0.f, 0.f, 0.f, 0.f);

  int frame = kt0 / S.tpf, kin = (kt0 - frame * S.tpf) * BK;
  typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
  // Branch-free loads, as K1b's: an out-of-range piece reads the handle's zero page instead of being skipped -- and here ROLE-free too
  // wherever the two roles can share an instruction sequence: the prefetch rests on `s_waitcnt vmcnt(N)` leaving the N newest loads in
  // flight, and behind a branch whose sides issue different numbers of loads hipcc has to wait as if the fewest had been issued.  So
  // every thread issues the same loads in the same order, the pieces of the other role (and of a K-tile past the chunk's end: `valid`)
  // reading the zero page: fp32 maps: five 16-byte loads with the role's pointers selected; 16-bit maps: the five a loads, then the four
  // 8-byte X loads.  Only the 2-byte X loader of the 7x7 sites (16-bit NCHW maps, HW % 4 != 0) keeps a branch of its own.
  auto load_tile = [&](auto VT, auto SET, bool valid) {
    float4 (&rg)[5] = regs(SET).rg;
    unsigned long long (&rx)[4] = regs(SET).rx;
    regs(SET).kin = kin;
    constexpr int V = decltype(VT)::value;
    const float* qa[5];           // the a loader's five pieces: gen pixels 4 pq .. + 3 (channels 4 cq .. + 3), one down pixel
    {
      const float* ga = S.dG + ((size_t)frame * HW + kin + 4 * pq) * kGenCh + 4 * cq;
#pragma unroll
      for (int j = 0; j < 4; ++j) qa[j] = (valid && is_a && kin + 4 * pq + j < HW) ? ga + (size_t)j * kGenCh : p.zeros;
      const int dr = down_row(frame, p.L, p.P, p.slice_mode);
      qa[4] = (valid && is_a && dr >= 0 && kin + dpx < HW) ? S.dD + ((size_t)dr * HW + kin + dpx) * kDownCh + 4 * dcq : p.zeros;
    }
    const int k = kin + 4 * (lt & 7), kk = min(k, HW - 4);
    const bool xrole = valid && !is_a;
    if constexpr (FT == kFeatF32) {
      // X NCHW: quad k..k+3 of rows (lt >> 3) + 32 r; a quad that straddles the row end (HW % 4 != 0) is read from HW-4 and shifted by
      // store_tile.  X channels-last: pixel kin + 4 pq + j, channels 4 (cq & 7) .. + 3 of the wave's group; store_tile transposes
      const float* qx[4];
      if constexpr (CL) {
        const size_t px = (size_t)frame * HW + kin + 4 * pq;
#pragma unroll
        for (int j = 0; j < 4; ++j) qx[j] = (xrole && wave_on && kin + 4 * pq + j < HW) ? xcl + (px + j) * xcs + 4 * (cq & 7) : p.zeros;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) qx[r] = (xrole && xok[r] && k < HW) ? xrow[r] + (size_t)frame * xfs[r] + (rowoff + kk) : p.zeros;
      }
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const f4u v = *reinterpret_cast<const f4u*>(is_a || j == 4 ? qa[j] : qx[j & 3]);      // (7x7 maps: rows are only 4-byte aligned)
        rg[j] = make_float4(v.x, v.y, v.z, v.w);
      }
    } else if constexpr (CL || V == 1) {
#pragma unroll
      for (int j = 0; j < 5; ++j) rg[j] = *reinterpret_cast<const float4*>(qa[j]);
      const unsigned short* z16 = reinterpret_cast<const unsigned short*>(p.zeros);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned short* q;
        if constexpr (CL)
          q = (xrole && wave_on && kin + 4 * pq + j < HW)
                  ? reinterpret_cast<const unsigned short*>(xcl) + ((size_t)frame * HW + kin + 4 * pq + j) * xcs + 4 * (cq & 7) : z16;
        else
          q = (xrole && xok[j] && k < HW) ? reinterpret_cast<const unsigned short*>(xrow[j]) + (size_t)frame * xfs[j] + (rowoff + k) : z16;
        rx[j] = *reinterpret_cast<const unsigned long long*>(q);
      }
    } else {
      // 16-bit NCHW maps at the 7x7 sites (98-byte rows): four 2-byte loads per row, widened by store_tile
      if (is_a) {
#pragma unroll
        for (int j = 0; j < 5; ++j) rg[j] = *reinterpret_cast<const float4*>(qa[j]);
      } else {
        const unsigned short* z16 = reinterpret_cast<const unsigned short*>(p.zeros);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const unsigned short* row = reinterpret_cast<const unsigned short*>(xrow[r]) + (size_t)frame * xfs[r] + (rowoff + k);
          const bool on = valid && xok[r];
          const unsigned e0 = *((on && k < HW) ? row : z16), e1 = *((on && k + 1 < HW) ? row + 1 : z16);
          const unsigned e2 = *((on && k + 2 < HW) ? row + 2 : z16), e3 = *((on && k + 3 < HW) ? row + 3 : z16);
          rg[r] = make_float4(__uint_as_float(e0), __uint_as_float(e1), __uint_as_float(e2), __uint_as_float(e3));
        }
      }
    }
  };
  auto fix_x_tail = [&](float4 (&rg)[5], int kin_ld) {   // HW % 4 != 0 only: the quad was loaded `sh` floats early
    const int k = kin_ld + 4 * (lt & 7);
    const int sh = k < HW ? k - min(k, HW - 4) : 0;
    if (sh) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float4 v = rg[r];
        rg[r] = sh == 1 ? make_float4(v.y, v.z, v.w, 0.f) : (sh == 2 ? make_float4(v.z, v.w, 0.f, 0.f) : make_float4(v.w, 0.f, 0.f, 0.f));
      }
    }
  };
  // where the 8 bytes of (row, pixel quad kq) lie in a plane image; swz_shift: see the head of the file
  auto quad_at = [](char* img, int row, int kq, int swz_shift) {
    const int kg = kq >> 1;
    return img + (row >> 4) * WS_PIECE + kg * 256 + (((row & 15) ^ (kg << swz_shift)) << 4) + (kq & 1) * 8;
  };
  // the tile held in rg[] / rx[] -> plane images of buffer `buf`
  auto store_tile = [&](auto VT, auto SET, char* buf) {
    float4 (&rg)[5] = regs(SET).rg;
    unsigned long long (&rx)[4] = regs(SET).rx;
    char* const Ap = buf;
    char* const Xp = buf + 3 * WS_APLANE;
    if (is_a) {
      // the bias sums: K1b's, in K1b's order, on the operand before the cut
      bs_g.x += (rg[0].x + rg[1].x) + (rg[2].x + rg[3].x); bs_g.y += (rg[0].y + rg[1].y) + (rg[2].y + rg[3].y);
      bs_g.z += (rg[0].z + rg[1].z) + (rg[2].z + rg[3].z); bs_g.w += (rg[0].w + rg[1].w) + (rg[2].w + rg[3].w);
      bs_d.x += rg[4].x; bs_d.y += rg[4].y; bs_d.z += rg[4].z; bs_d.w += rg[4].w;
      // gen: pixel j's four channels -> channel i's four pixels, as K1b transposes them
      sp_store_quad<3>(quad_at(Ap, 4 * cq, pq, 0), WS_APLANE, rg[0].x, rg[1].x, rg[2].x, rg[3].x);
      sp_store_quad<3>(quad_at(Ap, 4 * cq + 1, pq, 0), WS_APLANE, rg[0].y, rg[1].y, rg[2].y, rg[3].y);
      sp_store_quad<3>(quad_at(Ap, 4 * cq + 2, pq, 0), WS_APLANE, rg[0].z, rg[1].z, rg[2].z, rg[3].z);
      sp_store_quad<3>(quad_at(Ap, 4 * cq + 3, pq, 0), WS_APLANE, rg[0].w, rg[1].w, rg[2].w, rg[3].w);
      // down: one pixel (k = dpx), rows 128 + 4 dcq .. + 3: one 16-bit word per row and plane
      const int kg = dpx >> 3;
      const float dv[4] = {rg[4].x, rg[4].y, rg[4].z, rg[4].w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = kGenCh + 4 * dcq + i;
        unsigned h, m, l;
        sp_cut(dv[i], h, m, l);
        char* dst = Ap + (row >> 4) * WS_PIECE + kg * 256 + (((row & 15) ^ kg) << 4) + (dpx & 7) * 2;
        *reinterpret_cast<unsigned short*>(dst) = (unsigned short)(h >> 16);
        *reinterpret_cast<unsigned short*>(dst + WS_APLANE) = (unsigned short)(m >> 16);
        *reinterpret_cast<unsigned short*>(dst + 2 * WS_APLANE) = (unsigned short)(l >> 16);
      }
      return;
    }
    if constexpr (CL) {
      // pixel j's four channels -> channel i's four pixels (the transpose of K1b's channels-last loader), cut on the way
      if constexpr (FT != kFeatF32) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const unsigned a = (unsigned)rx[j], b = (unsigned)(rx[j] >> 32);
          rg[j] = widen16x4<FT>(a, b);
        }
      }
      sp_store_quad<NPX>(quad_at(Xp, 4 * cq, pq, 0), WS_XPLANE, rg[0].x, rg[1].x, rg[2].x, rg[3].x);
      sp_store_quad<NPX>(quad_at(Xp, 4 * cq + 1, pq, 0), WS_XPLANE, rg[0].y, rg[1].y, rg[2].y, rg[3].y);
      sp_store_quad<NPX>(quad_at(Xp, 4 * cq + 2, pq, 0), WS_XPLANE, rg[0].z, rg[1].z, rg[2].z, rg[3].z);
      sp_store_quad<NPX>(quad_at(Xp, 4 * cq + 3, pq, 0), WS_XPLANE, rg[0].w, rg[1].w, rg[2].w, rg[3].w);
    } else {
      if constexpr (FEAT != kFeatF32) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (decltype(VT)::value == 1) {
            const unsigned a = (unsigned)rx[r], b = (unsigned)(rx[r] >> 32);
            rg[r] = widen16x4<FT>(a, b);
          } else {
            rg[r] = make_float4(widen16<FT>(__float_as_uint(rg[r].x)), widen16<FT>(__float_as_uint(rg[r].y)),
                                widen16<FT>(__float_as_uint(rg[r].z)), widen16<FT>(__float_as_uint(rg[r].w)));
          }
        }
      } else {
        if (!vec) fix_x_tail(rg, regs(SET).kin);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sp_store_quad<NPX>(quad_at(Xp, (lt >> 3) + 32 * r, lt & 7, 1), WS_XPLANE, rg[r].x, rg[r].y, rg[r].z, rg[r].w);
    }
  };

  // accumulators [row tile][channel tile]: A1 = sum a_h x_h, A2 = the small products
  spf4 a1[WS_MT][2], a2[WS_MT][2];
#pragma unroll
  for (int mt = 0; mt < WS_MT; ++mt)
#pragma unroll
    for (int j = 0; j < 2; ++j) { a1[mt][j] = spf4{0.f, 0.f, 0.f, 0.f}; a2[mt][j] = spf4{0.f, 0.f, 0.f, 0.f}; }

  const int lr16 = lane & 15, lq = lane >> 4;
  // operand offsets inside a buffer: a + mt * WS_PIECE + plane * WS_APLANE, X + j * WS_PIECE + plane * WS_XPLANE
  const int aoff = wm * WS_MT * WS_PIECE + lq * 256 + ((lr16 ^ lq) << 4);
  const int xoff = 3 * WS_APLANE + (2 * wc) * WS_PIECE + lq * 256 + ((lr16 ^ (lq << (CL ? 0 : 1))) << 4);

  auto mma_tile = [&](const char* buf) {
    spu4 xb[2][NPX];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < NPX; ++q) xb[j][q] = *reinterpret_cast<const spu4*>(buf + xoff + j * WS_PIECE + q * WS_XPLANE);
    // the a operands of row tile mt + 1 are read BEFORE the MFMAs of row tile mt (two register sets, a scheduling barrier pins the order,
    // as units_dx_split_kernel does)
    spu4 ab[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) ab[0][q] = *reinterpret_cast<const spu4*>(buf + aoff + q * WS_APLANE);
#pragma unroll
    for (int mt = 0; mt < WS_MT; ++mt) {
      spu4 (&a)[3] = ab[mt & 1];
      if (mt + 1 < WS_MT) {
#pragma unroll
        for (int q = 0; q < 3; ++q) ab[(mt + 1) & 1][q] = *reinterpret_cast<const spu4*>(buf + aoff + (mt + 1) * WS_PIECE + q * WS_APLANE);
      }
      __builtin_amdgcn_sched_barrier(0);
      // synth.SPLIT_PRODUCTS order (a plane, x plane): (2, 0), (0, 2), (1, 1), (1, 0), (0, 1) -> A2; (0, 0) -> A1.  A product with a plane
      // the map's type does not have is not issued (it would add +-0)
#pragma unroll
      for (int j = 0; j < 2; ++j) sp_mfma(a2[mt][j], a[2], xb[j][0]);
      if constexpr (NPX > 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[mt][j], a[0], xb[j][NPX > 2 ? 2 : 0]);
      }
      if constexpr (NPX > 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[mt][j], a[1], xb[j][NPX > 1 ? 1 : 0]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) sp_mfma(a2[mt][j], a[1], xb[j][0]);
      if constexpr (NPX > 1) {
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[mt][j], a[0], xb[j][NPX > 1 ? 1 : 0]);
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) sp_mfma(a1[mt][j], a[0], xb[j][0]);
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // K-tile kt lives in buffer (kt - kt0) & 1 and came through register set (kt - kt0) % WS_DEPTH.  A step: load K-tile kt + WS_DEPTH into the
  // set K-tile kt left, MFMAs of K-tile kt, cut K-tile kt + 1 into the other buffer -- whose last readers (the MFMAs of K-tile kt - 1) are
  // behind the barrier that ended the previous step -- and one barrier.  (Fully unrolled over the sets: every set index is a constant.)
  auto next_tile = [&]() {
    kin += BK;
    if (kin >= HW) { kin = 0; ++frame; }
  };
  auto k_loop = [&](auto VT) {
    // (the loads of a step are unconditional: a K-tile past the chunk's end reads the zero page and is never stored)
    load_tile(VT, WsVec<0>(), true);
    next_tile();
    load_tile(VT, WsVec<1 % WS_DEPTH>(), kt0 + 1 < kt1);
    if constexpr (WS_DEPTH > 2) {
      next_tile();
      load_tile(VT, WsVec<2 % WS_DEPTH>(), kt0 + 2 < kt1);
    }
    store_tile(VT, WsVec<0>(), lds_raw);
    __syncthreads();
    auto step = [&](int kt, auto SET) {
      constexpr int S = decltype(SET)::value;
      const int cur = (kt - kt0) & 1;
      next_tile();
      load_tile(VT, SET, kt + WS_DEPTH < kt1);
      if (wave_on) mma_tile(lds_raw + cur * BUF_BYTES);
      if (kt + 1 < kt1) store_tile(VT, WsVec<(S + 1) % WS_DEPTH>(), lds_raw + (cur ^ 1) * BUF_BYTES);
      __syncthreads();
    };
    for (int kt = kt0; kt < kt1; kt += WS_DEPTH) {      // (every condition here is block-uniform)
      step(kt, WsVec<0>());
      if (kt + 1 >= kt1) break;
      step(kt + 1, WsVec<1 % WS_DEPTH>());
      if constexpr (WS_DEPTH > 2) {
        if (kt + 2 >= kt1) break;
        step(kt + 2, WsVec<2 % WS_DEPTH>());
      }
    }
  };
  // one K loop per X loader form (a block-uniform choice), as K1b
  if constexpr (CL) k_loop(WsVec<2>());
  else if constexpr (FEAT == kFeatF32) k_loop(WsVec<-1>());
  else if (vec) k_loop(WsVec<1>());
  else k_loop(WsVec<0>());

  // ---- epilogue: partial tile -> slab [chunk][160][ntiles*128]; (a1 + a2)[mt][j][i] = row 80 wm + 16 mt + 4 lq + i, channel 32 wc + 16 j + lr16 ----
  const int cpad = S.ntiles * WS_BN;
  if (wave_on) {
    float* out = S.slab + (size_t)chunk * WS_BM * cpad + nt * WS_BN + wc * 32 + lr16;
#pragma unroll
    for (int mt = 0; mt < WS_MT; ++mt)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const spf4 v = a1[mt][j] + a2[mt][j];
#pragma unroll
        for (int i = 0; i < 4; ++i) out[(size_t)((wm * WS_MT + mt) * 16 + 4 * lq + i) * cpad + 16 * j] = v[i];
      }
  }
  // ---- bias partials (first channel slab only): K1b's reduction of K1b's sums (the K loop ended with a barrier) ----
  if (nt == 0) {
    float* red = reinterpret_cast<float*>(lds_raw);   // [8][128] gen, then [32][32] down
    if (is_a) {
      *reinterpret_cast<float4*>(red + pq * kGenCh + 4 * cq) = bs_g;
      *reinterpret_cast<float4*>(red + 8 * kGenCh + dpx * kDownCh + 4 * dcq) = bs_d;
    }
    __syncthreads();
    if (tid < kGenCh) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) s += red[i * kGenCh + tid];
      S.bpart[(size_t)chunk * WS_BM + tid] = s;
    } else if (tid < WS_BM) {
      float s = 0.f;
#pragma unroll 8
      for (int i = 0; i < 32; ++i) s += red[8 * kGenCh + i * kDownCh + (tid - kGenCh)];
      S.bpart[(size_t)chunk * WS_BM + tid] = s;
    }
  }
}

template <int FEAT>
static hipError_t ws_launch(const WgParams& p, hipStream_t st) {
  constexpr int FT = FEAT & ~kFeatCl;
  constexpr int lds = 2 * (3 * WS_APLANE + (FT == kFeatBf16 ? 1 : (FT == kFeatF16 ? 2 : 3)) * WS_XPLANE);
  hipError_t e = lds_attr_once(reinterpret_cast<const void*>(pw_wgrad_split_kernel<FEAT>), lds);
  if (e != hipSuccess) return e;                                 // nothing enqueued yet
  hipLaunchKernelGGL(pw_wgrad_split_kernel<FEAT>, dim3(p.total_blocks), dim3(WS_THREADS), lds, st, p);
  return hipGetLastError();
}

// feat_dtype: kFeatF32 / kFeatBf16 / kFeatF16; cl: channels-last maps (xp[] as pw_wgrad_cl_launch wants them, else as pw_wgrad_launch /
// pw_wgrad_feat16_launch do)
hipError_t pw_wgrad_split_launch(const WgParams& p, int feat_dtype, bool cl, hipStream_t st) {
  if (p.total_blocks <= 0) return hipSuccess;
  switch (feat_dtype) {
    case kFeatF32: return cl ? ws_launch<kFeatF32 | kFeatCl>(p, st) : ws_launch<kFeatF32>(p, st);
    case kFeatBf16: return cl ? ws_launch<kFeatBf16 | kFeatCl>(p, st) : ws_launch<kFeatBf16>(p, st);
    case kFeatF16: return cl ? ws_launch<kFeatF16 | kFeatCl>(p, st) : ws_launch<kFeatF16>(p, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace offk
