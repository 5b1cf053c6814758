// The feature-map gradient of the OFF units in split-fp32 arithmetic (offk_off_units_backward_feats_split): units_dx.hip's GEMM
//   dX[n, q, c] = sum_{k < 160} a[n HW + q, k] w[c, k],   a = [dGpre (k 0..127) | dD at row r(n) (k 128..159)],  w[c] = [Wg[:, c] ; Wd[:, c]]
// on the bf16 matrix pipe, DESIGN.md 5.1: both operands are cut into THREE bf16 planes by truncation (h = the upper 16 bits of the word, the
// remainder is exact in fp32, cut again, and again; synth.cut3), and per 32-k step six of the nine plane products are issued on
// v_mfma_f32_16x16x32_bf16 in synth.SPLIT_PRODUCTS order -- w_l a_h, w_h a_l, w_m a_m, w_m a_h, w_h a_m into accumulator A2, w_h a_h into A1 --
// five steps in increasing k (gen channels, then down), out = A1 + A2 once in the epilogue: synth.emulate_split_dot(form="units"), K = 160.
// No split-K, no atomics, one fixed order: bit-reproducible.  r(n) is down_row of offk_common.h; a frame outside the slice multiplies
// zeros (the cut of 0 is 0), rows past the site's end are zeros too and store nothing.
//
// TWO launches on the caller's stream (units_dx_split_launch):
//   1. units_dx_split_pack_kernel cuts [Wg ; Wd] of the requested sites, as they are at launch time, into the operand-order plane image
//      [16-channel tile][k step 5][plane 3][lane 64] x 16 B (960 B per channel, 5.3 MB for all nine sites, a buffer of the handle):
//      lane l of a tile's piece holds channel l & 15, k = 32 step + 8 (l >> 4) .. + 7 -- the A operand of the MFMA as it lies;
//   2. units_dx_split_kernel: a block owns 128 consecutive (frame, pixel) rows of one site.  It cuts a = [dGpre | dD] of those rows ONCE
//      while staging them into three LDS plane images ([16-row tile][k group of 8][16 rows] x 16 B: a wave's ds_read_b128 of one tile and
//      k step is 1 KB contiguous, conflict-free; 3 x 40960 B = 122880 B) and sweeps the channel tiles of 64 with them.  Wave (wr, wc) holds
//      rows 64 wr .. + 63 x channels 32 wc .. + 31 of the tile: 4 row tiles x 2 channel tiles x (A1, A2) = 64 accumulator registers.  The
//      weight operands come from the plane image (L2) straight into registers, one k step ahead of their use (24 registers in flight, the
//      index clamped at the end: no conditional prefetch), so the channel sweep needs no LDS for them and NO block-wide barrier: after
//      the one barrier behind the staging the four waves run on their own.  The row operands are read from LDS one 16-row step ahead
//      of their MFMAs.  One block per CU (128 rows halve the weight re-reads of a 64-row block: C x 960 B per block, about 3.8 GB per
//      launch at B = 64 x 7); weight bytes per MFMA through the L1: 6144 B / 48 = 128 B.
//
// Weights are the A operand, rows the B operand: a lane ends with FOUR consecutive channels of one row.  NHWC stores them as they lie (16 B,
// 8 B for a 16-bit dtype); NCHW turns the wave's 64 x 32 tile through a wave-private LDS image (row stride 68 words: conflict-free both ways)
// so that the stores run along the pixel axis, element by element (the 49-element rows of the 7x7 sites are only element-aligned).  The
// six output forms share everything up to the accumulators; the epilogues are units_dx.hip's contracts: fp32 stores the sum, a 16-bit form
// rounds each finished fp32 sum ONCE to nearest-even (v_cvt_pk_bf16_f32 / v_cvt_f16_f32), accumulate stores old + new, respectively
// rne16(widen(old) + new).
#include "units_common.h"
#include "split_common.h"

namespace offk {
namespace {

constexpr int XS_BM = 128, XS_BN = 64, XS_THREADS = 256, XS_KSTEPS = kUnitCh / 32;
constexpr int XS_RT_BYTES = (kUnitCh / 8) * 16 * 16;        // one 16-row tile of one plane: 20 k groups x 16 rows x 16 B
constexpr int XS_PLANE = (XS_BM / 16) * XS_RT_BYTES;        // 40960
constexpr int XS_A_BYTES = 3 * XS_PLANE;                    // 122880 = 96 granules of 1280 B
constexpr int XS_TS = 68;                                   // row stride (words) of a wave's transpose image [32 channels][64 rows]
constexpr int XS_T_BYTES = (XS_THREADS / 64) * 32 * XS_TS * 4;
constexpr int XS_WPIECE = 1024;                             // one (16-channel tile, k step, plane) piece of the weight image
static_assert(XS_A_BYTES + XS_T_BYTES <= 160 * 1024, "one block per CU");
static_assert(kUnitCh % 32 == 0 && kGenCh % 32 == 0, "whole k steps, gen / down split on a step boundary");

template <int OUT>
__device__ __forceinline__ unsigned xs_pack16(float lo, float hi) {     // element lo in bits 0..15 (the lower address)
  if constexpr (OUT == kFeatBf16) {
    unsigned r;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
    return r;
  } else {
    const _Float16 l = (_Float16)lo, u = (_Float16)hi;                   // v_cvt_f16_f32 under the default (nearest-even) mode
    return (unsigned)__builtin_bit_cast(unsigned short, l) | ((unsigned)__builtin_bit_cast(unsigned short, u) << 16);
  }
}
template <int OUT>
__device__ __forceinline__ unsigned short xs_round16(float v) {
  if constexpr (OUT == kFeatBf16) return (unsigned short)(xs_pack16<OUT>(v, 0.f) & 0xFFFFu);
  else return __builtin_bit_cast(unsigned short, (_Float16)v);
}

}  // namespace

// ---- 1. the weight pre-pass: [Wg ; Wd] as they are NOW -> plane image.  One wave per (16-channel tile, k step) of a site ----
__global__ __launch_bounds__(XS_THREADS) void units_dx_split_pack_kernel(DxsParams p) {
  const int bid = (int)blockIdx.x;
  const float *wg = p.s[0].wg, *wd = p.s[0].wd;
  char* img = static_cast<char*>(p.s[0].wimg);
  int C = p.s[0].C, begin = 0;
#pragma unroll
  for (int i = 1; i < kNumSites; ++i)
    if (i < p.nsites && bid >= p.s[i].pack_begin) { wg = p.s[i].wg; wd = p.s[i].wd; img = static_cast<char*>(p.s[i].wimg); C = p.s[i].C; begin = p.s[i].pack_begin; }
  const int lane = threadIdx.x & 63;
  const int u = (bid - begin) * (XS_THREADS / 64) + ((int)threadIdx.x >> 6);
  if (u >= (C / 16) * XS_KSTEPS) return;
  const int ch16 = u / XS_KSTEPS, ks = u - ch16 * XS_KSTEPS;
  const int c = ch16 * 16 + (lane & 15), k0 = 32 * ks + 8 * (lane >> 4);          // eight k of one channel: all gen or all down
  const float* src = k0 < kGenCh ? wg + (size_t)k0 * C + c : wd + (size_t)(k0 - kGenCh) * C + c;
  unsigned h[8], m[8], l[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) sp_cut(src[(size_t)j * C], h[j], m[j], l[j]);
  char* dst = img + (size_t)(ch16 * XS_KSTEPS + ks) * 3 * XS_WPIECE + lane * 16;
  *reinterpret_cast<spu4*>(dst) = spu4{sp_pair(h[0], h[1]), sp_pair(h[2], h[3]), sp_pair(h[4], h[5]), sp_pair(h[6], h[7])};
  *reinterpret_cast<spu4*>(dst + XS_WPIECE) = spu4{sp_pair(m[0], m[1]), sp_pair(m[2], m[3]), sp_pair(m[4], m[5]), sp_pair(m[6], m[7])};
  *reinterpret_cast<spu4*>(dst + 2 * XS_WPIECE) = spu4{sp_pair(l[0], l[1]), sp_pair(l[2], l[3]), sp_pair(l[4], l[5]), sp_pair(l[6], l[7])};
}

// ---- 2. the GEMM ----
template <bool NCHW, int OUT>
__global__ __launch_bounds__(XS_THREADS, 1) void units_dx_split_kernel(DxsParams p) {
  extern __shared__ __attribute__((aligned(16))) char xs_lds[];
  char* const Ap = xs_lds;                                        // three plane images of the block's 128 rows
  float* const Ts = reinterpret_cast<float*>(xs_lds + XS_A_BYTES);  // NCHW: [4 waves][32][XS_TS]

  const int bid = (int)blockIdx.x;
  OFFK_PICK_SITE(S, p, bid >= p.s[i].blk_begin)
  const int C = S.C, HW = S.HW, M = S.M;
  const int row0 = (bid - S.blk_begin) * XS_BM;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: what depends on it alone is decided on the scalar unit
  const int wr = wave >> 1, wc = wave & 1;                        // the wave's 64 rows x 32 channels of the 128 x 64 tile
  const int nct = (C + XS_BN - 1) / XS_BN, nch16 = C / 16;
  const int last_step = nct * XS_KSTEPS - 1;

  // weight operands of one k step: 2 channel tiles x 3 planes, 16 B per lane each, from the plane image (index clamped, never conditional)
  const char* const wsrc = static_cast<const char*>(S.wimg) + lane * 16;
  auto load_w = [&](spu4 (&w)[2][3], int step) {
    step = min(step, last_step);
    const int ct = step / XS_KSTEPS, ks = step - ct * XS_KSTEPS;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int ch16 = min(ct * 4 + wc * 2 + j, nch16 - 1);
#pragma unroll
      for (int q = 0; q < 3; ++q) w[j][q] = *reinterpret_cast<const spu4*>(wsrc + (size_t)((ch16 * XS_KSTEPS + ks) * 3 + q) * XS_WPIECE);
    }
  };
  spu4 wn[2][3];
  load_w(wn, 0);

  // ---- a = [dGpre | dD] of the block's rows, cut while staged (branch-free loads: what is masked out reads the zero page).  Unit
  //      u = wave + 4 i of 80: 16 rows (one row tile) x 16 k; a lane takes four k of one row: 64 B contiguous per row and lane quad ----
  {
    constexpr int NU = (XS_BM / 16) * (kUnitCh / 16) / (XS_THREADS / 64);     // 20 units per wave
    spf4 areg[NU];
    const int lr = lane >> 2, lc = lane & 3;
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = wave + 4 * i, rt = u / (kUnitCh / 16), cg = u - rt * (kUnitCh / 16);
      const int row = row0 + rt * 16 + lr, k = cg * 16 + 4 * lc;
      const float* src = p.zeros;
      if (cg < kGenCh / 16) {                                     // wave-uniform
        if (row < M) src = S.dG + (size_t)row * kGenCh + k;
      } else {
        const int f = row / HW, px = row - f * HW;
        const int dr = down_row(f, p.L, p.P, p.slice_mode);
        if (row < M && dr >= 0) src = S.dD + ((size_t)dr * HW + px) * kDownCh + (k - kGenCh);
      }
      areg[i] = *reinterpret_cast<const spf4*>(src);
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      const int u = wave + 4 * i, rt = u / (kUnitCh / 16), cg = u - rt * (kUnitCh / 16);
      unsigned h[4], m[4], l[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) sp_cut(areg[i][j], h[j], m[j], l[j]);
      char* dst = Ap + rt * XS_RT_BYTES + (cg * 2 + (lc >> 1)) * 256 + lr * 16 + (lc & 1) * 8;
      sp_store_quad<3>(dst, XS_PLANE, h, m, l);
    }
  }
  __syncthreads();                   // the only block-wide barrier: the plane images are in place

  const int lr16 = lane & 15, lq = lane >> 4;
  const char* const xsrc = Ap + wr * 4 * XS_RT_BYTES + lane * 16;     // + rt * XS_RT_BYTES + ks * 1024 + plane * XS_PLANE
  float* const T = Ts + wave * 32 * XS_TS;
  // NCHW epilogue: the lane's row of the wave tile and where its pixel lies
  const int erow = row0 + wr * 64 + lane;
  const int ef = erow / HW, epx = erow - ef * HW;

  // B operand (rows) of step s = 4 ks + rt of a channel tile: three ds_read_b128.  The reads of step s + 1 are issued BEFORE the MFMAs of step
  // s (two register sets, a scheduling barrier pins the order, as WaveAcc::mma_ktile does): with one wave per SIMD nothing else hides an
  // LDS latency.  The plane images serve every channel tile, so the last step of a tile reads step 0 of the next.
  auto rdx = [&](spu4 (&x)[3], int s) {
#pragma unroll
    for (int q = 0; q < 3; ++q) x[q] = *reinterpret_cast<const spu4*>(xsrc + (s & 3) * XS_RT_BYTES + (s >> 2) * 1024 + q * XS_PLANE);
  };
  spu4 xb[2][3];
  rdx(xb[0], 0);

  for (int ct = 0; ct < nct; ++ct) {
    const int cbase = ct * XS_BN + wc * 32;
    if (cbase >= C) break;           // wave-uniform: the half tile past C (C % 64 == 32) is the last one; no barrier follows

    spf4 a1[4][2], a2[4][2];         // [row tile][channel tile]: A1 = sum w_h a_h, A2 = the five small products
#pragma unroll
    for (int rt = 0; rt < 4; ++rt)
#pragma unroll
      for (int j = 0; j < 2; ++j) { a1[rt][j] = spf4{0.f, 0.f, 0.f, 0.f}; a2[rt][j] = spf4{0.f, 0.f, 0.f, 0.f}; }

#pragma unroll
    for (int ks = 0; ks < XS_KSTEPS; ++ks) {
      spu4 w[2][3];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) w[j][q] = wn[j][q];
      load_w(wn, ct * XS_KSTEPS + ks + 1);
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        constexpr int NS = 4 * XS_KSTEPS;
        const int s = 4 * ks + rt;                       // (even: 20 steps per tile, the register sets keep their parity across tiles)
        spu4 (&x)[3] = xb[s & 1];
        rdx(xb[(s + 1) & 1], (s + 1) % NS);
        __builtin_amdgcn_sched_barrier(0);
        // synth.SPLIT_PRODUCTS order (w plane, a plane): (2, 0), (0, 2), (1, 1), (1, 0), (0, 1) -> A2; (0, 0) -> A1
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[rt][j], w[j][2], x[0]);
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[rt][j], w[j][0], x[2]);
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[rt][j], w[j][1], x[1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[rt][j], w[j][1], x[0]);
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a2[rt][j], w[j][0], x[1]);
#pragma unroll
        for (int j = 0; j < 2; ++j) sp_mfma(a1[rt][j], w[j][0], x[0]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }

    // ---- epilogue: (a1 + a2)[rt][j][i] = row wr * 64 + rt * 16 + lr16, channel cbase + 16 j + 4 lq + i ----
    if constexpr (!NCHW) {
#pragma unroll
      for (int rt = 0; rt < 4; ++rt) {
        const int row = row0 + wr * 64 + rt * 16 + lr16;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          spf4 v = a1[rt][j] + a2[rt][j];
          const size_t at = (size_t)row * C + cbase + 16 * j + 4 * lq;      // a multiple of 4 elements: 16-byte / 8-byte aligned
          if (row < M) {
            if constexpr (OUT == kFeatF32) {
              spf4* o = reinterpret_cast<spf4*>(static_cast<float*>(S.out) + at);
              if (p.accumulate) v = *o + v;
              *o = v;
            } else {
              spu2* o = reinterpret_cast<spu2*>(static_cast<unsigned short*>(S.out) + at);
              if (p.accumulate) {
                const spu2 old = *o;
                v[0] += widen16<OUT>((unsigned short)(old[0] & 0xFFFFu));
                v[1] += widen16<OUT>((unsigned short)(old[0] >> 16));
                v[2] += widen16<OUT>((unsigned short)(old[1] & 0xFFFFu));
                v[3] += widen16<OUT>((unsigned short)(old[1] >> 16));
              }
              *o = spu2{xs_pack16<OUT>(v[0], v[1]), xs_pack16<OUT>(v[2], v[3])};
            }
          }
        }
      }
    } else {
      // wave-private turn: [channel][row] image, then lanes along the rows.  One wave's LDS operations complete in order; the fences
      // keep the compiler from moving the reads over the writes (and the next tile's writes over these reads)
#pragma unroll
      for (int rt = 0; rt < 4; ++rt)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const spf4 v = a1[rt][j] + a2[rt][j];
#pragma unroll
          for (int i = 0; i < 4; ++i) T[(16 * j + 4 * lq + i) * XS_TS + rt * 16 + lr16] = v[i];
        }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if (erow < M) {
        const size_t at = ((size_t)ef * C + cbase) * HW + epx;
        if constexpr (OUT == kFeatF32) {
          float* o = static_cast<float*>(S.out) + at;
#pragma unroll 8
          for (int ch = 0; ch < 32; ++ch) {
            const float v = T[ch * XS_TS + lane];
            float* oc = o + (size_t)ch * HW;
            *oc = p.accumulate ? *oc + v : v;
          }
        } else {
          unsigned short* o = static_cast<unsigned short*>(S.out) + at;
#pragma unroll 8
          for (int ch = 0; ch < 32; ++ch) {
            const float v = T[ch * XS_TS + lane];
            unsigned short* oc = o + (size_t)ch * HW;
            *oc = xs_round16<OUT>(p.accumulate ? widen16<OUT>(*oc) + v : v);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

template <bool NCHW, int OUT>
static hipError_t xs_launch(const DxsParams& p, hipStream_t st) {
  constexpr int lds = XS_A_BYTES + (NCHW ? XS_T_BYTES : 0);
  hipError_t e = lds_attr_once(reinterpret_cast<const void*>(units_dx_split_kernel<NCHW, OUT>), lds);
  if (e != hipSuccess) return e;                                 // nothing enqueued yet
  hipLaunchKernelGGL(units_dx_split_pack_kernel, dim3(p.pack_blocks), dim3(XS_THREADS), 0, st, p);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((units_dx_split_kernel<NCHW, OUT>), dim3(p.total_blocks), dim3(XS_THREADS), lds, st, p);
  return hipGetLastError();
}

hipError_t units_dx_split_launch(const DxsParams& p, hipStream_t st) {
  if (p.total_blocks <= 0 || p.pack_blocks <= 0) return hipSuccess;
  switch (p.out_dtype) {
    case kFeatF32: return p.nchw ? xs_launch<true, kFeatF32>(p, st) : xs_launch<false, kFeatF32>(p, st);
    case kFeatBf16: return p.nchw ? xs_launch<true, kFeatBf16>(p, st) : xs_launch<false, kFeatBf16>(p, st);
    case kFeatF16: return p.nchw ? xs_launch<true, kFeatF16>(p, st) : xs_launch<false, kFeatF16>(p, st);
  }
  return hipErrorInvalidValue;
}

int units_dx_split_rows_per_block() { return XS_BM; }
int units_dx_split_pack_blocks(int C) { return ((C / 16) * XS_KSTEPS + XS_THREADS / 64 - 1) / (XS_THREADS / 64); }
size_t units_dx_split_image_bytes(int C) { return (size_t)C * kUnitCh * 6; }

}  // namespace offk
