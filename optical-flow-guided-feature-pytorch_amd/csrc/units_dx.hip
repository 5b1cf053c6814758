// Training side of the OFF units: the gradient w.r.t. the nine feature maps (offk_off_units_backward_feats).
//   dX[frame n, pixel q, c] = sum_o dGpre[n, q, o] Wg[o, c] + sum_j dD[r(n), q, j] Wd[j, c]
// from what K2b (units_bwd.hip) left in the train workspace -- dG_<site> [N*HW][128], dD_<site> [P*HW][32] -- and the gen / down
// weights as fp32 rows [128][C] / [32][C].  r(n) is the row of frame n in the spatial slice (down_row of offk_common.h: flat slice
// r = n for n < P; per-clip slice: frame (b, t), t < L - 1 -> b (L - 1) + t), none for a frame outside the slice.
//
// Per site a GEMM [N*HW rows] x [K = 160] x [C], all requested sites in ONE grouped launch.  A block owns DX_BM = 128 consecutive
// (frame, pixel) rows of one site: it stages A = [dGpre | dD] of those rows ONCE into LDS ([row][k], the image the fp32 MFMA core
// wants) and sweeps the channel tiles of DX_BN = 64; the weight tile [160][64] is copied to LDS as it lies in memory ([k][c]; the
// B operand of v_mfma_f32_32x32x2_f32 is one float per lane, lanes along c: conflict-free scalar reads), the next tile's loads
// in flight behind the current tile's MFMAs.  dG / dD are read once, dX is written once, W is re-read from L2 per block.
//
// Frames outside the slice MULTIPLY ZEROS: their rows carry zeros in k = 128..159 (read from the zero page), every row runs
// the same 160 k-steps.  Rows past the site's end are zeros too and store nothing; channels past C (C % 32 == 0, the tile is
// 64 wide) load zeros and their wave neither multiplies nor stores.
//
// Exact fp32 on v_mfma_f32_32x32x2_f32, fixed k order (group g of eight k: lanes 0-31 take k = 8 g + e, lanes 32-63 k = 8 g + 4 + e,
// e = 0..3), no atomics, no split-K: bit-reproducible.  The two output layouts share everything up to the accumulators; NHWC
// stores them as they lie (lanes along c), NCHW turns the wave's 64 x 32 tile through a wave-private LDS image so that the
// stores run along the pixel axis (scalar stores: the 49-float rows of the 7x7 sites are only 4-byte aligned and a tile crosses
// image boundaries there).  accumulate adds the finished sum to what is there: out = old + new, new the overwrite form's bits.
//
// 16-bit dX (offk_off_units_backward_feats_typed, OUT = kFeatBf16 / kFeatF16): the same body up to the accumulators; the epilogue
// rounds each finished fp32 sum ONCE, to nearest-even, and stores 16-bit elements (accumulate: rne16(widen(old) + new), one fp32
// add of the exactly widened old element, one rounding).  NHWC: lane pairs (2 j, 2 j + 1) exchange one register of two (DPP
// quad_perm [1, 0, 3, 2]) -- the even lane ends with channels (c, c + 1) of the first register's row, the odd lane with
// (c - 1, c) of the second's -- and every lane issues ONE aligned 4-byte store per register pair: 16 stores per wave tile, not 32.
// NCHW: the turn through Ts carries the fp32 sums, the lanes round what they read back and store 2-byte elements along the pixel
// axis (the 98-byte rows of the 7x7 sites are only 2-byte aligned).
//
// This file is compiled twice: as it is (the two fp32 kernels and units_dx_launch), and through units_dx_f16.hip with
// OFFK_UNITS_DX_F16 defined (the four 16-bit kernels and units_dx16_launch alone), so that the fp32 kernels keep the code they have.
#include "units_common.h"

namespace offk {
namespace {

constexpr int DX_BM = 128, DX_BN = 64, DX_THREADS = 256;
constexpr int DX_AS = kUnitCh + 4;       // row stride of the A image: 164 = 36 mod 64 words, the conflict-free stride of offk_common.h
constexpr int DX_TS = 2 * 32 + 1;        // row stride of a wave's transpose image [32 channels][64 rows]
constexpr int DX_A4 = kUnitCh / 4;       // float4 pieces of an A row
constexpr int DX_LDS_FLOATS = DX_BM * DX_AS + kUnitCh * DX_BN + (DX_THREADS / 64) * 32 * DX_TS;
static_assert(DX_LDS_FLOATS * 4 <= 160 * 1024, "one block per CU");
static_assert(DX_BM * DX_A4 % DX_THREADS == 0 && kUnitCh * DX_BN / 4 % DX_THREADS == 0, "whole loader rounds");

typedef float dxf4 __attribute__((ext_vector_type(4)));

// ---- 16-bit output elements: one rounding to nearest-even, exact widening ----
template <int OUT>
__device__ __forceinline__ unsigned dx_pack16(float lo, float hi) {     // element lo in bits 0..15 (the lower address)
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
__device__ __forceinline__ unsigned short dx_round16(float v) {
  if constexpr (OUT == kFeatBf16) return (unsigned short)(dx_pack16<OUT>(v, 0.f) & 0xFFFFu);
  else return __builtin_bit_cast(unsigned short, (_Float16)v);
}

}  // namespace

// one kernel text under two names: the fp32 kernels of this object, the 16-bit kernels (OUT a template parameter) of units_dx_f16.o
#ifndef OFFK_UNITS_DX_F16
template <bool NCHW>
__global__ __launch_bounds__(DX_THREADS, 1) void units_dx_kernel(DxParams p) {
  constexpr int OUT = kFeatF32;
#else
template <bool NCHW, int OUT>
__global__ __launch_bounds__(DX_THREADS, 1) void units_dx16_kernel(DxParams p) {
#endif
  extern __shared__ __attribute__((aligned(16))) float dx_lds[];
  float* As = dx_lds;                            // [128][DX_AS]
  float* Bs = dx_lds + DX_BM * DX_AS;            // [160][64]
  float* Ts = Bs + kUnitCh * DX_BN;              // [4 waves][32][DX_TS]

  const int bid = (int)blockIdx.x;
  OFFK_PICK_SITE(S, p, bid >= p.s[i].blk_begin)
  const int C = S.C, HW = S.HW, M = S.M;
  const int row0 = (bid - S.blk_begin) * DX_BM;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1;       // the wave's 64 rows x 32 channels of the 128 x 64 tile
  const int nct = (C + DX_BN - 1) / DX_BN;

  // ---- weight tile: rows k of [Wg (128) ; Wd (32)], channels ct * 64 .. + 63, a plain copy (branch-free: the zero page past C) ----
  constexpr int WR = kUnitCh * DX_BN / 4 / DX_THREADS;   // 10 float4 per thread
  dxf4 wreg[WR];
  const int wk = tid >> 4, wc4 = 4 * (tid & 15);         // piece i: row wk + 16 i, channels wc4 .. + 3 of the tile
#define OFFK_DX_LOAD_W(ct)                                                                                   \
  _Pragma("unroll") for (int i = 0; i < WR; ++i) {                                                           \
    const int k = wk + 16 * i, c = (ct) * DX_BN + wc4;                                                       \
    const float* base = k < kGenCh ? S.wg : S.wd;                                                            \
    const size_t off = (size_t)(k < kGenCh ? k : k - kGenCh) * C + c;                                        \
    wreg[i] = *reinterpret_cast<const dxf4*>(c < C ? base + off : p.zeros);                                  \
  }
  OFFK_DX_LOAD_W(0)

  // ---- A = [dGpre | dD] of the block's rows, once (branch-free: what is masked out reads the zero page) ----
  constexpr int AR = DX_BM * DX_A4 / DX_THREADS;         // 20 float4 per thread, in two halves
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    float4 areg[AR / 2];
#pragma unroll
    for (int i = 0; i < AR / 2; ++i) {
      const int idx = tid + DX_THREADS * (half * (AR / 2) + i), r = idx / DX_A4, c4 = idx - r * DX_A4;
      const int row = row0 + r;
      const int f = row / HW, px = row - f * HW;
      const int dr = down_row(f, p.L, p.P, p.slice_mode);
      const bool gen = c4 < kGenCh / 4;
      const float* base = gen ? S.dG : S.dD;
      const size_t off = gen ? (size_t)row * kGenCh + 4 * c4 : ((size_t)(dr < 0 ? 0 : dr) * HW + px) * kDownCh + 4 * (c4 - kGenCh / 4);
      areg[i] = *reinterpret_cast<const float4*>((row < M && (gen || dr >= 0)) ? base + off : p.zeros);
    }
#pragma unroll
    for (int i = 0; i < AR / 2; ++i) {
      const int idx = tid + DX_THREADS * (half * (AR / 2) + i), r = idx / DX_A4, c4 = idx - r * DX_A4;
      *reinterpret_cast<float4*>(As + r * DX_AS + 4 * c4) = areg[i];
    }
  }

  const int r32 = lane & 31, h = lane >> 5;
  const float* asrc = As + (wr * 64 + r32) * DX_AS + 4 * h;
  const float* bsrc = Bs + 4 * h * DX_BN + wc * 32 + r32;
  float* T = Ts + wave * 32 * DX_TS;
  // NCHW epilogue: the lane's row of the wave tile and where its pixel lies
  const int erow = row0 + wr * 64 + lane;
  const int ef = erow / HW, epx = erow - ef * HW;

  for (int ct = 0; ct < nct; ++ct) {
    __syncthreads();                 // the tile before is read (first round: nothing to wait for)
#pragma unroll
    for (int i = 0; i < WR; ++i) *reinterpret_cast<dxf4*>(Bs + (wk + 16 * i) * DX_BN + wc4) = wreg[i];
    __syncthreads();                 // As (first round) and Bs are in place
    if (ct + 1 < nct) { OFFK_DX_LOAD_W(ct + 1) }
    const int cbase = ct * DX_BN + wc * 32;
    if (cbase >= C) continue;        // wave-uniform: the half tile past C (C % 64 == 32)

    f32x16 acc[2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
#pragma unroll 4
    for (int g = 0; g < kUnitCh / 8; ++g) {
      const float4 a0 = *reinterpret_cast<const float4*>(asrc + 8 * g);
      const float4 a1 = *reinterpret_cast<const float4*>(asrc + 32 * DX_AS + 8 * g);
      const float b0 = bsrc[(8 * g + 0) * DX_BN], b1 = bsrc[(8 * g + 1) * DX_BN];
      const float b2 = bsrc[(8 * g + 2) * DX_BN], b3 = bsrc[(8 * g + 3) * DX_BN];
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, b0, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, b0, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, b1, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, b1, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, b2, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, b2, acc[1], 0, 0, 0);
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, b3, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, b3, acc[1], 0, 0, 0);
    }

    // ---- epilogue: acc[t][reg] = row wr * 64 + t * 32 + acc_row(reg, h), channel cbase + r32 ----
    if constexpr (!NCHW && OUT == kFeatF32) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = row0 + wr * 64 + t * 32 + acc_row(reg, h);
          if (row < M) {
            float* o = static_cast<float*>(S.out) + (size_t)row * C + cbase + r32;
            *o = p.accumulate ? *o + acc[t][reg] : acc[t][reg];
          }
        }
    } else if constexpr (!NCHW) {
      // registers (2 i, 2 i + 1) are two adjacent rows: the even lane keeps the first and takes its neighbour's first (channel + 1),
      // the odd lane keeps the second and takes its neighbour's second (channel - 1).  The exchange runs in every lane (a DPP read
      // of a lane that sat out a branch is undefined); only the store is masked by the row.
      const bool odd = lane & 1;
      unsigned short* const o16 = static_cast<unsigned short*>(S.out);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float a = acc[t][2 * i], b = acc[t][2 * i + 1];
          const float got = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, odd ? a : b), 0xB1, 0xF, 0xF, false));
          float lo = odd ? got : a, hi = odd ? b : got;
          const int row = row0 + wr * 64 + t * 32 + acc_row(2 * i, h) + (odd ? 1 : 0);
          if (row < M) {       // channels cbase + (r32 & ~1), + 1: both below C (C and cbase are even), 4-byte aligned (row * C is even)
            unsigned* o = reinterpret_cast<unsigned*>(o16 + (size_t)row * C + cbase + (r32 & ~1));
            if (p.accumulate) {
              const unsigned old = *o;
              lo += widen16<OUT>((unsigned short)(old & 0xFFFFu));
              hi += widen16<OUT>((unsigned short)(old >> 16));
            }
            *o = dx_pack16<OUT>(lo, hi);
          }
        }
    } else {
      // wave-private turn: [channel][row] image, then lanes along the rows.  One wave's LDS operations complete in order; the
      // fences keep the compiler from moving the reads over the writes (and the next tile's writes over these reads)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) T[r32 * DX_TS + t * 32 + acc_row(reg, h)] = acc[t][reg];
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      if constexpr (OUT == kFeatF32) {
        if (erow < M) {
          float* o = static_cast<float*>(S.out) + ((size_t)ef * C + cbase) * HW + epx;
#pragma unroll 8
          for (int ch = 0; ch < 32; ++ch) {
            const float v = T[ch * DX_TS + lane];
            float* oc = o + (size_t)ch * HW;
            *oc = p.accumulate ? *oc + v : v;
          }
        }
      } else {
        if (erow < M) {
          unsigned short* o = static_cast<unsigned short*>(S.out) + ((size_t)ef * C + cbase) * HW + epx;
#pragma unroll 8
          for (int ch = 0; ch < 32; ++ch) {
            const float v = T[ch * DX_TS + lane];
            unsigned short* oc = o + (size_t)ch * HW;
            *oc = dx_round16<OUT>(p.accumulate ? widen16<OUT>(*oc) + v : v);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

#undef OFFK_DX_LOAD_W

#ifndef OFFK_UNITS_DX_F16
hipError_t units_dx_launch(const DxParams& p, hipStream_t st) {
  if (p.total_blocks <= 0) return hipSuccess;
  constexpr int lds = DX_LDS_FLOATS * (int)sizeof(float);
  const void* k = p.nchw ? reinterpret_cast<const void*>(units_dx_kernel<true>) : reinterpret_cast<const void*>(units_dx_kernel<false>);
  hipError_t e = lds_attr_once(k, lds);
  if (e != hipSuccess) return e;
  if (p.nchw) hipLaunchKernelGGL(units_dx_kernel<true>, dim3(p.total_blocks), dim3(DX_THREADS), lds, st, p);
  else hipLaunchKernelGGL(units_dx_kernel<false>, dim3(p.total_blocks), dim3(DX_THREADS), lds, st, p);
  return hipGetLastError();
}

int units_dx_rows_per_block() { return DX_BM; }

#else   // OFFK_UNITS_DX_F16
template <bool NCHW, int OUT>
static hipError_t dx16_launch(const DxParams& p, hipStream_t st) {
  constexpr int lds = DX_LDS_FLOATS * (int)sizeof(float);
  hipError_t e = lds_attr_once(reinterpret_cast<const void*>(units_dx16_kernel<NCHW, OUT>), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((units_dx16_kernel<NCHW, OUT>), dim3(p.total_blocks), dim3(DX_THREADS), lds, st, p);
  return hipGetLastError();
}

hipError_t units_dx16_launch(const DxParams& p, hipStream_t st) {
  if (p.total_blocks <= 0) return hipSuccess;
  if (p.out_dtype == kFeatBf16) return p.nchw ? dx16_launch<true, kFeatBf16>(p, st) : dx16_launch<false, kFeatBf16>(p, st);
  if (p.out_dtype == kFeatF16) return p.nchw ? dx16_launch<true, kFeatF16>(p, st) : dx16_launch<false, kFeatF16>(p, st);
  return hipErrorInvalidValue;
}
#endif  // OFFK_UNITS_DX_F16

}  // namespace offk
