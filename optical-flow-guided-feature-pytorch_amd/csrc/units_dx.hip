// Training side of the OFF units: the gradient w.r.t. the nine feature maps (offk_off_units_backward_feats).
//   dX[frame n, pixel q, c] = sum_o dGpre[n, q, o] Wg[o, c] + sum_j dD[r(n), q, j] Wd[j, c]
// from what K2b (units_bwd.hip) left in the train workspace -- dG_<site> [N*HW][128], dD_<site> [P*HW][32] -- and the gen / down
// weights as fp32 rows [128][C] / [32][C].  r(n) is the row of frame n in the spatial slice (wg_down_row of K1b: flat slice
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
#include "offk_common.h"
#include "offk_internal.h"

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

__device__ __forceinline__ int dx_down_row(int f, int L, int P, int slice_mode) {   // wg_down_row of units_bwd.hip
  if (slice_mode == 0) return f < P ? f : -1;
  const int b = f / L, t = f - b * L;
  return t < L - 1 ? b * (L - 1) + t : -1;
}

}  // namespace

template <bool NCHW>
__global__ __launch_bounds__(DX_THREADS, 1) void units_dx_kernel(DxParams p) {
  extern __shared__ __attribute__((aligned(16))) float dx_lds[];
  float* As = dx_lds;                            // [128][DX_AS]
  float* Bs = dx_lds + DX_BM * DX_AS;            // [160][64]
  float* Ts = Bs + kUnitCh * DX_BN;              // [4 waves][32][DX_TS]

  const int bid = (int)blockIdx.x;
  DxSite S;
#define OFFK_DX_PICK(i)                                                                                      \
  S.dG = p.s[i].dG; S.dD = p.s[i].dD; S.wg = p.s[i].wg; S.wd = p.s[i].wd; S.out = p.s[i].out; S.C = p.s[i].C; \
  S.HW = p.s[i].HW; S.M = p.s[i].M; S.blk_begin = p.s[i].blk_begin;
  OFFK_DX_PICK(0)
#pragma unroll
  for (int i = 1; i < kNumSites; ++i)
    if (i < p.nsites && bid >= p.s[i].blk_begin) { OFFK_DX_PICK(i) }
#undef OFFK_DX_PICK
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
      const int dr = dx_down_row(f, p.L, p.P, p.slice_mode);
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
    if constexpr (!NCHW) {
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
          const int row = row0 + wr * 64 + t * 32 + acc_row(reg, h);
          if (row < M) {
            float* o = S.out + (size_t)row * C + cbase + r32;
            *o = p.accumulate ? *o + acc[t][reg] : acc[t][reg];
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
      if (erow < M) {
        float* o = S.out + ((size_t)ef * C + cbase) * HW + epx;
#pragma unroll 8
        for (int ch = 0; ch < 32; ++ch) {
          const float v = T[ch * DX_TS + lane];
          float* oc = o + (size_t)ch * HW;
          *oc = p.accumulate ? *oc + v : v;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
}

#undef OFFK_DX_LOAD_W

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

}  // namespace offk
