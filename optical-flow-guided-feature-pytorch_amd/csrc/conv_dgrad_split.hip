// K4b, stride 1: the data gradient of the 22 stride-1 fusion convs (1x1 and 3x3 / 1 / (k - 1) / 2) in split-fp32 arithmetic on the bf16
// matrix pipe (offk_conv2d_backward_data_split).  conv_dgrad_s2_split.hip's GEMM with ONE phase:
//     dx[n, h, w, ci] = sum_{kh, kw, co} g[n, h + pad - kh, w + pad - kw, co] * w[co, ci, kh, kw]
// with K = (tap = kh * k + kw, co) in steps of 32 co (Co % 64 == 0: a step never straddles a tap); a tap whose g pixel leaves the map --
// its ROW or its IMAGE -- contributes zeros.  The weight takes the role of `w` and g the role of `x` of
// synth.emulate_split_dot(form="units"): both are cut by truncation into three bf16 planes (synth.cut3) and per step the six products
// w_l g_h, w_h g_l, w_m g_m, w_m g_h, w_h g_m (into accumulator A2) and w_h g_h (into A1) are issued on v_mfma_f32_16x16x32_bf16 in this
// order, steps in increasing order; dx = A1 + A2, added once, and `accumulate` adds that once-rounded value to dx.  K is not split, no
// atomics, every dx element is written by exactly one thread.  k = 1 is the one-tap case of the same kernel.
//
// Two pre-pass launches per call cut BOTH operands into `scratch`, so the GEMM's step loop holds no cut, no v_perm and no fp32 operand:
//   conv_wpack_split_kernel: w_oihw (read in place, NOT rotated: the sum above reads w[co, ci, kh, kw] as it stands) ->
//       [tap][32-co step][16-ci tile][plane][lane] x 16 B, the MFMA's A-operand order: lane (lq = lane / 16, lr = lane % 16) holds co
//       8 lq .. 8 lq + 7 of the step for ci = 16 tile + lr.  (Ci % 64 == 0: there is no partial 16-row tile.)
//   conv_s2_gcut_split_kernel (conv_dgrad_split_common.h, the stride-2 entry's): g -> [plane][n H W][Co] channels-last bf16 plane images.
// The GEMM is conv_s2_dgrad_split_kernel's: eight waves, operands global -> registers -> LDS in operand order through two LDS buffers, the
// next step loaded before the current step's MFMAs and written behind them, one barrier per step; border taps and the M tail by an
// unconditional load at a clamped index and a select to zero.  Three block forms (ci x pixels), chosen by conv_dgrad_split_form from the
// seven integers alone:
//   128 x 256 (2 x 4 waves of 64 x 64)   the stride-2 entry's block: the least staging per MFMA
//   128 x 128 (2 x 4 waves of 64 x 32)   where the 128 x 256 grid would leave more than half of 256 CUs without a block
//    64 x 256 (1 x 8 waves of 64 x 32)   Ci = 64: the upper half of a 128-row block would idle
#include "conv_dgrad_split_common.h"
#include "offk_internal.h"

namespace offk {
namespace {

constexpr int kDgThreads = 512;                // eight waves
constexpr int kDgCus = 256;                    // the grid the form rule is sized for (a constant of the plan, not a device query)

struct DgArgs {
  const spu4* wp;                  // packed weight planes
  const spu4* gp;                  // g planes [plane][M][Co / 8] pieces
  float* dx; int dx_cs, dx_coff;
  int n_img, H, W, Ci, Co, KS, pad, accumulate;
};

// one thread = one lane's piece of one (tap, co step, ci tile), all three planes
__global__ __launch_bounds__(256) void conv_wpack_split_kernel(const float* __restrict__ src, spu4* __restrict__ dst, int Co, int Ci, int KS) {
  const int nct = Ci >> 4, ncs = Co >> 5;
  const int total = KS * KS * ncs * nct * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int lane = i & 63;
    int rest = i >> 6;
    const int tile = rest % nct;
    rest /= nct;
    const int cs = rest % ncs;
    const int tap = rest / ncs;
    const int kh = tap / KS, kw = tap - kh * KS;
    const int ci = tile * 16 + (lane & 15), co = cs * 32 + (lane >> 4) * 8;
    const float* s = src + (((size_t)co * Ci + ci) * KS + kh) * KS + kw;
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = s[(size_t)e * Ci * KS * KS];
    spu4 a, b, c;
    sp_cut8(v, a, b, c);
    spu4* d = dst + (size_t)(i >> 6) * 192 + lane;
    d[0] = a; d[64] = b; d[128] = c;
  }
}

// WM x WN waves of CT (16-ci tiles) x PT (16-pixel tiles) each; WM * WN = 8
template <int WM, int WN, int CT, int PT>
__global__ __launch_bounds__(kDgThreads, 2) void conv_dgrad_split_kernel(DgArgs p) {
  constexpr int CiTiles = WM * CT, PxTiles = WN * PT, Px = PxTiles * 16;
  constexpr int APieces = CiTiles * 192, BPieces = PxTiles * 192, Buf = APieces + BPieces;
  constexpr int AJ = (APieces + kDgThreads - 1) / kDgThreads, PJ = Px * 4 / kDgThreads;       // A pieces and pixels of a thread per step
  constexpr bool AWhole = APieces % kDgThreads == 0;                                        // else the last A piece only for tid < the rest
  static_assert(WM * WN * 64 == kDgThreads && (Px * 4) % kDgThreads == 0 && PJ >= 1, "geometry");
  // two buffers of: A pieces [ci tile][plane][lane], then B pieces [pixel tile][plane][lane]
  extern __shared__ __attribute__((aligned(16))) spu4 lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int lq = lane >> 4, lr = lane & 15;
  const int H = p.H, W = p.W, KS = p.KS, pad = p.pad;
  const int M = p.n_img * H * W;
  const int m0 = blockIdx.x * Px, ct0 = blockIdx.y * CiTiles;
  const int nct = p.Ci >> 4, ncs = p.Co >> 5, c8 = p.Co >> 3;
  const int nsteps = KS * KS * ncs;
  const int step_pieces = nct * 192;

  // this thread's A pieces of a step (a block's ci tiles behind Ci: the last real piece) and its pixels of the B operand, decoded once
  const int abase = ct0 * 192 + tid, alast = step_pieces - 1;
  const int kg = tid & 3, px0 = tid >> 2;
  int gimg[PJ], ga[PJ], gb[PJ];
#pragma unroll
  for (int j = 0; j < PJ; ++j) {
    const int m = m0 + px0 + 128 * j;
    const int mc = min(m, M - 1);
    const int img = mc / (H * W), rem = mc - img * (H * W);
    ga[j] = rem / W;
    gb[j] = rem - ga[j] * W;
    gimg[j] = m < M ? img : -1;
  }
  const int bdst = APieces + (px0 >> 4) * 192 + kg * 16 + (px0 & 15);      // pixel px0 + 128 j: eight pixel tiles further

  spu4 ar[AJ], br[PJ][3];
  int kh = 0, kw = 0, cs = 0, t_next = 0;                              // the step load_step loads next
  auto load_step = [&]() {
    const spu4* wstep = p.wp + (size_t)t_next * step_pieces;
#pragma unroll
    for (int j = 0; j < AJ; ++j) ar[j] = wstep[min(abase + kDgThreads * j, alast)];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      // the pixel shifted by (pad - kh, pad - kw): one that leaves its row or its image is a zero, not the neighbour's pixel
      const int a = ga[j] + pad - kh, b = gb[j] + pad - kw;
      const bool ok = gimg[j] >= 0 && a >= 0 && a < H && b >= 0 && b < W;
      const size_t pix = ok ? (size_t)((gimg[j] * H + a) * W + b) : 0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        spu4 v = p.gp[((size_t)q * M + pix) * c8 + cs * 4 + kg];
        if (!ok) v = spu4{0u, 0u, 0u, 0u};
        br[j][q] = v;
      }
    }
    ++t_next;
    if (++cs == ncs) {
      cs = 0;
      if (++kw == KS) { kw = 0; ++kh; }
    }
  };
  auto store_step = [&](int buf) {
    spu4* const d = lds + buf * Buf;
#pragma unroll
    for (int j = 0; j < AJ; ++j)
      if (AWhole || j + 1 < AJ || tid + kDgThreads * j < APieces) d[tid + kDgThreads * j] = ar[j];
#pragma unroll
    for (int j = 0; j < PJ; ++j)
#pragma unroll
      for (int q = 0; q < 3; ++q) d[bdst + j * (8 * 192) + q * 64] = br[j][q];
  };

  spf4 a1[CT][PT], a2[CT][PT];
#pragma unroll
  for (int mt = 0; mt < CT; ++mt)
#pragma unroll
    for (int nt = 0; nt < PT; ++nt) { a1[mt][nt] = spf4{0.f, 0.f, 0.f, 0.f}; a2[mt][nt] = spf4{0.f, 0.f, 0.f, 0.f}; }
  const bool busy = ct0 + wm * CT < nct;             // a wave whose ci tiles lie behind Ci stages, waits at the barriers and computes nothing

  auto mma_step = [&](int buf) {
    const spu4* const la = lds + buf * Buf + wm * CT * 192 + lane;
    const spu4* const lb = lds + buf * Buf + APieces + wn * PT * 192 + lane;
    spu4 wa[CT][3];
#pragma unroll
    for (int mt = 0; mt < CT; ++mt)
#pragma unroll
      for (int q = 0; q < 3; ++q) wa[mt][q] = la[(mt * 3 + q) * 64];
#pragma unroll
    for (int nt = 0; nt < PT; ++nt) {
      spu4 gx[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) gx[q] = lb[(nt * 3 + q) * 64];
      // synth.SPLIT_PRODUCTS order (w plane, g plane): (2, 0), (0, 2), (1, 1), (1, 0), (0, 1) -> A2; (0, 0) -> A1
#pragma unroll
      for (int mt = 0; mt < CT; ++mt) sp_mfma(a2[mt][nt], wa[mt][2], gx[0]);
#pragma unroll
      for (int mt = 0; mt < CT; ++mt) sp_mfma(a2[mt][nt], wa[mt][0], gx[2]);
#pragma unroll
      for (int mt = 0; mt < CT; ++mt) sp_mfma(a2[mt][nt], wa[mt][1], gx[1]);
#pragma unroll
      for (int mt = 0; mt < CT; ++mt) sp_mfma(a2[mt][nt], wa[mt][1], gx[0]);
#pragma unroll
      for (int mt = 0; mt < CT; ++mt) sp_mfma(a2[mt][nt], wa[mt][0], gx[1]);
#pragma unroll
      for (int mt = 0; mt < CT; ++mt) sp_mfma(a1[mt][nt], wa[mt][0], gx[0]);
    }
  };

  // step t's operands are in buffer t & 1; step t + 1's are loaded into registers before the MFMAs of step t and written to the other
  // buffer behind them (every wave has left that buffer: it was read in step t - 1, before the last barrier): one barrier per step
  load_step();
  store_step(0);
  __syncthreads();
  for (int t = 0; t < nsteps; ++t) {
    const bool more = t + 1 < nsteps;
    if (more) load_step();
    if (busy) mma_step(t & 1);
    if (more) store_step((t + 1) & 1);
    __syncthreads();
  }

  // D of the 16x16x32 form: row (ci) = 4 * (lane / 16) + reg, column (pixel) = lane % 16: four consecutive ci of one pixel per lane
  if (!busy) return;
#pragma unroll
  for (int nt = 0; nt < PT; ++nt) {
    const int m = m0 + (wn * PT + nt) * 16 + lr;
    if (m >= M) continue;
    float* row = p.dx + (size_t)m * p.dx_cs + p.dx_coff;
#pragma unroll
    for (int mt = 0; mt < CT; ++mt) {
      const int ci = (ct0 + wm * CT + mt) * 16 + lq * 4;
      if (ci >= p.Ci) continue;
      spf4 v = a1[mt][nt] + a2[mt][nt];
      spf4* dst = reinterpret_cast<spf4*>(row + ci);
      if (p.accumulate) v += *dst;
      *dst = v;
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_nop 1");
      __builtin_amdgcn_sched_barrier(0);
    }
  }
}

template <int WM, int WN, int CT, int PT>
hipError_t dg_launch(const DgArgs& a, int M, hipStream_t st) {
  constexpr int CiTiles = WM * CT, Px = WN * PT * 16;
  constexpr int lds = 2 * (CiTiles + WN * PT) * 192 * 16;
  hipError_t e = lds_attr_once(reinterpret_cast<const void*>(conv_dgrad_split_kernel<WM, WN, CT, PT>), lds);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((M + Px - 1) / Px), (unsigned)((a.Ci / 16 + CiTiles - 1) / CiTiles), 1);
  hipLaunchKernelGGL((conv_dgrad_split_kernel<WM, WN, CT, PT>), grid, dim3(kDgThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace

// the block of the GEMM: 64 ci wide where Ci is 64; else 128 ci x 256 pixels unless that grid leaves more than half of kDgCus idle
void conv_dgrad_split_form(int n_img, int H, int W, int Ci, int* ci_per_block, int* pixels_per_block) {
  const long long M = (long long)n_img * H * W;
  int cb = 128, pb = 256;
  if (Ci == 64) {
    cb = 64;
  } else if (((M + 255) / 256) * ((Ci + 127) / 128) * 2 <= kDgCus) {
    pb = 128;
  }
  *ci_per_block = cb;
  *pixels_per_block = pb;
}

// scratch of the split data gradient: the three planes of the packed weight (Co Ci k k x 6 bytes), then the three planes of g
// (n H W Co x 6 bytes), each region rounded up to 256 bytes; a function of these seven integers only
bool conv_dgrad_split_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_bytes, size_t* g_bytes) {
  if (!conv_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return false;
  const size_t M = (size_t)n_img * H * W;
  if (M + 256 > 0x7fffffffULL || (size_t)Co * Ci * KH * KW * 4 > 0x7fffffffULL) return false;
  if (weight_bytes) *weight_bytes = ds_round256((size_t)Co * Ci * KH * KW * 6);
  if (g_bytes) *g_bytes = ds_round256(M * Co * 6);
  return true;
}

hipError_t conv_dgrad_split_launch(const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw, int Ci, int KS,
                                   int pad, float* dx, int dx_cs, int dx_coff, int accumulate, void* scratch, hipStream_t st) {
  size_t wbytes = 0;
  if (!conv_dgrad_split_plan(n_img, H, W, Ci, Co, KS, KS, &wbytes, nullptr)) return hipErrorInvalidValue;
  const int M = n_img * H * W;
  spu4* wp = static_cast<spu4*>(scratch);
  spu4* gp = reinterpret_cast<spu4*>(static_cast<char*>(scratch) + wbytes);
  const long long wthreads = (long long)KS * KS * (Co / 32) * (Ci / 16) * 64;
  hipLaunchKernelGGL(conv_wpack_split_kernel, dim3((unsigned)((wthreads + 255) / 256)), dim3(256), 0, st, w_oihw, wp, Co, Ci, KS);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long gthreads = (long long)M * (Co / 8);
  const long long gblocks = (gthreads + 255) / 256;
  hipLaunchKernelGGL(conv_s2_gcut_split_kernel, dim3((unsigned)(gblocks < 65536 ? gblocks : 65536)), dim3(256), 0, st, g, g_cs, g_coff, gp, M, Co);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  DgArgs a;
  a.wp = wp; a.gp = gp; a.dx = dx; a.dx_cs = dx_cs; a.dx_coff = dx_coff;
  a.n_img = n_img; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.KS = KS; a.pad = pad; a.accumulate = accumulate;
  int cb = 0, pb = 0;
  conv_dgrad_split_form(n_img, H, W, Ci, &cb, &pb);
  if (cb == 64) return dg_launch<1, 8, 4, 2>(a, M, st);
  if (pb == 128) return dg_launch<2, 4, 4, 2>(a, M, st);
  return dg_launch<2, 4, 4, 4>(a, M, st);
}

}  // namespace offk
