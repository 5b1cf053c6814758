// K4b, stride 2: the data gradient of the two stage-opening fusion convs (7x7 / 2 / 3 and 5x5 / 2 / 2) in split-fp32 arithmetic on the bf16
// matrix pipe (offk_conv2d_s2_backward_data_split).  The sums are conv_s2_dgrad_kernel's (conv_bwd_s2.hip), phase by
// phase: an input pixel is (2a + r, 2b + s) and
//     dx[n, 2a + r, 2b + s, ci] = sum_{th, tw, co} g[n, a + dh0(r) - th, b + dw0(s) - tw, co] * w[co, ci, kh0(r) + 2 th, kw0(s) + 2 tw]
// with K = (tap = th * nw + tw, co) in steps of 32 co (Co % 64 == 0: a step never straddles a tap); a tap that leaves the map at a pixel
// contributes zeros.  The weight takes the role of `w` and g the role of `x` of synth.emulate_split_dot(form="units"): both are cut by
// truncation into three bf16 planes (synth.cut3) and per step the six products w_l g_h, w_h g_l, w_m g_m, w_m g_h, w_h g_m (into accumulator
// A2) and w_h g_h (into A1) are issued on v_mfma_f32_16x16x32_bf16 in this order, steps in increasing order; dx = A1 + A2, added once, and
// `accumulate` adds that once-rounded value to dx.  K is not split, no atomics, every dx element is written by exactly one thread.
//
// Two pre-pass launches per call cut BOTH operands into `scratch`, so the GEMM's step loop holds no cut, no v_perm and no fp32 operand:
//   conv_s2_wpack_split_kernel: w_oihw (read in place) -> [phase][tap][32-co step][16-ci tile][plane][lane] x 16 B, the MFMA's A-operand
//       order: lane (lq = lane / 16, lr = lane % 16) holds co 8 lq .. 8 lq + 7 of the step for ci = 16 tile + lr.  A block's eight ci tiles of
//       one step are 24 KB in one piece, and consecutive steps of a phase follow each other: the staging copy is linear.  Phases and taps
//       in conv_s2_pack_kernel's order.  (Ci % 32 == 0: there is no partial 16-row tile, nothing to zero-fill.)
//   conv_s2_gcut_split_kernel (conv_dgrad_split_common.h, shared with the stride-1 entry): g (the caller's channel-sliced view) -> three channels-last bf16 plane images [plane][n OH OW][Co]: the B
//       operand of (pixel, 8 co) is one aligned 16-byte read.
// The GEMM: one block = 128 ci x 256 pixels of one phase, eight waves (2 along ci x 4 along the pixels) of 64 x 64 each: 16 tiles of 16 x 16 in
// A1 and A2, 128 accumulator registers; one block per CU (two waves per SIMD, at most 256 registers: build.py's register guard).  Per step
// a thread copies three 16-byte pieces of A and six of B global -> registers -> LDS (72 KB per step, both already in operand order:
// [16-row tile][plane][lane], so every ds_read_b128 / ds_write_b128 of a wave covers 1 KB without a bank conflict); two LDS buffers
// (144 KB), the next step's pieces are loaded before the current step's MFMAs and written to the other buffer behind them: one barrier
// per step.  Boundary taps and the M tail use unconditional loads with a clamped index and a select to zero; ci tiles behind Ci read the
// last real piece (clamped) and are neither computed (whole waves) nor stored.  blockIdx.z walks the phases longest first (16 / 12 / 12 /
// 9 taps for the 7x7).  The same kernel with a 128 x 128 block (eight waves of 32 x 64) took 1.25 / 1.01 ms where this one takes 1.03 /
// 0.83 ms: per MFMA it stages and reads a third more.
#include "conv_dgrad_split_common.h"
#include "offk_internal.h"

namespace offk {
namespace {

constexpr int kDsThreads = 512;                // eight waves
constexpr int kDsWM = 2, kDsWN = 4, kDsCT = 4, kDsPT = 4;      // 2 x 4 waves of 4 (16-ci tiles) x 4 (16-pixel tiles): a block is 128 ci x 256 pixels
#ifndef DS_WAVES_PER_EU
#define DS_WAVES_PER_EU 2                       // one block per CU
#endif

struct DsArgs {
  const spu4* wp;                  // packed weight planes
  const spu4* gp;                  // g planes [plane][M][Co / 8] pieces
  float* dx; int dx_cs, dx_coff;
  int n_img, H, W, Ci, Co, KS, pad, accumulate;
  int order[4];                    // phase of blockIdx.z: longest first
};

// taps of phase bit r along one axis, first kernel index, and the g offset of tap 0 (tap t reads g at a + d0 - t): conv_bwd_s2.hip's s2_axis
__host__ __device__ __forceinline__ void ds_axis(int KS, int pad, int r, int* ntap, int* k0, int* d0) {
  *k0 = (r + pad) & 1;
  *ntap = (KS - *k0 + 1) / 2;
  *d0 = (r + pad - *k0) / 2;
}
__host__ __device__ __forceinline__ int ds_phase_taps(int KS, int pad, int ph) {
  int nh, nw, k0, d0;
  ds_axis(KS, pad, ph >> 1, &nh, &k0, &d0);
  ds_axis(KS, pad, ph & 1, &nw, &k0, &d0);
  return nh * nw;
}

// one thread = one lane's piece of one (phase, tap, co step, ci tile), all three planes
__global__ __launch_bounds__(256) void conv_s2_wpack_split_kernel(const float* __restrict__ src, spu4* __restrict__ dst, int Co, int Ci, int KS,
                                                                  int pad) {
  const int nct = Ci >> 4, ncs = Co >> 5;
  const int total = KS * KS * ncs * nct * 64;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int lane = i & 63;
    int rest = i >> 6;
    const int tile = rest % nct;
    rest /= nct;
    const int cs = rest % ncs;
    int tap = rest / ncs;
    int ph = 0;
    for (; ph < 3; ++ph) {
      const int t = ds_phase_taps(KS, pad, ph);
      if (tap < t) break;
      tap -= t;
    }
    int nh, nw, kh0, kw0, d0;
    ds_axis(KS, pad, ph >> 1, &nh, &kh0, &d0);
    ds_axis(KS, pad, ph & 1, &nw, &kw0, &d0);
    const int th = tap / nw, tw = tap - th * nw;
    const int ci = tile * 16 + (lane & 15), co = cs * 32 + (lane >> 4) * 8;
    const float* s = src + (((size_t)co * Ci + ci) * KS + (kh0 + 2 * th)) * KS + (kw0 + 2 * tw);
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
__global__ __launch_bounds__(kDsThreads, DS_WAVES_PER_EU) void conv_s2_dgrad_split_kernel(DsArgs p) {
  constexpr int CiTiles = WM * CT, PxTiles = WN * PT, Px = PxTiles * 16;
  constexpr int APieces = CiTiles * 192, BPieces = PxTiles * 192, Buf = APieces + BPieces;
  constexpr int AJ = APieces / kDsThreads, PJ = Px * 4 / kDsThreads;       // A pieces and pixels of a thread per step
  static_assert(WM * WN * 64 == kDsThreads && APieces % kDsThreads == 0 && (Px * 4) % kDsThreads == 0, "geometry");
  // two buffers of: A pieces [ci tile][plane][lane], then B pieces [pixel tile][plane][lane]
  extern __shared__ __attribute__((aligned(16))) spu4 lds[];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int lq = lane >> 4, lr = lane & 15;
  const int ph = p.order[blockIdx.z], r = ph >> 1, s = ph & 1;
  const int OH = p.H >> 1, OW = p.W >> 1;
  const int M = p.n_img * OH * OW;
  const int m0 = blockIdx.x * Px, ct0 = blockIdx.y * CiTiles;
  const int nct = p.Ci >> 4, ncs = p.Co >> 5, c8 = p.Co >> 3;

  int nh, nw, k0, dh0, dw0;
  ds_axis(p.KS, p.pad, r, &nh, &k0, &dh0);
  ds_axis(p.KS, p.pad, s, &nw, &k0, &dw0);
  int tapbase = 0;
  for (int q = 0; q < ph; ++q) tapbase += ds_phase_taps(p.KS, p.pad, q);
  const int nsteps = nh * nw * ncs;
  const int step_pieces = nct * 192;
  const spu4* wsrc = p.wp + (size_t)tapbase * ncs * step_pieces;

  // this thread's A pieces of a step (a block's ci tiles behind Ci: the last real piece) and its pixels of the B operand
  const int abase = ct0 * 192 + tid, alast = step_pieces - 1;
  const int kg = tid & 3, px0 = tid >> 2;
  int gimg[PJ], ga[PJ], gb[PJ];
#pragma unroll
  for (int j = 0; j < PJ; ++j) {
    const int m = m0 + px0 + 128 * j;
    const int mc = min(m, M - 1);
    const int img = mc / (OH * OW), rem = mc - img * (OH * OW);
    ga[j] = rem / OW;
    gb[j] = rem - ga[j] * OW;
    gimg[j] = m < M ? img : -1;
  }
  const int bdst = APieces + (px0 >> 4) * 192 + kg * 16 + (px0 & 15);      // pixel px0 + 128 j: eight pixel tiles further

  spu4 ar[AJ], br[PJ][3];
  int th = 0, tw = 0, cs = 0, t_next = 0;                              // the step load_step loads next
  auto load_step = [&]() {
    const spu4* wstep = wsrc + (size_t)t_next * step_pieces;
#pragma unroll
    for (int j = 0; j < AJ; ++j) ar[j] = wstep[min(abase + kDsThreads * j, alast)];
#pragma unroll
    for (int j = 0; j < PJ; ++j) {
      const int a = ga[j] + dh0 - th, b = gb[j] + dw0 - tw;
      const bool ok = gimg[j] >= 0 && a >= 0 && a < OH && b >= 0 && b < OW;
      const size_t pix = ok ? (size_t)((gimg[j] * OH + a) * OW + b) : 0;
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
      if (++tw == nw) { tw = 0; ++th; }
    }
  };
  auto store_step = [&](int buf) {
    spu4* const d = lds + buf * Buf;
#pragma unroll
    for (int j = 0; j < AJ; ++j) d[tid + kDsThreads * j] = ar[j];
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
    const int img = m / (OH * OW), rem = m - img * (OH * OW);
    const int a = rem / OW, b = rem - a * OW;
    float* row = p.dx + ((size_t)(img * p.H + 2 * a + r) * p.W + 2 * b + s) * p.dx_cs + p.dx_coff;
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
hipError_t ds_launch(const DsArgs& a, int M, hipStream_t st) {
  constexpr int CiTiles = WM * CT, Px = WN * PT * 16;
  constexpr int lds = 2 * (CiTiles + WN * PT) * 192 * 16;
  hipError_t e = lds_attr_once(reinterpret_cast<const void*>(conv_s2_dgrad_split_kernel<WM, WN, CT, PT>), lds);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)((M + Px - 1) / Px), (unsigned)((a.Ci / 16 + CiTiles - 1) / CiTiles), 4);
  hipLaunchKernelGGL((conv_s2_dgrad_split_kernel<WM, WN, CT, PT>), grid, dim3(kDsThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace

// scratch of the split data gradient: the three planes of the packed weight (Co Ci k k x 6 bytes), then the three planes of g
// (n (H / 2)(W / 2) Co x 6 bytes), each region rounded up to 256 bytes; a function of these seven integers only
bool conv_s2_dgrad_split_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_bytes, size_t* g_bytes) {
  if (!conv_s2_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return false;
  const size_t M = (size_t)n_img * (H / 2) * (W / 2);
  if (M + kDsWN * kDsPT * 16 > 0x7fffffffULL) return false;
  if (weight_bytes) *weight_bytes = ds_round256((size_t)Co * Ci * KH * KW * 6);
  if (g_bytes) *g_bytes = ds_round256(M * Co * 6);
  return true;
}

hipError_t conv_s2_dgrad_split_launch(const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw, int Ci, int KS,
                                      int pad, float* dx, int dx_cs, int dx_coff, int accumulate, void* scratch, hipStream_t st) {
  size_t wbytes = 0;
  if (!conv_s2_dgrad_split_plan(n_img, H, W, Ci, Co, KS, KS, &wbytes, nullptr)) return hipErrorInvalidValue;
  const int M = n_img * (H / 2) * (W / 2);
  spu4* wp = static_cast<spu4*>(scratch);
  spu4* gp = reinterpret_cast<spu4*>(static_cast<char*>(scratch) + wbytes);
  const long long wthreads = (long long)KS * KS * (Co / 32) * (Ci / 16) * 64;
  hipLaunchKernelGGL(conv_s2_wpack_split_kernel, dim3((unsigned)((wthreads + 255) / 256)), dim3(256), 0, st, w_oihw, wp, Co, Ci, KS, pad);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long gthreads = (long long)M * (Co / 8);
  const long long gblocks = (gthreads + 255) / 256;
  hipLaunchKernelGGL(conv_s2_gcut_split_kernel, dim3((unsigned)(gblocks < 65536 ? gblocks : 65536)), dim3(256), 0, st, g, g_cs, g_coff, gp, M, Co);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  DsArgs a;
  a.wp = wp; a.gp = gp; a.dx = dx; a.dx_cs = dx_cs; a.dx_coff = dx_coff;
  a.n_img = n_img; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.KS = KS; a.pad = pad; a.accumulate = accumulate;
  // phases by falling tap count (ties in phase order)
  int k = 0;
  for (int taps = KS * KS; taps > 0; --taps)
    for (int ph = 0; ph < 4; ++ph)
      if (ds_phase_taps(KS, pad, ph) == taps) a.order[k++] = ph;
  return ds_launch<kDsWM, kDsWN, kDsCT, kDsPT>(a, M, st);
}

}  // namespace offk
