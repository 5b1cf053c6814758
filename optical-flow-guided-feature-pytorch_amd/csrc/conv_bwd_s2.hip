// K4b, stride 2. Backward of the two stage-opening fusion convolutions (7x7 / 2 / 3 and 5x5 / 2 / 2, H and W even), exact fp32 on
// v_mfma_f32_16x16x4_f32.  An input pixel is (2a + r, 2b + s): the conv reads phase image (r, s) of x at stride 1.
//
// Data gradient, one implicit GEMM per phase, all four in one launch (blockIdx.z = 2 r + s):
//     dx[n, 2a + r, 2b + s, ci] = sum_{th, tw, co} g[n, a + dh(th), b + dw(tw), co] * w[co, ci, kh0(r) + 2 th, kw0(s) + 2 tw]
//   kh0(r) = (r + pad) & 1, dh(th) = (r + pad - kh0) / 2 - th: 3 or 4 taps per axis for the 7x7, 3 or 2 for the 5x5 -- only taps that exist.
//   A block owns 64 (ci) x 64 (pixels of the phase); K = the phase's taps x Co in tiles of one tap x 32 co.  The weight is the MFMA's A
//   operand, so a lane's four results are four consecutive ci of one pixel: one 16-byte store straight to the dx pixel, no staging copy.
//   conv_s2_pack_kernel cuts [phase][tap][Co][Ci] from w_oihw into scratch on every call (exactly Co * Ci * k * k floats).  K is not
//   split: every dx element is one fixed-order chain, rounded once before `accumulate` adds it.
//
// Weight gradient, one block = one 64 (co) x 64 (ci) tile of dw for ONE kernel row kh (7 or 5 taps: 112 or 80 accumulator registers)
// over one chunk of whole images.  With r = (kh - pad) & 1, fh = floor((kh - pad) / 2) (and s, fw for kw)
//     dw[co][ci][kh][kw] = sum_{n, oh, ow} g[n, oh, ow, co] * x[n, 2 (oh + fh) + r, 2 (ow + fw) + s, ci]
//   K runs over the output pixels q = (n, oh, ow) of the chunk, images back to back, NO padding: g is staged as it lies, x as the two
//   column-phase windows X_s[q + j - LO] of the block's input row (zero where the row 2 (oh + fh) + r is outside the map), and the kw taps
//   are row offsets fw + LO into the window of their phase (fw = -2 .. 1 for the 7x7, -1 .. 1 for the 5x5) -- the trick of
//   conv_wgrad_kernel<3> (conv_bwd.hip), same LDS layout.  Without a zero ring, row q + fw of a window is the NEIGHBOURING row's pixel where
//   ow + fw leaves the map; those terms are removed on the g side: the loader leaves every position's ow in LDS and a lane zeroes its g
//   operand for the taps whose fw leaves the map at its position (three compares and six selects per 28 or 20 MFMAs).  A zero ring
//   instead costs 16 / 14 (7x7) or 8 / 7 (5x5) of the MFMAs; measured, profiles/fusion_bwd/README.md.
//   A last ci tile of 32 loads zeros for its upper half and does not store it.
//   Slabs [chunk][Co][Ci * k * k] + [chunk][Co] and the reduce in chunk order are conv_bwd.hip's.
#include "offk_common.h"
#include "offk_internal.h"

namespace offk {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kKT = 32;           // K-tile: positions (weight gradient) or output channels of one tap (data gradient)
constexpr int kLd = 80;           // LDS stride of a [k][64 channels] row: rows k .. k + 3 start 16 banks apart (conv_bwd.hip)
constexpr int kLdG = 36;          // LDS stride of a [pixel][32 co] row of the data gradient: 16-byte aligned rows
constexpr int kS2Slots = 512;     // weight gradient: two blocks of four waves per CU on 256 CUs
constexpr int kS2MinPositions = 256;

// ---------------------------------------------------------------- data gradient ----------------------------------------------------------------
struct S2DgradArgs {
  const float* g; int g_cs, g_coff;
  const float* wp;                 // [phase][tap][Co][Ci]
  float* dx; int dx_cs, dx_coff;
  int n_img, H, W, Ci, Co, KS, pad, accumulate;
};

// taps of phase bit r along one axis, first kernel index, and the g offset of tap 0 (tap t reads g at a + d0 - t)
__host__ __device__ __forceinline__ void s2_axis(int KS, int pad, int r, int* ntap, int* k0, int* d0) {
  *k0 = (r + pad) & 1;
  *ntap = (KS - *k0 + 1) / 2;
  *d0 = (r + pad - *k0) / 2;
}

__host__ __device__ __forceinline__ int s2_phase_taps(int KS, int pad, int ph) {
  int nh, nw, k0, d0;
  s2_axis(KS, pad, ph >> 1, &nh, &k0, &d0);
  s2_axis(KS, pad, ph & 1, &nw, &k0, &d0);
  return nh * nw;
}

// w_oihw [Co][Ci][k][k] -> [phase][tap = th * nw + tw][Co][Ci]
__global__ void conv_s2_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int Co, int Ci, int KS, int pad) {
  const size_t cc = (size_t)Co * Ci, n = cc * KS * KS;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    int tap = (int)(i / cc);
    const size_t rem = i - (size_t)tap * cc;
    const int co = (int)(rem / Ci), ci = (int)(rem - (size_t)co * Ci);
    int ph = 0;
    for (; ph < 3; ++ph) {
      const int t = s2_phase_taps(KS, pad, ph);
      if (tap < t) break;
      tap -= t;
    }
    int nh, nw, kh0, kw0, d0;
    s2_axis(KS, pad, ph >> 1, &nh, &kh0, &d0);
    s2_axis(KS, pad, ph & 1, &nw, &kw0, &d0);
    const int th = tap / nw, tw = tap - th * nw;
    dst[i] = src[(((size_t)co * Ci + ci) * KS + (kh0 + 2 * th)) * KS + (kw0 + 2 * tw)];
  }
}

__global__ __launch_bounds__(256) void conv_s2_dgrad_kernel(S2DgradArgs p) {
  __shared__ __attribute__((aligned(16))) float ws[kKT * kLd];      // [co of the K-tile][ci of the tile]
  __shared__ __attribute__((aligned(16))) float gs[64 * kLdG];      // [pixel of the tile][co of the K-tile]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;           // wave tile: 32 (ci) x 32 (pixels)
  const int lk = lane >> 4, lr = lane & 15;
  const int ph = blockIdx.z, r = ph >> 1, s = ph & 1;
  const int OH = p.H >> 1, OW = p.W >> 1;
  const int M = p.n_img * OH * OW;
  const int m0 = blockIdx.x * 64, ci0 = blockIdx.y * 64;

  int nh, nw, k0, dh0, dw0;
  s2_axis(p.KS, p.pad, r, &nh, &k0, &dh0);
  s2_axis(p.KS, p.pad, s, &nw, &k0, &dw0);
  size_t wbase = 0;
  for (int q = 0; q < ph; ++q) wbase += (size_t)s2_phase_taps(p.KS, p.pad, q) * p.Co * p.Ci;
  const float* wsrc = p.wp + wbase + ci0;
  const float* gsrc = p.g + p.g_coff;
  const int ncc = p.Co / kKT, ntiles = nh * nw * ncc;

  // the two g slots of this thread: pixel row tid / 8 (+ 32), four co at (tid % 8) * 4; the two w slots: co row tid / 16 (+ 16), four ci
  const int gc4 = (tid & 7) * 4, wc4 = (tid & 15) * 4;
  int gimg[2], ga[2], gb[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int m = m0 + (tid >> 3) + j * 32;
    if (m < M) {
      gimg[j] = m / (OH * OW);
      const int rem = m - gimg[j] * (OH * OW);
      ga[j] = rem / OW;
      gb[j] = rem - ga[j] * OW;
    } else {
      gimg[j] = -1; ga[j] = 0; gb[j] = 0;
    }
  }
  const bool w_in = ci0 + wc4 < p.Ci;

  float4 gr[2], wr[2];
  auto load_tile = [&](int t) {
    const int tap = t / ncc, c0 = (t - tap * ncc) * kKT;
    const int th = tap / nw, tw = tap - th * nw;
    const int dh = dh0 - th, dw = dw0 - tw;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      const int a = ga[j] + dh, b = gb[j] + dw;
      if (gimg[j] >= 0 && a >= 0 && a < OH && b >= 0 && b < OW)
        v = *reinterpret_cast<const float4*>(gsrc + ((size_t)(gimg[j] * OH + a) * OW + b) * p.g_cs + c0 + gc4);
      gr[j] = v;
      float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
      if (w_in) u = *reinterpret_cast<const float4*>(wsrc + ((size_t)tap * p.Co + c0 + (tid >> 4) + j * 16) * p.Ci + wc4);
      wr[j] = u;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      *reinterpret_cast<float4*>(gs + ((tid >> 3) + j * 32) * kLdG + gc4) = gr[j];
      *reinterpret_cast<float4*>(ws + ((tid >> 4) + j * 16) * kLd + wc4) = wr[j];
    }
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) acc[mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_tile(0);
  for (int t = 0; t < ntiles; ++t) {
    store_tile();
    __syncthreads();
    if (t + 1 < ntiles) load_tile(t + 1);
    const float* wa = ws + lk * kLd + wm * 32 + lr;                  // A[row = ci][k = co]
    const float* gb_ = gs + (wn * 32 + lr) * kLdG + lk;              // B[k = co][col = pixel]
#pragma unroll
    for (int kk = 0; kk < kKT / 4; ++kk) {
      const float a0 = wa[kk * 4 * kLd], a1 = wa[kk * 4 * kLd + 16];
      const float b0 = gb_[kk * 4], b1 = gb_[kk * 4 + 16 * kLdG];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }

  // D of the 16x16x4 form: row (ci) = 4 * (lane / 16) + reg, column (pixel) = lane % 16: four consecutive ci of one pixel per lane
#pragma unroll
  for (int ni = 0; ni < 2; ++ni) {
    const int m = m0 + wn * 32 + ni * 16 + lr;
    if (m >= M) continue;
    const int img = m / (OH * OW), rem = m - img * (OH * OW);
    const int a = rem / OW, b = rem - a * OW;
    float* row = p.dx + ((size_t)(img * p.H + 2 * a + r) * p.W + 2 * b + s) * p.dx_cs + p.dx_coff;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int ci = ci0 + wm * 32 + mi * 16 + lk * 4;
      if (ci >= p.Ci) continue;
      float4 v = make_float4(acc[mi][ni][0], acc[mi][ni][1], acc[mi][ni][2], acc[mi][ni][3]);
      float4* dst = reinterpret_cast<float4*>(row + ci);
      if (p.accumulate) { const float4 o = *dst; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
      *dst = v;
    }
  }
}

// ---------------------------------------------------------------- weight gradient ----------------------------------------------------------------
struct S2WgradArgs {
  const float* x; int x_cs, x_coff;
  const float* g; int g_cs, g_coff;
  int n_img, H, W, Ci, Co;
  int relu_in, want_db;
  int chunks, ipc;                 // images per chunk = ceil(n_img / chunks)
  float* slab;                     // [chunks][Co][Ci * KS * KS]
  float* dbslab;                   // [chunks][Co]
};

template <int KS>
__global__ __launch_bounds__(256) void conv_s2_wgrad_kernel(S2WgradArgs p) {
  constexpr int PADC = (KS - 1) / 2;                 // the form's padding
  constexpr int LO = KS == 7 ? 2 : 1;                // -(smallest fw)
  constexpr int WROWS = kKT + LO + 1;                // rows of one x window: offsets -LO .. 1
  constexpr int GSLOTS = kKT * 16 / 256;             // float4 slots of the g tile per thread (2)
  constexpr int XSLOTS_ALL = 2 * WROWS * 16;         // float4 slots of the two column-phase windows
  constexpr int XSLOTS = (XSLOTS_ALL + 255) / 256;   // ... per thread (5)
  __shared__ __attribute__((aligned(16))) float gs[kKT * kLd];
  __shared__ __attribute__((aligned(16))) float xs[2 * WROWS * kLd];
  __shared__ int ows[kKT];                           // ow of the K-tile's positions

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;           // wave tile: 32 (co) x 32 (ci)
  const int lk = lane >> 4, lr = lane & 15;
  const int NT = (p.Ci + 63) >> 6;
  int bx = blockIdx.x;
  const int kh = bx % KS;
  bx /= KS;
  const int mt = bx / NT, nt = bx - mt * NT;
  const int co0 = mt * 64, ci0 = nt * 64;
  const int chunk = blockIdx.y;
  const int OH = p.H >> 1, OW = p.W >> 1;
  const int PW = OW, PP = OH * OW;                   // positions per row and per image (no padding: wp below is ow)
  const int img_b = chunk * p.ipc, img_e = min(p.n_img, img_b + p.ipc);
  const int qb = img_b * PP, qe = img_e * PP;
  const int ntiles = (qe - qb + kKT - 1) / kKT;
  const int rph = (kh - PADC) & 1, fh = (kh - PADC - rph) / 2;     // input row = 2 (oh + fh) + rph

  const float* gsrc = p.g + p.g_coff + co0;
  const float* xsrc = p.x + p.x_coff + ci0;

  // Every staged row of this thread is a fixed offset from the tile's first position, so its (image, output row, column) is
  // decoded once and then advanced by the K-tile's 32 positions with two carries: no division inside the K loop.
  const int adv_img = kKT / PP, adv_rem = kKT - adv_img * PP;
  const int adv_oh = adv_rem / PW, adv_wp = adv_rem - adv_oh * PW;
  int g_img[GSLOTS], g_oh[GSLOTS], g_wp[GSLOTS], x_img[XSLOTS], x_oh[XSLOTS], x_wp[XSLOTS];
  auto decode = [&](int q, int* img, int* oh, int* wp) {      // q >= -LO >= -2 PP
    const int qq = q + 2 * PP, i = qq / PP, rem = qq - i * PP;
    *img = i - 2;
    *oh = rem / PW;
    *wp = rem - *oh * PW;
  };
  auto advance = [&](int* img, int* oh, int* wp) {
    *wp += adv_wp;
    const int c = *wp >= PW;
    *wp -= c ? PW : 0;
    *oh += adv_oh + c;                                          // < 2 OH: adv_oh < OH
    const int c2 = *oh >= OH;
    *oh -= c2 ? OH : 0;
    *img += adv_img + c2;
  };
#pragma unroll
  for (int sl = 0; sl < GSLOTS; ++sl) decode(qb + ((tid + sl * 256) >> 4), &g_img[sl], &g_oh[sl], &g_wp[sl]);
#pragma unroll
  for (int sl = 0; sl < XSLOTS; ++sl) {
    const int rowall = (tid + sl * 256) >> 4;
    decode(qb + rowall % WROWS - LO, &x_img[sl], &x_oh[sl], &x_wp[sl]);
  }

  float4 gr[GSLOTS], xr[XSLOTS];
  int gow[GSLOTS];
  auto load_tile = [&]() {                                      // the tile at the slots' current positions; moves them to the next one
#pragma unroll
    for (int sl = 0; sl < GSLOTS; ++sl) {
      const int c4 = (tid + sl * 256) & 15;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (g_img[sl] < img_e) v = *reinterpret_cast<const float4*>(gsrc + ((size_t)(g_img[sl] * OH + g_oh[sl]) * OW + g_wp[sl]) * p.g_cs + c4 * 4);
      gr[sl] = v;
      gow[sl] = g_wp[sl];
      advance(&g_img[sl], &g_oh[sl], &g_wp[sl]);
    }
#pragma unroll
    for (int sl = 0; sl < XSLOTS; ++sl) {
      const int slot = tid + sl * 256;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (slot < XSLOTS_ALL) {
        const int sph = (slot >> 4) / WROWS, c4 = slot & 15;
        const int a = x_oh[sl] + fh;
        if (x_img[sl] >= 0 && x_img[sl] < p.n_img && ci0 + c4 * 4 < p.Ci && a >= 0 && a < OH) {
          v = *reinterpret_cast<const float4*>(xsrc + ((size_t)(x_img[sl] * p.H + 2 * a + rph) * p.W + 2 * x_wp[sl] + sph) * p.x_cs + c4 * 4);
          if (p.relu_in) v = relu4(v);
        }
        advance(&x_img[sl], &x_oh[sl], &x_wp[sl]);
      }
      xr[sl] = v;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int sl = 0; sl < GSLOTS; ++sl) {
      const int slot = tid + sl * 256, row = slot >> 4, c4 = slot & 15;
      *reinterpret_cast<float4*>(gs + row * kLd + c4 * 4) = gr[sl];
      if (c4 == 0) ows[row] = gow[sl];
    }
#pragma unroll
    for (int sl = 0; sl < XSLOTS; ++sl) {
      const int slot = tid + sl * 256;
      if (slot < XSLOTS_ALL) {
        const int rowall = slot >> 4, c4 = slot & 15;
        *reinterpret_cast<float4*>(xs + rowall * kLd + c4 * 4) = xr[sl];
      }
    }
  };

  f32x4 acc[KS][2][2];
#pragma unroll
  for (int t = 0; t < KS; ++t)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[t][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbsum = 0.f;
  const bool do_db = p.want_db && nt == 0 && kh == 0 && tid < 64;

  load_tile();
  for (int t = 0; t < ntiles; ++t) {
    store_tile();
    __syncthreads();
    if (t + 1 < ntiles) load_tile();
    if (do_db) {
#pragma unroll 8
      for (int k = 0; k < kKT; ++k) dbsum += gs[k * kLd + tid];
    }
    const float* ga = gs + lk * kLd + wm * 32 + lr;
    const float* xb = xs + lk * kLd + wn * 32 + lr;
#pragma unroll 2
    for (int kk = 0; kk < kKT / 4; ++kk) {
      const float a0 = ga[kk * 4 * kLd], a1 = ga[kk * 4 * kLd + 16];
      const int ow = ows[kk * 4 + lk];
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int d = kw - PADC, sph = d & 1, fw = (d - sph) / 2;        // column = 2 (ow + fw) + sph; folded at compile time
        const float* bp = xb + (sph * WROWS + kk * 4 + fw + LO) * kLd;
        const float b0 = bp[0], b1 = bp[16];
        const bool in = fw == 0 || (ow + fw >= 0 && ow + fw < OW);        // one compare per distinct fw: the taps of a phase share it
        const float m0 = in ? a0 : 0.f, m1 = in ? a1 : 0.f;
        acc[kw][0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(m0, b0, acc[kw][0][0], 0, 0, 0);
        acc[kw][0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(m0, b1, acc[kw][0][1], 0, 0, 0);
        acc[kw][1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(m1, b0, acc[kw][1][0], 0, 0, 0);
        acc[kw][1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(m1, b1, acc[kw][1][1], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // D of the 16x16x4 form: row (co) = 4 * (lane / 16) + reg, column (ci) = lane % 16
  float* slab = p.slab + (size_t)chunk * p.Co * p.Ci * (KS * KS);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int ci = ci0 + wn * 32 + ni * 16 + lr;
      if (ci >= p.Ci) continue;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int co = co0 + wm * 32 + mi * 16 + lk * 4 + reg;
        float* dst = slab + ((size_t)co * p.Ci + ci) * (KS * KS) + kh * KS;
#pragma unroll
        for (int t = 0; t < KS; ++t) dst[t] = acc[t][mi][ni][reg];
      }
    }
  if (do_db) p.dbslab[(size_t)chunk * p.Co + co0 + tid] = dbsum;
}

}  // namespace

bool conv_s2_bwd_supported(int n_img, int H, int W, int Ci, int Co, int KH, int KW) {
  if (n_img < 1 || H < 2 || W < 2 || (H & 1) || (W & 1) || Ci < 32 || Co < 64 || Ci % 32 || Co % 64 || KH != KW || (KH != 5 && KH != 7)) return false;
  const long long PP = (long long)(H / 2) * (W / 2);
  if (PP * n_img > 0x7fffffffLL - 4096 || (long long)n_img * H * W > 0x7fffffffLL || (long long)Ci * Co * KH * KW > 0x7fffffffLL) return false;
  return true;
}

// The plan of one stride-2 conv's backward: a function of these seven integers only.
//   weight gradient: tiles = (Co / 64) ceil(Ci / 64) k blocks per chunk; as many chunks as fit the resident slots in one round, but a chunk
//   no shorter than kS2MinPositions output pixels; whole images per chunk, ceil(n_img / chunks) each (conv_wgrad_chunks, conv_bwd.hip)
//   data gradient: the phase-major weight, nothing else (K is not split)
bool conv_s2_bwd_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_floats, size_t* weight_floats, int* chunks_out) {
  if (!conv_s2_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return false;
  const int KK = KH * KW;
  const long long PP = (long long)(H / 2) * (W / 2);
  const long long tiles = (long long)(Co / 64) * ((Ci + 63) / 64) * KH;
  const int chunks = conv_wgrad_chunks(n_img, PP, tiles, kS2Slots, kS2MinPositions);
  if (data_floats) *data_floats = (size_t)Co * Ci * KK;
  if (weight_floats) *weight_floats = (size_t)chunks * ((size_t)Co * Ci * KK + Co);
  if (chunks_out) *chunks_out = chunks;
  return true;
}

hipError_t conv_s2_bwd_data_launch(const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw, int Ci, int KS,
                                   int pad, float* dx, int dx_cs, int dx_coff, int accumulate, float* scratch, hipStream_t st) {
  const size_t wfloats = (size_t)Co * Ci * KS * KS;
  int blocks = (int)((wfloats + 255) / 256 < 4096 ? (wfloats + 255) / 256 : 4096);
  hipLaunchKernelGGL(conv_s2_pack_kernel, dim3(blocks), dim3(256), 0, st, w_oihw, scratch, Co, Ci, KS, pad);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  S2DgradArgs a;
  a.g = g; a.g_cs = g_cs; a.g_coff = g_coff; a.wp = scratch; a.dx = dx; a.dx_cs = dx_cs; a.dx_coff = dx_coff;
  a.n_img = n_img; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.KS = KS; a.pad = pad; a.accumulate = accumulate;
  const long long M = (long long)n_img * (H / 2) * (W / 2);
  const dim3 grid((unsigned)((M + 63) / 64), (Ci + 63) / 64, 4);
  hipLaunchKernelGGL(conv_s2_dgrad_kernel, grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t conv_s2_bwd_weight_launch(const float* x, int x_cs, int x_coff, const float* g, int g_cs, int g_coff, int n_img, int H, int W,
                                     int Ci, int Co, int KS, int relu_in, float* dw, float* db, int accumulate, float* scratch,
                                     int chunks, hipStream_t st) {
  S2WgradArgs a;
  a.x = x; a.x_cs = x_cs; a.x_coff = x_coff; a.g = g; a.g_cs = g_cs; a.g_coff = g_coff;
  a.n_img = n_img; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.relu_in = relu_in; a.want_db = db != nullptr;
  a.chunks = chunks; a.ipc = (n_img + chunks - 1) / chunks;
  a.slab = scratch; a.dbslab = scratch + (size_t)chunks * Co * Ci * KS * KS;
  const dim3 grid((Co / 64) * ((Ci + 63) / 64) * KS, chunks);
  if (KS == 7) hipLaunchKernelGGL(conv_s2_wgrad_kernel<7>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(conv_s2_wgrad_kernel<5>, grid, dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return conv_wgrad_reduce_launch(a.slab, a.dbslab, Co, Ci, KS * KS, chunks, dw, db, accumulate, st);
}

}  // namespace offk
