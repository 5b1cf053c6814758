// K4b. Backward of one stride-1 fusion convolution (k = 1 or 3, pad = (k - 1) / 2), exact fp32: the ReLU mask, the data gradient
// (the library's own direct conv on the transposed, 180-degree rotated weight) and the weight / bias gradient (a TN GEMM over the
// pixels on the fp32 matrix pipe, v_mfma_f32_16x16x4_f32, split over K at image granularity).
//
// Weight gradient, one block = one 64 (co) x 64 (ci) tile of dw for ALL k*k taps over one chunk of images:
//   K runs over the PADDED pixel positions q of the chunk: an image is (H + 2)(W + 2) positions with a zero ring (k = 3) or its H * W
//   pixels (k = 1), images back to back, so a 32-position K-tile packs across image boundaries.  g is staged with zeros on the ring, x
//   with zeros on the ring and outside the tensor, and the nine taps become nine row offsets into the staged x:
//       dw[co][ci][kh][kw] = sum_q g_pad[q][co] * x_pad[q + (kh - 1)(W + 2) + (kw - 1)][ci]
//   (g_pad[q] != 0 only inside an image, where every shifted position stays inside that image's padded block).  Per K-tile a block
//   stages the g rows and, per kernel row kh, ONE window of 32 + 2 x rows; the three kw taps of a kernel row read that window at row
//   offsets 0, 1, 2.  Rows are [position][channel] in LDS with an 80-float stride: the MFMA operand of a lane is the single float
//   [4 kk + lane / 16][tile + lane % 16], and four consecutive rows then cover all 64 banks -- this is the transposing stage, K moves
//   from the slow index of the channels-last rows to the MFMA's k lanes with no shuffle.
//   The next K-tile's rows are loaded into registers before the MFMAs of the current one and stored to LDS behind them.
// The partial tiles go to slab [chunk][Co][Ci * k * k] (the layout of dw itself) and the column sums of g to [chunk][Co] behind the
// slabs; conv_wgrad_reduce_kernel adds the slabs in chunk order -- the split-K rule of the library: the same bits on every run.
#include "offk_common.h"
#include "offk_internal.h"

namespace offk {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kWgKT = 32;        // positions per K-tile
constexpr int kWgLd = 80;        // LDS row stride in floats (64 channels + 16: rows r .. r + 3 start 16 banks apart)
constexpr int kWgSlots3 = 512;         // 3x3: two blocks per CU on 256 CUs are resident (224 registers, 42 KB of LDS per block)
constexpr int kWgSlots1 = 1024;        // 1x1: four blocks per CU (60 registers, 20 KB)
constexpr int kWgMinPositions = 256;   // a chunk is at least eight K-tiles long (unless the whole problem is shorter)

struct WgradArgs {
  const float* x; int x_cs, x_coff;
  const float* g; int g_cs, g_coff;
  int n_img, H, W, Ci, Co;
  int relu_in, want_db;
  int chunks, ipc;                 // images per chunk = ceil(n_img / chunks)
  float* slab;                     // [chunks][Co][Ci * KK]
  float* dbslab;                   // [chunks][Co]
  float* dw; float* db; int accumulate;
};

// pixel row index of padded position q (>= 0 and < n_img * PP is the caller's business), or -1 on the zero ring
template <int KS>
__device__ __forceinline__ long long wg_pixel(int q, int H, int W) {
  if constexpr (KS == 1) {
    return q;
  } else {
    const int PW = W + 2, PP = (H + 2) * PW;
    const int img = q / PP, rem = q - img * PP;
    const int hp = rem / PW, wp = rem - hp * PW;
    if (hp == 0 || hp == H + 1 || wp == 0 || wp == W + 1) return -1;
    return ((long long)img * H + (hp - 1)) * W + (wp - 1);
  }
}

template <int KS>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(WgradArgs p) {
  constexpr int KK = KS * KS;
  constexpr int WROWS = kWgKT + KS - 1;              // rows of one x window
  constexpr int GSLOTS = kWgKT * 16 / 256;           // float4 slots of the g tile per thread (2)
  constexpr int XSLOTS_ALL = KS * WROWS * 16;        // float4 slots of the x windows
  constexpr int XSLOTS = (XSLOTS_ALL + 255) / 256;   // ... per thread (2 or 7)
  __shared__ __attribute__((aligned(16))) float gs[kWgKT * kWgLd];
  __shared__ __attribute__((aligned(16))) float xs[KS * WROWS * kWgLd];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;           // wave tile: 32 (co) x 32 (ci)
  const int lk = lane >> 4, lr = lane & 15;
  const int NT = p.Ci >> 6;
  const int mt = blockIdx.x / NT, nt = blockIdx.x - mt * NT;
  const int co0 = mt * 64, ci0 = nt * 64;
  const int chunk = blockIdx.y;
  const int PW = KS == 1 ? p.W : p.W + 2;
  const int PP = KS == 1 ? p.H * p.W : (p.H + 2) * PW;
  const int img_b = chunk * p.ipc, img_e = min(p.n_img, img_b + p.ipc);
  const int qb = img_b * PP, qe = img_e * PP, q_all = p.n_img * PP;
  const int ntiles = (qe - qb + kWgKT - 1) / kWgKT;

  const float* gsrc = p.g + p.g_coff + co0;
  const float* xsrc = p.x + p.x_coff + ci0;

  float4 gr[GSLOTS], xr[XSLOTS];
  auto load_tile = [&](int q0) {
#pragma unroll
    for (int s = 0; s < GSLOTS; ++s) {
      const int slot = tid + s * 256, row = slot >> 4, c4 = slot & 15;
      const int q = q0 + row;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q < qe) {
        const long long pix = wg_pixel<KS>(q, p.H, p.W);
        if (pix >= 0) v = *reinterpret_cast<const float4*>(gsrc + pix * p.g_cs + c4 * 4);
      }
      gr[s] = v;
    }
#pragma unroll
    for (int s = 0; s < XSLOTS; ++s) {
      const int slot = tid + s * 256;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (slot < XSLOTS_ALL) {
        const int rowall = slot >> 4, c4 = slot & 15;
        const int kh = rowall / WROWS, r = rowall - kh * WROWS;
        const int q = KS == 1 ? q0 + r : q0 + (kh - 1) * PW - 1 + r;
        if (q >= 0 && q < q_all) {
          const long long pix = wg_pixel<KS>(q, p.H, p.W);
          if (pix >= 0) {
            v = *reinterpret_cast<const float4*>(xsrc + pix * p.x_cs + c4 * 4);
            if (p.relu_in) v = relu4(v);
          }
        }
      }
      xr[s] = v;
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int s = 0; s < GSLOTS; ++s) {
      const int slot = tid + s * 256, row = slot >> 4, c4 = slot & 15;
      *reinterpret_cast<float4*>(gs + row * kWgLd + c4 * 4) = gr[s];
    }
#pragma unroll
    for (int s = 0; s < XSLOTS; ++s) {
      const int slot = tid + s * 256;
      if (slot < XSLOTS_ALL) {
        const int rowall = slot >> 4, c4 = slot & 15;
        *reinterpret_cast<float4*>(xs + rowall * kWgLd + c4 * 4) = xr[s];
      }
    }
  };

  f32x4 acc[KK][2][2];
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
      for (int ni = 0; ni < 2; ++ni) acc[t][mi][ni] = f32x4{0.f, 0.f, 0.f, 0.f};
  float dbsum = 0.f;
  const bool do_db = p.want_db && nt == 0 && tid < 64;

  load_tile(qb);
  for (int t = 0; t < ntiles; ++t) {
    store_tile();
    __syncthreads();
    if (t + 1 < ntiles) load_tile(qb + (t + 1) * kWgKT);
    if (do_db) {
#pragma unroll 8
      for (int k = 0; k < kWgKT; ++k) dbsum += gs[k * kWgLd + tid];
    }
    const float* ga = gs + lk * kWgLd + wm * 32 + lr;
    const float* xb = xs + lk * kWgLd + wn * 32 + lr;
#pragma unroll 2
    for (int kk = 0; kk < kWgKT / 4; ++kk) {
      const float a0 = ga[kk * 4 * kWgLd], a1 = ga[kk * 4 * kWgLd + 16];
#pragma unroll
      for (int kh = 0; kh < KS; ++kh)
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
          const float* bp = xb + (kh * WROWS + kk * 4 + kw) * kWgLd;
          const float b0 = bp[0], b1 = bp[16];
          const int tap = kh * KS + kw;
          acc[tap][0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[tap][0][0], 0, 0, 0);
          acc[tap][0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[tap][0][1], 0, 0, 0);
          acc[tap][1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[tap][1][0], 0, 0, 0);
          acc[tap][1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[tap][1][1], 0, 0, 0);
        }
    }
    __syncthreads();
  }

  // D of the 16x16x4 form: row (co) = 4 * (lane / 16) + reg, column (ci) = lane % 16
  float* slab = p.slab + (size_t)chunk * p.Co * p.Ci * KK;
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
      const int ci = ci0 + wn * 32 + ni * 16 + lr;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int co = co0 + wm * 32 + mi * 16 + lk * 4 + reg;
        float* dst = slab + ((size_t)co * p.Ci + ci) * KK;
#pragma unroll
        for (int t = 0; t < KK; ++t) dst[t] = acc[t][mi][ni][reg];
      }
    }
  if (do_db) p.dbslab[(size_t)chunk * p.Co + co0 + tid] = dbsum;
}

// dw[i] (+)= slab[0][i] + slab[1][i] + ... in chunk order; the same for db behind it
__global__ __launch_bounds__(256) void conv_wgrad_reduce_kernel(WgradArgs p, int KK) {
  const size_t nw = (size_t)p.Co * p.Ci * KK;
  const size_t n = nw + (p.want_db ? p.Co : 0);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const bool is_w = i < nw;
    const float* src = is_w ? p.slab + i : p.dbslab + (i - nw);
    const size_t step = is_w ? nw : (size_t)p.Co;
    // chunk order, sixteen loads in flight: a thread's loads are independent, only its additions are a chain
    float v = src[0];
    int z = 1;
    for (; z + 16 <= p.chunks; z += 16) {
      float t[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) t[j] = src[(size_t)(z + j) * step];
#pragma unroll
      for (int j = 0; j < 16; ++j) v += t[j];
    }
    for (; z < p.chunks; ++z) v += src[(size_t)z * step];
    float* dst = is_w ? p.dw + i : p.db + (i - nw);
    *dst = p.accumulate ? *dst + v : v;
  }
}

// [Co][Ci][k][k] -> the library's K order of the TRANSPOSED conv, rotated by 180 degrees: [Ci][Co / 32][k * k][32]
__global__ void pack_oihw_rot_kernel(const float* __restrict__ src, float* __restrict__ dst, int Co, int Ci, int KK) {
  const size_t n = (size_t)Co * Ci * KK;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int cl = (int)(i & 31);
    size_t t = i >> 5;
    const int tap = (int)(t % KK);
    t /= KK;
    const int chunk = (int)(t % (Co >> 5));
    const int ci = (int)(t / (Co >> 5));
    dst[i] = src[((size_t)(chunk * 32 + cl) * Ci + ci) * KK + (KK - 1 - tap)];
  }
}

// g = dy where y > 0, else exactly 0 (y <= 0, -0.0, NaN); 16-byte accesses, C % 4 == 0
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* dy, int dy_cs, const float* __restrict__ y, int y_cs, float* g, int g_cs,
                                                       size_t rows, int C4, int accumulate) {
  const size_t n = rows * C4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t row = i / C4;
    const int c = (int)(i - row * C4) * 4;
    const float4 d = *reinterpret_cast<const float4*>(dy + row * dy_cs + c);
    const float4 m = *reinterpret_cast<const float4*>(y + row * y_cs + c);
    float4 v;
    v.x = m.x > 0.f ? d.x : 0.f; v.y = m.y > 0.f ? d.y : 0.f; v.z = m.z > 0.f ? d.z : 0.f; v.w = m.w > 0.f ? d.w : 0.f;
    float4* dst = reinterpret_cast<float4*>(g + row * g_cs + c);
    if (accumulate) { const float4 o = *dst; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
    *dst = v;
  }
}

}  // namespace

bool conv_bwd_supported(int n_img, int H, int W, int Ci, int Co, int KH, int KW) {
  if (n_img < 1 || H < 1 || W < 1 || Ci < 64 || Co < 64 || Ci % 64 || Co % 64 || KH != KW || (KH != 1 && KH != 3)) return false;
  const long long PP = KH == 1 ? (long long)H * W : (long long)(H + 2) * (W + 2);
  if (PP * n_img > 0x7fffffffLL - 4096 || (long long)Ci * Co * KH * KW > 0x7fffffffLL) return false;
  return true;
}

// The chunk rule of every conv weight gradient (fp32 and split-fp32, stride 1 and 2): as many chunks as FIT `slots` resident blocks in one
// round at `tiles` blocks per chunk, but a chunk no shorter than `min_positions` positions (a block's slab write and its share of the
// reduce are paid per chunk); whole images per chunk, ceil(n_img / chunks) each, settled so that no chunk is empty
int conv_wgrad_chunks(int n_img, long long positions_per_image, long long tiles, int slots, int min_positions) {
  long long want = slots / tiles;
  const long long min_imgs = (min_positions + positions_per_image - 1) / positions_per_image;
  const long long max_chunks = (n_img + min_imgs - 1) / min_imgs;
  if (want > max_chunks) want = max_chunks;
  if (want < 1) want = 1;
  int chunks = (int)want;
  for (;;) {       // settle on chunks == ceil(n_img / ceil(n_img / chunks)): the kernels derive the images per chunk
    const int ipc = (n_img + chunks - 1) / chunks;
    const int c2 = (n_img + ipc - 1) / ipc;
    if (c2 == chunks) break;
    chunks = c2;
  }
  return chunks;
}

// The plan of one conv's backward: a function of these seven integers only.
//   weight gradient: tiles = (Co / 64)(Ci / 64) blocks per chunk; as many chunks as FIT the resident slots in one round (floor: 520
//   blocks on 512 slots ran 832 -> 256 in two rounds, 1.69 ms; 468 blocks in one), but a chunk no shorter than kWgMinPositions padded
//   positions (a block's slab write and its share of the reduce are paid per chunk); whole images per chunk, ceil(n_img / chunks) each
//   data gradient: the direct conv's own automatic plan (conv2d_auto_plan) for the transposed problem
bool conv_bwd_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_floats, size_t* weight_floats, int* chunks_out,
                   int* dgrad_splitk) {
  if (!conv_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return false;
  const int KK = KH * KW;
  const long long PP = KH == 1 ? (long long)H * W : (long long)(H + 2) * (W + 2);
  const long long tiles = (long long)(Co / 64) * (Ci / 64);
  const int chunks = conv_wgrad_chunks(n_img, PP, tiles, KH == 1 ? kWgSlots1 : kWgSlots3, kWgMinPositions);
  const long long M = (long long)n_img * H * W;
  const int nkt = KK * (Co / 32);
  int cfg = 3, sk = 1;
  conv2d_auto_plan(M, Ci, nkt, &cfg, &sk, 0);
  if (sk > nkt) sk = nkt;
  if (sk < 1) sk = 1;
  if (data_floats) *data_floats = (size_t)Co * Ci * KK + (sk > 1 ? (size_t)sk * (size_t)M * Ci : 0);
  if (weight_floats) *weight_floats = (size_t)chunks * ((size_t)Co * Ci * KK + Co);
  if (chunks_out) *chunks_out = chunks;
  if (dgrad_splitk) *dgrad_splitk = sk;
  return true;
}

hipError_t relu_backward_launch(const float* dy, int dy_cs, int dy_coff, const float* y, int y_cs, int y_coff, long long rows, int C, float* g,
                                int g_cs, int g_coff, int accumulate, hipStream_t st) {
  const size_t n4 = (size_t)rows * (C / 4);
  int blocks = (int)((n4 + 255) / 256 < 4096 ? (n4 + 255) / 256 : 4096);
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(relu_bwd_kernel, dim3(blocks), dim3(256), 0, st, dy + dy_coff, dy_cs, y + y_coff, y_cs, g + g_coff, g_cs, (size_t)rows, C / 4,
                     accumulate);
  return hipGetLastError();
}

hipError_t conv_bwd_data_launch(const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw, int Ci, int KS,
                                float* dx, int dx_cs, int dx_coff, int accumulate, float* scratch, size_t scratch_floats, hipStream_t st,
                                const char** why) {
  *why = nullptr;
  const int KK = KS * KS;
  const size_t wfloats = (size_t)Co * Ci * KK;
  int blocks = (int)((wfloats + 255) / 256 < 4096 ? (wfloats + 255) / 256 : 4096);
  hipLaunchKernelGGL(pack_oihw_rot_kernel, dim3(blocks), dim3(256), 0, st, w_oihw, scratch, Co, Ci, KK);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  ConvDesc d;
  d.x = g; d.x_cs = g_cs; d.x_coff = g_coff; d.n_img = n_img; d.H = H; d.W = W; d.Ci = Co;
  d.w = scratch; d.bias = nullptr; d.Co = Ci; d.KH = KS; d.KW = KS; d.stride = 1; d.pad = (KS - 1) / 2;
  // accumulate: dx as the conv's residual, in place -- every element of the residual is read by the thread that stores it, right before
  // the store, in the unsplit epilogue and in splitk_reduce_kernel alike
  d.res = accumulate ? dx : nullptr; d.res_cs = dx_cs; d.res_coff = dx_coff;
  d.flags = 0;
  d.y = dx; d.y_cs = dx_cs; d.y_coff = dx_coff;
  d.partial = scratch + wfloats; d.partial_floats = scratch_floats - wfloats;
  return conv2d_launch(d, st, why);
}

hipError_t conv_bwd_weight_launch(const float* x, int x_cs, int x_coff, const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Ci,
                                  int Co, int KS, int relu_in, float* dw, float* db, int accumulate, float* scratch, int chunks,
                                  hipStream_t st) {
  WgradArgs a;
  a.x = x; a.x_cs = x_cs; a.x_coff = x_coff; a.g = g; a.g_cs = g_cs; a.g_coff = g_coff;
  a.n_img = n_img; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.relu_in = relu_in; a.want_db = db != nullptr;
  a.chunks = chunks; a.ipc = (n_img + chunks - 1) / chunks;
  a.slab = scratch; a.dbslab = scratch + (size_t)chunks * Co * Ci * KS * KS;
  a.dw = dw; a.db = db; a.accumulate = accumulate;
  const dim3 grid((Co / 64) * (Ci / 64), chunks);
  if (KS == 1) hipLaunchKernelGGL(conv_wgrad_kernel<1>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(conv_wgrad_kernel<3>, grid, dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t n = (size_t)Co * Ci * KS * KS + Co;
  int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, st, a, KS * KS);
  return hipGetLastError();
}

// the same reduce for the slabs of another weight-gradient kernel (conv_bwd_s2.hip): one kernel, one summation order
hipError_t conv_wgrad_reduce_launch(float* slab, float* dbslab, int Co, int Ci, int KK, int chunks, float* dw, float* db, int accumulate,
                                    hipStream_t st) {
  WgradArgs a = {};
  a.Ci = Ci; a.Co = Co; a.want_db = db != nullptr; a.chunks = chunks;
  a.slab = slab; a.dbslab = dbslab; a.dw = dw; a.db = db; a.accumulate = accumulate;
  const size_t n = (size_t)Co * Ci * KK + Co;
  int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(conv_wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, st, a, KK);
  return hipGetLastError();
}

}  // namespace offk
