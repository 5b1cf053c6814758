// K4b, stride 2: the weight / bias gradient of the two stage openers (7x7 / 2 / 3 and 5x5 / 2 / 2) in split-fp32 arithmetic on the bf16
// matrix pipe (offk_conv2d_s2_backward_weight_split).  conv_s2_wgrad_kernel's decomposition (conv_bwd_s2.hip) with
// conv_wgrad_split_kernel's operand handling (conv_wgrad_split.hip):
//     dw[co][ci][kh][kw] = sum_{n, oh, ow} g[n, oh, ow, co] * in(x)[n, 2 (oh + fh) + rph, 2 (ow + fw) + sph, ci],   db[co] = sum g
//   with rph = (kh - pad) & 1, fh = floor((kh - pad) / 2) and sph, fw the same for kw (fw = -2 .. 1 for the 7x7, -1 .. 1 for the 5x5).
// Both operands are cut into THREE bf16 planes by truncation (sp_cut of split_common.h = synth.cut3) and per 32-position step and tap
// six of the nine plane products are issued on v_mfma_f32_16x16x32_bf16 in synth.SPLIT_PRODUCTS order with g in the role of w: g_l x_h,
// g_h x_l, g_m x_m, g_m x_h, g_h x_m into accumulator A2, g_h x_h into A1; steps in increasing order, the block's partial tile is A1 + A2,
// added once: synth.emulate_split_dot(form="units") over the block's chunk.  The slabs [chunk][Co][Ci k k] (+ [chunk][Co]) are summed in
// chunk order by the unchanged conv_wgrad_reduce_kernel (conv_bwd.hip).
//
// K order (include/offk.h states it for callers; tests/conv_s2_wgrad_split.py follows it on the CPU).  K runs over the OUTPUT pixels
// q = (img * OH + oh) * OW + ow, real pixels only, images back to back, PP = OH OW positions per image: no zero column, no zero row.  A chunk
// holds the positions [img_b * PP, img_e * PP) of its ceil(n_img / chunks) whole images; its step t holds the 32 positions from
// img_b * PP + 32 t on, both operands zero from img_e * PP on (the last step of a chunk may be partly empty).  Tap (kh, kw) pairs g at q with
// X_(kh, kw)[q] = in(x)[img, 2 oh + kh - pad, 2 ow + kw - pad], ZERO where that row or column leaves the map: the taps are removed on the x
// side, so the step loop has no select on g and no table of columns (the fp32 kernel's way).
// Eight consecutive k of one channel are one lane's 16-byte MFMA operand, so a tap's column shift cannot be an operand offset: one block
// owns ONE kernel row kh (as the fp32 kernel) and stages one x plane image PER kw, 7 or 5 of them, each 32 positions x 64 ci x 3 planes =
// 12 KB, beside the 12 KB of g: 96 KB (7x7) or 72 KB (5x5) of LDS per buffer; the 5x5 has two buffers and one barrier per step, the 7x7 one
// buffer and two barriers (two would be 192 KB).  Plane images are [plane][16-row tile][k group][16 rows] x 16 B with row r
// of a (tile, k group) piece at r ^ (k group & 3): conv_wgrad_split_kernel's layout and its loader's thread mapping (a thread stores the
// four rows of one position quad; sixteen lanes of a ds_write_b64 hit sixteen different 8-byte slots).
// Loader: one unit = (image, position quad, channel quad): four 16-byte loads -- the quad's four positions are decoded one from the other
// with two carries, so a quad may straddle rows and images --, sixteen cuts, twelve 8-byte LDS stores.  7 + 1 (5 + 1) images x 128 units
// over 512 threads: two units per thread (7x7) or one and a half (5x5), an image's 128 units on two whole waves.  Each x value is loaded
// and cut once per tap that reads it (3 or 4 times per kernel row for the 7x7); the loads hit the L1 / L2.  The position of a thread's
// quad advances by the step's 32 positions with two carries: no division in the K loop.  The next step's rows are loaded into registers
// before the MFMAs of the current one, unconditionally (a position that is a zero reads the view's first row), and replaced by zeros,
// passed through the ReLU and cut into LDS behind them: nothing reads a load's result in front of the MFMAs.  A half ci tile (Ci % 64 == 32) stages zeros for its upper half and does not store it.
// Geometry: eight waves, wave w owns co tiles 2 (w & 1) .. + 1 x ci tile (w >> 1) x k taps x (A1, A2) = 112 (7x7) or 80 (5x5) accumulator
// registers, one block per CU (two waves per SIMD, 256 registers each; build.py's register guard).
// db is the fp32 sum of the g rows as loaded, per thread over its position quads in step order, then over the eight quads of a step in a
// fixed order: nothing is split.  The blocks of kernel row 0 and ci tile 0 write it.
#include "offk_common.h"
#include "offk_internal.h"
#include "split_common.h"

namespace offk {
namespace {

constexpr int kWsKT = 32;               // positions per step
// block slots the plan fills (A/B builds of tools/bench_fusion_bwd_s2.py --wgrad-arith f32split override them; DESIGN.md 8.9 has the times)
#ifndef OFFK_S2S_SLOTS7
#define OFFK_S2S_SLOTS7 256
#endif
#ifndef OFFK_S2S_SLOTS5
#define OFFK_S2S_SLOTS5 512
#endif
constexpr int kWsSlots7 = OFFK_S2S_SLOTS7;   // 7x7: one round of one block per CU (35 tiles: 7 chunks = 245 blocks)
constexpr int kWsSlots5 = OFFK_S2S_SLOTS5;   // 5x5: two rounds of one block per CU (170 tiles: 3 chunks = 510 blocks)
constexpr int kWsMinPositions = 256;    // a chunk is at least eight steps long (unless the whole problem is shorter)
constexpr int kWsPlane = 4096;          // one plane of an image: 4 tiles x 4 k groups x 256 B
constexpr int kWsImage = 3 * kWsPlane;  // x images 0 .. KS - 1, then g

struct WsArgs {
  const float* x; int x_cs, x_coff;
  const float* g; int g_cs, g_coff;
  int n_img, H, W, Ci, Co;
  int relu_in, want_db;
  int ipc;                        // images per chunk = ceil(n_img / chunks)
  float* slab;                    // [chunks][Co][Ci * KS * KS]
  float* dbslab;                  // [chunks][Co]
};

template <int KS>
__global__ __launch_bounds__(512) void conv_s2_wgrad_split_kernel(WsArgs p) {
  constexpr int PADC = (KS - 1) / 2;                 // the form's padding
  constexpr int NBUF = KS == 5 ? 2 : 1;              // LDS buffers: two fit for the 5x5 (144 KB), one for the 7x7 (96 KB)
  constexpr int BUFB = (KS + 1) * kWsImage;          // bytes of one buffer
  extern __shared__ __attribute__((aligned(16))) char lds[];   // [buffer][KS x images, then g][3 planes][4 tiles][4 k groups][256 B]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int NT = (p.Ci + 63) >> 6;
  int bx = blockIdx.x;
  const int kh = bx % KS;
  bx /= KS;
  const int mtile = bx / NT, ntile = bx - mtile * NT;
  const int co0 = mtile * 64, ci0 = ntile * 64;
  const int chunk = blockIdx.y;
  const int H = p.H, W = p.W, OH = H >> 1, OW = W >> 1, PP = OH * OW;
  const int img_b = chunk * p.ipc, img_e = min(p.n_img, img_b + p.ipc);
  const int nsteps = (int)(((long long)(img_e - img_b) * PP + kWsKT - 1) / kWsKT);
  const int rph = (kh - PADC) & 1, fh = (kh - PADC - rph) / 2;     // input row = 2 (oh + fh) + rph

  // ---- loader roles: unit s of this thread is (image (wave >> 1) + 4 s, position quad pq, channel quad cq) ----
  const int item = tid & 127, pq = item & 7, cq = item >> 3;
  const int slot = pq >> 1, half = pq & 1;                 // the k group of the quad and its half of the 16 bytes
  bool on[2], is_g[2], cok[2];
  int ufh[2], ufw[2], umul[2], uy0[2], ux0[2], uHs[2], uWs[2], ucs[2];
  const float* usrc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int im = (wave >> 1) + 4 * s;
    on[s] = im <= KS;
    is_g[s] = im == KS;
    const int d = im - PADC, sph = d & 1, fw = (d - sph) / 2;       // column = 2 (ow + fw) + sph
    if (is_g[s]) {
      ufh[s] = 0; ufw[s] = 0; umul[s] = 1; uy0[s] = 0; ux0[s] = 0; uHs[s] = OH; uWs[s] = OW; ucs[s] = p.g_cs;
      usrc[s] = p.g + p.g_coff + co0 + 4 * cq;
      cok[s] = true;
    } else {
      ufh[s] = fh; ufw[s] = fw; umul[s] = 2; uy0[s] = rph; ux0[s] = sph; uHs[s] = H; uWs[s] = W; ucs[s] = p.x_cs;
      cok[s] = on[s] && ci0 + 4 * cq < p.Ci;
      usrc[s] = p.x + p.x_coff + (cok[s] ? ci0 + 4 * cq : 0);
    }
  }
  // the ReLU of the x units as max(v, lo): lo = 0, or a quiet NaN where there is none (v_max_f32 returns its other operand: v, bit for bit)
  float ulo[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) ulo[s] = (p.relu_in != 0 && !is_g[s]) ? 0.f : __uint_as_float(0x7FC00000u);

  // the quad's first position q = img_b * PP + 32 t + 4 pq as (image, output row, column): decoded once, then advanced by the step's 32
  // positions with two carries
  const int adv_img = kWsKT / PP, adv_rem = kWsKT - adv_img * PP;
  const int adv_oh = adv_rem / OW, adv_ow = adv_rem - adv_oh * OW;
  int q_img, q_oh, q_ow;
  {
    const int rel = 4 * pq, i = rel / PP, rem = rel - i * PP;
    q_img = img_b + i;
    q_oh = rem / OW;
    q_ow = rem - q_oh * OW;
  }

  float4 r[2][4];
  unsigned vbits = 0;             // bit 4 s + j: load j of unit s is a value (else a zero: it read the view's first row)
  // Unconditional loads and nothing else: a position that is a zero reads the view's first row, and the value is replaced (and the ReLU
  // applied) in store_step, BEHIND the MFMAs of the step in between -- nothing here reads a load's result, so no wait for it stands in
  // front of the MFMAs and no branch around it.  A unit that has no image (5x5: the last two of sixteen) loads zeros it never stores.
  auto load_step = [&]() {
    int pi[4], po[4], pw[4];
    pi[0] = q_img; po[0] = q_oh; pw[0] = q_ow;
#pragma unroll
    for (int j = 1; j < 4; ++j) {
      const int w1 = pw[j - 1] + 1;
      const bool c = w1 == OW;
      pw[j] = c ? 0 : w1;
      const int o1 = po[j - 1] + (c ? 1 : 0);
      const bool c2 = o1 == OH;
      po[j] = c2 ? 0 : o1;
      pi[j] = pi[j - 1] + (c2 ? 1 : 0);
    }
    unsigned vb = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int a = po[j] + ufh[s], b = pw[j] + ufw[s];
        const bool valid = cok[s] && pi[j] < img_e && (unsigned)a < (unsigned)OH && (unsigned)b < (unsigned)OW;
        const unsigned row = ((unsigned)pi[j] * (unsigned)uHs[s] + (unsigned)(umul[s] * a + uy0[s])) * (unsigned)uWs[s] + (unsigned)(umul[s] * b + ux0[s]);
        const float* ptr = usrc[s] + (size_t)(valid ? row : 0u) * (size_t)ucs[s];
        r[s][j] = *reinterpret_cast<const float4*>(ptr);
        vb |= (valid ? 1u : 0u) << (4 * s + j);
      }
    }
    vbits = vb;
    q_ow += adv_ow;
    const bool c = q_ow >= OW;
    q_ow -= c ? OW : 0;
    q_oh += adv_oh + (c ? 1 : 0);                         // < 2 OH: adv_oh < OH
    const bool c2 = q_oh >= OH;
    q_oh -= c2 ? OH : 0;
    q_img += adv_img + (c2 ? 1 : 0);
  };

  float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
  // where this thread's 8 bytes of (row 4 (cq & 3) + i, its k group, its half) lie inside a plane: + i * 16 before the swizzle
  char* const dst0 = lds + (cq >> 2) * 1024 + slot * 256 + half * 8;
  auto store_step = [&](int buf) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (!on[s]) continue;                               // (wave-uniform)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned keep = 0u - ((vbits >> (4 * s + j)) & 1u);
        float4 v = r[s][j];
        v.x = fmaxf(__uint_as_float(__float_as_uint(v.x) & keep), ulo[s]); v.y = fmaxf(__uint_as_float(__float_as_uint(v.y) & keep), ulo[s]);
        v.z = fmaxf(__uint_as_float(__float_as_uint(v.z) & keep), ulo[s]); v.w = fmaxf(__uint_as_float(__float_as_uint(v.w) & keep), ulo[s]);
        r[s][j] = v;
      }
      if (is_g[s]) {
        bs.x += (r[s][0].x + r[s][1].x) + (r[s][2].x + r[s][3].x); bs.y += (r[s][0].y + r[s][1].y) + (r[s][2].y + r[s][3].y);
        bs.z += (r[s][0].z + r[s][1].z) + (r[s][2].z + r[s][3].z); bs.w += (r[s][0].w + r[s][1].w) + (r[s][2].w + r[s][3].w);
      }
      char* const d0 = dst0 + buf * BUFB + ((wave >> 1) + 4 * s) * kWsImage;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        unsigned h[4], m[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float v = i == 0 ? r[s][j].x : (i == 1 ? r[s][j].y : (i == 2 ? r[s][j].z : r[s][j].w));
          sp_cut(v, h[j], m[j], l[j]);
        }
        sp_store_quad<3>(d0 + (((4 * (cq & 3) + i) ^ slot) << 4), kWsPlane, h, m, l);
      }
    }
  };

  // ---- MFMA roles ----
  const int gt0 = 2 * (wave & 1);        // first co tile
  const int xt0 = wave >> 1;             // the ci tile
  const int goff = KS * kWsImage + gt0 * 1024 + lq * 256 + ((lr ^ lq) << 4);
  const int xoff = xt0 * 1024 + lq * 256 + ((lr ^ lq) << 4);

  spf4 a1[KS][2], a2[KS][2];
#pragma unroll
  for (int t = 0; t < KS; ++t)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) { a1[t][mt] = spf4{0.f, 0.f, 0.f, 0.f}; a2[t][mt] = spf4{0.f, 0.f, 0.f, 0.f}; }

  auto mma_step = [&](int buf) {
    const char* const base = lds + buf * BUFB;
    spu4 ga[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int q = 0; q < 3; ++q) ga[mt][q] = *reinterpret_cast<const spu4*>(base + goff + mt * 1024 + q * kWsPlane);
#pragma unroll
    for (int kw = 0; kw < KS; ++kw) {
      spu4 xb[3];
#pragma unroll
      for (int q = 0; q < 3; ++q) xb[q] = *reinterpret_cast<const spu4*>(base + xoff + kw * kWsImage + q * kWsPlane);
      // synth.SPLIT_PRODUCTS order (g plane, x plane): (2, 0), (0, 2), (1, 1), (1, 0), (0, 1) -> A2; (0, 0) -> A1
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) sp_mfma(a2[kw][mt], ga[mt][2], xb[0]);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) sp_mfma(a2[kw][mt], ga[mt][0], xb[2]);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) sp_mfma(a2[kw][mt], ga[mt][1], xb[1]);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) sp_mfma(a2[kw][mt], ga[mt][1], xb[0]);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) sp_mfma(a2[kw][mt], ga[mt][0], xb[1]);
#pragma unroll
      for (int mt = 0; mt < 2; ++mt) sp_mfma(a1[kw][mt], ga[mt][0], xb[0]);
    }
  };

  load_step();
  // One buffer: a barrier in front of the MFMAs and one behind them.  Two buffers: step t + 1 is written into the other buffer, and a wave
  // writes buffer t & 1 again only behind the barrier of step t + 1, which every wave reaches with its MFMAs of step t done: one barrier
  // per step, and a wave's store_step runs beside the MFMAs of the SIMD's other wave.
  for (int t = 0; t < nsteps; ++t) {
    const int buf = NBUF == 2 ? (t & 1) : 0;
    store_step(buf);
    __syncthreads();
    load_step();                 // (the step behind the last one lies from img_e * PP on: zeros, never stored)
    mma_step(buf);
    if (NBUF == 1) __syncthreads();
  }

  // ---- epilogue: (a1 + a2)[kw][mt][i] = co tile gt0 + mt, row 4 lq + i; ci tile xt0, column lr -> slab [chunk][Co][Ci][KS KS], row kh ----
  float* slab = p.slab + (size_t)chunk * p.Co * p.Ci * (KS * KS);
  const int ci = ci0 + xt0 * 16 + lr;
  if (ci < p.Ci) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = co0 + (gt0 + mt) * 16 + 4 * lq + i;
        float* dst = slab + ((size_t)co * p.Ci + ci) * (KS * KS) + kh * KS;
#pragma unroll
        for (int t = 0; t < KS; ++t) dst[t] = a1[t][mt][i] + a2[t][mt][i];
      }
  }
  // ---- bias partials (kernel row 0 of the first ci tile only; behind a barrier): the eight position quads of a channel in quad order ----
  if (p.want_db && ntile == 0 && kh == 0) {
    if (NBUF == 2) __syncthreads();                    // (the K loop of the two-buffer form does not end with a barrier)
    sp_db_quads(reinterpret_cast<float*>(lds), is_g[0] || (on[1] && is_g[1]), pq, cq, bs, tid, p.dbslab, (size_t)chunk * p.Co + co0);
  }
}

}  // namespace

// The plan of the stride-2 split weight gradient: a function of these seven integers only.  tiles = (Co / 64) ceil(Ci / 64) k blocks per
// chunk at one block per CU; as many chunks as fit one round of the 256 CUs (7x7) or two (5x5: 170 tiles would leave a third of the CUs
// idle in one), but a chunk no shorter than kWsMinPositions output pixels; whole images per chunk, ceil(n_img / chunks) each, no empty chunk
// (conv_wgrad_chunks, conv_bwd.hip)
bool conv_s2_wgrad_split_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_floats, int* chunks_out) {
  if (!conv_s2_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return false;
  const int KK = KH * KW;
  const long long PP = (long long)(H / 2) * (W / 2);
  const long long tiles = (long long)(Co / 64) * ((Ci + 63) / 64) * KH;
  const int chunks = conv_wgrad_chunks(n_img, PP, tiles, KH == 5 ? kWsSlots5 : kWsSlots7, kWsMinPositions);
  if (weight_floats) *weight_floats = (size_t)chunks * ((size_t)Co * Ci * KK + Co);
  if (chunks_out) *chunks_out = chunks;
  return true;
}

hipError_t conv_s2_wgrad_split_launch(const float* x, int x_cs, int x_coff, const float* g, int g_cs, int g_coff, int n_img, int H, int W,
                                      int Ci, int Co, int KS, int relu_in, float* dw, float* db, int accumulate, float* scratch,
                                      int chunks, hipStream_t st) {
  WsArgs a;
  a.x = x; a.x_cs = x_cs; a.x_coff = x_coff; a.g = g; a.g_cs = g_cs; a.g_coff = g_coff;
  a.n_img = n_img; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.relu_in = relu_in; a.want_db = db != nullptr;
  a.ipc = (n_img + chunks - 1) / chunks;
  a.slab = scratch; a.dbslab = scratch + (size_t)chunks * Co * Ci * KS * KS;
  const int lds = (KS == 5 ? 2 : 1) * (KS + 1) * kWsImage;
  const dim3 grid((Co / 64) * ((Ci + 63) / 64) * KS, chunks);
  if (KS == 7) {
    hipError_t e = lds_attr_once(reinterpret_cast<const void*>(conv_s2_wgrad_split_kernel<7>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(conv_s2_wgrad_split_kernel<7>, grid, dim3(512), lds, st, a);
  } else {
    hipError_t e = lds_attr_once(reinterpret_cast<const void*>(conv_s2_wgrad_split_kernel<5>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(conv_s2_wgrad_split_kernel<5>, grid, dim3(512), lds, st, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return conv_wgrad_reduce_launch(a.slab, a.dbslab, Co, Ci, KS * KS, chunks, dw, db, accumulate, st);
}

}  // namespace offk
