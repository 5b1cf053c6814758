// K4b's weight / bias gradient in split-fp32 arithmetic on the bf16 matrix pipe (offk_conv2d_backward_weight_split):
//   dw[co][ci][kh][kw] = sum_q g_pad[q][co] * x_pad[q + (kh - pad) * pitch + (kw - pad)][ci],   db[co] = sum_q g_pad[q][co]
// for one stride-1 fusion conv, k = 1 or 3.  Both operands are cut into THREE bf16 planes by truncation (sp_cut of split_common.h =
// synth.cut3) and per 32-position step six of the nine plane products are issued on v_mfma_f32_16x16x32_bf16 in
// synth.SPLIT_PRODUCTS order with g in the role of w: g_l x_h, g_h x_l, g_m x_m, g_m x_h, g_h x_m into accumulator A2, g_h x_h into A1; steps
// in increasing position order, the block's partial tile is A1 + A2, added once: synth.emulate_split_dot(form="units") over the block's chunk.
// The slabs [chunk][Co][Ci k k] (+ [chunk][Co]) are summed in chunk order by the unchanged conv_wgrad_reduce_kernel (conv_bwd.hip).
//
// K order (include/offk.h states it for callers; tests/conv_wgrad_split.py follows it on the CPU).  K runs over POSITIONS q:
//   k = 1: the pixels themselves, q = (img * H + h) * W + w, images back to back (PP = H W positions per image).
//   k = 3: a row of an image is `pitch` = 8 ceil((W + 1) / 8) positions: its W pixels, then pitch - W >= 1 zero columns; an image is its H
//          rows and ONE zero row, PP = (H + 1) pitch positions, q = img * PP + h * pitch + w.  The zero columns behind a row are the left
//          neighbours of the next row's first pixel, the zero row below an image is the row above the next image; positions below 0 and
//          from n_img * PP on are zeros.  Tap (kh, kw) pairs g at q with x at q + (kh - 1) pitch + (kw - 1).
//   A chunk holds the positions [img_b * PP, img_e * PP) of its ceil(n_img / chunks) whole images; its step t holds the 32 positions from
//   img_b * PP + 32 t on, g zero from img_e * PP on (the last step of a chunk may be partly empty).
// Eight consecutive k of one channel are one lane's 16-byte MFMA operand, so a tap's shift has to be a multiple of 8 positions to stay an
// aligned ds_read_b128: (kh - 1) pitch is one, and the (kw - 1) is staged: the x planes are written THREE times, image kw holding
// X_kw[q] = x_pad[q + kw - 1].  A thread loads six consecutive positions (q - 1 .. q + 4, q a multiple of 4) of four channels, cuts each value
// once and stores the three shifted quads.  Per step the block stages the g rows (64 co x 32 k x 3 planes, 12 KB) and NG = 4 + 2 pg k groups
// of x (pg = min(pitch / 8, 4): the three kernel rows' windows of four k groups start pg groups apart and overlap where pitch < 32 -- 6 groups
// on 7x7 maps, 8 on 14x14, 12 from pitch 32 on, where the windows are disjoint), 9216 B per group.  Plane images are [16-row tile][k group]
// [16 rows] x 16 B with row r of a (tile, k group) piece at r ^ (k group & 3): pw_wgrad_split_kernel's channels-last loader, thread for
// thread (a thread stores the four rows of one position quad; sixteen lanes of a ds_write_b64 hit sixteen different 8-byte slots).
// Geometry: one block = one 64 (co) x 64 (ci) tile of dw for all k k taps over one chunk.  k = 3: eight waves, wave w owns co tiles
// 2 (w & 1) .. + 1 x ci tile (w >> 1) x nine taps x (A1, A2) = 144 accumulator registers, one block per CU (two waves per SIMD, 256 registers
// each; build.py's register guard); threads 0 .. 383 load x, 384 .. 511 g.  k = 1: four waves of 32 x 32, threads 0 .. 127 x, 128 .. 255 g.
// The next step's rows are loaded into registers before the MFMAs of the current one (unconditionally, the step index clamped) and cut
// into LDS behind them.  db is the fp32 sum of the g rows as loaded, per thread over its position quads in step order, then over the
// eight quads of a step in a fixed order: nothing is split.
#include "offk_common.h"
#include "offk_internal.h"
#include "split_common.h"

namespace offk {
namespace {

constexpr int kCsKT = 32;               // positions per step
constexpr int kCsSlots3 = 256;          // 3x3: one block per CU
constexpr int kCsSlots1 = 1024;         // 1x1: four blocks per CU (24 KB of LDS, four waves)
constexpr int kCsMinPositions = 256;    // a chunk is at least eight steps long (unless the whole problem is shorter)
constexpr int kCsGPlane = 4096;         // one plane of the g rows: 4 tiles x 4 k groups x 256 B
constexpr int kCsXBase = 3 * kCsGPlane;

struct CsArgs {
  const float* x; int x_cs;       // channel offset and the block's first channel are added by the kernel
  const float* g; int g_cs;
  int x_coff, g_coff;
  int n_img, H, W, Ci, Co;
  int relu_in, want_db;
  int ipc;                        // images per chunk = ceil(n_img / chunks)
  int pitch, PP;                  // positions per row (k = 3) and per image
  int pg, NG;                     // k groups between two kernel rows' windows; k groups staged per x image (k = 1: 4)
  float* slab;                    // [chunks][Co][Ci * KK]
  float* dbslab;                  // [chunks][Co]
};

// pixel row of position q, or -1 where the position is a zero (pad column, zero row, outside [0, q_lim))
template <int KS>
__device__ __forceinline__ long long cs_pixel(int q, int q_lim, int H, int W, int pitch, int PP) {
  if (q < 0 || q >= q_lim) return -1;
  if constexpr (KS == 1) {
    return q;
  } else {
    const unsigned img = (unsigned)q / (unsigned)PP, rem = (unsigned)q - img * (unsigned)PP;
    const unsigned h = rem / (unsigned)pitch, w = rem - h * (unsigned)pitch;
    if ((int)h >= H || (int)w >= W) return -1;
    return ((long long)img * H + h) * W + w;
  }
}

template <int KS>
__global__ __launch_bounds__(KS == 3 ? 512 : 256) void conv_wgrad_split_kernel(CsArgs p) {
  constexpr int KK = KS * KS;
  constexpr int XTH = KS == 3 ? 384 : 128;    // threads 0 .. XTH - 1 load x, the 128 behind them g
  constexpr int NL = KS == 3 ? 6 : 4;         // 16-byte loads per thread and step
  constexpr int J0 = KS == 3 ? 1 : 0;         // the load that holds the quad's first position
  constexpr int NTW = KS == 3 ? 1 : 2;        // ci tiles of a wave (co tiles: always two)
  extern __shared__ __attribute__((aligned(16))) char lds[];   // g planes [3][4 tiles][4 k groups][256 B], then x [KS images][3 planes][4 tiles][NG][256 B]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lq = lane >> 4;
  const int NT = p.Ci >> 6;
  const int mtile = blockIdx.x / NT, ntile = blockIdx.x - mtile * NT;
  const int co0 = mtile * 64, ci0 = ntile * 64;
  const int chunk = blockIdx.y;
  const int H = p.H, W = p.W, pitch = p.pitch, PP = p.PP, NG = p.NG;
  const int img_b = chunk * p.ipc, img_e = min(p.n_img, img_b + p.ipc);
  const int qb = img_b * PP, qe = img_e * PP, q_all = p.n_img * PP;
  const int nsteps = (qe - qb + kCsKT - 1) / kCsKT;
  const int xplane = 4 * NG * 256, ximg = 3 * xplane;

  // ---- loader roles ----
  const bool is_g = tid >= XTH;
  const int item = is_g ? tid - XTH : tid;
  const int pq = item & 7, cq = (item >> 3) & 15;       // position quad inside four k groups, channel quad
  const int slot = 4 * (item >> 7) + (pq >> 1), half = pq & 1;   // x: the k group of the image the quad goes to
  const bool on = is_g || slot < NG;
  int rel;                                               // the quad's first position, relative to the step's
  if (is_g || KS == 1) {
    rel = 8 * slot + 4 * half;
  } else {
    const int kh = min(slot / p.pg, 2);
    rel = (kh - 1) * pitch + 8 * (slot - kh * p.pg) + 4 * half;
  }
  const float* const src = is_g ? p.g + p.g_coff + co0 + 4 * cq : p.x + p.x_coff + ci0 + 4 * cq;
  const int src_cs = is_g ? p.g_cs : p.x_cs;
  const int q_lim = is_g ? qe : q_all;
  const bool relu = !is_g && p.relu_in;

  float4 r[NL];
  // (unconditional loads: a position that is a zero reads the view's first row and is replaced behind the load)
  auto load_step = [&](int q0) {
    const int qq = q0 + rel;
    long long pix[NL];
    if constexpr (KS == 3) {
      // the quad lies inside one row (pitch % 8 == 0, qq % 4 == 0 relative to the image); its two neighbours may not
      const long long pm = (on && !is_g) ? cs_pixel<3>(qq - 1, q_lim, H, W, pitch, PP) : -1;
      const long long pn = (on && !is_g) ? cs_pixel<3>(qq + 4, q_lim, H, W, pitch, PP) : -1;
      long long row = -1;
      int w0 = 0;
      if (on && qq >= 0 && qq < q_lim) {
        const unsigned img = (unsigned)qq / (unsigned)PP, rem = (unsigned)qq - img * (unsigned)PP;
        const unsigned h = rem / (unsigned)pitch;
        w0 = (int)(rem - h * (unsigned)pitch);
        if ((int)h < H) row = ((long long)img * H + h) * W;
      }
      // The g role has no neighbours (pm = pn = -1): its loads 0 and 5 read the view's first row, one cached line for the whole block, and
      // their cuts in store_step are dead code.  Left so on purpose: the two roles share one unconditional load sequence (DESIGN.md section
      // 10), and the g threads are a quarter of the loaders, so the two spare loads are one twelfth of the block's, none of them from HBM.
      pix[0] = pm; pix[5] = pn;
#pragma unroll
      for (int j = 0; j < 4; ++j) pix[1 + j] = (row >= 0 && w0 + j < W && qq + j < q_lim) ? row + w0 + j : -1;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) pix[j] = on ? cs_pixel<1>(qq + j, q_lim, H, W, pitch, PP) : -1;
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const float* ptr = src + (pix[j] >= 0 ? pix[j] : 0) * src_cs;
      float4 v = *reinterpret_cast<const float4*>(ptr);
      if (pix[j] < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
      r[j] = v;
    }
  };

  float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
  // where this thread's 8 bytes of (row 4 (cq & 3) + i, its k group, its half) lie inside a plane: + i * 16 before the swizzle
  const int swz = slot & 3;
  char* const gdst = lds + (cq >> 2) * 1024 + slot * 256 + half * 8;                    // g role: slot = pq >> 1 < 4
  char* const xdst = lds + kCsXBase + (cq >> 2) * (NG * 256) + slot * 256 + half * 8;
  auto store_step = [&]() {
    if (is_g) {
      bs.x += (r[J0].x + r[J0 + 1].x) + (r[J0 + 2].x + r[J0 + 3].x); bs.y += (r[J0].y + r[J0 + 1].y) + (r[J0 + 2].y + r[J0 + 3].y);
      bs.z += (r[J0].z + r[J0 + 1].z) + (r[J0 + 2].z + r[J0 + 3].z); bs.w += (r[J0].w + r[J0 + 1].w) + (r[J0 + 2].w + r[J0 + 3].w);
    } else if (!on) {
      return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      unsigned h[NL], m[NL], l[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const float v = i == 0 ? r[j].x : (i == 1 ? r[j].y : (i == 2 ? r[j].z : r[j].w));
        sp_cut(v, h[j], m[j], l[j]);
      }
      const int rowoff = (((4 * (cq & 3) + i) ^ swz) << 4);
      if (is_g) {
        sp_store_quad<3>(gdst + rowoff, kCsGPlane, h + J0, m + J0, l + J0);
      } else {
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {      // image kw holds x_pad[q + kw - pad]: loads kw .. kw + 3
          sp_store_quad<3>(xdst + kw * ximg + rowoff, xplane, h + kw, m + kw, l + kw);
        }
      }
    }
  };

  // ---- MFMA roles ----
  const int gt0 = KS == 3 ? 2 * (wave & 1) : 2 * (wave >> 1);     // first co tile
  const int xt0 = KS == 3 ? (wave >> 1) : 2 * (wave & 1);         // first ci tile
  const int goff = gt0 * 1024 + lq * 256 + ((lr ^ lq) << 4);
  int xoff[KS];                                                    // per kernel row: the window's k group lq of ci tile xt0, plane 0, image 0
#pragma unroll
  for (int kh = 0; kh < KS; ++kh) {
    const int s = (KS == 3 ? kh * p.pg : 0) + lq;
    xoff[kh] = kCsXBase + xt0 * (NG * 256) + s * 256 + ((lr ^ (s & 3)) << 4);
  }

  spf4 a1[KK][2][NTW], a2[KK][2][NTW];
#pragma unroll
  for (int t = 0; t < KK; ++t)
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < NTW; ++nt) { a1[t][mt][nt] = spf4{0.f, 0.f, 0.f, 0.f}; a2[t][mt][nt] = spf4{0.f, 0.f, 0.f, 0.f}; }

  auto mma_step = [&]() {
    spu4 ga[2][3];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int q = 0; q < 3; ++q) ga[mt][q] = *reinterpret_cast<const spu4*>(lds + goff + mt * 1024 + q * kCsGPlane);
#pragma unroll
    for (int kh = 0; kh < KS; ++kh)
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
        const int tap = kh * KS + kw;
        spu4 xb[NTW][3];
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt)
#pragma unroll
          for (int q = 0; q < 3; ++q) xb[nt][q] = *reinterpret_cast<const spu4*>(lds + xoff[kh] + kw * ximg + q * xplane + nt * (NG * 256));
        sp_issue6<2, NTW>(a1[tap], a2[tap], ga, xb);      // g in the role of w
      }
  };

  load_step(qb);
  for (int t = 0; t < nsteps; ++t) {
    store_step();
    __syncthreads();
    load_step(qb + min(t + 1, nsteps - 1) * kCsKT);      // (the last step loads itself again: never stored)
    mma_step();
    __syncthreads();
  }

  // ---- epilogue: (a1 + a2)[tap][mt][nt][i] = co tile gt0 + mt, row 4 lq + i; ci tile xt0 + nt, column lr -> slab [chunk][Co][Ci][KK] ----
  float* slab = p.slab + (size_t)chunk * p.Co * p.Ci * KK;
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
      const int ci = ci0 + (xt0 + nt) * 16 + lr;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int co = co0 + (gt0 + mt) * 16 + 4 * lq + i;
        float* dst = slab + ((size_t)co * p.Ci + ci) * KK;
#pragma unroll
        for (int t = 0; t < KK; ++t) dst[t] = a1[t][mt][nt][i] + a2[t][mt][nt][i];
      }
    }
  // ---- bias partials (first ci tile only; the K loop ended with a barrier): the eight position quads of a channel in quad order ----
  if (p.want_db && ntile == 0) {
    sp_db_quads(reinterpret_cast<float*>(lds), is_g, pq, cq, bs, tid, p.dbslab, (size_t)chunk * p.Co + co0);
  }
}

int cs_pitch(int W, int KS) { return KS == 1 ? W : 8 * ((W + 1 + 7) / 8); }

bool conv_wgrad_split_supported(int n_img, int H, int W, int Ci, int Co, int KH, int KW) {
  if (!conv_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return false;
  const long long pitch = KH == 1 ? W : 8 * (((long long)W + 8) / 8);
  const long long PP = KH == 1 ? (long long)H * W : ((long long)H + 1) * pitch;
  return PP * n_img + 2 * pitch + 4096 < 0x7fffffffLL;       // every position a block computes (a window reaches pitch + 40 past the end) is an int
}

}  // namespace

// The plan of the split weight gradient: a function of these seven integers only.  tiles = (Co / 64)(Ci / 64) blocks per chunk; as many
// chunks as fit the resident slots in one round (k = 3: one block per CU; k = 1: four), but a chunk no shorter than kCsMinPositions
// positions; whole images per chunk, ceil(n_img / chunks) each, no empty chunk (conv_wgrad_chunks, conv_bwd.hip)
bool conv_wgrad_split_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_floats, int* chunks_out) {
  if (!conv_wgrad_split_supported(n_img, H, W, Ci, Co, KH, KW)) return false;
  const int KK = KH * KW;
  const long long PP = KH == 1 ? (long long)H * W : ((long long)H + 1) * cs_pitch(W, KH);
  const long long tiles = (long long)(Co / 64) * (Ci / 64);
  const int chunks = conv_wgrad_chunks(n_img, PP, tiles, KH == 1 ? kCsSlots1 : kCsSlots3, kCsMinPositions);
  if (weight_floats) *weight_floats = (size_t)chunks * ((size_t)Co * Ci * KK + Co);
  if (chunks_out) *chunks_out = chunks;
  return true;
}

hipError_t conv_wgrad_split_launch(const float* x, int x_cs, int x_coff, const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Ci,
                                   int Co, int KS, int relu_in, float* dw, float* db, int accumulate, float* scratch, int chunks,
                                   hipStream_t st) {
  CsArgs a;
  a.x = x; a.x_cs = x_cs; a.x_coff = x_coff; a.g = g; a.g_cs = g_cs; a.g_coff = g_coff;
  a.n_img = n_img; a.H = H; a.W = W; a.Ci = Ci; a.Co = Co; a.relu_in = relu_in; a.want_db = db != nullptr;
  a.ipc = (n_img + chunks - 1) / chunks;
  a.pitch = cs_pitch(W, KS);
  a.PP = KS == 1 ? H * W : (H + 1) * a.pitch;
  a.pg = KS == 1 ? 0 : (a.pitch / 8 < 4 ? a.pitch / 8 : 4);
  a.NG = KS == 1 ? 4 : 4 + 2 * a.pg;
  a.slab = scratch; a.dbslab = scratch + (size_t)chunks * Co * Ci * KS * KS;
  const int lds = kCsXBase + KS * 3 * 4 * a.NG * 256;
  const dim3 grid((Co / 64) * (Ci / 64), chunks);
  if (KS == 1) {
    hipError_t e = lds_attr_once(reinterpret_cast<const void*>(conv_wgrad_split_kernel<1>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(conv_wgrad_split_kernel<1>, grid, dim3(256), lds, st, a);
  } else {
    hipError_t e = lds_attr_once(reinterpret_cast<const void*>(conv_wgrad_split_kernel<3>), kCsXBase + 9 * 4 * 12 * 256);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(conv_wgrad_split_kernel<3>, grid, dim3(512), lds, st, a);
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return conv_wgrad_reduce_launch(a.slab, a.dbslab, Co, Ci, KS * KS, chunks, dw, db, accumulate, st);
}

}  // namespace offk
