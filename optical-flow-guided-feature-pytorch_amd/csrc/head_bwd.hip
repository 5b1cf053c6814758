// K5t / K5b. Training side of the three classifier heads (reference RGB_OFF.py:782-793, 843-847 with the
// nn.Dropout(p = 0.8) of :785 / :791 / :845 in training mode, train_off.py:39-45, 126-146):
//   pooled[n][c] = mean over the map (maxpool = 0) or over the MaxPool2d(3, 2, ceil_mode) windows (maxpool = 1)        -- K5's definition
//   z[n][c]      = pooled * keep * scale,   out = z . fc_w^T + fc_b
//   dz = g . fc_w,  dpooled = dz * keep * scale,  v = dpooled * (1.f / nwin)
//   dx[n, y, x, c] (+)= v[n][c]                                          (maxpool = 0: every pixel)
//   dx[n, y, x, c] (+)= sum of v[n][c] over the windows whose FIRST maximum (row-major window order) is (y, x)      (maxpool = 1)
//   dw[o][c] (+)= sum_n g[n][o] z[n][c],  db[o] (+)= sum_n g[n][o]
// keep is the library's reproducible dropout (offk_common.h drop_mul) on stream (seed, 16 + head_index): draw n * (C / 4) + c / 4 serves
// a channel quad, 16 bits each, kept iff the field >= round(p * 65536) -- offk_amd/synth.py head_dropout_keep is the same integer function.
//
// All of it is memory-bound (at 384 images the three dx are 77 / 38.5 / 77 MB, the GEMMs <= 79 MFLOP), so every map access is a 16-byte
// load or store along the channels, a block owns 128 channels of one image (32 lanes = 512 contiguous bytes per pixel) and its 256 threads
// are 32 channel quads x 8 groups that split the pixels / windows / classes; group partials meet in LDS and are added in group order.
//   head_pool_drop_kernel  grid (image, C / 128): pooling partials -> LDS -> mean, dropout -> z.  The FC behind it is heads.hip's
//                          fc_launch on z (unchanged).
//   head_dx_kernel         grid (image, C / 128, pixel splits): dz of the block's 128 channels from g and fc_w (51 KB of fc_w out of L2
//                          per block) stays in LDS, never in HBM; then every thread stores its pixels.  The max-pool form is a GATHER: the
//                          thread that owns a dx element visits the (at most four) windows that contain it, recomputes each window's
//                          first maximum from x and adds v where that is its own pixel.  No atomics; every element of the slice is stored.
//   head_wgrad_kernel      grid (classes / 16, C / 256, chunk): a wave = 4 classes x 256 channels over the chunk's images, g through
//                          the scalar unit; slabs [chunk][classes][C] + [chunk][classes]
//   head_wgrad_reduce_kernel  adds the slabs in chunk order (the library's split-K rule): the same bits whatever the scratch held.
// NaN in x on the max-pool path is outside the contract: K5's forward (fmaxf) drops a NaN where torch propagates it.
#include "offk_common.h"
#include "offk_internal.h"

namespace offk {

namespace {

constexpr int kSlabC = 128;       // channels of one block
constexpr int kQuads = kSlabC / 4;
constexpr int kGroups = 256 / kQuads;
constexpr int kWgImages = 16;     // weight gradient: a chunk is no shorter than this many images ...
constexpr int kWgMaxChunks = 24;  // ... and there are at most this many chunks

struct HeadDrop { unsigned long long base; unsigned thresh; float scale; };

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 max4(float4 a, float4 b) {
  return make_float4(fmaxf(a.x, b.x), fmaxf(a.y, b.y), fmaxf(a.z, b.z), fmaxf(a.w, b.w));
}
// the eight group partials of channel quad `quad` in group order
__device__ __forceinline__ float4 sum_groups(const float (*part)[kSlabC], int quad) {
  float4 t = ld4(&part[0][4 * quad]);
#pragma unroll
  for (int j = 1; j < kGroups; ++j) t = add4(t, ld4(&part[j][4 * quad]));
  return t;
}

// ---------------------------------------------------------------- train forward ----------------------------------------------------------------
__global__ __launch_bounds__(256) void head_pool_drop_kernel(const float* __restrict__ x, int cs, int coff, int H, int W, int C, int maxpool,
                                                             HeadDrop d, float* __restrict__ z) {
  __shared__ __attribute__((aligned(16))) float part[kGroups][kSlabC];
  const int img = blockIdx.x, c0 = blockIdx.y * kSlabC, tid = threadIdx.x;
  const int q = tid & (kQuads - 1), grp = tid >> 5;
  const float* xi = x + (size_t)img * H * W * cs + coff + c0 + 4 * q;
  const int Ho = maxpool ? (H - 2) / 2 + 1 : H, Wo = maxpool ? (W - 2) / 2 + 1 : W;
  const int nwin = Ho * Wo;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c0 + 4 * q < C) {
    if (maxpool) {
      for (int wdw = grp; wdw < nwin; wdw += kGroups) {
        const int oy = wdw / Wo, ox = wdw - oy * Wo;
        float4 v[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dx = 0; dx < 3; ++dx) {
            const int y = min(2 * oy + dy, H - 1), xx = min(2 * ox + dx, W - 1);      // a clipped tap repeats its neighbour: same max
            v[3 * dy + dx] = ld4(xi + (size_t)(y * W + xx) * cs);
          }
        float4 m = v[0];
#pragma unroll
        for (int t = 1; t < 9; ++t) m = max4(m, v[t]);
        s = add4(s, m);
      }
    } else {
#pragma unroll 4
      for (int px = grp; px < nwin; px += kGroups) s = add4(s, ld4(xi + (size_t)px * cs));
    }
  }
  *reinterpret_cast<float4*>(&part[grp][4 * q]) = s;
  __syncthreads();
  if (tid < kQuads && c0 + 4 * tid < C) {
    const float4 t = sum_groups(part, tid);
    const float inv = 1.f / (float)nwin;
    const float4 k = drop_mul(d.base, (unsigned long long)img * (unsigned)(C >> 2) + (unsigned)((c0 >> 2) + tid), d.thresh, d.scale);
    *reinterpret_cast<float4*>(z + (size_t)img * C + c0 + 4 * tid) =
        make_float4(t.x * inv * k.x, t.y * inv * k.y, t.z * inv * k.z, t.w * inv * k.w);
  }
}

// ---------------------------------------------------------------- data gradient ----------------------------------------------------------------
struct HeadDxArgs {
  const float* g;                  // [n_img][ncls]
  const float* x; int x_cs, x_coff;
  const float* fw;                 // [ncls][C]
  int H, W, C, ncls, maxpool;
  HeadDrop d;
  float* dx; int dx_cs, dx_coff, accumulate;
};

__global__ __launch_bounds__(256) void head_dx_kernel(HeadDxArgs p) {
  __shared__ __attribute__((aligned(16))) float part[kGroups][kSlabC];
  __shared__ __attribute__((aligned(16))) float vs[kSlabC];
  const int img = blockIdx.x, c0 = blockIdx.y * kSlabC, tid = threadIdx.x;
  const int q = tid & (kQuads - 1), grp = tid >> 5;
  const int H = p.H, W = p.W, C = p.C;
  const bool live = c0 + 4 * q < C;
  const int Ho = p.maxpool ? (H - 2) / 2 + 1 : H, Wo = p.maxpool ? (W - 2) / 2 + 1 : W;

  // dz of the block's channels: group j sums the classes j, j + 8, ... ; the groups meet in LDS
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  if (live) {
    const float* gi = p.g + (size_t)img * p.ncls;
    const float* wq = p.fw + c0 + 4 * q;
#pragma unroll 4
    for (int o = grp; o < p.ncls; o += kGroups) {
      const float gv = gi[o];
      const float4 w = ld4(wq + (size_t)o * C);
      a.x = fmaf(gv, w.x, a.x); a.y = fmaf(gv, w.y, a.y); a.z = fmaf(gv, w.z, a.z); a.w = fmaf(gv, w.w, a.w);
    }
  }
  *reinterpret_cast<float4*>(&part[grp][4 * q]) = a;
  __syncthreads();
  if (tid < kQuads && c0 + 4 * tid < C) {
    const float4 t = sum_groups(part, tid);
    const float inv = 1.f / (float)(Ho * Wo);
    const float4 k = drop_mul(p.d.base, (unsigned long long)img * (unsigned)(C >> 2) + (unsigned)((c0 >> 2) + tid), p.d.thresh, p.d.scale);
    *reinterpret_cast<float4*>(&vs[4 * tid]) = make_float4(t.x * k.x * inv, t.y * k.y * inv, t.z * k.z * inv, t.w * k.w * inv);
  }
  __syncthreads();
  if (!live) return;
  const float4 v = ld4(&vs[4 * q]);
  const int HW = H * W;
  float* di = p.dx + (size_t)img * HW * p.dx_cs + p.dx_coff + c0 + 4 * q;
  if (!p.maxpool) {
    for (int px = blockIdx.z * kGroups + grp; px < HW; px += kGroups * gridDim.z) {
      float4* dst = reinterpret_cast<float4*>(di + (size_t)px * p.dx_cs);
      float4 o = v;
      if (p.accumulate) o = add4(*dst, o);
      *dst = o;
    }
    return;
  }
  const float* xi = p.x + (size_t)img * HW * p.x_cs + p.x_coff + c0 + 4 * q;
  for (int px = blockIdx.z * kGroups + grp; px < HW; px += kGroups * gridDim.z) {
    const int y = px / W, xx = px - y * W;
    // the windows (oy, ox) with 2 o <= coordinate <= 2 o + 2: one or two per axis
    const int oy_lo = (y - 1) / 2 < 0 ? 0 : (y - 1) / 2, oy_hi = min(y >> 1, Ho - 1);
    const int ox_lo = (xx - 1) / 2 < 0 ? 0 : (xx - 1) / 2, ox_hi = min(xx >> 1, Wo - 1);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = oy_lo; oy <= oy_hi; ++oy)
      for (int ox = ox_lo; ox <= ox_hi; ++ox) {
        // the window's first maximum per channel: taps in row-major order, replaced only by a strictly greater one.  A tap outside the
        // map is clamped onto its neighbour inside, which came EARLIER in that order (tap 1 of an axis always exists), so it never wins.
        float4 t[9];
        int pos[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
          for (int dxx = 0; dxx < 3; ++dxx) {
            pos[3 * dy + dxx] = min(2 * oy + dy, H - 1) * W + min(2 * ox + dxx, W - 1);
            t[3 * dy + dxx] = ld4(xi + (size_t)pos[3 * dy + dxx] * p.x_cs);
          }
        float4 best = t[0];
        int bx = pos[0], by = pos[0], bz = pos[0], bw = pos[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) {
          if (t[k].x > best.x) { best.x = t[k].x; bx = pos[k]; }
          if (t[k].y > best.y) { best.y = t[k].y; by = pos[k]; }
          if (t[k].z > best.z) { best.z = t[k].z; bz = pos[k]; }
          if (t[k].w > best.w) { best.w = t[k].w; bw = pos[k]; }
        }
        acc.x += bx == px ? v.x : 0.f; acc.y += by == px ? v.y : 0.f;
        acc.z += bz == px ? v.z : 0.f; acc.w += bw == px ? v.w : 0.f;
      }
    float4* dst = reinterpret_cast<float4*>(di + (size_t)px * p.dx_cs);
    if (p.accumulate) acc = add4(*dst, acc);
    *dst = acc;
  }
}

// ---------------------------------------------------------------- weight gradient ----------------------------------------------------------------
struct HeadWgArgs {
  const float* g;                  // [n_img][ncls]
  const float* z;                  // [n_img][C]
  int n_img, C, ncls, ipc;         // images per chunk = ceil(n_img / chunks)
  int want_dw, want_db;
  float* slab;                     // [chunks][ncls][C]
  float* dbslab;                   // [chunks][ncls]
};

__global__ __launch_bounds__(256) void head_wgrad_kernel(HeadWgArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int o0 = blockIdx.x * 16 + wave * 4, c = blockIdx.y * 256 + 4 * lane, chunk = blockIdx.z;
  if (o0 >= p.ncls) return;
  const int n0 = chunk * p.ipc, n1 = min(p.n_img, n0 + p.ipc);
  const bool live = p.want_dw && c < p.C;
  int oc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) oc[j] = min(o0 + j, p.ncls - 1);
  float4 acc[4];
  float s[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { acc[j] = make_float4(0.f, 0.f, 0.f, 0.f); s[j] = 0.f; }
#pragma unroll 4
  for (int n = n0; n < n1; ++n) {
    const float* gn = p.g + (size_t)n * p.ncls;
    const float4 zv = live ? ld4(p.z + (size_t)n * p.C + c) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float gv = gn[oc[j]];
      s[j] += gv;
      acc[j].x = fmaf(gv, zv.x, acc[j].x); acc[j].y = fmaf(gv, zv.y, acc[j].y);
      acc[j].z = fmaf(gv, zv.z, acc[j].z); acc[j].w = fmaf(gv, zv.w, acc[j].w);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (o0 + j >= p.ncls) continue;
    if (live) *reinterpret_cast<float4*>(p.slab + ((size_t)chunk * p.ncls + o0 + j) * p.C + c) = acc[j];
    if (p.want_db && blockIdx.y == 0 && lane == 0) p.dbslab[(size_t)chunk * p.ncls + o0 + j] = s[j];
  }
}

// dw[i] (+)= slab[0][i] + slab[1][i] + ... in chunk order; the same for db behind it (either may be absent)
__global__ __launch_bounds__(256) void head_wgrad_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ dbslab, size_t nw, int ncls,
                                                                int chunks, float* dw, float* db, int accumulate) {
  const size_t nwe = dw ? nw : 0, n = nwe + (db ? (size_t)ncls : 0);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const bool is_w = i < nwe;
    const float* src = is_w ? slab + i : dbslab + (i - nwe);
    const size_t step = is_w ? nw : (size_t)ncls;
    float v = src[0];
    for (int z = 1; z < chunks; ++z) v += src[(size_t)z * step];
    float* dst = is_w ? dw + i : db + (i - nwe);
    *dst = accumulate ? *dst + v : v;
  }
}

HeadDrop make_head_drop(int head_index, unsigned long long seed, double p) {
  HeadDrop d;
  d.base = drop_stream_base(seed, 16 + head_index);
  d.thresh = (unsigned)llround(p * 65536.0);
  d.scale = (float)(1.0 / (1.0 - p));
  return d;
}

}  // namespace

// The plan of one head's weight gradient: a function of these three integers only.  Whole images per chunk, ceil(n_img / chunks) each,
// a chunk no shorter than kWgImages images, at most kWgMaxChunks chunks, no empty chunk (conv_bwd_plan's settling rule).
bool head_bwd_plan(int n_img, int C, int ncls, size_t* scratch_floats, int* chunks_out) {
  if (n_img < 1 || C < 4 || C > 1024 || (C & 3) || ncls < 1) return false;
  int chunks = (n_img + kWgImages - 1) / kWgImages;
  if (chunks > kWgMaxChunks) chunks = kWgMaxChunks;
  for (;;) {
    const int ipc = (n_img + chunks - 1) / chunks;
    const int c2 = (n_img + ipc - 1) / ipc;
    if (c2 == chunks) break;
    chunks = c2;
  }
  if (scratch_floats) *scratch_floats = (size_t)chunks * ((size_t)ncls * C + ncls);
  if (chunks_out) *chunks_out = chunks;
  return true;
}

hipError_t head_train_launch(const float* x, int x_cs, int x_coff, int n_img, int H, int W, int C, int maxpool, const float* fw, const float* fb,
                             int ncls, int head_index, unsigned long long seed, double drop_p, float* z, float* out, hipStream_t st) {
  hipLaunchKernelGGL(head_pool_drop_kernel, dim3(n_img, (C + kSlabC - 1) / kSlabC), dim3(256), 0, st, x, x_cs, x_coff, H, W, C, maxpool,
                     make_head_drop(head_index, seed, drop_p), z);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return fc_launch(z, n_img, C, fw, fb, ncls, out, st);
}

hipError_t head_bwd_data_launch(const float* g, const float* x, int x_cs, int x_coff, int n_img, int H, int W, int C, int maxpool, const float* fw,
                                int ncls, int head_index, unsigned long long seed, double drop_p, float* dx, int dx_cs, int dx_coff,
                                int accumulate, hipStream_t st) {
  HeadDxArgs a;
  a.g = g; a.x = x; a.x_cs = x_cs; a.x_coff = x_coff; a.fw = fw; a.H = H; a.W = W; a.C = C; a.ncls = ncls; a.maxpool = maxpool;
  a.d = make_head_drop(head_index, seed, drop_p);
  a.dx = dx; a.dx_cs = dx_cs; a.dx_coff = dx_coff; a.accumulate = accumulate;
  // enough blocks to fill the chip at small n_img: the pixels of an image are dealt to up to `split` blocks (each recomputes dz)
  const int slabs = (C + kSlabC - 1) / kSlabC;
  const long long base = (long long)n_img * slabs;
  long long split = (2048 + base - 1) / base;
  const long long max_split = ((long long)H * W + kGroups - 1) / kGroups;
  if (split > max_split) split = max_split;
  if (split > 64) split = 64;
  if (split < 1) split = 1;
  hipLaunchKernelGGL(head_dx_kernel, dim3(n_img, slabs, (unsigned)split), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t head_bwd_weight_launch(const float* g, const float* z, int n_img, int C, int ncls, float* dw, float* db, int accumulate, float* scratch,
                                  int chunks, hipStream_t st) {
  HeadWgArgs a;
  a.g = g; a.z = z; a.n_img = n_img; a.C = C; a.ncls = ncls; a.ipc = (n_img + chunks - 1) / chunks;
  a.want_dw = dw != nullptr; a.want_db = db != nullptr;
  a.slab = scratch; a.dbslab = scratch + (size_t)chunks * ncls * C;
  // without dw one channel slab is enough: its lane 0 carries the bias sums
  hipLaunchKernelGGL(head_wgrad_kernel, dim3((ncls + 15) / 16, dw ? (C + 255) / 256 : 1, chunks), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t nw = (size_t)ncls * C, n = (dw ? nw : 0) + (db ? ncls : 0);
  const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(head_wgrad_reduce_kernel, dim3(blocks), dim3(256), 0, st, a.slab, a.dbslab, nw, ncls, chunks, dw, db, accumulate);
  return hipGetLastError();
}

}  // namespace offk
