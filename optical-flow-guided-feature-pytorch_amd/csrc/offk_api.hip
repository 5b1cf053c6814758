// liboffk C ABI: handle, weight registry/packing, workspace plan, forward orchestration.
// See include/offk.h for the contract and the reference lines each entry point stands for.
#include "../../include/offk.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "offk_internal.h"

using namespace offk;

typedef const void* const* MapPtrs;      // nine maps of any element type, as the _typed / _cl entries take them

// A path switch of the library (the list: offk_create): unset or anything else = on, "0" = off, an integer n > 1 = on from n frame
// pairs (*min_p = n; left alone otherwise).
static bool path_switch(const char* name, int* min_p = nullptr) {
  const char* e = getenv(name);
  if (e && min_p && atoi(e) > 1) *min_p = atoi(e);
  return !(e && *e == '0');
}

// One conv launch: views, weights and plan (the last five: ConvDesc's own defaults); the batched / grouped / pooling fields are the caller's.
static ConvDesc conv_desc(const float* x, int x_cs, int x_coff, int n_img, int H, int W, int Ci, const float* w, const float* bias, int Co, int KH,
                          int KW, int stride, int pad, const float* res, int res_cs, int res_coff, int flags, float* y, int y_cs, int y_coff,
                          int tile_cfg = -1, int splitk = 0, float* partial = nullptr, size_t partial_floats = 0, int precision = 0) {
  ConvDesc d;
  d.x = x; d.x_cs = x_cs; d.x_coff = x_coff; d.n_img = n_img; d.H = H; d.W = W; d.Ci = Ci;
  d.w = w; d.bias = bias; d.Co = Co; d.KH = KH; d.KW = KW; d.stride = stride; d.pad = pad;
  d.res = res; d.res_cs = res_cs; d.res_coff = res_coff; d.flags = flags;
  d.y = y; d.y_cs = y_cs; d.y_coff = y_coff;
  d.tile_cfg = tile_cfg; d.splitk = splitk; d.partial = partial; d.partial_floats = partial_floats; d.precision = precision;
  return d;
}

// The batched GEMMs of a conv on a Winograd path (M[point] = V[point] . U[point]^T): one persistent launch of wino_gemm_kernel
// (wino_gemm.hip), or -- persistent == false, OFFK_WINO_GEMM=0 -- gridDim.y problems of the generic 1x1 kernel (conv_igemm.hip, 64 x 64
// LDS-DMA tile).  Bit-identical.  grp / ngrp: winograd.hip's wino_groups / winograd7.hip's wino7_groups; rows = rows of every V[point].
static hipError_t wino_gemms_launch(const WinoGroup* grp, int ngrp, int npoints, int rows, int Ci, int Co, const float* V, const float* U,
                                    float* M, bool persistent, hipStream_t s, const char** why, const void* U_planes = nullptr) {
  if (persistent || U_planes) {
    WinoGemmArgs a{};
    a.x = V; a.w = U; a.y = M; a.M = rows; a.Co = Co; a.ngroups = ngrp;
    for (int gi = 0; gi < ngrp; ++gi) {
      a.g_batch[gi] = grp[gi].batch; a.g_K[gi] = grp[gi].kmul * Ci;
      a.g_x[gi] = grp[gi].v_off; a.g_w[gi] = grp[gi].u_off; a.g_y[gi] = grp[gi].m_off;
    }
    a.w_planes = U_planes;
    if (U_planes && wino_gemm_split_supported(a)) return wino_gemm_split_launch(a, s);     // split-fp32 handles (wino_gemm_split.hip)
    if (persistent && wino_gemm_supported(a)) return wino_gemm_launch(a, s);     // every error of the launch itself goes to the caller
    // a shape the persistent kernel does not take: the generic one
  }
  const int K0 = grp[0].kmul * Ci;
  ConvDesc d = conv_desc(V, K0, 0, rows, 1, 1, K0, U, nullptr, Co, 1, 1, 1, 0, nullptr, 0, 0, 0, M, Co, 0, 3, 1);
#ifdef OFFK_TUNING_KNOBS
  { const char* e = getenv("OFFK_WINO_CFG"); if (e && (Co % 128 == 0 || atoi(e) == 1 || atoi(e) == 2)) d.tile_cfg = atoi(e); }     // tools: one tile for every Winograd GEMM launch
#endif
  d.batch = npoints; d.x_bstride = (long long)rows * K0; d.w_bstride = (long long)Co * K0; d.y_bstride = (long long)rows * Co;
  if (ngrp > 1) {
    d.ngroups = ngrp;
    for (int gi = 0; gi < ngrp; ++gi) {
      d.g_batch[gi] = grp[gi].batch; d.g_Ci[gi] = grp[gi].kmul * Ci;
      d.g_x[gi] = grp[gi].v_off; d.g_w[gi] = grp[gi].u_off; d.g_y[gi] = grp[gi].m_off;
    }
  }
  return conv2d_launch(d, s, why);
}
// stage entry points have no handle: OFFK_WINO_GEMM is read once per process for them (offk_create reads it per handle)
static bool wino_gemm_stage_default() {
  static const bool on = path_switch("OFFK_WINO_GEMM");
  return on;
}

namespace {

struct SiteSpec { const char* name; int C, H; };
// reference RGB_OFF.py:395..590 (tap sites) and the view() literals at :600..817
const SiteSpec kSites[kNumSites] = {{"3a", 256, 28}, {"3b", 320, 28}, {"3c", 576, 14}, {"4a", 576, 14}, {"4b", 576, 14},
                                    {"4c", 608, 14}, {"4d", 608, 14}, {"5a", 1024, 7}, {"5b", 1024, 7}};
// launch order of the grouped K1 grid: longest K first so the tail is made of short blocks
const int kPwOrder[kNumSites] = {7, 8, 5, 6, 2, 3, 4, 1, 0};
// fusion buffer of each site and its channel offset there (RGB_OFF.py:656, :760, :832)
const int kSiteFusion[kNumSites] = {0, 0, 1, 1, 1, 1, 1, 2, 2};
const int kSiteCoff[kNumSites] = {0, 160, 0, 160, 320, 480, 640, 0, 160};
const int kFusionC[3] = {320, 1056, 832};

// Workspace regions, one id space.  A per-site family takes kNumSites ids from its enumerator on: site_region(R_G, s).  What each region
// is called, how large it is and which handles have it: kRegions, behind the handle.
enum Region {
  R_G, R_D = R_G + kNumSites,                                                      // K1's outputs per site
  R_DG = R_D + kNumSites, R_DD = R_DG + kNumSites, R_DWP = R_DD + kNumSites,      // training side: K2b's outputs per site
  R_WGS = R_DWP + kNumSites, R_WGB = R_WGS + kNumSites,                            // ... K1b's partial slabs per site
  R_FUSION_28 = R_WGB + kNumSites, R_FUSION_14, R_FUSION_7,
  R_XT_28, R_T1_28, R_SA_28, R_SB_28, R_XU_14, R_U1_14, R_SA_14, R_XV_7, R_V1_7, R_SUM_7,
  R_LOGIT_7, R_LOGIT_14, R_LOGIT_28, R_POOLED_7, R_POOLED_14, R_POOLED_28, R_POOLPART_28, R_POOLPART_7, R_POOLPART_14,
  R_WINO_V, R_WINO_M, R_POOLPART_14T, R_POOLPART_7T, R_SPLITK, kNumRegions
};
constexpr Region site_region(Region family, int site) { return Region(family + site); }
const Region kFusionRegion[3] = {R_FUSION_28, R_FUSION_14, R_FUSION_7};      // by kSiteFusion

struct ConvSpec { const char* key; int Co, Ci, K, stride, pad; };
enum ConvId {
  C_T28, C1_28A, C2_28A, C3_28A, CB_28A, C1_28B, C2_28B, C3_28B, C1_28C, C2_28C, C3_28C,
  C_T14, C1_14A, C2_14A, C3_14A, CE_14A, C1_14B, C2_14B, C3_14B,
  C_T7, C1_7, C2_7, C3_7, CB_7, kNumConvs
};
// reference RGB_OFF.py:278-290, 308-316, 326-330
const ConvSpec kConvs[kNumConvs] = {
    {"motion_conv_trans_28", 64, 320, 7, 2, 3},      {"motion_conv1_trans_28a", 64, 64, 1, 1, 0},
    {"motion_conv2_trans_28a", 64, 64, 3, 1, 1},     {"motion_conv3_trans_28a", 256, 64, 1, 1, 0},
    {"motion_conv_branch_28a", 256, 64, 1, 1, 0},    {"motion_conv1_trans_28b", 64, 256, 1, 1, 0},
    {"motion_conv2_trans_28b", 64, 64, 3, 1, 1},     {"motion_conv3_trans_28b", 256, 64, 1, 1, 0},
    {"motion_conv1_trans_28c", 64, 256, 1, 1, 0},    {"motion_conv2_trans_28c", 64, 64, 3, 1, 1},
    {"motion_conv3_trans_28c", 256, 64, 1, 1, 0},    {"motion_conv_trans_14", 128, 1056, 5, 2, 2},
    {"motion_conv1_trans_14a", 128, 128, 1, 1, 0},   {"motion_conv2_trans_14a", 128, 128, 3, 1, 1},
    {"motion_conv3_trans_14a", 512, 128, 1, 1, 0},   {"motion_conv_expand_trans_14a", 512, 128, 1, 1, 0},
    {"motion_conv1_trans_14b", 128, 512, 1, 1, 0},   {"motion_conv2_trans_14b", 128, 128, 3, 1, 1},
    {"motion_conv3_trans_14b", 512, 128, 3, 1, 1},   {"motion_conv_trans", 256, 832, 3, 1, 1},
    {"motion_conv1_trans", 256, 256, 1, 1, 0},       {"motion_conv2_trans", 256, 256, 3, 1, 1},
    {"motion_conv3_trans", 1024, 256, 1, 1, 0},      {"motion_conv_branch_trans", 1024, 256, 1, 1, 0}};
// (tile_cfg, splitk) per fusion conv measured fastest by tools/tune_conv.py at P = 384 pairs
// (BASELINE config 2: B = 64, L = 7) on MI355X; other sizes use conv2d_auto_plan.
// (round 2: re-tuned in situ, tools/tune_forward.py --precision fp32, after the fp32 K loop went lean -- with the addressing
// VALU gone the 64x64 tile wins almost everywhere: 6.13 -> 5.89 ms; profiles/r02/tune_fp32_lean.txt)
// (round 3: after the K loops changed again -- LDS-DMA tiles, fused bottleneck chains at 28 -- the conv2d_auto_plan rule
// re-derived from the B = 42 sweep beats this table at P = 384 (5.221 vs 5.253 ms, same box) and an in-situ sweep started
// from it finds nothing better (profiles/r03/tune_b64_fp32_from_heuristic.txt): exact fp32 has no P = 384 table any more;
// {-1, 0} = automatic)
// (main 1x1, branch 1x1) pairs whose outputs are summed: RGB_OFF.py:663-666, :768-770, :839-841
struct MergedSpec { const char* name; int main_id, branch_id; };
const MergedSpec kMerged[3] = {{"merged_28a", C3_28A, CB_28A}, {"merged_14a", C3_14A, CE_14A}, {"merged_7", C3_7, CB_7}};
// test-time shape of the reference eval scripts: 10 crops x 25 segments -> P = 240 (test_rgb_off.py:24-25)
// (round 2: both tables re-tuned in situ with the buffer-addressed loaders, tools/tune_forward.py --batch 10 --length 25 --wide:
// fp32 3.64 -> 3.54 ms, bf16x3 1.77 -> 1.68 ms; profiles/r02/tune_p240_*.txt; splits the sweep reports beyond the slab space of
// the workspace run unsplit and are written as 1 here)
const int kTunedP240[kNumConvs][2] = {   // round 3: the two entries an in-situ sweep from the automatic plans still moves (3.427 -> 3.359 ms)
    {3, 2}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0},
    {4, 4}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0},
    {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}, {-1, 0}};
// plans of the three merged 1x1 convs (kMerged order): [P == 240][conv] = {tile_cfg, splitk}
const int kMergedPlan[2][3][2] = {
    {{3, 1}, {3, 1}, {3, 1}},                                         // P = 384 (and the default)
    {{1, 1}, {3, 1}, {3, 1}}};                                        // P = 240
struct HeadSpec { const char* key; int C; };
const HeadSpec kHeads[3] = {{"fc_action_motion", 1024}, {"fc_action_motion_28", 256}, {"fc_action_motion_14", 512}};
const char* kSobelKey = "sobel_edge_diagonal.conv.weight";

// (the first six: the unit parameters of a site, each its own row of kUnitParams and its own UnitParam record on the handle)
enum SlotKind { SK_GEN_W, SK_GEN_B, SK_DOWN_W, SK_DOWN_B, SK_DW_W, SK_DW_B, SK_SOBEL, SK_CONV_W, SK_CONV_B, SK_FC_W, SK_FC_B };
constexpr int kNumUnitParams = SK_DW_B + 1;
// one unit parameter of one site on a handle; slot < 0: the variant has no such parameter
struct UnitParam {
  float* own = nullptr;          // the library's copy (offk_set_weight), in the layout its kernels read
  const float* bound = nullptr;  // the caller's own tensor, reference layout, read at launch time (offk_bind_weight); nullptr: the copy is read
  int slot = -1;                 // its index in offk_handle::slots
  size_t grad_off = 0;           // where its gradient starts in the caller's gradient buffer, floats (offk_unit_grad_slot)
};
struct RegionSpan { size_t off = 0, bytes = 0; bool on = false; };      // on: the handle has the region
struct Slot {
  std::string key;
  std::vector<int64_t> shape;
  SlotKind kind;
  int idx;
  bool set = false;
};

// What is derived from the weights of one fusion conv (slot kNumConvs + m: of merged conv m); kDerived below names every image, where it
// exists, how large it is and how it is packed.  The plane images (6 bytes per element) are those of split-fp32 handles.
struct Derived {
  float* u = nullptr;            // transformed weights of the conv on its Winograd path
  float* u_planes = nullptr;     // the plane image of u (wino_gemm_split.hip); nullptr: fp32 GEMMs
  float* u2 = nullptr;           // F(2x2, 3x3) weights [16][64][64] of a chain's 3x3 conv (chain_fused.hip, OFFK_CHAIN_WINO)
  float* planes = nullptr;       // the plane image of the [Co][K] weights for the fused kernel that runs the conv: chain_split.hip (c1 / c2 in
                                 // the packed K order / c3 / the branch of chain 28a), wino_mid.hip (its 1x1 conv)
  float* gemm_planes = nullptr;  // ... for the conv as a launch of its own on wino_gemm_split.hip's kernel with its conv epilogue
  float* head = nullptr;         // merged_7 only: the 7-head composed with it, W' = Wfc Wm [num_classes][512], then b' = Wfc bm + bfc [num_classes]
};
constexpr int kNumDerived = kNumConvs + 3;
constexpr int merged_slot(int m) { return kNumConvs + m; }

thread_local std::string g_err;

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

}  // namespace

struct offk_handle {
  offk_config cfg;
  int N = 0, P = 0;
  std::vector<Slot> slots;
  std::map<std::string, int> index;
  // packed device weights
  float* pw_w[kNumSites] = {};   // [160][C]
  float* pw_wt16[kNumSites] = {};   // the same matrix in the operand order of the fused units kernel's 16-pixel form (fp32)
  float* pw_wt16s[kNumSites] = {};  // ... as three bf16 planes for the split-fp32 form (OFFK_PRECISION_F32SPLIT; 1.5 x the floats)
  bool split_gemm = false;          // a split-fp32 handle runs the Winograd GEMMs with Co % 128 == 0 in split-fp32 too (OFFK_SPLIT_GEMM=0: fp32 pipe)
  int split_gemm_skip = 0;          // (tuning builds: OFFK_SPLIT_GEMM_SKIP, the bit of a kDerived row = that image stays on the fp32 pipe)
  bool split_chain = false;         // a split-fp32 handle runs the bottleneck chains on chain_split.hip (OFFK_SPLIT_CHAIN=0: chain_fused.hip)
  bool split_mid = false;           // ... and the 1x1 convs inside wino_mid in split-fp32 (OFFK_SPLIT_MID=0: fp32 pipe)
  bool f32split = false;            // created with OFFK_PRECISION_F32SPLIT: cfg.precision is OFFK_PRECISION_FP32 inside the library, the
                                    // kernels that have a split form take it
  bool pw_dirty = true;
  float* pw_b[kNumSites] = {};   // [160]
  float* dw_w[kNumSites] = {};   // [9][32]
  float* dw_b[kNumSites] = {};   // [32] or null
  UnitParam unit[kNumSites][kNumUnitParams];   // the six parameters of a site's unit, by SlotKind: copy, binding, slot, gradient (kUnitParams)
  int sobel_slot = -1;           // the slot of kSobelKey (diag variant)
  float* sobel_w = nullptr;      // shared [9][32] (diag variant)
  bool sobel_taps4 = false;      // the loaded Sobel weight is zero outside the four taps of util.py:61 -> K2's four-tap path
  float* conv_w[kNumConvs] = {};
  float* conv_b[kNumConvs] = {};
  float* fc_w[3] = {};
  float* fc_b[3] = {};
  // residual-branch 1x1 convs merged into their sibling: out = W3*t + Wb*x == [W3|Wb] * [t|x] (K-concatenated)
  float* merged_w[3] = {};
  float* merged_b[3] = {};
  int merged_cfg[3] = {3, 3, 3}, merged_sk[3] = {1, 1, 1};   // kMergedPlan at offk_create
  bool merged_dirty = true;

  // training side (offk_off_units_backward): workspace superset, K1b chunking, gradient-buffer layout
  float* zero_page = nullptr;    // 256 B of zeros (target of masked-out loads)
  float* dx_split_w[kNumSites] = {};   // offk_off_units_backward_feats_split: plane image of [Wg ; Wd] per site, rewritten by every call (960 B per channel)
  float* fwd_split_w[kNumSites] = {};  // offk_off_units_train_split: plane image of [Wg ; Wd] per site in K1's operand order, rewritten by every call (960 B per channel)
  bool fused_units = true;       // forward: K1 fused with the temporal difference (OFFK_FUSED_UNITS=0 at offk_create: K1 + K2)
  bool winograd = true;          // fp32: Winograd F(4x4, 3x3) for the three 3x3 / stride 1 convs on 7x7 maps (winograd.hip); OFFK_WINOGRAD=0: direct
  bool wino_7x7 = true;          // the 7x7 / stride 2 conv of fusion@28 in polyphase Winograd form F(5x5, 4x4) (OFFK_WINOGRAD_7X7=0: direct)
  int wino7_min_p = 12;          // ... from this many pairs (OFFK_WINOGRAD_7X7=<n> with n > 1 at offk_create: tools)
  Derived derived[kNumDerived];  // the weight images of the Winograd, chain and split-fp32 paths, per conv (kDerived)
  bool derived_dirty = true;
  bool chain_wino = false;       // the 3x3 conv inside a bottleneck chain in Winograd F(2x2, 3x3) form (OFFK_CHAIN_WINO=0: direct)
  int wino5_min_p = 40;          // ... from this many pairs (OFFK_WINOGRAD_5X5=<n> with n > 1 at offk_create: tools)
  bool wino_5x5 = true;          // the 5x5 / stride 2 conv of fusion@14 in polyphase Winograd form (OFFK_WINOGRAD_5X5=0: direct)
  bool wino_gemm = true;         // the batched GEMMs of a Winograd conv as one persistent launch (wino_gemm.hip); false: the generic 1x1 kernel
  bool wino_mid = true;          // fp32 + Winograd: output transform + 1x1 conv + input transform between two Winograd convs in one launch
                                 // (wino_mid.hip); OFFK_WINO_MID=0 at offk_create: three launches
  bool chain = true;             // fp32: one launch per bottleneck chain of fusion@28 (chain_fused.hip); OFFK_CHAIN=0 at offk_create: three convs
  int chain_min_p = 72;          // ... from this many pairs (OFFK_CHAIN=<n> with n > 1 at offk_create: tests / tools)
  size_t train_ws_bytes = 0;
  bool units_bwd_done = false;   // an offk_off_units_backward* call has been enqueued since offk_create: dG_<site> / dD_<site> hold a backward's output
  int wg_kpb = 0;                // 32-pixel K-tiles one pw_wgrad block walks
  size_t grad_floats = 0;        // the caller's gradient buffer: every UnitParam::grad_off of the handle lies in it

  int conv_cfg[kNumConvs];       // tile plan per fusion conv (-1 = automatic)
  int conv_splitk[kNumConvs];    // K-split per fusion conv (0 = automatic)
  size_t splitk_floats = 0;      // size of the "splitk" workspace region
  // 7-head, pool first: motion_sum = merged_7(xv) feeds the head's average pool and FC alone and has no ReLU (RGB_OFF.py:839-847), so
  // logits_7 = (Wfc Wm) mean49(xv) + (Wfc bm + bfc): the producers of xv_7 leave its per-tile sums, the FC launch reads those with the composed
  // weights, and merged_7 (19.7 GFLOP at P = 384) runs only when sum_7 is asked for (offk_stage_tensors)
  bool pool_first7 = false;      // this handle takes that path: winograd, wino_mid, fold_pool on and P >= the gate of OFFK_POOL_FIRST_7 (96 pairs)
  bool sum7_pending = false;     // a forward skipped merged_7 and offk_stage_tensors has not run it since
  bool fold_pool = true;         // 7- / 14-head: average pool in the producing conv's epilogue + MFMA FC (OFFK_FOLD_POOL=0: pool + fc kernels)
  std::vector<void*> allocs;
  // workspace plan (plan_workspace walks kRegions)
  RegionSpan regions[kNumRegions];
  size_t ws_bytes = 0;
  // profiling: 0 off, 1 per-stage events, 2 per-launch trace (one event in front of every launch group, by name)
  int profiling = 0;
  std::vector<hipEvent_t> events;   // groups of OFFK_NUM_STAGES + 1
  size_t ev_used = 0;
  std::vector<hipEvent_t> tr_events;
  std::vector<int> tr_marks;        // per recorded event: index into tr_names, -1 = end of a forward
  std::vector<std::string> tr_names;
  mutable std::string err;
};

namespace {

int fail(offk_handle* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  g_err = msg;
  return code;
}
int fail_hip(offk_handle* h, hipError_t e, const char* what) {
  return fail(h, OFFK_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIP_TRY(h, expr)                                   \
  do {                                                     \
    hipError_t e__ = (expr);                               \
    if (e__ != hipSuccess) return fail_hip(h, e__, #expr); \
  } while (0)
#define TRY(expr)            \
  do {                       \
    int rc__ = (expr);       \
    if (rc__ != OFFK_OK) return rc__; \
  } while (0)

// per-launch trace (offk_set_profiling(h, 2)): an event on `st` in front of the launch group `name`; name == nullptr closes
// the forward.  The time of a group is the distance to the next mark on the same stream.
constexpr size_t kTraceMaxEvents = 1 << 16;
int trace_mark(offk_handle* h, hipStream_t st, const char* name) {
  if (h->profiling != 2 || h->tr_marks.size() >= kTraceMaxEvents) return OFFK_OK;
  int id = -1;
  if (name) {
    for (size_t i = 0; i < h->tr_names.size() && id < 0; ++i)
      if (h->tr_names[i] == name) id = (int)i;
    if (id < 0) { id = (int)h->tr_names.size(); h->tr_names.push_back(name); }
  }
  if (h->tr_marks.size() >= h->tr_events.size()) {
    hipEvent_t e;
    HIP_TRY(h, hipEventCreate(&e));
    h->tr_events.push_back(e);
  }
  HIP_TRY(h, hipEventRecord(h->tr_events[h->tr_marks.size()], st));
  h->tr_marks.push_back(id);
  return OFFK_OK;
}

int dev_alloc(offk_handle* h, float** p, size_t nfloats) {
  void* q = nullptr;
  HIP_TRY(h, hipMalloc(&q, nfloats * sizeof(float)));
  HIP_TRY(h, hipMemset(q, 0, nfloats * sizeof(float)));
  h->allocs.push_back(q);
  *p = static_cast<float*>(q);
  return OFFK_OK;
}

void add_slot(offk_handle* h, const std::string& key, std::vector<int64_t> shape, SlotKind kind, int idx) {
  Slot s;
  s.key = key; s.shape = std::move(shape); s.kind = kind; s.idx = idx;
  h->index[key] = (int)h->slots.size();
  h->slots.push_back(std::move(s));
}

// nullptr: the handle has no such region
float* region(const offk_handle* h, void* ws, Region r) {
  return h->regions[r].on ? reinterpret_cast<float*>(static_cast<char*>(ws) + h->regions[r].off) : nullptr;
}

// S-blocks of the units' backward: 7-row strips at 28x28, whole planes below (two LDS tiles per block; shorter
// strips for a third resident block per CU measured slower: 1.39 ms -> 1.41 .. 1.54 ms for the whole backward)
void ub_plan(int H, int* strips, int* rows) {
  *rows = H >= 28 ? 7 : H;
  *strips = (H + *rows - 1) / *rows;
}
constexpr int kUbTpix = 8;     // pixels per T-block of the backward: one task per thread (as K2, sobel_tdiff.hip st_tpix)

// ---- the six parameters of a site's OFF unit: ONE table, in the order of their slots (offk_missing_weights reports the first unset one) and
// of their gradients in the caller's buffer.  offk_create, plan_workspace, offk_set_weight, offk_bind_weight, site_weights_ready and
// the backward's reduce go by it; the per-site state is offk_handle::unit.  A new bindable parameter is a row. ----
constexpr int64_t kC = -1;       // in a shape: the site's channel count
struct UnitParamSpec {
  const char* prefix; const char* suffix;      // the key: <prefix><site><suffix>
  SlotKind kind;                               // = its row
  int ndim; int64_t shape[4];                  // of the reference's tensor
  bool dw;                                     // a depthwise parameter: on the learned-depthwise variant only, and what K2 / K2b read (else: K1 / K1b / dX)
  float* (offk_handle::*buf)[kNumSites];       // the library's copy lives in this per-site buffer of the handle ...
  int buf_row;                                 // ... from this row on: gen and down share one, [gen 128 ; down 32] rows -- the pack kernels read it whole
  bool repack_dw;                              // offk_set_weight stages it through repack_dw_launch ([32][1][3][3] -> [9][32]); else a plain copy
  float* WrSite::*grad;                        // where the reduce kernel is told the destination of its gradient
};
const char kGenKey[] = "motion_conv_gen_", kDownKey[] = "motion_spatial_down_", kDwKey[] = "motion_spatial_grad_";
const UnitParamSpec kUnitParams[kNumUnitParams] = {
    {kGenKey, ".weight", SK_GEN_W, 4, {kGenCh, kC, 1, 1}, false, &offk_handle::pw_w, 0, false, &WrSite::gen_w},
    {kGenKey, ".bias", SK_GEN_B, 1, {kGenCh}, false, &offk_handle::pw_b, 0, false, &WrSite::gen_b},
    {kDownKey, ".weight", SK_DOWN_W, 4, {kDownCh, kC, 1, 1}, false, &offk_handle::pw_w, kGenCh, false, &WrSite::down_w},
    {kDownKey, ".bias", SK_DOWN_B, 1, {kDownCh}, false, &offk_handle::pw_b, kGenCh, false, &WrSite::down_b},
    {kDwKey, ".weight", SK_DW_W, 4, {kDownCh, 1, 3, 3}, true, &offk_handle::dw_w, 0, true, &WrSite::dw_w},
    {kDwKey, ".bias", SK_DW_B, 1, {kDownCh}, true, &offk_handle::dw_b, 0, false, &WrSite::dw_b}};
std::vector<int64_t> unit_shape(const UnitParamSpec& p, int C) {
  std::vector<int64_t> shape(p.shape, p.shape + p.ndim);
  std::replace(shape.begin(), shape.end(), kC, (int64_t)C);
  return shape;
}
size_t unit_count(const UnitParamSpec& p, int C) {
  size_t n = 1;
  for (int i = 0; i < p.ndim; ++i) n *= (size_t)(p.shape[i] == kC ? C : p.shape[i]);
  return n;
}
// the parameter a launch reads: the tensor bound in place if there is one, else the library's copy
struct ParamPtr { const float* p; bool bound; };
ParamPtr unit_param(const offk_handle* h, int site, SlotKind k) {
  const UnitParam& u = h->unit[site][k];
  return ParamPtr{u.bound ? u.bound : u.own, u.bound != nullptr};
}
// the first site with a gen / down weight bound in place (the operand-order images of the fused units kernel are packed from the copies); -1: none
int bound_contraction_site(const offk_handle* h) {
  for (int s = 0; s < kNumSites; ++s)
    if (unit_param(h, s, SK_GEN_W).bound || unit_param(h, s, SK_DOWN_W).bound) return s;
  return -1;
}

// ---- the workspace regions: ONE table, in layout order.  plan_workspace walks it, offk_workspace_region finds names in it, everything
// else goes by id.  A new region is an enumerator and a row. ----
enum { PER_SITE = 1, TRAIN = 2 };      // PER_SITE: a family, "<name><site>" at site_region(id, site); TRAIN: behind the forward layout (offk_train_workspace_bytes)
#define OFFK_REGION_ARGS const offk_handle* h, size_t N, size_t P, int s      /* s: the site of a family's region */
struct RegionRow {
  Region id;
  const char* name;
  int flags;
  size_t (*floats)(OFFK_REGION_ARGS);
  bool (*exists)(const offk_handle* h) = nullptr;      // nullptr: on every handle
};
size_t site_hw(int s) { return (size_t)kSites[s].H * kSites[s].H; }
size_t wg_chunks(const offk_handle* h, size_t N, int s) { return (N * ((site_hw(s) + 31) / 32) + h->wg_kpb - 1) / h->wg_kpb; }      // K1b's K chunks of a site
const RegionRow kRegions[] = {
    // (a run of families is laid out site by site: G_3a, D_3a, G_3b, ...)
    {R_G, "G_", PER_SITE, [](OFFK_REGION_ARGS) { return N * site_hw(s) * kGenCh; }},
    {R_D, "D_", PER_SITE, [](OFFK_REGION_ARGS) { return P * site_hw(s) * kDownCh; }},
    {R_FUSION_28, "fusion_28", 0, [](OFFK_REGION_ARGS) { return P * 784 * 320; }},
    {R_FUSION_14, "fusion_14", 0, [](OFFK_REGION_ARGS) { return P * 196 * 1056; }},
    {R_FUSION_7, "fusion_7", 0, [](OFFK_REGION_ARGS) { return P * 49 * 832; }},
    // fusion@28 temporaries, 14x14 maps
    {R_XT_28, "xt_28", 0, [](OFFK_REGION_ARGS) { return P * 196 * 128; }},   // [t2 (c2 output) | x0 (pre-ReLU 7x7 output)]: input of the merged c3+branch conv
    {R_T1_28, "t1_28", 0, [](OFFK_REGION_ARGS) { return P * 196 * 64; }},
    {R_SA_28, "sa_28", 0, [](OFFK_REGION_ARGS) { return P * 196 * 256; }},
    {R_SB_28, "sb_28", 0, [](OFFK_REGION_ARGS) { return P * 196 * 256; }},
    // fusion@14 temporaries, 7x7 maps
    {R_XU_14, "xu_14", 0, [](OFFK_REGION_ARGS) { return P * 49 * 256; }},    // [u2 | x1]
    {R_U1_14, "u1_14", 0, [](OFFK_REGION_ARGS) { return P * 49 * 128; }},
    {R_SA_14, "sa_14", 0, [](OFFK_REGION_ARGS) { return P * 49 * 512; }},
    // fusion@7
    {R_XV_7, "xv_7", 0, [](OFFK_REGION_ARGS) { return P * 49 * 512; }},      // [v2 | x2]
    {R_V1_7, "v1_7", 0, [](OFFK_REGION_ARGS) { return P * 49 * 256; }},
    {R_SUM_7, "sum_7", 0, [](OFFK_REGION_ARGS) { return P * 49 * 1024; }},
    // per-pair logits when consensus averages them afterwards
    {R_LOGIT_7, "logit_7", 0, [](OFFK_REGION_ARGS) { return P * (size_t)h->cfg.num_classes; }},
    {R_LOGIT_14, "logit_14", 0, [](OFFK_REGION_ARGS) { return P * (size_t)h->cfg.num_classes; }},
    {R_LOGIT_28, "logit_28", 0, [](OFFK_REGION_ARGS) { return P * (size_t)h->cfg.num_classes; }},
    {R_POOLED_7, "pooled_7", 0, [](OFFK_REGION_ARGS) { return P * 1024; }},
    {R_POOLED_14, "pooled_14", 0, [](OFFK_REGION_ARGS) { return P * 512; }},
    {R_POOLED_28, "pooled_28", 0, [](OFFK_REGION_ARGS) { return P * 256; }},
    {R_POOLPART_28, "poolpart_28", 0, [](OFFK_REGION_ARGS) { return (size_t)4 * P * 256; }},   // 28-head: max-pooled cells summed per block of pool rows (maxpool_rows_kernel)
    // average pools of the 7- and 14-heads folded into the producing conv: per 32-row slab, two partial column sums
    {R_POOLPART_7, "poolpart_7", 0, [](OFFK_REGION_ARGS) { return ((P * 49 + 31) / 32) * 2 * 1024; }},
    {R_POOLPART_14, "poolpart_14", 0, [](OFFK_REGION_ARGS) { return ((P * 49 + 31) / 32) * 2 * 512; }},
    // Winograd path of the 3x3 convs at 7x7: transformed input [121][P][Ci <= 832], GEMM output [121][P][Co <= 512], per-tile sums of
    // sum_14b for the 14-head.  wino_v, widest: the polyphase 7x7 / 2 conv (9 P tiles x 225 x 320 floats: 1.0 GB at P = 384), then the
    // polyphase 5x5 / 2 conv (400 P x 1056)
    {R_WINO_V, "wino_v", 0, [](OFFK_REGION_ARGS) { return std::max((size_t)kWinoUnits4 * P * 1056, (size_t)kWino7Tiles * P * kWino7Units * 320); }},
    {R_WINO_M, "wino_m", 0, [](OFFK_REGION_ARGS) { return (size_t)kWinoPoints * P * 512; }},    // (7x7: 64 x 9 P x 64 is smaller)
    {R_POOLPART_14T, "poolpart_14t", 0, [](OFFK_REGION_ARGS) { return (size_t)4 * P * 512; }},
    {R_POOLPART_7T, "poolpart_7t", 0, [](OFFK_REGION_ARGS) { return (size_t)4 * P * 512; },      // per-tile sums of xv_7 = [v2 | x2]
     [](const offk_handle* h) { return h->pool_first7; }},
    {R_SPLITK, "splitk", 0, [](OFFK_REGION_ARGS) { return h->splitk_floats; }},
    // training side (offk_off_units_backward*)
    {R_DG, "dG_", PER_SITE | TRAIN, [](OFFK_REGION_ARGS) { return N * site_hw(s) * kGenCh; }},
    {R_DD, "dD_", PER_SITE | TRAIN, [](OFFK_REGION_ARGS) { return P * site_hw(s) * kDownCh; }},
    {R_DWP, "dwp_", PER_SITE | TRAIN, [](OFFK_REGION_ARGS) {
       int strips, rows;
       ub_plan(kSites[s].H, &strips, &rows);
       return P * strips * 10 * kDownCh;
     }},
    {R_WGS, "wgs_", PER_SITE | TRAIN, [](OFFK_REGION_ARGS) { return wg_chunks(h, N, s) * kUnitCh * ((size_t)((kSites[s].C + 127) / 128) * 128); }},
    {R_WGB, "wgb_", PER_SITE | TRAIN, [](OFFK_REGION_ARGS) { return wg_chunks(h, N, s) * kUnitCh; }}};
constexpr int kNumRegionRows = sizeof(kRegions) / sizeof(kRegions[0]);

// the id behind a name (offk_workspace_region); kNumRegions: no region is called that
Region region_by_name(const char* name) {
  for (const RegionRow& row : kRegions) {
    const size_t n = (row.flags & PER_SITE) ? strlen(row.name) : 0;
    if (!n && !strcmp(name, row.name)) return row.id;
    for (int s = 0; n && s < kNumSites; ++s)
      if (!strncmp(name, row.name, n) && !strcmp(name + n, kSites[s].name)) return site_region(row.id, s);
  }
  return kNumRegions;
}

void plan_workspace(offk_handle* h) {
  const size_t N = h->N, P = h->P;
  // split-K partial slabs: room for 8 slices of the widest large-K conv output (7x7: [P*196, 64], 3x3 @7: [P*49, 256]) -- up
  // to 64 at small P, where the plans split deeper (conv2d_auto_plan); a conv whose plan needs more gets as many as fit
  h->splitk_floats = (size_t)std::min<size_t>(64, std::max<size_t>(8, 1536 / P)) * P * 196 * 64;
  long long work = 0;   // (K-tile, channel slab) steps of the grouped weight-gradient GEMM
  for (int s = 0; s < kNumSites; ++s) work += (long long)N * ((site_hw(s) + 31) / 32) * ((kSites[s].C + 127) / 128);
  h->wg_kpb = (int)std::max<long long>(4, (work + 1535) / 1536);

  size_t end = 0, fwd_end = 0;
  for (int i = 0, j; i < kNumRegionRows; i = j) {
    const int flags = kRegions[i].flags;
    for (j = i + 1; (flags & PER_SITE) && j < kNumRegionRows && kRegions[j].flags == flags; ++j) {}      // rows [i, j): one region, or a run of families
    for (int s = 0; s < ((flags & PER_SITE) ? kNumSites : 1); ++s)
      for (int r = i; r < j; ++r) {
        const RegionRow& row = kRegions[r];
        if (row.exists && !row.exists(h)) continue;
        RegionSpan& sp = h->regions[site_region(row.id, s)];
        sp.off = align_up(end, 256);
        sp.bytes = row.floats(h, N, P, s) * sizeof(float);
        sp.on = true;
        end = sp.off + sp.bytes;
        if (!(flags & TRAIN)) fwd_end = end;
      }
  }
  h->ws_bytes = align_up(fwd_end, 256);
  h->train_ws_bytes = align_up(end, 256);      // the forward layout with the backward's regions behind it

  // the caller's gradient buffer: per site, the parameters the variant has, in table order
  for (int s = 0; s < kNumSites; ++s)
    for (const UnitParamSpec& p : kUnitParams)
      if (h->unit[s][p.kind].slot >= 0) {
        h->unit[s][p.kind].grad_off = h->grad_floats;
        h->grad_floats += unit_count(p, kSites[s].C);
      }
}

struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int want) {
    if (hipGetDevice(&prev) == hipSuccess && prev != want) changed = hipSetDevice(want) == hipSuccess;
  }
  ~DeviceGuard() { if (changed) (void)hipSetDevice(prev); }
};

int check_ready(offk_handle* h) {
  for (const Slot& s : h->slots)
    if (!s.set) return fail(h, OFFK_ERR_MISSING_WEIGHT, "weight not set: " + s.key);
  return OFFK_OK;
}

// need_pw: the four 1x1 parameters of the site (K1, K1b, dX); need_dw: its depthwise ones, or the shared Sobel weight (K2, K2b)
int site_weights_ready(offk_handle* h, int site, bool need_pw, bool need_dw) {
  auto ready = [&](int slot) { return h->slots[slot].set ? OFFK_OK : fail(h, OFFK_ERR_MISSING_WEIGHT, "weight not set: " + h->slots[slot].key); };
  for (const UnitParamSpec& p : kUnitParams)
    if ((p.dw ? need_dw : need_pw) && h->unit[site][p.kind].slot >= 0) TRY(ready(h->unit[site][p.kind].slot));
  if (need_dw && h->sobel_slot >= 0) TRY(ready(h->sobel_slot));
  return OFFK_OK;
}

void pw_weight_ptrs(const offk_handle* h, int site, const float** w, const float** w_down, const float** b,
                    const float** b_down) {
  *w = unit_param(h, site, SK_GEN_W).p;
  *w_down = unit_param(h, site, SK_DOWN_W).p;
  *b = unit_param(h, site, SK_GEN_B).p;
  *b_down = unit_param(h, site, SK_DOWN_B).p;
}

// What the per-site records of the units' launches share, filled where a record has the fields: the map as channel groups (xp / cp /
// nparts; fp == nullptr: none to fill), C, HW and the row count M = N HW (PtSite's M is its fusion buffer: not that one).
template <class S, class = void> struct has_parts : std::false_type {};
template <class S> struct has_parts<S, std::void_t<decltype(S::nparts)>> : std::true_type {};
template <class S, class = void> struct has_rows : std::false_type {};
template <class S> struct has_rows<S, std::enable_if_t<std::is_same<decltype(S::M), int>::value>> : std::true_type {};
template <class S>
void fill_site_shape(const offk_handle* h, int site, const offk_feat_parts* fp, S* o) {
  if constexpr (has_parts<S>::value) {
    for (int q = 0; q < 4; ++q) { o->xp[q] = q < fp->n_parts ? fp->data[q] : nullptr; o->cp[q] = q < fp->n_parts ? fp->channels[q] : 0; }
    o->nparts = fp->n_parts;
  }
  o->C = kSites[site].C; o->HW = kSites[site].H * kSites[site].H;
  if constexpr (has_rows<S>::value) o->M = h->N * o->HW;
}

void fill_pw_site(const offk_handle* h, int site, const offk_feat_parts& fp, float* G, float* D, PwSite* o) {
  fill_site_shape(h, site, &fp, o);
  pw_weight_ptrs(h, site, &o->w, &o->w_down, &o->bias, &o->bias_down);
  o->G = G; o->D = D;
  o->blk_begin = 0;
}
void fill_st_site(const offk_handle* h, int site, const float* G, const float* D, float* M, int m_cs, int m_coff, StSite* o) {
  o->G = G; o->D = D;
  // one unit = [S 32 | T 128] of a channels-last row (RGB_OFF.py:616); the kernel takes the two halves as separate views
  o->Ms = M; o->s_cs = m_cs; o->s_coff = m_coff; o->Mt = M; o->t_cs = m_cs; o->t_coff = m_coff + kDownCh;
  const bool sobel = h->cfg.variant == OFFK_VARIANT_DIAG_SOBEL;
  o->dw = sobel ? h->sobel_w : unit_param(h, site, SK_DW_W).p;
  o->dw_ref = !sobel && unit_param(h, site, SK_DW_W).bound;
  o->db = sobel ? nullptr : unit_param(h, site, SK_DW_B).p;
  o->H = kSites[site].H;
  st_plan(o->H, &o->strips, &o->rows);
  st_recips(o->H, &o->wrecip, &o->twrecip);
  o->tchunks = st_tchunks(o->H);
  o->s_begin = 0; o->t_begin = 0;
}

struct DropCfg { unsigned thresh = 0; float scale = 1.f; unsigned long long seed = 0; };
int make_drop(offk_handle* h, unsigned long long seed, double p, DropCfg* d) {
  if (!(p >= 0.0) || p >= 1.0) return fail(h, OFFK_ERR_INVALID, "dropout probability must be in [0, 1)");
  d->thresh = (unsigned)llround(p * 65536.0);
  d->scale = (float)(1.0 / (1.0 - p));
  d->seed = seed;
  return OFFK_OK;
}

int run_sobel_tdiff_all(offk_handle* h, hipStream_t st, void* ws, int algo, const DropCfg& drop = DropCfg()) {
  StParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.nsites = kNumSites; sp.B = h->cfg.batch; sp.L = h->cfg.length;
  sp.drop_thresh = drop.thresh; sp.drop_scale = drop.scale;
  sp.zeros = h->zero_page;
  sp.taps4 = h->cfg.variant == OFFK_VARIANT_DIAG_SOBEL && h->sobel_taps4;
  int sblk = 0, tblk = 0;
  for (int s = 0; s < kNumSites; ++s) {
    fill_st_site(h, s, region(h, ws, site_region(R_G, s)),
                 region(h, ws, site_region(R_D, s)), region(h, ws, kFusionRegion[kSiteFusion[s]]),
                 kFusionC[kSiteFusion[s]], kSiteCoff[s], &sp.s[s]);
    sp.s[s].s_begin = sblk;
    sp.s[s].drop_base = drop_stream_base(drop.seed, s);
    sblk += h->P * sp.s[s].strips;
    if (algo >= 4) sp.s[s].tchunks = st_tchunks_flat(kSites[s].H, h->cfg.length);
    sp.s[s].t_begin = tblk;
    tblk += h->cfg.batch * sp.s[s].tchunks;
  }
  sp.total_s = sblk; sp.total_t = tblk;
  HIP_TRY(h, sobel_tdiff_launch(sp, algo, st));
  return OFFK_OK;
}

offk_feat_parts whole_map(int site, const float* p) {
  offk_feat_parts fp;
  memset(&fp, 0, sizeof(fp));
  fp.n_parts = 1; fp.channels[0] = kSites[site].C; fp.data[0] = p;
  return fp;
}

// nine non-null pointers -> nine whole maps, else "<fn>: null feature map"
template <class T>
int whole_maps(offk_handle* h, const T* const feats[], offk_feat_parts parts[], const char* fn) {
  for (int s = 0; s < kNumSites; ++s) {
    if (!feats[s]) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null feature map");
    parts[s] = whole_map(s, static_cast<const float*>(feats[s]));
  }
  return OFFK_OK;
}

int check_parts(offk_handle* h, const offk_feat_parts parts[]) {
  for (int s = 0; s < kNumSites; ++s) {
    const offk_feat_parts& fp = parts[s];
    if (fp.n_parts < 1 || fp.n_parts > 4) return fail(h, OFFK_ERR_INVALID, "feature map must come as 1..4 channel groups");
    int sum = 0;
    for (int q = 0; q < fp.n_parts; ++q) {
      if (!fp.data[q]) return fail(h, OFFK_ERR_INVALID, "null feature map");
      if (fp.channels[q] <= 0 || fp.channels[q] % 32) return fail(h, OFFK_ERR_INVALID, "channel groups must be multiples of 32 channels");
      sum += fp.channels[q];
    }
    if (sum != kSites[s].C) return fail(h, OFFK_ERR_INVALID, std::string("channel groups of site ") + kSites[s].name + " do not add up to C");
  }
  return OFFK_OK;
}

int finalize_pw(offk_handle* h, hipStream_t st) {
  if (!h->pw_dirty) return OFFK_OK;
  // the operand-order image the fused units kernel reads straight into registers (pw_tdiff16_kernel; split-fp32: the plane image too)
  for (int s = 0; s < kNumSites; ++s) HIP_TRY(h, pw_pack_direct16_launch(h->pw_w[s], kSites[s].C, h->pw_wt16[s], st));
  if (h->f32split)
    for (int s = 0; s < kNumSites; ++s) HIP_TRY(h, pw_pack_split16_launch(h->pw_w[s], kSites[s].C, h->pw_wt16s[s], st));
  h->pw_dirty = false;
  return OFFK_OK;
}

// ---- the kinds of feature maps beside contiguous fp32: 16-bit NCHW (the _typed entries), channels-last in any dtype (the _cl entries) ----
// One table for both sides.  Channels-last: the layout belongs to the call, cfg.feat_layout is not looked at.
struct FeatKind {
  const char* noun;      // in the messages
  bool f32_ok;           // OFFK_FEAT_F32 is one of its dtypes (the _typed entries forward it to the untyped entry instead)
  int align;             // of the map pointers, bytes: the inference side (K1T)
  int align_train;       // ... the training side (K1, K1b)
  bool cl;               // channels-last parts (else NCHW, and an NHWC handle is refused)
};
// Pointer alignments, bytes, each from the widest load of the kernels behind it:
constexpr int kAlign16Infer = 4;    // 16-bit NCHW, K1T: the 28x28 and 14x14 sites are read as pixel pairs (pw_tdiff_f16.hip)
constexpr int kAlign16Train = 8;    // 16-bit NCHW, K1 / K1b: four pixels per load there (pw_reduce.hip, units_bwd.hip) -- intended, not drift from 4
constexpr int kAlignCl = 16;        // channels-last, every loader on either side: 16-byte pieces of a pixel's channel row
constexpr FeatKind kKind16{"16-bit", false, kAlign16Infer, kAlign16Train, false}, kKindCl{"channels-last", true, kAlignCl, kAlignCl, true};
// one 16-bit map, bytes (either kind, training side): K1 / K1b address such maps through a buffer descriptor (pw_reduce.hip, 2 GiB less a guard)
constexpr unsigned long long kFeat16MaxBytes = 0x7fffff00ull;

// The launchers of K1, K1T and K1b by (channels-last, feat_dtype), each with the name its launch goes under in the per-launch
// trace: [channels-last][enum offk_feat_dtype].  K1 on channels-last fp32 maps is the plain kernel (its nhwc form) under the plain name.
constexpr const char* kK1Plain = "units:pw_reduce (K1)";
const char* const kK1Name[2][3] = {{kK1Plain, "units:pw_reduce (K1, bf16 maps)", "units:pw_reduce (K1, fp16 maps)"},
                                   {kK1Plain, "units:pw_reduce (K1, channels-last bf16 maps)", "units:pw_reduce (K1, channels-last fp16 maps)"}};
const char* const kK1TName[2][3] = {{"units:pw_tdiff (K1T)", "units:pw_tdiff (K1T, bf16 maps)", "units:pw_tdiff (K1T, fp16 maps)"},
                                    {"units:pw_tdiff (K1T, channels-last maps)", "units:pw_tdiff (K1T, channels-last bf16 maps)",
                                     "units:pw_tdiff (K1T, channels-last fp16 maps)"}};
// K1 (pw_reduce.hip; pp.nhwc says channels-last).  traced: false for the stage entries offk_pw_reduce*, which leave no mark.
int launch_k1(offk_handle* h, hipStream_t st, const PwParams& pp, int feat_dtype, bool traced) {
  if (traced) TRY(trace_mark(h, st, kK1Name[pp.nhwc ? 1 : 0][feat_dtype]));
  if (feat_dtype != OFFK_FEAT_F32) HIP_TRY(h, pw_reduce_feat16_launch(pp, feat_dtype, st));
  else HIP_TRY(h, pw_reduce_launch(pp, st));
  return OFFK_OK;
}
// K1T (pw_tdiff.hip / pw_tdiff_split.hip; pw_tdiff_f16.hip; pw_tdiff_cl.hip)
int launch_k1t(offk_handle* h, hipStream_t st, const PtParams& pt, int feat_dtype, bool cl) {
  TRY(trace_mark(h, st, kK1TName[cl][feat_dtype]));
  if (cl) HIP_TRY(h, pw_tdiff_cl_launch(pt, feat_dtype, st));
  else if (feat_dtype != OFFK_FEAT_F32) HIP_TRY(h, pw_tdiff_feat16_launch(pt, feat_dtype, st));
  else HIP_TRY(h, pw_tdiff_launch(pt, st));
  return OFFK_OK;
}
// K1b (units_bwd.hip, units_bwd_cl.hip); the backward leaves no marks in the trace
int launch_k1b(offk_handle* h, hipStream_t st, const WgParams& wp, int feat_dtype, bool cl) {
  if (cl) HIP_TRY(h, pw_wgrad_cl_launch(wp, feat_dtype, st));
  else if (feat_dtype != OFFK_FEAT_F32) HIP_TRY(h, pw_wgrad_feat16_launch(wp, feat_dtype, st));
  else HIP_TRY(h, pw_wgrad_launch(wp, st));
  return OFFK_OK;
}

// feat_dtype OFFK_FEAT_BF16 / OFFK_FEAT_F16 (the typed training entries; check_feat_train has passed): K1 runs its 16-bit map form
// on the same grid; the parts' data pointers then address 16-bit elements.
// nhwc: the maps of THIS call are channels-last (the untyped entries pass the handle's cfg.feat_layout, the _cl entries true).
int run_off_units(offk_handle* h, hipStream_t st, const offk_feat_parts feats[], void* ws, hipEvent_t* ev, bool nhwc,
                  const DropCfg& drop = DropCfg(), int feat_dtype = OFFK_FEAT_F32) {
  { int rc = finalize_pw(h, st); if (rc != OFFK_OK) return rc; }
  PwParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.nsites = kNumSites; pp.L = h->cfg.length; pp.P = h->P; pp.slice_mode = h->cfg.slice_mode;
  pp.nhwc = nhwc;
  pp.zeros = h->zero_page;
  int blk = 0;
  for (int i = 0; i < kNumSites; ++i) {
    int s = kPwOrder[i];
    fill_pw_site(h, s, feats[s], region(h, ws, site_region(R_G, s)),
                 region(h, ws, site_region(R_D, s)), &pp.s[i]);
    pp.s[i].blk_begin = blk;
    blk += pw_blocks_for(pp.s[i].M);
  }
  pp.total_blocks = blk;
  if (ev) HIP_TRY(h, hipEventRecord(ev[0], st));
  if (feat_dtype != OFFK_FEAT_F32 && !pw_reduce_feat16_supported(pp))
    return fail(h, OFFK_ERR_INVALID, "16-bit feature maps: a map of 2 GiB or more is not supported");
  TRY(launch_k1(h, st, pp, feat_dtype, true));
  if (ev) HIP_TRY(h, hipEventRecord(ev[1], st));

  { int rc = trace_mark(h, st, "units:sobel_tdiff (K2)"); if (rc != OFFK_OK) return rc; }
  { int rc = run_sobel_tdiff_all(h, st, ws, 0, drop); if (rc != OFFK_OK) return rc; }
  if (ev) HIP_TRY(h, hipEventRecord(ev[2], st));
  return OFFK_OK;
}

// offk_off_units_train_split: run_off_units with K1 in split-fp32 arithmetic (units_fwd_split.hip) -- the weight pre-pass, the GEMM on K1's
// grid into the same G_<site> / D_<site> regions, then K2 as above.  cl: the maps of THIS call are channels-last.
const char* const kK1SplitPack = "units:pw_reduce weight cut (K1, split)";
const char* const kK1SplitName[2][3] = {
    {"units:pw_reduce (K1, NCHW, split)", "units:pw_reduce (K1, NCHW, split, bf16)", "units:pw_reduce (K1, NCHW, split, fp16)"},
    {"units:pw_reduce (K1, NHWC, split)", "units:pw_reduce (K1, NHWC, split, bf16)", "units:pw_reduce (K1, NHWC, split, fp16)"}};
int run_off_units_split(offk_handle* h, hipStream_t st, const offk_feat_parts feats[], void* ws, bool cl, const DropCfg& drop, int feat_dtype) {
  TRY(finalize_pw(h, st));
  UfsParams up;
  memset(&up, 0, sizeof(up));
  up.nsites = kNumSites; up.L = h->cfg.length; up.P = h->P; up.slice_mode = h->cfg.slice_mode;
  int blk = 0, pblk = 0;
  for (int i = 0; i < kNumSites; ++i) {
    const int s = kPwOrder[i];
    UfsSite& o = up.s[i];
    fill_site_shape(h, s, &feats[s], &o);
    pw_weight_ptrs(h, s, &o.wg, &o.wd, &o.bias, &o.bias_down);
    o.wimg = h->fwd_split_w[s];
    o.G = region(h, ws, site_region(R_G, s));
    o.D = region(h, ws, site_region(R_D, s));
    o.blk_begin = blk; o.pack_begin = pblk;
    blk += pw_blocks_for(o.M);
    pblk += units_fwd_split_pack_blocks(o.C);
  }
  up.total_blocks = blk; up.pack_blocks = pblk;
  TRY(trace_mark(h, st, kK1SplitPack));
  HIP_TRY(h, units_fwd_split_pack_launch(up, st));
  TRY(trace_mark(h, st, kK1SplitName[cl ? 1 : 0][feat_dtype]));
  HIP_TRY(h, units_fwd_split_launch(up, feat_dtype, cl, st));
  TRY(trace_mark(h, st, "units:sobel_tdiff (K2)"));
  TRY(run_sobel_tdiff_all(h, st, ws, 0, drop));
  return trace_mark(h, st, nullptr);
}

// Inference path of the units: K1 fused with the temporal difference (pw_tdiff.hip), then the S-blocks of K2 alone.
// feat_dtype OFFK_FEAT_BF16 / OFFK_FEAT_F16 (split-fp32 handles, the library's own weight image: offk_forward_typed checks): the
// 16-bit maps' units kernel (pw_tdiff_f16.hip), which writes the same regions with the same values.
// cl (offk_forward_cl and its siblings, whose checks have passed): every part is physically channels-last, elements of feat_dtype --
// the channels-last units kernel (pw_tdiff_cl.hip), the same regions with the same values again.  (Both: one block body,
// pw_tdiff_staged.h, with a loader each.)
int run_off_units_fused(offk_handle* h, hipStream_t st, const offk_feat_parts feats[], void* ws, hipEvent_t* ev, int feat_dtype = OFFK_FEAT_F32,
                        bool cl = false) {
  { int rc = finalize_pw(h, st); if (rc != OFFK_OK) return rc; }
  PtParams pt;
  memset(&pt, 0, sizeof(pt));
  pt.nsites = kNumSites; pt.B = h->cfg.batch; pt.L = h->cfg.length; pt.P = h->P; pt.slice_mode = h->cfg.slice_mode;
  pt.tgroups = pt_tgroups(h->cfg.length);
  pt.zeros = h->zero_page;
  // the operand-order weight image is the library's own copy: not with contraction weights bound in place
  pt.bdirect = bound_contraction_site(h) < 0;
  pt.f32split = h->f32split;
  for (int i = 0; i < kNumSites; ++i) {      // (the block layout -- chunks, leftover blocks, blk_begin, total_blocks -- is the launchers')
    const int s = kPwOrder[i];
    PtSite& o = pt.s[i];
    fill_site_shape(h, s, &feats[s], &o);
    pw_weight_ptrs(h, s, &o.w, &o.w_down, &o.bias, &o.bias_down);
    o.wt = nullptr;
    o.wt16 = h->pw_wt16[s];
    o.wt16s = h->pw_wt16s[s];
    o.D = region(h, ws, site_region(R_D, s));
    o.M = region(h, ws, kFusionRegion[kSiteFusion[s]]);
    o.m_cs = kFusionC[kSiteFusion[s]]; o.m_coff = kSiteCoff[s];
  }
  if (ev) HIP_TRY(h, hipEventRecord(ev[0], st));
  TRY(launch_k1t(h, st, pt, feat_dtype, cl));
  if (ev) HIP_TRY(h, hipEventRecord(ev[1], st));
  { int rc = trace_mark(h, st, "units:sobel S-blocks (K2 spatial half)"); if (rc != OFFK_OK) return rc; }
  { int rc = run_sobel_tdiff_all(h, st, ws, 3); if (rc != OFFK_OK) return rc; }   // S-blocks only: M[.., coff .. coff+32)
  if (ev) HIP_TRY(h, hipEventRecord(ev[2], st));
  return OFFK_OK;
}

// ---- the training side of the kinds (K1 + K2, K1b): what offk_pw_reduce_typed / _cl and their siblings refuse, and the bodies they share ----
// Everything such a call is refused for, checked before anything is enqueued.  Unlike check_feat (the inference forward) there is no
// condition on the handle's precision, on bound weights or on OFFK_FUSED_UNITS: these entries run the fp32 kernels K1 / K1b.
int check_feat_train(offk_handle* h, const FeatKind& k, int feat_dtype, const void* const* feats, int first, int count, const char* fn) {
  const std::string f(fn), maps = std::string(": ") + k.noun + " feature map";
  if (!(feat_dtype == OFFK_FEAT_F32 && k.f32_ok) && feat_dtype != OFFK_FEAT_BF16 && feat_dtype != OFFK_FEAT_F16)
    return fail(h, OFFK_ERR_INVALID, f + ": unknown feat_dtype " + std::to_string(feat_dtype) + " (OFFK_FEAT_F32 / _BF16 / _F16)");
  if (!k.cl && h->cfg.feat_layout == OFFK_FEAT_NHWC) return fail(h, OFFK_ERR_INVALID, f + maps + "s are NCHW-only (this handle is NHWC)");
  for (int i = 0; i < count; ++i) {
    const SiteSpec& site = kSites[first + i];
    if (!feats[i]) return fail(h, OFFK_ERR_INVALID, f + ": null feature map");
    if (reinterpret_cast<uintptr_t>(feats[i]) & (k.align_train - 1))
      return fail(h, OFFK_ERR_INVALID, f + maps + " pointers must be " + std::to_string(k.align_train) + "-byte aligned (site " + site.name + ")");
    if (feat_dtype != OFFK_FEAT_F32 && (unsigned long long)h->N * site.H * site.H * site.C * 2ull >= kFeat16MaxBytes)
      return fail(h, OFFK_ERR_INVALID, f + ": 16-bit feature maps of 2 GiB or more are not supported (site " + site.name + ")");
  }
  return OFFK_OK;
}

// K1 of one site into the caller's G / D: offk_pw_reduce (k == nullptr: the handle's layout, fp32) and its _typed / _cl forms
int pw_reduce_site(offk_handle* h, void* stream, const FeatKind* k, int feat_dtype, int site, const void* feat, float* G, float* D, const char* fn) {
  if (!h || site < 0 || site >= kNumSites || !feat || !G || !D) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": bad argument");
  if (k) TRY(check_feat_train(h, *k, feat_dtype, &feat, site, 1, fn));
  TRY(site_weights_ready(h, site, true, false));
  DeviceGuard guard(h->cfg.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PwParams pp;
  memset(&pp, 0, sizeof(pp));
  pp.nsites = 1; pp.L = h->cfg.length; pp.P = h->P; pp.slice_mode = h->cfg.slice_mode;
  pp.nhwc = k ? k->cl : h->cfg.feat_layout == OFFK_FEAT_NHWC;
  pp.zeros = h->zero_page;
  TRY(finalize_pw(h, st));
  fill_pw_site(h, site, whole_map(site, static_cast<const float*>(feat)), G, D, &pp.s[0]);
  pp.total_blocks = pw_blocks_for(pp.s[0].M);
  return launch_k1(h, st, pp, feat_dtype, false);
}

// K1 + K2 of nine whole maps into the workspace: offk_off_units, offk_off_units_train (train: with the dropout of drop_seed / drop_p)
// and their _typed / _cl forms (k == nullptr: the plain entries -- the handle's layout, fp32)
int off_units_whole(offk_handle* h, void* stream, const FeatKind* k, int feat_dtype, const void* const feats[OFFK_NUM_SITES], void* workspace,
                    bool train, uint64_t drop_seed, double drop_p, const char* fn) {
  if (!h || !feats || !workspace) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  DropCfg drop;
  if (train) TRY(make_drop(h, drop_seed, drop_p, &drop));
  if (k) TRY(check_feat_train(h, *k, feat_dtype, feats, 0, kNumSites, fn));
  offk_feat_parts parts[kNumSites];
  TRY(whole_maps(h, feats, parts, fn));
  for (int s = 0; s < kNumSites; ++s) TRY(site_weights_ready(h, s, true, true));
  DeviceGuard guard(h->cfg.device);
  return run_off_units(h, static_cast<hipStream_t>(stream), parts, workspace, nullptr, k ? k->cl : h->cfg.feat_layout == OFFK_FEAT_NHWC, drop,
                       feat_dtype);
}

struct View { const float* p; int cs, coff; };

// ---- what is derived from the fusion convs' weights: ONE table.  offk_create walks it to allocate, finalize_derived to pack, and the
// forward asks h->derived[conv] (Derived, above) for what a launch needs. ----
enum DerivedKind {
  DK_U_F43,        // Winograd F(4, 3) x F(3, 3) U of a 3x3 / stride 1 conv on 7x7 maps: 121 points (winograd.hip)
  DK_U_POLY,       // U of the 5x5 / stride 2 conv in polyphase form: 400 row-Ci units in four K groups (winograd.hip, phases = 4)
  DK_U_F54,        // F(5x5, 4x4) U of the 7x7 / stride 2 conv: 225 units in four groups (winograd7.hip)
  DK_CHAIN_U2,     // F(2x2, 3x3) U2 of a bottleneck chain's 3x3 conv (chain_fused.hip)
  DK_PLANES,       // split-fp32 plane image of a [Co][K] matrix (wino_pack_split_launch, one problem)
  DK_U_PLANES,     // split-fp32 plane image of the conv's U, group by group
  DK_HEAD_COMPOSED // the 7-head's FC composed with merged conv 7 (heads.hip: head_compose_launch); its sources are biases and FC slots too
};
DerivedKind u_kind(const ConvSpec& c) { return c.K == 7 ? DK_U_F54 : c.K == 5 ? DK_U_POLY : DK_U_F43; }
int u_units(DerivedKind k) { return k == DK_U_F54 ? kWino7Units : k == DK_U_POLY ? kWinoUnits4 : kWinoPoints; }
size_t u_elems(const ConvSpec& c) { return (size_t)u_units(u_kind(c)) * c.Co * c.Ci; }
int wino_phases(const ConvSpec& c) { return u_kind(c) == DK_U_POLY ? 4 : 1; }      // winograd.hip's `phases` of a conv on that path
// the K groups of the conv's batched GEMMs with `rows` rows per V[point] (winograd.hip / winograd7.hip; the offsets into U do not depend on rows)
int wino_conv_groups(const ConvSpec& c, long long rows, WinoGroup grp[4]) {
  return u_kind(c) == DK_U_F54 ? wino7_groups(rows, c.Ci, c.Co, grp) : wino_groups(wino_phases(c), rows, c.Ci, c.Co, grp);
}
size_t plane_floats(size_t elems) { return (elems * 3 + 1) / 2; }                  // three bf16 planes: 6 bytes per element

// the handle switches an image needs: all of a row's bits, each stated once in derived_exists, and h->winograd (every image belongs to
// a path OFFK_WINOGRAD=0 turns off -- the chain and wino_mid plane images too: such a handle runs chain_fused.hip's direct form and no wino_mid)
enum { ON_7X7 = 1, ON_SPLIT_GEMM = 2, ON_CHAIN_WINO = 4, ON_SPLIT_CHAIN = 8, ON_SPLIT_MID = 16, ON_POOL_FIRST7 = 32 };
struct DerivedRow {
  int slot;                      // ConvId, or merged_slot(m)
  DerivedKind kind;
  float* Derived::*image;        // where the image lives in h->derived[slot]
  int needs = 0;                 // ON_* bits
  int skip_bit = 0;              // tuning builds: its bit in OFFK_SPLIT_GEMM_SKIP
  int alloc_K = 0;               // > 0: DK_PLANES sized for this K (chain 28a's c1 has always been allocated like its siblings' 256-channel c1)
};
bool derived_exists(const offk_handle* h, const DerivedRow& r) {
  const int on = h->wino_7x7 * ON_7X7 | h->split_gemm * ON_SPLIT_GEMM | h->chain_wino * ON_CHAIN_WINO | (h->chain && h->split_chain) * ON_SPLIT_CHAIN |
                 (h->wino_mid && h->split_mid) * ON_SPLIT_MID | h->pool_first7 * ON_POOL_FIRST7;
  const bool shape = r.kind != DK_U_PLANES || (kConvs[r.slot].Co % 64 == 0 && kConvs[r.slot].Ci >= 64);      // (Co = 64: the kernel's 64-channel form)
  return h->winograd && !(r.needs & ~on) && shape && !(h->split_gemm_skip & r.skip_bit);
}

const DerivedRow kDerived[] = {      // (a conv's U in front of the plane image of that U: finalize_derived packs in this order)
    {C3_14B, DK_U_F43, &Derived::u}, {C_T7, DK_U_F43, &Derived::u}, {C2_7, DK_U_F43, &Derived::u}, {C2_14A, DK_U_F43, &Derived::u},
    {C2_14B, DK_U_F43, &Derived::u}, {C_T14, DK_U_POLY, &Derived::u}, {C_T28, DK_U_F54, &Derived::u, ON_7X7},
    {C3_14B, DK_U_PLANES, &Derived::u_planes, ON_SPLIT_GEMM, 1}, {C_T7, DK_U_PLANES, &Derived::u_planes, ON_SPLIT_GEMM, 2},
    {C2_7, DK_U_PLANES, &Derived::u_planes, ON_SPLIT_GEMM, 4}, {C2_14A, DK_U_PLANES, &Derived::u_planes, ON_SPLIT_GEMM, 8},
    {C2_14B, DK_U_PLANES, &Derived::u_planes, ON_SPLIT_GEMM, 16}, {C_T14, DK_U_PLANES, &Derived::u_planes, ON_SPLIT_GEMM, 32},
    {C_T28, DK_U_PLANES, &Derived::u_planes, ON_7X7 | ON_SPLIT_GEMM, 64},
    // the 1x1 convs on 7x7 maps as launches of their own on wino_gemm_split.hip
    {merged_slot(1), DK_PLANES, &Derived::gemm_planes, ON_SPLIT_GEMM, 128}, {merged_slot(2), DK_PLANES, &Derived::gemm_planes, ON_SPLIT_GEMM, 128},
    {C1_14B, DK_PLANES, &Derived::gemm_planes, ON_SPLIT_GEMM, 128},
    {C2_28A, DK_CHAIN_U2, &Derived::u2, ON_CHAIN_WINO}, {C2_28B, DK_CHAIN_U2, &Derived::u2, ON_CHAIN_WINO}, {C2_28C, DK_CHAIN_U2, &Derived::u2, ON_CHAIN_WINO},
    // chain_split.hip: c1, c2, c3 of the three chains, and the branch 1x1 that chain 28a runs on its pre-ReLU input
    {C1_28A, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN, 0, 256}, {C2_28A, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN}, {C3_28A, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN},
    {CB_28A, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN},
    {C1_28B, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN}, {C2_28B, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN}, {C3_28B, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN},
    {C1_28C, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN}, {C2_28C, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN}, {C3_28C, DK_PLANES, &Derived::planes, ON_SPLIT_CHAIN},
    // the 1x1 convs inside wino_mid
    {C1_14A, DK_PLANES, &Derived::planes, ON_SPLIT_MID}, {C1_7, DK_PLANES, &Derived::planes, ON_SPLIT_MID},
    // the 7-head behind the pooled sums of xv_7 (both arithmetic modes: the FC launch is fp32)
    {merged_slot(2), DK_HEAD_COMPOSED, &Derived::head, ON_POOL_FIRST7}};

// the [Co][K] weights behind a slot: a conv's (library K order, K = Ci k k) or a merged conv's ([Co][Ci_main | Ci_branch])
struct Matrix { const float* w; int Co, K; };
Matrix slot_matrix(const offk_handle* h, int slot) {
  if (slot < kNumConvs) return Matrix{h->conv_w[slot], kConvs[slot].Co, kConvs[slot].Ci * kConvs[slot].K * kConvs[slot].K};
  const MergedSpec& m = kMerged[slot - kNumConvs];
  return Matrix{h->merged_w[slot - kNumConvs], kConvs[m.main_id].Co, kConvs[m.main_id].Ci + kConvs[m.branch_id].Ci};
}
size_t derived_floats(const offk_handle* h, const DerivedRow& r) {
  switch (r.kind) {
    case DK_U_F43: case DK_U_POLY: case DK_U_F54: return (size_t)u_units(r.kind) * kConvs[r.slot].Co * kConvs[r.slot].Ci;
    case DK_CHAIN_U2: return (size_t)16 * 64 * 64;
    case DK_PLANES: { const Matrix m = slot_matrix(h, r.slot); return plane_floats((size_t)m.Co * (r.alloc_K ? r.alloc_K : m.K)); }
    case DK_U_PLANES: return plane_floats(u_elems(kConvs[r.slot]));
    case DK_HEAD_COMPOSED: return (size_t)h->cfg.num_classes * (slot_matrix(h, r.slot).K + 1);
  }
  return 0;
}
int pack_derived(offk_handle* h, const DerivedRow& r, hipStream_t st) {
  const Derived& d = h->derived[r.slot];
  switch (r.kind) {
    case DK_U_F43: case DK_U_POLY:
      HIP_TRY(h, wino_weight_launch(h->conv_w[r.slot], kConvs[r.slot].Co, kConvs[r.slot].Ci, wino_phases(kConvs[r.slot]), d.u, st));
      break;
    case DK_U_F54: HIP_TRY(h, wino7_weight_launch(h->conv_w[r.slot], kConvs[r.slot].Co, kConvs[r.slot].Ci, d.u, st)); break;
    case DK_CHAIN_U2: HIP_TRY(h, chain_wino_weight_launch(h->conv_w[r.slot], d.u2, st)); break;
    case DK_PLANES: {
      const Matrix m = slot_matrix(h, r.slot);
      HIP_TRY(h, wino_pack_split_launch(m.w, d.*r.image, m.Co, m.K, 1, st));
      break;
    }
    case DK_U_PLANES: {
      const ConvSpec& c = kConvs[r.slot];
      WinoGroup grp[4];
      const int ngrp = wino_conv_groups(c, 1, grp);
      for (int g = 0; g < ngrp; ++g)
        HIP_TRY(h, wino_pack_split_launch(d.u + grp[g].u_off, reinterpret_cast<char*>(d.u_planes) + grp[g].u_off * 6, c.Co, grp[g].kmul * c.Ci, grp[g].batch, st));
      break;
    }
    case DK_HEAD_COMPOSED: {
      const Matrix m = slot_matrix(h, r.slot);
      HIP_TRY(h, head_compose_launch(h->fc_w[0], h->fc_b[0], h->cfg.num_classes, m.w, h->merged_b[r.slot - kNumConvs], m.Co, m.K, d.head,
                                     d.head + (size_t)h->cfg.num_classes * m.K, st));
      break;
    }
  }
  return OFFK_OK;
}

// (re)build the merged weights after any conv weight or bias changed: [Co][Ci_main | Ci_branch], bias = b_main + b_branch
int finalize_merged(offk_handle* h, hipStream_t st) {
  if (!h->merged_dirty) return OFFK_OK;
  for (int m = 0; m < 3; ++m) {
    const ConvSpec& a = kConvs[kMerged[m].main_id];
    const ConvSpec& b = kConvs[kMerged[m].branch_id];
    const size_t K = (size_t)a.Ci + b.Ci;
    HIP_TRY(h, hipMemcpy2DAsync(h->merged_w[m], K * 4, h->conv_w[kMerged[m].main_id], (size_t)a.Ci * 4, (size_t)a.Ci * 4, a.Co, hipMemcpyDeviceToDevice, st));
    HIP_TRY(h, hipMemcpy2DAsync(h->merged_w[m] + a.Ci, K * 4, h->conv_w[kMerged[m].branch_id], (size_t)b.Ci * 4, (size_t)b.Ci * 4, a.Co, hipMemcpyDeviceToDevice, st));
    HIP_TRY(h, vec_add_launch(h->conv_b[kMerged[m].main_id], h->conv_b[kMerged[m].branch_id], h->merged_b[m], a.Co, st));
  }
  h->merged_dirty = false;
  return OFFK_OK;
}
// (re)pack every derived image after any of its sources changed (behind finalize_merged: the merged matrices and biases are sources too)
int finalize_derived(offk_handle* h, hipStream_t st) {
  if (!h->derived_dirty) return OFFK_OK;
  for (const DerivedRow& r : kDerived)
    if (h->derived[r.slot].*r.image) TRY(pack_derived(h, r, st));
  h->derived_dirty = false;
  return OFFK_OK;
}

// ---- the forward behind the units: one call's context, the launches of a conv on each path, one function per stage ----
constexpr int RI = OFFK_CONV_RELU_IN_, RP = OFFK_CONV_RELU_PRE_, RO = OFFK_CONV_RELU_POST_;
// a launch name in two pieces, put together only when the per-launch trace is on
int trace_mark(offk_handle* h, hipStream_t st, const char* key, const char* what) {
  return h->profiling != 2 ? OFFK_OK : trace_mark(h, st, (std::string(key) + what).c_str());
}
// the fields of a wino_mid launch (the order of offk_winograd_between's parameters); w1p: the plane image of w1, or nullptr
WinoMidArgs wino_mid_args(const float* M, const float* bias_in, int phases_in, int n_img, int Cin, float* x, int x_cs, int x_coff, const float* w1,
                          const float* b1, int Cmid, float* V, const void* w1p = nullptr) {
  WinoMidArgs m;
  m.M = M; m.bias_in = bias_in; m.phases_in = phases_in; m.x = x; m.x_cs = x_cs; m.x_coff = x_coff;
  m.w1 = w1; m.b1 = b1; m.Cin = Cin; m.Cmid = Cmid; m.n_img = n_img; m.V = V; m.w1p = w1p;
  return m;
}
// the view, weight and x_bytes fields of a chain launch; u2 and the plane images are the caller's
ChainArgs chain_args(const float* x, int x_cs, int x_coff, int n_img, int Cin, int relu_in, const float* w1, const float* b1, const float* w2,
                     const float* b2, const float* w3, const float* b3, int K3, const float* res, int res_cs, int res_coff, float* y, int y_cs,
                     int y_coff) {
  ChainArgs a{};
  a.x = x; a.x_cs = x_cs; a.x_coff = x_coff; a.Cin = Cin; a.relu_in = relu_in ? 1 : 0;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.w3 = w3; a.b3 = b3; a.K3 = K3;
  a.res = res; a.res_cs = res_cs; a.res_coff = res_coff; a.y = y; a.y_cs = y_cs; a.y_coff = y_coff;
  a.n_img = n_img; a.relu_out = 1;
  const unsigned long long xb = ((unsigned long long)n_img * 196 * x_cs - x_coff) * 4ull;
  a.x_bytes = xb < 0x7fffffffull ? (unsigned)xb : 0u;
  return a;
}

struct Fwd {
  offk_handle* h;
  hipStream_t s;
  void* ws;
  int n;                           // = P: every launch covers all P pairs (the buffers are pair-major)
  hipEvent_t* ev = nullptr;        // profiling == 1: the stage events of this call
  float *F14, *F7;                 // fusion_14 / fusion_7: written by the stage in front, read by the stage behind
  float *wino_V, *wino_M;          // Winograd domain: GEMM input and output (nullptr without the Winograd paths)
  float* splitk;                   // split-K partial slabs
  float *out7, *out14, *out28;     // the caller's (out28 nullptr: no 28-head)
  float *l7, *l14, *l28;           // where the heads write: those, or the per-pair regions consensus averages afterwards
  FcPooledJobs fcj{};              // the folded-pool FCs of the heads, launched together behind the last stage (fc_pooled_multi_kernel)
  bool wino, w7, mid, w5, chained, fold, fold14t, pool7;      // the paths of this call (init)

  float* reg(Region r) const { return region(h, ws, r); }

  // stage_only (offk_stage_tensors): a launch outside a forward -- it takes no stage events
  int init(offk_handle* handle, hipStream_t st, void* workspace, float* o7, float* o14, float* o28, bool stage_only = false) {
    h = handle; s = st; ws = workspace; n = h->P; out7 = o7; out14 = o14; out28 = o28;
    if (h->profiling == 1 && !stage_only) {
      const size_t per = OFFK_NUM_STAGES + 1;
      if ((h->ev_used + 1) * per > h->events.size() && h->events.size() < 4096 * per) {
        for (size_t i = 0; i < per; ++i) {
          hipEvent_t e;
          HIP_TRY(h, hipEventCreate(&e));
          h->events.push_back(e);
        }
      }
      if ((h->ev_used + 1) * per <= h->events.size()) ev = &h->events[h->ev_used++ * per];
    }
    wino = h->winograd;
    // the 7x7 / stride 2 conv in polyphase Winograd form
    // (from P = 12 pairs -- B = 2: 0.495 against 0.503 ms, B = 8: 0.813 against 0.874, B = 64: 3.88 against 4.24; B = 1: equal)
    w7 = h->derived[C_T28].u && wino && h->wino_7x7 && n >= h->wino7_min_p;
    mid = wino && h->wino_mid;
    // (from P = 40 pairs: below, its 132-K-tile GEMMs have too few row tiles to fill the chip and the split-K direct conv wins --
    // B = 1: 0.435 vs 0.50 ms, B = 4: 0.672 vs 0.695, B = 8: 0.892 vs 0.874, B = 12: 1.157 vs 1.12; OFFK_WINOGRAD_5X5=<pairs> moves the gate)
    w5 = wino && h->wino_5x5 && n >= h->wino5_min_p;
    // (from P = 72 pairs: a chain block walks its three convs alone -- 45 us per launch however few blocks there are; B = 8: three
    //  convs per chain 0.885 ms per forward against 0.90, B = 16: 1.37 against 1.345; OFFK_CHAIN=<pairs> moves the gate)
    chained = h->chain && n >= h->chain_min_p && (unsigned long long)n * 196 * 256 * 4ull < 0x7fffffffull;
    // (fold: the conv's epilogue also leaves per-slab column sums of its output: the head's average pool)
    auto generic = [](int cfg) { return cfg != 6 && cfg != 7 && cfg != 10; };      // the LDS-patch kernels have no pooling epilogue
    fold = h->fold_pool && generic(h->conv_cfg[C3_14B]) && generic(h->merged_cfg[2]);
    fold14t = wino && h->fold_pool;      // (the Winograd output transform of sum_14b leaves per-tile sums)
    pool7 = h->pool_first7 && mid && fold14t && h->derived[merged_slot(2)].head;      // (the 7-head from the per-tile sums of xv_7)
    F14 = reg(R_FUSION_14); F7 = reg(R_FUSION_7); splitk = reg(R_SPLITK);
    wino_V = wino ? reg(R_WINO_V) : nullptr;
    wino_M = wino ? reg(R_WINO_M) : nullptr;
    const bool cons = h->cfg.consensus == OFFK_CONSENSUS_AVG;
    l7 = cons ? reg(R_LOGIT_7) : out7; l14 = cons ? reg(R_LOGIT_14) : out14; l28 = cons ? reg(R_LOGIT_28) : out28;
    fcj.n_img = n; fcj.ncls = h->cfg.num_classes;
    return OFFK_OK;
  }

  // pool_part: the launch's epilogue also emits the pooled partial sums of a head there
  int conv_raw(const char* name, int Co, int Ci, int K, int stride, int pad, const float* w, const float* bias, int cfg, int sk, int H, View x,
               const float* res, int res_cs, int res_coff, int flags, float* y, int y_cs, int y_coff, const void* w_planes, float* pool_part) {
    if (w_planes && K == 1 && stride == 1 && pad == 0 && !res && !(flags & OFFK_CONV_RELU_IN_)) {
      // a 1x1 conv of a split-fp32 handle: wino_gemm_split.hip's kernel with its conv epilogue (bias, ReLU, the folded pool)
      WinoGemmArgs a{};
      a.x = x.p; a.w = w; a.y = y; a.M = n * H * H; a.Co = Co; a.ngroups = 1; a.g_batch[0] = 1; a.g_K[0] = Ci;
      a.w_planes = w_planes;
      a.epilogue = 1; a.x_rs = x.cs; a.x_coff = x.coff; a.y_rs = y_cs; a.y_coff = y_coff; a.bias = bias;
      a.relu = (flags & (OFFK_CONV_RELU_PRE_ | OFFK_CONV_RELU_POST_)) ? 1 : 0;
      a.pool_part = pool_part; a.pool_hw = pool_part ? H * H : 0;
      if (wino_gemm_split_supported(a)) {
        TRY(trace_mark(h, s, name));
        hipError_t e = wino_gemm_split_launch(a, s);
        if (e != hipSuccess) return fail_hip(h, e, name);
        return OFFK_OK;
      }
    }
    ConvDesc d = conv_desc(x.p, x.cs, x.coff, n, H, H, Ci, w, bias, Co, K, K, stride, pad, res, res_cs, res_coff, flags, y, y_cs, y_coff, cfg, sk,
                           splitk, h->splitk_floats, h->cfg.precision);
    d.pool_part = pool_part; d.pool_hw = pool_part ? H * H / (stride * stride) : 0;
    const char* why = nullptr;
    TRY(trace_mark(h, s, name));
    hipError_t e = conv2d_launch(d, s, &why);
    if (e != hipSuccess) return fail(h, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, std::string(name) + ": " + (why ? why : hipGetErrorString(e)));
    return OFFK_OK;
  }
  int conv(ConvId id, int H, View x, const float* res, int res_cs, int res_coff, int flags, float* y, int y_cs, int y_coff, float* pool_part = nullptr) {
    const ConvSpec& c = kConvs[id];
    return conv_raw(c.key, c.Co, c.Ci, c.K, c.stride, c.pad, h->conv_w[id], h->conv_b[id], h->conv_cfg[id], h->conv_splitk[id], H, x, res, res_cs,
                    res_coff, flags, y, y_cs, y_coff, h->derived[id].gemm_planes, pool_part);
  }
  // main 1x1 + branch 1x1 as ONE conv over the channel-concatenated input [t | x]
  int conv_merged(int m, int H, View x, int flags, float* y, int y_cs, int y_coff, float* pool_part = nullptr) {
    const Matrix w = slot_matrix(h, merged_slot(m));
    return conv_raw(kMerged[m].name, w.Co, w.K, 1, 1, 0, w.w, h->merged_b[m], h->merged_cfg[m], h->merged_sk[m], H, x, nullptr, 0, 0, flags, y, y_cs,
                    y_coff, h->derived[merged_slot(m)].gemm_planes, pool_part);
  }

  // A conv on its Winograd path in three steps: V = B^T x B (wino_V), M = V U per point (wino_M), y = epilogue(A^T M A).  winograd.hip: a
  // 3x3 / stride 1 conv on 7x7 maps (phases = 1), the 5x5 / stride 2 conv on 14x14 maps in polyphase form (phases = 4); winograd7.hip: the
  // 7x7 / stride 2 conv on 28x28 maps in polyphase form F(5x5, 4x4), nine tiles per image (no residual, no pooled sums).
  // (7x7: the input transform INSIDE the GEMM kernel was built and measured in round 4 -- tools/experiments/winograd7_fused.hip, out of the
  //  product build since round 5: 0.84 ms against 0.54 ms for these two launches; profiles/r04/wino7_fused_attempt.txt)
  int wino_in(ConvId id, View x) {
    const ConvSpec& c = kConvs[id];
    TRY(trace_mark(h, s, c.key, " [winograd: input transform]"));
    if (u_kind(c) == DK_U_F54) HIP_TRY(h, wino7_input_launch(x.p, x.cs, x.coff, n, c.Ci, wino_V, s));
    else HIP_TRY(h, wino_input_launch(x.p, x.cs, x.coff, n, c.Ci, wino_phases(c), wino_V, s));
    return OFFK_OK;
  }
  // the batched GEMMs: ONE launch, the K groups ride on gridDim.y (four launches left the short groups alone on the chip: slower than
  // not skipping their zero products)
  int wino_mm(ConvId id) {
    const ConvSpec& c = kConvs[id];
    const bool f54 = u_kind(c) == DK_U_F54;
    TRY(trace_mark(h, s, c.key, f54 ? " [winograd: 64 GEMMs]" : " [winograd: 121 GEMMs]"));
    const int rows = f54 ? kWino7Tiles * n : n;
    WinoGroup grp[4];
    const int ngrp = wino_conv_groups(c, rows, grp);
    const char* why = nullptr;
    hipError_t e = wino_gemms_launch(grp, ngrp, f54 ? kWino7Points : kWinoPoints, rows, c.Ci, c.Co, wino_V, h->derived[id].u, wino_M, h->wino_gemm, s, &why,
                                     h->derived[id].u_planes);
    if (e != hipSuccess) return fail(h, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, std::string(c.key) + " (winograd): " + (why ? why : hipGetErrorString(e)));
    return OFFK_OK;
  }
  int wino_out(ConvId id, const float* res, int res_cs, int res_coff, int flags, float* y, int y_cs, int y_coff, float* pool_t, int pool_cs = 0) {
    const ConvSpec& c = kConvs[id];
    TRY(trace_mark(h, s, c.key, " [winograd: output transform]"));
    if (u_kind(c) == DK_U_F54) HIP_TRY(h, wino7_output_launch(wino_M, n, c.Co, h->conv_b[id], flags, y, y_cs, y_coff, s));
    else HIP_TRY(h, wino_output_launch(wino_M, n, c.Co, wino_phases(c), h->conv_b[id], res, res_cs, res_coff, flags, y, y_cs, y_coff, pool_t, s, pool_cs, 0));
    return OFFK_OK;
  }
  int wino_conv(ConvId id, View x, const float* res, int res_cs, int res_coff, int flags, float* y, int y_cs, int y_coff, float* pool_t) {
    TRY(wino_in(id, x));
    TRY(wino_mm(id));
    return wino_out(id, res, res_cs, res_coff, flags, y, y_cs, y_coff, pool_t);
  }
  // What sits between two convs on that path, in ONE launch (wino_mid.hip): the output transform (+ bias, ReLU) of conv `a` from
  // wino_M, optionally the 1x1 conv `c1` (+ bias, ReLU; kNumConvs: none), the input transform of the conv behind into wino_V.  xa: where
  // the activation of conv `a` is ALSO stored (the merged convs read x1 / x2 from there later); nullptr: nowhere.  pool_t: the per-tile sums
  // of that activation go to rows of xa_cs floats there, at xa_coff as well.
  int wino_between(ConvId a, ConvId c1, float* xa, int xa_cs, int xa_coff, const char* name, float* pool_t = nullptr) {
    const bool has = c1 != kNumConvs;
    WinoMidArgs m = wino_mid_args(wino_M, h->conv_b[a], wino_phases(kConvs[a]), n, kConvs[a].Co, xa, xa_cs, xa_coff, has ? h->conv_w[c1] : nullptr,
                                        has ? h->conv_b[c1] : nullptr, kConvs[has ? c1 : a].Co, wino_V, has ? h->derived[c1].planes : nullptr);
    m.pool_part = pool_t; m.pool_cs = xa_cs; m.pool_coff = xa_coff;
    TRY(trace_mark(h, s, name));
    HIP_TRY(h, wino_mid_launch(m, s));
    return OFFK_OK;
  }
  // x = relu(conv k x k (F)) -> c1 (1x1) -> c2 (3x3), the head of fusion@14 and fusion@7: xx = [c2's output | x] per pixel, t: c1's output.
  // wino_t: `ct` on its Winograd path; with wino_mid the 1x1 conv then sits between the two Winograd GEMM launches.
  // pool_t (that form only): the per-tile sums of xx, [4 n][cs], from the two launches that store xx.
  int conv_t_c1_c2(ConvId ct, bool wino_t, int H, View F, ConvId c1, ConvId c2, float* xx, int cs, float* t, const char* between,
                   float* pool_t = nullptr) {
    const int half = cs / 2;
    if (wino_t && mid) {
      TRY(wino_in(ct, F));
      TRY(wino_mm(ct));
      TRY(wino_between(ct, c1, xx, cs, half, between, pool_t));
      TRY(wino_mm(c2));
      return wino_out(c2, nullptr, 0, 0, RP, xx, cs, 0, pool_t, pool_t ? cs : 0);
    }
    if (wino_t) TRY(wino_conv(ct, F, nullptr, 0, 0, RP, xx, cs, half, nullptr));
    else TRY(conv(ct, H, F, nullptr, 0, 0, RP, xx, cs, half));
    TRY(conv(c1, 7, View{xx, cs, half}, nullptr, 0, 0, RP, t, half, 0));
    if (wino) return wino_conv(c2, View{t, half, 0}, nullptr, 0, 0, RP, xx, cs, 0, nullptr);
    return conv(c2, 7, View{t, half, 0}, nullptr, 0, 0, RP, xx, cs, 0);
  }

  // 1x1 -> 3x3 -> 1x1 (+ residual) as ONE launch per chain (a block owns half an image, t1 / t2 stay in LDS).  m >= 0: chain 28a, whose c3
  // is summed with the branch 1x1 kMerged[m] on the chain input -- merged into c3's K (K3 = 128, the fp32 kernel), or, split_branch, as
  // a 1x1 conv of its own inside chain_split.hip's kernel (c3 with K3 = 64; its output passes through y as the chain's residual).
  int chain(const char* name, View x, int Cin, int relu_in, ConvId c1, ConvId c2, ConvId c3, int m, bool split_branch, const float* res, float* y, int y_cs, int y_coff) {
    const bool merged = m >= 0 && !split_branch;
    ChainArgs a = chain_args(x.p, x.cs, x.coff, n, Cin, relu_in, h->conv_w[c1], h->conv_b[c1], h->conv_w[c2], h->conv_b[c2],
                             merged ? h->merged_w[m] : h->conv_w[c3], merged ? h->merged_b[m] : h->conv_b[c3], merged ? 128 : 64, res, 256, 0, y, y_cs, y_coff);
    a.u2 = h->derived[c2].u2;
    a.w1p = h->derived[c1].planes; a.w2p = h->derived[c2].planes; a.w3p = h->derived[c3].planes;
    if (split_branch) { a.wbp = h->derived[kMerged[m].branch_id].planes; a.bbr = h->conv_b[kMerged[m].branch_id]; }
    TRY(trace_mark(h, s, name));
    const char* why = nullptr;
    hipError_t e = chain14_split_supported(a) ? chain14_split_launch(a, s, &why) : chain14_launch(a, s, &why);
    if (e != hipSuccess) return fail(h, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, std::string(name) + ": " + (why ? why : hipGetErrorString(e)));
    return OFFK_OK;
  }

  // head k (kHeads order) from the pooled partial sums `part` its producing launch left (heads.hip: fc_pooled), or -- part == nullptr: the
  // paths that cannot fold the pool into that launch (LDS-patch tiles, OFFK_FOLD_POOL=0) -- pool_kernel + fc_kernel on its output x
  int head(int k, float* logits, const float* part, int tiles, const float* x, int x_cs, int x_coff, int Hh, int maxpool, Region pooled_region) {
    const int C = kHeads[k].C;
    if (part) { fcj.job[fcj.njobs++] = FcPooledJob{part, 49, tiles, C, h->fc_w[k], h->fc_b[k], logits}; return OFFK_OK; }
    float* pooled = reg(pooled_region);
    TRY(trace_mark(h, s, k == 0 ? "head_7 (pool + fc)" : k == 1 ? "head_28 (pool + fc)" : "head_14 (pool + fc)"));
    hipError_t e = pool_launch(x, x_cs, x_coff, n, Hh, Hh, C, maxpool, pooled, s);
    if (e == hipSuccess) e = fc_launch(pooled, n, C, h->fc_w[k], h->fc_b[k], h->cfg.num_classes, logits, s);
    if (e != hipSuccess) return fail_hip(h, e, "head");
    return OFFK_OK;
  }

  int units(const offk_feat_parts feats[], int feat_dtype, bool cl) {
    if (cl) return run_off_units_fused(h, s, feats, ws, ev, feat_dtype, true);       // (check_feat: fused_units, whatever cfg.feat_layout)
    if (h->fused_units && h->cfg.feat_layout != OFFK_FEAT_NHWC) return run_off_units_fused(h, s, feats, ws, ev, feat_dtype);
    return run_off_units(h, s, feats, ws, ev, h->cfg.feat_layout == OFFK_FEAT_NHWC);
  }

  // ---- fusion @28 -> 14x14 (RGB_OFF.py:655-685) and the 28-head (:782-787) ----
  int fusion28() {
    float *F28 = reg(R_FUSION_28), *xt = reg(R_XT_28), *t1 = reg(R_T1_28), *sa = reg(R_SA_28), *sb = reg(R_SB_28);
    // xt = [t2 | x0] per pixel: c3(t2) + branch(x0) (:663-666) is then ONE 1x1 conv over 128 channels
    // :657 x0, pre-ReLU kept for the branch
    if (w7) TRY(wino_conv(C_T28, View{F28, 320, 0}, nullptr, 0, 0, 0, xt, 128, 64, nullptr));
    else TRY(conv(C_T28, 28, View{F28, 320, 0}, nullptr, 0, 0, 0, xt, 128, 64));
    if (chained) {
      // split-fp32 (chain_split.hip, BR form): the branch 1x1 on the pre-ReLU chain input inside the kernel -- RGB_OFF.py:663-667; in the
      // fp32 kernel the branch is merged into c3's K
      TRY(chain("chain_28a = motion_conv1_trans_28a + motion_conv2_trans_28a + merged_28a", View{xt, 128, 64}, 64, 1, C1_28A, C2_28A, C3_28A, 0,
                h->derived[CB_28A].planes != nullptr, nullptr, sa, 256, 0));                                                       // :658-667
      TRY(chain("chain_28b = motion_conv1_trans_28b + motion_conv2_trans_28b + motion_conv3_trans_28b", View{sa, 256, 0}, 256, 0, C1_28B, C2_28B, C3_28B,
                -1, false, sa, sb, 256, 0));                                                                                       // :670-676
      TRY(chain("chain_28c = motion_conv1_trans_28c + motion_conv2_trans_28c + motion_conv3_trans_28c", View{sb, 256, 0}, 256, 0, C1_28C, C2_28C, C3_28C,
                -1, false, sb, F14, 1056, 800));                                                                    // :679-685 -> cat at :760
    } else {
      TRY(conv(C1_28A, 14, View{xt, 128, 64}, nullptr, 0, 0, RI | RP, t1, 64, 0));            // :658-660
      TRY(conv(C2_28A, 14, View{t1, 64, 0}, nullptr, 0, 0, RP, xt, 128, 0));                  // :661-662 t2
      TRY(conv_merged(0, 14, View{xt, 128, 0}, RO, sa, 256, 0));                               // :663-667
      TRY(conv(C1_28B, 14, View{sa, 256, 0}, nullptr, 0, 0, RP, t1, 64, 0));                  // :670-671
      TRY(conv(C2_28B, 14, View{t1, 64, 0}, nullptr, 0, 0, RP, xt, 128, 0));                  // :672-673
      TRY(conv(C3_28B, 14, View{xt, 128, 0}, sa, 256, 0, RO, sb, 256, 0));                     // :674-676
      TRY(conv(C1_28C, 14, View{sb, 256, 0}, nullptr, 0, 0, RP, t1, 64, 0));                  // :679-680
      TRY(conv(C2_28C, 14, View{t1, 64, 0}, nullptr, 0, 0, RP, xt, 128, 0));                  // :681-682
      TRY(conv(C3_28C, 14, View{xt, 128, 0}, sb, 256, 0, RO, F14, 1056, 800));                 // :683-685 -> cat at :760
    }
    if (ev) HIP_TRY(h, hipEventRecord(ev[3], s));
    if (!out28) return OFFK_OK;
    float* pp = nullptr;     // the 28-head only reads sum_28c: pool-row partial sums + the FC as an MFMA GEMM instead of pool_kernel + fc_kernel
    if (h->fold_pool) {
      pp = reg(R_POOLPART_28);
      TRY(trace_mark(h, s, "head_28 (max pool rows)"));
      HIP_TRY(h, maxpool_rows_launch(F14, 1056, 800, n, 14, 14, 256, pp, s));
    }
    return head(1, l28, pp, 1, F14, 1056, 800, 14, 1, R_POOLED_28);
  }

  // ---- fusion @14 -> 7x7 (RGB_OFF.py:759-780) and the 14-head (:789-793) ----
  int fusion14() {
    float *xu = reg(R_XU_14), *u1 = reg(R_U1_14), *s14 = reg(R_SA_14);                           // xu = [u2 | x1]
    TRY(conv_t_c1_c2(C_T14, w5, 14, View{F14, 1056, 0}, C1_14A, C2_14A, xu, 256, u1,                // :762-767
                     "motion_conv_trans_14 out + motion_conv1_trans_14a + motion_conv2_trans_14a in [winograd: between]"));
    TRY(conv_merged(1, 7, View{xu, 256, 0}, RO, s14, 512, 0));                                   // :768-771
    TRY(conv(C1_14B, 7, View{s14, 512, 0}, nullptr, 0, 0, RP, u1, 128, 0));                     // :773-774
    // the 14-head's average pool of sum_14b: per-tile sums from the Winograd output transform (fold14t), or per-slab column sums from
    // the direct conv's epilogue (fold)
    float* pp14t = fold14t ? reg(R_POOLPART_14T) : nullptr;
    float* pp14 = !wino && fold ? reg(R_POOLPART_14) : nullptr;
    if (mid) {            // :775-780: c2_14b's output feeds c3_14b alone -- output transform, ReLU and input transform in one launch
      TRY(wino_in(C2_14B, View{u1, 128, 0}));
      TRY(wino_mm(C2_14B));
      TRY(wino_between(C2_14B, kNumConvs, nullptr, 0, 0, "motion_conv2_trans_14b out + motion_conv3_trans_14b in [winograd: between]"));
      TRY(wino_mm(C3_14B));
      TRY(wino_out(C3_14B, s14, 512, 0, RP | RO, F7, 832, 320, pp14t));                          // :777-780 -> cat at :832
    } else if (wino) {
      TRY(wino_conv(C2_14B, View{u1, 128, 0}, nullptr, 0, 0, RP, xu, 256, 0, nullptr));          // :775-776
      TRY(wino_conv(C3_14B, View{xu, 256, 0}, s14, 512, 0, RP | RO, F7, 832, 320, pp14t));       // :777-780 -> cat at :832
    } else {
      TRY(conv(C2_14B, 7, View{u1, 128, 0}, nullptr, 0, 0, RP, xu, 256, 0));                     // :775-776
      TRY(conv(C3_14B, 7, View{xu, 256, 0}, s14, 512, 0, RP | RO, F7, 832, 320, pp14));          // :777-780 -> cat at :832
    }
    if (ev) HIP_TRY(h, hipEventRecord(ev[4], s));
    return head(2, l14, pp14t ? pp14t : pp14, pp14t ? 1 : 0, F7, 832, 320, 7, 0, R_POOLED_14);      // only reads sum_14b
  }

  // ---- fusion @7 (RGB_OFF.py:831-841) and the 7-head (:843-847) ----
  int fusion7() {
    float *xv = reg(R_XV_7), *v1 = reg(R_V1_7), *s7 = reg(R_SUM_7);                              // xv = [v2 | x2]
    float* pp7t = pool7 ? reg(R_POOLPART_7T) : nullptr;
    TRY(conv_t_c1_c2(C_T7, wino, 7, View{F7, 832, 0}, C1_7, C2_7, xv, 512, v1,                      // :833-838
                     "motion_conv_trans out + motion_conv1_trans + motion_conv2_trans in [winograd: between]", pp7t));
    if (pool7) {
      // :839-847 is linear from xv to the logits (no ReLU on motion_sum, which feeds nothing else): the average pool first, then ONE FC
      // with the composed weights in the heads' launch; sum_7 itself is left to offk_stage_tensors
      const float* wc = h->derived[merged_slot(2)].head;
      fcj.job[fcj.njobs++] = FcPooledJob{pp7t, 49, 1, 512, wc, wc + (size_t)h->cfg.num_classes * 512, l7};
      h->sum7_pending = true;
      if (ev) HIP_TRY(h, hipEventRecord(ev[5], s));
      return OFFK_OK;
    }
    float* pp7 = fold ? reg(R_POOLPART_7) : nullptr;      // the 7-head's average pool in the merged conv's epilogue
    TRY(merged7());
    if (ev) HIP_TRY(h, hipEventRecord(ev[5], s));
    return head(0, l7, pp7, 0, s7, 1024, 0, 7, 0, R_POOLED_7);
  }
  // :839-841 (no ReLU): sum_7 from xv_7, and with `fold` the pooled sums of the 7-head in its epilogue (fusion7; offk_stage_tensors)
  int merged7() { return conv_merged(2, 7, View{reg(R_XV_7), 512, 0}, 0, reg(R_SUM_7), 1024, 0, fold ? reg(R_POOLPART_7) : nullptr); }

  // ---- the folded-pool FCs of all heads in one launch, segment consensus (Flow_OFF.py:874-876) ----
  int heads() {
    if (fcj.njobs > 0) {
      TRY(trace_mark(h, s, "heads (fc on folded pools, one launch)"));
      HIP_TRY(h, fc_pooled_multi_launch(fcj, s));
    }
    if (h->cfg.consensus == OFFK_CONSENSUS_AVG) {
      TRY(trace_mark(h, s, "consensus (K6)"));
      const float* const cx[3] = {l7, l14, out28 ? l28 : l14};                                    // one launch
      float* const co[3] = {out7, out14, out28 ? out28 : out14};
      HIP_TRY(h, consensus_multi_launch(cx, co, out28 ? 3 : 2, h->cfg.batch, h->cfg.length - 1, h->cfg.num_classes, s));
    }
    if (ev) HIP_TRY(h, hipEventRecord(ev[6], s));
    return trace_mark(h, s, nullptr);
  }
};
}  // namespace

extern "C" {

int offk_abi_version(void) { return OFFK_ABI_VERSION; }

const char* offk_last_error(const offk_handle* h) { return h ? h->err.c_str() : g_err.c_str(); }

int offk_create(const offk_config* cfg, offk_handle** out) {
  if (!cfg || !out) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: null argument");
  *out = nullptr;
  if (cfg->batch < 1 || cfg->length < 2) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: need batch >= 1 and length >= 2");
  if (cfg->variant != OFFK_VARIANT_RGB_LEARNED_DW && cfg->variant != OFFK_VARIANT_DIAG_SOBEL) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: bad variant");
  if (cfg->slice_mode != OFFK_SLICE_REFERENCE_FLAT && cfg->slice_mode != OFFK_SLICE_PER_CLIP) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: bad slice_mode");
  if (cfg->consensus != OFFK_CONSENSUS_NONE && cfg->consensus != OFFK_CONSENSUS_AVG) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: bad consensus");
  if (cfg->feat_layout != OFFK_FEAT_NCHW && cfg->feat_layout != OFFK_FEAT_NHWC) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: bad feat_layout");
  if (cfg->precision != OFFK_PRECISION_FP32 && cfg->precision != OFFK_PRECISION_F32SPLIT)
    return fail(nullptr, OFFK_ERR_INVALID, "offk_create: bad precision (0 = fp32, 2 = f32split; 1 was the two-plane bf16x3 mode, retired in ABI v9)");
  if (cfg->num_classes < 1 || cfg->num_classes > 4096) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: bad num_classes");
  if ((long long)cfg->batch * cfg->length * 784 * 320 > 0x7fffffffLL) return fail(nullptr, OFFK_ERR_INVALID, "offk_create: batch*length too large for one call; shard the clips");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || cfg->device < 0 || cfg->device >= ndev)
    return fail(nullptr, OFFK_ERR_NO_DEVICE, "offk_create: HIP device not available");
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, cfg->device) != hipSuccess || !strstr(prop.gcnArchName, "gfx950"))
    return fail(nullptr, OFFK_ERR_NO_DEVICE, "offk_create: device is not gfx950 (MI355X); this library has no other code path");

  offk_handle* h = new offk_handle();
  h->cfg = *cfg;
  offk_config cfg_in = *cfg;
  if (cfg_in.precision == OFFK_PRECISION_F32SPLIT) { h->f32split = true; h->cfg.precision = cfg_in.precision = OFFK_PRECISION_FP32; }
  cfg = &cfg_in;        // below: the library's own view (split-fp32 = the fp32 plans and buffers + the split kernels' weight images)
  h->N = cfg->batch * cfg->length;
  h->P = cfg->batch * (cfg->length - 1);
  for (int c = 0; c < kNumConvs; ++c) {
    const int (*tab)[2] = h->P == 240 ? kTunedP240 : nullptr;      // (P = 384: the automatic plans, see above)
    h->conv_cfg[c] = tab ? tab[c][0] : -1;
    h->conv_splitk[c] = tab ? tab[c][1] : 0;
  }
  for (int m = 0; m < 3; ++m) {
    const int (*mp)[2] = kMergedPlan[h->P == 240];
    h->merged_cfg[m] = mp[m][0];
    h->merged_sk[m] = mp[m][1];
  }
  DeviceGuard guard(cfg->device);
  int rc = OFFK_OK;
  for (int s = 0; s < kNumSites && rc == OFFK_OK; ++s) {
    const int C = kSites[s].C;
    const bool learned_dw = cfg->variant == OFFK_VARIANT_RGB_LEARNED_DW;
    rc = dev_alloc(h, &h->pw_w[s], (size_t)kUnitCh * C);
    if (rc == OFFK_OK && cfg->precision == OFFK_PRECISION_FP32) rc = dev_alloc(h, &h->pw_wt16[s], (size_t)kUnitCh * C);
    if (rc == OFFK_OK && h->f32split) rc = dev_alloc(h, &h->pw_wt16s[s], (size_t)kUnitCh * C * 3 / 2);
    if (rc == OFFK_OK) rc = dev_alloc(h, &h->pw_b[s], kUnitCh);
    if (rc == OFFK_OK && learned_dw) rc = dev_alloc(h, &h->dw_w[s], 9 * kDownCh);
    if (rc == OFFK_OK && learned_dw) rc = dev_alloc(h, &h->dw_b[s], kDownCh);
    for (const UnitParamSpec& p : kUnitParams) {
      if (rc != OFFK_OK || (p.dw && !learned_dw)) continue;
      UnitParam& u = h->unit[s][p.kind];
      u.own = (h->*p.buf)[s] + p.buf_row * (unit_count(p, C) / p.shape[0]);
      u.slot = (int)h->slots.size();
      add_slot(h, std::string(p.prefix) + kSites[s].name + p.suffix, unit_shape(p, C), p.kind, s);
    }
  }
  if (cfg->variant == OFFK_VARIANT_DIAG_SOBEL && rc == OFFK_OK) {
    h->sobel_slot = (int)h->slots.size();
    add_slot(h, kSobelKey, {kDownCh, 1, 3, 3}, SK_SOBEL, 0);
    rc = dev_alloc(h, &h->sobel_w, 9 * kDownCh);
  }
  for (int c = 0; c < kNumConvs && rc == OFFK_OK; ++c) {
    const ConvSpec& cs = kConvs[c];
    add_slot(h, std::string(cs.key) + ".weight", {cs.Co, cs.Ci, cs.K, cs.K}, SK_CONV_W, c);
    add_slot(h, std::string(cs.key) + ".bias", {cs.Co}, SK_CONV_B, c);
    rc = dev_alloc(h, &h->conv_w[c], (size_t)cs.Co * cs.Ci * cs.K * cs.K);
    if (rc == OFFK_OK) rc = dev_alloc(h, &h->conv_b[c], cs.Co);
  }
  for (int m = 0; m < 3 && rc == OFFK_OK; ++m) {
    const ConvSpec& a = kConvs[kMerged[m].main_id];
    const ConvSpec& b = kConvs[kMerged[m].branch_id];
    const size_t n = (size_t)a.Co * (a.Ci + b.Ci);
    rc = dev_alloc(h, &h->merged_w[m], n);
    if (rc == OFFK_OK) rc = dev_alloc(h, &h->merged_b[m], a.Co);
  }
  for (int k = 0; k < 3 && rc == OFFK_OK; ++k) {
    add_slot(h, std::string(kHeads[k].key) + ".weight", {cfg->num_classes, kHeads[k].C}, SK_FC_W, k);
    add_slot(h, std::string(kHeads[k].key) + ".bias", {cfg->num_classes}, SK_FC_B, k);
    rc = dev_alloc(h, &h->fc_w[k], (size_t)cfg->num_classes * kHeads[k].C);
    if (rc == OFFK_OK) rc = dev_alloc(h, &h->fc_b[k], cfg->num_classes);

  }
  if (rc == OFFK_OK) rc = dev_alloc(h, &h->zero_page, 64);
  for (int s = 0; s < kNumSites && rc == OFFK_OK; ++s) rc = dev_alloc(h, &h->dx_split_w[s], units_dx_split_image_bytes(kSites[s].C) / sizeof(float));
  for (int s = 0; s < kNumSites && rc == OFFK_OK; ++s) rc = dev_alloc(h, &h->fwd_split_w[s], units_fwd_split_image_bytes(kSites[s].C) / sizeof(float));
  // The path switches of the product library, all read HERE and nowhere else (INTEGRATION.md lists them): each names one
  // algorithm choice of the exact-fp32 forward; "0" = off, a number > 1 = use it from that many frame pairs P = B (L - 1).
  //   OFFK_FUSED_UNITS   K1 fused with the temporal difference (pw_tdiff.hip); 0: K1 + K2 (what training always runs)
  //   OFFK_WINOGRAD      Winograd forms of the k x k fusion convs (winograd.hip, winograd7.hip); 0: direct implicit GEMMs everywhere
  //   OFFK_WINOGRAD_5X5  ... of the 5x5 / stride 2 conv (default: from P = 40)     OFFK_WINOGRAD_7X7  ... of the 7x7 / stride 2 conv (from P = 12)
  //   OFFK_CHAIN         one launch per bottleneck chain of fusion@28 (chain_fused.hip; from P = 72)
  //   OFFK_FOLD_POOL     7- / 14-head average pools taken in the producing conv's epilogue; 0: pool + fc kernels
  //   OFFK_WINO_MID      what sits between two Winograd convs on 7x7 maps (output transform, 1x1 conv, input transform) in one launch
  //                      (wino_mid.hip); 0: three launches
  //   OFFK_CHAIN_WINO    the 3x3 conv inside a bottleneck chain in Winograd F(2x2, 3x3) form (chain_fused.hip); 0: direct (also with OFFK_WINOGRAD=0)
  //   OFFK_POOL_FIRST_7  the 7-head from pooled sums of xv_7 and composed weights, merged_7 only on demand (offk_stage_tensors; from P = 96;
  //                      needs OFFK_WINOGRAD, OFFK_WINO_MID and OFFK_FOLD_POOL on)
  //   OFFK_WINO_GEMM     the batched GEMMs of a Winograd conv as one persistent launch (wino_gemm.hip); 0: one block of the generic 1x1 kernel per
  //                      tile (bit-identical).  The handle-less stage entry points read it once per process.
  h->fused_units = path_switch("OFFK_FUSED_UNITS");
  h->split_chain = h->f32split && path_switch("OFFK_SPLIT_CHAIN");
  h->split_mid = h->f32split && path_switch("OFFK_SPLIT_MID");
  {
    int from = 0;
    h->chain = path_switch("OFFK_CHAIN", &from);
    if (from) h->chain_min_p = from;
    // split-fp32 handles: chain14_split_kernel from the first pair on (a block of it alone on a CU is ~25 us per chain where the fp32 kernel's
    // sixteen phases are 45 us: B = 1 .. 4 0.432 / 0.482 / 0.565 -> 0.425 / 0.477 / 0.555 ms, B = 8 level; profiles/r06/small_batch_gates.txt)
    else if (h->split_chain) h->chain_min_p = 1;
  }
  h->fold_pool = path_switch("OFFK_FOLD_POOL");
  h->wino_mid = path_switch("OFFK_WINO_MID");
  h->wino_gemm = path_switch("OFFK_WINO_GEMM");
  h->winograd = path_switch("OFFK_WINOGRAD") && cfg->precision == OFFK_PRECISION_FP32;
  h->wino_5x5 = path_switch("OFFK_WINOGRAD_5X5", &h->wino5_min_p);
  h->wino_7x7 = path_switch("OFFK_WINOGRAD_7X7", &h->wino7_min_p);
  h->split_gemm = h->winograd && h->f32split && path_switch("OFFK_SPLIT_GEMM");
#ifdef OFFK_TUNING_KNOBS
  { const char* e = getenv("OFFK_SPLIT_GEMM_SKIP"); if (e) h->split_gemm_skip = atoi(e); }
#endif
  h->chain_wino = h->winograd && h->chain && path_switch("OFFK_CHAIN_WINO");
  {
    // (from P = 96 pairs, B = 16 x L = 7: below, the recorded launch plans and the head tests read the device's own sum_7 after every
    //  forward, and whether the path pays there is not measured; OFFK_POOL_FIRST_7=<pairs> moves the gate)
    int gate = 96;
    const bool on = path_switch("OFFK_POOL_FIRST_7", &gate);
    h->pool_first7 = on && h->winograd && h->wino_mid && h->fold_pool && h->P >= gate;
  }
  for (const DerivedRow& r : kDerived)
    if (rc == OFFK_OK && derived_exists(h, r)) rc = dev_alloc(h, &(h->derived[r.slot].*r.image), derived_floats(h, r));
  if (rc != OFFK_OK) {
    g_err = h->err;
    offk_destroy(h);
    return rc;
  }
  plan_workspace(h);
  *out = h;
  return OFFK_OK;
}

int offk_destroy(offk_handle* h) {
  if (!h) return OFFK_OK;
  DeviceGuard guard(h->cfg.device);
  for (hipEvent_t e : h->events) (void)hipEventDestroy(e);
  for (hipEvent_t e : h->tr_events) (void)hipEventDestroy(e);
  for (void* p : h->allocs) (void)hipFree(p);
  delete h;
  return OFFK_OK;
}

int offk_set_weight(offk_handle* h, const char* key, const float* data, const int64_t* shape, int ndim) {
  if (!h || !key || !data || !shape) return fail(h, OFFK_ERR_INVALID, "offk_set_weight: null argument");
  std::string k(key);
  if (k.compare(0, 7, "module.") == 0) k = k.substr(7);
  auto it = h->index.find(k);
  if (it == h->index.end()) return fail(h, OFFK_ERR_UNKNOWN_KEY, "offk_set_weight: not an OFF sub-network key for this variant: " + k);
  Slot& s = h->slots[it->second];
  bool ok = ndim == (int)s.shape.size();
  size_t n = 1;
  for (int i = 0; ok && i < ndim; ++i) { ok = shape[i] == s.shape[i]; n *= (size_t)s.shape[i]; }
  if (!ok) return fail(h, OFFK_ERR_INVALID, "offk_set_weight: shape mismatch for " + k);
  DeviceGuard guard(h->cfg.device);
  // A load-time call, blocking by contract: wait for everything enqueued on the device first -- a kernel that still reads
  // the copy being replaced, or (device source) the kernel that is still producing `data` on some non-blocking stream.
  // Parameters that change every step are not pushed through here: offk_bind_weight.
  HIP_TRY(h, hipDeviceSynchronize());
  const size_t bytes = n * sizeof(float);
  auto copy = [&](float* dst) -> int {
    HIP_TRY(h, hipMemcpy(dst, data, bytes, hipMemcpyDefault));
    return OFFK_OK;
  };
  auto staged = [&](auto&& pack) -> int {   // copy to a temp device buffer, then run a packing kernel
    void* tmp = nullptr;
    HIP_TRY(h, hipMalloc(&tmp, bytes));
    hipError_t e = hipMemcpy(tmp, data, bytes, hipMemcpyDefault);
    if (e == hipSuccess) e = pack(static_cast<const float*>(tmp));
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail_hip(h, e, "offk_set_weight pack");
    return OFFK_OK;
  };
  int rc = OFFK_OK;
  const int i = s.idx;
  UnitParam* unit = s.kind < kNumUnitParams ? &h->unit[i][s.kind] : nullptr;
  switch (s.kind) {
    case SK_GEN_W: case SK_GEN_B: case SK_DOWN_W: case SK_DOWN_B: case SK_DW_W: case SK_DW_B:
      if (kUnitParams[s.kind].repack_dw) rc = staged([&](const float* t) { return repack_dw_launch(t, unit->own, nullptr); });
      else rc = copy(unit->own);
      break;
    case SK_SOBEL: {
      rc = staged([&](const float* t) { return repack_dw_launch(t, h->sobel_w, nullptr); });
      // frozen parameter (util.py:72), but it travels in checkpoints: take the four-tap path only for weights that
      // really are zero at the corners and the centre
      std::vector<float> host(n);
      if (rc == OFFK_OK && hipMemcpy(host.data(), data, bytes, hipMemcpyDefault) == hipSuccess) {
        bool four = true;
        for (int c = 0; c < kDownCh && four; ++c)
          for (int tap : {0, 2, 4, 6, 8}) four = four && host[(size_t)c * 9 + tap] == 0.f;
        h->sobel_taps4 = four;
      } else {
        h->sobel_taps4 = false;
      }
      break;
    }
    case SK_CONV_W:
      if (kConvs[i].K == 1) rc = copy(h->conv_w[i]);
      else rc = staged([&](const float* t) { return pack_conv_weight_launch(t, kConvs[i].Co, kConvs[i].Ci, kConvs[i].K, kConvs[i].K, h->conv_w[i], nullptr); });
      break;
    case SK_CONV_B: rc = copy(h->conv_b[i]); break;
    case SK_FC_W: rc = copy(h->fc_w[i]); break;
    case SK_FC_B: rc = copy(h->fc_b[i]); break;
  }
  if (rc == OFFK_OK) {
    s.set = true;
    if (unit) unit->bound = nullptr;       // an explicit copy replaces an earlier in-place binding of the same key
  }
  if (s.kind == SK_CONV_W || s.kind == SK_CONV_B) h->merged_dirty = true;
  if (s.kind == SK_CONV_W) h->derived_dirty = true;
  // the composed 7-head also follows the two biases of merged_7 and the head's own weight and bias
  if (h->derived[merged_slot(2)].head && ((s.kind == SK_CONV_B && (i == C3_7 || i == CB_7)) || ((s.kind == SK_FC_W || s.kind == SK_FC_B) && i == 0)))
    h->derived_dirty = true;
  if (s.kind == SK_GEN_W || s.kind == SK_DOWN_W) h->pw_dirty = true;
  return rc;
}

int offk_bind_weight(offk_handle* h, const char* key, const float* device_data, const int64_t* shape, int ndim) {
  if (!h || !key || !device_data || !shape) return fail(h, OFFK_ERR_INVALID, "offk_bind_weight: null argument");
  std::string k(key);
  if (k.compare(0, 7, "module.") == 0) k = k.substr(7);
  auto it = h->index.find(k);
  if (it == h->index.end()) return fail(h, OFFK_ERR_UNKNOWN_KEY, "offk_bind_weight: not an OFF sub-network key for this variant: " + k);
  Slot& s = h->slots[it->second];
  // the tensor is read in place by every later launch (buffer descriptors sized from the key's shape): check it IS that shape
  bool shape_ok = ndim == (int)s.shape.size();
  size_t need = sizeof(float);
  for (int i = 0; shape_ok && i < ndim; ++i) { shape_ok = shape[i] == s.shape[i]; need *= (size_t)s.shape[i]; }
  if (!shape_ok) return fail(h, OFFK_ERR_INVALID, "offk_bind_weight: shape mismatch for " + k);
  if ((reinterpret_cast<uintptr_t>(device_data) & 15) != 0) return fail(h, OFFK_ERR_INVALID, "offk_bind_weight: pointer must be 16-byte aligned: " + k);
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, device_data) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != h->cfg.device) {
    (void)hipGetLastError();
    return fail(h, OFFK_ERR_INVALID, "offk_bind_weight: needs a device pointer on the handle's device: " + k);
  }
  {   // ... and that the allocation behind the pointer really holds that many bytes from there on
    hipDeviceptr_t base = nullptr;
    size_t asz = 0;
    if (hipMemGetAddressRange(&base, &asz, const_cast<float*>(device_data)) == hipSuccess) {
      const size_t off = (size_t)(reinterpret_cast<const char*>(device_data) - reinterpret_cast<const char*>(base));
      if (off > asz || asz - off < need) return fail(h, OFFK_ERR_INVALID, "offk_bind_weight: allocation too small for " + k);
    } else {
      (void)hipGetLastError();
    }
  }
  if (s.kind >= kNumUnitParams)
    return fail(h, OFFK_ERR_INVALID, "offk_bind_weight: only the OFF units' parameters (motion_conv_gen_*, motion_spatial_down_*, "
                                     "motion_spatial_grad_*) can be bound in place: " + k);
  h->unit[s.idx][s.kind].bound = device_data;
  s.set = true;
  return OFFK_OK;
}

int offk_missing_weights(const offk_handle* h, char* buf, size_t buflen) {
  if (!h) return OFFK_ERR_INVALID;
  int missing = 0;
  for (const Slot& s : h->slots)
    if (!s.set) {
      if (missing == 0 && buf && buflen) snprintf(buf, buflen, "%s", s.key.c_str());
      ++missing;
    }
  return missing;
}

size_t offk_workspace_bytes(const offk_handle* h) { return h ? h->ws_bytes : 0; }

int offk_workspace_region(const offk_handle* h, const char* name, size_t* offset_bytes, size_t* nbytes) {
  if (!h || !name) return OFFK_ERR_INVALID;
  const Region r = region_by_name(name);
  if (r == kNumRegions || !h->regions[r].on) { h->err = std::string("unknown workspace region: ") + name; return OFFK_ERR_INVALID; }
  if (offset_bytes) *offset_bytes = h->regions[r].off;
  if (nbytes) *nbytes = h->regions[r].bytes;
  return OFFK_OK;
}

int offk_set_profiling(offk_handle* h, int enable) {
  if (!h) return OFFK_ERR_INVALID;
  if (enable < 0 || enable > 2) return fail(h, OFFK_ERR_INVALID, "offk_set_profiling: 0 off, 1 per-stage events, 2 per-launch trace");
  h->profiling = enable;
  return OFFK_OK;
}

int offk_launch_times(offk_handle* h, char* names, size_t names_len, double* ms, int64_t* calls, int max_entries, int reset) {
  if (!h || max_entries < 0 || (max_entries > 0 && (!ms || !calls))) return fail(h, OFFK_ERR_INVALID, "offk_launch_times: bad argument");
  DeviceGuard guard(h->cfg.device);
  const int n = (int)h->tr_names.size();
  std::vector<double> sum(n, 0.0);
  std::vector<int64_t> cnt(n, 0);
  if (!h->tr_marks.empty()) HIP_TRY(h, hipEventSynchronize(h->tr_events[h->tr_marks.size() - 1]));
  for (size_t i = 0; i + 1 < h->tr_marks.size(); ++i) {
    const int id = h->tr_marks[i];
    if (id < 0) continue;
    float t = 0.f;
    HIP_TRY(h, hipEventElapsedTime(&t, h->tr_events[i], h->tr_events[i + 1]));
    sum[id] += t;
    cnt[id] += 1;
  }
  std::string all;
  for (int i = 0; i < n && i < max_entries; ++i) {
    ms[i] = sum[i];
    calls[i] = cnt[i];
    all += h->tr_names[i];
    all += '\n';
  }
  if (names && names_len) snprintf(names, names_len, "%s", all.c_str());
  if (reset) { h->tr_marks.clear(); h->tr_names.clear(); }
  return n;
}

int offk_stage_times(offk_handle* h, double ms[OFFK_NUM_STAGES], int64_t calls[OFFK_NUM_STAGES], int reset) {
  if (!h || !ms || !calls) return fail(h, OFFK_ERR_INVALID, "offk_stage_times: null argument");
  DeviceGuard guard(h->cfg.device);
  const size_t per = OFFK_NUM_STAGES + 1;
  for (int s = 0; s < OFFK_NUM_STAGES; ++s) { ms[s] = 0.0; calls[s] = 0; }
  for (size_t g = 0; g < h->ev_used; ++g) {
    hipEvent_t* ev = &h->events[g * per];
    HIP_TRY(h, hipEventSynchronize(ev[OFFK_NUM_STAGES]));
    for (int s = 0; s < OFFK_NUM_STAGES; ++s) {
      float t = 0.f;
      HIP_TRY(h, hipEventElapsedTime(&t, ev[s], ev[s + 1]));
      ms[s] += t;
      calls[s] += 1;
    }
  }
  if (reset) h->ev_used = 0;
  return OFFK_OK;
}

int offk_pw_reduce(offk_handle* h, void* stream, int site, const float* feat, float* G, float* D) {
  return pw_reduce_site(h, stream, nullptr, OFFK_FEAT_F32, site, feat, G, D, "offk_pw_reduce");
}

int offk_sobel_tdiff(offk_handle* h, void* stream, int site, const float* G, const float* D, float* M, int m_cstride,
                     int m_coff, int algo) {
  if (!h || site < 0 || site >= kNumSites || !G || !D || !M) return fail(h, OFFK_ERR_INVALID, "offk_sobel_tdiff: bad argument");
  if (m_cstride % 4 || m_coff % 4 || m_coff < 0 || m_coff + kUnitCh > m_cstride || algo < 0 || algo > 5)
    return fail(h, OFFK_ERR_INVALID, "offk_sobel_tdiff: need 16-byte aligned channel slice of 160 channels inside m_cstride, algo in 0..5");
  TRY(site_weights_ready(h, site, false, true));
  DeviceGuard guard(h->cfg.device);
  StParams sp;
  memset(&sp, 0, sizeof(sp));
  sp.nsites = 1; sp.B = h->cfg.batch; sp.L = h->cfg.length;
  sp.zeros = h->zero_page; sp.drop_scale = 1.f;
  sp.taps4 = h->cfg.variant == OFFK_VARIANT_DIAG_SOBEL && h->sobel_taps4;
  fill_st_site(h, site, G, D, M, m_cstride, m_coff, &sp.s[0]);
  if (algo >= 4) sp.s[0].tchunks = st_tchunks_flat(kSites[site].H, h->cfg.length);
  sp.total_s = h->P * sp.s[0].strips;
  sp.total_t = h->cfg.batch * sp.s[0].tchunks;
  HIP_TRY(h, sobel_tdiff_launch(sp, algo, static_cast<hipStream_t>(stream)));
  return OFFK_OK;
}

int offk_sobel_tdiff_all(offk_handle* h, void* stream, void* workspace, int algo) {
  if (!h || !workspace || algo < 0 || algo > 5) return fail(h, OFFK_ERR_INVALID, "offk_sobel_tdiff_all: bad argument");
  for (int s = 0; s < kNumSites; ++s) {
    int rc = site_weights_ready(h, s, false, true);
    if (rc != OFFK_OK) return rc;
  }
  DeviceGuard guard(h->cfg.device);
  return run_sobel_tdiff_all(h, static_cast<hipStream_t>(stream), workspace, algo);
}

int offk_off_units(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES], void* workspace) {
  return off_units_whole(h, stream, nullptr, OFFK_FEAT_F32, reinterpret_cast<MapPtrs>(feats), workspace, false, 0, 0.0, "offk_off_units");
}

int offk_off_units_fused(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES], void* workspace) {
  if (!h || !feats || !workspace) return fail(h, OFFK_ERR_INVALID, "offk_off_units_fused: null argument");
  offk_feat_parts parts[kNumSites];
  TRY(whole_maps(h, feats, parts, "offk_off_units_fused"));
  for (int s = 0; s < kNumSites; ++s) TRY(site_weights_ready(h, s, true, true));
  DeviceGuard guard(h->cfg.device);
  if (h->fused_units && h->cfg.feat_layout != OFFK_FEAT_NHWC) return run_off_units_fused(h, static_cast<hipStream_t>(stream), parts, workspace, nullptr);
  return run_off_units(h, static_cast<hipStream_t>(stream), parts, workspace, nullptr, h->cfg.feat_layout == OFFK_FEAT_NHWC);
}

int offk_forward(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES], float* out7, float* out14,
                 float* out28, void* workspace) {
  if (!h || !feats) return fail(h, OFFK_ERR_INVALID, "offk_forward: null argument");
  offk_feat_parts parts[kNumSites];
  TRY(whole_maps(h, feats, parts, "offk_forward"));
  return offk_forward_parts(h, stream, parts, out7, out14, out28, workspace);
}

static int forward_parts(offk_handle* h, void* stream, const offk_feat_parts feats[OFFK_NUM_SITES], float* out7, float* out14,
                         float* out28, void* workspace, int feat_dtype, bool cl = false);

int offk_forward_parts(offk_handle* h, void* stream, const offk_feat_parts feats[OFFK_NUM_SITES], float* out7, float* out14,
                       float* out28, void* workspace) {
  return forward_parts(h, stream, feats, out7, out14, out28, workspace, OFFK_FEAT_F32);
}

// ---- 16-bit NCHW feature maps (offk_forward_typed and its siblings), channels-last feature maps (offk_forward_cl and its siblings): FeatKind ----
// Everything such a call is refused for, checked before anything is enqueued.
static int check_feat(offk_handle* h, const FeatKind& k, int feat_dtype, const offk_feat_parts parts[], const char* fn) {
  const std::string f(fn), maps = std::string(": ") + k.noun + " feature maps ";
  if (!(feat_dtype == OFFK_FEAT_F32 && k.f32_ok) && feat_dtype != OFFK_FEAT_BF16 && feat_dtype != OFFK_FEAT_F16)
    return fail(h, OFFK_ERR_INVALID, f + ": unknown feat_dtype " + std::to_string(feat_dtype) + " (OFFK_FEAT_F32 / _BF16 / _F16)");
  if (!h->f32split)
    return fail(h, OFFK_ERR_INVALID, f + maps + "need an OFFK_PRECISION_F32SPLIT handle (precision=\"f32split\"); this handle runs the fp32 pipe");
  if (!k.cl && h->cfg.feat_layout == OFFK_FEAT_NHWC) return fail(h, OFFK_ERR_INVALID, f + maps + "are NCHW-only (this handle is NHWC)");
  if (!h->fused_units)
    return fail(h, OFFK_ERR_INVALID, f + maps + "need the fused units kernel (the handle was created with OFFK_FUSED_UNITS=0)");
  if (const int s = bound_contraction_site(h); s >= 0)
    return fail(h, OFFK_ERR_INVALID, f + maps + "need the library's own unit weights (a gen / down weight is bound through offk_bind_weight: " +
                                         kSites[s].name + ")");
  TRY(check_parts(h, parts));
  for (int s = 0; s < kNumSites; ++s)
    for (int q = 0; q < parts[s].n_parts; ++q)
      if (reinterpret_cast<uintptr_t>(parts[s].data[q]) & (k.align - 1))
        return fail(h, OFFK_ERR_INVALID, f + ": " + k.noun + " feature map pointers must be " + std::to_string(k.align) + "-byte aligned (site " +
                                             kSites[s].name + ")");
  return OFFK_OK;
}

// the common tails of the two families' entries; fn: the name the messages carry
static int forward_parts_kind(offk_handle* h, void* stream, const FeatKind& k, int feat_dtype, const offk_feat_parts parts[OFFK_NUM_SITES],
                              float* out7, float* out14, float* out28, void* workspace, const char* fn) {
  if (!h || !parts || !out7 || !out14 || !workspace) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  TRY(check_feat(h, k, feat_dtype, parts, fn));
  return forward_parts(h, stream, parts, out7, out14, out28, workspace, feat_dtype, k.cl);
}

static int forward_kind(offk_handle* h, void* stream, const FeatKind& k, int feat_dtype, const void* const feats[OFFK_NUM_SITES], float* out7,
                        float* out14, float* out28, void* workspace, const char* fn) {
  if (!h || !feats) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  offk_feat_parts parts[kNumSites];
  TRY(whole_maps(h, feats, parts, fn));
  return forward_parts_kind(h, stream, k, feat_dtype, parts, out7, out14, out28, workspace, fn);
}

static int off_units_fused_kind(offk_handle* h, void* stream, const FeatKind& k, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                                void* workspace, const char* fn) {
  if (!h || !feats || !workspace) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  offk_feat_parts parts[kNumSites];
  TRY(whole_maps(h, feats, parts, fn));
  TRY(check_feat(h, k, feat_dtype, parts, fn));
  for (int s = 0; s < kNumSites; ++s) TRY(site_weights_ready(h, s, true, true));
  DeviceGuard guard(h->cfg.device);
  return run_off_units_fused(h, static_cast<hipStream_t>(stream), parts, workspace, nullptr, feat_dtype, k.cl);
}

int offk_forward_parts_typed(offk_handle* h, void* stream, int feat_dtype, const offk_feat_parts parts[OFFK_NUM_SITES], float* out7,
                             float* out14, float* out28, void* workspace) {
  if (feat_dtype == OFFK_FEAT_F32) return offk_forward_parts(h, stream, parts, out7, out14, out28, workspace);
  return forward_parts_kind(h, stream, kKind16, feat_dtype, parts, out7, out14, out28, workspace, "offk_forward_typed");
}

int offk_forward_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], float* out7,
                       float* out14, float* out28, void* workspace) {
  if (feat_dtype == OFFK_FEAT_F32)
    return offk_forward(h, stream, reinterpret_cast<const float* const*>(feats), out7, out14, out28, workspace);
  return forward_kind(h, stream, kKind16, feat_dtype, feats, out7, out14, out28, workspace, "offk_forward_typed");
}

int offk_off_units_fused_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], void* workspace) {
  if (feat_dtype == OFFK_FEAT_F32) return offk_off_units_fused(h, stream, reinterpret_cast<const float* const*>(feats), workspace);
  return off_units_fused_kind(h, stream, kKind16, feat_dtype, feats, workspace, "offk_off_units_fused_typed");
}

int offk_forward_parts_cl(offk_handle* h, void* stream, int feat_dtype, const offk_feat_parts parts[OFFK_NUM_SITES], float* out7,
                          float* out14, float* out28, void* workspace) {
  return forward_parts_kind(h, stream, kKindCl, feat_dtype, parts, out7, out14, out28, workspace, "offk_forward_cl");
}

int offk_forward_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], float* out7, float* out14,
                    float* out28, void* workspace) {
  return forward_kind(h, stream, kKindCl, feat_dtype, feats, out7, out14, out28, workspace, "offk_forward_cl");
}

int offk_off_units_fused_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], void* workspace) {
  return off_units_fused_kind(h, stream, kKindCl, feat_dtype, feats, workspace, "offk_off_units_fused_cl");
}

static int forward_parts(offk_handle* h, void* stream, const offk_feat_parts feats[OFFK_NUM_SITES], float* out7, float* out14,
                         float* out28, void* workspace, int feat_dtype, bool cl) {
  if (!h || !feats || !out7 || !out14 || !workspace) return fail(h, OFFK_ERR_INVALID, "offk_forward: null argument");
  TRY(check_parts(h, feats));
  TRY(check_ready(h));
  DeviceGuard guard(h->cfg.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Fwd f;
  TRY(f.init(h, st, workspace, out7, out14, out28));
  TRY(f.units(feats, feat_dtype, cl));
  TRY(finalize_merged(h, st));
  TRY(finalize_derived(h, st));
  TRY(f.fusion28());
  TRY(f.fusion14());
  TRY(f.fusion7());
  return f.heads();
}

int offk_stage_tensors(offk_handle* h, void* stream, void* workspace) {
  if (!h || !workspace) return fail(h, OFFK_ERR_INVALID, "offk_stage_tensors: null argument");
  if (!h->sum7_pending) return OFFK_OK;
  DeviceGuard guard(h->cfg.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  Fwd f;
  TRY(f.init(h, st, workspace, nullptr, nullptr, nullptr, true));
  TRY(finalize_merged(h, st));
  TRY(finalize_derived(h, st));
  const int prof = h->profiling;      // not a launch of a forward: it leaves no mark in the per-launch trace
  h->profiling = 0;
  const int rc = f.merged7();
  h->profiling = prof;
  if (rc == OFFK_OK) h->sum7_pending = false;
  return rc;
}

// ---- training side of the OFF units -----------------------------------
size_t offk_train_workspace_bytes(const offk_handle* h) { return h ? h->train_ws_bytes : 0; }

size_t offk_unit_grad_floats(const offk_handle* h) { return h ? h->grad_floats : 0; }

int offk_unit_grad_slot(const offk_handle* h, const char* key, size_t* offset_floats, size_t* count) {
  if (!h || !key) return OFFK_ERR_INVALID;
  std::string k(key);
  if (k.rfind("module.", 0) == 0) k = k.substr(7);
  auto it = h->index.find(k);
  const Slot* s = it == h->index.end() ? nullptr : &h->slots[it->second];
  if (!s || s->kind >= kNumUnitParams) { h->err = "no unit gradient for key: " + k; return OFFK_ERR_INVALID; }
  if (offset_floats) *offset_floats = h->unit[s->idx][s->kind].grad_off;
  if (count) *count = unit_count(kUnitParams[s->kind], kSites[s->idx].C);
  return OFFK_OK;
}

int offk_off_units_train(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES], void* workspace,
                         uint64_t drop_seed, double drop_p) {
  return off_units_whole(h, stream, nullptr, OFFK_FEAT_F32, reinterpret_cast<MapPtrs>(feats), workspace, true, drop_seed, drop_p, "offk_off_units_train");
}

// feat_dtype != OFFK_FEAT_F32: feats[] address 16-bit elements; nhwc: the maps of this call are channels-last (offk_off_units_backward_cl).
// Either way check_feat_train has passed, and only K1b reads the maps.
// split (offk_off_units_backward_split): K1b's GEMM runs in split-fp32 arithmetic (units_wgrad_split.hip) on K1b's launch plan; K2b and the
// reduce are the same launches either way.
static int off_units_backward(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES],
                              const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed, double drop_p,
                              float* grads, int accumulate, int feat_dtype, bool nhwc, bool split = false) {
  if (!h || !feats || !gm || !workspace || !grads) return fail(h, OFFK_ERR_INVALID, "offk_off_units_backward: null argument");
  DropCfg drop;
  TRY(make_drop(h, drop_seed, drop_p, &drop));
  for (int s = 0; s < kNumSites; ++s) {
    if (!feats[s] || !gm[s].data) return fail(h, OFFK_ERR_INVALID, "offk_off_units_backward: null feature map or gradient");
    if (gm[s].cstride < gm[s].coff + kUnitCh || (gm[s].cstride & 3) || (gm[s].coff & 3) || gm[s].coff < 0)
      return fail(h, OFFK_ERR_INVALID, "offk_off_units_backward: gradient view needs 16-byte aligned 160 channels inside cstride");
    TRY(site_weights_ready(h, s, false, true));
  }
  DeviceGuard guard(h->cfg.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  void* ws = workspace;
  const bool learned_dw = h->cfg.variant != OFFK_VARIANT_DIAG_SOBEL;
  auto reg = [&](Region family, int s) { return region(h, ws, site_region(family, s)); };

  // K2b: dM -> dGpre, dD, depthwise partials
  UbParams up;
  memset(&up, 0, sizeof(up));
  up.nsites = kNumSites; up.B = h->cfg.batch; up.L = h->cfg.length; up.tpix = kUbTpix;
  up.drop_thresh = drop.thresh; up.drop_scale = drop.scale; up.zeros = h->zero_page;
  int sblk = 0, tblk = 0;
  int nsblocks[kNumSites];
  for (int s = 0; s < kNumSites; ++s) {
    UbSite& u = up.s[s];
    u.G = reg(R_G, s); u.D = reg(R_D, s);
    u.dw = learned_dw ? unit_param(h, s, SK_DW_W).p : h->sobel_w;
    u.dw_ref = learned_dw && unit_param(h, s, SK_DW_W).bound;
    u.gm = gm[s].data; u.gm_cs = gm[s].cstride; u.gm_coff = gm[s].coff;
    u.dG = reg(R_DG, s); u.dD = reg(R_DD, s);
    u.dw_part = learned_dw ? reg(R_DWP, s) : nullptr;
    u.drop_base = drop_stream_base(drop.seed, s);
    u.H = kSites[s].H;
    ub_plan(u.H, &u.strips, &u.rows);
    u.tchunks = (u.H * u.H + kUbTpix - 1) / kUbTpix;
    u.s_begin = sblk; u.t_begin = tblk;
    nsblocks[s] = h->P * u.strips;
    sblk += nsblocks[s];
    tblk += h->cfg.batch * u.tchunks;
  }
  up.total_s = sblk; up.total_t = tblk;
  HIP_TRY(h, units_bwd_launch(up, st));

  // K1b: weight-gradient GEMM, per-chunk slabs
  WgParams wp;
  memset(&wp, 0, sizeof(wp));
  wp.nsites = kNumSites; wp.L = h->cfg.length; wp.P = h->P; wp.slice_mode = h->cfg.slice_mode; wp.kt_per_blk = h->wg_kpb;
  wp.precision = 0;
  wp.dbg = 0;   // ablation bits of the tools build only
  wp.zeros = h->zero_page;
  WrParams rp;
  memset(&rp, 0, sizeof(rp));
  rp.nsites = kNumSites; rp.accumulate = accumulate ? 1 : 0;
  int blk = 0;
  for (int i = 0; i < kNumSites; ++i) {
    const int s = kPwOrder[i];
    WgSite& w = wp.s[i];
    const offk_feat_parts whole = whole_map(s, feats[s]);
    fill_site_shape(h, s, &whole, &w);
    w.dG = reg(R_DG, s); w.dD = reg(R_DD, s); w.slab = reg(R_WGS, s); w.bpart = reg(R_WGB, s);
    w.tpf = (w.HW + 31) / 32; w.kt_total = h->N * w.tpf;
    w.ntiles = (w.C + 127) / 128; w.nchunks = (w.kt_total + h->wg_kpb - 1) / h->wg_kpb;
    w.blk_begin = blk;
    blk += w.nchunks * w.ntiles;
    WrSite& r = rp.s[i];
    r.slab = w.slab; r.bpart = w.bpart; r.dw_part = learned_dw ? reg(R_DWP, s) : nullptr;
    for (const UnitParamSpec& p : kUnitParams)      // (a parameter the variant lacks: nullptr, rp is zeroed)
      if (h->unit[s][p.kind].slot >= 0) r.*p.grad = grads + h->unit[s][p.kind].grad_off;
    r.C = w.C; r.cpad = w.ntiles * 128; r.nchunks = w.nchunks; r.nsblocks = nsblocks[s];
  }
  wp.total_blocks = blk;
  if (split) HIP_TRY(h, pw_wgrad_split_launch(wp, feat_dtype, nhwc, st));
  else TRY(launch_k1b(h, st, wp, feat_dtype, nhwc));
  HIP_TRY(h, wgrad_reduce_launch(rp, st));
  h->units_bwd_done = true;   // what offk_off_units_backward_feats asks for
  return OFFK_OK;
}

// the common prologue of the three offk_off_units_backward* entries (k == nullptr: the plain one, NCHW handles only)
static int off_units_backward_kind(offk_handle* h, void* stream, const FeatKind* k, int feat_dtype, MapPtrs feats, const offk_grad_view gm[OFFK_NUM_SITES],
                                   void* workspace, uint64_t drop_seed, double drop_p, float* grads, int accumulate, const char* fn,
                                   bool split = false) {
  if (!h || !feats || !gm || !workspace || !grads) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  if (!k && h->cfg.feat_layout == OFFK_FEAT_NHWC) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": NCHW feature maps only");
  if (k) TRY(check_feat_train(h, *k, feat_dtype, feats, 0, kNumSites, fn));
  return off_units_backward(h, stream, reinterpret_cast<const float* const*>(feats), gm, workspace, drop_seed, drop_p, grads, accumulate, feat_dtype,
                            k && k->cl, split);
}

int offk_off_units_backward(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES],
                            const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed, double drop_p,
                            float* grads, int accumulate) {
  return off_units_backward_kind(h, stream, nullptr, OFFK_FEAT_F32, reinterpret_cast<MapPtrs>(feats), gm, workspace, drop_seed, drop_p, grads, accumulate,
                                 "offk_off_units_backward");
}

// ---- 16-bit feature maps on the training side: the _typed entries forward OFFK_FEAT_F32 to the untyped entry ----
int offk_pw_reduce_typed(offk_handle* h, void* stream, int feat_dtype, int site, const void* feat, float* G, float* D) {
  if (feat_dtype == OFFK_FEAT_F32) return offk_pw_reduce(h, stream, site, static_cast<const float*>(feat), G, D);
  return pw_reduce_site(h, stream, &kKind16, feat_dtype, site, feat, G, D, "offk_pw_reduce_typed");
}

int offk_off_units_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], void* workspace) {
  if (feat_dtype == OFFK_FEAT_F32) return offk_off_units(h, stream, reinterpret_cast<const float* const*>(feats), workspace);
  return off_units_whole(h, stream, &kKind16, feat_dtype, feats, workspace, false, 0, 0.0, "offk_off_units_typed");
}

int offk_off_units_train_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], void* workspace,
                               uint64_t drop_seed, double drop_p) {
  if (feat_dtype == OFFK_FEAT_F32)
    return offk_off_units_train(h, stream, reinterpret_cast<const float* const*>(feats), workspace, drop_seed, drop_p);
  return off_units_whole(h, stream, &kKind16, feat_dtype, feats, workspace, true, drop_seed, drop_p, "offk_off_units_train_typed");
}

int offk_off_units_backward_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                                  const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed, double drop_p,
                                  float* grads, int accumulate) {
  if (feat_dtype == OFFK_FEAT_F32)
    return offk_off_units_backward(h, stream, reinterpret_cast<const float* const*>(feats), gm, workspace, drop_seed, drop_p, grads, accumulate);
  return off_units_backward_kind(h, stream, &kKind16, feat_dtype, feats, gm, workspace, drop_seed, drop_p, grads, accumulate,
                                 "offk_off_units_backward_typed");
}

// ---- channels-last feature maps on the training side ----
int offk_pw_reduce_cl(offk_handle* h, void* stream, int feat_dtype, int site, const void* feat, float* G, float* D) {
  return pw_reduce_site(h, stream, &kKindCl, feat_dtype, site, feat, G, D, "offk_pw_reduce_cl");
}

int offk_off_units_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], void* workspace) {
  return off_units_whole(h, stream, &kKindCl, feat_dtype, feats, workspace, false, 0, 0.0, "offk_off_units_cl");
}

int offk_off_units_train_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES], void* workspace,
                            uint64_t drop_seed, double drop_p) {
  return off_units_whole(h, stream, &kKindCl, feat_dtype, feats, workspace, true, drop_seed, drop_p, "offk_off_units_train_cl");
}

int offk_off_units_backward_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                               const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed, double drop_p,
                               float* grads, int accumulate) {
  return off_units_backward_kind(h, stream, &kKindCl, feat_dtype, feats, gm, workspace, drop_seed, drop_p, grads, accumulate,
                                 "offk_off_units_backward_cl");
}

// ---- the units' backward with the weight-gradient GEMM in split-fp32 arithmetic (units_wgrad_split.hip) ----
// The kind of the maps follows from (layout, feat_dtype) as it follows from the entry's name elsewhere: NHWC -> the _cl entry's checks, NCHW
// 16-bit -> the _typed entry's, NCHW fp32 -> the plain entry's.
int offk_off_units_backward_split(offk_handle* h, void* stream, int feat_dtype, int layout, const void* const feats[OFFK_NUM_SITES],
                                  const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed, double drop_p,
                                  float* grads, int accumulate) {
  const char* fn = "offk_off_units_backward_split";
  if (!h || !feats || !gm || !workspace || !grads) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  if (layout != OFFK_FEAT_NCHW && layout != OFFK_FEAT_NHWC)
    return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": layout must be OFFK_FEAT_NCHW or OFFK_FEAT_NHWC");
  if (feat_dtype != OFFK_FEAT_F32 && feat_dtype != OFFK_FEAT_BF16 && feat_dtype != OFFK_FEAT_F16)
    return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": unknown feat_dtype " + std::to_string(feat_dtype) + " (OFFK_FEAT_F32 / _BF16 / _F16)");
  const FeatKind* k = layout == OFFK_FEAT_NHWC ? &kKindCl : (feat_dtype == OFFK_FEAT_F32 ? nullptr : &kKind16);
  return off_units_backward_kind(h, stream, k, feat_dtype, feats, gm, workspace, drop_seed, drop_p, grads, accumulate, fn, true);
}

// ---- the units' train forward with K1 in split-fp32 arithmetic (units_fwd_split.hip): offk_off_units_train / _typed / _cl in one entry ----
int offk_off_units_train_split(offk_handle* h, void* stream, int feat_dtype, int layout, const void* const feats[OFFK_NUM_SITES], void* workspace,
                               uint64_t drop_seed, double drop_p) {
  const char* fn = "offk_off_units_train_split";
  if (!h || !feats || !workspace) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  if (layout != OFFK_FEAT_NCHW && layout != OFFK_FEAT_NHWC)
    return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": layout must be OFFK_FEAT_NCHW or OFFK_FEAT_NHWC");
  if (feat_dtype != OFFK_FEAT_F32 && feat_dtype != OFFK_FEAT_BF16 && feat_dtype != OFFK_FEAT_F16)
    return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": unknown feat_dtype " + std::to_string(feat_dtype) + " (OFFK_FEAT_F32 / _BF16 / _F16)");
  DropCfg drop;
  TRY(make_drop(h, drop_seed, drop_p, &drop));
  const bool cl = layout == OFFK_FEAT_NHWC;
  if (cl || feat_dtype != OFFK_FEAT_F32) TRY(check_feat_train(h, cl ? kKindCl : kKind16, feat_dtype, feats, 0, kNumSites, fn));
  else if (h->cfg.feat_layout == OFFK_FEAT_NHWC) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": NCHW feature maps on an NHWC handle (pass OFFK_FEAT_NHWC)");
  offk_feat_parts parts[kNumSites];
  TRY(whole_maps(h, feats, parts, fn));
  for (int s = 0; s < kNumSites; ++s) TRY(site_weights_ready(h, s, true, true));
  DeviceGuard guard(h->cfg.device);
  return run_off_units_split(h, static_cast<hipStream_t>(stream), parts, workspace, cl, drop, feat_dtype);
}

// ---- gradient w.r.t. the feature maps (units_dx.hip) ----
// the launches of offk_off_units_backward_feats_split (units_dx_split.hip) behind the checks all dX entries share
static int off_units_backward_feats_split(offk_handle* h, hipStream_t st, void* workspace, int out_dtype, void* const dfeats[OFFK_NUM_SITES], int layout,
                                          int accumulate) {
  DxsParams dp;
  memset(&dp, 0, sizeof(dp));
  dp.L = h->cfg.length; dp.P = h->P; dp.slice_mode = h->cfg.slice_mode;
  dp.nchw = layout == OFFK_FEAT_NCHW; dp.accumulate = accumulate ? 1 : 0; dp.zeros = h->zero_page; dp.out_dtype = out_dtype;
  int blk = 0, pblk = 0, n = 0;
  for (int i = 0; i < kNumSites; ++i) {      // the widest sites first, as the fp32 entry orders them
    const int s = kPwOrder[i];
    if (!dfeats[s]) continue;
    DxsSite& d = dp.s[n++];
    const float *b, *bd;
    pw_weight_ptrs(h, s, &d.wg, &d.wd, &b, &bd);
    d.dG = region(h, workspace, site_region(R_DG, s));
    d.dD = region(h, workspace, site_region(R_DD, s));
    d.wimg = h->dx_split_w[s];
    d.out = dfeats[s];
    fill_site_shape(h, s, nullptr, &d);
    d.blk_begin = blk; d.pack_begin = pblk;
    blk += (d.M + units_dx_split_rows_per_block() - 1) / units_dx_split_rows_per_block();
    pblk += units_dx_split_pack_blocks(d.C);
  }
  dp.nsites = n; dp.total_blocks = blk; dp.pack_blocks = pblk;
  static const char* const kDxsTrace[3][2] = {
      {"units:feature-map gradient (dX, NHWC, split)", "units:feature-map gradient (dX, NCHW, split)"},
      {"units:feature-map gradient (dX, NHWC, split, bf16)", "units:feature-map gradient (dX, NCHW, split, bf16)"},
      {"units:feature-map gradient (dX, NHWC, split, fp16)", "units:feature-map gradient (dX, NCHW, split, fp16)"}};
  TRY(trace_mark(h, st, kDxsTrace[out_dtype][dp.nchw]));
  HIP_TRY(h, units_dx_split_launch(dp, st));
  return trace_mark(h, st, nullptr);
}

// the body of both entries: out_dtype kFeatF32 (fn the untyped entry's name: its launch, its bits) / kFeatBf16 / kFeatF16
static int off_units_backward_feats(offk_handle* h, void* stream, void* workspace, int out_dtype, void* const dfeats[OFFK_NUM_SITES], int layout,
                                    int accumulate, const char* fn, bool split = false) {
  if (!h || !workspace || !dfeats) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": null argument");
  if (out_dtype != kFeatF32 && out_dtype != kFeatBf16 && out_dtype != kFeatF16)
    return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": grad_dtype must be OFFK_FEAT_F32, OFFK_FEAT_BF16 or OFFK_FEAT_F16");
  const size_t esize = out_dtype == kFeatF32 ? sizeof(float) : 2;
  if (layout != OFFK_FEAT_NCHW && layout != OFFK_FEAT_NHWC)
    return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": layout must be OFFK_FEAT_NCHW or OFFK_FEAT_NHWC");
  if (!h->units_bwd_done)
    return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": no offk_off_units_backward has run on this handle: dG_<site> / dD_<site> hold nothing yet");
  const char* ws_lo = static_cast<const char*>(workspace);
  const char* ws_hi = ws_lo + h->train_ws_bytes;
  int nreq = 0;
  for (int s = 0; s < kNumSites; ++s) {
    if (!dfeats[s]) continue;
    ++nreq;
    if (reinterpret_cast<uintptr_t>(dfeats[s]) & 15) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": gradient pointers must be 16-byte aligned");
    const char* lo = reinterpret_cast<const char*>(dfeats[s]);
    const char* hi = lo + (size_t)h->N * kSites[s].C * kSites[s].H * kSites[s].H * esize;
    if (lo < ws_hi && ws_lo < hi) return fail(h, OFFK_ERR_INVALID, std::string(fn) + ": a gradient buffer overlaps the workspace");
    TRY(site_weights_ready(h, s, true, false));
  }
  if (!nreq) return OFFK_OK;
  DeviceGuard guard(h->cfg.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (split) return off_units_backward_feats_split(h, st, workspace, out_dtype, dfeats, layout, accumulate);
  DxParams dp;
  memset(&dp, 0, sizeof(dp));
  dp.L = h->cfg.length; dp.P = h->P; dp.slice_mode = h->cfg.slice_mode;
  dp.nchw = layout == OFFK_FEAT_NCHW; dp.accumulate = accumulate ? 1 : 0; dp.zeros = h->zero_page; dp.out_dtype = out_dtype;
  int blk = 0, n = 0;
  for (int i = 0; i < kNumSites; ++i) {      // the widest sites first, as K1 / K1b order theirs
    const int s = kPwOrder[i];
    if (!dfeats[s]) continue;
    DxSite& d = dp.s[n++];
    const float *b, *bd;
    pw_weight_ptrs(h, s, &d.wg, &d.wd, &b, &bd);
    d.dG = region(h, workspace, site_region(R_DG, s));
    d.dD = region(h, workspace, site_region(R_DD, s));
    d.out = dfeats[s];
    fill_site_shape(h, s, nullptr, &d);
    d.blk_begin = blk;
    blk += (d.M + units_dx_rows_per_block() - 1) / units_dx_rows_per_block();
  }
  dp.nsites = n; dp.total_blocks = blk;
  static const char* const kDxTrace[3][2] = {
      {"units:feature-map gradient (dX, NHWC)", "units:feature-map gradient (dX, NCHW)"},
      {"units:feature-map gradient (dX, NHWC, bf16)", "units:feature-map gradient (dX, NCHW, bf16)"},
      {"units:feature-map gradient (dX, NHWC, fp16)", "units:feature-map gradient (dX, NCHW, fp16)"}};
  TRY(trace_mark(h, st, kDxTrace[out_dtype][dp.nchw]));
  HIP_TRY(h, out_dtype == kFeatF32 ? units_dx_launch(dp, st) : units_dx16_launch(dp, st));
  return trace_mark(h, st, nullptr);
}

int offk_off_units_backward_feats(offk_handle* h, void* stream, void* workspace, float* const dfeats[OFFK_NUM_SITES], int layout,
                                  int accumulate) {
  return off_units_backward_feats(h, stream, workspace, kFeatF32, reinterpret_cast<void* const*>(dfeats), layout, accumulate,
                                  "offk_off_units_backward_feats");
}

int offk_off_units_backward_feats_typed(offk_handle* h, void* stream, void* workspace, int grad_dtype, void* const dfeats[OFFK_NUM_SITES],
                                        int layout, int accumulate) {
  if (grad_dtype == OFFK_FEAT_F32)
    return offk_off_units_backward_feats(h, stream, workspace, reinterpret_cast<float* const*>(dfeats), layout, accumulate);
  return off_units_backward_feats(h, stream, workspace, grad_dtype, dfeats, layout, accumulate, "offk_off_units_backward_feats_typed");
}

int offk_off_units_backward_feats_split(offk_handle* h, void* stream, void* workspace, int grad_dtype, void* const dfeats[OFFK_NUM_SITES],
                                        int layout, int accumulate) {
  return off_units_backward_feats(h, stream, workspace, grad_dtype, dfeats, layout, accumulate, "offk_off_units_backward_feats_split", true);
}

int offk_segment_consensus_backward(void* stream, const float* grad_out, int B, int T, int C, float* grad_in) {
  if (!grad_out || !grad_in || B < 1 || T < 1 || C < 1) return fail(nullptr, OFFK_ERR_INVALID, "offk_segment_consensus_backward: bad argument");
  hipError_t e = consensus_bwd_launch(grad_out, B, T, C, grad_in, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(nullptr, OFFK_ERR_HIP, hipGetErrorString(e));
  return OFFK_OK;
}

int offk_conv2d(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int Ci, const float* w,
                const float* bias, int Co, int KH, int KW, int stride, int pad, const float* res, int res_cstride,
                int res_coff, int flags, float* y, int y_cstride, int y_coff) {
  if (!x || !w || !y || n_img < 1 || H < 1 || W < 1) return fail(nullptr, OFFK_ERR_INVALID, "offk_conv2d: bad argument");
  return offk_conv2d_ex(stream, x, x_cstride, x_coff, n_img, H, W, Ci, w, bias, Co, KH, KW, stride, pad, res, res_cstride, res_coff, flags, y,
                        y_cstride, y_coff, -1, 0, nullptr, 0, 0);      // ConvDesc's own defaults
}

int offk_conv2d_ex(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int Ci, const float* w,
                   const float* bias, int Co, int KH, int KW, int stride, int pad, const float* res, int res_cstride,
                   int res_coff, int flags, float* y, int y_cstride, int y_coff, int tile_cfg, int splitk, float* partial,
                   size_t partial_floats, int precision) {
  if (!x || !w || !y || n_img < 1 || H < 1 || W < 1) return fail(nullptr, OFFK_ERR_INVALID, "offk_conv2d_ex: bad argument");
  const ConvDesc d = conv_desc(x, x_cstride, x_coff, n_img, H, W, Ci, w, bias, Co, KH, KW, stride, pad, res, res_cstride, res_coff, flags, y,
                               y_cstride, y_coff, tile_cfg, splitk, partial, partial_floats, precision);
  const char* why = nullptr;
  hipError_t e = conv2d_launch(d, static_cast<hipStream_t>(stream), &why);
  if (e != hipSuccess) return fail(nullptr, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, why ? why : hipGetErrorString(e));
  return OFFK_OK;
}

// ---- K4b: backward of one fusion conv: stride 1 (conv_bwd.hip) or stride 2 (conv_bwd_s2.hip), exact fp32 or split-fp32 ----
namespace {
// a channels-last view [rows][cstride] that holds C channels at coff; nullptr = fine, else what is wrong with it
const char* view_problem(const void* ptr, int cstride, int coff, int C) {
  if (!ptr) return "null pointer";
  if (coff < 0) return "negative channel offset";
  if (cstride % 4 || coff % 4) return "strides and offsets must be multiples of 4";
  if (cstride < coff + C) return "cstride < coff + C";
  return nullptr;
}
bool views_overlap(const void* a, int a_cs, long long a_rows, const void* b, int b_cs, long long b_rows) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), a1 = a0 + (size_t)a_rows * (size_t)a_cs * sizeof(float);
  const uintptr_t b0 = reinterpret_cast<uintptr_t>(b), b1 = b0 + (size_t)b_rows * (size_t)b_cs * sizeof(float);
  return a0 < b1 && b0 < a1;
}
int conv_bwd_shape(const char* who, int n_img, int H, int W, int Ci, int Co, int KH, int KW, int pad) {
  if (n_img < 1 || H < 1 || W < 1) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument (n_img, H, W >= 1)");
  if (KH != KW || (KH != 1 && KH != 3)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": the kernel must be 1x1 or 3x3");
  if (pad != (KH - 1) / 2) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": pad must be (KH - 1) / 2 (stride 1, same-size output)");
  if (Ci < 64 || Co < 64 || Ci % 64 || Co % 64) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": need Ci % 64 == 0 and Co % 64 == 0");
  if (!conv_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": problem too large");
  return OFFK_OK;
}
int conv_s2_bwd_shape(const char* who, int n_img, int H, int W, int Ci, int Co, int KH, int KW, int pad) {
  if (n_img < 1 || H < 2 || W < 2) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument (n_img >= 1, H, W >= 2)");
  if (!(KH == KW && ((KH == 7 && pad == 3) || (KH == 5 && pad == 2))))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": the form must be 7x7 with pad 3 or 5x5 with pad 2 (stride 2)");
  if ((H & 1) || (W & 1)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": H and W (the input map) must be even");
  if (Ci < 32 || Co < 64 || Ci % 32 || Co % 64) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": need Ci % 32 == 0 and Co % 64 == 0");
  if (!conv_s2_bwd_supported(n_img, H, W, Ci, Co, KH, KW)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": problem too large");
  return OFFK_OK;
}

// One row per (stride, arithmetic): what the entries of that form differ in.  The bodies below are the entries; a new form is a row.
struct ConvBwdForm {
  int (*shape)(const char* who, int n_img, int H, int W, int Ci, int Co, int KH, int KW, int pad);
  int g_step;                          // g (the output's gradient) has (H / g_step)(W / g_step) rows per image
  const char* plan_fail;               // what a plan that refuses a shape the shape check let through is reported as
  // data gradient: scratch bytes, the launch, the plan entry named by "scratch too small (...)", must the scratch be 16-byte aligned
  bool (*data_plan)(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* bytes);
  hipError_t (*data_launch)(const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw, int Ci, int KS, int pad,
                            float* dx, int dx_cs, int dx_coff, int accumulate, void* scratch, size_t plan_bytes, hipStream_t st, const char** why);
  const char* data_plan_entry;
  bool data_align16;
  // weight gradient: scratch floats and K chunks, the launch, the plan entry named by "scratch too small (...)"
  bool (*weight_plan)(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* floats, int* chunks);
  hipError_t (*weight_launch)(const float* x, int x_cs, int x_coff, const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Ci, int Co,
                              int KS, int relu_in, float* dw, float* db, int accumulate, float* scratch, int chunks, hipStream_t st);
  const char* weight_plan_entry;
};

#define OFFK_DATA_PLAN_ARGS int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* bytes
#define OFFK_DATA_LAUNCH_ARGS                                                                                                                  \
  const float* g, int g_cs, int g_coff, int n_img, int H, int W, int Co, const float* w, int Ci, int KS, int pad, float* dx, int dx_cs, int dx_coff, \
      int acc, void* scratch, size_t plan_bytes, hipStream_t st, const char** why
bool split_bytes(bool ok, size_t wb, size_t gb, size_t* bytes) { *bytes = wb + gb; return ok; }

const ConvBwdForm kConvBwdS1 = {
    conv_bwd_shape, 1, ": unsupported shape",
    [](OFFK_DATA_PLAN_ARGS) {
      const bool ok = conv_bwd_plan(n_img, H, W, Ci, Co, KH, KW, bytes, nullptr, nullptr, nullptr);
      *bytes *= sizeof(float);
      return ok;
    },
    [](OFFK_DATA_LAUNCH_ARGS) {
      return conv_bwd_data_launch(g, g_cs, g_coff, n_img, H, W, Co, w, Ci, KS, dx, dx_cs, dx_coff, acc, static_cast<float*>(scratch),
                                  plan_bytes / sizeof(float), st, why);
    },
    "offk_conv2d_backward_plan", false,
    [](int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* floats, int* chunks) {
      return conv_bwd_plan(n_img, H, W, Ci, Co, KH, KW, nullptr, floats, chunks, nullptr);
    },
    conv_bwd_weight_launch, "offk_conv2d_backward_plan"};
const ConvBwdForm kConvBwdS1Split = {
    conv_bwd_shape, 1, ": problem too large",
    [](OFFK_DATA_PLAN_ARGS) {
      size_t wb = 0, gb = 0;
      return split_bytes(conv_dgrad_split_plan(n_img, H, W, Ci, Co, KH, KW, &wb, &gb), wb, gb, bytes);
    },
    [](OFFK_DATA_LAUNCH_ARGS) { return conv_dgrad_split_launch(g, g_cs, g_coff, n_img, H, W, Co, w, Ci, KS, pad, dx, dx_cs, dx_coff, acc, scratch, st); },
    "offk_conv2d_backward_data_plan_split", true,
    conv_wgrad_split_plan, conv_wgrad_split_launch, "offk_conv2d_backward_plan_split"};
const ConvBwdForm kConvBwdS2 = {
    conv_s2_bwd_shape, 2, ": unsupported shape",
    [](OFFK_DATA_PLAN_ARGS) {
      const bool ok = conv_s2_bwd_plan(n_img, H, W, Ci, Co, KH, KW, bytes, nullptr, nullptr);
      *bytes *= sizeof(float);
      return ok;
    },
    [](OFFK_DATA_LAUNCH_ARGS) {
      return conv_s2_bwd_data_launch(g, g_cs, g_coff, n_img, H, W, Co, w, Ci, KS, pad, dx, dx_cs, dx_coff, acc, static_cast<float*>(scratch), st);
    },
    "offk_conv2d_s2_backward_plan", false,
    [](int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* floats, int* chunks) {
      return conv_s2_bwd_plan(n_img, H, W, Ci, Co, KH, KW, nullptr, floats, chunks);
    },
    conv_s2_bwd_weight_launch, "offk_conv2d_s2_backward_plan"};
const ConvBwdForm kConvBwdS2Split = {
    conv_s2_bwd_shape, 2, ": problem too large",
    [](OFFK_DATA_PLAN_ARGS) {
      size_t wb = 0, gb = 0;
      return split_bytes(conv_s2_dgrad_split_plan(n_img, H, W, Ci, Co, KH, KW, &wb, &gb), wb, gb, bytes);
    },
    [](OFFK_DATA_LAUNCH_ARGS) { return conv_s2_dgrad_split_launch(g, g_cs, g_coff, n_img, H, W, Co, w, Ci, KS, pad, dx, dx_cs, dx_coff, acc, scratch, st); },
    "offk_conv2d_s2_backward_plan_split", true,
    conv_s2_wgrad_split_plan, conv_s2_wgrad_split_launch, "offk_conv2d_s2_backward_weight_plan_split"};
#undef OFFK_DATA_PLAN_ARGS
#undef OFFK_DATA_LAUNCH_ARGS

// A plan entry: the shape check, then the data gradient's scratch bytes and / or the weight gradient's scratch bytes and chunks (whatever
// the entry returns; a null output pointer is skipped)
int conv_bwd_plan_entry(const ConvBwdForm& f, const char* who, int n_img, int H, int W, int Ci, int Co, int KH, int KW, bool data, bool weight,
                        size_t* data_scratch_bytes, size_t* weight_scratch_bytes, int* weight_chunks) {
  if (int rc = f.shape(who, n_img, H, W, Ci, Co, KH, KW, (KH - 1) / 2)) return rc;
  size_t db = 0, wf = 0;
  int chunks = 0;
  if ((data && !f.data_plan(n_img, H, W, Ci, Co, KH, KW, &db)) || (weight && !f.weight_plan(n_img, H, W, Ci, Co, KH, KW, &wf, &chunks)))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + f.plan_fail);
  if (data_scratch_bytes) *data_scratch_bytes = db;
  if (weight_scratch_bytes) *weight_scratch_bytes = wf * sizeof(float);
  if (weight_chunks) *weight_chunks = chunks;
  return OFFK_OK;
}

int conv_bwd_data_entry(const ConvBwdForm& f, const char* who, void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W,
                        int Co, const float* w_oihw, int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff, int accumulate,
                        void* scratch, size_t scratch_bytes) {
  if (!w_oihw || !scratch) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": null pointer");
  if (int rc = f.shape(who, n_img, H, W, Ci, Co, KH, KW, pad)) return rc;
  if (const char* w = view_problem(g, g_cstride, g_coff, Co)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": g: " + w);
  if (const char* w = view_problem(dx, dx_cstride, dx_coff, Ci)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": dx: " + w);
  const long long g_rows = (long long)n_img * (H / f.g_step) * (W / f.g_step), dx_rows = (long long)n_img * H * W;
  if (views_overlap(dx, dx_cstride, dx_rows, g, g_cstride, g_rows)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": dx overlaps g");
  size_t bytes = 0;
  if (!f.data_plan(n_img, H, W, Ci, Co, KH, KW, &bytes)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + f.plan_fail);
  if (scratch_bytes < bytes) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": scratch too small (" + f.data_plan_entry + ")");
  if (f.data_align16 && reinterpret_cast<uintptr_t>(scratch) % 16)
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": scratch must be 16-byte aligned");
  const char* why = nullptr;
  hipError_t e = f.data_launch(g, g_cstride, g_coff, n_img, H, W, Co, w_oihw, Ci, KH, pad, dx, dx_cstride, dx_coff, accumulate != 0, scratch, bytes,
                               static_cast<hipStream_t>(stream), &why);
  if (e != hipSuccess) return why ? fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": " + why) : fail_hip(nullptr, e, who);
  return OFFK_OK;
}

int conv_bwd_weight_entry(const ConvBwdForm& f, const char* who, void* stream, const float* x, int x_cstride, int x_coff, const float* g,
                          int g_cstride, int g_coff, int n_img, int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in,
                          float* dw_oihw, float* db, int accumulate, void* scratch, size_t scratch_bytes) {
  if (!dw_oihw || !scratch) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": null pointer");
  if (int rc = f.shape(who, n_img, H, W, Ci, Co, KH, KW, pad)) return rc;
  if (const char* w = view_problem(x, x_cstride, x_coff, Ci)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": x: " + w);
  if (const char* w = view_problem(g, g_cstride, g_coff, Co)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": g: " + w);
  size_t wf = 0;
  int chunks = 0;
  if (!f.weight_plan(n_img, H, W, Ci, Co, KH, KW, &wf, &chunks)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + f.plan_fail);
  if (scratch_bytes < wf * sizeof(float))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": scratch too small (" + f.weight_plan_entry + ")");
  hipError_t e = f.weight_launch(x, x_cstride, x_coff, g, g_cstride, g_coff, n_img, H, W, Ci, Co, KH, relu_in != 0, dw_oihw, db, accumulate != 0,
                                 static_cast<float*>(scratch), chunks, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  return OFFK_OK;
}
}  // namespace

int offk_conv2d_backward_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes,
                              size_t* weight_scratch_bytes, int* weight_chunks) {
  return conv_bwd_plan_entry(kConvBwdS1, "offk_conv2d_backward_plan", n_img, H, W, Ci, Co, KH, KW, true, true, data_scratch_bytes,
                             weight_scratch_bytes, weight_chunks);
}

int offk_relu_backward(void* stream, const float* dy, int dy_cstride, int dy_coff, const float* y, int y_cstride, int y_coff, int rows, int C,
                       float* g, int g_cstride, int g_coff, int accumulate) {
  const char* who = "offk_relu_backward";
  if (rows < 1 || C < 4 || C % 4) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument (rows >= 1, C % 4 == 0)");
  if (const char* w = view_problem(dy, dy_cstride, dy_coff, C)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": dy: " + w);
  if (const char* w = view_problem(y, y_cstride, y_coff, C)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": y: " + w);
  if (const char* w = view_problem(g, g_cstride, g_coff, C)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": g: " + w);
  const bool in_place = g == dy && g_cstride == dy_cstride && g_coff == dy_coff;
  if (!in_place && views_overlap(g, g_cstride, rows, dy, dy_cstride, rows))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": g overlaps dy without being dy itself (same pointer, stride and offset)");
  if (views_overlap(g, g_cstride, rows, y, y_cstride, rows)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": g overlaps y");
  hipError_t e = relu_backward_launch(dy, dy_cstride, dy_coff, y, y_cstride, y_coff, rows, C, g, g_cstride, g_coff, accumulate != 0,
                                      static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  return OFFK_OK;
}

int offk_conv2d_backward_data(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw,
                              int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff, int accumulate, void* scratch,
                              size_t scratch_bytes) {
  return conv_bwd_data_entry(kConvBwdS1, "offk_conv2d_backward_data", stream, g, g_cstride, g_coff, n_img, H, W, Co, w_oihw, Ci, KH, KW, pad, dx,
                             dx_cstride, dx_coff, accumulate, scratch, scratch_bytes);
}

int offk_conv2d_backward_weight(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff, int n_img,
                                int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw, float* db, int accumulate,
                                void* scratch, size_t scratch_bytes) {
  return conv_bwd_weight_entry(kConvBwdS1, "offk_conv2d_backward_weight", stream, x, x_cstride, x_coff, g, g_cstride, g_coff, n_img, H, W, Ci, Co,
                               KH, KW, pad, relu_in, dw_oihw, db, accumulate, scratch, scratch_bytes);
}

// ---- K4b in split-fp32 arithmetic (conv_wgrad_split.hip, conv_dgrad_split.hip) ----
int offk_conv2d_backward_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_scratch_bytes, int* weight_chunks) {
  return conv_bwd_plan_entry(kConvBwdS1Split, "offk_conv2d_backward_plan_split", n_img, H, W, Ci, Co, KH, KW, false, true, nullptr,
                             weight_scratch_bytes, weight_chunks);
}

int offk_conv2d_backward_weight_split(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff,
                                      int n_img, int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw, float* db,
                                      int accumulate, void* scratch, size_t scratch_bytes) {
  return conv_bwd_weight_entry(kConvBwdS1Split, "offk_conv2d_backward_weight_split", stream, x, x_cstride, x_coff, g, g_cstride, g_coff, n_img, H,
                               W, Ci, Co, KH, KW, pad, relu_in, dw_oihw, db, accumulate, scratch, scratch_bytes);
}

int offk_conv2d_backward_data_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes) {
  return conv_bwd_plan_entry(kConvBwdS1Split, "offk_conv2d_backward_data_plan_split", n_img, H, W, Ci, Co, KH, KW, true, false,
                             data_scratch_bytes, nullptr, nullptr);
}

int offk_conv2d_backward_data_form_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, int* ci_per_block, int* pixels_per_block) {
  const char* who = "offk_conv2d_backward_data_form_split";
  if (int rc = conv_bwd_shape(who, n_img, H, W, Ci, Co, KH, KW, (KH - 1) / 2)) return rc;
  if (!conv_dgrad_split_plan(n_img, H, W, Ci, Co, KH, KW, nullptr, nullptr)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": problem too large");
  int cb = 0, pb = 0;
  conv_dgrad_split_form(n_img, H, W, Ci, &cb, &pb);
  if (ci_per_block) *ci_per_block = cb;
  if (pixels_per_block) *pixels_per_block = pb;
  return OFFK_OK;
}

int offk_conv2d_backward_data_split(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co,
                                    const float* w_oihw, int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff,
                                    int accumulate, void* scratch, size_t scratch_bytes) {
  return conv_bwd_data_entry(kConvBwdS1Split, "offk_conv2d_backward_data_split", stream, g, g_cstride, g_coff, n_img, H, W, Co, w_oihw, Ci, KH, KW,
                             pad, dx, dx_cstride, dx_coff, accumulate, scratch, scratch_bytes);
}

// ---- K4b, stride 2: the 7x7 / 2 / 3 and 5x5 / 2 / 2 fusion convs (conv_bwd_s2.hip; conv_dgrad_s2_split.hip, conv_wgrad_s2_split.hip) ----
int offk_conv2d_s2_backward_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes,
                                 size_t* weight_scratch_bytes, int* weight_chunks) {
  return conv_bwd_plan_entry(kConvBwdS2, "offk_conv2d_s2_backward_plan", n_img, H, W, Ci, Co, KH, KW, true, true, data_scratch_bytes,
                             weight_scratch_bytes, weight_chunks);
}

int offk_conv2d_s2_backward_data(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw,
                                 int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff, int accumulate, void* scratch,
                                 size_t scratch_bytes) {
  return conv_bwd_data_entry(kConvBwdS2, "offk_conv2d_s2_backward_data", stream, g, g_cstride, g_coff, n_img, H, W, Co, w_oihw, Ci, KH, KW, pad,
                             dx, dx_cstride, dx_coff, accumulate, scratch, scratch_bytes);
}

int offk_conv2d_s2_backward_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes) {
  return conv_bwd_plan_entry(kConvBwdS2Split, "offk_conv2d_s2_backward_plan_split", n_img, H, W, Ci, Co, KH, KW, true, false, data_scratch_bytes,
                             nullptr, nullptr);
}

int offk_conv2d_s2_backward_data_split(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co,
                                       const float* w_oihw, int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff,
                                       int accumulate, void* scratch, size_t scratch_bytes) {
  return conv_bwd_data_entry(kConvBwdS2Split, "offk_conv2d_s2_backward_data_split", stream, g, g_cstride, g_coff, n_img, H, W, Co, w_oihw, Ci, KH,
                             KW, pad, dx, dx_cstride, dx_coff, accumulate, scratch, scratch_bytes);
}

int offk_conv2d_s2_backward_weight(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff, int n_img,
                                   int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw, float* db,
                                   int accumulate, void* scratch, size_t scratch_bytes) {
  return conv_bwd_weight_entry(kConvBwdS2, "offk_conv2d_s2_backward_weight", stream, x, x_cstride, x_coff, g, g_cstride, g_coff, n_img, H, W, Ci,
                               Co, KH, KW, pad, relu_in, dw_oihw, db, accumulate, scratch, scratch_bytes);
}

int offk_conv2d_s2_backward_weight_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_scratch_bytes,
                                              int* weight_chunks) {
  return conv_bwd_plan_entry(kConvBwdS2Split, "offk_conv2d_s2_backward_weight_plan_split", n_img, H, W, Ci, Co, KH, KW, false, true, nullptr,
                             weight_scratch_bytes, weight_chunks);
}

int offk_conv2d_s2_backward_weight_split(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff,
                                         int n_img, int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw,
                                         float* db, int accumulate, void* scratch, size_t scratch_bytes) {
  return conv_bwd_weight_entry(kConvBwdS2Split, "offk_conv2d_s2_backward_weight_split", stream, x, x_cstride, x_coff, g, g_cstride, g_coff, n_img,
                               H, W, Ci, Co, KH, KW, pad, relu_in, dw_oihw, db, accumulate, scratch, scratch_bytes);
}

int offk_bottleneck_chain14(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Cin, int relu_in,
                            const float* w1, const float* b1, const float* w2_packed, const float* b2, const float* w3,
                            const float* b3, int K3, const float* res, int res_cstride, int res_coff, float* y, int y_cstride,
                            int y_coff) {
  if (!x || !w1 || !b1 || !w2_packed || !b2 || !w3 || !b3 || !y || n_img < 1)
    return fail(nullptr, OFFK_ERR_INVALID, "offk_bottleneck_chain14: bad argument");
  // (u2 stays nullptr: the stage entry point runs the direct 3x3, it has no place for transformed weights)
  const ChainArgs a = chain_args(x, x_cstride, x_coff, n_img, Cin, relu_in, w1, b1, w2_packed, b2, w3, b3, K3, res, res_cstride, res_coff, y,
                                 y_cstride, y_coff);
  const char* why = nullptr;
  hipError_t e = chain14_launch(a, static_cast<hipStream_t>(stream), &why);
  if (e != hipSuccess) return fail(nullptr, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, why ? why : hipGetErrorString(e));
  return OFFK_OK;
}

int offk_bottleneck_chain14_split(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Cin, int relu_in,
                                  const float* w1, const float* b1, const float* w2_packed, const float* b2, const float* w3,
                                  const float* b3, const float* branch_w, const float* branch_b, const float* res, int res_cstride,
                                  int res_coff, float* y, int y_cstride, int y_coff, void* scratch, size_t scratch_bytes) {
  const char* who = "offk_bottleneck_chain14_split";
  if (!x || !w1 || !b1 || !w2_packed || !b2 || !w3 || !b3 || !y || !scratch || n_img < 1 || (Cin != 64 && Cin != 256) || (branch_w && !branch_b))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument");
  // the kernel loads x / res and stores y through raw pointers: every view must hold its slice, and y may alias neither input (a block's
  // stores would race with the other half-image block's halo reads of x, and with later blocks' residual loads)
  if (x_coff < 0 || y_coff < 0 || (res && res_coff < 0)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": negative channel offset");
  if (x_cstride < x_coff + Cin) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": x_cstride < x_coff + Cin");
  if (y_cstride < y_coff + 256) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": y_cstride < y_coff + 256");
  if (res && res_cstride < res_coff + 256) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": res_cstride < res_coff + 256");
  if (branch_w && res) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": the branch form takes no residual (res must be NULL)");
  {
    const size_t rows = (size_t)n_img * 196 * sizeof(float);
    const uintptr_t y0 = reinterpret_cast<uintptr_t>(y), y1 = y0 + rows * (size_t)y_cstride;
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), x1 = x0 + rows * (size_t)x_cstride;
    if (y0 < x1 && x0 < y1) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": y overlaps x (the chain does not run in place)");
    if (res) {
      const uintptr_t r0 = reinterpret_cast<uintptr_t>(res), r1 = r0 + rows * (size_t)res_cstride;
      if (y0 < r1 && r0 < y1) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": y overlaps res (the chain does not run in place)");
    }
  }
  const size_t e1 = (size_t)64 * Cin, e2 = (size_t)64 * 576, e3 = (size_t)256 * 64;
  if (scratch_bytes < 6 * (e1 + e2 + 2 * e3)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": scratch too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* sp = static_cast<char*>(scratch);
  ChainArgs a = chain_args(x, x_cstride, x_coff, n_img, Cin, relu_in, w1, b1, w2_packed, b2, w3, b3, 64, res, res_cstride, res_coff, y, y_cstride,
                           y_coff);
  a.w1p = sp; a.w2p = sp + 6 * e1; a.w3p = sp + 6 * (e1 + e2);
  hipError_t e = wino_pack_split_launch(w1, const_cast<void*>(a.w1p), 64, Cin, 1, st);
  if (e == hipSuccess) e = wino_pack_split_launch(w2_packed, const_cast<void*>(a.w2p), 64, 576, 1, st);
  if (e == hipSuccess) e = wino_pack_split_launch(w3, const_cast<void*>(a.w3p), 256, 64, 1, st);
  if (e == hipSuccess && branch_w) {
    a.wbp = sp + 6 * (e1 + e2 + e3); a.bbr = branch_b;
    e = wino_pack_split_launch(branch_w, const_cast<void*>(a.wbp), 256, 64, 1, st);
  }
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  const char* why = nullptr;
  e = chain14_split_launch(a, st, &why);
  if (e != hipSuccess) return fail(nullptr, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, std::string(who) + ": " + (why ? why : hipGetErrorString(e)));
  return OFFK_OK;
}

namespace {
// shared body of the three Winograd entry points: phases = 1 (3x3 / stride 1 on 7x7), 4 (polyphase 5x5 / stride 2 on 14x14) -- winograd.hip --
// or 7: the polyphase 7x7 / stride 2 conv on 28x28 maps, nine tiles per image (winograd7.hip; no residual, no pooled sums)
int winograd_entry(const char* who, void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Ci, int phases,
                   const float* w_packed, const float* bias, int Co, const float* res, int res_cstride, int res_coff, int flags,
                   float* y, int y_cstride, int y_coff, float* scratch, size_t scratch_floats, float* pool_part) {
  if (!x || !w_packed || !y || !scratch || n_img < 1 || Ci < 32 || (Ci & 31) || Co < 64 || (Co & 63) || (flags & OFFK_CONV_RELU_IN_))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument (Ci % 32 == 0, Co % 64 == 0, no RELU_IN)");
  const bool f54 = phases == 7;
  const size_t T = f54 ? (size_t)kWino7Tiles * n_img : (size_t)n_img;      // rows per batch entry
  const size_t units = f54 ? kWino7Units : phases == 4 ? kWinoUnits4 : kWinoPoints, points = f54 ? kWino7Points : kWinoPoints;   // row-Ci units of U / V
  const size_t need = units * Ci * ((size_t)Co + T) + points * T * Co;
  if (scratch_floats < need) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": scratch too small");
  hipStream_t st = static_cast<hipStream_t>(stream);
  float* U = scratch;
  float* V = U + units * Co * Ci;
  float* M = V + units * T * Ci;
  hipError_t e = f54 ? wino7_weight_launch(w_packed, Co, Ci, U, st) : wino_weight_launch(w_packed, Co, Ci, phases, U, st);
  if (e == hipSuccess) e = f54 ? wino7_input_launch(x, x_cstride, x_coff, n_img, Ci, V, st) : wino_input_launch(x, x_cstride, x_coff, n_img, Ci, phases, V, st);
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  WinoGroup grp[4];
  const int ngrp = f54 ? wino7_groups((long long)T, Ci, Co, grp) : wino_groups(phases, (long long)T, Ci, Co, grp);
  {
    const char* why = nullptr;
    e = wino_gemms_launch(grp, ngrp, (int)points, (int)T, Ci, Co, V, U, M, wino_gemm_stage_default(), st, &why);
    if (e != hipSuccess) return fail(nullptr, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, why ? why : hipGetErrorString(e));
  }
  e = f54 ? wino7_output_launch(M, n_img, Co, bias, flags, y, y_cstride, y_coff, st)
          : wino_output_launch(M, n_img, Co, phases, bias, res, res_cstride, res_coff, flags, y, y_cstride, y_coff, pool_part, st);
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  return OFFK_OK;
}
}  // namespace

int offk_winograd_conv3x3(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Ci, const float* w_packed,
                          const float* bias, int Co, const float* res, int res_cstride, int res_coff, int flags, float* y,
                          int y_cstride, int y_coff, float* scratch, size_t scratch_floats, float* pool_part) {
  return winograd_entry("offk_winograd_conv3x3", stream, x, x_cstride, x_coff, n_img, Ci, 1, w_packed, bias, Co, res, res_cstride,
                        res_coff, flags, y, y_cstride, y_coff, scratch, scratch_floats, pool_part);
}

int offk_winograd_conv5x5s2(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Ci, const float* w_packed,
                            const float* bias, int Co, const float* res, int res_cstride, int res_coff, int flags, float* y,
                            int y_cstride, int y_coff, float* scratch, size_t scratch_floats) {
  return winograd_entry("offk_winograd_conv5x5s2", stream, x, x_cstride, x_coff, n_img, Ci, 4, w_packed, bias, Co, res, res_cstride,
                        res_coff, flags, y, y_cstride, y_coff, scratch, scratch_floats, nullptr);
}

int offk_winograd_conv7x7s2(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Ci, const float* w_packed,
                            const float* bias, int Co, int flags, float* y, int y_cstride, int y_coff, float* scratch,
                            size_t scratch_floats) {
  return winograd_entry("offk_winograd_conv7x7s2", stream, x, x_cstride, x_coff, n_img, Ci, 7, w_packed, bias, Co, nullptr, 0, 0, flags, y, y_cstride,
                        y_coff, scratch, scratch_floats, nullptr);
}

int offk_winograd_between(void* stream, const float* M, const float* bias_in, int phases_in, int n_img, int Cin, float* x,
                          int x_cstride, int x_coff, const float* w1, const float* b1, int Cmid, float* V) {
  const char* who = "offk_winograd_between";
  if (!M || !V || n_img < 1 || (w1 && !b1) || (x && (x_cstride < x_coff + Cin || (x_cstride & 3) || (x_coff & 3) || x_coff < 0)))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument");
  if (!wino_mid_supported(Cin, Cmid, w1 != nullptr, phases_in))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": shape not built ((Cin, Cmid) = (128, 128) / (256, 256); phases_in 1, or 4 with Cin 128)");
  hipError_t e = wino_mid_launch(wino_mid_args(M, bias_in, phases_in, n_img, Cin, x, x_cstride, x_coff, w1, b1, Cmid, V), static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  return OFFK_OK;
}

int offk_winograd_between_ex(void* stream, const float* M, const float* bias_in, int phases_in, int n_img, int Cin, float* x,
                             int x_cstride, int x_coff, const float* w1, const float* b1, int Cmid, float* V, int precision,
                             void* scratch, size_t scratch_bytes) {
  const char* who = "offk_winograd_between_ex";
  if (precision == OFFK_PRECISION_FP32) return offk_winograd_between(stream, M, bias_in, phases_in, n_img, Cin, x, x_cstride, x_coff, w1, b1, Cmid, V);
  if (precision != OFFK_PRECISION_F32SPLIT || !w1 || !b1 || !scratch || scratch_bytes < (size_t)Cmid * Cin * 6)
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": split-fp32 needs the 1x1 conv and Cmid * Cin * 6 bytes of scratch");
  if (!M || !V || n_img < 1 || (x && (x_cstride < x_coff + Cin || (x_cstride & 3) || (x_coff & 3) || x_coff < 0)))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument");
  if (!wino_mid_supported(Cin, Cmid, true, phases_in))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": shape not built ((Cin, Cmid) = (128, 128) / (256, 256); phases_in 1, or 4 with Cin 128)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e = wino_pack_split_launch(w1, scratch, Cmid, Cin, 1, st);
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  e = wino_mid_launch(wino_mid_args(M, bias_in, phases_in, n_img, Cin, x, x_cstride, x_coff, w1, b1, Cmid, V, scratch), st);
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  return OFFK_OK;
}

int offk_batched_gemm_nt(void* stream, const float* x, const float* w, float* y, int batch, int M, int K, int Co, int precision,
                         void* scratch, size_t scratch_bytes) {
  const char* who = "offk_batched_gemm_nt";
  if (!x || !w || !y || batch < 1 || M < 1 || K < 32 || (K & 31) || Co < 64 || (Co & 63))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument (K % 32 == 0, Co % 64 == 0)");
  if (precision != OFFK_PRECISION_FP32 && precision != OFFK_PRECISION_F32SPLIT)
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": precision must be OFFK_PRECISION_FP32 or OFFK_PRECISION_F32SPLIT");
  hipStream_t st = static_cast<hipStream_t>(stream);
  WinoGroup grp{batch, 1, 0, 0, 0};
  const void* planes = nullptr;
  if (precision == OFFK_PRECISION_F32SPLIT) {
    if (K < 64) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": the split-fp32 form takes K >= 64");
    if (!scratch || scratch_bytes < (size_t)batch * Co * K * 6)
      return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": scratch smaller than batch * Co * K * 6 bytes (the plane image of w)");
    hipError_t e = wino_pack_split_launch(w, scratch, Co, K, batch, st);
    if (e != hipSuccess) return fail_hip(nullptr, e, who);
    planes = scratch;
  }
  const char* why = nullptr;
  hipError_t e = wino_gemms_launch(&grp, 1, batch, M, K, Co, x, w, y, true, st, &why, planes);
  if (e != hipSuccess) return fail(nullptr, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, std::string(who) + ": " + (why ? why : hipGetErrorString(e)));
  return OFFK_OK;
}

int offk_set_conv_plan(offk_handle* h, const char* conv_key, int tile_cfg, int splitk) {
  if (!h || !conv_key) return fail(h, OFFK_ERR_INVALID, "offk_set_conv_plan: null argument");
  for (int c = 0; c < kNumConvs; ++c)
    if (!strcmp(kConvs[c].key, conv_key)) {
      h->conv_cfg[c] = tile_cfg < 0 ? -1 : tile_cfg;
      h->conv_splitk[c] = splitk < 1 ? 0 : splitk;
      return OFFK_OK;
    }
  for (int m = 0; m < 3; ++m)
    if (!strcmp(kMerged[m].name, conv_key)) {
      h->merged_cfg[m] = tile_cfg < 0 ? -1 : tile_cfg;
      h->merged_sk[m] = splitk < 1 ? 0 : splitk;
      return OFFK_OK;
    }
  return fail(h, OFFK_ERR_UNKNOWN_KEY, std::string("offk_set_conv_plan: unknown conv ") + conv_key);
}

int offk_pack_conv_weight(void* stream, const float* w_oihw, int Co, int Ci, int KH, int KW, float* w_ohwi) {
  if (!w_oihw || !w_ohwi || Co < 1 || Ci < 32 || (Ci & 31) || KH < 1 || KW < 1) return fail(nullptr, OFFK_ERR_INVALID, "offk_pack_conv_weight: bad argument (Ci % 32 == 0)");
  hipError_t e = pack_conv_weight_launch(w_oihw, Co, Ci, KH, KW, w_ohwi, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, "offk_pack_conv_weight");
  return OFFK_OK;
}

int offk_head(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int C, int maxpool,
              const float* fc_w, const float* fc_b, int num_classes, float* out) {
  if (!x || !fc_w || !fc_b || !out) return fail(nullptr, OFFK_ERR_INVALID, "offk_head: null argument");
  const char* why = nullptr;
  hipError_t e = head_launch(x, x_cstride, x_coff, n_img, H, W, C, maxpool, fc_w, fc_b, num_classes, out,
                             static_cast<hipStream_t>(stream), &why);
  if (e != hipSuccess) return fail(nullptr, why ? OFFK_ERR_INVALID : OFFK_ERR_HIP, why ? why : hipGetErrorString(e));
  return OFFK_OK;
}

// ---- K5t / K5b: training side of one classifier head (head_bwd.hip) ----
namespace {
// what offk_head_train and offk_head_backward share: the domain of K5 plus the dropout arguments
int head_train_shape(const char* who, int n_img, int H, int W, int C, int maxpool, int num_classes, int head_index, double drop_p) {
  if (n_img < 1 || H < 1 || W < 1 || num_classes < 1) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": bad argument (n_img, H, W, num_classes >= 1)");
  if (C < 4 || C > 1024 || C % 4) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": need 4 <= C <= 1024 and C % 4 == 0");
  if (maxpool && (H < 3 || W < 3)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": maxpool needs H, W >= 3");
  if (head_index < 0 || head_index > 239) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": head_index must be in [0, 239] (0 / 1 / 2: the 28 / 14 / 7 head)");
  if (!(drop_p >= 0.0) || drop_p >= 1.0) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": dropout probability must be in [0, 1)");
  if ((long long)n_img * H * W > 0x7fffffffLL || (long long)n_img * num_classes > 0x7fffffffLL)
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": problem too large");
  return OFFK_OK;
}
bool bytes_overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
}  // namespace

int offk_head_backward_plan(int n_img, int C, int num_classes, size_t* scratch_bytes, int* chunks) {
  const char* who = "offk_head_backward_plan";
  size_t sf = 0;
  int ch = 0;
  if (!head_bwd_plan(n_img, C, num_classes, &sf, &ch))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": need n_img >= 1, 4 <= C <= 1024, C % 4 == 0, num_classes >= 1");
  if (scratch_bytes) *scratch_bytes = sf * sizeof(float);
  if (chunks) *chunks = ch;
  return OFFK_OK;
}

int offk_head_train(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int C, int maxpool, const float* fc_w,
                    const float* fc_b, int num_classes, int head_index, uint64_t drop_seed, double drop_p, float* z, float* out) {
  const char* who = "offk_head_train";
  if (!fc_w || !fc_b || !z || !out) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": null pointer");
  if (int rc = head_train_shape(who, n_img, H, W, C, maxpool, num_classes, head_index, drop_p)) return rc;
  if (const char* w = view_problem(x, x_cstride, x_coff, C)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": x: " + w);
  hipError_t e = head_train_launch(x, x_cstride, x_coff, n_img, H, W, C, maxpool != 0, fc_w, fc_b, num_classes, head_index, drop_seed, drop_p, z,
                                   out, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, who);
  return OFFK_OK;
}

int offk_head_backward(void* stream, const float* g, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int C, int maxpool,
                       const float* fc_w, int num_classes, const float* z, int head_index, uint64_t drop_seed, double drop_p, float* dx,
                       int dx_cstride, int dx_coff, int accumulate_dx, float* dw, float* db, int accumulate_w, void* scratch,
                       size_t scratch_bytes) {
  const char* who = "offk_head_backward";
  if (!g) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": null pointer (g)");
  if (dx && !fc_w) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": null pointer (fc_w, needed for dx)");
  if (dw && !z) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": null pointer (z, needed for dw)");
  if ((dw || db) && !scratch) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": null pointer (scratch, needed for dw and db)");
  if (int rc = head_train_shape(who, n_img, H, W, C, maxpool, num_classes, head_index, drop_p)) return rc;
  if (dx) {
    if (const char* w = view_problem(x, x_cstride, x_coff, C)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": x: " + w);
    if (const char* w = view_problem(dx, dx_cstride, dx_coff, C)) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": dx: " + w);
    const size_t rows = (size_t)n_img * H * W, dx_bytes = rows * (size_t)dx_cstride * sizeof(float);
    if (bytes_overlap(dx, dx_bytes, x, rows * (size_t)x_cstride * sizeof(float))) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": dx overlaps x");
    if (bytes_overlap(dx, dx_bytes, g, (size_t)n_img * num_classes * sizeof(float))) return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": dx overlaps g");
  }
  size_t sf = 0;
  int chunks = 0;
  head_bwd_plan(n_img, C, num_classes, &sf, &chunks);
  if ((dw || db) && scratch_bytes < sf * sizeof(float))
    return fail(nullptr, OFFK_ERR_INVALID, std::string(who) + ": scratch too small (offk_head_backward_plan)");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dx) {
    hipError_t e = head_bwd_data_launch(g, x, x_cstride, x_coff, n_img, H, W, C, maxpool != 0, fc_w, num_classes, head_index, drop_seed, drop_p, dx,
                                        dx_cstride, dx_coff, accumulate_dx != 0, st);
    if (e != hipSuccess) return fail_hip(nullptr, e, who);
  }
  if (dw || db) {
    hipError_t e = head_bwd_weight_launch(g, z, n_img, C, num_classes, dw, db, accumulate_w != 0, static_cast<float*>(scratch), chunks, st);
    if (e != hipSuccess) return fail_hip(nullptr, e, who);
  }
  return OFFK_OK;
}

int offk_segment_consensus(void* stream, const float* x, int B, int T, int C, float* out) {
  if (!x || !out || B < 1 || T < 1 || C < 1) return fail(nullptr, OFFK_ERR_INVALID, "offk_segment_consensus: bad argument");
  hipError_t e = consensus_launch(x, B, T, C, out, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, "offk_segment_consensus");
  return OFFK_OK;
}

int offk_score_fusion(void* stream, const float* const* scores, const float* weights, int n_sets, int videos, int crops,
                      int classes, float* fused, int32_t* pred) {
  if (!scores || !weights || !fused || n_sets < 1 || n_sets > 8 || videos < 1 || crops < 1 || classes < 1)
    return fail(nullptr, OFFK_ERR_INVALID, "offk_score_fusion: bad argument (1..8 score sets)");
  for (int i = 0; i < n_sets; ++i)
    if (!scores[i]) return fail(nullptr, OFFK_ERR_INVALID, "offk_score_fusion: null score set");
  hipError_t e = score_fusion_launch(scores, weights, n_sets, videos, crops, classes, fused, pred, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, "offk_score_fusion");
  return OFFK_OK;
}

int offk_nchw_to_nhwc(void* stream, const float* src, int n_img, int C, int HW, float* dst) {
  if (!src || !dst || n_img < 1 || n_img > 65535 || C < 1 || HW < 1) return fail(nullptr, OFFK_ERR_INVALID, "offk_nchw_to_nhwc: bad argument");
  hipError_t e = nchw_to_nhwc_launch(src, n_img, C, HW, dst, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, "offk_nchw_to_nhwc");
  return OFFK_OK;
}

int offk_nhwc_to_nchw(void* stream, const float* src, int cstride, int coff, int n_img, int C, int HW, float* dst) {
  if (!src || !dst || n_img < 1 || n_img > 65535 || C < 1 || HW < 1 || coff < 0 || coff + C > cstride)
    return fail(nullptr, OFFK_ERR_INVALID, "offk_nhwc_to_nchw: bad argument");
  hipError_t e = nhwc_to_nchw_launch(src, cstride, coff, n_img, C, HW, dst, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail_hip(nullptr, e, "offk_nhwc_to_nchw");
  return OFFK_OK;
}

}  // extern "C"
