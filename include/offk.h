/*
 * offk.h -- C ABI of liboffk.so: the MI355X-native OFF sub-network forward.
 *
 * The reference (JoeHEZHAO/Optical-Flow-Guided-Feature-Pytorch) has NO plugin /
 * operator / FFI boundary for this path: the OFF sub-network is inline Python inside
 * BNInception_OFF.RGB_OFF_forward (RGB_OFF.py:360-860, OFF part :596-847) and
 * BNInception_OFF.forward (Flow_OFF.py:370-887, OFF part :606-876).  The cut this
 * library replaces is therefore the set of nine local tensors
 * inception_{3a,3b,3c,4a,4b,4c,4d,5a,5b}_output_out (RGB_OFF.py:395,418,435,458,481,
 * 504,527,567,590) on the way in and fc_action_motion{,_14,_28} (RGB_OFF.py:787,793,
 * 847) on the way out.  Each entry point below cites the reference lines it stands for.
 *
 * Conventions
 *  - plain C types only; every function returns 0 (OFFK_OK) or a negative error code
 *    and never throws; offk_last_error() gives the message.
 *  - the caller owns every data buffer (device pointers, e.g. torch tensor.data_ptr());
 *    the library owns the handle and its packed weight copies only.
 *  - all work is enqueued asynchronously on the hipStream_t passed as `void* stream`
 *    (NULL = default stream); there is no implicit synchronisation and no other stream: every launch of a call goes to
 *    `stream` in order, so the call can be stream-captured (ABI v8: the handle-owned side stream of v5 - v7 is gone).
 *  - offk_forward runs the units as ONE kernel that fuses the 1x1 reduces with the temporal difference (the gen output G
 *    never goes to HBM) plus the spatial half of K2; OFFK_FUSED_UNITS=0 in the environment at offk_create selects the
 *    two-kernel form (K1 then K2), which offk_off_units / offk_off_units_train always use (the backward needs G).  Both
 *    give the same values (to 2e-6 in fp32: the fused kernel sums k in another grouping).
 *  - a handle is not thread-safe; distinct handles are independent.
 *  - fp32 everywhere (16-bit feature maps: offk_forward_typed).  Boundary tensors are NCHW contiguous exactly as the reference
 *    backbone produces them (a channels_last backbone's NHWC-strided maps, fp32 or 16-bit: offk_forward_cl, and on the
 *    training side offk_off_units_train_cl / offk_off_units_backward_cl, layout per call);
 *    INTERNAL activations (workspace, stage entry points) are
 *    channels-last: [rows = image*H*W + y*W + x][channels], see DESIGN.md.
 */
#ifndef OFFK_H_
#define OFFK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OFFK_ABI_VERSION 10
#define OFFK_NUM_SITES 9 /* 3a 3b 3c 4a 4b 4c 4d 5a 5b */

enum offk_status {
  OFFK_OK = 0,
  OFFK_ERR_INVALID = -1,        /* bad argument / shape */
  OFFK_ERR_HIP = -2,            /* a HIP runtime call failed */
  OFFK_ERR_MISSING_WEIGHT = -3, /* forward called before every weight was set */
  OFFK_ERR_UNKNOWN_KEY = -4,    /* state_dict key not part of the OFF sub-network */
  OFFK_ERR_NO_DEVICE = -5       /* no gfx950 device visible */
};

enum offk_variant {
  OFFK_VARIANT_RGB_LEARNED_DW = 0, /* RGB_OFF.py: learned depthwise 3x3 + bias (:268,611) */
  OFFK_VARIANT_DIAG_SOBEL = 1      /* Flow_OFF.py:51,622 / RGB_OFF_v2.py:58: util.SobelFilter_Diagonal */
};
enum offk_slice_mode {
  OFFK_SLICE_REFERENCE_FLAT = 0, /* spatial branch = X[:B*(L-1)] on the flat frame axis (RGB_OFF.py:609) */
  OFFK_SLICE_PER_CLIP = 1        /* drop each clip's last frame (what the comment at :608 says) */
};
enum offk_consensus {
  OFFK_CONSENSUS_NONE = 0, /* RGB_OFF.py:849-860: per-pair logits [B*(L-1), classes] */
  OFFK_CONSENSUS_AVG = 1   /* Flow_OFF.py:867-876 / basic_ops.py:19-21: mean over L-1 -> [B, classes] */
};
enum offk_feat_layout {
  OFFK_FEAT_NCHW = 0, /* what the reference backbone's torch.cat produces */
  OFFK_FEAT_NHWC = 1  /* channels_last physical layout of the same logical tensor */
};

enum offk_precision {
  OFFK_PRECISION_FP32 = 0,  /* v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate */
  /* (1 was OFFK_PRECISION_BF16X3 until ABI v8: each fp32 operand as TWO bf16 planes, three products, ~1e-5 of the fp32 path;
   *  retired in ABI v9 -- offk_create rejects it -- in favour of the exact three-plane mode below) */
  OFFK_PRECISION_F32SPLIT = 2 /* fp32 arithmetic on the bf16 matrix pipe: each fp32 operand cut into THREE bf16 planes by
                               truncation (h = the upper 16 bits, the exact remainder cut again: 8 + 8 + 8 significand bits
                               = the fp32 value exactly), six of the nine plane products (w_h x_h, w_h x_m, w_m x_h, w_m x_m,
                               w_h x_l, w_l x_h) on v_mfma_f32_16x16x32_bf16 with fp32 accumulation -- in every split
                               kernel (units, batched GEMMs, chains, the 1x1 of winograd_between) the leading product in
                               one running accumulator and the five small ones in another, added once at the end.
                               Contract: the dropped products w_m x_l + w_l x_m + w_l x_l are below
                               (2^-21 + 2^-30) sum_k |w_k x_k| per output (|m| < 2^-7 |v|, |l| < 2^-15 |v| for the
                               truncating cut; reached within 3 % when both operands carry mantissa 0x00FFFF), beside an
                               fp32 accumulation error.  On the parity distributions (synthetic maps, 24-bit mantissas,
                               heavy tail, cancellation) the measured error against fp64 is no larger than the fp32 pipe's
                               own; on worst-case mantissas that comparison does not hold -- there the
                               bound above is what is tested, dropped and accumulation parts separately
                               (tests/test_split_contract.py on the CPU, tests/test_gpu_split.py::test_*_worst_case_mantissas).
                               Kernels that have no split form run exactly as in OFFK_PRECISION_FP32.
                               Non-finite inputs: the cut of +-Inf leaves Inf - Inf = NaN in the lower planes, so every
                               output such an operand touches is NaN where the fp32 pipe gives +-Inf (or NaN): non-finite
                               in both modes, but not the same non-finite value.  Tiny inputs: a plane below the bf16
                               normal range is a bf16 subnormal, which the MFMA honours (tools/probe_split_mfma.hip part
                               2); a plane below 2^-133 (the last bf16 subnormal) is lost -- only operands below 2^-109
                               in magnitude have such planes (tests/test_gpu_split.py::test_split_nonfinite_and_tiny_inputs). */
};

typedef struct offk_config {
  int32_t batch;       /* B clips            (BNInception_OFF.batch,  RGB_OFF.py:35) */
  int32_t length;      /* L segments / clip  (BNInception_OFF.length, RGB_OFF.py:36), >= 2 */
  int32_t variant;     /* enum offk_variant */
  int32_t slice_mode;  /* enum offk_slice_mode */
  int32_t consensus;   /* enum offk_consensus */
  int32_t num_classes; /* 101 (RGB_OFF.py:332-334) */
  int32_t feat_layout; /* enum offk_feat_layout */
  int32_t device;      /* HIP device ordinal the handle lives on */
  int32_t precision;   /* enum offk_precision: arithmetic of the contractions (1x1 reduce, fusion convs) */
} offk_config;

typedef struct offk_handle offk_handle;

int offk_abi_version(void);

/* Message for the last error on `h` (or, with h == NULL, the last error of a failed
 * offk_create / handle-less call on this thread).  Never NULL. */
const char* offk_last_error(const offk_handle* h);

/* Replaces: BNInception_OFF.__init__ motion_* declarations (RGB_OFF.py:265-358). */
int offk_create(const offk_config* cfg, offk_handle** out);
int offk_destroy(offk_handle* h);

/* Replaces: load_state_dict for the motion_*, fc_action_motion* and sobel_edge_diagonal
 * keys (model_utils.py:188-216, Flow_OFF.py:1398-1413).  `key` is the reference
 * state_dict key (an optional "module." prefix is ignored, test_flow_off.py:52-58);
 * `data` may be a host or a device pointer; shape is checked against the reference's.
 * The library keeps its own packed device copy.  Blocking, load-time call: it first waits for all work on the device
 * (so no kernel still reads the copy being replaced and a device-side `data` is complete whatever stream produced it).
 * The copy and every image derived from it (the operand-order images of the units kernels, the merged matrices, the Winograd,
 * chain, plane and composed-head images) are handle-owned and made again IN PLACE: the copy by this call, the images by the
 * first forward enqueued after it.  A captured forward (HIP graph) therefore sees a later offk_set_weight once one forward has
 * passed through the library after it, and not before: until then a replay reads the new copy beside images of the old weight.
 * Two updates change the launches themselves, which a graph fixes at capture, and need a re-capture: a sobel_edge_diagonal weight
 * that leaves or enters the four-tap form of util.py:61 (the host picks the four-tap or the nine-tap kernel from its values at
 * every launch; a graph captured on the four-tap kernel goes on ignoring the other five taps), and offk_set_weight on a key bound
 * with offk_bind_weight (the bound pointer, and for a gen / down weight the register-staged units kernel, stay in the graph). */
int offk_set_weight(offk_handle* h, const char* key, const float* data, const int64_t* shape, int ndim);
/* Training-side alternative for the parameters that change every optimizer step.  (train_off.py:39-45 un-freezes every tensor
 * whose name contains "motion" or "fc_action_motion" -- the units, the fusion stages and the heads; the OFF UNITS' share of
 * those, which this library trains, is motion_conv_gen_<s>, motion_spatial_down_<s>, motion_spatial_grad_<s>, weight and bias):
 * bind the caller's own parameter storage instead of copying it.  `device_data` is the tensor in the reference layout of
 * the key ([128,C,1,1], [128], [32,C,1,1], [32], [32,1,3,3], [32]; contiguous, 16-byte aligned, on the handle's device);
 * every later launch reads it in place, so an in-place optimizer update needs NO call at all -- it only has to be ordered
 * before the next launch, which it is when both are enqueued on the same stream.  The caller keeps the storage alive and
 * re-binds if the tensor is re-allocated.  A later offk_set_weight of the same key replaces the binding by a copy.
 * Binding ANY gen / down weight moves all nine sites off the operand-order weight images of the fused units kernels (the library's
 * own packed copies: the fp32 form's and the split-fp32 form's) onto the register-staged fp32 kernel that reads the bound tensors.
 * `shape` / `ndim` are checked against the key's reference shape, and the allocation behind `device_data` must hold that
 * many bytes (hipMemGetAddressRange): every later launch sizes its buffer descriptors from the key, not from the tensor.
 * Not blocking, no allocation, no kernel launch. */
int offk_bind_weight(offk_handle* h, const char* key, const float* device_data, const int64_t* shape, int ndim);
/* Number of weights still unset (0 = ready); if buf != NULL the first missing key is copied there. */
int offk_missing_weights(const offk_handle* h, char* buf, size_t buflen);

/* Bytes of caller-provided device scratch offk_forward needs for this (B, L). */
size_t offk_workspace_bytes(const offk_handle* h);

/* Replaces: RGB_OFF.py:596-847 / Flow_OFF.py:606-876 (nine OFF units, fusion @28/@14/@7,
 * three heads, optional SegmentConsensus).
 *   feats[i]: site i feature map, [B*L, C_i, H_i, H_i] fp32 (layout per cfg.feat_layout)
 *   out7/out14/out28: [rows, num_classes] fp32, rows = B*(L-1) (consensus none) or B (avg);
 *   out28 may be NULL (the reference computes it but never returns it, RGB_OFF.py:860). */
int offk_forward(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES],
                 float* out7, float* out14, float* out28, void* workspace);

/* Same forward with every feature map handed over as its 1..4 channel groups in concat order --
 * the inception block's branch outputs BEFORE the torch.cat that builds inception_*_output_out
 * (RGB_OFF.py:395,418,435,458,481,504,527,567,590) -- so the backbone can skip that copy (31.6 MB
 * written + re-read per clip).  Group p of site i is [B*L, channels[p], H_i, H_i] (layout per
 * cfg.feat_layout), channels[p] % 32 == 0 (true for every BN-Inception branch), sum = C_i. */
typedef struct offk_feat_parts {
  int32_t n_parts;      /* 1..4 */
  int32_t channels[4];
  const float* data[4];
} offk_feat_parts;
int offk_forward_parts(offk_handle* h, void* stream, const offk_feat_parts parts[OFFK_NUM_SITES],
                       float* out7, float* out14, float* out28, void* workspace);

/* 16-bit feature maps (ABI v10, additive).  A backbone run under torch.autocast hands the nine maps over in fp16 (autocast's
 * default) or bf16; these entries take them as they are, with no fp32 copy.
 *   feat_dtype OFFK_FEAT_F32: exactly offk_forward / offk_forward_parts / offk_off_units_fused (feats cast to const float*).
 *   OFFK_FEAT_BF16 / OFFK_FEAT_F16: feats[i] (and offk_feat_parts.data[q], which then holds the address of 16-bit elements cast
 *   to const float*) point at [B*L, C_i, H_i, H_i] NCHW maps of that type, 4-byte aligned (the units kernel reads the 28x28 and
 *   14x14 sites as pixel pairs).  Outputs, workspace (offk_workspace_bytes is unchanged) and stream rules are offk_forward's:
 *   no synchronisation and no allocation on the call, stream-capturable.
 * Contract: for FINITE maps the three heads and the workspace regions the units fill (the unit channels of fusion_28/14/7,
 * D_<site>) are EQUAL, element for element (only the sign of a zero may differ), to what the same handle computes from
 * x.float() -- not a new tolerance.  Why: a bf16 value is exactly its own leading bf16 plane (x_m = x_l = +0), an fp16 value
 * (11 significant bits, subnormals included: each is a normal number in bf16's exponent range) exactly two (x_l = +0).  The
 * fp32-map units kernel issues per output tile and 32-k group, into A2: w_l x_h, w_h x_l, w_m x_m, w_m x_h, w_h x_m, then
 * into A1: w_h x_h; the products of a +0 plane are +-0.  The 16-bit kernel (csrc/pw_tdiff_f16.hip: its loader on the block
 * body of csrc/pw_tdiff_staged.h, which the channels-last kernel below shares) issues the other MFMAs --
 * bf16 three, fp16 five -- with the same k in the same operand slots, in the same order, into the same two accumulators,
 * from the same weight plane image, and ends in the same epilogue; every launch after it is the fp32-map path's, on the
 * same buffers.  Non-finite maps are outside the equality: every output a non-finite value touches is non-finite, as in
 * the split mode.
 * Refused with OFFK_ERR_INVALID before anything is enqueued: an unknown feat_dtype; a 16-bit dtype on an
 * OFFK_PRECISION_FP32 handle; an NHWC handle; a handle created with OFFK_FUSED_UNITS=0; any gen / down weight bound
 * through offk_bind_weight; a data pointer that is not 4-byte aligned. */
enum offk_feat_dtype { OFFK_FEAT_F32 = 0, OFFK_FEAT_BF16 = 1, OFFK_FEAT_F16 = 2 };
int offk_forward_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                       float* out7, float* out14, float* out28, void* workspace);
int offk_forward_parts_typed(offk_handle* h, void* stream, int feat_dtype, const offk_feat_parts parts[OFFK_NUM_SITES],
                             float* out7, float* out14, float* out28, void* workspace);

/* Channels-last feature maps (ABI v10, additive).  A backbone run in torch.channels_last hands the nine maps over with NHWC
 * strides; these entries take them as they are, with no copy, for every feat_dtype.  The layout is a property of the CALL:
 * cfg.feat_layout keeps describing what the entries above are given and is ignored here.
 *   feats / parts as in the _typed entries, but every map (part) is physically channels-last: [B*L*H_i*H_i][C_i] (part q:
 *   [B*L*H_i*H_i][channels[q]]), elements of feat_dtype (OFFK_FEAT_F32 / _BF16 / _F16), 16-byte aligned.  Outputs, workspace
 *   (offk_workspace_bytes is unchanged) and stream rules are offk_forward's: no synchronisation and no allocation on the call,
 *   stream-capturable.
 * Contract: for FINITE maps the three heads and the workspace regions the units fill are EQUAL, element for element, to what
 * the same handle computes through offk_forward / offk_forward_typed from the NCHW copy of the same logical tensor -- not a
 * new tolerance.  Why: the channels-last units kernel (csrc/pw_tdiff_cl.hip: its loader on the block body of
 * csrc/pw_tdiff_staged.h, the 16-bit kernel's) puts the same k into the same operand slots
 * (K-tile kt, lane group g, element e <-> channel 32 kt + 8 g + e of the part that holds it), cuts the values the same way,
 * multiplies them with the same weight plane image in the same order into the same two accumulators (fp32 maps six MFMAs per
 * tile and 32-k group, fp16 five, bf16 three) and ends in the same epilogue; only the loader differs: the eight k of a lane's
 * B operand are 16 or 32 contiguous bytes of a channels-last map.  Every launch after the units is the existing path.
 * Refused with OFFK_ERR_INVALID before anything is enqueued: null arguments; an unknown feat_dtype; a handle that is not
 * OFFK_PRECISION_F32SPLIT; a handle created with OFFK_FUSED_UNITS=0; any gen / down weight bound through offk_bind_weight; a
 * data pointer that is not 16-byte aligned; channel groups offk_forward_parts refuses. */
int offk_forward_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                    float* out7, float* out14, float* out28, void* workspace);
int offk_forward_parts_cl(offk_handle* h, void* stream, int feat_dtype, const offk_feat_parts parts[OFFK_NUM_SITES],
                          float* out7, float* out14, float* out28, void* workspace);

/* Named regions of the workspace after offk_forward (for stage-level parity tests):
 * "G_<site>", "D_<site>", "fusion_28", "fusion_14", "fusion_7", "sum_7".  All channels-last.
 * "sum_7" (motion_sum of RGB_OFF.py:839-841) is filled after a forward, or -- on a handle at or above the gate of
 * OFFK_POOL_FIRST_7 (96 frame pairs by default), whose forward takes the 7-head from pooled sums of "xv_7" and never forms
 * motion_sum -- after offk_stage_tensors. */
int offk_workspace_region(const offk_handle* h, const char* name, size_t* offset_bytes, size_t* nbytes);

/* Fills the stage tensors the last forward on `h` left out: today "sum_7" on handles that take the 7-head pool-first
 * (RGB_OFF.py:839-847 is linear from [t2 | x2] to the logits; the merged 1x1 conv then runs only here, from "xv_7" in
 * `workspace`, the launch and plan the forward would have used, so the bits are those of a handle below the gate).  Enqueued on
 * `stream`, which must be ordered behind that forward.  Every forward that skipped the launch sets a pending flag on the
 * handle, this call clears it; with nothing pending it enqueues nothing and returns OFFK_OK.  (A forward replayed from a
 * captured graph does not pass through the library and sets no flag.) */
int offk_stage_tensors(offk_handle* h, void* stream, void* workspace);

/* Per-stage device timing.  When enabled, offk_forward brackets each stage with HIP
 * events on the caller's stream; offk_stage_times synchronises those events and
 * returns accumulated milliseconds + launch counts since the last reset.
 * Stage order: 0 pw_reduce (K1), 1 sobel_tdiff (K2), 2 fusion_28, 3 fusion_14,
 * 4 fusion_7, 5 heads+consensus. */
#define OFFK_NUM_STAGES 6
int offk_set_profiling(offk_handle* h, int enable);   /* 0 off, 1 per-stage events, 2 per-launch trace (below) */
int offk_stage_times(offk_handle* h, double ms[OFFK_NUM_STAGES], int64_t calls[OFFK_NUM_STAGES], int reset);
/* Per-launch trace (offk_set_profiling(h, 2)): offk_forward records one HIP event on the caller's stream in front of every
 * launch group -- the units kernels, each fusion conv by its state_dict name (a split-K conv includes its reduction), each
 * head, the consensus.  Returns the number of distinct groups seen since
 * the last reset; the first min(n, max_entries) are written: names as one '\n'-separated string into `names`, accumulated
 * milliseconds and call counts into `ms` / `calls`.  An event between two short kernels costs a few microseconds of
 * command-processor time: use rocprofv3's kernel trace for absolute times of the small launches. */
int offk_launch_times(offk_handle* h, char* names, size_t names_len, double* ms, int64_t* calls, int max_entries, int reset);

/* ---- stage entry points (the same kernels offk_forward launches) ------------------ */

/* Size limits of the entries below ("Size limits"; tests/test_gpu_big_slabs.py runs every strided view with its last
 * rows past 2 GiB and past 4 GiB, tests/test_gpu_big_batch.py the units at N = 2142).  A view is (pointer, cstride, coff, rows);
 * its byte extent is rows * cstride * 4.  "any extent": every row index times a stride is a 64-bit product in the kernels.
 *   offk_conv2d / offk_conv2d_ex       x, y, res: any extent (x below 2^31 - 1 bytes: buffer-descriptor loader, else the pointer
 *                                      loader; y below 0x7f000000 bytes without a residual: buffer stores, else pointer stores);
 *                                      n_img * Ho * Wo <= 2^31 - 257 rows, else OFFK_ERR_INVALID "conv2d: bad problem size"
 *   offk_bottleneck_chain14            x: (n_img * 196 * x_cstride - x_coff) * 4 < 2^31 - 1 bytes, else OFFK_ERR_INVALID "chain14: input
 *                                      beyond 31-bit byte offsets"; y, res: any extent
 *   offk_bottleneck_chain14_split      x as above and n_img * 196 * y_cstride * 4 < 0x7fffff00 bytes, else OFFK_ERR_INVALID "... input
 *                                      and output below 2^31 bytes"; res: any extent
 *   offk_winograd_conv3x3 / 5x5s2 / 7x7s2, offk_winograd_between / _ex     x, y, res: any extent
 *   offk_head, offk_head_train, offk_head_backward                         x, dx: any extent; n_img * H * W and n_img * num_classes <= 2^31 - 1
 *   offk_relu_backward                 dy, y, g: any extent
 *   offk_conv2d_backward_data / _weight / _weight_split, offk_conv2d_s2_backward_data / _data_split / _weight / _weight_split
 *                                      x, g, dx: any extent; the padded positions n_img * (H + 2) * (W + 2) (and n_img * H * W) stay
 *                                      below 2^31 less a tile, else OFFK_ERR_INVALID "problem too large"
 *   offk_nhwc_to_nchw                  src: any extent; n_img <= 65535
 *   offk_sobel_tdiff                   M (m_cstride, m_coff): any extent
 *   offk_pw_reduce, offk_off_units, offk_off_units_fused, offk_forward, offk_forward_parts (fp32 maps)
 *                                      a map part of 0x7fffff00 bytes or more (site 3b from N = 2140 frames) moves the WHOLE launch from
 *                                      the buffer-descriptor kernels to the pointer-loader kernels (pw_reduce_kernel<0, 0>,
 *                                      pw_tdiff_kernel<0, 0>).  These are fp32 kernels: an OFFK_PRECISION_F32SPLIT handle computes its
 *                                      units in exact fp32 arithmetic, not split-fp32, from that size on (same contract, other bits); handing the
 *                                      maps over as parts below that size (offk_forward_parts) keeps the split-fp32 kernel.
 *   offk_off_units_train, offk_off_units_backward, offk_off_units_backward_feats (fp32 maps, and their _split forms)
 *                                      any extent: K1 / K2 as above, K2b / K1b and the dX kernel index with 64-bit products (units_bwd.hip,
 *                                      units_dx.hip, units_wgrad_split.hip, units_fwd_split.hip, units_dx_split.hip: no buffer descriptor).
 *                                      Run at N = 2142 (the fp32 forms).
 *   16-bit maps, training side         offk_pw_reduce_typed, offk_off_units_typed, _train_typed, _backward_typed refuse a map of 0x7fffff00
 *                                      bytes or more (3b from N = 4280 frames) before anything is enqueued: "16-bit feature maps of 2 GiB or
 *                                      more are not supported (site 3b)".  Tested at B = 612.
 *   offk_forward_typed / _cl, offk_off_units_fused_typed / _cl
 *                                      any extent: the 16-bit and channels-last units kernels are pointer loaders with 64-bit products
 *                                      (pw_tdiff_f16.hip, pw_tdiff_cl.hip, pw_tdiff_staged.h).  offk_forward_typed is run at B = 612 (3b as
 *                                      bf16 / fp16 = 2.15 GB, fusion_28 3.7 GB, the Winograd V array 9.5 GB).
 *   offk_pw_reduce_cl, offk_off_units_cl, and offk_pw_reduce / offk_off_units / offk_forward on an OFFK_FEAT_NHWC handle (fp32 maps)
 *                                      any extent: mode 2 of pw_reduce_kernel<0, 0>, (size_t)row * cpart (pw_reduce.hip:222-227); read,
 *                                      not run at 2 GiB by any test.
 *   offk_create                        batch * length * 784 * 320 <= 2^31 - 1 (N <= 8559 frames), else OFFK_ERR_INVALID "offk_create:
 *                                      batch*length too large for one call; shard the clips"
 * offk_forward / offk_forward_parts / offk_stage_tensors are run at N = 2142 too (the Winograd V array of the 7x7 / 2 conv is 4.76 GB
 * there: the transforms index it with 64-bit products, the batched GEMMs take one descriptor per problem). */

/* K1. Replaces motion_conv_gen_<s> + motion_relu_gen_<s> on all N frames and
 * motion_spatial_down_<s> on the sliced frames (RGB_OFF.py:597-598, 609-610), stacked so
 * the map is read once.  G: [N*HW, 128] (post-ReLU), D: [P*HW, 32] channels-last. */
int offk_pw_reduce(offk_handle* h, void* stream, int site, const float* feat, float* G, float* D);

/* K2. Replaces the temporal subtraction (RGB_OFF.py:599-604), the depthwise 3x3 /
 * diagonal Sobel (RGB_OFF.py:611; Flow_OFF.py:622 + util.py:52-77) and the concats
 * (RGB_OFF.py:616,656,760,832): writes [spatial 32 | temporal 128] into channels
 * [m_coff, m_coff+160) of M, a channels-last buffer with m_cstride channels per pixel.
 * algo: temporal difference by 0 = register rotation over t (default), 1 = t across lanes + wavefront shuffle,
 * 4 = flat shifted stream (T_row[r] = G_row[r + HW] - G_row[r] within a clip; every frame read twice, second time from cache);
 * 2 / 3 / 5 = diagnostics for bandwidth attribution (temporal half only with rotation / spatial half only / temporal
 * half only, flat form). */
int offk_sobel_tdiff(offk_handle* h, void* stream, int site, const float* G, const float* D,
                     float* M, int m_cstride, int m_coff, int algo);

/* K2 alone for all nine sites in ONE grouped launch (exactly what offk_forward enqueues), reading
 * the G_<site> / D_<site> workspace regions a previous offk_off_units / offk_forward filled and
 * writing the fusion buffers.  algo as in offk_sobel_tdiff.  Used by bench / tools to time K2. */
int offk_sobel_tdiff_all(offk_handle* h, void* stream, void* workspace, int algo);

/* K1+K2 for all nine sites into the workspace fusion buffers (two grouped launches). */
int offk_off_units(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES], void* workspace);
/* The units exactly as offk_forward runs them (ABI v9): the fused form when OFFK_FUSED_UNITS is on -- the 1x1 reduces with the
 * temporal difference in one kernel (T and S straight into the fusion_<28|14|7> regions, D_<site> filled, G_<site> NOT) --
 * in the handle's arithmetic (OFFK_PRECISION_F32SPLIT: the split-fp32 kernel).  For stage tests and profiling. */
int offk_off_units_fused(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES], void* workspace);
/* The same stage for 16-bit maps (offk_forward_typed's dtypes, checks and contract). */
int offk_off_units_fused_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                               void* workspace);
/* The same stage for channels-last maps of any feat_dtype (offk_forward_cl's layout, checks and contract). */
int offk_off_units_fused_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                            void* workspace);

/* K4. Generic channels-last convolution (the fusion convs, RGB_OFF.py:657-685,762-780,
 * 833-841): y = post( pre(conv(in(x)) + bias) + res ).  x,y,res are channel-sliced views
 * (ptr, channels-per-pixel stride, first channel).  w is in the library's K order
 * [Co][Ci/32][KH*KW][32] (see offk_pack_conv_weight).  Requires Ci % 32 == 0, Co % 64 == 0,
 * strides/offsets % 4 == 0.  Tile shape and K-split are chosen automatically.
 * Non-finite values (tests/test_gpu_train_ranges.py): a +-Inf or NaN in x reaches its footprint in its own image, all output channels,
 * and nothing else; in w[co, ci, kh, kw] at most every pixel of y[.., co] (a tap that leaves the map is a zero times it), in bias[co]
 * every pixel of y[.., co]; other images / other output channels are bit-equal. */
enum offk_conv_flags { OFFK_CONV_RELU_IN = 1, OFFK_CONV_RELU_PRE = 2, OFFK_CONV_RELU_POST = 4,
                       /* (256 was OFFK_CONV_WINO7_FUSED in ABI v8: an experiment that lost, out of the library since ABI v9) */ };
int offk_conv2d(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int Ci,
                const float* w, const float* bias, int Co, int KH, int KW, int stride, int pad,
                const float* res, int res_cstride, int res_coff, int flags,
                float* y, int y_cstride, int y_coff);
/* Same with an explicit plan (tuning / micro-benchmarks): tile_cfg 0..5 = block tile 128x128,
 * 128x64, 256x64, 64x64, 64x128, 128x256 (pixels x channels), 6 / 7 = the LDS-patch kernel (k x k
 * convs whose 196-pixel output groups come from a 28x28 / four 14x14 / one 14x14 / four 7x7 input patch: 7x7s2@28,
 * 5x5s2@14, 3x3s1@14, 3x3s1@7; 128 / 64 output channels per block; splitk then splits the channel chunks)
 * (10 was its half-chunk bf16x3 form: retired in ABI v9), < 0 = automatic; splitk >= 1
 * K-slices whose fp32 partial slabs [splitk][M][Co] go to `partial` (summed in slice order by
 * a second launch, so results are bit-reproducible); splitk < 1 = automatic; precision must be
 * OFFK_PRECISION_FP32 (the stage entry has no split form). */
int offk_conv2d_ex(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int Ci,
                   const float* w, const float* bias, int Co, int KH, int KW, int stride, int pad,
                   const float* res, int res_cstride, int res_coff, int flags,
                   float* y, int y_cstride, int y_coff, int tile_cfg, int splitk, float* partial, size_t partial_floats,
                   int precision);
/* [Co][Ci][KH][KW] (PyTorch) -> [Co][Ci/32][KH*KW][32]; both device pointers. */
int offk_pack_conv_weight(void* stream, const float* w_oihw, int Co, int Ci, int KH, int KW, float* w_packed);
/* K4b (additive, ABI v10). Backward of ONE stride-1 fusion convolution (22 of the reference's 24: RGB_OFF.py:657-685, 766-780, 833-841), exact
 * fp32, as stage entry points with the view conventions above: activations and gradients are channels-last rows [n_img * H * W][cstride]
 * addressed as (ptr, cstride, coff); weights and weight gradients are PyTorch's [Co][Ci][KH][KW], contiguous (a bound nn.Conv2d.weight and
 * its .grad).  Shapes: KH = KW in {1, 3}, stride 1, pad = (KH - 1) / 2, Ci % 64 == 0, Co % 64 == 0, any H, W >= 1, strides and offsets
 * % 4 == 0.  Every entry enqueues on `stream` in order, does not synchronise and does not allocate (capturable).  Refused with
 * OFFK_ERR_INVALID before any HIP call, the entry's name in offk_last_error(NULL): a null pointer (db excepted), another shape, a negative
 * offset, cstride < coff + C, a scratch smaller than offk_conv2d_backward_plan says, and the overlaps named below.
 *
 * offk_relu_backward: g = dy where y > 0, else exactly 0 (y <= 0, y = -0.0, y = NaN: torch's rule); accumulate != 0: g += that.  C % 4 == 0.
 * g may be dy itself (same pointer, stride and offset: in place); any other overlap of g's bytes [g, g + rows * g_cstride * 4) with dy's
 * or y's is refused.  Serves the ReLU behind a conv (y = the conv's stored output), behind a residual add, and in front of a conv
 * (OFFK_CONV_RELU_IN: y = the conv's input, applied to its dx).
 *
 * offk_conv2d_backward_data: dx[n,h,w,ci] (+)= sum_{co,kh,kw} g[n, h - kh + pad, w - kw + pad, co] * w[co,ci,kh,kw], terms outside the map 0:
 * the library's direct conv (never a Winograd form) on the transposed, 180-degree rotated weight, which a device kernel cuts into `scratch`
 * on every call.  accumulate != 0 adds the (completely summed, once rounded) result to dx.  dx's bytes may not overlap g's.
 *
 * offk_conv2d_backward_weight: dw[co,ci,kh,kw] (+)= sum_{n,h,w} g[n,h,w,co] * in(x)[n, h + kh - pad, w + kw - pad, ci], in(x) = max(x, 0) if
 * relu_in else x; db[co] (+)= sum_{n,h,w} g[n,h,w,co] (db may be NULL).  A TN GEMM over K = the pixels on the fp32 matrix pipe, K split into
 * weight_chunks chunks of ceil(n_img / weight_chunks) whole images (the last one may be shorter); the partial slabs [chunk][Co][Ci * KH * KW]
 * (+ [chunk][Co] for db) live in `scratch` and a second launch adds them in chunk order: bit-reproducible.
 *
 * offk_conv2d_backward_plan: pure host code (no GPU needed): the scratch bytes of the two entries above and the number of K chunks.  A function
 * of these seven integers only -- not of the device, the stream or the environment.  Output pointers may be NULL.
 *
 * Range and non-finite values (these entries, the stride-2 ones and the heads' below; tests/test_gpu_scale_equivariance.py,
 * tests/test_gpu_train_ranges.py).  The sums are fp32 +, x and fma in a fixed order with no constant that is not an operand, so multiplying an
 * operand by 2^a multiplies the result by exactly 2^a, bit for bit, as long as no term or sum leaves fp32's normal range.  fp32 subnormal
 * operands are kept, not flushed (hipcc's default keeps fp32 denormals and v_mfma_f32_16x16x4_f32 honours them).  A +-Inf or NaN in an
 * operand comes out non-finite in every output element whose sum it enters (0 * Inf = NaN) and leaves every other image (dx), every other
 * input channel (dw under a value in x) and every other output channel (a value in g) finite and bit-equal.  INSIDE those limits a kernel
 * that removes a term by zeroing one operand turns 0 * Inf into NaN where the value does not belong:
 *   offk_relu_backward selects: dy reaches its own element where y > 0, nothing else; y = NaN or -Inf gives exactly 0, y = +Inf passes dy.
 *   offk_conv2d_backward_data: a value in g reaches exactly the pixels of its footprint; a value in w[co,ci,kh,kw] makes EVERY pixel of
 *   dx[.., ci] non-finite, in every image (k = 3: the taps that leave the map multiply it by a zero).
 *   offk_conv2d_backward_weight (and _split): k = 3: a value in x[.., ci] makes ALL NINE taps of dw[:, ci] non-finite (g is zero on the ring
 *   around the pixel), a value in g[.., co] all nine taps of dw[co, :] (x is zero on the ring) and db[co]; k = 1: exactly the elements reached.
 *   relu_in: max(x, 0) in hardware -- x = NaN and x = -Inf count as 0, x = +Inf as above. */
int offk_relu_backward(void* stream, const float* dy, int dy_cstride, int dy_coff, const float* y, int y_cstride, int y_coff, int rows, int C,
                       float* g, int g_cstride, int g_coff, int accumulate);
int offk_conv2d_backward_data(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw,
                              int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff, int accumulate, void* scratch,
                              size_t scratch_bytes);
int offk_conv2d_backward_weight(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff, int n_img,
                                int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw, float* db, int accumulate,
                                void* scratch, size_t scratch_bytes);
int offk_conv2d_backward_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes,
                              size_t* weight_scratch_bytes, int* weight_chunks);
/* K4b's weight / bias gradient in split-fp32 arithmetic on the bf16 matrix pipe (additive, ABI v10; csrc/conv_wgrad_split.hip).
 * offk_conv2d_backward_weight_split has offk_conv2d_backward_weight's argument list, shapes, conventions and refusals word for word (its own
 * name in offk_last_error(NULL); the scratch is sized by offk_conv2d_backward_plan_split) and computes the same dw and db.  An opt-in entry:
 * nothing in the library calls it on its own.
 *
 * Arithmetic: g and in(x) (the ReLU comes before the cut) are cut by truncation into three bf16 planes h, m, l (the upper 16 bits of the
 * word, of the exact remainder, and of its remainder).  K runs over POSITIONS q in steps of 32:
 *   k = 1: the pixels, q = (img * H + h) * W + w, PP = H * W positions per image, images back to back.
 *   k = 3: pitch = 8 * ceil((W + 1) / 8) positions per row (the W pixels, then pitch - W >= 1 zeros), PP = (H + 1) * pitch positions per image
 *          (its H rows, then one row of zeros), q = img * PP + h * pitch + w; every position outside [0, n_img * PP) is a zero.  Tap (kh, kw)
 *          multiplies g at q with x at q + (kh - 1) * pitch + (kw - 1).
 * Chunk c holds the positions [img_b * PP, img_e * PP) of its whole images img_b = c * ceil(n_img / weight_chunks) .. img_e (the last chunk may
 * be shorter); its step t is the 32 positions from img_b * PP + 32 t on, g counting as zero from img_e * PP on.  Per step and tap the six
 * products g_l x_h, g_h x_l, g_m x_m, g_m x_h, g_h x_m (into accumulator A2) and g_h x_h (into A1) are issued on v_mfma_f32_16x16x32_bf16 in
 * this order, steps in increasing order; a chunk's partial is A1 + A2, added once; the partial slabs [chunk][Co][Ci * KH * KW] live in
 * `scratch` and the second launch of offk_conv2d_backward_weight (the same kernel) adds them in chunk order.  No atomics, every slab element
 * is written by exactly one thread: bit-reproducible from run to run and under graph capture.  db is an fp32 sum of g itself in a fixed
 * order (per chunk: a thread's position quads q % 32 in {4 j .. 4 j + 3} in step order, each quad as (g0 + g1) + (g2 + g3); then j = 0 .. 7 in
 * order; then the chunks in order): nothing is split.
 * Contract: the three dropped products g_m x_l + g_l x_m + g_l x_l are at most (2^-21 + 2^-30) sum |g x| per element of dw, beside an fp32
 * accumulation error: |dw - exact| <= |dropped| + A * 2^-24 * sum |g x| + 2^-24 |exact| with A = max(1, 2 c_acc), c_acc the accumulation
 * constant of the CPU emulation of exactly this order (tests/conv_wgrad_split.py); integer operands whose planes and sums fit are exact.
 * Non-finite and tiny inputs behave as the split-mode paragraph at OFFK_PRECISION_F32SPLIT says (+-Inf in an operand gives NaN: Inf - Inf
 * in the cut; below 2^-109 an operand's last plane is lost).  One difference under relu_in, shared with offk_conv2d_backward_weight: the
 * ReLU is max(x, 0) in hardware, so a NaN in x counts as 0 there, where torch's relu would keep it.  Which elements a non-finite value
 * reaches is offk_conv2d_backward_weight's paragraph above, word for word (the zero columns and the zero row of the K layout play the
 * ring's part: all nine taps of dw[:, ci] or dw[co, :]); dw holds NaN there, db -- an fp32 sum of g itself -- +-Inf or NaN.  Scaling
 * an operand by 2^a scales dw and db by exactly 2^a (the cut masks significand bits), operands and planes in the normal range.
 *
 * offk_conv2d_backward_plan_split: pure host code, a function of the seven integers only; output pointers may be NULL.  weight_scratch_bytes
 * = weight_chunks * (Co * Ci * KH * KW + Co) * 4.  The chunks are the split kernel's own (its tile, occupancy and minimum chunk length
 * differ from the fp32 kernel's) under the same rules: whole images per chunk, ceil(n_img / weight_chunks) each, no empty chunk. */
int offk_conv2d_backward_weight_split(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff,
                                      int n_img, int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw, float* db,
                                      int accumulate, void* scratch, size_t scratch_bytes);
int offk_conv2d_backward_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_scratch_bytes, int* weight_chunks);
/* K4b's data gradient in split-fp32 arithmetic on the bf16 matrix pipe (additive, ABI v10; csrc/conv_dgrad_split.hip).
 * offk_conv2d_backward_data_split has offk_conv2d_backward_data's argument list, shapes, views, forms and refusals word for word (k in {1, 3}
 * with pad (k - 1) / 2, Ci % 64 == 0 and Co % 64 == 0, strides and offsets % 4 == 0, dx may not overlap g; its own name in
 * offk_last_error(NULL); the scratch is sized by offk_conv2d_backward_data_plan_split and must be 16-byte aligned) and computes the same dx.
 * An opt-in entry: nothing in the library calls it on its own; DESIGN.md 8.8 has the measured times per shape and names the shapes on
 * which it is NOT faster than the fp32 entry.  Enqueue only: three launches on `stream` (two pre-passes that cut the weight and g into
 * planes, then the GEMM), no allocation, no library-owned stream, capturable; a refused call makes no HIP call and writes nothing.
 *
 * Arithmetic (DESIGN.md 5.1's): dx[n,h,w,ci] (+)= sum_{kh,kw,co} g[n, h + pad - kh, w + pad - kw, co] * w[co,ci,kh,kw] is one contraction
 * over K = (tap, co) with the conv weight in the role of `w` and g in the role of `x`.  Both are cut by truncation into three bf16 planes
 * h, m, l (the upper 16 bits of the word, of the exact remainder, and of its remainder).  K order: K index = tap * Co + co with
 * tap = kh * k + kw (kh major, then kw; k = 1 is the one-tap case), inside a tap co in steps of 32 (Co % 64 == 0: a step
 * never straddles a tap); a tap whose g pixel leaves the map -- its row or its image -- contributes zeros.  Per 32-k step the six products
 * w_l g_h, w_h g_l, w_m g_m, w_m g_h, w_h g_m (into accumulator A2) and w_h g_h (into A1) are issued on v_mfma_f32_16x16x32_bf16 in this order,
 * steps in increasing order; the result is A1 + A2, added once; accumulate != 0 then adds that once-rounded value to dx.  K is not split,
 * there is no reduce launch, there are no atomics and every dx element is written by exactly one thread: bit-reproducible from run to
 * run, whatever `scratch` held before, and under graph capture.
 * Contract: the three dropped products w_m g_l + w_l g_m + w_l g_l are at most (2^-21 + 2^-30) sum |g w| per element of dx, beside an fp32
 * accumulation error: |dx - exact| <= |dropped| + A * 2^-24 * sum |g w| + 2^-24 |exact| with A = max(1, 2 c_acc), c_acc the accumulation
 * constant of the CPU emulation of exactly this order (tests/conv_dgrad_split.py), and one more 2^-24 |result| when accumulating; integer
 * operands whose planes and sums fit are exact.  Non-finite and tiny inputs behave as the split-mode paragraph at OFFK_PRECISION_F32SPLIT
 * says (+-Inf in an operand gives NaN: Inf - Inf in the cut; below 2^-109 an operand's last plane is lost).  The elements a non-finite
 * value reaches are offk_conv2d_backward_data's (the footprint for g, every pixel of dx[.., ci] for w, NaN here); the ci tiles behind Ci
 * that a block stages are never stored.  Scaling g or w by 2^a scales dx by exactly 2^a.
 *
 * offk_conv2d_backward_data_plan_split: pure host code, a function of the seven integers only; the output pointer may be NULL.
 * data_scratch_bytes = round256(Co * Ci * KH * KW * 6) + round256(n_img * H * W * Co * 6): the three bf16 planes of the packed weight
 * ([tap][32-co step][16-ci tile][plane][lane] x 16 B), then the three channels-last bf16 plane images of g, each region rounded up to 256
 * bytes.  offk_conv2d_backward_data_form_split: the block of the GEMM the same seven integers choose -- (ci_per_block, pixels_per_block)
 * = (64, 256) where Ci == 64, else (128, 128) where ceil(n_img H W / 256) * ceil(Ci / 128) <= 128, else (128, 256); the arithmetic and
 * the bits of dx do not depend on it.  Output pointers may be NULL. */
int offk_conv2d_backward_data_split(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co,
                                    const float* w_oihw, int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff,
                                    int accumulate, void* scratch, size_t scratch_bytes);
int offk_conv2d_backward_data_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes);
int offk_conv2d_backward_data_form_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, int* ci_per_block, int* pixels_per_block);
/* K4b, stride 2 (additive, ABI v10). Backward of the two stage-opening fusion convolutions (motion_conv_trans_28: 7x7 / 2 / 3, RGB_OFF.py:657;
 * motion_conv_trans_14: 5x5 / 2 / 2, RGB_OFF.py:762), exact fp32 -- with the entries above all 24 fusion convs.  The conventions are K4b's,
 * word for word (views, enqueue only, no synchronisation, no allocation, refusals with OFFK_ERR_INVALID and the entry's name before any HIP
 * call: a null pointer (db excepted), another form, an odd H or W, bad channel counts, a negative offset, cstride < coff + C, a scratch
 * smaller than the plan's, dx overlapping g).  H and W are the INPUT map's size, even and >= 2; g is [n_img * (H/2) * (W/2)][g_cstride].
 * Forms: (KH = KW, pad) in {(7, 3), (5, 2)}; Ci % 32 == 0, Co % 64 == 0; strides and offsets % 4 == 0.  The stride-1 entries above keep
 * refusing k = 5 and k = 7.
 *
 * offk_conv2d_s2_backward_data: dx[n, 2a+r, 2b+s, ci] (+)= sum_co sum_{kh = r+pad (mod 2)} sum_{kw = s+pad (mod 2)}
 * g[n, a + (r+pad-kh)/2, b + (s+pad-kw)/2, co] * w[co,ci,kh,kw], terms outside the map 0: one implicit GEMM per phase (r, s) of the input
 * pixel on the fp32 matrix pipe, all four in one launch, only the taps that exist, stored straight to the dx pixels.  A device kernel cuts the
 * phase weights into `scratch` on every call.  K is not split; accumulate != 0 adds the completely summed, once rounded result to dx.
 *
 * offk_conv2d_s2_backward_weight: dw[co,ci,kh,kw] (+)= sum_{n,oh,ow} g[n,oh,ow,co] * in(x)[n, 2 oh + kh - pad, 2 ow + kw - pad, ci];
 * db[co] (+)= sum g (db may be NULL).  Split over K into weight_chunks chunks of ceil(n_img / weight_chunks) whole images; partial slabs
 * [chunk][Co][Ci * KH * KW] (+ [chunk][Co]) in `scratch`, added in chunk order by the stride-1 entry's reduce: bit-reproducible.
 *
 * Range and non-finite values: the paragraph at the stride-1 entries holds (exact power-of-two scaling, subnormals kept, a non-finite
 * value reaches every sum it enters and no other image / input channel / output channel).  Inside those limits:
 *   offk_conv2d_s2_backward_data (and _split, which gives NaN): a value in g reaches exactly the pixels of its footprint; a value in
 *   w[co,ci,kh,kw] makes every pixel of ITS PHASE of dx[.., ci] non-finite -- rows of parity (kh + pad) & 1, columns of parity (kw + pad) & 1,
 *   every image (a tap that leaves the map is a zero times the weight).
 *   offk_conv2d_s2_backward_weight: a value in x[n, R, C, ci] makes dw[:, ci, kh, kw] non-finite for the kernel rows kh that read row R
 *   (R = 2 oh + kh - pad, 0 <= oh < H / 2) and in them for EVERY kw of C's parity ((C + pad - kw) even), also where 2 ow + kw - pad = C has no
 *   ow inside the map: the kernel removes the taps that wrap into the neighbouring row by zeroing its g operand, and 0 * Inf is NaN.  A
 *   value in g[n, oh, ow, co] makes dw[co, :, kh, kw] non-finite for EVERY kernel row kh (a row outside the map is a row of zeros times it)
 *   and the kw whose x column 2 ow + kw - pad lies inside the map -- the wrapped column taps are removed by a select on g and stay
 *   clean, bit for bit -- and db[co].  relu_in: x = NaN and x = -Inf count as 0.
 *
 * offk_conv2d_s2_backward_plan: pure host code, a function of these seven integers only.  Output pointers may be NULL. */
int offk_conv2d_s2_backward_data(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co, const float* w_oihw,
                                 int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff, int accumulate, void* scratch,
                                 size_t scratch_bytes);
int offk_conv2d_s2_backward_weight(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff, int n_img,
                                   int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw, float* db,
                                   int accumulate, void* scratch, size_t scratch_bytes);
int offk_conv2d_s2_backward_plan(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes,
                                 size_t* weight_scratch_bytes, int* weight_chunks);
/* K4b, stride 2: the data gradient in split-fp32 arithmetic on the bf16 matrix pipe (additive, ABI v10; csrc/conv_dgrad_s2_split.hip).
 * offk_conv2d_s2_backward_data_split has offk_conv2d_s2_backward_data's argument list, shapes, views, forms and refusals word for word (its
 * own name in offk_last_error(NULL); the scratch is sized by offk_conv2d_s2_backward_plan_split and must be 16-byte aligned) and computes
 * the same dx (at n_img = 384 in 0.99 against 1.36 ms (7x7 / 2, 320 -> 64) and 0.91 against 1.18 ms (5x5 / 2, 1056 -> 128)
 * on the fp32 entry).  An opt-in entry: nothing in the library calls it on its own.  Enqueue only: three launches on `stream` (two pre-passes and
 * the GEMM), no allocation, no library-owned stream, capturable; a refused call makes no HIP call and writes nothing.
 *
 * Arithmetic (DESIGN.md 5.1's): per phase (r, s) of the input pixel the sum above is a contraction over K = (tap, co) with the conv weight
 * in the role of `w` and g in the role of `x`.  Both are cut by truncation into three bf16 planes h, m, l (the upper 16 bits of the word,
 * of the exact remainder, and of its remainder).  K order of phase (r, s): the taps in the fp32 entry's packing order (th major, then tw;
 * tap (th, tw) is kernel element (kh0 + 2 th, kw0 + 2 tw), kh0 = (r + pad) & 1, and reads g at (a + (r + pad - kh0) / 2 - th, b + ... - tw)),
 * inside a tap co in steps of 32 (Co % 64 == 0: a step never straddles a tap); a tap that leaves the map at a pixel contributes zeros.
 * Per 32-k step the six products w_l g_h, w_h g_l, w_m g_m, w_m g_h, w_h g_m (into accumulator A2) and w_h g_h (into A1) are issued on
 * v_mfma_f32_16x16x32_bf16 in this order, steps in increasing order; the result is A1 + A2, added once; accumulate != 0 then adds that
 * once-rounded value to dx.  K is not split, there are no atomics and every dx element is written by exactly one thread: bit-reproducible
 * from run to run, whatever `scratch` held before, and under graph capture.
 * Contract: the three dropped products w_m g_l + w_l g_m + w_l g_l are at most (2^-21 + 2^-30) sum |g w| per element of dx, beside an fp32
 * accumulation error: |dx - exact| <= |dropped| + A * 2^-24 * sum |g w| + 2^-24 |exact| with A = max(1, 2 c_acc), c_acc the accumulation
 * constant of the CPU emulation of exactly this order (tests/conv_s2_dgrad_split.py), and one more 2^-24 |result| when accumulating; integer
 * operands whose planes and sums fit are exact.  Non-finite and tiny inputs behave as the split-mode paragraph at OFFK_PRECISION_F32SPLIT
 * says (+-Inf in an operand gives NaN: Inf - Inf in the cut; below 2^-109 an operand's last plane is lost).  The elements a non-finite
 * value reaches are offk_conv2d_s2_backward_data's (the paragraph above: the footprint for g, the whole phase of dx[.., ci] for w); the ci
 * tiles behind Ci that a block stages are never stored.  Scaling g or w by 2^a scales dx by exactly 2^a.
 *
 * offk_conv2d_s2_backward_plan_split: pure host code, a function of the seven integers only; the output pointer may be NULL.
 * data_scratch_bytes = round256(Co * Ci * KH * KW * 6) + round256(n_img * (H/2) * (W/2) * Co * 6): the three bf16 planes of the packed
 * weight, then the three channels-last bf16 plane images of g, each region rounded up to 256 bytes. */
int offk_conv2d_s2_backward_data_split(void* stream, const float* g, int g_cstride, int g_coff, int n_img, int H, int W, int Co,
                                       const float* w_oihw, int Ci, int KH, int KW, int pad, float* dx, int dx_cstride, int dx_coff,
                                       int accumulate, void* scratch, size_t scratch_bytes);
int offk_conv2d_s2_backward_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* data_scratch_bytes);
/* K4b, stride 2: the weight / bias gradient in split-fp32 arithmetic on the bf16 matrix pipe (additive, ABI v10; csrc/conv_wgrad_s2_split.hip).
 * offk_conv2d_s2_backward_weight_split has offk_conv2d_s2_backward_weight's argument list, shapes, views, forms and refusals word for word
 * (its own name in offk_last_error(NULL); the scratch is sized by offk_conv2d_s2_backward_weight_plan_split) and computes the same dw and
 * db (at n_img = 384 in 1.14 against 1.55 ms (7x7 / 2, 320 -> 64) and 1.00 against 1.30 ms (5x5 / 2, 1056 -> 128) on the fp32 entry,
 * DESIGN.md 8.9).  An opt-in entry: nothing in the library calls it on its own.  Enqueue only: two launches on `stream` (the GEMM and the reduce), no allocation, no library-owned stream, capturable; a
 * refused call makes no HIP call and writes nothing.  db may be NULL.
 *
 * Arithmetic (DESIGN.md 5.1's): g and in(x) (the relu_in ReLU comes before the cut) are cut by truncation into three bf16 planes h, m, l
 * (the upper 16 bits of the word, of the exact remainder, and of its remainder).  K layout: K runs over the OUTPUT pixels, real pixels
 * only, q = (img * (H/2) + oh) * (W/2) + ow, PP = (H/2) * (W/2) positions per image, images back to back: no zero column, no zero row.
 * Tap (kh, kw) multiplies g at q with X_(kh,kw)[q] = in(x)[img, 2 oh + kh - pad, 2 ow + kw - pad], which is a ZERO where that row or that
 * column leaves the map (the tap is removed on the x side; g is staged as it lies).  Chunk c holds the positions [img_b * PP, img_e * PP) of
 * its whole images img_b = c * ceil(n_img / weight_chunks) .. img_e (the last chunk may be shorter); its step t is the 32 positions from
 * img_b * PP + 32 t on (steps of 32), both operands counting as zero from img_e * PP on.  Per step and tap the six products
 * g_l x_h, g_h x_l, g_m x_m, g_m x_h, g_h x_m (into accumulator A2) and g_h x_h (into A1) are issued on v_mfma_f32_16x16x32_bf16 in this
 * order, steps in increasing order; a chunk's partial is A1 + A2, added once; the partial slabs [chunk][Co][Ci * KH * KW] (+ [chunk][Co]) live in `scratch`
 * and the second launch of offk_conv2d_backward_weight (the same kernel) adds them in chunk order.  No atomics, every slab element is
 * written by exactly one thread, the scratch's old contents never show: bit-reproducible from run to run and under graph capture.  db has no
 * products: it is an fp32 sum of g itself in a fixed order (per chunk: a thread's position quads q % 32 in {4 j .. 4 j + 3} in step order,
 * each quad as (g0 + g1) + (g2 + g3); then j = 0 .. 7 in order; then the chunks in order): nothing is split.
 * Contract: the three dropped products g_m x_l + g_l x_m + g_l x_l are at most (2^-21 + 2^-30) sum |g x| per element of dw, beside an fp32
 * accumulation error: |dw - exact| <= |dropped| + A * 2^-24 * sum |g x| + 2^-24 |exact| with A = max(1, 2 c_acc), c_acc the accumulation
 * constant of the CPU emulation of exactly this order (tests/conv_s2_wgrad_split.py); integer operands whose planes and sums fit are
 * exact.  Scaling an operand by 2^a scales dw and db by exactly 2^a (the cut masks significand bits), operands and planes in the normal
 * range.  Non-finite and tiny inputs behave as the split-mode paragraph at OFFK_PRECISION_F32SPLIT says (+-Inf in an operand gives NaN:
 * Inf - Inf in the cut; below 2^-109 an operand's last plane is lost).  Which elements a non-finite value reaches DIFFERS from
 * offk_conv2d_s2_backward_weight's paragraph, because the taps that leave the map are zeros on the x side here:
 *   a value in x[n, R, C, ci] makes dw[:, ci, kh, kw] NaN for exactly the taps whose sum it enters -- the kernel rows kh with
 *   R = 2 oh + kh - pad for an oh in [0, H/2) and the kernel columns kw with C = 2 ow + kw - pad for an ow in [0, W/2) -- and nothing else
 *   (every staged x value is a pixel of the tap itself or a constant zero); relu_in: max(x, 0) in hardware, x = NaN and x = -Inf count as 0;
 *   a value in g[n, oh, ow, co] makes ALL KH * KW taps of dw[co, :] NaN, every ci: where a tap leaves the map at (oh, ow) its x operand
 *   is a zero and g = Inf (NaN after the cut) times a zero is NaN -- the fp32 entry's select on g keeps those taps clean, this entry does
 *   not; db[co] is +-Inf or NaN (an fp32 sum of g itself).  Every other output channel, and every input channel under a value in x, stays
 *   finite and bit-equal.
 *
 * offk_conv2d_s2_backward_weight_plan_split: pure host code, a function of the seven integers only; output pointers may be NULL; the
 * refusals of offk_conv2d_s2_backward_plan under its own name.  weight_scratch_bytes = weight_chunks * (Co * Ci * KH * KW + Co) * 4.  The
 * chunks are the split kernel's own (one block of eight waves per CU: tiles = (Co / 64) * ceil(Ci / 64) * KH blocks per chunk, as many
 * chunks as fit one round of 256 blocks for the 7x7 and two rounds for the 5x5, a chunk at least 256 positions long) under the same
 * rules: whole images per chunk, ceil(n_img / weight_chunks) each, no empty chunk.  Positions n_img * (H/2) * (W/2) above the fp32 entry's
 * limit are refused with "problem too large". */
int offk_conv2d_s2_backward_weight_split(void* stream, const float* x, int x_cstride, int x_coff, const float* g, int g_cstride, int g_coff, int n_img,
                                   int H, int W, int Ci, int Co, int KH, int KW, int pad, int relu_in, float* dw_oihw, float* db,
                                   int accumulate, void* scratch, size_t scratch_bytes);
int offk_conv2d_s2_backward_weight_plan_split(int n_img, int H, int W, int Ci, int Co, int KH, int KW, size_t* weight_scratch_bytes,
                                              int* weight_chunks);
/* Override the plan offk_forward uses for one fusion conv (key = its state_dict name without
 * ".weight", e.g. "motion_conv_trans_28"); tile_cfg < 0 / splitk < 1 restore the automatic choice. */
int offk_set_conv_plan(offk_handle* h, const char* conv_key, int tile_cfg, int splitk);

/* K4c. One bottleneck chain of fusion@28 at 14x14 in one launch (exact fp32): t1 = relu(c1(in(x))), t2 = relu(c2_3x3(t1)),
 * y = relu(c3([t2 | x]) + b3 + res) -- RGB_OFF.py:658-667 (28a: K3 = 128, c3's weight = [motion_conv3_trans_28a |
 * motion_conv_branch_28a] over [t2 | pre-ReLU x], relu_in = 1, no residual) and :670-676 / :679-685 (28b / 28c: Cin = 256, K3 = 64,
 * res = x).  x: [n_img * 196][x_cstride] channels-last, Cin in {64, 256} channels at x_coff; w1 [64][Cin], w2 the packed
 * 3x3 weight [64][2][9][32] (offk_pack_conv_weight), w3 [256][K3]; res / y: 256 channels at res_coff / y_coff.  t1 and t2
 * never leave the chip (csrc/chain_fused.hip). */
int offk_bottleneck_chain14(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Cin, int relu_in,
                            const float* w1, const float* b1, const float* w2_packed, const float* b2,
                            const float* w3, const float* b3, int K3,
                            const float* res, int res_cstride, int res_coff, float* y, int y_cstride, int y_coff);
/* K4cs (ABI v10). The same chain in split-fp32 arithmetic on the bf16 matrix pipe (csrc/chain_split.hip: what an OFFK_PRECISION_F32SPLIT handle
 * runs in offk_forward; the 3x3 direct, every contraction as six bf16 plane products into two fp32 accumulators): c3 over t2 only (K3 = 64).
 * branch_w == NULL: the residual chains 28b / 28c (Cin = 256 or 64; res may be NULL).  branch_w != NULL (Cin = 64, res must be NULL): chain 28a --
 * y = relu(c3(t2) + b3 + branch_w . x + branch_b) with the branch 1x1 [256][64] on the chain input BEFORE relu_in's ReLU, RGB_OFF.py:657-667.
 * Weights as for offk_bottleneck_chain14 (fp32, device); scratch: device memory for their plane images, at least
 * 6 * (64 * Cin + 64 * 576 + 2 * 256 * 64) bytes (cut on every call: a stage entry point, not a fast path).
 * Views and aliasing, checked before anything is enqueued (OFFK_ERR_INVALID otherwise): offsets >= 0, x_cstride >= x_coff + Cin,
 * y_cstride >= y_coff + 256, res_cstride >= res_coff + 256 (res != NULL).  The chain does NOT run in place: y's bytes
 * [y, y + n_img * 196 * y_cstride * 4) may overlap neither x's [x, x + n_img * 196 * x_cstride * 4) nor res's (a block stores y while the
 * block of the image's other half still reads x's halo rows); res may be x itself (28b / 28c) or any view of x's buffer. */
int offk_bottleneck_chain14_split(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Cin, int relu_in,
                                  const float* w1, const float* b1, const float* w2_packed, const float* b2,
                                  const float* w3, const float* b3, const float* branch_w, const float* branch_b,
                                  const float* res, int res_cstride, int res_coff, float* y, int y_cstride, int y_coff,
                                  void* scratch, size_t scratch_bytes);
/* K4w. 3x3 / stride 1 / pad 1 convolution on 7x7 maps in Winograd form, fp32 arithmetic (csrc/winograd.hip: a map = four tiles,
 * F(4, 3) x F(3, 3) per axis, 121 points): the five such
 * convs of fusion@14 / @7 (RGB_OFF.py:766-767, 775-780, 833-834, 837-838).  Same epilogue and views as offk_conv2d (flags without
 * OFFK_CONV_RELU_IN); w_packed as for offk_conv2d.  scratch: 121 * (Co * Ci + n_img * (Ci + Co)) floats of device memory
 * (transformed weights, transformed input, GEMM output).  pool_part != NULL: [4 * n_img][Co] sums of the stored values of each
 * output tile (an image = 4 consecutive rows): the average pool of a head that follows. */
int offk_winograd_conv3x3(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Ci,
                          const float* w_packed, const float* bias, int Co,
                          const float* res, int res_cstride, int res_coff, int flags,
                          float* y, int y_cstride, int y_coff, float* scratch, size_t scratch_floats, float* pool_part);

/* The 5x5 / stride 2 / pad 2 conv on 14x14 maps (motion_conv_trans_14, RGB_OFF.py:762-763) through the same machinery in polyphase
 * form: four 7x7 phase images x 3x3 phase kernels concatenated along K.  x: [n_img * 196][x_cstride]; y: [n_img * 49][y_cstride];
 * w_packed: the packed 5x5 weight [Co][Ci/32][25][32]; scratch: 400 * Ci * (Co + n_img) + 121 * n_img * Co floats. */
int offk_winograd_conv5x5s2(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Ci,
                            const float* w_packed, const float* bias, int Co,
                            const float* res, int res_cstride, int res_coff, int flags,
                            float* y, int y_cstride, int y_coff, float* scratch, size_t scratch_floats);

/* The 7x7 / stride 2 / pad 3 conv on 28x28 maps (motion_conv_trans_28, RGB_OFF.py:657) in polyphase Winograd form F(5x5, 4x4):
 * four 14x14 phase images x 4x4 phase kernels concatenated along K, 9 output tiles of 5x5 per image, 64 points (winograd7.hip).
 * x: [n_img * 784][x_cstride]; y: [n_img * 196][y_cstride]; w_packed: the packed 7x7 weight [Co][Ci/32][49][32]; flags: ReLU
 * (PRE / POST; no residual input);
 * scratch: 225 * Ci * (Co + 9 * n_img) + 64 * 9 * n_img * Co floats. */
int offk_winograd_conv7x7s2(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int Ci,
                            const float* w_packed, const float* bias, int Co, int flags,
                            float* y, int y_cstride, int y_coff, float* scratch, size_t scratch_floats);

/* What sits BETWEEN two convolutions on the Winograd path at 7x7 maps, in one launch (wino_mid.hip; ABI v8).  Replaces, for the runs
 * 3x3 -> 1x1 -> 3x3 of RGB_OFF.py:762-767 (x1 -> motion_conv1_trans_14a -> motion_conv2_trans_14a) and :833-838 (x2 ->
 * motion_conv1_trans -> motion_conv2_trans), the output transform of the first conv, the 1x1 conv and the input transform of the
 * last one; with w1 == NULL, for :775-780 (motion_conv2_trans_14b -> motion_conv3_trans_14b), the two transforms alone.
 *   M      GEMM output of the conv in front in the Winograd domain, [121][n_img][Cin] (point order: phases_in = 1 a 3x3 / stride 1
 *          conv, 4 the polyphase 5x5 / stride 2 conv); bias_in [Cin] its bias (nullable); ReLU is applied behind it
 *   x      nullable: relu(A^T M A + bias_in) is also stored there, channels-last rows [n_img * 49][x_cstride] at x_coff
 *   w1     1x1 conv [Cmid][Cin] with bias b1 [Cmid] and ReLU behind it; NULL: none (Cmid == Cin)
 *   V      GEMM input of the conv behind, [121][n_img][Cmid]
 * Shapes built: (Cin, Cmid) = (128, 128) and (256, 256); without w1 also Cin = 128 / 256. */
int offk_winograd_between(void* stream, const float* M, const float* bias_in, int phases_in, int n_img, int Cin,
                          float* x, int x_cstride, int x_coff, const float* w1, const float* b1, int Cmid, float* V);
/* (ABI v10) The same with the 1x1 conv in the handle's arithmetic: precision OFFK_PRECISION_F32SPLIT runs stage B in split-fp32 on the bf16
 * matrix pipe (what a split-fp32 handle does in offk_forward; needs w1) -- scratch: Cmid * Cin * 6 bytes of device memory for w1's plane image;
 * OFFK_PRECISION_FP32 = offk_winograd_between. */
int offk_winograd_between_ex(void* stream, const float* M, const float* bias_in, int phases_in, int n_img, int Cin, float* x,
                             int x_cstride, int x_coff, const float* w1, const float* b1, int Cmid, float* V, int precision,
                             void* scratch, size_t scratch_bytes);

/* The batched GEMMs of a convolution on a Winograd path as a stage of their own (wino_gemm.hip / wino_gemm_split.hip; ABI v9):
 *   y[b] = x[b] . w[b]^T,  x [batch][M][K], w [batch][Co][K], y [batch][M][Co], all contiguous fp32; K % 32 == 0, Co % 64 == 0.
 * precision OFFK_PRECISION_FP32: the fp32 matrix pipe.  OFFK_PRECISION_F32SPLIT (K >= 64): split-fp32 arithmetic on the
 * bf16 pipe -- both operands cut into three bf16 planes, six plane products per multiply (the arithmetic of the split units kernel);
 * scratch (>= batch * Co * K * 6 bytes, device) receives the plane image of w.  What a handle created with that precision runs for the
 * fusion convolutions on a Winograd path (RGB_OFF.py:657, 762, 766, 775-777, 833, 837). */
int offk_batched_gemm_nt(void* stream, const float* x, const float* w, float* y, int batch, int M, int K, int Co, int precision,
                         void* scratch, size_t scratch_bytes);

/* K5. Replaces motion_pool_trans_28 / global_pool / squeeze / fc_action_motion*
 * (RGB_OFF.py:782-787, 789-793, 843-847): optional MaxPool(3,2,ceil) then global
 * average over the (pooled) map then Linear.  x: channel slice [x_coff, x_coff+C) of a
 * channels-last buffer with x_cstride channels per pixel. */
int offk_head(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int C,
              int maxpool, const float* fc_w, const float* fc_b, int num_classes, float* out);

/* K5t / K5b (additive, ABI v10). Training side of ONE classifier head (fc_action_motion_28 / _14 / fc_action_motion, un-frozen by
 * train_off.py:39-45): K5's pooling, the training-mode nn.Dropout(p = 0.8) on the pooled vector (RGB_OFF.py:785, 791, 845), the Linear, and
 * their backward -- exact fp32, as stage entry points in K4b's conventions: x and dx are the channel slice [coff, coff + C) of channels-last
 * rows [n_img * H * W][cstride]; fc_w is PyTorch's [num_classes][C] and dw has the same layout (a bound nn.Linear.weight and its .grad);
 * g, out are [n_img][num_classes], z is [n_img][C], all contiguous.  Every entry enqueues on `stream` in order, does not synchronise and
 * does not allocate (capturable).  Domain (K5's): 4 <= C <= 1024, C % 4 == 0, strides and offsets % 4 == 0, H, W >= 1 (>= 3 with maxpool),
 * any num_classes >= 1, 0 <= drop_p < 1, 0 <= head_index <= 239.  Refused with OFFK_ERR_INVALID before any HIP call, the entry's name in
 * offk_last_error(NULL): a null pointer that the call needs, anything outside the domain, a negative offset, cstride < coff + C, a scratch
 * smaller than offk_head_backward_plan says, dx's bytes [dx, dx + n_img * H * W * dx_cstride * 4) overlapping x's or g's.
 *
 * offk_head_train: pooled[n][c] = the mean over the map (maxpool = 0) or over the MaxPool2d(3, 2, ceil_mode) windows, clipped at the border
 * (maxpool = 1), as K5 defines it; z[n][c] = pooled * keep * scale, scale = (float)(1.0 / (1.0 - drop_p)); out = z . fc_w^T + fc_b.  z is
 * caller-owned and is what the backward reads.  keep is the library's reproducible dropout, not the framework's generator: stream
 * (drop_seed, 16 + head_index) -- head_index 0 / 1 / 2 for the 28 / 14 / 7 head, beside the units' streams 0 .. 8 --, draw
 * n * (C / 4) + c / 4 serves a channel quad, 16 bits each, kept iff the field >= round(drop_p * 65536) (the units' rule;
 * offk_amd.synth.head_dropout_keep is the same integer function).  drop_p = 0 is eval arithmetic: every keep * scale is exactly 1.0f.
 *
 * offk_head_backward: g = d loss / d out.  Any of dx, dw, db may be NULL and then that work is not launched (x and fc_w are needed for dx only,
 * z for dw only, scratch for dw and db only).
 *   dz[n][c] = sum_o g[n][o] fc_w[o][c];  dpooled = dz * keep * scale, the mask recomputed from the seed, never stored;
 *   v = dpooled * (1.f / nwin), nwin = H * W (maxpool = 0) or Ho * Wo windows (maxpool = 1)
 *   maxpool = 0: dx[n,h,w,c] (+)= v[n][c] for every pixel
 *   maxpool = 1: dx[n,y,x,c] (+)= the sum of v[n][c] over the windows whose maximum sits at (y, x); the maximum of a window is the FIRST one
 *   in row-major window order (torch's rule, CPU and GPU): an all-zero window sends its gradient to its top-left pixel.  A gather -- no
 *   atomics, every dx element of the slice is written, zeros included; accumulate_dx != 0 adds to what dx holds (a head's input also feeds
 *   the next stage).  NaN in x on this path is outside the contract: K5's forward drops a NaN where torch propagates it.
 *   dw[o][c] (+)= sum_n g[n][o] z[n][c], db[o] (+)= sum_n g[n][o]  (accumulate_w), split over n_img into `chunks` chunks of
 *   ceil(n_img / chunks) whole images (the last one may be shorter); the partial slabs [chunk][num_classes][C] + [chunk][num_classes] live
 *   in `scratch` and a second launch adds them in chunk order: bit-reproducible whatever the scratch held.
 * Range and non-finite values (tests/test_gpu_scale_equivariance.py, tests/test_gpu_train_ranges.py): x and fc_b, fc_w and fc_b, or g times
 * 2^a scale every output by exactly 2^(a degree) and the max-pool picks the same cells; fp32 subnormals are kept, and where a result
 * is itself subnormal (z of a subnormal x) each rounded operation may add half of 2^-149 beside its relative error: the format's.  Nothing here zeroes an
 * operand to remove a term, so a +-Inf or NaN comes out non-finite in exactly the elements IEEE arithmetic on the formulas above gives
 * (a dropped channel's keep * scale = 0 turns an Inf into NaN), every other element bit-equal -- except under the max-pool, where a NaN
 * or -Inf in x is not there (fmaxf drops the NaN, -Inf is never a maximum) and a +Inf in x moves the route of dx without entering it.
 *
 * offk_head_backward_plan: pure host code (no GPU needed), a function of these three integers only.  Output pointers may be NULL. */
int offk_head_train(void* stream, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int C, int maxpool, const float* fc_w,
                    const float* fc_b, int num_classes, int head_index, uint64_t drop_seed, double drop_p, float* z, float* out);
int offk_head_backward(void* stream, const float* g, const float* x, int x_cstride, int x_coff, int n_img, int H, int W, int C, int maxpool,
                       const float* fc_w, int num_classes, const float* z, int head_index, uint64_t drop_seed, double drop_p, float* dx,
                       int dx_cstride, int dx_coff, int accumulate_dx, float* dw, float* db, int accumulate_w, void* scratch,
                       size_t scratch_bytes);
int offk_head_backward_plan(int n_img, int C, int num_classes, size_t* scratch_bytes, int* chunks);

/* K6. Replaces ConsensusModule('avg') (basic_ops.py:12-46) as applied in
 * Flow_OFF.py:867-876: x [B, T, C] -> mean over T -> [B, C]. */
int offk_segment_consensus(void* stream, const float* x, int B, int T, int C, float* out);

/* K7. Late score fusion as the eval scripts do it after the forward (test_rgb_off.py:138:
 * np.mean over the 10 crops, weighted sum of the score sets; score_fusion.ipynb cell 8: six sets,
 * weights 1.0/1.5/1.6 (RGB 7x7 / TSN / 14x14) and 1.2/0.8/1.7 (Flow), then argmax):
 *   fused[v][c] = sum_i weights[i] * mean_k scores[i][v][k][c],   pred[v] = argmax_c fused[v][c]
 * scores: n_sets device pointers to [videos, crops, classes] fp32 (host array of pointers);
 * weights: n_sets host floats; pred may be NULL.  With crops = 1 this is the plain weighted sum
 * used for the modality_fuse return (Flow_OFF.py:881). */
int offk_score_fusion(void* stream, const float* const* scores, const float* weights, int n_sets, int videos,
                      int crops, int classes, float* fused, int32_t* pred);

/* ---- Training side of the OFF units ------------------------------
 * What train_off.py:126-151 needs from the path: the units' forward in training mode (nn.Dropout(p=0.8),
 * RGB_OFF.py:356, on every spatial gradient, :612 ...), and the gradients of the units' parameters --
 * the unit-side tensors among those train_off.py:39-45 leaves trainable; the feature maps come from a backbone
 * the reference's scripts freeze (their gradient, for callers that un-freeze it: offk_off_units_backward_feats).  The fusion stages / heads between the units and the loss are ordinary
 * convolutions and stay with the caller's autograd; the cut is the gradient w.r.t. each unit output
 * motion_<site> = cat(S 32, T 128) (:616), i.e. the leading channels of the gradients of the three cat
 * results (:656, :760, :832).
 *
 * Dropout is reproducible instead of drawn from the framework's generator: element (pair, c, y, x) of site
 * s is kept iff a 16-bit field of splitmix64(stream(drop_seed, s), (pair*H*W + y*W + x)*8 + c/4) is
 * >= round(drop_p * 65536); kept values are scaled by 1/(1-drop_p).  offk_amd/synth.py (dropout_keep)
 * is the same function in numpy.  drop_p = 0 is eval mode. */
typedef struct offk_grad_view {
  const float* data;   /* channels-last rows [P*H*W][cstride] (e.g. a torch channels_last gradient tensor) */
  int32_t cstride;     /* channels per pixel of that buffer */
  int32_t coff;        /* first of the unit's 160 channels: [coff, coff+32) = S, [coff+32, coff+160) = T */
} offk_grad_view;

/* Workspace for the calls below: the offk_workspace_bytes layout followed by the backward regions
 * ("dG_<site>", "dD_<site>", partial-sum slabs); a superset, usable for offk_forward as well. */
size_t offk_train_workspace_bytes(const offk_handle* h);

/* offk_off_units in training mode: like offk_off_units, with the dropout above applied to S.  Leaves
 * G_<site> / D_<site> in the workspace for the backward.
 * Non-finite values (this entry and offk_off_units_train_split; tests/test_gpu_train_ranges.py).  The ReLU of G is a hardware max: a
 * pre-activation that is NaN or -Inf gives exactly 0, +Inf stays.  A +-Inf or NaN in x[n, c, y, x] makes D of that pixel non-finite in all
 * 32 channels (NaN in split arithmetic) and G of that pixel +Inf or 0 in each of its 128 channels; K2 carries the D part into the 3 x 3
 * neighbourhood of the pixel, all 32 spatial channels of the pair the frame is the spatial row of (kept or dropped: 0 * NaN is NaN), and
 * the G part at most into the 128 temporal channels of that pixel in the pairs of its clip that hold the frame.  A value in Wg[o, c] or
 * bg[o] makes column o of G +Inf or 0 (bg[o] = +Inf: +Inf everywhere; the bias is added in fp32 in split arithmetic too) and at most
 * temporal channel o of the unit output non-finite; a value in Wd[j, c] or bd[j] makes column j of D non-finite everywhere (NaN for Wd in
 * split arithmetic) and at most spatial channel j of the unit output.  Every other pixel, column and site is bit-equal. */
int offk_off_units_train(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES], void* workspace,
                         uint64_t drop_seed, double drop_p);

/* Gradient buffer: one flat fp32 device array the caller owns; offk_unit_grad_slot gives the offset and
 * element count of a parameter (reference state_dict key, e.g. "motion_conv_gen_3a.weight") in the
 * reference's own layout ([128,C,1,1], [128], [32,C,1,1], [32], [32,1,3,3], [32]). */
size_t offk_unit_grad_floats(const offk_handle* h);
int offk_unit_grad_slot(const offk_handle* h, const char* key, size_t* offset_floats, size_t* count);

/* Backward of the nine units.  Needs the G_<site> / D_<site> regions of `workspace` as the matching
 * offk_off_units(_train) / offk_forward call on the same feats left them, and the same drop_seed / drop_p.
 * gm[s]: gradient w.r.t. motion_<site>.  grads: the flat buffer above; accumulate != 0 adds to it (the
 * reference calls backward three times per step, train_off.py:141-143), otherwise it is overwritten.
 * Every reduction has a fixed order: results are bit-reproducible.  NCHW feature maps only (channels-last maps:
 * offk_off_units_backward_cl below).
 * Non-finite values (this entry and offk_off_units_backward_split, whose two weight matrices then hold NaN; tests/test_gpu_train_ranges.py).
 * The parameter gradients read the maps, g and the forward's G (as a mask: a select), not Wg, Wd or the biases.  A +-Inf or NaN in g at
 * spatial channel j of a site makes exactly down.weight[j, :], down.bias[j] and the depthwise conv's weight[j] and bias[j] of that site
 * non-finite; at temporal channel o, where the forward's G is positive in one of the pair's two frames, exactly gen.weight[o, :] and
 * gen.bias[o]; in x[n, c, y, x] (seen by forward and backward alike) exactly gen.weight[:, c], down.weight[:, c] (a frame of the slice)
 * and the depthwise weight of that site, whose other gradients stay finite (the pixel's ReLU mask changed).  Every other element, and
 * every other site, is bit-equal to the run without the value. */
int offk_off_units_backward(offk_handle* h, void* stream, const float* const feats[OFFK_NUM_SITES],
                            const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed, double drop_p,
                            float* grads, int accumulate);

/* ---- 16-bit feature maps on the training side (additive; ABI version unchanged) -----------
 * The backbone is frozen in training (train_off.py:39-56) and is what runs under autocast, so its nine maps arrive as
 * bf16 / fp16.  These four entries are offk_pw_reduce, offk_off_units, offk_off_units_train and offk_off_units_backward
 * on such maps as they are: NCHW [B*L, C_i, H_i, H_i] of `feat_dtype` (enum offk_feat_dtype), no fp32 copy.
 * OFFK_FEAT_F32 forwards to the untyped entry.  Outputs, gradients and the workspace stay fp32, and
 * offk_train_workspace_bytes is unchanged.
 *
 * Unlike offk_forward_typed they make no condition on the handle: both precisions (a handle's precision does not choose the
 * training side's kernels: these entries run the fp32 kernels, the _split entries below are the opt-in), weights bound through offk_bind_weight, any OFFK_FUSED_UNITS setting (they run the
 * two-kernel form K1 + K2, never the fused kernel).  Only the two kernels that read the maps have 16-bit forms: K1
 * (the stacked 1x1 reduces) and K1b (the weight-gradient GEMM dW = A^T X); K2, K2b and the reductions are the untyped
 * entries' own launches.
 *
 * Contract: EQUAL VALUES, not a tolerance.  For the same handle, weights, seed and cotangents, everything a typed call
 * writes -- G_<site>, D_<site>, the unit channels of fusion_28/14/7, the whole flat gradient buffer in both accumulate
 * modes -- is bit-equal to what the untyped call writes from the maps widened to fp32 (x.float()); not even the sign of a
 * zero differs.  Why: a 16-bit loader reads the elements, widens each in registers to the exact fp32 value it stands for
 * (bf16: a 16-bit shift; fp16: the hardware conversion, subnormals included) and stores it into the LDS position the fp32
 * loader uses.  From the LDS store on the 16-bit forms are the same kernel text as the fp32 ones: the same fp32 operands
 * in the same LDS slots, the same MFMA sequence in the same order, the same epilogue and slab layout, the same
 * wgrad reduction.  The launch plan does not depend on feat_dtype either: block count, rows per block, the split-K
 * chunking of K1b, slab sizes and every summation order are the untyped call's.  Rows past the end of a site read zeros
 * (K1: through an out-of-range buffer offset; K1b: from the handle's zero page, which serves as 16-bit zeros unchanged).
 *
 * Refused with OFFK_ERR_INVALID before anything is enqueued: an unknown feat_dtype; an NHWC handle; a null map; a map
 * pointer that is not 8-byte aligned (the 14x14 / 28x28 sites fetch four pixels per 8-byte load; every row of those maps
 * then is 8-byte aligned, the 98-byte rows of the 7x7 sites are read with 2-byte loads); a single map of 2 GiB or more
 * (the 16-bit loader of K1 exists in the buffer-descriptor form only).  The untyped entries' own checks (dropout
 * probability, gradient views) apply unchanged. */
int offk_pw_reduce_typed(offk_handle* h, void* stream, int feat_dtype, int site, const void* feat, float* G, float* D);
int offk_off_units_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                         void* workspace);
int offk_off_units_train_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                               void* workspace, uint64_t drop_seed, double drop_p);
int offk_off_units_backward_typed(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                                  const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed,
                                  double drop_p, float* grads, int accumulate);

/* ---- channels-last feature maps on the training side (additive; ABI version unchanged) -----------
 * A frozen backbone run in torch.channels_last hands over NHWC-strided maps.  These four entries are offk_pw_reduce,
 * offk_off_units, offk_off_units_train and offk_off_units_backward on such maps as they are, argument for argument the
 * _typed entries above:
 *   feat_dtype OFFK_FEAT_F32 / _BF16 / _F16 (OFFK_FEAT_F32 is a form of its own here, not a forward to the untyped entry);
 *   feats[i] (feat): the channels-last image [B*L*H_i*H_i][C_i] of the logical [B*L, C_i, H_i, H_i] map, elements of
 *   feat_dtype, 16-byte aligned.
 * The layout belongs to the call, as in offk_forward_cl: cfg.feat_layout keeps describing what the untyped entries are
 * given and is not looked at here.  No condition on the handle either: both precisions, bound or set weights, any
 * OFFK_FUSED_UNITS setting (K1 + K2, never the fused kernel).  Outputs, gradients and the workspace stay fp32;
 * offk_train_workspace_bytes is unchanged.
 *
 * Contract: EQUAL VALUES, not a tolerance.  Everything a _cl call writes -- G_<site>, D_<site>, the unit channels of
 * fusion_28/14/7, the whole flat gradient buffer in both accumulate modes -- is bit-equal to what the untyped / _typed
 * call of the same feat_dtype writes from the NCHW copy of the same logical tensors.  Why: only the loaders of K1 and
 * K1b differ.  K1 reads four consecutive channels of a row per load (fp32: 16 bytes, the kernel's existing channels-last
 * loader, now chosen per call; 16-bit: 8 bytes through a buffer descriptor, widened on the way into LDS); K1b reads four
 * consecutive channels of a pixel per load and transposes 4 x 4 in registers, as it always did for dG.  Both fill
 * exactly the LDS image the NCHW loaders fill, in front of the same MFMA sequence, epilogue, slab layout and launch plan.
 * Rows / pixels past the end of a site read zeros (K1 16-bit: an out-of-range buffer offset; K1b: the zero page).
 *
 * Refused with OFFK_ERR_INVALID before anything is enqueued: an unknown feat_dtype; a null map; a map pointer that is
 * not 16-byte aligned; a single 16-bit map of 2 GiB or more (K1's 16-bit loaders address through a buffer descriptor;
 * fp32 maps have no such limit).  The untyped entries' own checks (dropout probability, gradient views) apply unchanged.
 * The _typed entries keep refusing an NHWC handle: their maps are NCHW. */
int offk_pw_reduce_cl(offk_handle* h, void* stream, int feat_dtype, int site, const void* feat, float* G, float* D);
int offk_off_units_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                      void* workspace);
int offk_off_units_train_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                            void* workspace, uint64_t drop_seed, double drop_p);
int offk_off_units_backward_cl(offk_handle* h, void* stream, int feat_dtype, const void* const feats[OFFK_NUM_SITES],
                               const offk_grad_view gm[OFFK_NUM_SITES], void* workspace, uint64_t drop_seed,
                               double drop_p, float* grads, int accumulate);

/* ---- gradient w.r.t. the nine feature maps (additive; ABI version unchanged) -----------
 * The reference's training scripts freeze the backbone (train_off.py:39-56), so the entries above give parameter gradients
 * only.  A caller that un-freezes inception_5a / 5b (the usual TSN partial fine-tune) or the whole backbone for a joint last
 * stage needs dX as well, and it is linear in what the backward already left behind:
 *   dX[frame n, pixel, c] = sum_o dGpre[n, pixel, o] Wg[o, c]                     (all B*L frames)
 *                         + sum_j dD[r(n), pixel, j] Wd[j, c]                     (frames inside the spatial slice only)
 *   r(n): OFFK_SLICE_REFERENCE_FLAT: r = n for n < B*(L-1), none above; OFFK_SLICE_PER_CLIP: frame (b, t), t < L-1 ->
 *   r = b*(L-1) + t, none for t = L-1.
 * It needs neither the maps, the dropout seed nor the maps' dtype, so there is one entry for all three backward forms.
 *
 * Gradient w.r.t. the feature maps, from the dG_<site> / dD_<site> regions the LAST offk_off_units_backward
 * (any of its three forms) on `h` left in `workspace`, and the gen / down weights as they are at launch time
 * (bound: read in place -> enqueue before the optimizer step).  dfeats[i] == NULL: site i is skipped.
 * layout: OFFK_FEAT_NCHW ([B*L, C_i, H_i, H_i]) or OFFK_FEAT_NHWC ([B*L*H_i*H_i][C_i]), fp32, 16-byte aligned,
 * not overlapping `workspace`.  accumulate != 0 adds (out = old + new, new being the bits the overwrite form stores).
 * One launch on `stream` (csrc/units_dx.hip), no sync, no allocation, capturable.
 * Exact fp32 on the fp32 matrix pipe whatever the handle's precision (the training side's three GEMMs run in split-fp32
 * arithmetic only through the opt-in _split entries below, on any handle), a fixed k order, no atomics: bit-reproducible, and the two layouts hold the same sums bit for bit.
 * Refused with OFFK_ERR_INVALID, nothing enqueued: a null h, workspace or dfeats; an unknown layout; a pointer that is not
 * 16-byte aligned; a buffer that overlaps the offk_train_workspace_bytes of `workspace`; a handle on which no
 * offk_off_units_backward* has run since offk_create.  That last check is a flag the backward entries set on the handle: a
 * backward replayed from a captured graph does not pass through the library and sets none (as for offk_stage_tensors) -- run
 * one backward through the library first.  The library cannot see how large `workspace` is: it must be the train workspace
 * (offk_train_workspace_bytes), the one the backward wrote.  All nine pointers NULL: OFFK_OK, nothing enqueued.
 * Range and non-finite values (this entry and its _split form, which gives NaN; tests/test_gpu_train_ranges.py): g times 2^a scales dX by
 * exactly 2^a; a +-Inf or NaN in dGpre or dD reaches all channels of its own pixel (dD: of the frame whose row it is) and no other
 * element; in Wg[o, c] channel c of every pixel of every frame; in Wd[j, c] channel c of every frame too -- also of the frames outside
 * the slice, whose dD part is a row of zeros times it (0 * Inf = NaN).  Every other element, every other site, is bit-equal.
 * Per-launch trace: "units:feature-map gradient (dX, NCHW)" / "... (dX, NHWC)". */
int offk_off_units_backward_feats(offk_handle* h, void* stream, void* workspace,
                                  float* const dfeats[OFFK_NUM_SITES], int layout, int accumulate);

/* ---- the same gradient in the maps' own 16-bit dtype (additive; ABI version unchanged) -----------
 * An un-frozen backbone under autocast hands over bf16 / fp16 maps and wants their gradients in that dtype.  The kernel holds
 * every finished fp32 sum in a register in front of its store, so it rounds there: no fp32 dX buffer, no cast kernels.
 * grad_dtype: enum offk_feat_dtype, one per call.  OFFK_FEAT_F32 forwards to offk_off_units_backward_feats (dfeats cast to
 * float* const*): same launch, same bits.  OFFK_FEAT_BF16 / OFFK_FEAT_F16: dfeats[i] is [B*L, C_i, H_i, H_i] (OFFK_FEAT_NCHW) or
 * [B*L*H_i*H_i][C_i] (OFFK_FEAT_NHWC) in that element type.
 * Rounding: every fp32 sum is rounded ONCE, to nearest-even, to grad_dtype.  For finite sums every element is the fp32 entry's
 * element rounded to nearest-even: the result is bit-equal to dx32.to(dtype), dx32 being what the overwrite form of
 * offk_off_units_backward_feats stores.  fp16 overflow gives +-Inf (so does a bf16 sum above the largest finite bf16); fp16
 * subnormal results are kept, not flushed.
 * accumulate != 0: out = rne16(widen(old) + new) -- the old 16-bit element widened exactly to fp32, ONE fp32 add of the finished
 * sum, ONE rounding; the partial sums never pass through 16 bits: bit-equal to (old.float() + dx32).to(dtype).
 * Equal bits across the two layouts, across runs and under graph replay follow from that.  A NaN, or the sign of a zero sum, is
 * outside the equality.
 * Everything else is offk_off_units_backward_feats': a NULL site is skipped, all nine NULL is OFFK_OK with nothing enqueued;
 * pointers 16-byte aligned; no buffer may overlap the offk_train_workspace_bytes of `workspace` (tested with the buffer's real
 * byte size, 2 bytes per element here); the handle's backward-has-run flag; weights read as they are at launch; one launch on
 * `stream` (csrc/units_dx_f16.hip: the fp32 kernel's body with a 16-bit epilogue), no sync, no allocation, capturable.
 * Refused with OFFK_ERR_INVALID, nothing enqueued: the fp32 entry's refusals, plus an unknown grad_dtype.
 * Per-launch trace: "units:feature-map gradient (dX, NCHW, bf16)" / "(dX, NHWC, bf16)" / "(dX, NCHW, fp16)" / "(dX, NHWC, fp16)". */
int offk_off_units_backward_feats_typed(offk_handle* h, void* stream, void* workspace, int grad_dtype,
                                        void* const dfeats[OFFK_NUM_SITES], int layout, int accumulate);

/* ---- the same gradient in split-fp32 arithmetic on the bf16 matrix pipe (additive, opt-in; ABI version unchanged) -----------
 * The first piece of the training side in the arithmetic of OFFK_PRECISION_F32SPLIT; it works on ANY handle, whatever its
 * precision, and the entries above stay the default with their contract (exact fp32 on the fp32 matrix pipe).
 * Arithmetic: dX[n, q, c] = sum_{k < 160} a[n, q, k] w[c, k], a = [dGpre | dD at row r(n), zeros for a frame outside the slice],
 * w[c] = [Wg[:, c] ; Wd[:, c]].  Both fp32 operands are cut into THREE bf16 planes by truncation (exactly: h + m + l == value);
 * per 32-k step six of the nine plane products run on v_mfma_f32_16x16x32_bf16, w_h a_h into one fp32 accumulator and the five
 * small ones (w_l a_h, w_h a_l, w_m a_m, w_m a_h, w_h a_m, in that order) into a second, five steps in increasing k (gen
 * channels, then down), out = A1 + A2 once in the epilogue.  The three dropped products are below (2^-21 + 2^-30) sum|a w| per
 * element; to that come the fp32 accumulation of the two accumulators and the one epilogue add.  +-Inf in an operand gives NaN
 * (Inf - Inf in the cut), and tiny operands behave as the split-mode paragraph at OFFK_PRECISION_F32SPLIT says (below 2^-109 an
 * operand's last plane falls under the last bf16 subnormal).  No split-K, no atomics, one fixed order.
 * Equal bits: across the two layouts, across runs and under graph replay.  It is NOT bit-equal to offk_off_units_backward_feats.
 * grad_dtype: enum offk_feat_dtype, OFFK_FEAT_F32 included (dfeats[i] then points at fp32).  The 16-bit forms round each
 * finished fp32 sum ONCE, to nearest-even: for finite sums they are dx32s.to(dtype), and with accumulate != 0
 * (old.float() + dx32s).to(dtype), bit for bit, dx32s being what the fp32 overwrite form of THIS entry stores (a NaN, or the
 * sign of a zero sum, is outside the equality).  fp32 with accumulate: out = old + dx32s.  fp16 overflow gives +-Inf, fp16
 * subnormal results are kept.
 * TWO launches on `stream` (csrc/units_dx_split.hip): a pre-pass that cuts [Wg ; Wd] of the requested sites, as they are at
 * launch time (bound weights: read in place -> enqueue before the optimizer step), into a plane image the handle owns (5.3 MB,
 * allocated at offk_create), then the GEMM.  No sync, no allocation, capturable.  The image is per handle: two calls on one
 * handle must be ordered (one stream, or an event), like every other use of the handle's buffers.
 * Everything else is offk_off_units_backward_feats_typed's: a NULL site is skipped, all nine NULL is OFFK_OK with nothing
 * enqueued; pointers 16-byte aligned; no buffer may overlap the offk_train_workspace_bytes of `workspace` (tested with the
 * buffer's real byte size); the handle's backward-has-run flag.  Refused with OFFK_ERR_INVALID, nothing enqueued: a null h,
 * workspace or dfeats, an unknown layout or grad_dtype, a misaligned pointer, an overlap, no backward run yet.
 * Per-launch trace: "units:feature-map gradient (dX, NCHW, split)" / "(dX, NHWC, split)", with ", bf16" / ", fp16" behind
 * "split" for the 16-bit forms. */
int offk_off_units_backward_feats_split(offk_handle* h, void* stream, void* workspace, int grad_dtype,
                                        void* const dfeats[OFFK_NUM_SITES], int layout, int accumulate);

/* ---- the units' backward with the weight gradient in split-fp32 arithmetic on the bf16 matrix pipe (additive, opt-in; ABI version unchanged) -----------
 * The second piece of the training side in the arithmetic of OFFK_PRECISION_F32SPLIT: offk_off_units_backward, _typed and _cl in one
 * entry whose largest kernel, the weight-gradient GEMM K1b (dW[160][C] = [dGpre | dD]^T X), runs on v_mfma_f32_16x16x32_bf16.  It works
 * on ANY handle -- either precision, bound or set weights, any OFFK_FUSED_UNITS setting -- and is opt-in: the three entries above keep
 * their kernels and their contracts, and a split-fp32 handle does not switch it on by itself.
 * feat_dtype: enum offk_feat_dtype, OFFK_FEAT_F32 included.  layout: OFFK_FEAT_NCHW (feats[i] = [B*L, C_i, H_i, H_i], what
 * offk_off_units_backward / _typed take) or OFFK_FEAT_NHWC (the channels-last image [B*L*H_i*H_i][C_i], what offk_off_units_backward_cl
 * takes); the layout belongs to the call, as in the _cl entries.  Every other argument is offk_off_units_backward's.
 * Arithmetic: for site s, dW[m][c] = sum over (frame f, pixel q) a[(f, q)][m] X[f][c][q], a = [dGpre (128) | dD at row r(f) (32), zeros
 * for a frame outside the spatial slice].  Both operands are cut into THREE bf16 planes by truncation (exactly: h + m + l == value).  A
 * k step is K1b's K-tile: 32 pixels of one frame, ceil(HW / 32) per frame, pad pixels zeros.  Per step six of the nine plane products
 * are issued, a_h x_h into one fp32 accumulator and the five small ones (a_l x_h, a_h x_l, a_m x_m, a_m x_h, a_h x_m, in that order)
 * into a second; steps in increasing K-tile order over K1b's chunk of K-tiles, partial tile = A1 + A2 once, and the unchanged reduce
 * sums the per-chunk slabs in chunk order and then adds `accumulate`.  The three dropped products are below (2^-21 + 2^-30) sum|a x|
 * per element; to that come the fp32 accumulation of the two accumulators, the one A1 + A2 add and the slab sums.
 * bf16 maps: a bf16 value IS its leading plane, so only the three products with x_h exist and NOTHING is dropped.  fp16 maps: an fp16
 * value is exactly two planes, the five products without x_l are issued and only a_l x_m is dropped (below 2^-22 sum|a x|).  Both are
 * compile-time forms that leave out MFMAs which would have added +-0.
 * Equal bits: the result on bf16 / fp16 maps equals this entry's result on x.float() element for element (only the sign of a zero may
 * differ); NCHW and channels-last maps of the same logical tensor give the same bits; so do two runs, and a captured graph's replay.
 * Every bias gradient, every depthwise weight / bias gradient and the dG_<site> / dD_<site> regions are bit-equal to what
 * offk_off_units_backward* writes (the same launches, respectively the same sums in the same order), so every
 * offk_off_units_backward_feats* entry works behind this one exactly as behind those (it sets the same backward-has-run flag).
 * It is NOT bit-equal to offk_off_units_backward* for the two weight matrices (motion_conv_gen_*.weight, motion_spatial_down_*.weight).
 * +-Inf in an operand gives NaN (Inf - Inf in the cut), and tiny operands behave as the split-mode paragraph at OFFK_PRECISION_F32SPLIT
 * says (below 2^-109 an operand's last plane falls under the last bf16 subnormal).
 * The launch plan and the workspace are K1b's: the same blocks, chunks, slabs ("wgs_<site>") and bias partials ("wgb_<site>"), no split-K
 * beyond those chunks, no atomics, one fixed order: bit-reproducible.  offk_train_workspace_bytes is unchanged.
 * THREE launches on `stream`: K2b and the reduce as offk_off_units_backward enqueues them, between them the GEMM of
 * csrc/units_wgrad_split.hip.  No sync, no allocation, capturable.
 * Refused with OFFK_ERR_INVALID before anything is enqueued: a null h, feats, gm, workspace or grads; an unknown layout or feat_dtype;
 * for OFFK_FEAT_NCHW what offk_off_units_backward_typed refuses (an NHWC handle, a null map, a 16-bit map pointer that is not 8-byte
 * aligned, a single 16-bit map of 2 GiB or more); for OFFK_FEAT_NHWC what offk_off_units_backward_cl refuses (a null map, a map
 * pointer that is not 16-byte aligned, a single 16-bit map of 2 GiB or more); and the untyped entry's own checks (dropout probability
 * outside [0, 1), a gradient view without 16-byte aligned 160 channels inside its cstride). */
int offk_off_units_backward_split(offk_handle* h, void* stream, int feat_dtype, int layout,
                                  const void* const feats[OFFK_NUM_SITES], const offk_grad_view gm[OFFK_NUM_SITES],
                                  void* workspace, uint64_t drop_seed, double drop_p, float* grads, int accumulate);

/* ---- the units' train forward with the 1x1 reduces in split-fp32 arithmetic on the bf16 matrix pipe (additive, opt-in; ABI version unchanged) -----------
 * The third and last piece of the training side in the arithmetic of OFFK_PRECISION_F32SPLIT: offk_off_units_train, _typed and _cl in one
 * entry whose largest kernel, K1 (the stacked 1x1 reduces G = relu(Wg X + bg) on all frames, D = Wd X + bd on the frames of the spatial
 * slice), runs on v_mfma_f32_16x16x32_bf16.  It works on ANY handle -- either precision, bound or set weights, any OFFK_FUSED_UNITS
 * setting -- and is opt-in: the entries above keep their kernels and their contracts, and a split-fp32 handle does not switch it on by
 * itself.  drop_p = 0 is eval mode: the entry then stands for offk_off_units / _typed / _cl as well.
 * feat_dtype: enum offk_feat_dtype, OFFK_FEAT_F32 included.  layout: OFFK_FEAT_NCHW (feats[i] = [B*L, C_i, H_i, H_i]) or OFFK_FEAT_NHWC
 * (the channels-last image [B*L*H_i*H_i][C_i]); the layout belongs to the call.  Every other argument is offk_off_units_train's.
 * Arithmetic: both operands are cut into THREE bf16 planes by truncation (exactly: h + m + l == value).  A k step is 32 consecutive
 * channels; the steps run in increasing channel order over the whole C_i; channel 32 kt + 8 g + e sits in lane group g, element e of
 * step kt.  Per step six of the nine plane products are issued, w_h x_h into one fp32 accumulator A1 and the five small ones (w_l x_h,
 * w_h x_l, w_m x_m, w_m x_h, w_h x_m, in that order) into a second, A2; no split-K, no atomics; v = (A1 + A2) + bias, G = max(v, 0),
 * D = v.  The three dropped products are below (2^-21 + 2^-30) sum|w x| per element; to that come the fp32 accumulation of the two
 * accumulators, the one A1 + A2 add and the bias add.
 * bf16 maps: a bf16 value IS its leading plane, so only the three products with x_h exist and NOTHING is dropped.  fp16 maps: an fp16
 * value is exactly two planes, the five products without x_l are issued and only w_l x_m is dropped.  Both are compile-time forms that
 * leave out MFMAs which would have added +-0.
 * +-Inf in an operand gives NaN (Inf - Inf in the cut), and tiny operands behave as the split-mode paragraph at OFFK_PRECISION_F32SPLIT
 * says (below 2^-109 an operand's last plane falls under the last bf16 subnormal).
 * Equal bits: D_<site> and the temporal channels of fusion_28 / _14 / _7 equal what offk_off_units_fused writes on a split-fp32 handle
 * for the same fp32 NCHW maps and weights (the same arithmetic in front of the temporal difference; only the sign of a zero may
 * differ); the result on bf16 / fp16 maps equals this entry's result on x.float(); NCHW and channels-last maps of the same logical
 * tensor give the same bits; so do two runs, a captured graph's replay, and bound against set weights.  G_<site> / D_<site> are NOT
 * bit-equal to what offk_off_units_train* / offk_off_units* write.  They lie in the same workspace regions in the same layout, so K2 and
 * every offk_off_units_backward* / _feats* entry run behind this one unchanged.
 * THREE launches on `stream`: a pre-pass that cuts [Wg ; Wd] of the nine sites, as they are at launch time (bound weights: read in
 * place, an in-place update is picked up by the next call), into a plane image the handle owns (5,345,280 bytes, allocated at
 * offk_create; a buffer of its own, neither the dX image nor the fused kernel's), the GEMM of csrc/units_fwd_split.hip, and K2 exactly
 * as offk_off_units_train enqueues it.  No sync, no allocation, capturable; offk_train_workspace_bytes and offk_workspace_bytes are
 * unchanged.  The image is per handle: two calls on one handle must be ordered (one stream, or an event), like every other use of the
 * handle's buffers.
 * Refused with OFFK_ERR_INVALID before anything is enqueued: a null h, feats or workspace ("offk_off_units_train_split: null
 * argument"); an unknown layout or feat_dtype; a dropout probability outside [0, 1); for OFFK_FEAT_NCHW what
 * offk_off_units_train_typed refuses (an NHWC handle, a null map, a 16-bit map pointer that is not 8-byte aligned, a single 16-bit map
 * of 2 GiB or more); for OFFK_FEAT_NHWC what offk_off_units_train_cl refuses (a null map, a map pointer that is not 16-byte aligned, a
 * single 16-bit map of 2 GiB or more).
 * Per-launch trace: "units:pw_reduce weight cut (K1, split)", then "units:pw_reduce (K1, NCHW, split)" / "(K1, NHWC, split)", with
 * ", bf16" / ", fp16" behind "split" for 16-bit maps, then "units:sobel_tdiff (K2)". */
int offk_off_units_train_split(offk_handle* h, void* stream, int feat_dtype, int layout,
                               const void* const feats[OFFK_NUM_SITES], void* workspace,
                               uint64_t drop_seed, double drop_p);

/* Backward of offk_segment_consensus, basic_ops.py:29-33: grad_in[b*T + t][c] = grad_out[b][c] / T. */
int offk_segment_consensus_backward(void* stream, const float* grad_out, int B, int T, int C, float* grad_in);

/* NCHW <-> channels-last helpers (device pointers), used by tests and by callers that
 * want a reference-layout view of an internal buffer. */
int offk_nchw_to_nhwc(void* stream, const float* src, int n_img, int C, int HW, float* dst);
int offk_nhwc_to_nchw(void* stream, const float* src, int cstride, int coff, int n_img, int C, int HW, float* dst);

#ifdef __cplusplus
}
#endif
#endif /* OFFK_H_ */
