"""The argument lists and refusal tables of the stride-1 fusion convs' backward entries that the CPU ABI tests share
(tests/test_conv_bwd_abi.py, test_conv_wgrad_split_abi.py, test_conv_dgrad_split_abi.py, test_conv_bwd_entries.py): fake pointers that
are never dereferenced, one valid argument list per entry with keyword overrides, every refusal of the fp32 entries and what the split
twins refuse beside it.  A helper module: no tests of its own."""
import ctypes


def fake(addr):
    return ctypes.c_void_p(addr)


N, H, CI, CO = 2, 14, 64, 128
ROWS = N * H * H
BIG = 1 << 30                     # bytes: no plan of these shapes comes near


def data_args(**over):
    a = dict(stream=None, g=fake(0x10000000), g_cstride=CO, g_coff=0, n_img=N, H=H, W=H, Co=CO, w=fake(0x1000), Ci=CI, KH=3, KW=3,
             pad=1, dx=fake(0x20000000), dx_cstride=CI, dx_coff=0, accumulate=0, scratch=fake(0x30000000), scratch_bytes=BIG)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def weight_args(**over):
    a = dict(stream=None, x=fake(0x20000000), x_cstride=CI, x_coff=0, g=fake(0x10000000), g_cstride=CO, g_coff=0, n_img=N, H=H, W=H,
             Ci=CI, Co=CO, KH=3, KW=3, pad=1, relu_in=0, dw=fake(0x1000), db=fake(0x2000), accumulate=0, scratch=fake(0x30000000),
             scratch_bytes=BIG)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def relu_args(**over):
    a = dict(stream=None, dy=fake(0x10000000), dy_cstride=CO, dy_coff=0, y=fake(0x20000000), y_cstride=CO, y_coff=0, rows=ROWS, C=CO,
             g=fake(0x30000000), g_cstride=CO, g_coff=0, accumulate=0)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


G_BYTES = ROWS * CO * 4
REFUSALS = {
    "data_null_g": ("offk_conv2d_backward_data", data_args, dict(g=None)),
    "data_null_w": ("offk_conv2d_backward_data", data_args, dict(w=None)),
    "data_null_dx": ("offk_conv2d_backward_data", data_args, dict(dx=None)),
    "data_null_scratch": ("offk_conv2d_backward_data", data_args, dict(scratch=None)),
    "data_ci_96": ("offk_conv2d_backward_data", data_args, dict(Ci=96, dx_cstride=96)),
    "data_kh_5": ("offk_conv2d_backward_data", data_args, dict(KH=5, KW=5, pad=2)),
    "data_pad_not_half": ("offk_conv2d_backward_data", data_args, dict(pad=0)),
    "data_g_stride_short": ("offk_conv2d_backward_data", data_args, dict(g_cstride=CO, g_coff=64)),
    "data_dx_stride_short": ("offk_conv2d_backward_data", data_args, dict(dx_cstride=32)),
    "data_negative_offset": ("offk_conv2d_backward_data", data_args, dict(dx_coff=-4, dx_cstride=256)),
    "data_short_scratch": ("offk_conv2d_backward_data", data_args, dict(scratch_bytes=4 * CO * CI * 9 - 4)),
    "data_dx_is_g": ("offk_conv2d_backward_data", data_args, dict(dx=fake(0x10000000))),
    "data_dx_overlaps_g_tail": ("offk_conv2d_backward_data", data_args, dict(dx=fake(0x10000000 + G_BYTES - 1024))),
    "data_dx_slice_of_g_buffer": ("offk_conv2d_backward_data", data_args, dict(g_cstride=256, dx=fake(0x10000000), dx_cstride=256, dx_coff=128)),
    "weight_null_x": ("offk_conv2d_backward_weight", weight_args, dict(x=None)),
    "weight_null_g": ("offk_conv2d_backward_weight", weight_args, dict(g=None)),
    "weight_null_dw": ("offk_conv2d_backward_weight", weight_args, dict(dw=None)),
    "weight_null_scratch": ("offk_conv2d_backward_weight", weight_args, dict(scratch=None)),
    "weight_ci_96": ("offk_conv2d_backward_weight", weight_args, dict(Ci=96, x_cstride=96)),
    "weight_kh_5": ("offk_conv2d_backward_weight", weight_args, dict(KH=5, KW=5, pad=2)),
    "weight_pad_not_half": ("offk_conv2d_backward_weight", weight_args, dict(pad=2)),
    "weight_x_stride_short": ("offk_conv2d_backward_weight", weight_args, dict(x_cstride=128, x_coff=96)),
    "weight_g_stride_short": ("offk_conv2d_backward_weight", weight_args, dict(g_cstride=64)),
    "weight_odd_offset": ("offk_conv2d_backward_weight", weight_args, dict(x_cstride=130, x_coff=2)),
    "weight_short_scratch": ("offk_conv2d_backward_weight", weight_args, dict(scratch_bytes=4 * (CO * CI * 9 + CO) - 4)),
    "relu_null_dy": ("offk_relu_backward", relu_args, dict(dy=None)),
    "relu_null_y": ("offk_relu_backward", relu_args, dict(y=None)),
    "relu_null_g": ("offk_relu_backward", relu_args, dict(g=None)),
    "relu_stride_short": ("offk_relu_backward", relu_args, dict(g_cstride=CO, g_coff=4)),
    "relu_partial_overlap": ("offk_relu_backward", relu_args, dict(g=fake(0x10000000 + 4096))),
    "relu_same_pointer_other_offset": ("offk_relu_backward", relu_args, dict(dy_cstride=256, g=fake(0x10000000), g_cstride=256, g_coff=128)),
    "relu_g_overlaps_y": ("offk_relu_backward", relu_args, dict(g=fake(0x20000000 + 256))),
    "plan_ci_96": ("offk_conv2d_backward_plan", lambda **o: [2, 14, 14, 96, 64, 3, 3, None, None, None], {}),
    "plan_kh_5": ("offk_conv2d_backward_plan", lambda **o: [2, 14, 14, 64, 64, 5, 5, None, None, None], {}),
}


def round256(b):
    return -(-b // 256) * 256


# ---- the split weight gradient: every refusal of the fp32 entry (REFUSALS above), asked of the split entry;
# the scratch one byte short of the split plan's
WGRAD_SPLIT_SCRATCH = 4 * (CO * CI * 9 + CO)        # (2, 14, 14, 64, 128, 3): one chunk
WGRAD_SPLIT_REFUSALS = dict((rule, over) for rule, (entry, _make, over) in REFUSALS.items() if entry == "offk_conv2d_backward_weight")
WGRAD_SPLIT_REFUSALS["weight_short_scratch"] = dict(scratch_bytes=WGRAD_SPLIT_SCRATCH - 1)
WGRAD_SPLIT_REFUSALS.update(weight_kh_2=dict(KH=2, KW=2, pad=0), weight_kh_not_kw=dict(KH=3, KW=1), weight_co_96=dict(Co=96, g_cstride=96),
                            weight_negative_offset=dict(x_coff=-4, x_cstride=256), weight_g_negative_offset=dict(g_coff=-4, g_cstride=256),
                            weight_g_odd_stride=dict(g_cstride=130), weight_n_img_0=dict(n_img=0))

# ---- the split data gradient: every refusal of the fp32 data entry (REFUSALS above), asked of the split entry;
# the scratch one byte short of the split plan's
DGRAD_SPLIT_SCRATCH = round256(9 * CO * CI * 6) + round256(ROWS * CO * 6)
DGRAD_SPLIT_REFUSALS = dict((rule, over) for rule, (entry, _make, over) in REFUSALS.items() if entry == "offk_conv2d_backward_data")
DGRAD_SPLIT_REFUSALS["data_short_scratch"] = dict(scratch_bytes=DGRAD_SPLIT_SCRATCH - 1)
DGRAD_SPLIT_REFUSALS.update(data_kh_7=dict(KH=7, KW=7, pad=3), data_kh_not_kw=dict(KW=1), data_co_96=dict(Co=96, g_cstride=96), data_n_img_0=dict(n_img=0),
                            data_h_0=dict(H=0), data_g_negative_offset=dict(g_coff=-4, g_cstride=256), data_odd_offset=dict(dx_cstride=130, dx_coff=2),
                            data_scratch_not_aligned=dict(scratch=ctypes.c_void_p(0x30000008)))
