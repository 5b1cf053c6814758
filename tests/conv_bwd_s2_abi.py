"""The argument lists and refusal tables of the stride-2 fusion convs' backward entries that the CPU ABI tests share
(tests/test_conv_bwd_s2_abi.py, test_conv_s2_wgrad_split_abi.py, test_conv_s2_dgrad_split_abi.py, test_conv_bwd_entries.py), as
tests/conv_bwd_abi.py holds them for stride 1.  A helper module: no tests of its own."""
from .conv_bwd_abi import fake


N, H, CI, CO = 2, 14, 96, 128
G_BYTES = N * (H // 2) * (H // 2) * CO * 4
BIG = 1 << 30                     # bytes: no plan of these shapes comes near


def data_args(**over):
    a = dict(stream=None, g=fake(0x10000000), g_cstride=CO, g_coff=0, n_img=N, H=H, W=H, Co=CO, w=fake(0x1000), Ci=CI, KH=5, KW=5,
             pad=2, dx=fake(0x20000000), dx_cstride=CI, dx_coff=0, accumulate=0, scratch=fake(0x30000000), scratch_bytes=BIG)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def weight_args(**over):
    a = dict(stream=None, x=fake(0x20000000), x_cstride=CI, x_coff=0, g=fake(0x10000000), g_cstride=CO, g_coff=0, n_img=N, H=H, W=H,
             Ci=CI, Co=CO, KH=5, KW=5, pad=2, relu_in=0, dw=fake(0x1000), db=fake(0x2000), accumulate=0, scratch=fake(0x30000000),
             scratch_bytes=BIG)
    assert set(over) <= set(a)
    a.update(over)
    return list(a.values())


def plan_args(n=2, H=14, W=14, ci=96, co=128, kh=5, kw=5):
    return [n, H, W, ci, co, kh, kw, None, None, None]


DATA, WEIGHT, PLAN = "offk_conv2d_s2_backward_data", "offk_conv2d_s2_backward_weight", "offk_conv2d_s2_backward_plan"
REFUSALS = {
    "data_null_g": (DATA, data_args, dict(g=None)),
    "data_null_w": (DATA, data_args, dict(w=None)),
    "data_null_dx": (DATA, data_args, dict(dx=None)),
    "data_null_scratch": (DATA, data_args, dict(scratch=None)),
    "data_k3": (DATA, data_args, dict(KH=3, KW=3, pad=1)),
    "data_k7_pad2": (DATA, data_args, dict(KH=7, KW=7, pad=2)),
    "data_k5_pad3": (DATA, data_args, dict(pad=3)),
    "data_k5x7": (DATA, data_args, dict(KH=5, KW=7)),
    "data_odd_h": (DATA, data_args, dict(H=13)),
    "data_odd_w": (DATA, data_args, dict(W=15)),
    "data_ci_48": (DATA, data_args, dict(Ci=48, dx_cstride=48)),
    "data_co_96": (DATA, data_args, dict(Co=96, g_cstride=96)),
    "data_g_stride_short": (DATA, data_args, dict(g_cstride=CO, g_coff=64)),
    "data_dx_stride_short": (DATA, data_args, dict(dx_cstride=64)),
    "data_negative_offset": (DATA, data_args, dict(dx_coff=-4, dx_cstride=256)),
    "data_odd_offset": (DATA, data_args, dict(g_cstride=CO + 2, g_coff=2)),
    "data_short_scratch": (DATA, data_args, dict(scratch_bytes=4 * CO * CI * 25 - 4)),
    "data_dx_is_g": (DATA, data_args, dict(dx=fake(0x10000000))),
    "data_dx_overlaps_g_tail": (DATA, data_args, dict(dx=fake(0x10000000 + G_BYTES - 1024))),
    "data_g_inside_dx": (DATA, data_args, dict(g=fake(0x20000000 + 4096))),
    "weight_null_x": (WEIGHT, weight_args, dict(x=None)),
    "weight_null_g": (WEIGHT, weight_args, dict(g=None)),
    "weight_null_dw": (WEIGHT, weight_args, dict(dw=None)),
    "weight_null_scratch": (WEIGHT, weight_args, dict(scratch=None)),
    "weight_k3": (WEIGHT, weight_args, dict(KH=3, KW=3, pad=1)),
    "weight_k7_pad2": (WEIGHT, weight_args, dict(KH=7, KW=7, pad=2)),
    "weight_k5_pad3": (WEIGHT, weight_args, dict(pad=3)),
    "weight_odd_h": (WEIGHT, weight_args, dict(H=13)),
    "weight_odd_w": (WEIGHT, weight_args, dict(W=15)),
    "weight_ci_48": (WEIGHT, weight_args, dict(Ci=48, x_cstride=48)),
    "weight_co_96": (WEIGHT, weight_args, dict(Co=96, g_cstride=96)),
    "weight_x_stride_short": (WEIGHT, weight_args, dict(x_cstride=128, x_coff=64)),
    "weight_g_stride_short": (WEIGHT, weight_args, dict(g_cstride=64)),
    "weight_negative_offset": (WEIGHT, weight_args, dict(x_coff=-4, x_cstride=256)),
    "weight_odd_offset": (WEIGHT, weight_args, dict(x_cstride=CI + 2, x_coff=2)),
    "weight_short_scratch": (WEIGHT, weight_args, dict(scratch_bytes=4 * (CO * CI * 25 + CO) - 4)),
    "plan_k3": (PLAN, plan_args, dict(kh=3, kw=3)),
    "plan_k5x7": (PLAN, plan_args, dict(kw=7)),
    "plan_odd_h": (PLAN, plan_args, dict(H=13)),
    "plan_odd_w": (PLAN, plan_args, dict(W=15)),
    "plan_ci_48": (PLAN, plan_args, dict(ci=48)),
    "plan_co_96": (PLAN, plan_args, dict(co=96)),
}


# ---- the split weight gradient: every refusal of the fp32 entry (REFUSALS above), asked of the split entry;
# the scratch one byte short of the split plan's
WGRAD_SPLIT_SCRATCH = 4 * (CO * CI * 25 + CO)        # (2, 14, 14, 96, 128, 5): one chunk
WGRAD_SPLIT_REFUSALS = dict((rule, over) for rule, (entry, _make, over) in REFUSALS.items() if entry == WEIGHT)
WGRAD_SPLIT_REFUSALS["weight_short_scratch"] = dict(scratch_bytes=WGRAD_SPLIT_SCRATCH - 1)
WGRAD_SPLIT_REFUSALS.update(weight_k5x7=dict(KH=5, KW=7), weight_g_negative_offset=dict(g_coff=-4, g_cstride=256), weight_n_img_0=dict(n_img=0),
                            weight_h_0=dict(H=0))

# ---- the split data gradient: every refusal of the fp32 data entry (REFUSALS above), asked of the split entry;
# the scratch one byte short of the split plan's
DGRAD_SPLIT_SCRATCH = 25 * CO * CI * 6 + N * (H // 2) ** 2 * CO * 6
DGRAD_SPLIT_REFUSALS = dict((rule, over) for rule, (entry, _make, over) in REFUSALS.items() if entry == "offk_conv2d_s2_backward_data")
DGRAD_SPLIT_REFUSALS["data_short_scratch"] = dict(scratch_bytes=DGRAD_SPLIT_SCRATCH - 1)
DGRAD_SPLIT_REFUSALS.update(data_n_img_0=dict(n_img=0), data_h_0=dict(H=0), data_g_negative_offset=dict(g_coff=-4, g_cstride=256))
