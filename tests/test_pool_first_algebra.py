"""The algebra behind the pool-first 7-head (OFFK_POOL_FIRST_7), without a GPU.

The reference ends the 7x7 stage with  motion_sum = conv3(t2) + branch(x2)  (no ReLU after the add),  AvgPool2d(7),  Linear
(RGB_OFF.py:839-847, Flow_OFF.py:857-865, RGB_OFF_v2.py:864-872).  motion_sum feeds nothing else, so with xv = [t2 | x2],
Wm = [W3 | Wb] and bm = b3 + bb

    logits_7 = Wfc mean49(Wm xv + bm) + bfc = (Wfc Wm) mean49(xv) + (Wfc bm + bfc).

Here both association orders are evaluated in fp64 on the inputs of one golden per reference file (rgb, flow, rgbv2): the left one
through the oracle's own fusion_7 and head (which the goldens pin to the reference), the right one from t2 and x2 recomputed with the
same convs.  They must agree to 1e-9 of max |logit|: a ReLU on motion_sum, or a use of it elsewhere, would break the identity for all
three variants at once."""
import os

import numpy as np
import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import synth
from oracle import off_oracle as orc

TAGS = ("rgb_b2_l3", "flow_b2_l3", "rgbv2_b2_l3")


@pytest.mark.parametrize("tag", TAGS)
def test_pool_first_equals_conv_first_in_fp64(tag, golden_dir):
    g = np.load(os.path.join(golden_dir, tag + ".npz"))
    variant, B, L, cfg = (int(v) for v in g["meta"])
    feats = [torch.from_numpy(f) for f in synth.make_features(B, L, cfg)]
    w = orc.to_torch_weights(synth.make_weights(variant))
    with torch.no_grad():
        _out, st = orc.off_forward(feats, w, B, L, variant, orc.SLICE_FLAT, consensus=False, return_stages=True)
        w64 = dict((k, v.double()) for k, v in w.items())
        f7 = st["fusion_7"].double()
        # conv first: the oracle's own stage and head
        left = orc.head(orc.fusion_7(f7, w64), w64, "fc_action_motion", False)
        # pool first
        x2 = torch.relu(orc._conv(f7, w64, "motion_conv_trans", pad=1))
        t2 = torch.relu(orc._conv(torch.relu(orc._conv(x2, w64, "motion_conv1_trans")), w64, "motion_conv2_trans", pad=1))
        xv = torch.cat((t2, x2), 1)
        Wm = torch.cat((w64["motion_conv3_trans.weight"][:, :, 0, 0], w64["motion_conv_branch_trans.weight"][:, :, 0, 0]), 1)
        bm = w64["motion_conv3_trans.bias"] + w64["motion_conv_branch_trans.bias"]
        Wfc, bfc = w64["fc_action_motion.weight"], w64["fc_action_motion.bias"]
        right = xv.mean((2, 3)) @ (Wfc @ Wm).t() + (Wfc @ bm + bfc)
    assert Wm.shape == (1024, 512) and left.shape == right.shape == (B * (L - 1), Wfc.shape[0])
    err = (left - right).abs().max().item() / left.abs().max().item()
    print("%s: pool-first vs conv-first, fp64: %.2e of max |logit|" % (tag, err))
    assert err <= 1e-9
