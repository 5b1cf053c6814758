"""Every strided stage entry with its views past the 2 GiB and the 4 GiB mark (tests/big.py has the slabs and the case list,
tests/test_big_cases.py the arithmetic that makes each case meaningful and safe).

A case runs the entry twice on the same integer inputs: A on compact tensors (cstride = C, coff = 0: what the entry's own tests hold
to fp64) and B with the operands named in the case inside a BigSlab whose last rows lie past the mark.  Asserted: A equals the fp64
reference where the entry has an exact test; B's outputs equal A's bit for bit and hold no NaN; every word outside every view still
holds the sentinel (the 2 GiB front margins included); the inputs are unchanged; where the table says "refused", the return code and
message are the documented ones and the output slabs are untouched.  With accumulate the output view is pre-filled with the integer
bases of the exact tests.  Equality with A is the strongest statement available on both sides of a kernel switch too: the inputs are
integers whose every partial sum is exact in fp32, so ANY correct kernel gives A's bits.

The address arithmetic behind each entry, read before its case first ran (csrc/...; "size_t" etc. is the width of the product
row-or-image index x stride; entries without a constant have no size check of their views at all):

  entry                          extent compared with a constant              below | at or above it                        index width
  -----------------------------  -------------------------------------------  ------------------------------------------  ---------------------------
  offk_conv2d / _ex (generic)    x: (n H W cs - coff) 4 + (pad W + pad) cs 4  buffer-descriptor loader (PREC 4 LDS-DMA,    pointer loader: size_t
                                 < 0x7fffffff, conv_igemm.hip:1012           PREC 2 with RELU_IN) | pointer loader        (conv_igemm.hip:284)
                                                                              conv_igemm_kernel<PREC 0>
                                 y: ((M - 1) cs + coff + Co) 4 < 0x7f000000,  buffer stores (no residual) | pointer        size_t (:551, res :532);
                                 conv_igemm.hip:492                          stores                                        split-K reduce size_t (:609)
                                 M = n Ho Wo <= 0x7fffffff - 256, :1025       runs | refused "conv2d: bad problem size"
  offk_conv2d_ex (tile_cfg 6/7)  none: the patch kernel has pointer loads      one kernel                                   size_t (:679, :857)
                                 and stores only
  offk_bottleneck_chain14        x: (n 196 cs - coff) 4 < 0x7fffffff,         chain14_kernel | refused "chain14: input     y, res: size_t
                                 offk_api.hip:932, chain_fused.hip:508        beyond 31-bit byte offsets"                  (chain_fused.hip:287, :327)
  offk_bottleneck_chain14_split  x as above; y: n 196 cs 4 < 0x7fffff00,      chain14_split_kernel | refused "chain14      res: size_t
                                 chain_split.hip:366-367                      (split-fp32): need ... input and output      (chain_split.hip:144)
                                                                              below 2^31 bytes"
  offk_winograd_conv3x3 / 5x5s2  none on x, y, res (V, M are dense scratch:   one input and one output transform           size_t (winograd.hip:44,
                                 wino_gemm.hip:212-215 picks their GEMM)                                                  :94, :137-142)
  offk_winograd_conv7x7s2        none on x, y                                 one input and one output transform           size_t (winograd7.hip:91,
                                                                                                                           :102, :170)
  offk_winograd_between / _ex    none on x                                    one kernel per arithmetic                    size_t (wino_mid.hip:103)
  offk_head                      none                                         head_kernel                                  size_t (heads.hip:50, :71, :77)
  offk_head_train                n H W, n classes <= 0x7fffffff,              runs | refused "problem too large"            size_t (head_bwd.hip:59,
  offk_head_backward             offk_api.hip:2627 (counts, not bytes)                                                     :73, :82, :139-181)
  offk_relu_backward             none                                         relu_bwd_kernel                              size_t (conv_bwd.hip:237-243)
  offk_conv2d_backward_data      (H + 2)(W + 2) n <= 0x7fffffff - 4096,       runs as offk_conv2d of the transposed        as offk_conv2d; accumulate
                                 conv_bwd.hip:254 (positions, not bytes)      problem | refused "problem too large"        reads dx as the residual
  offk_conv2d_backward_weight    as above                                     conv_wgrad_kernel                            long long (conv_bwd.hip:58,
                                                                                                                           :97, :112)
  offk_conv2d_backward_weight    positions + 2 pitch + 4096 < 0x7fffffff,     conv_wgrad_split kernel | refused            long long
    _split                       conv_wgrad_split.hip:256                                                                  (conv_wgrad_split.hip:116-141)
  offk_conv2d_s2_backward_data   positions, n H W <= 0x7fffffff,              one kernel | refused "problem too large"     size_t (conv_bwd_s2.hip:134,
  offk_conv2d_s2_backward_weight conv_bwd_s2.hip:375                                                                       :181, :272, :285)
  offk_conv2d_s2_backward_data   M + 16 tiles <= 0x7fffffff,                  one kernel pair | refused                    size_t (conv_dgrad_s2_split
    _split                       conv_dgrad_s2_split.hip:263                                                               .hip:122-124, :272)
  offk_nhwc_to_nchw              none (n <= 65535: the grid's z)              nhwc_to_nchw_kernel                          size_t (heads.hip:478, :483)
  offk_sobel_tdiff               none on M (m_cstride, m_coff)                one kernel per algo                          size_t (sobel_tdiff.hip:148-200,
                                                                                                                           :221-293)

No 32-bit product of a row index and a stride was found in any of them: every entry is either 64-bit clean for its views or refuses.
What a 2 GiB / 4 GiB case cannot show is an ELEMENT index that is an int (it wraps at 8 GiB of fp32); the column on the right is the
statement about those.

Device memory: a slab is [2 GiB margin | one row more than the mark]; the largest case is offk_relu_backward with all three views
past 4 GiB, 3 x (2.1 + 4.4) GB = 19.6 GB.  Allocating and freeing such buffers costs seconds, so the module keeps three buffers of the
largest slab's size (6.8 GB each, 20.5 GB) for all its cases (big.Pool), refills them with the sentinel per case and frees them in the
fixture's teardown.
"""
import collections

import pytest
import torch

import offk_amd  # noqa: F401
from offk_amd import _lib, spec
from oracle import off_oracle as orc

from . import arena, big, exact
from .conv_bwd import S1 as cb
from .conv_bwd import S2 as cs2
from . import exact_fusion as ef
from . import exact_wino as ew
from . import head_bwd as hb
from .exact_units import conv_inputs, conv_ref
from .featmaps import rt  # noqa: F401
from .forward import RTOL, make_handle, rel_err

pytestmark = pytest.mark.gpu
NAN = float("nan")

# what an entry function returns: shapes {operand: (n, H, W, C)}, inputs {operand: CPU tensor}, bases {output operand: CPU tensor} for
# accumulate (None: the entry has none), call(bufs, accumulate) -> {name: dense device output} with bufs {operand: (buffer [n, H, W, cs],
# coff)}, check_a(outs, accumulate) asserting run A against fp64, refusal(case) -> None or the regular expression of the error
Spec = collections.namedtuple("Spec", "shapes inputs bases call check_a refusal")


@pytest.fixture(scope="module")
def pool():
    p = big.Pool()
    yield p
    p.release()


def dev(t):
    return None if t is None else t.cuda()


def never(_case):
    return None


def exact_check(refs):
    """check_a for entries with an exact test: outs[name] == refs(accumulate)[name] everywhere"""
    def check(outs, accumulate):
        mm = exact.Mismatches()
        for name, ref in refs(accumulate).items():
            mm.check(outs[name].cpu(), ref, "run A, %s" % name)
        mm.raise_if_any()
    return check


# ---- the entries -------------------------------------------------------------------------------------------------------------------
CONV = {  # key: (Ci, Co, k, stride, pad, H, n, tile_cfg, splitk, flags)
    "tile3x3": (64, 64, 3, 1, 1, 14, 2, -1, 0, 0),
    "tile3x3_res": (64, 64, 3, 1, 1, 14, 2, -1, 0, _lib.CONV_RELU_PRE | _lib.CONV_RELU_POST),
    "flat1x1_relu_in": (64, 256, 1, 1, 0, 14, 2, -1, 0, _lib.CONV_RELU_IN | _lib.CONV_RELU_PRE),
    "splitk": (64, 64, 3, 1, 1, 14, 2, 3, 2, 0),
    "patch6": (128, 256, 3, 1, 1, 14, 2, 6, 1, _lib.CONV_RELU_IN | _lib.CONV_RELU_PRE),
    "patch7_splitk": (64, 64, 3, 1, 1, 14, 3, 7, 2, 0),
}


def _p(rt, t):
    return rt._ptr(t)


def conv2d(rt, key):
    """through the library's entry itself (the Python wrapper has no res_coff): offk_conv2d_ex with every view's own stride and offset"""
    Ci, Co, k, stride, pad, H, n, cfg, splitk, flags = CONV[key]
    with_res = key.endswith("_res")
    Ho = (H + 2 * pad - k) // stride + 1
    x, w, b, res = conv_inputs(Ci + Co + k + len(key), n, Ci, Co, k, H, Ho)
    ref = conv_ref(x, w, b, stride, pad, res if with_res else None, flags)
    wd, bd = w.cuda(), b.cuda()
    wp = rt.pack_conv_weight(wd)
    lib = _lib.load()

    def call(bufs, accumulate):
        (xb, xc), (yb, yc) = bufs["x"], bufs["y"]
        rb, rc = bufs["res"] if with_res else (None, 0)
        nfl = splitk * n * Ho * Ho * Co if splitk > 1 else 0
        part = torch.empty(nfl, device="cuda") if nfl else None
        _lib.check(lib.offk_conv2d_ex(rt._stream(xb.device), _p(rt, xb), xb.shape[-1], xc, n, H, H, Ci, _p(rt, wp), _p(rt, bd), Co, k, k, stride, pad,
                                      _p(rt, rb), rb.shape[-1] if with_res else 0, rc, flags, _p(rt, yb), yb.shape[-1], yc, cfg, splitk,
                                      _p(rt, part), nfl, 0))
        return {}
    shapes = {"x": (n, H, H, Ci), "y": (n, Ho, Ho, Co)}
    inputs = {"x": x.permute(0, 2, 3, 1).contiguous()}
    if with_res:
        shapes["res"], inputs["res"] = (n, Ho, Ho, Co), res.permute(0, 2, 3, 1).contiguous()
    return Spec(shapes, inputs, None, call, exact_check(lambda acc: {"y": ref}), never)


def relu_backward(rt, key):
    shape = (2, 7, 7, 128)
    dy, y = exact.ints(0xB16, shape, -8, 8), exact.ints(0xB17, shape, -2, 2)
    base = exact.ints(0xB18, shape, -64, 64)
    want = torch.where(y > 0, dy, torch.zeros_like(dy)).double()

    def call(bufs, accumulate):
        (db, dc), (yb, yc), (gb, gc) = bufs["dy"], bufs["y"], bufs["g"]
        rt.relu_backward(db, yb, out=gb, accumulate=accumulate, dy_coff=dc, y_coff=yc, out_coff=gc, c=128)
        return {}
    return Spec({"dy": shape, "y": shape, "g": shape}, {"dy": dy, "y": y}, {"g": base}, call,
                exact_check(lambda acc: {"g": want + (base.double() if acc else 0.0)}), never)


BWD = {"k1": cb.Case(1, 2, 7, 7, 512, 128), "k3": cb.Case(3, 2, 5, 3, 128, 128)}
BWD_S2 = {"k7": cb.Case(7, 2, 6, 10, 64, 64), "k5": cb.Case(5, 2, 6, 4, 160, 64)}


def _bwd_data(rt, c, mod, fn, pad, **kw):
    inp, ref = mod.cached(c, "int", False)
    mod.check_caps(c, inp, ref)
    w = inp["w"].cuda()

    def call(bufs, accumulate):
        (gb, gc), (xb, xc) = bufs["g"], bufs["dx"]
        fn(gb, w, pad, dx=xb, dx_coff=xc, accumulate=accumulate, g_coff=gc, **kw)
        return {}
    return Spec({"g": tuple(inp["g"].shape), "dx": tuple(inp["dx0"].shape)}, {"g": inp["g"]}, {"dx": inp["dx0"]}, call,
                exact_check(lambda acc: {"dx": ref["dX"] + (inp["dx0"].double() if acc else 0.0)}), never)


def _bwd_weight(rt, c, mod, fn, pad, **kw):
    inp, ref = mod.cached(c, "int", False)
    mod.check_caps(c, inp, ref)

    def call(bufs, accumulate):
        (xb, xc), (gb, gc) = bufs["x"], bufs["g"]
        dw = torch.full((c.co, c.ci, c.k, c.k), NAN, device="cuda")
        db = torch.full((c.co,), NAN, device="cuda")
        fn(xb, gb, c.k, pad, x_coff=xc, ci=c.ci, g_coff=gc, co=c.co, dw=dw, db=db, **kw)
        return {"dw": dw, "db": db}
    return Spec({"x": tuple(inp["x"].shape), "g": tuple(inp["g"].shape)}, {"x": inp["x"], "g": inp["g"]}, None, call,
                exact_check(lambda acc: {"dw": ref["dW"], "db": ref["db"]}), never)


def conv2d_backward_data(rt, key):
    return _bwd_data(rt, BWD[key], cb, rt.conv2d_backward_data, (BWD[key].k - 1) // 2)


def conv2d_backward_weight(rt, key):
    return _bwd_weight(rt, BWD[key], cb, rt.conv2d_backward_weight, (BWD[key].k - 1) // 2)


def conv2d_backward_weight_split(rt, key):
    return _bwd_weight(rt, BWD[key], cb, rt.conv2d_backward_weight, (BWD[key].k - 1) // 2, arith="f32split")


def conv2d_s2_backward_data(rt, key):
    return _bwd_data(rt, BWD_S2[key], cs2, rt.conv2d_s2_backward_data, cs2.FORMS[BWD_S2[key].k])


def conv2d_s2_backward_data_split(rt, key):
    return _bwd_data(rt, BWD_S2[key], cs2, rt.conv2d_s2_backward_data, cs2.FORMS[BWD_S2[key].k], arith="f32split")


def conv2d_s2_backward_weight(rt, key):
    return _bwd_weight(rt, BWD_S2[key], cs2, rt.conv2d_s2_backward_weight, cs2.FORMS[BWD_S2[key].k])


HEAD = {"avg4x4": hb.EXACT_CASES[1], "max5x5": hb.EXACT_CASES[5]}


def head(rt, key):
    c = HEAD[key]
    d, ref = hb.exact_inputs(c)
    w, b = d["w"].cuda(), d["b"].cuda()
    want = ref["pooled"] @ d["w"].double().t() + d["b"].double()          # the eval head: no mask, no scale

    def call(bufs, accumulate):
        xb, xc = bufs["x"]
        return {"out": rt.head(xb, w, b, c.maxpool, x_coff=xc, c=c.C, out=torch.full((c.n, c.cls), NAN, device="cuda"))}

    def check_a(outs, accumulate):          # (offk_head has no exact test: the bound of test_head_and_consensus)
        assert rel_err(outs["out"], want) < RTOL
    return Spec({"x": (c.n, c.H, c.W, c.C)}, {"x": d["x"]}, None, call, check_a, never)


def head_train(rt, key):
    c = HEAD[key]
    d, ref = hb.exact_inputs(c)
    hb.check_exactness_condition(c, d, ref)
    w, b = d["w"].cuda(), d["b"].cuda()

    def call(bufs, accumulate):
        xb, xc = bufs["x"]
        out, z = rt.head_train(xb, w, b, c.maxpool, c.head, (c.seed, c.p), x_coff=xc, c=c.C, z=torch.full((c.n, c.C), NAN, device="cuda"),
                               out=torch.full((c.n, c.cls), NAN, device="cuda"))
        return {"out": out, "z": z}
    return Spec({"x": (c.n, c.H, c.W, c.C)}, {"x": d["x"]}, None, call, exact_check(lambda acc: {"out": ref["out"], "z": ref["z"]}), never)


def head_backward(rt, key):
    c = HEAD[key]
    d, ref = hb.exact_inputs(c)
    hb.check_exactness_condition(c, d, ref)
    w, g, z = d["w"].cuda(), d["g"].cuda(), ref["z"].float().cuda()       # (z is exact: the fp64 value is an fp32 number)
    shape = (c.n, c.H, c.W, c.C)

    def call(bufs, accumulate):
        (xb, xc), (dxb, dxc) = bufs["x"], bufs["dx"]
        _dx, dw, db = rt.head_backward(g, xb, w, z, c.maxpool, c.head, (c.seed, c.p), x_coff=xc, c=c.C, dx=dxb, dx_coff=dxc,
                                       accumulate_dx=accumulate, dw=torch.full((c.cls, c.C), NAN, device="cuda"),
                                       db=torch.full((c.cls,), NAN, device="cuda"))
        return {"dw": dw, "db": db}
    return Spec({"x": shape, "dx": shape}, {"x": d["x"]}, {"dx": d["dx0"]}, call,
                exact_check(lambda acc: {"dx": ref["dX"] + (d["dx0"].double() if acc else 0.0), "dw": ref["dW"], "db": ref["db"]}), never)


def nhwc_to_nchw(rt, key):
    shape = (3, 7, 5, 20)
    src = exact.ints(0xB19, shape, -8, 8)

    def call(bufs, accumulate):
        b, coff = bufs["src"]
        return {"dst": rt.nhwc_to_nchw(b, coff=coff, c=20, out=torch.full((3, 20, 7, 5), NAN, device="cuda"))}
    return Spec({"src": shape}, {"src": src}, None, call, exact_check(lambda acc: {"dst": src.permute(0, 3, 1, 2).contiguous().double()}), never)


def _winograd(rt, k, n, with_res=False):
    c = ew.ConvInputs(k, 32, 64, n)
    H = {3: 7, 5: 14, 7: 28}[k]
    Ho = 14 if k == 7 else 7
    fn = {3: rt.winograd_conv3x3, 5: rt.winograd_conv5x5s2, 7: rt.winograd_conv7x7s2}[k]
    w, b = c.w.cuda(), c.bias.cuda()
    wp = rt.pack_conv_weight(w)
    flags = ew.RELU_PRE | ew.RELU_POST if with_res else ew.RELU_PRE              # with_res: the 14b form, relu(relu(conv + bias) + res)
    ref, _pre, cap = ew.direct_reference(c.x, c.w, c.bias, k, flags, c.res if with_res else None)
    assert cap < exact.LIMIT
    lib = _lib.load()

    def call(bufs, accumulate):
        (xb, xc), (yb, yc) = bufs["x"], bufs["y"]
        if not with_res:
            fn(xb, w, b, flags=flags, x_coff=xc, y=yb, y_coff=yc, w_packed=wp)
            return {}
        rb, rc = bufs["res"]                 # (the entry itself: the Python wrapper has no res_coff)
        nfl = 121 * (64 * 32 + n * (32 + 64))
        scratch = torch.empty(nfl, device="cuda")
        _lib.check(lib.offk_winograd_conv3x3(rt._stream(xb.device), _p(rt, xb), xb.shape[-1], xc, n, 32, _p(rt, wp), _p(rt, b), 64, _p(rt, rb),
                                             rb.shape[-1], rc, flags, _p(rt, yb), yb.shape[-1], yc, _p(rt, scratch), nfl, None))
        return {}

    def check_a(outs, accumulate):
        if k == 7:      # (A^T of F(5x5, 4x4) holds 1/16 .. 16: not exact, tests/test_gpu_exact_wino.py has its derived bound; here the RTOL of the parity tests)
            assert rel_err(outs["y"], ref) < RTOL
        else:
            exact.assert_exact(outs["y"].cpu(), ref, "run A, y")
    shapes, inputs = {"x": (n, H, H, 32), "y": (n, Ho, Ho, 64)}, {"x": c.x}
    if with_res:
        shapes["res"], inputs["res"] = (n, 7, 7, 64), c.res
    return Spec(shapes, inputs, None, call, check_a, never)


def winograd_conv3x3(rt, key):
    return _winograd(rt, 3, 5, with_res=key.endswith("_res"))


def winograd_conv5x5s2(rt, key):
    return _winograd(rt, 5, 5)


def winograd_conv7x7s2(rt, key):
    return _winograd(rt, 7, 3)


CHAIN_REFUSAL = r"error -1: chain14: input beyond 31-bit byte offsets"
CHAIN_SPLIT_REFUSAL = r"error -1: offk_bottleneck_chain14_split: chain14 \(split-fp32\): need .* input and output below 2\^31 bytes"


def _chain(rt, split, kind):
    c = ef.ChainInputs(5, kind)
    out, cap = c.reference("direct")
    ef.check_caps(cap, kind + "-n5")
    with_res = c.res is not None
    w1, b1, w2, b2, w3, b3 = [dev(v) for v in (c.w1, c.b1, c.w2, c.b2, c.w3, c.b3)]
    w2p = rt.pack_conv_weight(w2)
    lib = _lib.load()
    scratch = torch.empty(6 * (64 * c.Cin + 64 * 576 + 2 * 256 * 64), dtype=torch.uint8, device="cuda")

    def call(bufs, accumulate):          # (the entries themselves: the Python wrappers have no res_coff)
        (xb, xc), (yb, yc) = bufs["x"], bufs["y"]
        rb, rc = bufs["res"] if with_res else (None, 0)
        head = (rt._stream(xb.device), _p(rt, xb), xb.shape[-1], xc, 5, c.Cin, int(c.relu_in), _p(rt, w1), _p(rt, b1), _p(rt, w2p), _p(rt, b2), _p(rt, w3),
                _p(rt, b3))
        tail = (_p(rt, rb), rb.shape[-1] if with_res else 0, rc, _p(rt, yb), yb.shape[-1], yc)
        if split:
            _lib.check(lib.offk_bottleneck_chain14_split(*(head + (None, None) + tail + (_p(rt, scratch), scratch.numel()))))
        else:
            _lib.check(lib.offk_bottleneck_chain14(*(head + (64,) + tail)))
        return {}

    def refusal(case):
        if split:                        # x and y are addressed through buffer descriptors; res through pointers: any extent
            return CHAIN_SPLIT_REFUSAL if ("x" in case.past or "y" in case.past) else None
        return CHAIN_REFUSAL if "x" in case.past else None
    shapes, inputs = {"x": (5, 14, 14, c.Cin), "y": (5, 14, 14, 256)}, {"x": c.x}
    if with_res:
        shapes["res"], inputs["res"] = (5, 14, 14, 256), c.res
    return Spec(shapes, inputs, None, call, exact_check(lambda acc: {"y": out["y"]}), refusal)


def bottleneck_chain14(rt, key):
    return _chain(rt, False, key)


def bottleneck_chain14_split(rt, key):
    return _chain(rt, True, key)


def winograd_between(rt, key):
    b = ef.BetweenInputs(5, 128, 1, True)
    out, cap = b.reference()
    ef.check_caps(cap, "between-128-1-n5")
    M, bias, w1, b1 = dev(b.M), dev(b.bias), dev(b.w1), dev(b.b1)

    def call(bufs, accumulate):
        xb, xc = bufs["x"]
        V = torch.full((121, 5, 128), NAN, device="cuda")
        rt.winograd_between(M, bias, 1, w1, b1, x=xb, x_coff=xc, precision=key, V=V)
        return {"V": V}
    return Spec({"x": (5, 7, 7, 128)}, {}, None, call, exact_check(lambda acc: {"V": out["V"], "x": out["x"]}), never)


def sobel_tdiff(rt, key):
    B, L, site = 2, 4, 7
    name, _C, H = spec.SITES[site]
    h, w = make_handle(rt, B, L, spec.VARIANT_RGB)
    G = torch.relu(exact.ints(0xB1A, (B * L, H, H, 128), -4, 4))
    D = exact.ints(0xB1B, (B * (L - 1), H, H, 32), -4, 4)
    Gd, Dd = G.cuda().view(-1, 128), D.cuda().view(-1, 32)
    Gn, Dn = G.permute(0, 3, 1, 2).double(), D.permute(0, 3, 1, 2).double()
    s_ref = torch.nn.functional.conv2d(Dn, w["motion_spatial_grad_%s.weight" % name].double(), w["motion_spatial_grad_%s.bias" % name].double(),
                                       padding=1, groups=32)
    t_ref = orc.temporal_diff(Gn, B)
    algo = int(key[4:])

    def call(bufs, accumulate):
        Mb, mc = bufs["M"]
        h.sobel_tdiff(site, Gd, Dd, Mb, mc, algo)
        return {}

    def check_a(outs, accumulate):          # (the bounds of test_sobel_tdiff_vs_oracle; the difference of integers is exact)
        got = outs["M"].permute(0, 3, 1, 2)
        assert rel_err(got[:, :32], s_ref) < RTOL
        exact.assert_exact(got[:, 32:].cpu(), t_ref, "run A, temporal half")
    return Spec({"M": (B * (L - 1), H, H, 160)}, {}, None, call, check_a, never)


ENTRY = {f.__name__: f for f in (sobel_tdiff, conv2d, relu_backward, conv2d_backward_data, conv2d_backward_weight, conv2d_backward_weight_split,
                                 conv2d_s2_backward_data, conv2d_s2_backward_data_split, conv2d_s2_backward_weight, head, head_train,
                                 head_backward, nhwc_to_nchw, winograd_conv3x3, winograd_conv5x5s2, winograd_conv7x7s2, bottleneck_chain14,
                                 bottleneck_chain14_split, winograd_between)}
HAS_ACCUMULATE = ("relu_backward", "conv2d_backward_data", "conv2d_s2_backward_data", "conv2d_s2_backward_data_split", "head_backward")


def params():
    """every case; with accumulate once more where an OUTPUT view lies past the mark"""
    out = []
    for c in big.cases():
        out.append(pytest.param(c, False, id=big.case_id(c)))
        if c.entry in HAS_ACCUMULATE and any(op.role == "out" and op.name in c.past for op in c.operands):
            out.append(pytest.param(c, True, id=big.case_id(c) + "-accumulate"))
    return out


def test_every_entry_of_the_case_list_has_its_runner():
    assert set(big.ENTRIES) == set(ENTRY)
    for entry, keys in big.ENTRIES.items():
        assert entry not in ("conv2d",) or set(keys) == set(CONV)


_SPECS = {}


def spec_of(rt, c):
    if (c.entry, c.key) not in _SPECS:
        _SPECS[(c.entry, c.key)] = ENTRY[c.entry](rt, c.key)
    return _SPECS[(c.entry, c.key)]


@pytest.mark.parametrize("c,accumulate", params())
def test_views_past_the_mark(rt, pool, c, accumulate):
    e = spec_of(rt, c)
    for op in c.operands:
        n, H, W, C = e.shapes[op.name]
        assert (n * H * W, C) == (op.rows, op.channels) and n >= 2, "tests/big.py and this file disagree on %s" % op.name

    # ---- A: compact tensors ----
    bufs = {}
    for op in c.operands:
        if op.role == "in":
            t = e.inputs[op.name].cuda().contiguous()
        else:
            t = e.bases[op.name].cuda().contiguous() if accumulate else torch.full(e.shapes[op.name], NAN, device="cuda")
        bufs[op.name] = (t, 0)
    outs_a = e.call(bufs, accumulate)
    torch.cuda.synchronize()
    outs_a.update({op.name: bufs[op.name][0] for op in c.operands if op.role == "out"})
    e.check_a(outs_a, accumulate)

    # ---- B: the same values, the case's operands past the mark ----
    slabs = big.make_slabs(c, pool=pool)          # (the pool asserts that its buffers fit the free memory, with 10 % to spare)
    try:
        for op in c.operands:
            if op.role == "in":
                slabs[op.name].fill(e.inputs[op.name])
            elif accumulate:
                slabs[op.name].fill(e.bases[op.name])
            if op.name in c.past:
                assert slabs[op.name].last_row_offset > c.mark and slabs[op.name].front_margin == big.FRONT_MARGIN
        bufs = {op.name: (slabs[op.name].images(*e.shapes[op.name][:3]), slabs[op.name].coff) for op in c.operands}
        refusal = e.refusal(c)
        if refusal is not None:
            with pytest.raises(_lib.OffkError, match=refusal):
                e.call(bufs, accumulate)
            torch.cuda.synchronize()
            for op in c.operands:
                if op.role == "out":
                    assert slabs[op.name].untouched(), "a refused call wrote into %s" % op.name
        else:
            outs_b = e.call(bufs, accumulate)
            torch.cuda.synchronize()
            outs_b.update({op.name: slabs[op.name].view.reshape(e.shapes[op.name]).contiguous() for op in c.operands if op.role == "out"})
            assert set(outs_b) == set(outs_a)
            for name, got in outs_b.items():
                assert not bool(got.isnan().any()), "%s holds a NaN: a read outside the view" % name
                assert arena.same_bits(got, outs_a[name]), "%s differs from the compact run at %d elements" % (
                    name, int((arena.bits(got) != arena.bits(outs_a[name])).sum()))
        for op in c.operands:
            changed = slabs[op.name].changed_outside()
            assert changed == 0, "%d words outside the view of %s changed" % (changed, op.name)
            if op.role == "in":
                assert torch.equal(slabs[op.name].view.cpu(), e.inputs[op.name].reshape(op.rows, op.channels)), "input %s was written" % op.name
    finally:
        del slabs, bufs               # the big buffers stay with the pool until the module is done
