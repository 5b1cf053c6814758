"""Slabs whose last rows lie past the 2 GiB / 4 GiB marks, and the list of cases that use them (tests/test_big_cases.py on the CPU,
tests/test_gpu_big_slabs.py on the device).  Like tests/arena.py it has no tests of its own.

A strided stage entry takes a channels-last view: `rows` rows of `channels` values, `cstride` values apart, the first one `coff` values
behind the pointer.  With a channel stride of megabytes a view of a few hundred rows spans gigabytes, so the byte offset of its last
rows needs more than 31 (32) bits although the arithmetic on it is a few microseconds: the shapes stay the small ones of the existing
tests and only the addresses grow.

BigSlab is ONE allocation [front margin | slab], every 32-bit word of it arena.SENTINEL (a NaN as fp32, bf16 and fp16).  The margin is
what makes a wrapped offset harmless and visible:

* an in-range byte offset that a kernel wraps as int32 becomes negative by at most 2^31, i.e. it lands in the 2 GiB front margin;
* an in-range byte offset that a kernel wraps as uint32 (offset mod 2^32) lands inside the slab itself when the slab is >= 4 GiB;
* either way the access stays inside memory the test owns.  A wrapped store changes a sentinel word outside the view
  (untouched_outside), a wrapped load brings a NaN -- or another row's values -- into the result.

Which wrap a mark can show is arithmetic (tests/test_big_cases.py checks it for every case): past 2^31 the int32 reading of the last
row's offset differs from the offset, the reading mod 2^32 does not (the offset is still below 2^32); past 2^32 both differ.  An index
counted in ELEMENTS that is 32 bits wide wraps at 2^31 elements = 8 GiB of fp32, beyond both marks: those are found by reading the code
(the table in tests/test_gpu_big_slabs.py), not by these cases.
"""
import collections

import torch

from . import arena

MARKS = (2 ** 31, 2 ** 32)
FRONT_MARGIN = 2 ** 31
SMALL_MARGIN = 1 << 20            # of an operand that stays below the mark in a case (a plain guarded buffer)
COFF = 32                         # channel offset of every view (non-zero, a multiple of 4 floats and of 32: the convs' 16-byte rule)


def cstride_past(rows, mark_bytes, align=4, elem_bytes=4):
    """The smallest channel stride (in elements), a multiple of `align`, that puts the first byte of row rows - 1 past mark_bytes."""
    if rows < 2:
        raise ValueError("a view of one row has no row past any mark")
    cs = mark_bytes // ((rows - 1) * elem_bytes) + 1
    return (cs + align - 1) // align * align


class BigSlab:
    """[front margin | rows x cstride elements], all sentinel; .view is the [rows, channels] slice at coff."""

    def __init__(self, rows, channels, cstride, coff, dtype=torch.float32, front_margin=FRONT_MARGIN, device="cuda", storage=None):
        esz = torch.empty((), dtype=dtype).element_size()
        if rows < 1 or channels < 1 or coff < 0 or coff + channels > cstride:
            raise ValueError("BigSlab: need rows, channels >= 1 and 0 <= coff, coff + channels <= cstride")
        if (cstride * esz) % 4 or (coff * esz) % 4 or (channels * esz) % 4 or front_margin % 4 or front_margin < 0:
            raise ValueError("BigSlab: row pitch, view offset, view width and margin must be whole 32-bit words")
        self.rows, self.channels, self.cstride, self.coff, self.dtype, self.esz = rows, channels, cstride, coff, dtype, esz
        self.front_margin = front_margin
        self.slab_bytes = rows * cstride * esz
        nwords = (front_margin + self.slab_bytes) // 4
        if storage is None:
            self.words = torch.full((nwords,), arena.SENTINEL, dtype=torch.int32, device=device)
        else:                     # the first words of an allocation somebody keeps (Pool): what lies behind them is not this slab's business
            self.words = storage[:nwords]
            assert self.words.numel() == nwords and storage.dtype == torch.int32 and storage.is_contiguous()
            self.words.fill_(arena.SENTINEL)
        self.slab = self.words[front_margin // 4:].view(dtype).view(rows, cstride)       # what the entry gets as its pointer
        self.view = self.slab[:, coff:coff + channels]

    @property
    def last_row_offset(self):
        """byte offset, from the slab's first byte, of the first value of the view's last row"""
        return ((self.rows - 1) * self.cstride + self.coff) * self.esz

    def images(self, n, H, W):
        """the slab as [n, H, W, cstride], as the runtime wrappers take a channels-last buffer (n * H * W = rows)"""
        return self.slab.view(n, H, W, self.cstride)

    def fill(self, t):
        self.view.copy_(t.reshape(self.rows, self.channels).to(self.view.device))
        return self

    def changed_outside(self):
        """Number of 32-bit words outside the view that no longer hold the sentinel: the margin, the columns in front of and behind the
        view in every row.  Compared as int32 on the slab's device (NaN != NaN through a float view)."""
        wpr = self.cstride * self.esz // 4
        lo, hi = self.coff * self.esz // 4, (self.coff + self.channels) * self.esz // 4
        m = self.front_margin // 4
        body = self.words[m:].view(self.rows, wpr)
        n = 0
        for part in (self.words[:m], body[:, :lo], body[:, hi:]):
            if part.numel():
                n += int((part != arena.SENTINEL).sum())
        return n

    def untouched_outside(self):
        return self.changed_outside() == 0

    def untouched(self):
        """every word of the allocation, the view included, still holds the sentinel"""
        return not bool((self.words != arena.SENTINEL).any())


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# An operand: name, rows, channels of its view, role ("in" / "out").  A case puts the operands named in `past` behind the mark
# (cstride_past, FRONT_MARGIN) and every other strided operand of the entry in a small guarded slab (cstride = channels + 64).
Operand = collections.namedtuple("Operand", "name rows channels role")
Case = collections.namedtuple("Case", "entry key mark past operands")


def _conv(n, H, Ho, Ci, Co):
    return (Operand("x", n * H * H, Ci, "in"), Operand("y", n * Ho * Ho, Co, "out"))


# entry -> {key: operands}.  The shapes are the smallest of the existing small-shape tests with two images or more (the last image is
# the one past the mark): tests/test_gpu_parity.py CONV_CASES / PATCH_CASES, tests/conv_bwd.py SHAPES, tests/head_bwd.py EXACT_CASES,
# test_layout_helpers.  The keys name the kernel family and are what tests/test_gpu_big_slabs.py looks the shape up by.
ENTRIES = collections.OrderedDict([
    # offk_conv2d_ex, one key per kernel family of conv_igemm.hip: the generic tile (3x3, automatic plan), the flat 1x1 form with
    # ReLU on load (PREC 2 below the mark), split-K (partial slabs + splitk_reduce_kernel), the two patch kernels (tile_cfg 6 / 7)
    ("conv2d", collections.OrderedDict([
        ("tile3x3", _conv(2, 14, 14, 64, 64)),
        ("tile3x3_res", _conv(2, 14, 14, 64, 64) + (Operand("res", 2 * 14 * 14, 64, "in"),)),       # the residual epilogue (pointer loads)
        ("flat1x1_relu_in", _conv(2, 14, 14, 64, 256)),
        ("splitk", _conv(2, 14, 14, 64, 64)),
        ("patch6", _conv(2, 14, 14, 128, 256)),
        ("patch7_splitk", _conv(3, 14, 14, 64, 64)),
    ])),
    ("relu_backward", collections.OrderedDict([
        ("c128", (Operand("dy", 2 * 7 * 7, 128, "in"), Operand("y", 2 * 7 * 7, 128, "in"), Operand("g", 2 * 7 * 7, 128, "out"))),
    ])),
    ("conv2d_backward_data", collections.OrderedDict([
        ("k1", (Operand("g", 2 * 7 * 7, 128, "in"), Operand("dx", 2 * 7 * 7, 512, "out"))),
        ("k3", (Operand("g", 2 * 5 * 3, 128, "in"), Operand("dx", 2 * 5 * 3, 128, "out"))),
    ])),
    ("conv2d_backward_weight", collections.OrderedDict([
        ("k1", (Operand("x", 2 * 7 * 7, 512, "in"), Operand("g", 2 * 7 * 7, 128, "in"))),
        ("k3", (Operand("x", 2 * 5 * 3, 128, "in"), Operand("g", 2 * 5 * 3, 128, "in"))),
    ])),
    ("head", collections.OrderedDict([
        ("avg4x4", (Operand("x", 3 * 4 * 4, 256, "in"),)),
        ("max5x5", (Operand("x", 3 * 5 * 5, 64, "in"),)),
    ])),
    ("head_train", collections.OrderedDict([
        ("avg4x4", (Operand("x", 3 * 4 * 4, 256, "in"),)),
        ("max5x5", (Operand("x", 3 * 5 * 5, 64, "in"),)),
    ])),
    ("head_backward", collections.OrderedDict([
        ("avg4x4", (Operand("x", 3 * 4 * 4, 256, "in"), Operand("dx", 3 * 4 * 4, 256, "out"))),
        ("max5x5", (Operand("x", 3 * 5 * 5, 64, "in"), Operand("dx", 3 * 5 * 5, 64, "out"))),
    ])),
    ("nhwc_to_nchw", collections.OrderedDict([
        ("c20", (Operand("src", 3 * 7 * 5, 20, "in"),)),
    ])),
    ("conv2d_backward_weight_split", collections.OrderedDict([
        ("k1", (Operand("x", 2 * 7 * 7, 512, "in"), Operand("g", 2 * 7 * 7, 128, "in"))),
        ("k3", (Operand("x", 2 * 5 * 3, 128, "in"), Operand("g", 2 * 5 * 3, 128, "in"))),
    ])),
    # tests/conv_bwd.py (S2) SHAPES: (2, 6, 10, 64, 64) for the 7x7 and (2, 6, 4, 160, 64) for the 5x5; g is the half-size map
    ("conv2d_s2_backward_data", collections.OrderedDict([
        ("k7", (Operand("g", 2 * 3 * 5, 64, "in"), Operand("dx", 2 * 6 * 10, 64, "out"))),
        ("k5", (Operand("g", 2 * 3 * 2, 64, "in"), Operand("dx", 2 * 6 * 4, 160, "out"))),
    ])),
    ("conv2d_s2_backward_data_split", collections.OrderedDict([
        ("k7", (Operand("g", 2 * 3 * 5, 64, "in"), Operand("dx", 2 * 6 * 10, 64, "out"))),
        ("k5", (Operand("g", 2 * 3 * 2, 64, "in"), Operand("dx", 2 * 6 * 4, 160, "out"))),
    ])),
    ("conv2d_s2_backward_weight", collections.OrderedDict([
        ("k7", (Operand("x", 2 * 6 * 10, 64, "in"), Operand("g", 2 * 3 * 5, 64, "in"))),
        ("k5", (Operand("x", 2 * 6 * 4, 160, "in"), Operand("g", 2 * 3 * 2, 64, "in"))),
    ])),
    # tests/exact_wino.py conv_cases: (32, 64) at n = 5 (3x3 on 7x7, 5x5 / 2 on 14x14) and n = 3 (7x7 / 2 on 28x28)
    ("winograd_conv3x3", collections.OrderedDict([
        ("32to64", (Operand("x", 5 * 49, 32, "in"), Operand("y", 5 * 49, 64, "out"))),
        ("32to64_res", (Operand("x", 5 * 49, 32, "in"), Operand("y", 5 * 49, 64, "out"), Operand("res", 5 * 49, 64, "in"))),   # the 14b form
    ])),
    ("winograd_conv5x5s2", collections.OrderedDict([("32to64", (Operand("x", 5 * 196, 32, "in"), Operand("y", 5 * 49, 64, "out")))])),
    ("winograd_conv7x7s2", collections.OrderedDict([("32to64", (Operand("x", 3 * 784, 32, "in"), Operand("y", 3 * 196, 64, "out")))])),
    # tests/exact_fusion.py: the 'plain' chain (Cin = 64, ReLU on the way in) at n = 5; between: Cin = 128 after a 3x3, with its 1x1, n = 5
    # ... and 'res_other' (Cin = 256, the residual in a buffer of its own)
    ("bottleneck_chain14", collections.OrderedDict([
        ("plain", (Operand("x", 5 * 196, 64, "in"), Operand("y", 5 * 196, 256, "out"))),
        ("res_other", (Operand("x", 5 * 196, 256, "in"), Operand("y", 5 * 196, 256, "out"), Operand("res", 5 * 196, 256, "in"))),
    ])),
    ("bottleneck_chain14_split", collections.OrderedDict([
        ("plain", (Operand("x", 5 * 196, 64, "in"), Operand("y", 5 * 196, 256, "out"))),
        ("res_other", (Operand("x", 5 * 196, 256, "in"), Operand("y", 5 * 196, 256, "out"), Operand("res", 5 * 196, 256, "in"))),
    ])),
    # test_sobel_tdiff_vs_oracle's shape at the smallest map: site 5a (7x7), B = 2, L = 4: six pairs; M is the fusion buffer's view
    ("sobel_tdiff", collections.OrderedDict([(k, (Operand("M", 6 * 49, 160, "out"),)) for k in ("algo0", "algo1", "algo4")])),
    ("winograd_between", collections.OrderedDict([
        ("fp32", (Operand("x", 5 * 49, 128, "out"),)),
        ("f32split", (Operand("x", 5 * 49, 128, "out"),)),
    ])),
])


def cases(entry=None):
    """Every case: per entry, key and mark, each operand alone past the mark and (two operands or more) all of them at once."""
    out = []
    for e, keys in ENTRIES.items():
        if entry is not None and e != entry:
            continue
        for key, ops in keys.items():
            for mark in MARKS:
                subsets = [(o.name,) for o in ops]
                if len(ops) > 1:
                    subsets.append(tuple(o.name for o in ops))
                for past in subsets:
                    out.append(Case(e, key, mark, past, ops))
    return out


def case_id(c):
    return "%s-%s-%dGiB-%s" % (c.entry, c.key, c.mark >> 30, "all" if len(c.past) > 1 else c.past[0])


def geometry(c, op):
    """(cstride, coff, front_margin) of operand `op` in case `c`"""
    if op.name in c.past:
        return cstride_past(op.rows, c.mark), COFF, FRONT_MARGIN
    return op.channels + 2 * COFF, COFF, SMALL_MARGIN


def slab_bytes(c, op):
    cs, _coff, margin = geometry(c, op)
    return margin + op.rows * cs * 4


class Pool:
    """The big allocations of the device test, made once and reused by every case: allocating and freeing 4 - 7 GB per slab costs
    seconds per case, refilling it with the sentinel milliseconds.  Buffer i serves the i-th operand past the mark of a case; each has
    the size of the largest slab of the case list.  release() frees them (the module fixture's teardown)."""

    def __init__(self, device="cuda"):
        self.device, self.bufs = device, []
        self.nwords = max(slab_bytes(c, op) for c in cases() for op in c.operands if op.name in c.past) // 4

    def storage(self, i):
        while len(self.bufs) <= i:
            if self.device != "cpu":
                free = torch.cuda.mem_get_info()[0]
                assert self.nwords * 4 * 1.1 < free, "a slab buffer of %.1f GB does not fit the %.1f GB that are free" % (self.nwords * 4 / 1e9, free / 1e9)
            self.bufs.append(torch.empty((self.nwords,), dtype=torch.int32, device=self.device))
        return self.bufs[i]

    def release(self):
        self.bufs.clear()
        if self.device != "cpu":
            torch.cuda.empty_cache()


def make_slabs(c, device="cuda", pool=None):
    """{operand name: BigSlab} of a case, all sentinel; with a pool the operands past the mark live in its buffers"""
    out, k = {}, 0
    for op in c.operands:
        cs, coff, margin = geometry(c, op)
        storage = None
        if pool is not None and op.name in c.past:
            storage, k = pool.storage(k), k + 1
        out[op.name] = BigSlab(op.rows, op.channels, cs, coff, front_margin=margin, device=device, storage=storage)
    return out


def peak_bytes(c):
    """device bytes of a case's slabs (margins included)"""
    return sum(slab_bytes(c, op) for op in c.operands)


def guarded(nbytes):
    """(int32 words of [2 GiB margin | nbytes], all sentinel; the uint8 view of the payload)"""
    words = torch.full(((FRONT_MARGIN + nbytes + 3) // 4,), arena.SENTINEL, dtype=torch.int32, device="cuda")
    return words, words.view(torch.uint8)[FRONT_MARGIN:FRONT_MARGIN + nbytes]


def margin_intact(words):
    return not bool((words[:FRONT_MARGIN // 4] != arena.SENTINEL).any())
