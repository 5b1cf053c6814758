"""A guarded arena for the memory tests (tests/test_gpu_bounds.py): every buffer a call touches is carved out of ONE int32 tensor
whose every word holds a sentinel, so that

* a write outside a buffer changes a known word (Arena.check finds it and says where), and
* a read of memory the call did not write meets a NaN, which makes whatever it reaches NaN.

The sentinel word 0x7FC57FC5 is a quiet NaN as fp32 (exponent all ones, mantissa 0x457FC5), and each 16-bit half, 0x7FC5, is a
quiet NaN as bf16 (exponent 0xFF, mantissa 0x45) and as fp16 (exponent 0x1F, mantissa 0x3C5).

Guard band.  Every carve has at least GUARD = 1 MiB of untouched sentinel of its own on each side (two neighbours are 2 MiB
apart, so a changed word belongs to one carve and one side).  The figure is derived, not measured:
the largest row tile of the library is 128 rows (the 128-row GEMM items, the 128-pixel conv tiles), the widest row at the test
shapes is the 1056 fp32 channels of fusion_14, and a kernel that runs one whole tile past the end of a buffer therefore writes
128 x 1056 x 4 B = 540 672 B.  The other candidates are smaller: a half-image chain block stores 98 rows x 256 channels x 4 B =
100 KB; a 256-pixel conv tile (tile_cfg 2 / 5) has at most 256 output channels per block, 256 x 256 x 4 B = 256 KB; a point of
the Winograd M / V arrays at n = 6 is 6 x 1056 x 4 B = 25 KB.  1 MiB is the next power of two above the largest and leaves room
for a tile that is also misplaced by a row.  A wider case widens GUARD.

The arena works on device="cpu" too; tests/test_arena.py proves there that the checker sees what it has to see.
"""
import torch

SENTINEL = 0x7FC57FC5
GUARD = 1 << 20
_SENTINEL_BYTES = (0xC5, 0x7F, 0xC5, 0x7F)       # little-endian bytes of the word


class GuardBreach(AssertionError):
    pass


class Arena:
    """One int32 tensor full of SENTINEL, handed out in guarded carves.

    Arena(capacity_bytes, device): capacity of the carves alone is not enough -- use Arena.for_sizes(sizes, device), which
    adds the guard bands and the alignment slack."""

    def __init__(self, capacity_bytes, device="cuda"):
        words = (int(capacity_bytes) + 3) // 4
        self.words = torch.full((words,), SENTINEL, dtype=torch.int32, device=device)
        self.bytes = self.words.view(torch.uint8)
        self.base = self.words.data_ptr()
        self.cursor = GUARD                       # first byte a carve may take
        self.carves = []                          # (name, start, nbytes), ascending

    @classmethod
    def for_sizes(cls, sizes, device="cuda", align=256):
        """An arena that holds one carve of each of `sizes` bytes at alignments up to `align` (+ offset < align)."""
        total = GUARD
        for n in sizes:
            total += int(n) + 2 * align + 4 + 2 * GUARD
        return cls(total + align, device)

    def carve(self, name, nbytes, align=256, offset=0):
        """uint8 view of `nbytes` bytes whose ADDRESS is align * k + offset, at least 2 GUARD bytes of sentinel away from every other
        carve and GUARD from both ends of the arena.  The bytes of the view hold the sentinel until somebody writes them."""
        nbytes = int(nbytes)
        if nbytes <= 0 or align <= 0 or align % 4 or offset % 4 or not 0 <= offset < align:
            raise ValueError("carve(%r, %d, align=%d, offset=%d): sizes are positive, align and offset multiples of 4, offset < align"
                             % (name, nbytes, align, offset))
        addr = self.base + self.cursor
        start = self.cursor + (offset - addr) % align
        end = start + nbytes
        if end + GUARD > self.bytes.numel():
            raise ValueError("arena exhausted at carve %r: %d bytes asked, %d left" % (name, nbytes, self.bytes.numel() - GUARD - start))
        self.carves.append((name, start, nbytes))
        self.cursor = end + 2 * GUARD
        return self.bytes[start:end]

    def put(self, name, t, align=256, offset=0):
        """A carve of exactly t's bytes holding a copy of t (contiguous), viewed in t's dtype and shape."""
        t = t.contiguous()
        v = self.carve(name, t.numel() * t.element_size(), align, offset).view(t.dtype).view(t.shape)
        v.copy_(t)
        return v

    def empty(self, name, shape, dtype=torch.float32, align=256, offset=0):
        """A carve of exactly shape x dtype, left full of sentinel, viewed in that dtype and shape."""
        n = 1
        for s in shape:
            n *= int(s)
        return self.carve(name, n * torch.empty((), dtype=dtype).element_size(), align, offset).view(dtype).view(*shape)

    # ---- checking ---------------------------------------------------------------------------------------------------------------
    def _changed(self, lo, hi):
        """Sorted arena byte offsets (first byte of each changed unit) in [lo, hi): whole words compared as int32 -- NaN != NaN as
        float, so never through a float view -- and the bytes of a word a carve shares with its band as uint8."""
        out = []
        wlo, whi = (lo + 3) // 4 * 4, hi // 4 * 4
        if wlo >= whi:                            # a band inside one word
            wlo = whi = hi
        for a, b in ((lo, min(wlo, hi)), (max(whi, lo), hi)):
            for i in range(a, b):
                if int(self.bytes[i]) != _SENTINEL_BYTES[i % 4]:
                    out.append(i)
        if wlo < whi:
            ne = self.words[wlo // 4:whi // 4] != SENTINEL
            if bool(ne.any()):
                out += [wlo + 4 * int(i) for i in ne.nonzero().flatten().tolist()]
        return sorted(out)

    def breaches(self):
        """[(carve name, "before" | "after", first offset, last offset, count)]: offsets in bytes relative to the carve's edge --
        "after": from the first byte behind the carve (0 = the byte right behind it); "before": from the carve's first byte
        (negative).  Count: changed words (changed bytes inside a word the carve shares with its band)."""
        found = []
        total = self.bytes.numel()
        prev_end = None
        for i, (name, start, nbytes) in enumerate(self.carves):
            end = start + nbytes
            lo = 0 if prev_end is None else prev_end + GUARD          # the bands tile the arena: nothing outside the carves goes unchecked
            hi = total if i + 1 == len(self.carves) else end + GUARD
            prev_end = end
            for side, lo, hi, edge in (("before", lo, start, start), ("after", end, hi, end)):
                ch = self._changed(lo, hi)
                if ch:
                    found.append((name, side, ch[0] - edge, ch[-1] - edge, len(ch)))
        return found

    def check(self):
        """Raises GuardBreach unless every guard band still holds the sentinel."""
        found = self.breaches()
        if found:
            raise GuardBreach("; ".join("%s: %d word(s) changed %s the carve, byte offsets %+d .. %+d from its %s"
                                        % (n, c, side, a, b, "first byte" if side == "before" else "end")
                                        for n, side, a, b, c in found))

    def untouched(self, view):
        """True when every word of a carve (or of a 4-byte-aligned slice of one) still holds the sentinel."""
        return bool((view.contiguous().view(torch.uint8).view(torch.int32) == SENTINEL).all())


def bits(t):
    """int32 view of a contiguous 4-byte-element tensor, for bit-exact comparisons."""
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sentinel_floats(*shape):
    """An fp32 tensor on the device whose every word is the sentinel."""
    n = 1
    for s in shape:
        n *= s
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32).view(*shape)


def untouched(t):
    """True when every word of a tensor made of sentinel words (sentinel_floats, an int32 fill) still holds it."""
    return not bool((t.view(torch.int32) != SENTINEL).any())
