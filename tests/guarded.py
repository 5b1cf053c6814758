"""The two runs of the guard-band and stale-memory tests (tests/test_gpu_bounds.py, tests/test_gpu_pool_first.py): run A in ordinary
allocations, run B with every buffer a carve of one sentinel-filled arena (tests/arena.py) -- and the body of a whole forward written
against either.  A helper module: no tests of its own."""
import torch

from offk_amd import spec, synth

from .arena import SENTINEL, Arena, bits, same_bits
from .featmaps import DTYPES

# unit channels (9 x [S 32 | T 128]) of the three fusion buffers: (region, channels per pixel, unit channels)
FUSION = (("fusion_28", 320, 320), ("fusion_14", 1056, 800), ("fusion_7", 832, 320))


# ---- the two runs -----------------------------------------------------------------------------------------------------------------
class Plain:
    """Run A: ordinary allocations.  Records the byte size of every buffer so that run B's arena can be sized."""
    arena = None

    def __init__(self):
        self.sizes = []

    def put(self, name, t, offset=0):
        self.sizes.append(t.numel() * t.element_size())
        return t.to("cuda").contiguous()

    def out(self, name, shape, dtype=torch.float32, offset=0):
        t = torch.empty(*shape, dtype=dtype, device="cuda")
        self.sizes.append(t.numel() * t.element_size())
        return t

    def workspace(self, h):
        self.sizes.append(h.workspace_bytes)
        h._ws = None                                   # the handle's own cached torch.empty, as ever
        return h.workspace

    def must_stay(self, view, what):
        pass


class Guarded:
    """Run B: every buffer a carve of one arena, inputs copied in, everything else left full of the sentinel."""

    def __init__(self, sizes):
        self.arena = Arena.for_sizes(sizes)
        self.stay = []

    def put(self, name, t, offset=0):
        return self.arena.put(name, t, offset=offset)

    def out(self, name, shape, dtype=torch.float32, offset=0):
        return self.arena.empty(name, shape, dtype, offset=offset)

    def workspace(self, h):
        ws = self.arena.carve("workspace", h.workspace_bytes)
        h.set_workspace(ws)
        return ws

    def must_stay(self, view, what):
        self.stay.append((view, what))


def two_runs(body):
    """body(run) -> {name: tensor the call must have filled}.  Runs it plain, then guarded; checks the guards, that everything is
    finite and bit-equal to the plain run, and that what must stay untouched did.  Returns (plain results, guarded results)."""
    plain = Plain()
    a = body(plain)
    torch.cuda.synchronize()
    a = dict((k, v.clone()) for k, v in a.items())
    g = Guarded(plain.sizes)
    b = body(g)
    torch.cuda.synchronize()
    g.arena.check()
    assert a.keys() == b.keys(), (sorted(a), sorted(b))
    for k in b:
        if b[k].is_floating_point():
            assert bool(torch.isfinite(b[k]).all()), "%s: %d non-finite value(s) -- the call left them unwritten, or read memory it did not write" \
                % (k, int((~torch.isfinite(b[k])).sum()))
        assert same_bits(a[k], b[k]), "%s differs from the run in ordinary allocations in %d element(s)" % (k, int((bits(a[k]) != bits(b[k])).sum()))
    for view, what in g.stay:
        words = view.contiguous().view(torch.int32) if view.element_size() == 4 else view.contiguous().view(torch.uint8).view(torch.int32)
        n = int((words != SENTINEL).sum())
        assert n == 0, "%s: %d word(s) written that the path documents as untouched" % (what, n)
    return a, b


def np_feats(B, L, cfg=5):
    return [torch.from_numpy(f) for f in synth.make_features(B, L, cfg)]


def part_channels(i, C):
    """Two to four channel groups of site i, multiples of 32, unequal."""
    units, k = C // 32, 2 + i % 3
    sizes = [units // k] * k
    sizes[0] += units - sum(sizes)
    return [32 * s for s in sizes]


def put_feats(r, feats, form="f32", offset=0, parts=False):
    """The nine maps in run r: form = dtype + optional "cl" (channels_last); parts: every site as its channel groups."""
    dtype, cl = DTYPES[form.replace("cl", "")], form.endswith("cl")
    out = []
    for i, f in enumerate(feats):
        groups = torch.split(f, part_channels(i, f.shape[1]), dim=1) if parts else [f]
        ts = []
        for q, t in enumerate(groups):
            name = "feat_%s%s" % (spec.SITES[i][0], "_part%d" % q if parts else "")
            t = t.to(dtype)
            if cl:
                ts.append(r.put(name, t.permute(0, 2, 3, 1).contiguous(), offset).permute(0, 3, 1, 2))
            else:
                ts.append(r.put(name, t.contiguous(), offset))
        out.append(ts if parts else ts[0])
    return out


def forward_regions(h, fused):
    """What offk.h names as filled after a forward: D_<site>, the fusion buffers, sum_7 -- and G_<site> in the two-kernel form."""
    out = {}
    for name, _c, _h in spec.SITES:
        out["D_" + name] = h.region("D_" + name, 32)
        if not fused:
            out["G_" + name] = h.region("G_" + name, 128)
    for name, ch, _u in FUSION:
        out[name] = h.region(name, ch)
    out["sum_7"] = h.region("sum_7", 1024)
    return out


def g_regions_stay(r, h):
    for name, _c, _h in spec.SITES:
        r.must_stay(h.region("G_" + name, 128), "G_%s (the fused units fill D_<site> but not G_<site>)" % name)


def forward_body(h, feats, form="f32", parts=False, offset=0, want28=True, fused=True, superset=False):
    """fused: True -- the fused units (G_<site> must stay untouched); False -- the two-kernel form (G_<site> filled); None -- neither is
    promised (bound weights)."""
    def body(r):
        fs = put_feats(r, feats, form, offset, parts)
        ws = r.workspace(h)
        shape = (h.out_rows(), h.num_classes)
        outs = (r.out("out7", shape), r.out("out14", shape), r.out("out28", shape) if want28 else None)
        got = h.forward(fs, want28=want28, out=outs)
        res = dict(("out%d" % s, o) for s, o in zip((7, 14, 28), got) if o is not None)
        assert all(o.data_ptr() == g_.data_ptr() for o, g_ in zip(outs, got) if o is not None), "forward(out=...) returned other tensors than it was given"
        res.update(forward_regions(h, fused is not False))
        if fused:
            g_regions_stay(r, h)
        if superset:
            fwd = int(h.lib.offk_workspace_bytes(h._h))
            assert fwd % 4 == 0 and ws.numel() == int(h.lib.offk_train_workspace_bytes(h._h)) > fwd, (fwd, ws.numel())
            r.must_stay(ws[fwd:], "workspace from offk_workspace_bytes to offk_train_workspace_bytes after a forward")
        return res
    return body
