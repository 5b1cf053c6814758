"""The contract of the split-fp32 arithmetic (OFFK_PRECISION_F32SPLIT), on the CPU: the truncating three-plane cut, the TRUE bound of the
three dropped plane products, and a model of the kernels' accumulation that the GPU tests (tests/test_gpu_split.py) take their limits from.

For a truncating cut |m| < 2^-7 |v| and |l| < 2^-15 |v|, so w_m x_l + w_l x_m + w_l x_l < (2 * 2^-22 + 2^-30) |w x| = 8.015625 * 2^-24 |w x|
-- not "below 2^-24", and mantissa 0x00FFFF in both operands reaches 7.83.  The model lives in offk_amd/synth.py (cut3, make_adversarial,
split_terms, emulate_split_dot)."""
import numpy as np
import pytest

import offk_amd  # noqa: F401
from offk_amd import synth

EPS = synth.SPLIT_EPS
MANTS = synth.ADVERSARIAL_MANTISSAS


def _adversarial_values():
    """Every adversarial mantissa at exponents -108 (the smallest whose three planes are all bf16 values) .. 127 and both signs, plus the
    exponent range the generator draws."""
    e = np.concatenate([np.arange(19, 255, 11), np.arange(124, 131)]).astype(np.uint32)
    v = np.concatenate([((e << np.uint32(23)) | np.uint32(m)).view(np.float32) for m in MANTS])
    return np.concatenate([v, -v])


def _random_bits(n, seed):
    b = (synth.raw_u64(seed, 0, n) >> np.uint64(32)).astype(np.uint32)
    v = b.view(np.float32)
    return v[np.isfinite(v)]


def _subnormals():
    m = (synth.raw_u64(77, 0, 4096) >> np.uint64(41)).astype(np.uint32)                  # 23 random mantissa bits, exponent field 0
    edge = np.array([1, 0xFFFF, 0x10000, 0x7FFFFF, 0x7F0000, 0x00FFFF], dtype=np.uint32)
    v = np.concatenate([m, edge]).view(np.float32)
    return np.concatenate([v, -v])


def _check_cut(x):
    h, m, l = synth.cut3(x)
    for p in (h, m, l):
        assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF)), "a plane is not a bf16 value"
    x64 = x.astype(np.float64)
    s = h.astype(np.float64) + m.astype(np.float64) + l.astype(np.float64)
    big = np.abs(x64) >= synth.SPLIT_EXACT_MIN
    assert np.array_equal(s[big], x64[big])
    # (a 24-bit value below 2^-109 does not fit three bf16 planes: its last bits are under the last bf16 subnormal, include/offk.h)
    assert np.all(np.abs(s[~big] - x64[~big]) < 2.0 ** -133)
    nz = x64 != 0
    assert np.all(np.abs(m.astype(np.float64))[nz] < 2.0 ** -7 * np.abs(x64)[nz])
    assert np.all(np.abs(l.astype(np.float64))[nz] < 2.0 ** -15 * np.abs(x64)[nz])
    assert np.all(m[~nz] == 0) and np.all(l[~nz] == 0)
    return big


def test_cut_is_exact_and_planes_are_bounded():
    assert _check_cut(_adversarial_values()).all()
    big = _check_cut(_random_bits(1 << 20, 5))
    assert big.sum() >= 10 ** 6 * 0.85
    sub = _subnormals()
    assert not _check_cut(sub).any()
    # subnormals that ARE bf16 values (low 16 bits clear) are their own leading plane, exactly
    rep = (sub.view(np.uint32) & np.uint32(0xFFFF)) == 0
    h, m, l = synth.cut3(sub[rep])
    assert rep.any() and np.array_equal(h, sub[rep]) and not m.any() and not l.any()


def _drop_ratio(w, x):
    """|w x - kept| / (2^-24 |w x|) per pair, kept = the six kept plane products summed in fp64 (each is exact there)."""
    wp = [p.astype(np.float64) for p in synth.cut3(w)]
    xp = [p.astype(np.float64) for p in synth.cut3(x)]
    kept = wp[0] * xp[0] + wp[0] * xp[1] + wp[1] * xp[0] + wp[1] * xp[1] + wp[0] * xp[2] + wp[2] * xp[0]
    full = w.astype(np.float64) * x.astype(np.float64)
    return np.abs(full - kept) / (EPS * np.abs(full))


def test_dropped_products_obey_the_true_bound():
    adv = _adversarial_values()
    adv = adv[(np.abs(adv) > 2.0 ** -60) & (np.abs(adv) < 2.0 ** 60)]
    r = _drop_ratio(np.repeat(adv, adv.size), np.tile(adv, adv.size))
    assert r.max() <= synth.SPLIT_DROP_BOUND
    a, b = _random_bits(1 << 20, 6), _random_bits(1 << 20, 7)
    n = min(a.size, b.size)
    a, b = a[:n], b[:n]
    ok = (np.abs(a) >= synth.SPLIT_EXACT_MIN) & (np.abs(b) >= synth.SPLIT_EXACT_MIN)
    assert ok.sum() >= 10 ** 6 * 0.7
    rr = _drop_ratio(a[ok], b[ok])
    assert rr.max() <= synth.SPLIT_DROP_BOUND
    print("dropped / (2^-24 |w x|): adversarial pairs max %.3f, %d random bit patterns max %.3f mean %.3f" % (r.max(), ok.sum(), rr.max(), rr.mean()))


def test_the_bound_is_reached_so_below_2_to_minus_24_was_wrong():
    one = lambda m: np.array([0x3F800000 | m], dtype=np.uint32).view(np.float32)
    assert 7.8 <= _drop_ratio(one(0x00FFFF), one(0x00FFFF))[0] <= synth.SPLIT_DROP_BOUND
    assert 1.9 < _drop_ratio(one(0x7FFFFF), one(0x7FFFFF))[0] < 2.0          # the one pattern the earlier review tried
    assert 5.8 < _drop_ratio(one(0x00FF7F), one(0x00FFFF))[0] < 5.9


def test_make_adversarial():
    for pat in MANTS + ("mixed",):
        v = synth.make_adversarial((6, 64), pat, "alternating", seed=3)
        assert v.dtype == np.float32 and v.shape == (6, 64)
        assert np.all(v[:, 0::2] > 0) and np.all(v[:, 1::2] < 0)
        mant = v.view(np.uint32) & np.uint32(0x7FFFFF)
        assert set(mant.ravel().tolist()) <= (set(MANTS) if pat == "mixed" else {pat})
        assert np.all((np.abs(v) >= 0.125) & (np.abs(v) < 16.0)) and len(set(np.frexp(v)[1].ravel().tolist())) == 7
    v = synth.make_adversarial((4, 8, 5, 5), 0x00FFFF, "same", seed=1, relu=True)
    assert np.all(v >= 0) and 0.35 < (v == 0).mean() < 0.65
    assert np.array_equal(v, synth.make_adversarial((4, 8, 5, 5), 0x00FFFF, "same", seed=1, relu=True))
    a = synth.make_adversarial((3, 32, 2), 0x7F7F7F, "alternating", seed=2, k_axis=1)
    assert np.all(a[:, 0::2] > 0) and np.all(a[:, 1::2] < 0)


def _operands(K, pattern, signs, seed, M=48, N=40, relu=False):
    w = synth.make_adversarial((N, K), pattern, signs, seed=seed) * np.float32(2.0 ** -np.round(np.log2(K) / 2))
    x = synth.make_adversarial((M, K), pattern, "same", seed=seed + 1, relu=relu)
    return w, x


@pytest.mark.parametrize("form", ["units", "gemm"])
def test_emulation_keeps_the_six_products(form):
    """The emulation against kept64: its accumulation error is fp32-class (c_acc of order 1), so the exact dropped part plus
    A 2^-24 sum |w x| holds with A = max(1, 2 c_acc) by construction -- and the dropped part alone is up to 7.8."""
    for K in (64, 1024):
        for signs in ("same", "alternating"):
            w, x = _operands(K, 0x00FFFF, signs, 11)
            ref, dropped, mag = synth.split_terms(w, x)
            c = synth.split_c_acc(synth.emulate_split_dot(w, x, form), ref, dropped, mag)
            print("emulation %-5s K %4d %-11s: c_acc max %.3f  dropped / (2^-24 mag) max %.3f" % (form, K, signs, c.max(), (np.abs(dropped) / (EPS * mag)).max()))
            assert c.max() < 8.0
            assert np.all(np.abs(dropped) <= synth.SPLIT_DROP_BOUND * EPS * mag)
            if signs == "same":
                assert (np.abs(dropped) / (EPS * mag)).max() > 7.0


def test_emulation_is_exact_where_the_arithmetic_is():
    """Operands with one plane and products that fit an fp32 accumulator exactly: both forms give the fp64 result."""
    g = np.random.default_rng(3)
    w = g.integers(-15, 16, (8, 96)).astype(np.float32)
    x = g.integers(-15, 16, (5, 96)).astype(np.float32)
    want = x.astype(np.float64) @ w.astype(np.float64).T
    for form in ("units", "gemm"):
        assert np.array_equal(synth.emulate_split_dot(w, x, form).astype(np.float64), want)


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("pattern", [0x00FFFF, 0x7FFFFF, 0x7F7F7F])
@pytest.mark.parametrize("signs", ["same", "alternating"])
@pytest.mark.parametrize("K", [64, 1024])
def test_losing_any_kept_product_breaks_the_gpu_inequality(K, signs, pattern, relu):
    """What makes the GPU tests of tests/test_gpu_split.py meaningful: on the adversarial inputs, an implementation that loses ANY one of the
    six kept plane products violates |out - ref64| <= |ref64 - kept64| + A 2^-24 sum |w x| (A = max(1, 2 c_acc of the intact emulation)),
    in both accumulation forms -- the smallest kept products (w_h x_l, w_l x_h) are ~2^-16 of the leading one, c ~ 256."""
    w, x = _operands(K, pattern, signs, 100 + K, relu=relu)
    ref, dropped, mag = synth.split_terms(w, x)
    for form in ("units", "gemm"):
        good = synth.emulate_split_dot(w, x, form)
        A = max(1.0, 2.0 * synth.split_c_acc(good, ref, dropped, mag).max())
        limit = np.abs(dropped) + A * EPS * mag
        assert np.all(np.abs(good.astype(np.float64) - ref) <= limit)
        for skip in range(6):
            bad = synth.emulate_split_dot(w, x, form, skip=skip)
            viol = np.abs(bad.astype(np.float64) - ref) > limit
            assert viol.mean() > 0.5, (form, skip, synth.SPLIT_PRODUCTS[skip], float(viol.mean()))
