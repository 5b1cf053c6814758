"""tests/big.py on the CPU: the checker sees what it has to see, and every case of tests/test_gpu_big_slabs.py is one at which a
32-bit byte offset really wraps AND the wrapped access stays inside the allocation the test owns.  No GPU and no big allocation here:
part 1 runs on slabs of a few hundred bytes, part 2 is integer arithmetic on the geometry the device test will allocate."""
import pytest
import torch

from . import arena, big


def small(dtype=torch.float32):
    return big.BigSlab(rows=5, channels=8, cstride=24, coff=8, dtype=dtype, front_margin=64, device="cpu")


# ---- part 1: the checker ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_a_fresh_slab_is_all_nan_and_untouched(dtype):
    s = small(dtype)
    assert s.untouched() and s.untouched_outside() and s.changed_outside() == 0
    assert bool(s.slab.isnan().all()), "the sentinel reads as NaN in %s" % dtype
    assert s.view.shape == (5, 8) and s.view.data_ptr() == s.slab.data_ptr() + 8 * s.esz
    assert s.slab.data_ptr() == s.words.data_ptr() + 64


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fill_changes_the_view_only(dtype):
    s = small(dtype)
    t = torch.arange(40, dtype=torch.float32).reshape(5, 8).to(dtype)
    s.fill(t)
    assert torch.equal(s.view, t)
    assert s.untouched_outside() and not s.untouched()


def words_per_row(s):
    return s.cstride * s.esz // 4


SPOTS = {
    "first word of the margin": lambda s: 0,
    "inside the margin": lambda s: s.front_margin // 8,
    "directly before the view": lambda s: s.front_margin // 4 + s.coff * s.esz // 4 - 1,
    "directly after the view's first row": lambda s: s.front_margin // 4 + (s.coff + s.channels) * s.esz // 4,
    "neighbouring channel in front of the last row": lambda s: s.front_margin // 4 + (s.rows - 1) * words_per_row(s) + s.coff * s.esz // 4 - 1,
    "neighbouring channel behind the last row": lambda s: s.front_margin // 4 + (s.rows - 1) * words_per_row(s) + (s.coff + s.channels) * s.esz // 4,
    "directly after the view (last word of the slab)": lambda s: s.words.numel() - 1,
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("spot", sorted(SPOTS))
def test_one_changed_word_outside_the_view_is_seen(spot, dtype):
    s = small(dtype)
    s.fill(torch.ones(5, 8))
    i = SPOTS[spot](s)
    s.words[i] = 0
    assert not s.untouched_outside() and s.changed_outside() == 1, spot
    s.words[i] = arena.SENTINEL
    assert s.untouched_outside()


def test_a_changed_half_word_is_seen():
    """a 16-bit store of the sentinel's own upper half into the lower half: the word differs although each half is a NaN"""
    s = small(torch.bfloat16)
    halves = s.words.view(torch.int16)
    i = 2 * (s.front_margin // 4 + 2 * words_per_row(s))        # row 2, channel 0
    assert int(halves[i]) == int(halves[i + 1]) == 0x7FC5
    halves[i] = 0x7FC6                                           # still a NaN as bf16
    assert bool(s.slab[2, 0].isnan()) and s.changed_outside() == 1


def test_a_nan_with_another_payload_is_a_change():
    s = small()
    s.slab[4, 23] = float("nan")                 # torch's default NaN, 0x7FC00000
    assert s.changed_outside() == 1, "compared as int32, never through a float view"


def test_a_view_that_ends_with_the_row_has_nothing_behind_it():
    s = big.BigSlab(rows=3, channels=8, cstride=16, coff=8, front_margin=0, device="cpu")
    s.fill(torch.zeros(3, 8))
    assert s.untouched_outside()
    s.slab[1, 7] = 0.0
    assert s.changed_outside() == 1


def test_geometry_is_checked():
    with pytest.raises(ValueError):
        big.BigSlab(2, 8, 12, 8, device="cpu")                                  # coff + channels > cstride
    with pytest.raises(ValueError):
        big.BigSlab(2, 8, 17, 2, dtype=torch.bfloat16, front_margin=0, device="cpu")   # a row pitch of 34 bytes
    with pytest.raises(ValueError):
        big.cstride_past(1, 2 ** 31)


@pytest.mark.parametrize("rows", [2, 3, 30, 98, 392, 588])
@pytest.mark.parametrize("mark", big.MARKS)
@pytest.mark.parametrize("align", [1, 4, 32])
def test_cstride_past_is_the_smallest(rows, mark, align):
    cs = big.cstride_past(rows, mark, align)
    assert cs % align == 0
    assert (rows - 1) * cs * 4 > mark
    assert (rows - 1) * (cs - align) * 4 <= mark
    assert cs < 2 ** 31, "the entries take the stride as an int"


# ---- part 2: every case of the device test, arithmetic only ------------------------------------------------------------------------
CASES = big.cases()


def as_int32(v):
    v &= 0xFFFFFFFF
    return v - 2 ** 32 if v >= 2 ** 31 else v


def test_marks_and_case_list():
    assert big.MARKS == (2 ** 31, 2 ** 32) and big.FRONT_MARGIN == 2 ** 31
    ids = [big.case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    for entry, keys in big.ENTRIES.items():
        for key, ops in keys.items():
            assert all(op.rows >= 2 for op in ops), (entry, key)
            for mark in big.MARKS:
                mine = [c for c in CASES if (c.entry, c.key, c.mark) == (entry, key, mark)]
                assert {c.past for c in mine} >= {(op.name,) for op in ops}, "each operand alone past the mark"
                assert tuple(op.name for op in ops) in {c.past for c in mine}, "one case with every operand past the mark"


@pytest.mark.parametrize("c", CASES, ids=[big.case_id(c) for c in CASES])
def test_the_last_rows_offset_wraps_inside_the_allocation(c):
    assert c.past, "a case puts at least one operand past its mark"
    for op in c.operands:
        cs, coff, margin = big.geometry(c, op)
        assert cs % 4 == 0 and coff % 4 == 0 and coff > 0 and coff + op.channels <= cs and 0 < cs < 2 ** 31
        slab_bytes = op.rows * cs * 4
        first = ((op.rows - 1) * cs + coff) * 4                       # first byte of the view's last row
        last = first + op.channels * 4 - 4                            # its last word
        if op.name not in c.past:
            assert slab_bytes < 2 ** 24 and margin == big.SMALL_MARGIN      # far below either mark
            continue
        assert margin == big.FRONT_MARGIN
        assert (op.rows - 1) * cs * 4 > c.mark, "the last row starts past the mark"
        assert slab_bytes <= c.mark * op.rows / (op.rows - 1) + 32 * op.rows, "one row past the mark, not more: rows / (rows - 1) of the mark"
        for off in (first, last):
            wrapped = [as_int32(off)]                                  # what an int byte offset holds
            if c.mark == 2 ** 32:
                wrapped.append(off % 2 ** 32)                          # what an unsigned one holds; below 2^32 it is the offset itself
            else:
                assert off % 2 ** 32 == off and off < 2 ** 32
            for w in wrapped:
                assert w != off, "the wrap is visible: another address than the right one"
                assert -margin <= w < slab_bytes - 3, "... and inside the allocation"
                # the wrapped word is not one of the view's own last-row words (it would then read the right values by accident)
                assert not first <= w <= last
        # the image before the last one is below the mark in the 2 GiB cases with two images: the call covers both sides
        assert op.rows * cs * 4 < 2 ** 33, "element indices stay below 2^31: only byte offsets can wrap here"


def test_peak_memory_of_a_case():
    worst = max(big.peak_bytes(c) for c in CASES)
    assert worst <= 3 * (1.05 * 2 ** 32 + big.FRONT_MARGIN), worst          # three slabs of 98 rows past 4 GiB, each behind its margin: 19.6 GB


# ---- the handle limit: offk_create's batch * length * 784 * 320 <= 2^31 - 1 (the largest map, site 3b, counted in elements) ----------
def _create(batch, length):
    import ctypes

    import offk_amd  # noqa: F401
    from offk_amd import _lib
    lib = _lib.load()
    cfg = _lib.OffkConfig(batch, length, 0, 0, 0, 101, 0, 0, 0)
    h = ctypes.c_void_p()
    rc = lib.offk_create(ctypes.byref(cfg), ctypes.byref(h))
    msg = (lib.offk_last_error(None) or b"").decode()
    if h.value:
        lib.offk_destroy(h)
    return rc, msg


def test_offk_create_takes_8559_images_and_refuses_8560():
    """The size check precedes every device call, so its edge shows with and without a device: N = 8559 (8559 x 250 880 = 2 147 281 920
    elements <= 2^31 - 1) passes it -- the handle is created (weights only: nothing of a handle scales with N), or, without a device,
    the call gets as far as OFFK_ERR_NO_DEVICE; N = 8560 (2 147 532 800) is OFFK_ERR_INVALID with the documented message.  No forward
    is run at that size."""
    assert 8559 * 784 * 320 <= 2 ** 31 - 1 < 8560 * 784 * 320
    for batch, length in ((2853, 3), (951, 9)):
        assert batch * length == 8559
        rc, msg = _create(batch, length)
        assert rc in (0, -5), (rc, msg)
        assert "too large" not in msg or rc == 0
        if rc == -5:
            assert "device" in msg
    for batch, length in ((4280, 2), (1712, 5), (8560, 7)):
        rc, msg = _create(batch, length)
        assert rc == -1, (batch, length, rc, msg)
        assert msg == "offk_create: batch*length too large for one call; shard the clips"


def test_a_pool_buffer_is_reused_and_refilled():
    """big.Pool on the CPU with a stand-in size: two slabs carved from the same storage one after the other -- the second one starts all
    sentinel although the first was written, and words of the storage behind a slab are not the slab's"""
    pool = big.Pool(device="cpu")
    assert pool.nwords * 4 == max(big.slab_bytes(c, op) for c in CASES for op in c.operands if op.name in c.past) <= 7e9
    pool.nwords = 200
    a = big.BigSlab(5, 8, 24, 8, front_margin=64, device="cpu", storage=pool.storage(0))
    a.fill(torch.ones(5, 8))
    a.words[3] = 0
    assert a.changed_outside() == 1 and a.words.numel() == 16 + 5 * 24 and len(pool.bufs) == 1
    b = big.BigSlab(4, 8, 24, 8, front_margin=64, device="cpu", storage=pool.storage(0))
    assert b.words.data_ptr() == a.words.data_ptr() and b.untouched()
    assert torch.equal(pool.bufs[0][b.words.numel():a.words.numel()].view(torch.float32)[8:16], torch.ones(8))   # (behind b: a's last row, left as it was)
    pool.release()
    assert pool.bufs == []
