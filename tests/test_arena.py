"""The guarded arena of tests/arena.py on the CPU: the proof that its checker has teeth.  Every write here is torch indexing."""
import struct

import pytest
import torch

from .arena import GUARD, SENTINEL, Arena, GuardBreach, same_bits


def make(sizes=(4096, 1000, 64)):
    a = Arena.for_sizes(sizes, device="cpu")
    return a, [a.carve("c%d" % i, n) for i, n in enumerate(sizes)]


def test_sentinel_is_a_nan_in_all_three_formats():
    word = torch.tensor([SENTINEL], dtype=torch.int32)
    assert torch.isnan(word.view(torch.float32)).all()
    assert torch.isnan(word.view(torch.bfloat16)).all() and torch.isnan(word.view(torch.float16)).all()
    assert struct.pack("<i", SENTINEL) == bytes([0xC5, 0x7F, 0xC5, 0x7F])


def test_clean_arena_passes_and_carves_hold_the_sentinel():
    a, cs = make()
    a.check()
    assert a.breaches() == []
    for c in cs:
        assert c.dtype == torch.uint8 and a.untouched(c)
    assert torch.isnan(cs[0].view(torch.float32)).all() and torch.isnan(cs[1].view(torch.bfloat16)).all()
    cs[0].view(torch.float32).fill_(1.5)           # writing INSIDE a carve is no breach
    cs[1].fill_(0)
    a.check()
    assert not a.untouched(cs[0])


def test_guard_bands_are_at_least_one_mib_on_each_side():
    a, _cs = make()
    prev_end = 0
    for _name, start, nbytes in a.carves:
        assert start - prev_end >= (2 * GUARD if prev_end else GUARD)
        prev_end = start + nbytes
    assert a.bytes.numel() - prev_end >= GUARD


def test_one_word_changed_one_byte_past_a_carve():
    a = Arena.for_sizes((4099, 256), device="cpu")
    c = a.carve("odd", 4099)                       # ends one byte short of a word boundary
    a.carve("next", 256)
    _name, start, nbytes = a.carves[0]
    w = (start + nbytes + 1) // 4
    assert 4 * w == start + nbytes + 1
    a.words[w] = 0
    assert a.breaches() == [("odd", "after", 1, 1, 1)]
    with pytest.raises(GuardBreach, match=r"odd: 1 word\(s\) changed after the carve, byte offsets \+1 \.\. \+1 from its end"):
        a.check()
    assert a.untouched(c[:4096])
    a.words[w] = SENTINEL
    a.check()
    a.bytes[start + nbytes] = 0                    # the byte right behind the carve, inside the word the carve ends in
    assert a.breaches() == [("odd", "after", 0, 0, 1)]


def test_word_right_behind_and_right_in_front_of_a_carve():
    a, _cs = make()
    _name, start, nbytes = a.carves[1]             # 1000 bytes: a whole number of words
    a.words[(start + nbytes) // 4] = 1
    assert a.breaches() == [("c1", "after", 0, 0, 1)]
    a.words[(start + nbytes) // 4] = SENTINEL
    a.words[start // 4 - 1] = 1
    a.words[start // 4 - 3] = 1
    assert a.breaches() == [("c1", "before", -12, -4, 2)]
    with pytest.raises(GuardBreach, match=r"c1: 2 word\(s\) changed before the carve, byte offsets -12 \.\. -4 from its first byte"):
        a.check()


def test_a_float_nan_of_another_pattern_is_seen():
    """The comparison is on int32: another NaN, or the sentinel with one bit flipped, is a change."""
    a, _cs = make()
    _name, start, nbytes = a.carves[0]
    a.words[(start + nbytes) // 4 + 5].view(torch.float32).fill_(float("nan"))
    assert a.breaches() == [("c0", "after", 20, 20, 1)]


def test_one_word_changed_one_mib_minus_four_bytes_away_is_seen():
    a, _cs = make()
    _name, start, nbytes = a.carves[0]
    a.words[(start + nbytes + GUARD - 4) // 4] = 7
    assert a.breaches() == [("c0", "after", GUARD - 4, GUARD - 4, 1)]
    a.words[(start + nbytes + GUARD - 4) // 4] = SENTINEL
    a.words[(start - GUARD) // 4] = 7
    assert a.breaches() == [("c0", "before", -GUARD, -GUARD, 1)]
    a.words[(start - GUARD) // 4] = SENTINEL
    _name, start, nbytes = a.carves[-1]
    a.words[(start + nbytes + GUARD - 4) // 4] = 7
    a.words[(start - GUARD) // 4] = 7
    assert a.breaches() == [("c2", "before", -GUARD, -GUARD, 1), ("c2", "after", GUARD - 4, GUARD - 4, 1)]


@pytest.mark.parametrize("offset,more", [(0, 512), (4, 8), (8, 16), (16, 32)])
def test_carves_have_the_alignment_asked_for_and_no_more(offset, more):
    a = Arena.for_sizes((1024, 1024, 1024), device="cpu")
    a.carve("pad", 12)                             # leave the cursor at no round address
    for name in ("x", "y"):
        c = a.carve(name, 1024, align=256, offset=offset)
        assert c.data_ptr() % 256 == offset
        if offset:
            assert c.data_ptr() % offset == 0 and c.data_ptr() % more != 0
        assert c.numel() == 1024
        c.view(torch.bfloat16).fill_(1.0)          # typed views of a minimally aligned carve work
    a.check()


def test_put_and_empty_are_exact_size_typed_carves():
    a = Arena.for_sizes((3 * 5 * 4, 7 * 2), device="cpu")
    src = torch.arange(15, dtype=torch.float32).view(3, 5)
    p = a.put("in", src)
    e = a.empty("out", (7,), torch.bfloat16)
    assert same_bits(p, src) and p.shape == src.shape and a.carves[0][2] == 60
    assert a.carves[1][2] == 14 and torch.isnan(e).all()
    a.check()


def test_exhausted_arena_and_bad_arguments_raise():
    a = Arena(GUARD * 3 + 100 + 256, device="cpu")
    a.carve("fits", 100)
    with pytest.raises(ValueError, match="exhausted"):
        a.carve("too much", 4)
    with pytest.raises(ValueError):
        a.carve("odd offset", 8, align=256, offset=2)
