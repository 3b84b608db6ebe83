"""The guard harness of tests/test_gpu_l0_layouts.py on the CPU: a flipped word is found and named, wherever it is."""
import numpy as np
import pytest

from layout_harness import GUARD, POISON_IN, POISON_OUT, UNWRITTEN, Layout


def test_layout_places_columns_and_poison():
    lay = Layout(3, 8, 11)
    assert lay.words == GUARD + 2 * 11 + 8 + GUARD
    live = np.arange(24, dtype=np.uint64).reshape(3, 8)
    img = lay.image(live, POISON_IN)
    for c in range(3):
        assert (img[GUARD + 11 * c: GUARD + 11 * c + 8] == live[c]).all()
        if c < 2:
            assert (img[GUARD + 11 * c + 8: GUARD + 11 * (c + 1)] == POISON_IN).all()
    assert (img[:GUARD] == POISON_IN).all() and (img[-GUARD:] == POISON_IN).all()
    assert (lay.live(img) == live).all()
    assert int((img == POISON_IN).sum()) == lay.words - 24
    assert (Layout(2, 4, 4).image(UNWRITTEN, POISON_OUT)[GUARD:GUARD + 8] == UNWRITTEN).all()
    assert len({POISON_IN, POISON_OUT, UNWRITTEN}) == 3 and POISON_IN >= 0xFFFFFFFF00000001


@pytest.mark.parametrize("n_cols,n,stride", [(3, 8, 9), (3, 8, 16), (1, 8, 8), (5, 1, 2)])
def test_every_flipped_word_is_reported_with_its_offset(n_cols, n, stride):
    lay = Layout(n_cols, n, stride)
    want = lay.image(np.arange(n_cols * n, dtype=np.uint64).reshape(n_cols, n), POISON_OUT)
    assert lay.first_difference(want.copy(), want) is None
    seen = set()
    for off in list(range(GUARD - 2, GUARD + stride * (n_cols - 1) + n + 2)) + [0, lay.words - 1]:
        got = want.copy()
        got[off] ^= np.uint64(1 << 17)                       # one bit of one word
        found, text = lay.first_difference(got, want)
        assert found == off and ("offset %d " % off) in text
        rel = off - GUARD
        live = 0 <= rel < stride * (n_cols - 1) + n and rel % stride < n
        assert ("column %d, word %d" % (rel // stride, rel % stride) in text) == live, text
        assert ("1 column words and 0 guard" in text) == live and ("0 column words and 1 guard" in text) != live
        seen.add(lay.where(off).split(",")[0].split(" ")[0])
    assert seen >= {"lead", "tail", "column"} and (("pad" in seen) == (stride > n and n_cols > 1))


def test_first_of_several_differences_and_the_counts():
    lay = Layout(2, 4, 6)
    want = lay.image(7, POISON_IN)
    got = want.copy()
    got[GUARD + 5] = 0          # pad after column 0
    got[GUARD + 7] = 0          # column 1, word 1
    got[lay.words - 1] = 0      # tail
    off, text = lay.first_difference(got, want)
    assert off == GUARD + 5 and "pad after column 0, word 1 of 2" in text
    assert "holds 0x0000000000000000, must hold 0xffffffffffffffff" in text
    assert "1 column words and 2 guard / pad words differ" in text


def test_layouts_that_guard_nothing_are_refused():
    for args in ((0, 8, 8), (1, 0, 8), (2, 8, 7)):
        with pytest.raises(ValueError):
            Layout(*args)
    with pytest.raises(ValueError):
        Layout(2, 8, 8, lead=16)
