"""Guarded buffer layouts for the L0 entry points (include/bpg.h, "Buffers of the L0 entries").

A buffer of a call is one allocation of  lead | column 0 | pad | column 1 | pad | ... | column n_cols-1 | tail  words,
column c at lead + c * stride.  Everything outside the n-word column bodies is poison; the call gets base + lead and
the stride.  Afterwards the WHOLE allocation is compared with the image it must have: the oracle's words in the column
bodies, and every other word bit-identical to what it was -- so a kernel that writes a pad word, or that reads one as
data (input poison is 2^64 - 1: no oracle computes on it), fails with the offset of the first wrong word.

The layout arithmetic and the comparison are numpy only (tests/test_layout_harness.py runs them without a GPU); the
device half clones a pristine image per call and compares on the device, so a case costs the kernel and two passes
over the buffer."""
import numpy as np

GUARD = 4096                          # lead and tail, in words
POISON_IN = 0xFFFFFFFFFFFFFFFF        # pads of buffers a call reads (and of in-place buffers): not canonical
POISON_OUT = 0xA5A5A5A55A5A5A5A       # pads of buffers a call only writes
UNWRITTEN = 0x0BADC0DE0BADC0DE        # column bodies of an output before the call


class Layout:
    def __init__(self, n_cols, n, stride=None, lead=GUARD, tail=GUARD):
        stride = n if stride is None else stride
        if n_cols < 1 or n < 1 or stride < n or lead < GUARD or tail < GUARD:
            raise ValueError("layout: %d columns of %d words at stride %d, guards %d / %d" % (n_cols, n, stride, lead, tail))
        self.n_cols, self.n, self.stride, self.lead, self.tail = n_cols, n, stride, lead, tail
        self.words = lead + stride * (n_cols - 1) + n + tail

    def live(self, image):
        """the column bodies of a host image as a writable [n_cols, n] view"""
        assert image.dtype == np.uint64 and image.shape == (self.words,)
        return np.lib.stride_tricks.as_strided(image[self.lead:], shape=(self.n_cols, self.n),
                                               strides=(self.stride * 8, 8))

    def image(self, live, poison):
        """host image: `live` ([n_cols, n] words, or one word for all of them) in the column bodies, poison elsewhere"""
        img = np.full(self.words, poison, dtype=np.uint64)
        self.live(img)[...] = live
        return img

    def where(self, off):
        """what the word at offset `off` of the allocation is"""
        if off < self.lead:
            return "lead guard, %d words before the first column" % (self.lead - off)
        c, i = divmod(off - self.lead, self.stride)
        if c >= self.n_cols or (c == self.n_cols - 1 and i >= self.n):
            return "tail guard, %d words past the last column" % (off - self.lead - self.stride * (self.n_cols - 1) - self.n)
        if i >= self.n:
            return "pad after column %d, word %d of %d" % (c, i - self.n, self.stride - self.n)
        return "column %d, word %d" % (c, i)

    def first_difference(self, got, want):
        """None, or (offset, description) of the first word of `got` that is not `want`'s"""
        bad = np.flatnonzero(got != want)
        if not bad.size:
            return None
        off = int(bad[0])
        rel = bad - self.lead
        n_live = int(((rel >= 0) & (rel // self.stride < self.n_cols) & (rel % self.stride < self.n)).sum())
        return off, ("offset %d (%s) holds 0x%016x, must hold 0x%016x; %d column words and %d guard / pad words differ"
                     % (off, self.where(off), int(got[off]), int(want[off]), n_live, bad.size - n_live))


class Guarded:
    """A buffer of one call on the device: the pristine image, and a fresh copy of it per call."""

    def __init__(self, name, layout, live, poison):
        from util import to_dev
        self.name, self.layout = name, layout
        self.before = to_dev(layout.image(live, poison))
        self.poison = poison
        self.dev = None

    def fresh(self):
        """a new copy of the pristine image; returns the address of column 0"""
        self.dev = self.before.clone()
        return self.dev.data_ptr() + 8 * self.layout.lead

    def expect(self, live):
        """device image the buffer must have after a call that leaves `live` in the column bodies"""
        from util import to_dev
        return to_dev(self.layout.image(live, self.poison))

    def _bodies(self, t):
        lay = self.layout
        return t[lay.lead:lay.words - lay.tail].as_strided((lay.n_cols, lay.n), (lay.stride, 1))

    def check(self, want=None, what="", scratch=False):
        """the buffer is bit for bit `want` (from expect(); default: untouched).  scratch: the column bodies may hold
        anything (a scratch buffer of the stated size), everything around them is untouched."""
        import torch
        want = self.before if want is None else want
        if scratch:
            self._bodies(self.dev).copy_(self._bodies(want))
        if torch.equal(self.dev, want):
            return
        from util import to_host
        off, text = self.layout.first_difference(to_host(self.dev), to_host(want))
        raise AssertionError("%s%s: %s" % (self.name, " (%s)" % what if what else "", text))
