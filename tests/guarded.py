"""Output buffers between canary rows: every buffer a GPU test hands to a kernel is a view inside a larger allocation
whose surroundings must still hold the canary after the launch (a write outside the buffer that stays inside the
allocation is caught here, not by the next test's fault)."""
import math

import torch

GUARD = 64
CANARY = 12345.0
DIRTY = 1e30
CANARIES = {torch.uint8: 0xA5, torch.int8: 99, torch.int32: -77, torch.int64: -77, torch.float32: CANARY, torch.float64: CANARY}


class Guarded:
    """``rows`` x ``cols`` between GUARD canary rows on either side"""

    def __init__(self, rows, cols, dtype=torch.float32, fill=DIRTY, canary=CANARY):
        self.buf = torch.full((rows + 2 * GUARD, cols), canary, dtype=dtype, device="cuda")
        self.t = self.buf[GUARD:GUARD + rows]
        self.t.fill_(fill)
        self.rows, self.canary = rows, canary

    def intact(self):
        c = torch.full_like(self.buf[:GUARD], self.canary)
        return torch.equal(self.buf[:GUARD], c) and torch.equal(self.buf[GUARD + self.rows:], c)


class Flat:
    """``shape`` (or a count) elements of ``dtype`` in one flat allocation, GUARD x ``rows`` canary elements in front of
    them (``shift`` more, to move the inside off its alignment) and as many behind.  ``.t`` is the inside, which starts as
    the canary too unless ``fill`` is given; ``.buf`` the whole allocation"""

    def __init__(self, shape, dtype, canary=None, fill=None, rows=1, shift=0, device="cuda"):
        shape = tuple(shape) if isinstance(shape, (tuple, list)) else (shape,)
        self.canary = CANARIES[dtype] if canary is None else canary
        self.lo, self.n = GUARD * rows + shift, math.prod(shape)
        self.buf = torch.full((self.lo + self.n + GUARD * rows,), self.canary, dtype=dtype, device=device)
        self.t = self.buf[self.lo:self.lo + self.n].view(shape)
        if fill is not None:
            self.t.fill_(fill)

    def address(self):
        """of the inside (an empty view has no pointer of its own)"""
        return self.buf.data_ptr() + self.lo * self.buf.element_size()

    def intact(self):
        """every element in front of and behind the inside still holds the canary"""
        return bool((self.buf[:self.lo] == self.canary).all()) and bool((self.buf[self.lo + self.n:] == self.canary).all())

    def snapshot(self):
        return self.buf.clone()

    def unchanged(self, snapshot):
        """the whole allocation, inside included, against a snapshot: nothing at all was written"""
        return torch.equal(self.buf, snapshot)
