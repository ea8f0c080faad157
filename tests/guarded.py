"""Output buffers between canary rows: every buffer a GPU test hands to a kernel is a view inside a larger allocation
whose surroundings must still hold the canary after the launch (a write outside the buffer that stays inside the
allocation is caught here, not by the next test's fault)."""
import torch

GUARD = 64
CANARY = 12345.0
DIRTY = 1e30


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
