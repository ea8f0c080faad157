"""Numpy restatement of the event-biased patch selection (include/ramp_hip.h ``ramp_event_topk``) -- TEST INFRASTRUCTURE ONLY.

Four steps, each exact (no tolerance anywhere):

    score(ev)      [bins,H,W] -> [w,h], h = H // 4, w = W // 4: per bin the 16 |values| of a cell summed in (ky, kx) order in
                   float32 and divided by 16, the bins summed in order and divided by ``bins``, transposed.  Rows of H beyond
                   4 h are ignored.  For integer-valued events every step but the last division is exact, so the result does
                   not depend on the summation order and equals torch's avg_pool2d(...).transpose(3, 2).mean(1) to the bit.
    nms(s, ks)     a cell keeps its value when no cell of its (2r+1)^2 window, r = (ks - 1) // 2, clipped at the border, is
                   STRICTLY larger (equal neighbours all survive); otherwise it becomes value * 0.  ks 0 or 1: no NMS.
    topk(s, k)     flat indices of the [w,h] map, value descending, ties by lowest flat index.
    coords(idx, h) x = float32(idx) * (float32(1) / float32(h)) (the TRUE division upstream, as the device evaluates it: x
                   carries y / h), y = float32(idx % h).

The ``mistake`` keywords break the restatement on purpose (tests/test_selectref_cpu.py: each has to be rejected).

The second half builds the integer-valued event stacks that tests/test_patch_selection_gpu.py runs the kernel on (and
test_selectref_cpu.py the torch pipeline): deterministic, a seeded generator for placement only."""
import numpy as np

SCORE_MISTAKES = ("hw", "rows")
NMS_MISTAKES = ("ge", "radius", "wrap")
TOPK_MISTAKES = ("highest",)
COORD_MISTAKES = ("floordiv",)
TOPK_CAP = 6144              # csrc/select.hip: more non-zero cells than this stream from memory
SEL_SLOTS = 1024             # what the gather of cells >= threshold held before ties were taken in index order


def score(ev, mistake=None):
    assert mistake is None or mistake in SCORE_MISTAKES
    ev = np.asarray(ev, np.float32)
    bins, H, W = ev.shape
    h, w = H // 4, W // 4
    a = np.abs(ev[:, :4 * h, :4 * w]).reshape(bins, h, 4, w, 4)
    tot = np.zeros((h, w), np.float32)
    for b in range(bins):
        acc = np.zeros((h, w), np.float32)
        for ky in range(4):
            for kx in range(4):
                acc = acc + a[b, :, ky, :, kx]
        if mistake == "rows" and H > 4 * h:           # the leftover rows folded into the last row of cells
            acc[h - 1] = acc[h - 1] + np.abs(ev[b, 4 * h:, :4 * w]).reshape(-1, w, 4).sum((0, 2), dtype=np.float32)
        tot = tot + acc / np.float32(16)
    tot = tot / np.float32(bins)
    return np.ascontiguousarray(tot if mistake == "hw" else tot.T)


def nms(s, kernel_size, mistake=None):
    assert mistake is None or mistake in NMS_MISTAKES
    s = np.asarray(s, np.float32)
    if kernel_size <= 1:
        return s.copy()
    r = (kernel_size - 1) // 2 + (mistake == "radius")
    w, h = s.shape
    pad = np.full((w + 2 * r, h + 2 * r), -np.inf, np.float32)
    pad[r:r + w, r:r + h] = s
    larger = np.zeros(s.shape, bool)
    for dx in range(-r, r + 1):
        for dy in range(-r, r + 1):
            if dx == 0 and dy == 0:
                continue
            if mistake == "wrap":
                nb = np.roll(s, (-dx, -dy), (0, 1))
            else:
                nb = pad[r + dx:r + dx + w, r + dy:r + dy + h]
            larger |= (nb >= s) if mistake == "ge" else (nb > s)
    return np.where(larger, s * np.float32(0), s)


def topk(s, k, mistake=None):
    assert mistake is None or mistake in TOPK_MISTAKES
    flat = np.asarray(s, np.float32).reshape(-1)
    assert 0 < k <= flat.size
    if mistake == "highest":
        return (flat.size - 1 - np.argsort(-flat[::-1], kind="stable")[:k]).astype(np.int64)
    return np.argsort(-flat, kind="stable")[:k].astype(np.int64)


def coords(idx, h, mistake=None):
    assert mistake is None or mistake in COORD_MISTAKES
    idx = np.asarray(idx, np.int64)
    if mistake == "floordiv":
        x = (idx // h).astype(np.float32)
    else:
        x = idx.astype(np.float32) * (np.float32(1) / np.float32(h))
    return np.stack([x, (idx % h).astype(np.float32)], -1)


def select(ev, k, kernel_size, mistake=None):
    """the whole selection -> (flat indices [k] int64, coords [k,2] float32, the [w,h] map the top-k ran on)"""
    pick = lambda names: mistake if mistake in names else None
    s = nms(score(ev, pick(SCORE_MISTAKES)), kernel_size, pick(NMS_MISTAKES))
    idx = topk(s, k, pick(TOPK_MISTAKES))
    return idx, coords(idx, s.shape[1], pick(COORD_MISTAKES)), s


# ------------------------------------------------------------------------------------------------------------ event stacks
def by_cells(counts, bins, H, W, scale=1.0, leftover=7.0):
    """``counts`` [w,h] small non-negative integers -> events [bins,H,W]: that many events in the first pixel of the cell, bin
    0, so the cell's score is exactly count / 16 / bins (x ``scale``, a power of two).  Rows of H beyond 4 h hold
    ``leftover`` events per pixel: the selection must not see them."""
    counts = np.asarray(counts)
    w, h = counts.shape
    assert (h, w) == (H // 4, W // 4) and (counts >= 0).all() and (counts == np.round(counts)).all()
    ev = np.zeros((bins, H, W), np.float32)
    ev[0, 0:4 * h:4, 0:4 * w:4] = counts.T
    ev[:, 4 * h:] = leftover
    return ev * np.float32(scale)


def tied_counts(w, h, n_above, n_tied, seed, below=0):
    """[w,h] counts: ``n_above`` cells with the distinct counts t+1 .. t+n_above (shuffled) at the HIGHEST flat indices, n_tied
    cells with count t = below + 1 spread over all the indices under them, the other cells 0 (``below`` = 0) or 1 .. below
    drawn at random.  Top-k with n_above < k <= n_above + n_tied: the threshold is t"""
    rng = np.random.default_rng(seed)
    N = w * h
    t = below + 1
    flat = rng.integers(1, t, N) if below else np.zeros(N, np.int64)
    lo = N - n_above
    flat[rng.choice(lo, n_tied, replace=False)] = t
    flat[lo:] = t + 1 + rng.permutation(n_above)
    return flat.reshape(w, h)


def overflow_lds():
    """1 x 160 x 160, 1600 cells: 40 above the threshold at the highest indices, 1300 tied with it, 260 zero.  1340 cells >=
    the threshold are more than SEL_SLOTS; 1340 non-zero cells fit the LDS candidate list"""
    return by_cells(tied_counts(40, 40, 40, 1300, seed=101), 1, 160, 160)


def overflow_stream():
    """1 x 320 x 324, 6480 cells, none zero (> TOPK_CAP: the streaming passes): 40 above at the highest indices, all others tied"""
    return by_cells(tied_counts(81, 80, 40, 6440, seed=102), 1, 320, 324)


def cap_boundary(nnz):
    """the 6480-cell map with exactly ``nnz`` non-zero cells: 50 distinct counts above the threshold, 800 cells tied with it
    (850 < SEL_SLOTS: no overflow), the other non-zero cells at 1 .. 499, zeros scattered"""
    rng = np.random.default_rng(103)
    c = tied_counts(81, 80, 50, 800, seed=104, below=499).reshape(-1)
    low = np.flatnonzero(c < 500)
    c[rng.choice(low, c.size - nnz, replace=False)] = 0
    assert np.count_nonzero(c) == nnz
    return by_cells(c.reshape(81, 80), 1, 320, 324)


def ties_below_capacity():
    """5 x 96 x 128, 768 cells: 30 above the threshold, 200 tied with it, the rest 0 .. 2"""
    rng = np.random.default_rng(105)
    c = tied_counts(32, 24, 30, 200, seed=106, below=2).reshape(-1)
    low = np.flatnonzero(c < 3)
    c[rng.choice(low, 150, replace=False)] = 0
    return by_cells(c.reshape(32, 24), 5, 96, 128)


NMS_SHAPES = ((2, 132, 100), (3, 50, 68))        # h = 33, w = 25 (H % 4 == 0);  h = 12, w = 17 (H % 4 == 2)
NMS_SIZES = (0, 1, 3, 11, 17)


def plateau_map(shape, kernel_size):
    """events whose [w,h] count map holds, over a background of 0 .. 3: a maximum in each corner (9 .. 12: a window that wrapped would see a larger one); a 3 x 3 plateau (8);
    a plateau (8) across the 16-cell tile boundary of either axis the map reaches; and, r = the NMS radius, pairs of equal
    maxima (7) r and r + 1 cells apart and a 6 at r and at r + 1 cells from a 7 (the first is suppressed, the second kept).
    Features that do not fit the map are left out"""
    bins, H, W = shape
    h, w = H // 4, W // 4
    r = max(1, (kernel_size - 1) // 2)
    rng = np.random.default_rng(107 + kernel_size)
    c = rng.integers(0, 4, (w, h))

    def put(x, y, v):
        if 0 <= x < w and 0 <= y < h:
            c[x, y] = v
    for v, (x, y) in enumerate(((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))):
        put(x, y, 9 + v)
    for x in range(4, 7):
        for y in range(4, 7):
            put(x, y, 8)
    if w > 16:
        put(15, 9, 8), put(16, 9, 8)
    if h > 16:
        put(9, 15, 8), put(9, 16, 8)
    put(2, 8, 7), put(2 + r, 8, 7)                # equal, r apart along x: inside each other's window
    put(12, 2, 7), put(12, 2 + r + 1, 7)          # equal, r + 1 apart along y: outside
    put(2, 10, 6)                                 # r - 2 ... (2, 8) is 2 away: suppressed for r >= 2
    put(12 - r, 2, 6), put(12 + r + 1, 2, 6)      # r from a 7: suppressed;  r + 1 from it: the window does not reach
    return by_cells(c, bins, H, W)


def sparse_map(shape, seed, density=0.5):
    """counts 1 .. 6 in about ``density`` of the cells, 0 elsewhere"""
    bins, H, W = shape
    h, w = H // 4, W // 4
    rng = np.random.default_rng(seed)
    c = rng.integers(1, 7, (w, h)) * (rng.random((w, h)) < density)
    return by_cells(c, bins, H, W)


def subnormal_map(tied):
    """1 x 64 x 64 scaled by 2^-140: every score is count x 2^-144, exact and subnormal (top key byte 0).  ``tied``: 20 cells above the
    threshold, 100 tied with it, lower counts elsewhere; else 30 positive cells in all (fewer than k = 48)"""
    if tied:
        c = tied_counts(16, 16, 20, 100, seed=108, below=3)
    else:
        rng = np.random.default_rng(109)
        c = np.zeros(256, np.int64)
        c[rng.choice(256, 30, replace=False)] = rng.integers(1, 5, 30)
        c = c.reshape(16, 16)
    return by_cells(c, 1, 64, 64, scale=2.0 ** -140)


_BUILDERS = {
    "overflow_lds": overflow_lds, "overflow_stream": overflow_stream,
    "cap_6144": lambda: cap_boundary(TOPK_CAP), "cap_6145": lambda: cap_boundary(TOPK_CAP + 1),
    "ties_below_capacity": ties_below_capacity,
    "sparse_128": lambda: sparse_map((1, 128, 128), 111), "sparse_132": lambda: sparse_map((2, 132, 100), 112),
    "sparse_16": lambda: sparse_map((1, 16, 16), 113),
    "subnormal_tied": lambda: subnormal_map(True), "subnormal_few": lambda: subnormal_map(False),
}
for _shape in NMS_SHAPES:
    for _ks in NMS_SIZES:
        _BUILDERS["plateau_%dx%dx%d_nms%d" % (_shape + (_ks,))] = lambda s=_shape, k=_ks: plateau_map(s, k)
STACKS = tuple(_BUILDERS)
_built = {}


def stack(name):
    """the named event stack, built once and read-only"""
    if name not in _built:
        _built[name] = _BUILDERS[name]()
        _built[name].setflags(write=False)
    return _built[name]
