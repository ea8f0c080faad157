"""A numpy restatement of ramp_event_corners (include/ramp_hip.h, "event corner detection") that does NOT share the kernel's
structure: no sort by cell, no segments, no searches, no threshold sets.  The candidates are put in time order with a stable
argsort -- equal time stamps stay in index order, flowref.py's ordering -- and ONE sweep over a surface-of-active-events map
reads each event's two circles and then writes its own entry.  The arcs are tested by brute force: every (start, L) of an
allowed length, "the smallest value on the arc is above the largest value off it", the shortest passing arc reported.  Only
comparisons of time stamps: every output is exact.

``mistake=`` swaps one rule for a plausible wrong one (MISTAKES); tests/test_cornerref_cpu.py shows that the test streams tell
each of them from the definition."""
import numpy as np

import filterref

BAD_ORDER = filterref.BAD_ORDER
TICK = 1.0 / 1024
NAN = float("nan")
INNER = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
         (-2, 2), (-1, 3))
OUTER = ((0, 4), (1, 4), (2, 3), (3, 2), (4, 1), (4, 0), (4, -1), (3, -2), (2, -3), (1, -4), (0, -4), (-1, -4), (-2, -3), (-3, -2),
         (-4, -1), (-4, 0), (-4, 1), (-3, 2), (-2, 3), (-1, 4))
PAD = 4
MISTAKES = ("circle_reversed", "ties_by_ge", "own_predecessor_read", "state_ignored", "polarity_not_split", "border_3",
            "inner_hi_7", "outer_skipped", "no_wraparound", "nan_is_zero", "largest_L_reported", "wide_always")


def lengths(n, lo, hi, wide):
    """the allowed arc lengths of a circle of n pixels, ascending"""
    return [L for L in range(1, n) if lo <= L <= hi or (wide and lo <= n - L <= hi)]


def arcs(V, lo, hi, wide, own=None, mistake=None):
    """V [M, n] the circle's values (NaN: none) -> (start [M], L [M]) of the reported arc, L = 0 where no arc passes.
    ``own`` [M]: only the mistake that reads the event's own predecessor looks at it"""
    M, n = V.shape
    if mistake == "nan_is_zero":
        V = np.where(np.isnan(V), 0.0, V)
    isnan = np.isnan(V)
    Vn = np.where(isnan, -np.inf, V)
    start, length = np.zeros(M, np.int64), np.zeros(M, np.int64)
    for L in lengths(n, lo, hi, wide):
        for s in range(n):
            if mistake == "no_wraparound" and s + L > n:
                continue
            on = [(s + k) % n for k in range(L)]
            off = [k for k in range(n) if k not in on]
            on_min, off_max = Vn[:, on].min(axis=1), Vn[:, off].max(axis=1)
            if mistake == "own_predecessor_read":
                off_max = np.fmax(off_max, own)
                none_off = isnan[:, off].all(axis=1) & np.isnan(own)
            else:
                none_off = isnan[:, off].all(axis=1)           # (a NaN is below every number, -inf included)
            above = (on_min >= off_max) if mistake == "ties_by_ge" else (on_min > off_max)
            ok = ~isnan[:, on].any(axis=1) & (above | none_off)
            take = ok if mistake == "largest_L_reported" else ok & (length == 0)
            start[take], length[take] = s, L
    return start, length


def event_corners(x, y, t, H, W, p=None, inner=(3, 6), outer=(4, 8), wide=False, last_t=None, mistake=None):
    """-> dict: cls uint8 [N], arc uint8 [N, 4], index int32 [N], count int32 [1], corner_count int32 [H, W], last_t float64
    [S, H, W] ([H, W] without p), status int32 [8]"""
    assert mistake is None or mistake in MISTAKES
    for n, (lo, hi) in ((16, inner), (20, outer)):
        assert 1 <= lo <= hi <= n - 1
    if mistake == "inner_hi_7":
        inner = (inner[0], inner[1] + 1)
    if mistake == "wide_always":
        wide = True
    xf, yf = np.asarray(x).astype(np.float32).reshape(-1), np.asarray(y).astype(np.float32).reshape(-1)
    tf = np.asarray(t, np.float64).reshape(-1)
    N = len(tf)
    split = p is not None and mistake != "polarity_not_split"
    S = 2 if p is not None else 1
    shape = (H, W) if p is None else (2, H, W)
    state = np.full((S, H, W), NAN) if last_t is None else np.array(last_t, np.float64).reshape(S, H, W)
    status = np.zeros(8, np.int32)
    out = dict(cls=np.zeros(N, np.uint8), arc=np.zeros((N, 4), np.uint8), index=np.full(N, -1, np.int32), count=np.zeros(1, np.int32),
               corner_count=np.zeros((H, W), np.int32), last_t=state.reshape(shape).copy(), status=status)
    if N == 0:
        return out
    finite = np.isfinite(xf) & np.isfinite(yf) & np.isfinite(tf)
    with np.errstate(invalid="ignore"):
        xt, yt = np.trunc(xf), np.trunc(yf)
        inside = finite & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
    cls = np.zeros(N, int)
    cls[~finite], cls[finite & ~inside] = 2, 3
    cand = np.nonzero(inside)[0]
    px, py = xt[cand].astype(int), yt[cand].astype(int)
    plane = (np.asarray(p).reshape(-1)[cand] > 0).astype(int) if p is not None else np.zeros(len(cand), int)
    tc = tf[cand]
    status[1], status[2], status[3] = N, int((cls == 2).sum()), int((cls == 3).sum())

    # the order the call requires: per cell, in index order, the time stamps do not decrease and do not lie before the state
    seen = state.reshape(-1).tolist()
    for q, ti in zip((plane * H * W + py * W + px).tolist(), tc.tolist()):
        if ti < seen[q]:
            status[0] = BAD_ORDER
            out["last_t"][:] = NAN
            return out
        seen[q] = ti

    # the sweep, in time order (ties in index order), over a map with a border of PAD that holds nothing
    rows, Wp = H + 2 * PAD, W + 2 * PAD
    m = np.full((S, rows, Wp), NAN)
    if mistake != "state_ignored":
        m[:, PAD:PAD + H, PAD:PAD + W] = state
    sees = plane if split else np.zeros(len(cand), int)          # (not split: both polarities read and write plane 0)
    if p is not None and not split:
        m[0] = np.fmax(m[0], m[1])
    m = m.reshape(-1)
    cell = sees * rows * Wp + (py + PAD) * Wp + px + PAD
    rings = [list(reversed(c)) if mistake == "circle_reversed" else list(c) for c in (INNER, OUTER)]
    offs = np.array([dy * Wp + dx for c in rings for dx, dy in c] + [0])
    order = np.argsort(tc, kind="stable")
    V = np.full((len(cand), 37), NAN)                            # the inner circle, the outer circle, the own predecessor
    for k, c, ti in zip(order.tolist(), cell[order].tolist(), tc[order].tolist()):
        V[k] = m[c + offs]
        m[c] = ti
    final = m.reshape(S, rows, Wp)[:, PAD:PAD + H, PAD:PAD + W]

    b = 3 if mistake == "border_3" else 4
    border = (px < b) | (py < b) | (px > W - 1 - b) | (py > H - 1 - b)
    k_cls = np.where(border, 4, 5)
    arc = np.zeros((len(cand), 4), np.int64)
    live = np.nonzero(~border)[0]
    s_in, l_in = arcs(V[live, :16], inner[0], inner[1], wide, V[live, 36], mistake)
    hit = l_in > 0
    arc[live[hit], 0], arc[live[hit], 1] = s_in[hit], l_in[hit]
    live = live[hit]
    if mistake == "outer_skipped":
        k_cls[live] = 7
    else:
        s_out, l_out = arcs(V[live, 16:36], outer[0], outer[1], wide, V[live, 36], mistake)
        hit = l_out > 0
        k_cls[live] = np.where(hit, 7, 6)
        arc[live[hit], 2], arc[live[hit], 3] = s_out[hit], l_out[hit]
    cls[cand] = k_cls
    out["cls"] = cls.astype(np.uint8)
    out["arc"][cand] = arc.astype(np.uint8)
    for w_ in (4, 5, 6, 7):
        status[w_] = int((cls == w_).sum())
    corners = np.nonzero(cls == 7)[0]
    out["index"][:len(corners)] = corners
    out["count"][0] = len(corners)
    at = k_cls == 7
    np.add.at(out["corner_count"], (py[at], px[at]), 1)
    if split or p is None:
        out["last_t"] = final.reshape(shape).copy()
    else:                                                        # (the mistake's one plane, reported on both)
        out["last_t"] = np.stack([final[0], final[0]])
    return out


# ------------------------------------------------------------------------------------------------ closed forms
def painted(H, W, centre, inner=None, outer=None, on=2.0, rest=1.0):
    """a state with the two circles around ``centre`` = (x, y) painted: the arc (start, L) of each circle ``on``, the circle's
    other pixels ``rest`` (either may be NaN), everything else NaN; a circle given as None is left NaN"""
    s = np.full((H, W), NAN)
    for ring, a in ((INNER, inner), (OUTER, outer)):
        if a is None:
            continue
        n = len(ring)
        arc_k = {(a[0] + j) % n for j in range(a[1])}
        for k, (dx, dy) in enumerate(ring):
            s[centre[1] + dy, centre[0] + dx] = on if k in arc_k else rest
    return s


# ------------------------------------------------------------------------------------------------ test streams
H0, W0 = 33, 37
DIRECTIONS = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.7071, 0.7071), (0.6, -0.8))
SLOPES = (1.0, 0.5)


def wedge(d, h, H=H0, W=W0, steps=20, t0=0.0):
    """An apex moves along the unit direction ``d`` = (dx, dy) through the sensor's centre, ``steps`` steps of one pixel, half of
    them before the centre; the wedge {u <= 0, |v| <= h |u|} trails it (u along d, v across, from the apex).  Every pixel newly
    covered at step s >= 1 fires once at t = t0 + s / 1024, in raster order; the polarity alternates by step.
    -> x, y int32, t float64 (sorted), p int8"""
    ys, xs = np.mgrid[0:H, 0:W]
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0

    def covered(s):
        ax, ay = cx + (s - steps / 2.0) * d[0], cy + (s - steps / 2.0) * d[1]
        u = (xs - ax) * d[0] + (ys - ay) * d[1]
        v = -(xs - ax) * d[1] + (ys - ay) * d[0]
        return (u <= 0) & (np.abs(v) <= h * np.abs(u))

    x, y, t, p = [], [], [], []
    before = covered(0)
    for s in range(1, steps + 1):
        now = covered(s) | before
        qy, qx = np.nonzero(now & ~before)                       # (raster order)
        x.append(qx), y.append(qy), t.append(np.full(len(qx), t0 + s * TICK)), p.append(np.full(len(qx), 1 if s % 2 else -1))
        before = now
    return np.concatenate(x).astype(np.int32), np.concatenate(y).astype(np.int32), np.concatenate(t), np.concatenate(p).astype(np.int8)


def wedges(t0=0.0):
    """every (direction, slope) of the test set: (name, x, y, t, p)"""
    return [("d=%s h=%s" % (d, h),) + wedge(d, h, t0=t0) for d in DIRECTIONS for h in SLOPES]


def noise(N, seed=3, H=H0, W=W0, T=1.0):
    """uniform noise, time-sorted, on the tick grid (equal stamps occur) -> x, y float32, t, p"""
    rng = np.random.default_rng(seed)
    t = np.sort(np.round(rng.uniform(0, T, N) / (TICK / 8)) * (TICK / 8))
    return (rng.uniform(0, W, N).astype(np.float32), rng.uniform(0, H, N).astype(np.float32), t, rng.choice([-1, 1], N).astype(np.int8))


def stream(N, seed=3, H=H0, W=W0, distinct=False):
    """A time-sorted stream of N events: half of them wedge runs one after another (32 ticks apart, the set of wedges() cycled,
    each run on the surface its predecessors leave and of one polarity, so that both planes hold corners), half uniform noise
    over the same stretch.  The first run starts below
    t = 0, so that time stamps of either sign and 0 occur.  ``distinct``: every time stamp is made unique by an exact dyadic
    offset per event, so that no order across cells is left to the index.  -> x, y float32, t float64, p int8"""
    runs, n, k = [], 0, 0
    protos = [wedge(d, h, H, W) for d in DIRECTIONS for h in SLOPES]
    while n < N // 2:
        x, y, t, p = protos[k % len(protos)]
        runs.append((x, y, t + (32 * k - 12) * TICK, np.full(len(x), 1 if k % 2 else -1)))     # (one polarity per run)
        n, k = n + len(x), k + 1
    xs, ys, ts, ps = (np.concatenate([r[j] for r in runs])[:N // 2] for j in range(4)) if runs else (np.zeros(0),) * 4
    nx, ny, nt, npol = noise(N - len(xs), seed, H, W, T=max(32 * k, 1) * TICK)
    xs, ys = np.concatenate([xs.astype(np.float32) + 0.25, nx]), np.concatenate([ys.astype(np.float32) + 0.5, ny])
    ts, ps = np.concatenate([ts, nt - 12 * TICK]), np.concatenate([ps, npol])
    order = np.argsort(ts, kind="stable")
    xs, ys, ts, ps = xs[order].astype(np.float32), ys[order].astype(np.float32), ts[order], ps[order].astype(np.int8)
    if distinct:
        ts = ts + np.arange(len(ts)) * 2.0 ** -36
    return xs, ys, ts, ps


def shuffle_keeping_cells(x, y, p, rng):
    """a permutation of the events that keeps every cell's (plane, pixel) own events in their order"""
    cellkey = (np.asarray(p) > 0).astype(int) * 1000000 + np.trunc(y).astype(int) * 1000 + np.trunc(x).astype(int)
    slots = rng.permutation(len(x))
    perm = np.empty(len(x), int)
    for q in np.unique(cellkey):
        at = np.nonzero(cellkey == q)[0]
        perm[np.sort(slots[at])] = at
    return perm
