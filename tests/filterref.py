"""A numpy restatement of ramp_event_filter (include/ramp_hip.h, "event denoising") that does NOT share the kernel's structure:
no sort by pixel, no segments, no searches.  The candidates are put in time order with a stable argsort -- equal time stamps
stay in index order -- and the TEXTBOOK filter sweeps them once over a last-time-stamp map: test the own pixel's entry, test the
eight neighbours' entries, write the own entry.  All arithmetic is IEEE float64 on Python floats (one subtraction, one
comparison per test; no FMA anywhere), so every output is exact, not approximate.

``mistake=`` swaps one rule for a plausible wrong one (MISTAKES); tests/test_filterref_cpu.py shows that the test streams tell
each of them from the definition."""
import math

import numpy as np

BAD_ORDER = 1
MISTAKES = ("own_pixel_supports", "lt_at_support_dt", "le_at_refractory", "hot_pixels_support", "four_neighbours",
            "later_events_support", "refractory_drops_skip_the_map", "ties_by_larger_index", "sample_variance", "hot_in_ignored")
NAN = float("nan")


def hot_rule(c, hot_count=0, hot_sigma=0.0, hot_mask=None, mistake=None):
    """counts [H, W] -> (hot [H, W] uint8, stats float64 [4]: n, mean, std, thr), the formula of the header in its order"""
    n = int(np.count_nonzero(c))
    S1 = int(c.astype(np.int64).sum())
    S2 = int((c.astype(np.int64) ** 2).sum())
    mean = sd = thr = NAN
    if n > 0:
        mean = float(S1) / float(n)
        v = float(S2) / float(n) - mean * mean
        if mistake == "sample_variance":
            v = v * float(n) / float(n - 1) if n > 1 else NAN
        sd = math.sqrt(v if v > 0.0 else 0.0)
        if hot_sigma > 0.0:
            thr = mean + hot_sigma * sd
    hot = np.zeros(c.shape, bool)
    if hot_count > 0:
        hot |= c > hot_count
    if hot_sigma > 0.0 and n > 0:
        hot |= c.astype(np.float64) > thr
    if hot_mask is not None and mistake != "hot_in_ignored":
        hot |= np.asarray(hot_mask) != 0
    return hot.astype(np.uint8), np.array([float(n), mean, sd, thr], np.float64)


def event_filter(x, y, t, H, W, support_dt=None, refractory=0.0, hot_count=0, hot_sigma=0.0, hot_mask=None, last_t=None,
                 mistake=None):
    """-> dict: keep uint8 [N], cls int [N] (2 .. 7), xy float32 [N, 2], index int32 [N], count, hot uint8 [H, W], stats
    float64 [4], last_t float64 [H, W], status int32 [8]"""
    assert mistake is None or mistake in MISTAKES
    xf, yf = np.asarray(x).astype(np.float32).reshape(-1), np.asarray(y).astype(np.float32).reshape(-1)
    tf = np.asarray(t, np.float64).reshape(-1)
    N = len(tf)
    state = np.full((H, W), NAN) if last_t is None else np.array(last_t, np.float64).reshape(H, W)
    status = np.zeros(8, np.int32)
    if N == 0:
        hot = np.zeros((H, W), np.uint8) if hot_mask is None else (np.asarray(hot_mask) != 0).astype(np.uint8)
        return dict(keep=np.zeros(0, np.uint8), cls=np.zeros(0, int), xy=np.zeros((0, 2), np.float32), index=np.zeros(0, np.int32),
                    count=0, hot=hot, stats=np.array([0.0, NAN, NAN, NAN]), last_t=state, status=status)
    cls = np.zeros(N, int)
    finite = np.isfinite(xf) & np.isfinite(yf) & np.isfinite(tf)
    cls[~finite] = 2
    with np.errstate(invalid="ignore"):
        xt, yt = np.trunc(xf), np.trunc(yf)
        inside = finite & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
    cls[finite & ~inside] = 3
    cand = np.nonzero(inside)[0]
    px, py = xt[cand].astype(int), yt[cand].astype(int)
    counts = np.bincount(py * W + px, minlength=H * W).reshape(H, W)
    hot, stats = hot_rule(counts, hot_count, hot_sigma, hot_mask, mistake)

    # the order the call requires: per pixel, in index order, the time stamps do not decrease and do not lie before the state
    seen = state.reshape(-1).tolist()
    bad = False
    for q, ti in zip((py * W + px).tolist(), tf[cand].tolist()):
        if ti < seen[q]:
            bad = True
            break
        seen[q] = ti

    # the textbook sweep, in time order (ties in index order), over a map with a one-pixel border that never gives support
    Wp = W + 2
    hot_supports = mistake == "hot_pixels_support"
    m = np.full((H + 2, Wp), NAN)
    m[1:-1, 1:-1] = state if hot_supports else np.where(hot != 0, NAN, state)
    m = m.reshape(-1).tolist()
    tc = tf[cand]
    if mistake == "ties_by_larger_index":
        order = np.lexsort((-np.arange(len(cand)), tc))
    else:
        order = np.argsort(tc, kind="stable")
    cell = ((py + 1) * Wp + px + 1)
    ishot = hot[py, px] != 0
    nbrs = (-Wp, -1, 1, Wp) if mistake == "four_neighbours" else (-Wp - 1, -Wp, -Wp + 1, -1, 1, Wp - 1, Wp, Wp + 1)
    if mistake == "own_pixel_supports":
        nbrs = nbrs + (0,)
    act = support_dt is not None and support_dt >= 0
    out = [0] * len(cand)
    for k, c, ti, h in zip(order.tolist(), cell[order].tolist(), tc[order].tolist(), ishot[order].tolist()):
        if h:
            out[k] = 4
            if hot_supports:
                m[c] = ti
            continue
        d = ti - m[c]
        if refractory > 0 and (d <= refractory if mistake == "le_at_refractory" else d < refractory):
            out[k] = 5
            if mistake != "refractory_drops_skip_the_map":
                m[c] = ti
            continue
        if act:
            sup = False
            for o in nbrs:
                d = ti - m[c + o]
                if d < support_dt if mistake == "lt_at_support_dt" else d <= support_dt:
                    sup = True
                    break
            out[k] = 7 if sup else 6
        else:
            out[k] = 7
        m[c] = ti
    if mistake == "later_events_support" and act:                # a second sweep, backwards: the NEXT event of a neighbour counts too
        nxt = [NAN] * len(m)
        for k, c, ti, h in zip(order[::-1].tolist(), cell[order[::-1]].tolist(), tc[order[::-1]].tolist(), ishot[order[::-1]].tolist()):
            if h:
                continue
            if out[k] == 6 and any(nxt[c + o] - ti <= support_dt for o in nbrs):
                out[k] = 7
            nxt[c] = ti
    cls[cand] = out
    final = np.array(m).reshape(H + 2, Wp)[1:-1, 1:-1]
    final = np.where(hot != 0, state, final)                     # a hot pixel does not touch the state

    status[1] = N
    for w in (2, 3):
        status[w] = int((cls == w).sum())
    xy = np.full((N, 2), NAN, np.float32)
    index = np.full(N, -1, np.int32)
    if bad:
        status[0] = BAD_ORDER
        cls[cand] = 0
        return dict(keep=np.zeros(N, np.uint8), cls=cls, xy=xy, index=index, count=0, hot=hot, stats=np.full(4, NAN),
                    last_t=np.full((H, W), NAN), status=status)
    for w in (4, 5, 6, 7):
        status[w] = int((cls == w).sum())
    keep = (cls == 7).astype(np.uint8)
    kept = np.nonzero(keep)[0]
    xy[kept, 0], xy[kept, 1] = xf[kept], yf[kept]
    index[:len(kept)] = kept
    return dict(keep=keep, cls=cls, xy=xy, index=index, count=len(kept), hot=hot, stats=stats, last_t=final, status=status)


# ------------------------------------------------------------------------------------------------ test streams
STREAM_TICK = 2.0 ** -14          # the streams' time grid: a power of two, so that differences of stamps are exact
STREAM_PARAMS = dict(support_dt=32 * STREAM_TICK, refractory=6 * STREAM_TICK, hot_sigma=2.5)


def stream(N, seed=3, H=13, W=17, hot_pixels=3, tick=STREAM_TICK):
    """A time-sorted test stream of N events on an H x W sensor, made to exercise every class under STREAM_PARAMS: two moving
    edges (columns of events that sweep across the sensor, a part of them doubled within the refractory period), uniform
    noise, and a few hot pixels.  The time stamps lie on a grid of ``tick``, so that equal stamps occur and differences hit
    ``support_dt`` and ``refractory`` exactly; the coordinates carry a fraction.  -> x, y float32 [N], t float64 [N] (sorted)"""
    rng = np.random.default_rng(seed)
    T = 2.5e-4 * N                                               # ~ 18 events per pixel and second at 13 x 17
    n_hot = N * 12 // 100
    n_noise = N * 22 // 100
    n_edge = N - n_hot - n_noise
    n_first = int(n_edge / 1.25)
    te = rng.uniform(0, T, n_first)
    lane = rng.integers(0, 2, n_first)
    xe = np.where(lane == 0, (te / T) * (W - 1), (W - 1) * (1 - te / T)) + rng.normal(0, 0.35, n_first)
    ye = rng.uniform(0, H, n_first)
    twice = rng.choice(n_first, n_edge - n_first, replace=False)                       # doubled: the refractory period's share
    te = np.concatenate([te, te[twice] + rng.uniform(0.2, 1.6, len(twice)) * STREAM_PARAMS["refractory"]])
    xe, ye = np.concatenate([xe, xe[twice]]), np.concatenate([ye, ye[twice]])
    spots = rng.choice(H * W, hot_pixels, replace=False)
    hp = rng.choice(spots, n_hot)
    xs = np.concatenate([xe, rng.uniform(0, W, n_noise), hp % W + 0.25])
    ys = np.concatenate([ye, rng.uniform(0, H, n_noise), hp // W + 0.5])
    ts = np.concatenate([te, rng.uniform(0, T, n_noise), rng.uniform(0, T, n_hot)])
    xs, ys = np.clip(xs, 0, W - 0.01), np.clip(ys, 0, H - 0.01)
    ts = np.round(ts / tick) * tick
    order = np.argsort(ts, kind="stable")
    return xs[order].astype(np.float32), ys[order].astype(np.float32), ts[order]


def shuffle_keeping_pixels(x, y, rng):
    """a permutation of the events that keeps every pixel's own events in their order"""
    pix = np.trunc(y).astype(int) * 1000 + np.trunc(x).astype(int)
    slots = rng.permutation(len(x))
    perm = np.empty(len(x), int)
    for q in np.unique(pix):
        at = np.nonzero(pix == q)[0]
        perm[np.sort(slots[at])] = at
    return perm
