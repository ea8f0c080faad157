"""A numpy restatement of ramp_event_flow (include/ramp_hip.h, "event optical flow") that does NOT share the kernel's structure:
no sort by cell, no segments, no searches.  The candidates are put in time order with a stable argsort -- equal time stamps stay
in index order, filterref.py's ordering -- and ONE sweep over a surface-of-active-events map reads each event's window and then
writes its own entry.  The fit is a loop over the offsets j in ascending order; each statement is one IEEE float64 operation
on a vector that holds one element per event (numpy evaluates element by element, without FMA), so every output is exact.

``mistake=`` swaps one rule for a plausible wrong one (MISTAKES); tests/test_flowref_cpu.py shows that the test streams tell
each of them from the definition."""
import numpy as np

import filterref

BAD_ORDER = filterref.BAD_ORDER
TICK = filterref.STREAM_TICK
NAN = float("nan")
MISTAKES = ("dx_dy_exchanged", "window_wraps", "ties_by_le", "own_predecessor_is_centre", "ge_at_outlier_dt", "state_ignored",
            "polarity_not_split", "flow_is_a_b", "lt_at_window_dt", "descending_sums")


def _fit(S, used, r, min_points, mistake):
    """S [M, P] the points' s, used [M, P] bool -> (cls [M] in {4, 5, 7}, n [M], a, b, c [M]) by the header's formulas"""
    D = 2 * r + 1
    M = len(S)
    n, Sx, Sy, Sxx, Sxy, Syy = (np.zeros(M, np.int64) for _ in range(6))
    Sxs, Sys, Ss = np.zeros(M), np.zeros(M), np.zeros(M)
    js = range(D * D - 1, -1, -1) if mistake == "descending_sums" else range(D * D)
    for j in js:
        dy, dx = j // D - r, j % D - r
        if mistake == "dx_dy_exchanged":
            dx, dy = dy, dx
        u = used[:, j]
        s = np.where(u, S[:, j], 0.0)
        n, Sx, Sy, Sxx, Sxy, Syy = n + u, Sx + u * dx, Sy + u * dy, Sxx + u * dx * dx, Sxy + u * dx * dy, Syy + u * dy * dy
        with np.errstate(invalid="ignore"):
            Sxs = np.where(u, Sxs + float(dx) * s, Sxs)
            Sys = np.where(u, Sys + float(dy) * s, Sys)
            Ss = np.where(u, Ss + s, Ss)
    C00, C01, C02 = Syy * n - Sy * Sy, Sx * Sy - Sxy * n, Sxy * Sy - Syy * Sx
    C11, C12, C22 = Sxx * n - Sx * Sx, Sxy * Sx - Sxx * Sy, Sxx * Syy - Sxy * Sxy
    Det = Sxx * C00 + Sxy * C01 + Sx * C02
    cls = np.where(n < min_points, 4, np.where(Det == 0, 5, 7))
    f = lambda v: v.astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.where(cls == 7, f(Det), NAN)
        a = ((f(C00) * Sxs + f(C01) * Sys) + f(C02) * Ss) / d
        b = ((f(C01) * Sxs + f(C11) * Sys) + f(C12) * Ss) / d
        c = ((f(C02) * Sxs + f(C12) * Sys) + f(C22) * Ss) / d
    return cls, n, a, b, c, Det


def event_flow(x, y, t, H, W, p=None, radius=2, window_dt=None, min_points=5, refine=1, outlier_dt=None,
               max_speed=float("inf"), last_t=None, mistake=None, debug=False):
    """-> dict: flow float32 [N, 2], cls uint8 [N], n_used uint8 [N], fit float64 [N, 3], flow_map float32 [2, H, W], map_index
    int32 [H, W], last_t float64 [S, H, W] ([H, W] without p), status int32 [8]; ``debug``: also ``residual`` [N, P], the
    first pass's |s - plane| per point (NaN where there is none), and ``det`` [N]"""
    assert mistake is None or mistake in MISTAKES
    assert window_dt is not None
    r, D = radius, 2 * radius + 1
    P, centre = D * D, radius * D + radius
    outlier_dt = window_dt / 4 if outlier_dt is None else outlier_dt
    xf, yf = np.asarray(x).astype(np.float32).reshape(-1), np.asarray(y).astype(np.float32).reshape(-1)
    tf = np.asarray(t, np.float64).reshape(-1)
    N = len(tf)
    split = p is not None and mistake != "polarity_not_split"
    S = 2 if p is not None else 1
    shape = (H, W) if p is None else (2, H, W)
    state = np.full((S, H, W), NAN) if last_t is None else np.array(last_t, np.float64).reshape(S, H, W)
    status = np.zeros(8, np.int32)
    out = dict(flow=np.full((N, 2), NAN, np.float32), cls=np.zeros(N, np.uint8), n_used=np.zeros(N, np.uint8),
               fit=np.full((N, 3), NAN), flow_map=np.full((2, H, W), NAN, np.float32), map_index=np.full((H, W), -1, np.int32),
               last_t=state.reshape(shape).copy(), status=status)
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
    bad = False
    for q, ti in zip((plane * H * W + py * W + px).tolist(), tc.tolist()):
        if ti < seen[q]:
            bad = True
            break
        seen[q] = ti
    if bad:
        status[0] = BAD_ORDER
        out["last_t"][:] = NAN
        return out

    # the sweep, in time order (ties in index order), over a map with a border of r that never gives a point
    wraps = mistake == "window_wraps"
    Wp = W if wraps else W + 2 * r
    border = 0 if wraps else r
    m = np.full((S, H + 2 * r, Wp), NAN)
    if mistake != "state_ignored":
        m[:, r:r + H, border:border + W] = state
    rows = H + 2 * r
    sees = plane if split else np.zeros(len(cand), int)          # (not split: both polarities read and write plane 0)
    if p is not None and not split:
        m[0, r:r + H, border:border + W] = np.fmax(m[0, r:r + H, border:border + W], m[1, r:r + H, border:border + W])
    m = m.reshape(-1)
    cell = sees * rows * Wp + (py + r) * Wp + px + border
    offs = np.array([(j // D - r) * Wp + (j % D - r) for j in range(P)])
    order = np.argsort(tc, kind="stable")
    T = np.full((len(cand), P), NAN)                            # t_nb per candidate and offset
    oc, ot = cell[order].tolist(), tc[order].tolist()
    if mistake == "ties_by_le":                                  # every event with the same time stamp precedes, later ones too
        w = 0
        for k, c, ti in zip(order.tolist(), oc, ot):
            while w < len(oc) and ot[w] <= ti:
                m[oc[w]] = ot[w]
                w += 1
            T[k] = m[np.clip(c + offs, 0, len(m) - 1)]
    else:
        for k, c, ti in zip(order.tolist(), oc, ot):
            T[k] = m[np.clip(c + offs, 0, len(m) - 1)]           # (clip: only the wrapped window can leave the map)
            m[c] = ti
    final = m.reshape(S, rows, Wp)[:, r:r + H, border:border + W]

    with np.errstate(invalid="ignore"):
        delta = tc[:, None] - T                                  # one float64 subtraction
        used = (delta < window_dt) if mistake == "lt_at_window_dt" else (delta <= window_dt)
    Sv = -delta
    if mistake != "own_predecessor_is_centre":
        used[:, centre], Sv[:, centre] = True, 0.0
    Sv = np.where(used, Sv, NAN)
    k_cls, n, a, b, c, det = _fit(Sv, used, r, min_points, mistake)
    residual = None
    live = np.ones(len(cand), bool)                              # still refining
    for _ in range(refine):
        drop = np.zeros_like(used)
        for j in range(P):
            if j == centre:
                continue
            dy, dx = j // D - r, j % D - r
            with np.errstate(invalid="ignore"):
                res = np.abs(Sv[:, j] - ((a * float(dx) + b * float(dy)) + c))
                drop[:, j] = used[:, j] & ((res >= outlier_dt) if mistake == "ge_at_outlier_dt" else (res > outlier_dt))
        if residual is None:
            residual = np.full((len(cand), P), NAN)
            for j in range(P):
                dy, dx = j // D - r, j % D - r
                with np.errstate(invalid="ignore"):
                    residual[:, j] = np.where(used[:, j] & (j != centre), np.abs(Sv[:, j] - ((a * float(dx) + b * float(dy)) + c)), NAN)
        live &= (k_cls == 7) & drop.any(axis=1)
        if not live.any():
            break
        used2 = used & ~(drop & live[:, None])
        c2, n2, a2, b2, cc2, det2 = _fit(np.where(used2, Sv, NAN), used2, r, min_points, mistake)
        k_cls, n, a, b, c, det = (np.where(live, u, v) for u, v in ((c2, k_cls), (n2, n), (a2, a), (b2, b), (cc2, c), (det2, det)))
        used = used2
    with np.errstate(all="ignore"):
        g2 = a * a + b * b
        vx, vy = a / g2, b / g2
        flat = ~(g2 > 0) | ~np.isfinite(vx) | ~np.isfinite(vy) | (vx * vx + vy * vy > max_speed * max_speed)
    k_cls = np.where((k_cls == 7) & flat, 6, k_cls)
    valid = k_cls == 7
    if mistake == "flow_is_a_b":
        vx, vy = a, b
    cls[cand] = k_cls
    out["cls"] = cls.astype(np.uint8)
    out["n_used"][cand] = n.astype(np.uint8)
    formed = k_cls >= 6
    out["fit"][cand[formed]] = np.stack([a, b, c], 1)[formed]
    with np.errstate(over="ignore"):
        out["flow"][cand[valid]] = np.stack([vx, vy], 1)[valid].astype(np.float32)
    for w_ in (4, 5, 6, 7):
        status[w_] = int((cls == w_).sum())
    for i, qx, qy in zip(cand[valid].tolist(), px[valid].tolist(), py[valid].tolist()):      # ascending index: the largest wins
        out["map_index"][qy, qx] = i
    at = out["map_index"] >= 0
    out["flow_map"][:, at] = out["flow"][out["map_index"][at]].T
    if split or p is None:
        out["last_t"] = final.reshape(shape).copy()
    else:                                                        # (the mistake's one plane, reported on both)
        out["last_t"] = np.stack([final[0], final[0]])
    if debug:
        full = np.full((N, P), NAN)
        if residual is not None:
            full[cand] = residual
        out["residual"] = full
        out["det"] = np.zeros(N, np.int64)
        out["det"][cand] = det
    return out


# ------------------------------------------------------------------------------------------------ test streams
def edge(H, W, speed_inv=4, diagonal=False, probe=None):
    """every pixel fires once: column x at t = x / speed_inv (``diagonal``: t = (x + y) / (2 speed_inv)), in time order; among
    equal time stamps the pixel ``probe`` = (x, y) comes last, so that every pixel of its window that fires with it precedes
    it.  The time stamps are dyadic, so the probe's fit is exact: a = 1 / speed_inv, b = 0 (a = b = 1 / (2 speed_inv))"""
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    t = (xs + ys) / (2.0 * speed_inv) if diagonal else xs / float(speed_inv)
    is_probe = np.zeros(len(t), bool) if probe is None else (xs == probe[0]) & (ys == probe[1])
    order = np.lexsort((is_probe, t))
    return xs[order].astype(np.int32), ys[order].astype(np.int32), t[order]


STREAM_PARAMS = dict(window_dt=1024 * TICK, outlier_dt=192 * TICK)


def stream(N, seed=3, H=13, W=17, tick=TICK):
    """A time-sorted test stream of N events on an H x W sensor with polarity, made to exercise classes [4] to [7] under
    STREAM_PARAMS: two edges that sweep across the sensor in opposite directions (one per polarity, a share of their events
    late: outliers for the refinement), uniform noise, and a quiet first stretch (too few points).  Half of the time stamps
    lie on a grid of ``tick`` -- equal stamps occur and differences hit ``window_dt`` exactly --, the rest are arbitrary
    doubles, so that the order of the sums shows in the last bit.  -> x, y float32 [N], t float64 [N] (sorted), p int8 [N]"""
    rng = np.random.default_rng(seed)
    T = 2.5e-4 * N                                               # ~ 18 events per pixel and second at 13 x 17
    n_noise = N * 20 // 100
    n_edge = N - n_noise
    te = rng.uniform(0, T, n_edge)
    lane = rng.integers(0, 2, n_edge)
    ph = (te / (W * 340 * tick)) % 1.0                           # an edge moves a pixel in a third of window_dt
    xe = np.where(lane == 0, ph * W, W * (1 - ph)) + rng.normal(0, 0.3, n_edge)
    ye = rng.uniform(0, H, n_edge)
    late = rng.random(n_edge) < 0.06
    te = te + late * rng.uniform(250, 800, n_edge) * tick
    pe = np.where(lane == 0, 1, -1)
    xs = np.concatenate([xe, rng.uniform(0, W, n_noise)])
    ys = np.concatenate([ye, rng.uniform(0, H, n_noise)])
    ts = np.concatenate([te, rng.uniform(0, T, n_noise)])
    ps = np.concatenate([pe, rng.choice([-1, 1], n_noise)])
    xs, ys = np.clip(xs, 0, W - 0.01), np.clip(ys, 0, H - 0.01)
    grid = rng.random(N) < 0.5
    ts = np.where(grid, np.round(ts / tick) * tick, ts)
    order = np.argsort(ts, kind="stable")
    return xs[order].astype(np.float32), ys[order].astype(np.float32), ts[order], ps[order].astype(np.int8)


def shuffle_keeping_cells(x, y, p, rng):
    """a permutation of the events that keeps every cell's (plane, pixel) own events in their order"""
    cellkey = (np.asarray(p) > 0).astype(int) * 1000000 + np.trunc(y).astype(int) * 1000 + np.trunc(x).astype(int)
    slots = rng.permutation(len(x))
    perm = np.empty(len(x), int)
    for q in np.unique(cellkey):
        at = np.nonzero(cellkey == q)[0]
        perm[np.sort(slots[at])] = at
    return perm
