"""A numpy restatement of ramp_event_corner_tracks (include/ramp_hip.h, "event corner tracks") that does NOT share the
kernel's structure: no sort by cell, no segments, no searches, no pointer jumping.  The candidates are put in (t, i) order with
a stable argsort and swept ONCE over a per-cell record map (time stamp and source: an event of this call or the state); the
sweep reads each event's window as the definition reads it -- ascending j, the clipped cells holding nothing -- and then writes
the event's own cell.  The choice of the parent is written out over those windows, and the track quantities are handed down
in the same (t, i) order: a parent precedes its child, so it is complete when the child arrives.

``mistake=`` swaps one rule for a plausible wrong one (MISTAKES); tests/test_trackref_cpu.py shows that the streams of the GPU
test tell each of them from the definition."""
import numpy as np

import cornerref
import filterref

BAD_ORDER = filterref.BAD_ORDER
TICK = cornerref.TICK
NAN = float("nan")
PAD = 5                                                        # the largest radius
LEN_MAX = 2 ** 31 - 1
H0, W0 = cornerref.H0, cornerref.W0
MISTAKES = ("nearest_first", "ties_by_highest_j", "lt_for_le_max_dt", "window_not_clipped", "own_pixel_left_out", "planes_mixed",
            "id_from_sorted_position", "length_not_carried", "birth_of_parent", "non_candidates_overwrite_state")
KEYS = ("cls", "parent", "track", "length", "birth", "velocity", "state", "next_id", "status")


def empty_state(H, W, planes=1):
    s = np.zeros((planes, H, W, 4), np.int64)
    s[..., 0] = np.array(NAN).view(np.int64)
    return s if planes == 2 else s[0]


def pack_state(t, track, t0, x0, y0, length, W):
    """arrays of one shape -> the state words, a last axis of 4"""
    s = np.zeros(np.shape(t) + (4,), np.int64)
    s[..., 0], s[..., 1] = np.asarray(t, np.float64).view(np.int64), track
    s[..., 2] = np.asarray(t0, np.float64).view(np.int64)
    s[..., 3] = (np.asarray(length, np.int64) << 32) | (np.asarray(y0, np.int64) * W + np.asarray(x0, np.int64))
    return s


def unpack_state(state, W):
    """the state words -> dict t, track, t0, x0, y0, length"""
    state = np.asarray(state, np.int64)
    pix = state[..., 3] & 0xFFFFFFFF
    return dict(t=state[..., 0].copy().view(np.float64), track=state[..., 1].copy(), t0=state[..., 2].copy().view(np.float64),
                x0=(pix % W).astype(np.int64), y0=(pix // W).astype(np.int64), length=(state[..., 3] >> 32).astype(np.int32))


def event_corner_tracks(x, y, t, H, W, corner=None, p=None, radius=3, max_dt=None, state=None, next_id=0, mistake=None):
    """-> dict: cls uint8 [N], parent int32 [N], track int64 [N], length int32 [N], birth float64 [N, 3], velocity float32
    [N, 2], state int64 [S, H, W, 4] ([H, W, 4] without p), next_id int64 [1], status int32 [8]"""
    assert mistake is None or mistake in MISTAKES
    assert 0 <= radius <= 5 and max_dt is not None and max_dt >= 0
    xf, yf = np.asarray(x).astype(np.float32).reshape(-1), np.asarray(y).astype(np.float32).reshape(-1)
    tf = np.asarray(t, np.float64).reshape(-1)
    N, S = len(tf), 2 if p is not None else 1
    shape = (H, W, 4) if p is None else (2, H, W, 4)
    state_in = (empty_state(H, W, 2).reshape(2, H, W, 4)[:S] if state is None else np.array(state, np.int64).reshape(S, H, W, 4))
    status = np.zeros(8, np.int32)
    out = dict(cls=np.zeros(N, np.uint8), parent=np.full(N, -1, np.int32), track=np.full(N, -1, np.int64), length=np.zeros(N, np.int32),
               birth=np.full((N, 3), NAN), velocity=np.full((N, 2), NAN, np.float32), state=state_in.reshape(shape).copy(),
               next_id=np.array([next_id + N], np.int64), status=status)
    if N == 0:
        return out
    finite = np.isfinite(xf) & np.isfinite(yf) & np.isfinite(tf)
    with np.errstate(invalid="ignore"):
        xt, yt = np.trunc(xf), np.trunc(yf)
        inside = finite & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
    marked = np.ones(N, bool) if corner is None else np.asarray(corner).reshape(-1) != 0
    cls = np.zeros(N, int)
    cls[~finite], cls[finite & ~inside], cls[inside & ~marked] = 2, 3, 4
    status[1:5] = N, (cls == 2).sum(), (cls == 3).sum(), (cls == 4).sum()
    cand = np.nonzero(inside & marked)[0]
    px, py, tc = xt[cand].astype(int), yt[cand].astype(int), tf[cand]
    plane = (np.asarray(p).reshape(-1)[cand] > 0).astype(int) if p is not None else np.zeros(len(cand), int)
    rec = unpack_state(state_in, W)

    # the order the call requires: per cell, in index order, the time stamps do not decrease and do not lie before the state
    seen = rec["t"].reshape(-1).tolist()
    for q, ti in zip((plane * H * W + py * W + px).tolist(), tc.tolist()):
        if ti < seen[q]:
            status[0], status[4] = BAD_ORDER, 0                    # (words [4] .. [7] are 0)
            out["state"] = empty_state(H, W, S).reshape(shape)
            return out
        seen[q] = ti

    # the sweep, in (t, i) order, over a map with a border of PAD that holds nothing: per cell the time stamp of the last
    # candidate so far, else the state's, and its source (>= 0: a candidate's number, -2: the state)
    YP = PAD + 1                                                    # (one row more: the one mistake's windows run on in x)
    rows = H + 2 * YP
    Wp = W if mistake == "window_not_clipped" else W + 2 * PAD       # (the mistake: a window runs on into the neighbouring row)
    x_off = 0 if mistake == "window_not_clipped" else PAD
    mt = np.full((S, rows, Wp), NAN)
    mt[:, YP:YP + H, x_off:x_off + W] = rec["t"]
    msrc = np.full((S, rows, Wp), -2, np.int64)
    mt, msrc = mt.reshape(-1), msrc.reshape(-1)
    cell = plane * rows * Wp + (py + YP) * Wp + px + x_off
    r = radius
    window = [(dx, dy) for dy in range(-r, r + 1) for dx in range(-r, r + 1)]                    # ascending j
    offs = np.array([dy * Wp + dx for dx, dy in window])
    d2 = np.array([dx * dx + dy * dy for dx, dy in window])
    if mistake == "planes_mixed" and S == 2:                        # both planes' cells in every window, plane 0 first per j
        lo = np.stack([offs, offs + rows * Wp], 1).reshape(-1)
        hi = np.stack([offs - rows * Wp, offs], 1).reshape(-1)
        d2 = np.repeat(d2, 2)
        offs_of = lambda pl: hi if pl else lo
    else:
        offs_of = lambda pl: offs
    K = len(d2)
    Vt, Vs, Vc = np.full((len(cand), K), NAN), np.full((len(cand), K), -2, np.int64), np.zeros((len(cand), K), np.int64)
    order = np.argsort(tc, kind="stable")
    # every valid event that is not a candidate, merged in for the one mistake that lets it write
    writers = [(float(tk), int(i), int(k)) for k, (tk, i) in enumerate(zip(tc, cand))]
    if mistake == "non_candidates_overwrite_state":
        others = np.nonzero(inside & ~marked)[0]
        op = (np.asarray(p).reshape(-1)[others] > 0).astype(int) if p is not None else np.zeros(len(others), int)
        ocell = op * rows * Wp + (yt[others].astype(int) + YP) * Wp + xt[others].astype(int) + x_off
        writers += [(float(tf[i]), int(i), -1 - n) for n, i in enumerate(others)]
        writers.sort(key=lambda w: w[:2])
    else:
        writers = [writers[k] for k in order.tolist()]
    for tk, i, k in writers:
        if k < 0:                                                   # (the mistake: the cell is wiped)
            mt[ocell[-1 - k]], msrc[ocell[-1 - k]] = NAN, -3
            continue
        at = cell[k] + offs_of(plane[k])
        Vt[k], Vs[k], Vc[k] = mt[at], msrc[at], at
        mt[cell[k]], msrc[cell[k]] = tk, k

    # the parent: the eligible cell with the greatest t', ties to the smallest d^2, then to the lowest j
    with np.errstate(invalid="ignore"):
        gap = tc[:, None] - Vt
        eligible = ~np.isnan(Vt) & ((gap < max_dt) if mistake == "lt_for_le_max_dt" else (gap <= max_dt))
    if mistake == "own_pixel_left_out":
        eligible[:, d2 == 0] = False
    def narrowed(mask, values, take):                               # the cells of ``mask`` whose value is the row's ``take``
        v = np.where(mask, values, -take(np.array([-np.inf, np.inf])))
        return mask & (v == take(v, axis=1)[:, None])
    d2s = np.broadcast_to(d2.astype(np.float64), Vt.shape)
    if mistake == "nearest_first":
        left = narrowed(narrowed(eligible, d2s, np.min), Vt, np.max)
    else:
        left = narrowed(narrowed(eligible, Vt, np.max), d2s, np.min)
    best = (K - 1 - np.argmax(left[:, ::-1], axis=1)) if mistake == "ties_by_highest_j" else np.argmax(left, axis=1)
    any_ = eligible.any(axis=1)
    rows_ = np.arange(len(cand))
    src = np.where(any_, Vs[rows_, best], -1)                       # -1 a birth, -2 the state, >= 0 a candidate's number
    pcell = Vc[rows_, best]
    k_cls = np.where(src == -1, 5, np.where(src == -2, 6, 7))

    # the parent's state record, for the events whose parent is one: back from the padded map to the cell
    pp, prem = pcell // (rows * Wp), pcell % (rows * Wp)
    sy, sx = np.clip(prem // Wp - YP, 0, H - 1), np.clip(prem % Wp - x_off, 0, W - 1)

    track, length = np.zeros(len(cand), np.int64), np.zeros(len(cand), np.int64)
    b_t, b_x, b_y = np.zeros(len(cand)), np.zeros(len(cand), np.int64), np.zeros(len(cand), np.int64)
    for rank, k in enumerate(order.tolist()):                       # a parent precedes its child: it is complete
        s = int(src[k])
        if s == -1:
            track[k] = next_id + (rank if mistake == "id_from_sorted_position" else int(cand[k]))
            length[k], b_t[k], b_x[k], b_y[k] = 1, tc[k], px[k], py[k]
        elif s == -2:
            at = (pp[k], sy[k], sx[k])
            track[k], b_t[k], b_x[k], b_y[k] = rec["track"][at], rec["t0"][at], rec["x0"][at], rec["y0"][at]
            length[k] = 1 if mistake == "length_not_carried" else min(int(rec["length"][at]) + 1, LEN_MAX)
        else:
            track[k], length[k] = track[s], min(length[s] + 1, LEN_MAX)
            if mistake == "birth_of_parent":
                b_t[k], b_x[k], b_y[k] = tc[s], px[s], py[s]
            else:
                b_t[k], b_x[k], b_y[k] = b_t[s], b_x[s], b_y[s]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        dt = tc - b_t
        vel = np.stack([(px - b_x).astype(np.float64) / dt, (py - b_y).astype(np.float64) / dt], 1)
        vel[tc == b_t] = NAN
        vel = vel.astype(np.float32)

    cls[cand] = k_cls
    out["cls"] = cls.astype(np.uint8)
    out["parent"][cand] = np.where(src >= 0, cand[np.maximum(src, 0)], src).astype(np.int32)
    out["track"][cand], out["length"][cand] = track, length.astype(np.int32)
    out["birth"][cand] = np.stack([b_t, b_x.astype(np.float64), b_y.astype(np.float64)], 1)
    out["velocity"][cand] = vel
    for w_ in (5, 6, 7):
        status[w_] = int((cls == w_).sum())
    # the state: per cell the record of its last candidate, else the input's
    final = msrc.reshape(S, rows, Wp)[:, YP:YP + H, x_off:x_off + W]
    new = state_in.copy()
    at = final >= 0
    k = final[at]
    new[at] = pack_state(tc[k], track[k], b_t[k], b_x[k], b_y[k], length[k], W)
    new[final == -3] = empty_state(1, 1).reshape(4)
    out["state"] = new.reshape(shape)
    return out


def in_pieces(x, y, t, H, W, cuts, fn=event_corner_tracks, corner=None, p=None, **kw):
    """the stream fed in pieces at the indices ``cuts`` through the state -> the outputs concatenated, the last state and
    next_id, the status counters summed"""
    edges = [0] + list(cuts) + [len(t)]
    state, next_id, parts = None, 0, []
    for a, b in zip(edges, edges[1:]):
        g = fn(x[a:b], y[a:b], t[a:b], H, W, corner=None if corner is None else corner[a:b], p=None if p is None else p[a:b],
               state=state, next_id=next_id, **kw)
        g["parent"] = np.where(g["parent"] >= 0, g["parent"] + a, g["parent"])
        state, next_id = g["state"], int(g["next_id"][0])
        parts.append(g)
    res = {k: np.concatenate([g[k] for g in parts]) for k in ("cls", "parent", "track", "length", "birth", "velocity")}
    res.update(state=state, next_id=parts[-1]["next_id"], status=np.sum([g["status"] for g in parts], axis=0).astype(np.int32))
    return res


# ------------------------------------------------------------------------------------------------ test streams
def path(n, H=H0, W=W0, x0=2, y0=2):
    """n + 1 pixels, each one step (in x, or in y at a turn) from the one before: a snake over the rows 2 .. H - 3, columns
    2 .. W - 3, there and back again as often as n asks"""
    xs, ys, x, y, sx, sy = [], [], x0, y0, 1, 1
    while len(xs) <= n:
        xs.append(x), ys.append(y)
        if 2 <= x + sx <= W - 3:
            x += sx
        else:
            sx = -sx
            if not 2 <= y + sy <= H - 3:
                sy = -sy
            y += sy
    return np.array(xs, np.int32), np.array(ys, np.int32)


def chain(n, H=H0, W=W0, t0=0.0):
    """ONE chain of n links: n + 1 corner events a quarter of a time unit apart along ``path``.  With 1 <= radius and
    max_dt = 0.25 every event's only eligible cell is its predecessor's: one track of length n + 1.  -> x, y, t"""
    x, y = path(n, H, W)
    return x, y, t0 + 0.25 * np.arange(n + 1)


def stars(count, H=H0, W=W0):
    """``count`` stars one after another: a root at the sensor's centre and four children at the corners (+-5, +-5) of its
    window, one time unit apart; a star starts 10 units behind the one before.  With radius = 5 and max_dt = 4.5 the children see
    the root alone (they are 10 pixels from each other) and a root sees nothing (the newest event is 6 units old): every root
    has 4 children and nothing else.  Distinct children of one parent cannot see each other and lie in its window, and with
    distinct time stamps four is the most there can be.  -> x, y, t"""
    cx, cy = W // 2, H // 2
    dx, dy = np.array([0, 5, -5, 5, -5]), np.array([0, 5, 5, -5, -5])
    k = np.arange(count)[:, None]
    return ((cx + dx + 0 * k).reshape(-1).astype(np.int32), (cy + dy + 0 * k).reshape(-1).astype(np.int32),
            (10.0 * k + np.arange(5.0)).reshape(-1))


def mixed(N, seed=3, distinct=False, bad=True):
    """cornerref.stream -- wedge runs and noise, equal time stamps included -- with a candidate mask of three events in four and,
    with ``bad``, events that are not finite or outside -> x, y float32, t, p int8, corner uint8"""
    x, y, t, p = (v.copy() for v in cornerref.stream(N, seed=seed, distinct=distinct))
    rng = np.random.default_rng(seed + 100)
    corner = (rng.uniform(size=N) < 0.75).astype(np.uint8) * rng.integers(1, 256, N).astype(np.uint8)
    if bad and N >= 64:
        at = rng.permutation(N)[:N // 16]
        q = len(at) // 4
        x[at[:q]], t[at[q:2 * q]], x[at[2 * q:3 * q]], y[at[3 * q:]] = np.nan, np.inf, -1.0, float(H0)
    return x, y, t, p, corner


def wedge_masks():
    """the wedge streams of cornerref with the detector's own answer as the mask: (name, x, y, t, p, corner)"""
    res = []
    for name, x, y, t, p in cornerref.wedges():
        res.append((name, x, y, t, p, (cornerref.event_corners(x, y, t, H0, W0)["cls"] == 7).astype(np.uint8)))
    return res


def saturating(H=H0, W=W0):
    """a state whose one record has length 2^31 - 2 and was born at (3, 4) at t0 = -2, and two events that link to it one after
    the other -> x, y, t, state"""
    state = empty_state(H, W)
    state[10, 12] = pack_state(1.0, 77, -2.0, 3, 4, LEN_MAX - 1, W)
    return np.array([13, 14], np.int32), np.array([10, 11], np.int32), np.array([1.5, 2.0]), state


CHAIN_LINKS = (1, 2, 63, 64, 65, 4095, 4096, 4097, 5000)     # chains of n + 1 events: the pointer-jumping round edges


def cases():
    """the streams of tests/test_event_corner_tracks_gpu.py that go to the entry as they are: (name, (x, y, t), keywords of
    event_corner_tracks); the state of a second call is the reference's own after the first"""
    res = []
    x, y, t, p, c = mixed(4099)
    for r in (0, 1, 3, 5):
        res.append(("mixed r=%d" % r, (x, y, t), dict(corner=c, p=p, radius=r, max_dt=6 * TICK)))
    res.append(("mixed, every event a candidate", (x, y, t), dict(radius=2, max_dt=2 * TICK)))
    res.append(("mixed, p alone", (x, y, t), dict(p=p, radius=3, max_dt=float("inf"))))
    res.append(("mixed, corner alone, integers", (np.trunc(np.nan_to_num(x, nan=-7.0)).astype(np.int32), np.trunc(y).astype(np.int32), t),
                dict(corner=c, radius=3, max_dt=6 * TICK)))
    first = event_corner_tracks(x[:2000], y[:2000], t[:2000], H0, W0, corner=c[:2000], p=p[:2000], radius=3, max_dt=6 * TICK)
    res.append(("mixed, second call", (x[2000:], y[2000:], t[2000:]),
                dict(corner=c[2000:], p=p[2000:], radius=3, max_dt=6 * TICK, state=first["state"], next_id=int(first["next_id"][0]))))
    res.append(("one time stamp", (x, y, np.full(len(t), 3.25)), dict(corner=c, p=p, radius=3, max_dt=0.0)))
    for n in CHAIN_LINKS:
        res.append(("chain %d" % n, chain(n), dict(radius=1 + n % 3, max_dt=0.25)))
    res.append(("stars", stars(1250), dict(radius=5, max_dt=4.5)))
    for name, wx, wy, wt, wp, wc in wedge_masks():
        res.append(("wedge " + name, (wx, wy, wt), dict(corner=wc, radius=3, max_dt=4 * TICK)))
        res.append(("wedge p " + name, (wx, wy, wt), dict(corner=wc, p=wp, radius=3, max_dt=4 * TICK)))
    sx, sy, st, state = saturating()
    res.append(("saturation", (sx, sy, st), dict(radius=3, max_dt=1.0, state=state, next_id=100)))
    return res
