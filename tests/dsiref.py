"""Numpy restatement of the event plane sweep (include/ramp_hip.h ``ramp_event_dsi``) -- TEST INFRASTRUCTURE ONLY.

(a) ``coordinates``: per event and plane, tests/warpref.py's ``warp`` called with the scalar inverse depth d_k, in float64 (the
    reference) or float32 (the reference formulas' own rounding: the envelope of the GPU test's bound).  ``compare`` is the GPU
    test's check of a call's ``coords``.

(b) an EXACT emulator in integers: ``votes`` starts from given fp32 coordinates (as ``warpref.scatter`` does: numpy float32 for
    the weights, np.rint of the product times 2^24, np.add.at) and gives the accumulators bit for bit; ``detect`` starts from
    given integer accumulators: best plane, box sums (a summed-area table over Python's integers), threshold, refinement.

(c) the ``mistake`` keywords break the restatement on purpose (tests/test_dsiref_cpu.py: each has to be rejected).
"""
import numpy as np

import splatref
import warpref

FIX_BITS = warpref.FIX_BITS
MIN_Z = warpref.MIN_Z
COORD_MISTAKES = ("depth", "inverse", "fxfy", "plane")
VOTE_MISTAKES = ("trunc",)
DETECT_MISTAKES = ("tie_high", "gt", "area", "sign")


def plane_depths(rng, D, mistake=None):
    """d_k = float32(double(d_lo) + k * step), step = (double(d_hi) - double(d_lo)) / (D - 1); -> (d [D] float32, step)"""
    lo, hi = (float(v) for v in np.asarray(rng, np.float32).reshape(2))
    step = (hi - lo) / (D - 1) if D > 1 else 0.0
    k = np.arange(D, dtype=np.float64) + (1.0 if mistake == "plane" else 0.0)
    if mistake == "depth" and D > 1:                 # uniform in depth between the same two ends
        z = 1.0 / lo + k * (1.0 / hi - 1.0 / lo) / (D - 1)
        return (1.0 / z).astype(np.float32), step
    return (lo + k * step).astype(np.float32), step


def bad_range(rng, D):
    lo, hi = np.asarray(rng, np.float32).reshape(2)
    return bool(not np.isfinite(lo) or not np.isfinite(hi) or lo < 0 or (D > 1 and hi <= lo))


def coordinates(x, y, t, knots, times, t_ref, K, rng, D, H, W, extrapolate=False, dtype=np.float64, mistake=None):
    """-> (coords [N,D,2] in ``dtype``, NaN where the plane gets no vote; Z' [N,D])"""
    assert mistake is None or mistake in COORD_MISTAKES
    d, _ = plane_depths(rng, D, mistake)
    wm = mistake if mistake in warpref.WARP_MISTAKES else None
    per = [warpref.warp(x, y, t, knots, times, t_ref, K, dk, H, W, extrapolate, dtype, mistake=wm) for dk in d]
    return np.stack([p[0] for p in per], 1), np.stack([p[1] for p in per], 1)


def compare(coords_gpu, x, y, t, knots, times, t_ref, K, rng, D, H, W, extrapolate=False, z_margin=1e-4, mistake=None):
    """``warpref.compare`` over events x planes: ``warpref.compare_coords`` against this restatement"""
    r64, z64 = coordinates(x, y, t, knots, times, t_ref, K, rng, D, H, W, extrapolate, np.float64)
    r32, _ = coordinates(x, y, t, knots, times, t_ref, K, rng, D, H, W, extrapolate, np.float32)
    return warpref.compare_coords(coords_gpu, r64, z64, r32, z_margin)


# ------------------------------------------------------------------------------------------------------- the exact emulator
def votes(coords, H, W, mistake=None):
    """the accumulators from fp32 coordinates [N,D,2] (NaN: no vote) -> dict(dsi int64 [D,H,W], n_no_vote, n_voted: the events
    with no / at least one entry that is not NaN)"""
    assert mistake is None or mistake in VOTE_MISTAKES
    c = np.asarray(coords, np.float32)
    N, D = c.shape[:2]
    dsi = np.zeros((D, H, W), np.int64)
    valid = ~np.isnan(c).any(-1)
    for k in range(D):
        m0 = valid[:, k]
        xv, yv = np.where(m0, c[:, k, 0], 0).astype(np.float32), np.where(m0, c[:, k, 1], 0).astype(np.float32)
        ix, wx, inx = splatref.axis(xv, W, mistake=mistake)
        iy, wy, iny = splatref.axis(yv, H, mistake=mistake)
        for jy in range(2):
            for jx in range(2):
                w = splatref.fixed_weight(wx[jx], wy[jy], FIX_BITS)
                m = m0 & inx[jx] & iny[jy]
                np.add.at(dsi[k], ((iy + jy)[m], (ix + jx)[m]), w[m])
    any_vote = valid.any(1) if D else np.zeros(N, bool)
    return dict(dsi=dsi, n_voted=int(any_vote.sum()), n_no_vote=int((~any_vote).sum()))


def fixed(v):
    """llrint(v * 2^24)"""
    return int(np.rint(np.float64(v) * 2.0 ** FIX_BITS))


def box_sums(best, r, mistake=None):
    """-> (box, n_in): per pixel the sum of ``best`` over the (2r+1)^2 window clipped to the image, and the window's pixels
    inside the image; Python integers (object arrays): no width to overflow"""
    H, W = best.shape
    sat = np.zeros((H + 1, W + 1), object)
    sat[1:, 1:] = np.cumsum(np.cumsum(best.astype(object), 0), 1)
    ys, xs = np.arange(H), np.arange(W)
    y0, y1 = np.maximum(ys - r, 0), np.minimum(ys + r, H - 1) + 1
    x0, x1 = np.maximum(xs - r, 0), np.minimum(xs + r, W - 1) + 1
    box = sat[y1][:, x1] - sat[y0][:, x1] - sat[y1][:, x0] + sat[y0][:, x0]
    n_in = ((y1 - y0)[:, None] * (x1 - x0)[None, :]).astype(object)
    if mistake == "area":
        n_in = np.full((H, W), (2 * r + 1) ** 2, object)
    return box, n_in


def detect(dsi, rng, min_votes, adaptive_radius=0, adaptive_offset=0.0, fill=None, mistake=None):
    """from integer accumulators [D,H,W] -> dict(plane int32 (-1: not detected), detected bool, confidence float32, invdepth
    float32 (fill or NaN where not detected), best int64, n_detected)"""
    assert mistake is None or mistake in DETECT_MISTAKES
    dsi = np.asarray(dsi, np.int64)
    D, H, W = dsi.shape
    best = dsi.max(0)
    plane = (D - 1 - np.argmax(dsi[::-1], 0)) if mistake == "tie_high" else np.argmax(dsi, 0)       # argmax: the first = lowest
    at_least = (lambda a, b: a > b) if mistake == "gt" else (lambda a, b: a >= b)
    det = at_least(best.astype(object), fixed(min_votes))
    if adaptive_radius > 0:
        box, n_in = box_sums(best, adaptive_radius, mistake)
        det = det & at_least(best.astype(object), box // n_in + fixed(adaptive_offset))
    det = det.astype(bool)
    lo, hi = (float(v) for v in np.asarray(rng, np.float32).reshape(2))
    step = (hi - lo) / (D - 1) if D > 1 else 0.0
    yy, xx = np.mgrid[0:H, 0:W]
    inner = (plane > 0) & (plane < D - 1)
    a = dsi[np.clip(plane - 1, 0, D - 1), yy, xx]
    c = dsi[np.clip(plane + 1, 0, D - 1), yy, xx]
    den = a - 2 * best + c
    ok = inner & (den != 0)
    num = (c - a) if mistake == "sign" else (a - c)
    delta = np.where(ok, num.astype(np.float64) / (2.0 * np.where(ok, den, 1).astype(np.float64)), 0.0)
    inv = (lo + (plane.astype(np.float64) + delta) * step).astype(np.float32)
    f = np.float32(np.nan if fill is None else fill)
    return dict(plane=np.where(det, plane, -1).astype(np.int32), detected=det, best=best,
                confidence=best.astype(np.float32) * np.float32(2.0 ** -FIX_BITS), invdepth=np.where(det, inv, f).astype(np.float32),
                refined=inv, n_detected=int(det.sum()))


# ---------------------------------------------------------------------------------------------------------------- scenes
TWO_PLANE = dict(H=48, W=64, K=np.array([60.0, 60.0, 31.5, 23.5], np.float32), D=16, rng=(0.25, 1.75), t_ref=0.5, min_votes=32.0,
                 planes=(3, 10))


def two_plane_scene(seed=3, points=40, per_point=64):
    """the camera slides along x by 0.4 (t - 0.5) over t in [0, 1]; ``points`` scene points on each of two planes of the sweep
    (3 and 10 of 16 over (0.25, 1.75)), each seen by ``per_point`` events at random times, coordinates rounded to whole pixels
    -> (x, y, t, knots, times)"""
    s = TWO_PLANE
    rng = np.random.default_rng(seed)
    d, _ = plane_depths(s["rng"], s["D"])
    fx, fy, cx, cy = (float(v) for v in s["K"])
    knots = np.array([[-0.2, 0, 0, 0, 0, 0, 1], [0.2, 0, 0, 0, 0, 0, 1]], np.float32)
    times = np.array([0.0, 1.0])
    xs, ys, ts = [], [], []
    for k in s["planes"]:
        u, v = rng.uniform(10, s["W"] - 11, points), rng.uniform(4, s["H"] - 5, points)
        Z = 1.0 / float(d[k])
        X, Y = (u - cx) / fx * Z, (v - cy) / fy * Z               # the point in the camera at t_ref (at the origin)
        t = rng.uniform(0, 1, (points, per_point))
        cam = 0.4 * (t - 0.5)                                     # the camera's x at t (camera-to-world, no rotation)
        xs.append(np.rint(fx * (X[:, None] - cam) / Z + cx))
        ys.append(np.rint(np.repeat((fy * Y / Z + cy)[:, None], per_point, 1)))
        ts.append(t)
    return (np.concatenate(xs).reshape(-1).astype(np.float32), np.concatenate(ys).reshape(-1).astype(np.float32),
            np.concatenate(ts).reshape(-1), knots, times)


def two_plane_conditions(plane):
    """the two conditions of the two-plane scene on a detected ``plane`` map (-1: not detected)"""
    p = plane[plane >= 0]
    a, b = TWO_PLANE["planes"]
    near = (np.abs(p - a) <= 1) | (np.abs(p - b) <= 1)
    return dict(all_near=bool(near.all()), on_a=int((p == a).sum()), on_b=int((p == b).sum()), n=int(p.size),
                ok=bool(near.all()) and int((p == a).sum()) >= 30 and int((p == b).sum()) >= 30)
