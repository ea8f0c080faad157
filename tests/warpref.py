"""Numpy restatement of the event warp (include/ramp_hip.h ``ramp_event_warp``) -- TEST INFRASTRUCTURE ONLY.

Two parts:

(a) ``warp``: the warp of every event over tests/interpref.py's interpolation, in float64 (the reference) or float32 (the
    reference formulas' own rounding: the envelope of the GPU test's bound).  No tiles, no staging, no search loop.

        C(t) = interpref.interpolate(knots, times, t)          camera-to-world
        G    = C(t_ref)^-1 C(t)
        X'   = R_G ((x - cx) / fx, (y - cy) / fy, 1) + t_G d
        x'   = fx X'/Z' + cx,  y' = fy Y'/Z' + cy              NaN row: x, y, t not finite, Z' <= MIN_Z, x', y' not finite

(b) ``scatter`` / ``finish``: an EXACT emulator of the kernel's splat, from the kernel's own fp32 coordinates: numpy float32
    for wx, 1 - wx and the products, np.rint of the product times 2^24 to int64, np.add.at.  Integer sums have no order, so
    this reproduces the accumulators bit for bit.

The ``mistake`` keywords break the restatement on purpose (tests/test_warpref_cpu.py: each has to be rejected).
"""
import numpy as np

import georef
import interpref
import poseref
import splatref

MIN_Z = 0.2                  # RAMP_WARP_MIN_Z
FIX_BITS = 24
WARP_MISTAKES = ("fxfy", "inverse")
SCATTER_MISTAKES = ("trunc", "bin")


def sample_depth(invdepth, x, y, H, W):
    """a scalar, or the map's value at the event's rounded pixel (np.rint: halves to even), clamped to the image"""
    d = np.asarray(invdepth, np.float32)
    if d.size == 1:
        return np.full(len(x), d.reshape(-1)[0], np.float32)
    with np.errstate(invalid="ignore"):
        px = np.clip(np.rint(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)), 0, W - 1).astype(np.int64)
        py = np.clip(np.rint(np.nan_to_num(y, nan=0.0, posinf=0.0, neginf=0.0)), 0, H - 1).astype(np.int64)
    return d.reshape(H, W)[py, px]


def event_rays(x, y, t, knots, times, t_ref, K, invdepth, H, W, extrapolate, dtype, mistake=None):
    """what the warp and the contrast share, in ``dtype``: x, y read as float32 and t as float64 -> (fin: the events that are
    finite; tq: their time stamps, times[0] for the others; G [N,7] = C(t_ref)^-1 C(tq); the rays P [N,3]; the inverse depths
    d [N]; (fx, fy, cx, cy)).  None: time stamps that decrease or are not finite"""
    x32, y32 = np.asarray(x, np.float32).reshape(-1), np.asarray(y, np.float32).reshape(-1)
    t = np.asarray(t, np.float64).reshape(-1)
    N = len(x32)
    times = np.asarray(times, np.float64).reshape(-1)
    if not np.isfinite(times).all() or (np.diff(times) < 0).any():
        return None
    fin = np.isfinite(x32) & np.isfinite(y32) & np.isfinite(t)
    tq = np.where(fin, t, times[0])
    C, _ = interpref.interpolate(knots, times, tq, extrapolate, dtype)
    Cr, _ = interpref.interpolate(knots, times, np.array([t_ref]), extrapolate, dtype)
    _, _, inv, mul = poseref.se3_ops(dtype)
    Crn = np.repeat(np.asarray(Cr, dtype), N, 0)
    C = np.asarray(C, dtype)
    G = np.asarray(mul(inv(C), Crn) if mistake == "inverse" else mul(inv(Crn), C), dtype)
    fx, fy, cx, cy = (dtype(v) for v in np.asarray(K, np.float32).reshape(4))
    ux, uy = (fy, fx) if mistake == "fxfy" else (fx, fy)
    xs, ys = np.where(fin, x32, 0).astype(dtype), np.where(fin, y32, 0).astype(dtype)
    d = sample_depth(invdepth, x32, y32, H, W).astype(dtype)
    P = np.stack([(xs - cx) / ux, (ys - cy) / uy, np.ones(N, dtype)], -1)
    return fin, tq, G, P, d, (fx, fy, cx, cy)


def warp(x, y, t, knots, times, t_ref, K, invdepth, H, W, extrapolate=False, dtype=np.float64, mistake=None):
    """-> (xy [N,2] in ``dtype`` with NaN rows for invalid events, Z' [N])"""
    assert mistake is None or mistake in WARP_MISTAKES
    rays = event_rays(x, y, t, knots, times, t_ref, K, invdepth, H, W, extrapolate, dtype, mistake)
    if rays is None:
        N = np.asarray(x).size
        return np.full((N, 2), np.nan, dtype), np.full(N, np.nan, dtype)
    fin, _, G, P, d, (fx, fy, cx, cy) = rays
    with np.errstate(all="ignore"):
        X = poseref.qrot(G[:, 3:], P) + G[:, :3] * d[:, None]
        Z = X[:, 2]
        xy = np.stack([fx * (X[:, 0] / Z) + cx, fy * (X[:, 1] / Z) + cy], -1)
        bad = ~fin | ~(Z > dtype(MIN_Z)) | ~np.isfinite(xy).all(-1)
    xy[bad] = np.nan
    Z = np.where(fin, Z, np.nan)
    return xy.astype(dtype), Z.astype(dtype)


def compare_coords(out, r64, z64, r32, z_margin):
    """the check of coordinates [..., 2] (NaN: invalid) against the float64 restatement ``r64`` with its ``z64``.  err: largest
    coordinate difference over the entries both call valid; env: the float32 restatement's own (``r32``); bound =
    georef.bound(PIXEL_FLOOR x largest |coordinate|, env).  The NaN entries have to agree except where float64's Z' is within
    ``z_margin`` of MIN_Z."""
    out = np.asarray(out, np.float64)
    v64, v32, vg = ~np.isnan(r64).any(-1), ~np.isnan(r32).any(-1), ~np.isnan(out).any(-1)
    edge = np.abs(z64 - MIN_Z) < z_margin
    nan_ok = bool(((vg == v64) | edge).all())
    keep = v64 & vg
    err = float(np.abs(out[keep] - r64[keep]).max()) if keep.any() else 0.0
    k32 = v64 & v32
    env = float(np.abs(r32[k32].astype(np.float64) - r64[k32]).max()) if k32.any() else 0.0
    floor = georef.PIXEL_FLOOR * max(1.0, float(np.abs(r64[v64]).max()) if v64.any() else 1.0)
    b = georef.bound(floor, env)
    return dict(err=err, env=env, floor=floor, bound=b, nan_ok=nan_ok, n_valid=int(keep.sum()), ok=nan_ok and err <= b)


def compare(xy_gpu, x, y, t, knots, times, t_ref, K, invdepth, H, W, extrapolate=False, z_margin=1e-4):
    """the GPU test's check of one launch: ``compare_coords`` against this restatement"""
    r64, z64 = warp(x, y, t, knots, times, t_ref, K, invdepth, H, W, extrapolate, np.float64)
    r32, _ = warp(x, y, t, knots, times, t_ref, K, invdepth, H, W, extrapolate, np.float32)
    return compare_coords(xy_gpu, r64, z64, r32, z_margin)


# ------------------------------------------------------------------------------------------------------------ the splat
def bins_of(index, N, bins):
    """event i -> int32(float32(bins) * float32(i) / float32(N)), capped at bins - 1"""
    b = ((np.float32(bins) * np.asarray(index).astype(np.float32)) / np.float32(N)).astype(np.int32)
    return np.minimum(b, bins - 1).astype(np.int64)


def scatter(xy, p, H, W, bins=0, index=None, mistake=None):
    """the kernel's accumulators from ITS warped coordinates ``xy`` [N,2] float32 (NaN rows contribute nothing) ->
    dict(iwe int64 [2,H,W], stack int64 [bins,H,W] or None, n_outside, n_contributed, weight_sum int64 [N])"""
    assert mistake is None or mistake in SCATTER_MISTAKES
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    N = len(xy)
    p = np.asarray(p).astype(np.int64).reshape(-1)
    p = np.where(p == 0, -1, p)                       # (0 is read as -1)
    valid = ~np.isnan(xy).any(-1)
    xv = np.where(valid, xy[:, 0], 0).astype(np.float32)
    yv = np.where(valid, xy[:, 1], 0).astype(np.float32)
    ix, wx, inx = splatref.axis(xv, W, mistake=mistake)
    iy, wy, iny = splatref.axis(yv, H, mistake=mistake)
    iwe = np.zeros((2, H, W), np.int64)
    stack = np.zeros((bins, H, W), np.int64) if bins else None
    b = bins_of(np.arange(N) if index is None else index, N, bins) if bins else None
    if bins and mistake == "bin":
        b = np.minimum(b + 1, bins - 1)
    inside = valid & (inx[0] | inx[1]) & (iny[0] | iny[1])
    wsum = np.zeros(N, np.int64)
    for jy in range(2):
        for jx in range(2):
            c = splatref.fixed_weight(wx[jx], wy[jy], FIX_BITS)
            wsum += np.where(valid, c, 0)
            m = valid & inx[jx] & iny[jy]
            yy, xx = (iy + jy)[m], (ix + jx)[m]
            np.add.at(iwe[0], (yy, xx), p[m] * c[m])
            np.add.at(iwe[1], (yy, xx), c[m])
            if bins:
                np.add.at(stack, (b[m], yy, xx), p[m] * c[m])
    return dict(iwe=iwe, stack=stack, n_outside=int((valid & ~inside).sum()), n_contributed=int(inside.sum()), weight_sum=wsum)


def finish_f32(acc):
    """float(sum) * 2^-24: the int64 -> float32 conversion rounds once, the scaling is exact"""
    return acc.astype(np.float32) * np.float32(2.0 ** -FIX_BITS)


def finish_i8(acc):
    """the fixed-point sum divided by 2^24 toward zero, then modulo 256"""
    q = np.sign(acc) * (np.abs(acc) >> FIX_BITS)
    return (q & 0xFF).astype(np.uint8).view(np.int8)
