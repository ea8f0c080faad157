"""Numpy restatement of the lens-distortion entries (include/ramp_hip.h ``ramp_event_rectify`` / ``ramp_image_rectify``) -- TEST
INFRASTRUCTURE ONLY.

Three parts:

(a) ``distort`` / ``undistort`` / ``event_rectify`` / ``image_map``: both directions over whole arrays, parametrised by dtype.
    float64 is the reference; float32 is the formulas' own rounding: the envelope of the GPU test's bound.  No tiles, no
    staging.  The inversions are the ones the kernel is held to:

        radtan        p = (xd, yd);  ITERS times:  p <- p - J(p)^-1 (distort(p) - (xd, yd)),  J analytic and symmetric
        equidistant   thd = sqrt(xd^2 + yd^2);  th = thd;  ITERS times:  th <- th - (thd(th) - thd) / thd'(th);
                      (x, y) = (tan th / thd) (xd, yd),  thd == 0: (xd, yd)
        accepted      every iterate finite, det J (thd') > 0 at the start and at every iterate, the final residual in raw
                      pixels <= TOL, and for the equidistant model 0 <= th < pi / 2

(b) ``sample``: an EXACT float32 emulator of the bilinear and value arithmetic, from a given map (the kernel's own): numpy
    float32 products and sums in the kernel's order, so the pixel values are reproduced bit for bit.

(c) the test cameras: the five cameras the Newton count was chosen on, scaled to a 64 x 48 sensor with the same normalised
    field of view (the distortion, and so the difficulty, is unchanged; only pixel counts shrink), one with a rotation, one
    with rectified intrinsics that differ from the raw ones, and a pinhole whose numbers are dyadic, so that its map is exact.

The ``mistake`` keywords break the restatement on purpose (tests/test_rectifyref_cpu.py: each has to be rejected).
"""
import numpy as np

import georef

PINHOLE, RADTAN, EQUIDISTANT = 0, 1, 2
ITERS = 8                    # RAMP_RECTIFY_ITERS
TOL = 2.0 ** -6              # RAMP_RECTIFY_TOL, raw pixels
WORDS, RAW, MODEL, COEFFS, ROTATION, NEW = 32, 0, 4, 5, 12, 24          # RAMP_CAMERA_*
MISTAKES = ("p1p2", "fxfy", "transpose", "iters", "nodet", "ratio")
NOT_FINITE, NOT_INVERTIBLE, BEHIND, OUTSIDE, INSIDE = 2, 3, 4, 5, 6     # the status word an event is counted in
IM_INVALID, IM_OUTSIDE, IM_SAMPLED = 2, 3, 4                             # the status word a pixel is counted in
# The validity of a solution may differ from float64's only next to the two thresholds.  A determinant below DET_MARGIN
# multiplies a residual of TOL / f (f ~ 40: 4e-4 in normalised units) into a displacement of 4e-2 or more, enough to carry a
# float32 iterate across the fold float64 stays clear of; a float64 residual within a factor 2 of TOL is decided by rounding.
DET_MARGIN = 1e-2
HS, WS = 48, 64              # the raw sensor of every test camera


def _rotation(rx, ry, rz):
    """R = Rz Ry Rx from angles in degrees, float64"""
    a, b, c = np.deg2rad([rx, ry, rz])
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _cam(model, raw, coeffs=(), R=None, new=None):
    return dict(model=model, raw=tuple(float(v) for v in raw), coeffs=tuple(float(v) for v in coeffs), R=R,
                new=None if new is None else tuple(float(v) for v in new))


_S346, _S640 = 64.0 / 346.0, 0.1
CAMERAS = {
    # a pinhole with dyadic numbers: (u - c) / f * f + c is exact in float32, the map of the identity is the pixel grid itself
    "pinhole": _cam(PINHOLE, (64.0, 64.0, 31.5, 23.5)),
    # 346 x 260, f = 250, radtan
    "radtan346": _cam(RADTAN, (250 * _S346, 250.5 * _S346, 172.2 * _S346, 131.4 * _S346), (-0.38, 0.17, 4e-4, -6e-4, 0.0)),
    # 640 x 480, f = 766, radtan
    "radtan640": _cam(RADTAN, (76.6, 76.8, 31.9, 23.3), (-0.29, 0.11, -5e-4, 3e-4, -0.02)),
    # 640 x 480, f = 560, equidistant
    "equi640": _cam(EQUIDISTANT, (56.0, 56.1, 32.2, 23.6), (-0.035, 0.012, -0.006, 0.0012)),
    # a 280-pixel fisheye on 640 x 480
    "fisheye280": _cam(EQUIDISTANT, (28.0, 28.0, 31.7, 23.9), (0.02, -0.012, 0.006, -0.0015)),
    # the failure-path camera: 346 x 260, f = 200, a polynomial that folds inside the sensor
    "strong": _cam(RADTAN, (200 * _S346, 200 * _S346, 173 * _S346, 130 * _S346), (-0.45, 0.25, 1e-3, -1e-3, -0.07)),
    # the same sensor into a rectified camera that sees past the fold: 8 pixels more on every side (an image of 61 x 77 or
    # 64 x 80), so that the image direction has pixels without a sample of each kind
    "strong_wide": _cam(RADTAN, (200 * _S346, 200 * _S346, 173 * _S346, 130 * _S346), (-0.45, 0.25, 1e-3, -1e-3, -0.07),
                        new=(200 * _S346, 200 * _S346, 173 * _S346 + 8, 130 * _S346 + 8)),
    # radtan346 behind a rotation of a few degrees
    "rotated": _cam(RADTAN, (250 * _S346, 250.5 * _S346, 172.2 * _S346, 131.4 * _S346), (-0.38, 0.17, 4e-4, -6e-4, 0.0),
                    R=_rotation(2.0, -3.0, 1.5)),
    # equi640 into a rectified camera of its own
    "newK": _cam(EQUIDISTANT, (56.0, 56.1, 32.2, 23.6), (-0.035, 0.012, -0.006, 0.0012), new=(40.0, 41.0, 30.0, 25.0)),
}
ORDINARY = ("radtan346", "radtan640", "equi640", "fisheye280", "rotated", "newK")


def new_intrinsics(cam):
    return cam["raw"] if cam["new"] is None else cam["new"]


def record(cam):
    """the float32 camera record, as ops.camera lays it out"""
    w = np.zeros(WORDS, np.float32)
    w[RAW:RAW + 4] = cam["raw"]
    w[MODEL] = cam["model"]
    w[COEFFS:COEFFS + len(cam["coeffs"])] = cam["coeffs"]
    w[ROTATION:ROTATION + 9] = (np.eye(3) if cam["R"] is None else np.asarray(cam["R"])).reshape(-1)
    w[NEW:NEW + 4] = new_intrinsics(cam)
    return w


def _params(cam, T):
    """the record's numbers as the kernel reads them -- rounded to float32 first -- in dtype T"""
    w = record(cam)
    k = [T(v) for v in w[COEFFS:COEFFS + 5]]
    return [T(v) for v in w[RAW:RAW + 4]], k, w[ROTATION:ROTATION + 9].astype(T).reshape(3, 3), [T(v) for v in w[NEW:NEW + 4]]


# --------------------------------------------------------------------------------------------------------- the two models
def _radtan(k, x, y, T, mistake=None):
    """-> xd, yd, J11, J12, J22"""
    k1, k2, p1, p2, k3 = k
    if mistake == "p1p2":
        p1, p2 = p2, p1
    xx, yy, xy = x * x, y * y, x * y
    r2 = xx + yy
    rad = T(1) + r2 * (k1 + r2 * (k2 + r2 * k3))
    drad = k1 + r2 * (T(2) * k2 + r2 * (T(3) * k3))
    xd = x * rad + T(2) * p1 * xy + p2 * (r2 + T(2) * xx)
    yd = y * rad + p1 * (r2 + T(2) * yy) + T(2) * p2 * xy
    J11 = rad + T(2) * xx * drad + T(2) * p1 * y + T(6) * p2 * x
    J12 = T(2) * xy * drad + T(2) * p1 * x + T(2) * p2 * y
    J22 = rad + T(2) * yy * drad + T(6) * p1 * y + T(2) * p2 * x
    return xd, yd, J11, J12, J22


def _equi(k, th, T):
    """-> thd, d thd / d th"""
    t2 = th * th
    thd = th * (T(1) + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    dthd = T(1) + t2 * (T(3) * k[0] + t2 * (T(5) * k[1] + t2 * (T(7) * k[2] + t2 * (T(9) * k[3]))))
    return thd, dthd


def distort(model, k, x, y, T=np.float64, mistake=None):
    """normalised ray -> (xd, yd, det): the model's Jacobian determinant at the ray (d thd / d th for the equidistant model)"""
    x, y = np.atleast_1d(np.asarray(x, T)), np.atleast_1d(np.asarray(y, T))
    k = [T(v) for v in (list(k) + [0.0] * 5)[:5]]
    with np.errstate(all="ignore"):
        if model == RADTAN:
            xd, yd, J11, J12, J22 = _radtan(k, x, y, T, mistake)
            return xd, yd, J11 * J22 - J12 * J12
        if model == EQUIDISTANT:
            r = np.sqrt(x * x + y * y)
            thd, dthd = _equi(k, np.arctan(r), T)
            safe = np.where(r > 0, r, T(1))
            s = np.where(r > 0, (safe / np.where(thd != 0, thd, T(1))) if mistake == "ratio" else thd / safe, T(1))
            return s * x, s * y, dthd
    return x.copy(), y.copy(), np.ones_like(x)


def undistort(model, k, xd, yd, fx=1.0, fy=1.0, T=np.float64, iters=ITERS, mistake=None):
    """(xd, yd) -> dict(x, y, ok, detmin: the smallest determinant over the start and every iterate, res: the final residual in
    raw pixels)"""
    xd, yd = np.atleast_1d(np.asarray(xd, T)), np.atleast_1d(np.asarray(yd, T))
    k = [T(v) for v in (list(k) + [0.0] * 5)[:5]]
    fx, fy = T(fx), T(fy)
    if mistake == "iters":
        iters -= 1
    ok = np.ones(xd.shape, bool)
    with np.errstate(all="ignore"):
        if model == RADTAN:
            x, y = xd.copy(), yd.copy()
            detmin = np.full(xd.shape, np.inf, T)
            for _ in range(iters):
                fxv, fyv, J11, J12, J22 = _radtan(k, x, y, T, mistake)
                det = J11 * J22 - J12 * J12
                ex, ey = fxv - xd, fyv - yd
                detmin = np.fmin(detmin, np.where(np.isnan(det), -np.inf, det))
                x = x - (J22 * ex - J12 * ey) / det
                y = y - (J11 * ey - J12 * ex) / det
                ok &= np.isfinite(x) & np.isfinite(y)
            fxv, fyv, J11, J12, J22 = _radtan(k, x, y, T, mistake)
            det = J11 * J22 - J12 * J12
            detmin = np.fmin(detmin, np.where(np.isnan(det), -np.inf, det))
            ex, ey = (fxv - xd) * fx, (fyv - yd) * fy
            res2 = ex * ex + ey * ey
            res = np.sqrt(res2)
            ok &= res2 <= T(TOL) * T(TOL)
            if mistake != "nodet":
                ok &= detmin > 0
            return dict(x=x, y=y, ok=ok, detmin=detmin, res=res)
        if model == EQUIDISTANT:
            thd = np.sqrt(xd * xd + yd * yd)
            th = thd.copy()
            detmin = np.full(xd.shape, np.inf, T)
            for _ in range(iters):
                f, df = _equi(k, th, T)
                detmin = np.fmin(detmin, np.where(np.isnan(df), -np.inf, df))
                th = th - (f - thd) / df
                ok &= np.isfinite(th)
            f, df = _equi(k, th, T)
            detmin = np.fmin(detmin, np.where(np.isnan(df), -np.inf, df))
            res = np.abs(f - thd) * max(fx, fy)
            ok &= (res <= T(TOL)) & (th >= 0) & (th < T(np.float32(1.57079632679489662)))
            if mistake != "nodet":
                ok &= detmin > 0
            s = np.where(thd > 0, np.tan(np.where(ok, th, T(0))) / np.where(thd > 0, thd, T(1)), T(1))
            return dict(x=s * xd, y=s * yd, ok=ok, detmin=detmin, res=res)
    return dict(x=xd.copy(), y=yd.copy(), ok=ok, detmin=np.ones_like(xd), res=np.zeros_like(xd))


# ------------------------------------------------------------------------------------------------------ the two directions
def event_rectify(x, y, cam, H, W, T=np.float64, mistake=None, iters=ITERS):
    """raw pixels (read as float32, like the kernel) -> dict(xy [N,2] in T with NaN rows, cls: the status word of every event,
    detmin, res, status int64 [8])"""
    assert mistake is None or mistake in MISTAKES
    x32, y32 = np.asarray(x, np.float32).reshape(-1), np.asarray(y, np.float32).reshape(-1)
    (fx, fy, cx, cy), k, R, (nfx, nfy, ncx, ncy) = _params(cam, T)
    if mistake == "fxfy":
        fx, fy = fy, fx
    if mistake == "transpose":
        R = R.T
    fin = np.isfinite(x32) & np.isfinite(y32)
    xs, ys = np.where(fin, x32, 0).astype(T), np.where(fin, y32, 0).astype(T)
    xd, yd = (xs - cx) / fx, (ys - cy) / fy
    u = undistort(cam["model"], k, xd, yd, fx, fy, T, iters, mistake)
    with np.errstate(all="ignore"):
        X = R[0, 0] * u["x"] + R[0, 1] * u["y"] + R[0, 2]
        Y = R[1, 0] * u["x"] + R[1, 1] * u["y"] + R[1, 2]
        Z = R[2, 0] * u["x"] + R[2, 1] * u["y"] + R[2, 2]
        px, py = nfx * (X / Z) + ncx, nfy * (Y / Z) + ncy
        front = (Z > 0) & np.isfinite(px) & np.isfinite(py)
        inside = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
    cls = np.where(~fin, NOT_FINITE, np.where(~u["ok"], NOT_INVERTIBLE, np.where(~front, BEHIND, np.where(inside, INSIDE, OUTSIDE))))
    xy = np.stack([px, py], -1).astype(T)
    xy[cls < OUTSIDE] = np.nan
    status = np.zeros(8, np.int64)
    status[1] = len(x32)
    for c in (NOT_FINITE, NOT_INVERTIBLE, BEHIND, OUTSIDE, INSIDE):
        status[c] = int((cls == c).sum())
    return dict(xy=xy, cls=cls, detmin=np.where(fin, u["detmin"], np.nan), res=np.where(fin, u["res"], np.nan), status=status)


def image_map(cam, Hs, Ws, H, W, T=np.float64, mistake=None):
    """the forward direction per rectified pixel -> dict(map [H,W,2] in T, NaN where nothing is sampled; cls [H,W]: the status
    word of every pixel; det [H,W]; raw [H,W,2]: the source coordinates before any test; status int64 [8])"""
    assert mistake is None or mistake in MISTAKES
    (fx, fy, cx, cy), k, R, (nfx, nfy, ncx, ncy) = _params(cam, T)
    if mistake == "fxfy":
        fx, fy = fy, fx
    if mistake == "transpose":
        R = R.T
    v, u = np.meshgrid(np.arange(H, dtype=T), np.arange(W, dtype=T), indexing="ij")
    with np.errstate(all="ignore"):
        rx, ry = (u - ncx) / nfx, (v - ncy) / nfy
        X = R[0, 0] * rx + R[1, 0] * ry + R[2, 0]
        Y = R[0, 1] * rx + R[1, 1] * ry + R[2, 1]
        Z = R[0, 2] * rx + R[1, 2] * ry + R[2, 2]
        xd, yd, det = distort(cam["model"], k, (X / Z).reshape(-1), (Y / Z).reshape(-1), T, mistake)
        xs, ys = (fx * xd + cx).reshape(H, W), (fy * yd + cy).reshape(H, W)
        det = det.reshape(H, W)
        good = (Z > 0) & (det > 0) & np.isfinite(xs) & np.isfinite(ys)
        inside = (xs >= 0) & (xs <= Ws - 1) & (ys >= 0) & (ys <= Hs - 1)
    cls = np.where(~good, IM_INVALID, np.where(inside, IM_SAMPLED, IM_OUTSIDE))
    raw = np.stack([xs, ys], -1).astype(T)
    m = raw.copy()
    m[cls != IM_SAMPLED] = np.nan
    status = np.zeros(8, np.int64)
    status[1] = H * W
    for c in (IM_INVALID, IM_OUTSIDE, IM_SAMPLED):
        status[c] = int((cls == c).sum())
    return dict(map=m, cls=cls, det=det, raw=raw, status=status)


# ------------------------------------------------------------------------------------------------------ the exact emulator
def sample(src, m, norm=None, fill=0.0):
    """the kernel's pixel values from ITS map ``m`` [H,W,2] float32 (NaN: ``fill``): float32 products and sums in the kernel's
    order -> [C,H,W] float32, bit for bit.  ``src`` [C,Hs,Ws] uint8 or float32; ``norm`` None, "half" or "unit"."""
    f32 = np.float32
    src = np.asarray(src)
    C, Hs, Ws = src.shape
    m = np.asarray(m, f32)
    ok = ~np.isnan(m).any(-1)
    xs, ys = np.where(ok, m[..., 0], 0).astype(f32), np.where(ok, m[..., 1], 0).astype(f32)
    x0, y0 = np.floor(xs), np.floor(ys)
    wx, wy = (xs - x0).astype(f32), (ys - y0).astype(f32)
    vx, vy = (f32(1) - wx).astype(f32), (f32(1) - wy).astype(f32)
    ix0, iy0 = x0.astype(np.int64), y0.astype(np.int64)
    ix1, iy1 = np.minimum(ix0 + 1, Ws - 1), np.minimum(iy0 + 1, Hs - 1)
    s = src.astype(f32)
    a, b, c, d = s[:, iy0, ix0], s[:, iy0, ix1], s[:, iy1, ix0], s[:, iy1, ix1]
    top = ((vx * a).astype(f32) + (wx * b).astype(f32)).astype(f32)
    bot = ((vx * c).astype(f32) + (wx * d).astype(f32)).astype(f32)
    val = ((vy * top).astype(f32) + (wy * bot).astype(f32)).astype(f32)
    if norm is not None:
        val = ((f32(2) * (val / f32(255)).astype(f32)).astype(f32) - f32({"half": 0.5, "unit": 1.0}[norm])).astype(f32)
    return np.where(ok[None], val, f32(fill)).astype(f32)


# ------------------------------------------------------------------------------------------------------------ the checks
def excused(r64):
    """events whose validity rounding may decide: float64's smallest determinant within DET_MARGIN of 0, or its residual
    within a factor 2 of TOL"""
    with np.errstate(invalid="ignore"):
        return (np.abs(r64["detmin"]) < DET_MARGIN) | ((r64["res"] >= TOL / 2) & (r64["res"] <= TOL * 2))


def compare_events(xy, x, y, cam, H, W):
    """the GPU test's check of one call, the rule of warpref.compare.  err: the largest coordinate difference from the float64
    restatement over the rows both call valid; env: the float32 restatement's own; bound = georef.bound(PIXEL_FLOOR x largest
    |coordinate|, env).  The NaN rows have to agree with float64's except the ``excused`` ones, which are counted."""
    r64, r32 = event_rectify(x, y, cam, H, W, np.float64), event_rectify(x, y, cam, H, W, np.float32)
    out = np.asarray(xy, np.float64)
    v64, v32, vg = r64["cls"] >= OUTSIDE, r32["cls"] >= OUTSIDE, ~np.isnan(out).any(-1)
    ex = excused(r64)
    differ = vg != v64
    keep = v64 & vg
    err = float(np.abs(out[keep] - r64["xy"][keep]).max()) if keep.any() else 0.0
    k32 = v64 & v32
    env = float(np.abs(r32["xy"][k32].astype(np.float64) - r64["xy"][k32]).max()) if k32.any() else 0.0
    floor = georef.PIXEL_FLOOR * max(1.0, float(np.abs(r64["xy"][v64]).max()) if v64.any() else 1.0)
    b = georef.bound(floor, env)
    return dict(err=err, env=env, floor=floor, bound=b, n_valid=int(keep.sum()), n_differ=int(differ.sum()),
                n_unexcused=int((differ & ~ex).sum()), n_excused=int((differ & ex).sum()), r64=r64, r32=r32,
                ok=err <= b and not (differ & ~ex).any())


def compare_map(m, cam, Hs, Ws, H, W):
    """``map_out`` against float64 by the same rule.  The sampled set has to agree with float64's except where float64's
    determinant is within DET_MARGIN of 0 or its source coordinate within the bound of the source's border."""
    r64, r32 = image_map(cam, Hs, Ws, H, W, np.float64), image_map(cam, Hs, Ws, H, W, np.float32)
    out = np.asarray(m, np.float64)
    v64, v32, vg = r64["cls"] == IM_SAMPLED, r32["cls"] == IM_SAMPLED, ~np.isnan(out).any(-1)
    keep = v64 & vg
    err = float(np.abs(out[keep] - r64["map"][keep]).max()) if keep.any() else 0.0
    k32 = v64 & v32
    env = float(np.abs(r32["map"][k32].astype(np.float64) - r64["map"][k32]).max()) if k32.any() else 0.0
    floor = georef.PIXEL_FLOOR * max(1.0, float(np.abs(r64["map"][v64]).max()) if v64.any() else 1.0)
    b = georef.bound(floor, env)
    with np.errstate(invalid="ignore"):
        raw = r64["raw"]
        edge = np.minimum(np.minimum(np.abs(raw[..., 0]), np.abs(raw[..., 0] - (Ws - 1))),
                          np.minimum(np.abs(raw[..., 1]), np.abs(raw[..., 1] - (Hs - 1)))) <= b
        ex = (np.abs(r64["det"]) < DET_MARGIN) | edge
    differ = vg != v64
    return dict(err=err, env=env, floor=floor, bound=b, n_valid=int(keep.sum()), n_unexcused=int((differ & ~ex).sum()),
                n_excused=int((differ & ex).sum()), r64=r64, ok=err <= b and not (differ & ~ex).any())


def sensor_grid(Hs=HS, Ws=WS):
    """every integer pixel of the sensor -> (x, y) int32, row-major"""
    yy, xx = np.meshgrid(np.arange(Hs, dtype=np.int32), np.arange(Ws, dtype=np.int32), indexing="ij")
    return xx.reshape(-1), yy.reshape(-1)
