"""Numpy restatement of the event contrast and its gradient (include/ramp_hip.h ``ramp_event_contrast``) -- TEST
INFRASTRUCTURE ONLY.  Over tests/warpref.py and tests/interpref.py, with none of the kernel's structure (no tiles, no fixed
point, no partial sums):

    C(t), G = C(t_ref)^-1 C(t), d, P      as warpref.warp
    tau = float32(t - t_ref),  ds = d exp(lam)
    X1  = R_G P + t_G ds
    X2  = X1 + tau (v ds + w x X1)
    x'  = fx X2.x / X2.z + cx,  y' = fy X2.y / X2.z + cy        invalid as warpref.warp, with X2.z in the place of Z'
    I(u) = sum_k s_k b(u - x'_k)  (bilinear, neighbours outside the image dropped),  s_k = p_k or 1
    f   = (1 / P_n) sum_u (I(u) - mu)^2

``dtype=np.float64`` evaluates everything in double; ``dtype=np.float32`` the geometry (up to x', y' and the weights) with
the fp32 oracle and numpy float32, the image and every sum in double -- what the kernel does: its distance from float64 is
the rounding envelope of the GPU test.  ``gradient`` is the analytic derivative of f with respect to theta = (v, w, lam);
``compare`` the one check the GPU test and tests/test_contrastref_cpu.py use; the ``mistake`` keyword breaks the gradient on
purpose (every one of them has to be rejected by ``compare``).
"""
import numpy as np

import georef
import poseref
import splatref
import warpref

MISTAKES = ("nomean", "rotsign", "tausign", "nopol", "nolam", "unbiased")
GRAD_FLOOR = 1e-5            # x the sum of the absolute per-event terms of a component (PIXEL_FLOOR's role)


def _theta(theta, dtype):
    """theta in ``dtype``; taken as it is (the device reads float32: ``evaluator`` rounds first)"""
    return np.zeros(7, dtype) if theta is None else np.asarray(theta).reshape(7).astype(dtype)


def geometry(x, y, t, knots, times, t_ref, K, invdepth, H, W, theta=None, extrapolate=False, dtype=np.float64, mistake=None):
    """-> dict(xy [N,2] with NaN rows for invalid events, X1, X2, B = t_G ds [N,3], ds, tau [N]) in ``dtype``"""
    rays = warpref.event_rays(x, y, t, knots, times, t_ref, K, invdepth, H, W, extrapolate, dtype)
    if rays is None:
        N = np.asarray(x).size
        nan3 = np.full((N, 3), np.nan, dtype)
        return dict(xy=np.full((N, 2), np.nan, dtype), X1=nan3, X2=nan3, B=nan3, ds=nan3[:, 0], tau=nan3[:, 0])
    fin, tq, G, P, d, (fx, fy, cx, cy) = rays
    th = _theta(theta, dtype)
    v, w, lam = th[:3], th[3:6], th[6]
    tau = (tq - float(t_ref)).astype(np.float32).astype(dtype)
    if mistake == "tausign":
        tau = -tau
    with np.errstate(all="ignore"):
        ds = (d * np.exp(lam)).astype(dtype)
        B = (G[:, :3] * ds[:, None]).astype(dtype)
        X1 = (poseref.qrot(G[:, 3:], P) + B).astype(dtype)
        X2 = (X1 + tau[:, None] * (v[None, :] * ds[:, None] + np.cross(w[None, :], X1))).astype(dtype)
        Z = X2[:, 2]
        xy = np.stack([fx * (X2[:, 0] / Z) + cx, fy * (X2[:, 1] / Z) + cy], -1).astype(dtype)
        bad = ~fin | ~(Z > dtype(warpref.MIN_Z)) | ~np.isfinite(xy).all(-1)
    xy[bad] = np.nan
    return dict(xy=xy, X1=X1, X2=X2, B=B, ds=ds, tau=tau)


def _splat(xy, s, H, W):
    """the image in float64 from coordinates in their own dtype -> (I [H,W], per-event neighbour data)"""
    valid = ~np.isnan(xy).any(-1)
    xv, yv = np.where(valid, xy[:, 0], 0).astype(xy.dtype), np.where(valid, xy[:, 1], 0).astype(xy.dtype)
    ix, wx, inx = splatref.axis(xv, W, dtype=None)
    iy, wy, iny = splatref.axis(yv, H, dtype=None)
    img = np.zeros((H, W), np.float64)
    for jy in range(2):
        for jx in range(2):
            m = valid & inx[jx] & iny[jy]
            wgt = (wx[jx] * wy[jy]).astype(xy.dtype).astype(np.float64)     # one product in the geometry's dtype
            np.add.at(img, ((iy + jy)[m], (ix + jx)[m]), s[m] * wgt[m])
    return img, (valid, ix, iy, wx, wy, inx, iny)


def _signs(p, signed):
    p = np.asarray(p).astype(np.float64).reshape(-1)
    p = np.where(p == 0, -1.0, p)
    return p if signed else np.ones_like(p)


def contrast(x, y, t, p, knots, times, t_ref, K, invdepth, H, W, theta=None, signed=True, extrapolate=False, dtype=np.float64):
    """-> dict(variance, mean, sum_sq, image [H,W] float64, xy)"""
    g = geometry(x, y, t, knots, times, t_ref, K, invdepth, H, W, theta, extrapolate, dtype)
    img, _ = _splat(g["xy"], _signs(p, signed), H, W)
    mu = img.sum() / img.size
    return dict(variance=float(((img - mu) ** 2).sum() / img.size), mean=float(mu), sum_sq=float((img ** 2).sum()), image=img,
                xy=g["xy"])


def gradient(x, y, t, p, knots, times, t_ref, K, invdepth, H, W, theta=None, signed=True, extrapolate=False, dtype=np.float64,
             mistake=None):
    """-> (grad [7] float64, the sum of the absolute per-event terms [7]): the analytic derivative of ``contrast``'s variance,
    every term formed in float64 from the geometry in ``dtype``"""
    assert mistake is None or mistake in MISTAKES
    g = geometry(x, y, t, knots, times, t_ref, K, invdepth, H, W, theta, extrapolate, dtype, mistake)
    s = _signs(p, signed)
    img, (valid, ix, iy, wx, wy, inx, iny) = _splat(g["xy"], s, H, W)
    Pn = img.size
    mu = 0.0 if mistake == "nomean" else img.sum() / Pn
    N = len(s)
    gx, gy = np.zeros(N), np.zeros(N)
    for jy in range(2):
        for jx in range(2):
            m = valid & inx[jx] & iny[jy]
            dI = np.where(m, img[np.where(m, iy + jy, 0), np.where(m, ix + jx, 0)] - mu, 0.0)
            gx += dI * (1.0 if jx else -1.0) * wy[jy].astype(np.float64)
            gy += dI * (1.0 if jy else -1.0) * wx[jx].astype(np.float64)
    sk = np.ones(N) if mistake == "nopol" else s
    scale = 2.0 / (Pn - 1 if mistake == "unbiased" else Pn)
    fx, fy = float(np.float32(K[0])), float(np.float32(K[1]))
    X1, X2, B = (np.where(valid[:, None], g[k].astype(np.float64), 1.0) for k in ("X1", "X2", "B"))
    ds, tau = np.where(valid, g["ds"].astype(np.float64), 0.0), np.where(valid, g["tau"].astype(np.float64), 0.0)
    th = _theta(theta, dtype).astype(np.float64)
    v, w = th[:3], th[3:6]
    X, Y, Z = X2[:, 0], X2[:, 1], X2[:, 2]
    ga, gb = sk * gx * fx / Z, sk * gy * fy / Z
    gc = -(sk * gx * fx * X + sk * gy * fy * Y) / (Z * Z)
    dfdX = np.where(valid[:, None], np.stack([ga, gb, gc], -1), 0.0)
    cr = np.cross(X1, dfdX)                                             # g . (e_i x X1) = (X1 x g)_i
    if mistake == "rotsign":
        cr = -cr
    L = B if mistake == "nolam" else B + tau[:, None] * (v[None, :] * ds[:, None] + np.cross(w[None, :], B))
    terms = np.concatenate([(tau * ds)[:, None] * dfdX, tau[:, None] * cr, (dfdX * L).sum(-1, keepdims=True)], -1) * scale
    return terms.sum(0), np.abs(terms).sum(0)


def compare(grad_gpu, *args, **kw):
    """the GPU test's check of one gradient.  Per component: err = |grad - float64 restatement|, env = the float32-geometry
    restatement's own error against float64 on the same inputs, floor = GRAD_FLOOR x the sum of the absolute per-event terms
    (the natural scale of a cancelling sum), bound = georef.bound(floor, env)"""
    g64, a64 = gradient(*args, dtype=np.float64, **kw)
    g32, _ = gradient(*args, dtype=np.float32, **kw)
    out = np.asarray(grad_gpu, np.float64).reshape(7)
    err, env, floor = np.abs(out - g64), np.abs(g32 - g64), GRAD_FLOOR * a64
    bound = np.array([georef.bound(f, e) for f, e in zip(floor, env)])
    return dict(err=err, env=env, floor=floor, bound=bound, ref=g64, abs_terms=a64,
                ok=bool(np.isfinite(out).all() and (err <= bound).all()))


def align(evaluate, correction=None, free=(0, 0, 0, 1, 1, 1, 0), step=0.05, iters=20):
    """the loop of ``ops.event_align`` over ``evaluate(theta) -> (variance, grad)``, restated: the direction is the gradient
    masked by ``free`` over its norm; the step length starts at ``step``, doubles after an accepted step, halves up to 8
    times while the contrast does not rise; stops after ``iters`` accepted steps or when a step fails 8 halvings"""
    theta = np.zeros(7) if correction is None else np.asarray(correction, np.float64).reshape(7).copy()
    mask = np.asarray(free, np.float64)
    f, g = evaluate(theta)
    f0, history, length = f, [], float(step)
    while len(history) < iters:
        gm = np.asarray(g, np.float64) * mask
        norm = float(np.sqrt((gm * gm).sum()))
        if not (0.0 < norm < np.inf):
            break
        for _ in range(9):
            trial = theta + length * gm / norm
            ft, gt = evaluate(trial)
            if ft > f:
                break
            length *= 0.5
        else:
            break
        theta, f, g = trial, ft, gt
        history.append(f)
        length *= 2.0
    return dict(correction=theta, variance=f, variance0=f0, history=history)


def evaluator(x, y, t, p, knots, times, t_ref, K, invdepth, H, W, signed=True, dtype=np.float64):
    """``evaluate`` for ``align`` over this restatement; theta is rounded to float32 first, as the device reads it"""
    def evaluate(theta):
        th = np.asarray(theta, np.float32)
        c = contrast(x, y, t, p, knots, times, t_ref, K, invdepth, H, W, th, signed, dtype=dtype)
        return c["variance"], gradient(x, y, t, p, knots, times, t_ref, K, invdepth, H, W, th, signed, dtype=dtype)[0]
    return evaluate


# ---------------------------------------------------------------------------------------------------------------- scenes
ALIGN_H, ALIGN_W = 37, 53
ALIGN_K = np.array([40.0, 40.0, 26.0, 18.0], np.float32)
ALIGN_RATE = np.array([0.15, -0.10, 0.30])


def align_scene(seed=5, dots=40, per_dot=30):
    """events of a sharp random dot pattern seen under the constant rotation rate ALIGN_RATE: a dot at the ray P0 of the
    reference frame is seen at time tau on the ray P with (I + tau [w]_x) P ~ P0, so the correction w = ALIGN_RATE collapses
    every dot's events onto one point.  Identity trajectory (two knots at -1, 1), t_ref = 0, d = 0.
    -> dict(x, y, t, p, knots, times, t_ref, K, invdepth, H, W)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = ALIGN_K.astype(np.float64)
    u0, v0 = rng.uniform(6, ALIGN_W - 7, dots), rng.uniform(6, ALIGN_H - 7, dots)
    pol = rng.choice([-1, 1], dots)
    k = np.repeat(np.arange(dots), per_dot)
    tau = rng.uniform(-0.5, 0.5, len(k))
    P0 = np.stack([(u0[k] - cx) / fx, (v0[k] - cy) / fy, np.ones(len(k))], -1)
    wx, wy, wz = ALIGN_RATE
    Wx = np.array([[0, -wz, wy], [wz, 0, -wx], [-wy, wx, 0]])
    P = np.stack([np.linalg.solve(np.eye(3) + ti * Wx, Pi) for ti, Pi in zip(tau, P0)])
    x, y = fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy
    knots = np.tile(np.array([0, 0, 0, 0, 0, 0, 1], np.float32), (2, 1))
    return dict(x=x.astype(np.float32), y=y.astype(np.float32), t=tau, p=pol[k].astype(np.int8), knots=knots,
                times=np.array([-1.0, 1.0]), t_ref=0.0, K=ALIGN_K, invdepth=0.0, H=ALIGN_H, W=ALIGN_W)
