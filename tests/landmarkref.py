"""Float64 restatement of the event landmarks (include/ramp_hip.h ``ramp_event_landmarks``) -- TEST INFRASTRUCTURE ONLY.

Plain numpy with a Python loop per track and none of the kernel's structure (no sort, no scan, no waves): the events that are
observations, the landmarks in ascending id with their observations in (t, index) order, the midpoint solve, ``refine``
Gauss-Newton steps, the last pass, the classes and the status words.  The 3x3 Cholesky is written out in the header's order.

Two forms.  From EVENTS and a trajectory: the poses come from the pose kit (``interpref.interpolate``, float64 or the fp32
formulas) and the rays are formed in that dtype -- the reference of ``ev_ray``.  From the call's OWN RAYS: ``rays`` [N, 6] fp32
(centre, direction) as the call wrote them and ``quat`` [N, 4] fp32, the rotations ``ops.se3_interp`` gives at the events' time
stamps -- the same statements as the call's, hence the same bits, and the rays' first three words say so -- so that everything
behind the rays is held to the float64 algebra alone.

``mistake`` breaks the restatement on purpose (test_landmarkref_cpu.py: every one is rejected by ``compare`` on the GPU test's
streams)."""
import numpy as np

import interpref
import poseref

MIN_Z = 0.2                    # RAMP_WARP_MIN_Z
BAD_TIMES = 1
MISTAKES = ("w2c", "fxfy", "unnormalised", "alpha_clamp", "min_obs_off", "class_order", "cov_no_sigma", "parallax_mean",
            "first_by_index")
PER_LANDMARK = ("track", "point", "cov", "n_obs", "cls", "rms", "parallax", "span")
U = 2.0 ** -53


def chol(a):
    """a = (xx, xy, xz, yy, yz, zz) -> (factor, ok): the header's order; ok is False when a pivot is <= 0 or not finite"""
    with np.errstate(all="ignore"):
        ok = a[0] > 0 and np.isfinite(a[0])
        l00 = np.sqrt(a[0])
        l10, l20 = a[1] / l00, a[2] / l00
        p1 = a[3] - l10 * l10
        ok = ok and p1 > 0 and np.isfinite(p1)
        l11 = np.sqrt(p1)
        l21 = (a[4] - l20 * l10) / l11
        p2 = (a[5] - l20 * l20) - l21 * l21
        ok = ok and p2 > 0 and np.isfinite(p2)
        l22 = np.sqrt(p2)
    return (l00, l10, l11, l20, l21, l22, min(a[0], p1, p2)), bool(ok)


def chol_solve(f, b):
    l00, l10, l11, l20, l21, l22 = f[:6]
    with np.errstate(all="ignore"):
        y0 = b[0] / l00
        y1 = (b[1] - l10 * y0) / l11
        y2 = ((b[2] - l20 * y0) - l21 * y1) / l22
        x2 = y2 / l22
        x1 = (y1 - l21 * x2) / l11
        x0 = ((y0 - l10 * x1) - l20 * x2) / l00
    return np.array([x0, x1, x2])


def sym(a):
    return np.array([[a[0], a[1], a[2]], [a[1], a[3], a[4]], [a[2], a[4], a[5]]])


def unit(d):
    return d / np.sqrt((d[..., 0:1] * d[..., 0:1] + d[..., 1:2] * d[..., 1:2]) + d[..., 2:3] * d[..., 2:3])


def observations(x, y, t, track, times, extrapolate):
    """-> (class per event: 1 no track, 2 not finite, 3 outside the knots' range, 4 an observation)"""
    x, y, t = np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(t, np.float64)
    with np.errstate(invalid="ignore"):
        inside = (t >= times[0]) & (t <= times[-1])
    finite = np.isfinite(x) & np.isfinite(y) & np.isfinite(t)
    return np.where(np.asarray(track) < 0, 1, np.where(~finite, 2, np.where(inside | bool(extrapolate), 4, 3)))


def event_rays(x, y, t, knots, times, K, extrapolate=False, dtype=np.float64, mistake=None):
    """-> (rays [N, 6], quat [N, 4]) in ``dtype`` for finite events (others NaN): the pose kit's C(t) and d = q f"""
    x, y = np.asarray(x, np.float32).astype(dtype), np.asarray(y, np.float32).astype(dtype)
    K = np.asarray(K, np.float32).astype(dtype)
    t = np.asarray(t, np.float64)
    ok = np.isfinite(t)
    C, _ = interpref.interpolate(np.asarray(knots, np.float32), times, np.where(ok, t, times[0]),
                                 extrapolate and mistake != "alpha_clamp", dtype)
    C = np.asarray(C, dtype)
    if mistake == "w2c":
        C = np.stack([poseref.invert_pose(c) for c in C]).astype(dtype)
    fx, fy = (K[1], K[0]) if mistake == "fxfy" else (K[0], K[1])
    f = np.stack([(x - K[2]) / fx, (y - K[3]) / fy, np.ones_like(x)], -1)
    d = poseref.qrot(C[:, 3:], f)
    rays = np.concatenate([C[:, :3], d], 1)
    rays[~ok] = np.nan
    return rays, C[:, 3:]


def event_landmarks(x, y, t, track, knots, times, K, min_obs=3, refine=2, min_parallax=0.02, max_rms=2.0, sigma_px=1.0,
                    max_landmarks=None, extrapolate=False, rays=None, quat=None, mistake=None, want_cond=False):
    """the outputs of ``ramp_event_landmarks`` as a dict of numpy arrays in the call's dtypes (``point``, ``cov``, ``rms``,
    ``parallax``, ``residual`` and ``rays`` stay float64, unrounded); per-landmark arrays hold ``count`` rows.  ``want_cond``:
    also per landmark ``cond`` (the 2-norm condition of the last pass's H) and ``dist`` (|X - c0|), for the bound, ``zmin`` (the
    smallest Y.z of the last pass) and ``pivot`` (the smallest pivot of the midpoint system over n), for the gates' margins"""
    assert mistake is None or mistake in MISTAKES
    x32, y32 = np.asarray(x, np.float32), np.asarray(y, np.float32)
    t, track = np.asarray(t, np.float64), np.asarray(track, np.int64)
    times = np.ascontiguousarray(times, np.float64).reshape(-1)
    K32 = np.asarray(K, np.float32)
    N = len(t)
    L = max(1, min(N, 2 ** 20)) if max_landmarks is None else max_landmarks
    out = dict(index=np.full(N, -1, np.int32), residual=np.full((N, 2), np.nan), rays=np.full((N, 6), np.nan))
    status = np.zeros(8, np.int32)
    if N == 0:
        return {**out, **_empty(), "count": np.zeros(1, np.int32), "status": status}
    bad = not np.isfinite(times).all() or bool((np.diff(times) < 0).any())
    ev = observations(x32, y32, t, track, times, extrapolate)
    status[0] = BAD_TIMES if bad else 0
    status[1:4] = [(ev == c).sum() for c in (1, 2, 3)]
    if bad:
        return {**out, **_empty(), "count": np.zeros(1, np.int32), "status": status}
    obs = ev == 4
    status[4] = obs.sum()
    if rays is None:
        R6, Q = event_rays(x32, y32, t, knots, times, K32, extrapolate, mistake=mistake)
    else:
        R6, Q = np.asarray(rays, np.float32).astype(np.float64), np.asarray(quat, np.float32).astype(np.float64)
    out["rays"][obs] = R6[obs]
    fx, fy, cx, cy = K32.astype(np.float64)
    if mistake == "fxfy" and rays is not None:
        fx, fy = fy, fx
    xs, ys = x32.astype(np.float64), y32.astype(np.float64)
    ids = np.unique(track[obs])
    status[5], kept = len(ids), min(len(ids), L)
    status[6] = len(ids) - kept
    res = {k: [] for k in PER_LANDMARK + ("cond", "dist", "zmin", "pivot")}
    tt = np.where(t == 0.0, 0.0, t)
    for l, tid in enumerate(ids[:kept]):
        m = np.nonzero(obs & (track == tid))[0]
        m = m[np.lexsort((m, tt[m]))] if mistake != "first_by_index" else m
        n = len(m)
        out["index"][m] = l
        c, d = R6[m, :3], R6[m, 3:]
        u = d if mistake == "unnormalised" else unit(d)
        q = Q[m] / np.sqrt(((Q[m, 0:1] ** 2 + Q[m, 1:2] ** 2) + Q[m, 2:3] ** 2) + Q[m, 3:4] ** 2)
        qc = q * np.array([-1.0, -1.0, -1.0, 1.0])
        c0 = c[0]
        v = c - c0
        M = [1.0 - u[:, 0] * u[:, 0], -(u[:, 0] * u[:, 1]), -(u[:, 0] * u[:, 2]), 1.0 - u[:, 1] * u[:, 1], -(u[:, 1] * u[:, 2]),
             1.0 - u[:, 2] * u[:, 2]]
        A = np.array([e.sum() for e in M])
        b = np.array([((M[0] * v[:, 0] + M[1] * v[:, 1]) + M[2] * v[:, 2]).sum(), ((M[1] * v[:, 0] + M[3] * v[:, 1]) + M[4] * v[:, 2]).sum(),
                      ((M[2] * v[:, 0] + M[4] * v[:, 1]) + M[5] * v[:, 2]).sum()])
        against = unit(u.mean(0)) if mistake == "parallax_mean" else u[0]
        dot = (u[:, 0] * against[0] + u[:, 1] * against[1]) + u[:, 2] * against[2]
        par = float(np.arccos(np.clip(dot, -1.0, 1.0)).max())
        f, lin_ok = chol(A)
        X, cov, rms, zbad, cond, zmin = np.full(3, np.nan), np.full(6, np.nan), np.nan, False, np.nan, np.nan
        if lin_ok:
            X = c0 + chol_solve(f, b)
            for step in range(refine + 1):
                with np.errstate(all="ignore"):
                    Y = poseref.qrot(qc, X - c)
                    xn, yn = Y[:, 0] / Y[:, 2], Y[:, 1] / Y[:, 2]
                    rx, ry = (fx * xn + cx) - xs[m], (fy * yn + cy) - ys[m]
                    zero = np.zeros(n)
                    j0 = poseref.qrot(q, np.stack([fx / Y[:, 2], zero, -(fx * xn) / Y[:, 2]], -1))
                    j1 = poseref.qrot(q, np.stack([zero, fy / Y[:, 2], -(fy * yn) / Y[:, 2]], -1))
                    H = np.array([(j0[:, i] * j0[:, k] + j1[:, i] * j1[:, k]).sum() for i, k in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
                    g = np.array([(j0[:, i] * rx + j1[:, i] * ry).sum() for i in range(3)])
                    hf, h_ok = chol(H)
                    if step < refine:
                        Xn = X - chol_solve(hf, g)
                        if h_ok and np.isfinite(Xn).all():
                            X = Xn
                        continue
                    zbad, zmin = bool((~(Y[:, 2] > MIN_Z)).any()), float(Y[:, 2].min())
                    rms = float(np.sqrt((rx * rx + ry * ry).sum() / n))
                    out["residual"][m] = np.stack([rx, ry], -1)
                    s2 = 1.0 if mistake == "cov_no_sigma" else float(np.float32(sigma_px)) ** 2
                    if h_ok:
                        cols = [chol_solve(hf, e) for e in np.eye(3)]
                        cov = s2 * np.array([cols[0][0], cols[1][0], cols[2][0], cols[1][1], cols[2][1], cols[2][2]])
                        if np.isfinite(H).all():
                            w = np.linalg.eigvalsh(sym(H))
                            cond = float(w[-1] / w[0]) if w[0] > 0 else np.inf
        with np.errstate(all="ignore"):
            fin = bool(np.isfinite(X.astype(np.float32)).all() and np.isfinite(cov.astype(np.float32)).all())
        tests = [(1, n < min_obs + (1 if mistake == "min_obs_off" else 0)), (2, par < float(np.float32(min_parallax))), (3, not lin_ok),
                 (4, zbad), (5, rms > float(np.float32(max_rms))), (6, not fin), (7, True)]
        if mistake == "class_order":
            tests[0], tests[1] = tests[1], tests[0]
        cls = next(k for k, hit in tests if hit)
        status[7] += cls == 7
        for k, val in (("track", tid), ("point", X if cls == 7 else np.full(3, np.nan)), ("cov", cov if cls == 7 else np.full(6, np.nan)),
                       ("n_obs", n), ("cls", cls), ("rms", rms), ("parallax", par), ("span", (t[m[0]], t[m[-1]])), ("cond", cond),
                       ("dist", float(np.linalg.norm(X - c0))), ("zmin", zmin), ("pivot", f[6] / n)):
            res[k].append(val)
    shaped = _empty()
    if kept:
        shaped = dict(track=np.array(res["track"], np.int64), point=np.array(res["point"]).reshape(-1, 3), cov=np.array(res["cov"]).reshape(-1, 6),
                      n_obs=np.array(res["n_obs"], np.int32), cls=np.array(res["cls"], np.uint8), rms=np.array(res["rms"]),
                      parallax=np.array(res["parallax"]), span=np.array(res["span"], np.float64).reshape(-1, 2))
    if want_cond:
        shaped.update({k: np.array(res[k], np.float64) for k in ("cond", "dist", "zmin", "pivot")})
    return {**out, **shaped, "count": np.array([kept], np.int32), "status": status}


def _empty():
    return dict(track=np.zeros(0, np.int64), point=np.zeros((0, 3)), cov=np.zeros((0, 6)), n_obs=np.zeros(0, np.int32),
                cls=np.zeros(0, np.uint8), rms=np.zeros(0), parallax=np.zeros(0), span=np.zeros((0, 2)), cond=np.zeros(0), dist=np.zeros(0),
                zmin=np.zeros(0), pivot=np.zeros(0))


# ------------------------------------------------------------------------------------------------------------ the checks
EXACT = ("track", "n_obs", "cls", "span", "index", "count", "status")


def bounds(ref):
    """per landmark the second term of the bound without its scale: 64 n 2^-53 cond(H) (inf where H has no condition)"""
    with np.errstate(invalid="ignore"):
        return 64.0 * ref["n_obs"].astype(np.float64) * U * np.where(np.isfinite(ref["cond"]), ref["cond"], np.inf)


def compare(got, ref):
    """``got``: a call's outputs (per-landmark arrays cut to count); ``ref``: the restatement with ``want_cond``.  -> dict(exact:
    the names of the exact outputs that differ, nan: the names whose NaN pattern differs, ratio: the largest err / bound over
    ``point``, ``cov``, ``rms``, ``parallax`` and ``residual``).  The bound of an fp32 output v computed in float64: one fp32
    rounding, 2^-24 |v|, plus 64 n 2^-53 cond(H) scale with scale = |X - c0| for the point and the output's own magnitude
    otherwise -- per landmark the largest |entry| of cov, the rms for itself and for its residual rows, the parallax.  The
    parallax and the rms of a landmark without a condition (no H) are held to the rounding alone."""
    exact = []
    for k in EXACT:
        if k in got:
            g, r = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
            words = np.int64 if k == "span" else g.dtype
            if not (g.shape == r.shape and g.dtype == r.dtype and np.array_equal(g.view(words), r.view(words))):
                exact.append(k)
    nan, ratio = [], 0.0
    term = bounds(ref)
    idx = ref["index"]
    per_event = np.where(idx >= 0, term[np.maximum(idx, 0)] if len(term) else 0.0, 0.0)
    rms_ev = np.where(idx >= 0, ref["rms"][np.maximum(idx, 0)] if len(term) else 0.0, 0.0)
    scales = dict(point=(ref["dist"][:, None], term[:, None]), cov=(np.abs(ref["cov"]).max(-1, keepdims=True) if len(term) else ref["cov"], term[:, None]),
                  rms=(np.abs(ref["rms"]), np.where(np.isfinite(term), term, 0.0)),
                  parallax=(np.abs(ref["parallax"]), np.where(np.isfinite(term), term, 0.0)), residual=(np.abs(rms_ev)[:, None], per_event[:, None]))
    for k, (scale, tm) in scales.items():
        if k not in got:
            continue
        g, r = np.asarray(got[k], np.float64), np.asarray(ref[k], np.float64)
        if g.shape != r.shape or not np.array_equal(np.isnan(g), np.isnan(r)):
            nan.append(k)
            continue
        keep = ~np.isnan(r)
        with np.errstate(invalid="ignore", over="ignore"):
            bound = 2.0 ** -24 * np.abs(r) + np.where(np.isfinite(tm), tm, 0.0) * np.where(np.isfinite(scale), scale, 0.0) + 0.0 * r
            err = np.abs(g - r)
        if keep.any():
            e, b = err[keep], bound[keep]
            if not np.isfinite(e).all():
                ratio = np.inf
            else:
                ratio = max(ratio, float(np.where(e == 0, 0.0, e / np.maximum(b, 1e-300)).max()))
    return dict(exact=exact, nan=nan, ratio=ratio)


# ---------------------------------------------------------------------------------------------------------------- scenes
H0, W0 = 33, 37
K0 = np.array([30.0, 31.0, 18.0, 16.0], np.float32)


def trajectory(T, seed=0, t0=10.0, dt=0.5):
    """T hand-made knots: the camera moves sideways along a gentle arc and turns a little, always looking at the scene in front
    of it (z from 4 to 8), so that every track gets parallax; camera-to-world, fp32"""
    k = np.arange(T, dtype=np.float64)
    s = k / max(T - 1, 1)
    c = np.stack([3.0 * s - 1.5, 0.4 * np.sin(2.0 * s), 0.3 * s], 1)
    yaw = -0.25 * (s - 0.5)
    q = np.stack([0.02 * np.sin(3 * s), np.sin(yaw / 2), 0.0 * s, np.cos(yaw / 2)], 1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([c, q], 1).astype(np.float32), t0 + dt * k


def stream(sizes, T=9, seed=1, noise=0.3, bad=True, behind=0, spread=1.0):
    """events of len(sizes) tracks, track k with sizes[k] observations of one world point projected through the float64 geodesic
    of ``trajectory(T)`` at times spread over the knots' range, plus ``noise`` pixels of uniform error (so that no residual is
    tiny); ids are 7 k + 3, the events interleaved in time.  ``bad``: some events without a track, not finite and outside the
    range are mixed in.  ``behind``: that many tracks get one observation from a camera that looks away (class 4 comes from
    geometry, not noise).  -> dict(x, y, t, track, knots, times, K, points)"""
    rng = np.random.default_rng(seed)
    knots, times = trajectory(T)
    lo, hi = (times[0], times[-1]) if T > 1 else (times[0], times[0])
    xs, ys, ts, ids, pts = [], [], [], [], []
    for k, n in enumerate(sizes):
        P = np.array([rng.uniform(-1.0, 1.0), rng.uniform(-0.8, 0.8), rng.uniform(4.0, 8.0)])
        t = np.sort(rng.uniform(lo + 0.02 * (hi - lo), hi - 0.02 * (hi - lo), n)) if T > 1 else np.full(n, lo)
        if n > 1 and T > 1:
            a = 0.5 * (lo + hi) - 0.5 * spread * 0.96 * (hi - lo)
            t[0], t[-1] = a, a + spread * 0.96 * (hi - lo)
            t = np.sort(np.clip(t, t[0], t[-1]))
        C, _ = interpref.interpolate(knots, times, t, False, np.float64)
        Y = poseref.qrot(C[:, 3:] * np.array([-1.0, -1.0, -1.0, 1.0]), P - C[:, :3])
        xs.append(K0[0] * Y[:, 0] / Y[:, 2] + K0[2] + rng.uniform(-noise, noise, n))
        ys.append(K0[1] * Y[:, 1] / Y[:, 2] + K0[3] + rng.uniform(-noise, noise, n))
        ts.append(t), ids.append(np.full(n, 7 * k + 3, np.int64)), pts.append(P)
    x, y, t, track = (np.concatenate(v) if v else np.zeros(0) for v in (xs, ys, ts, ids))
    track = track.astype(np.int64)
    if bad and len(t) > 8:
        m = len(t)
        extra = max(4, m // 16)
        x = np.concatenate([x, rng.uniform(0, W0, 3 * extra)])
        y = np.concatenate([y, rng.uniform(0, H0, 3 * extra)])
        tb = rng.uniform(lo, hi, 3 * extra)
        tb[extra:2 * extra:2] = np.nan
        x[m + extra + 1:m + 2 * extra:2] = np.inf
        tb[2 * extra:] = np.where(np.arange(extra) % 2, hi + 1.0 + np.arange(extra), lo - 1.0 - np.arange(extra))
        t = np.concatenate([t, tb])
        track = np.concatenate([track, np.full(extra, -1, np.int64), rng.choice(track[:m], 2 * extra)])
    order = np.argsort(np.where(np.isfinite(t), t, lo), kind="stable")
    x, y, t, track = x[order].astype(np.float32), y[order].astype(np.float32), t[order], track[order]
    return dict(x=x, y=y, t=t, track=track, knots=knots, times=times, K=K0, points=np.array(pts).reshape(-1, 3))


EDGE_SIZES = (1, 2, 3, 63, 64, 65, 129, 5000)
PARAMS = dict(min_obs=3, refine=2, min_parallax=0.02, max_rms=2.0, sigma_px=0.75)


def cases():
    """name -> (scene, parameters): the streams of the GPU test"""
    out = {"edges T=9": (stream(EDGE_SIZES, 9, seed=1), PARAMS),
           "edges T=2, extrapolate": (stream(EDGE_SIZES[:7], 2, seed=2), dict(PARAMS, extrapolate=True)),
           "65 tracks": (stream([5 + k % 9 for k in range(65)], 9, seed=3), dict(PARAMS, refine=0)),
           "1000 tracks, cut": (stream([3 + k % 4 for k in range(1000)], 9, seed=4, bad=False), dict(PARAMS, max_landmarks=700, refine=1)),
           "one knot": (stream((3, 5), 1, seed=5, bad=False), PARAMS),
           "4097 knots": (stream((3, 64, 129), 4097, seed=6), dict(PARAMS, refine=4)),
           "short baselines": (stream([4] * 40, 9, seed=7, spread=0.001, noise=0.02, bad=False), PARAMS),
           "one track": (stream((17,), 9, seed=8, bad=False), PARAMS)}
    return out
