"""Float64 restatement of the continuous-time pose query (include/ramp_hip.h ``ramp_se3_interp``) -- TEST INFRASTRUCTURE ONLY.

Plain numpy over the oracle's SE3 formulas, with none of the kernel's structure (no tiles, no staging, no search loop):

    s     = the largest index with times[s] <= t, clamped to [0, T - 2]            (numpy.searchsorted, side "right")
    alpha = (t - times[s]) / (times[s + 1] - times[s])    in float64, rounded to fp32 once; a clamped segment of zero
            length: 0 for t < times[s], else 1; outside the range clamped to [0, 1] unless ``extrapolate``
    xi_s  = Log(X[s + 1] X[s]^-1)                         the left increment, (translation 3, rotation 3)
    X(t)  = Exp(alpha xi_s) X[s],     twist = xi_s / (times[s + 1] - times[s])   (zero for a zero-length segment, T == 1)

``dtype=np.float64`` evaluates the group operations with ``orc.se3_*_f64``; ``dtype=np.float32`` with the fp32 oracle (the
reference's float formulas): its distance from float64 is the rounding envelope of the GPU test.  The one check both the
GPU test and tests/test_interpref_cpu.py use is ``compare``.  The ``mistake`` keyword breaks the restatement on purpose
(test_interpref_cpu.py: every one of them has to be rejected by ``compare``).
"""
import numpy as np

import georef
import oracle as orc
import poseref

MISTAKES = ("right", "lower", "alpha32", "nlerp", "tlerp", "noclamp")


def segment_of(times, query, side="right"):
    T = len(times)
    return np.clip(np.searchsorted(times, query, side=side) - 1, 0, max(T - 2, 0))


def alpha_of(times, query, s, extrapolate=False, clamp=True):
    """float64 alpha and the segment lengths"""
    T = len(times)
    t0 = times[s]
    dt = times[s + 1] - t0 if T > 1 else np.zeros(len(query))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = np.where(dt > 0, (query - t0) / np.where(dt > 0, dt, 1.0), np.where(query < t0, 0.0, 1.0))
    if clamp and not extrapolate:
        a = np.clip(a, 0.0, 1.0)
    return a, dt


def interpolate(knots, times, query, extrapolate=False, dtype=np.float64, mistake=None):
    """-> (poses [Q,7], twist [Q,6]) in ``dtype``.  Time stamps that decrease or are not finite: everything NaN; a NaN query:
    that row NaN"""
    assert mistake is None or mistake in MISTAKES
    knots = np.ascontiguousarray(knots, dtype).reshape(-1, 7)
    times = np.ascontiguousarray(times, np.float64).reshape(-1)
    query = np.ascontiguousarray(query, np.float64).reshape(-1)
    T, Q = len(times), len(query)
    assert T >= 1 and len(knots) == T
    if not np.isfinite(times).all() or (np.diff(times) < 0).any():
        return np.full((Q, 7), np.nan, dtype), np.full((Q, 6), np.nan, dtype)
    nanq = np.isnan(query)
    q = np.where(nanq, times[0], query)
    exp, log, inv, mul = poseref.se3_ops(dtype)
    s = segment_of(times, q, side="left" if mistake == "lower" else "right")
    a, dt = alpha_of(times, q, s, extrapolate, clamp=mistake != "noclamp")
    if mistake == "alpha32" and T > 1:              # alpha formed in fp32 from the absolute times
        q32, t32, n32 = q.astype(np.float32), times[s].astype(np.float32), times[s + 1].astype(np.float32)
        with np.errstate(divide="ignore", invalid="ignore"):
            a32 = np.where(n32 > t32, (q32 - t32) / np.where(n32 > t32, n32 - t32, 1), np.where(q32 < t32, 0, 1))
        a = a32.astype(np.float64) if extrapolate else np.clip(a32.astype(np.float64), 0, 1)
    alpha = a.astype(np.float32).astype(dtype)[:, None]
    X0 = knots[s]
    if T > 1:
        xi = log(mul(knots[s + 1], inv(X0))).astype(dtype)
    else:
        xi = np.zeros((Q, 6), dtype)
    if mistake == "right":
        out = mul(X0, exp((alpha * xi).astype(dtype)))
    else:
        out = mul(exp((alpha * xi).astype(dtype)), X0)
    out = np.array(out, dtype)
    if mistake == "nlerp" and T > 1:                # normalised quaternion lerp (the translation stays the screw's)
        X1 = knots[s + 1]
        sign = np.where((X0[:, 3:] * X1[:, 3:]).sum(-1, keepdims=True) < 0, -1.0, 1.0).astype(dtype)
        qq = (1 - alpha) * X0[:, 3:] + alpha * sign * X1[:, 3:]
        out[:, 3:] = qq / np.sqrt((qq * qq).sum(-1, keepdims=True))
    if mistake == "tlerp" and T > 1:                # the V matrix dropped: the rotation's geodesic, the translation's chord
        out[:, :3] = (1 - alpha) * X0[:, :3] + alpha * knots[s + 1][:, :3]
    with np.errstate(divide="ignore", invalid="ignore"):
        tw = np.where(dt[:, None] > 0, xi.astype(np.float64) / np.where(dt > 0, dt, 1.0)[:, None], 0.0).astype(np.float32)
    tw = tw.astype(dtype)
    out[nanq] = np.nan
    tw[nanq] = np.nan
    return out, tw


def floor_of(knots):
    """georef.FLOOR["log"] x max(1, largest |translation|)"""
    k = np.asarray(knots, np.float64).reshape(-1, 7)
    return georef.FLOOR["log"] * max(1.0, float(np.abs(k[:, :3]).max()) if k.size else 1.0)


def compare(out, knots, times, query, extrapolate=False, twist=None):
    """the GPU test's check of one launch: dict(err, env, bound, ok) for the poses and, with ``twist``, (tw_err, tw_env,
    tw_bound).  err: largest element difference of ``out`` from the float64 restatement (quaternions up to sign); env: the
    fp32 restatement's own; bound: georef.bound(floor_of(knots), env).  Twists: the same rule with every row's difference
    multiplied by its segment's length (the floor divided by the length)."""
    knots = np.ascontiguousarray(knots, np.float32)
    r64, t64 = interpolate(knots, times, query, extrapolate, np.float64)
    r32, t32 = interpolate(knots, times, query, extrapolate, np.float32)
    floor = floor_of(knots)
    keep = ~np.isnan(r64).any(-1)
    out = np.asarray(out)
    nan_ok = bool(np.isnan(out[~keep]).all())       # NaN rows are NaN, all of them
    err = georef.pose_err(out[keep], r64[keep]) if np.isfinite(out[keep]).all() else float("inf")
    env = georef.pose_err(r32[keep], r64[keep])
    res = dict(err=err, env=env, floor=floor, bound=georef.bound(floor, env))
    res["ok"] = nan_ok and err <= res["bound"]
    if twist is not None:
        times = np.ascontiguousarray(times, np.float64).reshape(-1)
        q = np.where(np.isnan(query), times[0], np.asarray(query, np.float64).reshape(-1))
        _, dt = alpha_of(times, q, segment_of(times, q))
        w = np.where(dt > 0, dt, 1.0)[keep, None]
        tw = np.asarray(twist, np.float64)
        res["tw_err"] = float((np.abs(tw[keep] - t64[keep]) * w).max()) if keep.any() else 0.0
        res["tw_env"] = float((np.abs(t32[keep].astype(np.float64) - t64[keep]) * w).max()) if keep.any() else 0.0
        res["tw_bound"] = georef.bound(floor, res["tw_env"])
        res["tw_ok"] = bool(np.isnan(tw[~keep]).all()) and bool(np.isfinite(tw[keep]).all()) and res["tw_err"] <= res["tw_bound"]
    return res


# ---------------------------------------------------------------------------------------------------------------- scenes
def rand_pose(rng, k, scale=1.0):
    q = rng.standard_normal((k, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return np.concatenate([rng.uniform(-1, 1, (k, 3)) * scale, q], 1)


def pair_scene(seed, n, angle, scale):
    """n independent segments as 2n knots at times 0, 1, 2, ...: segment 2i -> 2i + 1 turns by ``angle`` rad about a random
    axis and moves by a random vector of size ``scale`` (X[2i+1] = Exp(xi) X[2i] in float64, rounded to fp32); the segments
    in between join unrelated poses and are not queried.  Queries of segment i at alpha: 2i + alpha"""
    rng = np.random.default_rng(seed)
    X0 = rand_pose(rng, n, scale)
    ax = rng.standard_normal((n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    xi = np.concatenate([rng.uniform(-1, 1, (n, 3)) * scale, ax * angle], 1)
    X1 = orc.se3_mul_f64(orc.se3_exp_f64(xi), X0)
    knots = np.empty((2 * n, 7))
    knots[0::2], knots[1::2] = X0, X1
    return knots.astype(np.float32), np.arange(2 * n, dtype=np.float64)


def walk_scene(seed, T, step=(0.05, 0.03, 0.04, 0.02, 0.03, 0.02), t0=0.0, dt=1.0):
    """T knots on a smooth random walk (a slowly varying twist, integrated), times t0 + k dt"""
    rng = np.random.default_rng(seed)
    v = np.cumsum(rng.normal(0, 0.2, (T, 6)), 0) / np.sqrt(np.arange(1, T + 1))[:, None] + rng.normal(0, 1, 6)
    X = np.zeros((T, 7))
    X[0] = rand_pose(rng, 1)[0]
    for k in range(1, T):
        X[k] = orc.se3_mul_f64(orc.se3_exp_f64((v[k] * np.asarray(step))[None]), X[k - 1:k])[0]
    return X.astype(np.float32), t0 + dt * np.arange(T, dtype=np.float64)
