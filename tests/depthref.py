"""Numpy restatement of the inverse-depth map (include/ramp_hip.h ``ramp_invdepth_map``) -- TEST INFRASTRUCTURE ONLY.

Two stages, each in float64 (the reference) or float32 (the formulas' own rounding, in the kernel's statement order: the
envelope of the GPU test's bound).  No tiles, no chunks, no culling.

(a) ``project``: per selected patch k of frame i = k // M

        G  = cam^-1 T_i^-1                          cam camera-to-world, T_i world-to-camera
        X' = R_G ((x - cx) / fx, (y - cy) / fy, 1) + t_G d
        u  = scale (fx X'/Z' + cx),  v likewise,  d' = d / Z'

    -> records [K,4] (u, v, d', c) and the class of every patch: 0 contributing, 2 depth or confidence not finite or <= 0,
    3 Z' <= MIN_Z or a projection that is not finite, 4 out of reach.  Rejected: weight 0 ((NaN, NaN, NaN, 0) for 2 and 3).

(b) ``regress``: per integer pixel

        s_k = 1 - ((x - u_k)^2 + (y - v_k)^2) / R^2,  w_k = c_k max(s_k, 0)^2
        invdepth = (pw prior + sum w_k d'_k) / (pw + sum w_k),  weight = sum w_k

    a pixel without data: the prior when pw > 0, else NaN.  float32: 1 / R^2 is formed once and multiplied, the sums run over
    the records in order, no FMA.

The ``mistake`` keywords break the restatement on purpose (tests/test_depthref_cpu.py: each has to be rejected).
"""
import numpy as np

import georef
import poseref

MIN_Z = 0.2                  # RAMP_WARP_MIN_Z
MAP_FLOOR = 1e-5             # x the largest d' (the map) / the largest weight
Z_MARGIN = 1e-4              # rejected sets may differ where float64's Z' is this close to MIN_Z
PROJECT_MISTAKES = ("fxfy", "inverse", "dz", "noscale")
REGRESS_MISTAKES = ("unsquared", "noprior_den")


def project(poses, patches, intr, cam, ids, M, H, W, R, scale=1.0, conf=None, conf_is_variance=False, dtype=np.float64,
            mistake=None):
    """-> (records [K,4] in ``dtype``, cls [K] int, Z' [K]).  Inputs are read as float32 (what the kernel reads)"""
    assert mistake is None or mistake in PROJECT_MISTAKES
    poses = np.asarray(poses, np.float32).reshape(-1, 7)
    P = patches.shape[-1]
    patches = np.asarray(patches, np.float32).reshape(-1, 3, P, P)
    ids = np.asarray(ids, np.int64).reshape(-1)
    K = len(ids)
    rec = np.zeros((K, 4), dtype)
    cls = np.zeros(K, np.int64)
    if K == 0:
        return rec, cls, np.zeros(0, dtype)
    cam = np.asarray(cam, np.float32).reshape(1, 7)
    ctr = patches[ids][:, :, P // 2, P // 2].astype(dtype)
    x, y, d = ctr[:, 0], ctr[:, 1], ctr[:, 2]
    c = np.ones(K, dtype)
    if conf is not None:
        cf = np.asarray(conf, np.float32).reshape(-1)[ids]
        with np.errstate(all="ignore"):
            c = ((np.float32(1.0) / cf) if conf_is_variance else cf).astype(dtype)      # (1 / conf is formed in float32)
    _, _, inv, mul = poseref.se3_ops(dtype)
    T = poses[ids // M].astype(dtype)
    C = np.repeat(cam.astype(dtype), K, 0)
    with np.errstate(all="ignore"):
        G = np.asarray(mul(T, C) if mistake == "inverse" else mul(inv(C), inv(T)), dtype)
        fx, fy, cx, cy = (dtype(v) for v in np.asarray(intr, np.float32).reshape(-1)[:4])
        ux, uy = (fy, fx) if mistake == "fxfy" else (fx, fy)
        sc = dtype(1.0 if mistake == "noscale" else np.float32(scale))
        r = np.stack([(x - cx) / ux, (y - cy) / uy, np.ones(K, dtype)], -1)
        X = poseref.qrot(G[:, 3:], r) + G[:, :3] * d[:, None]
        Z = X[:, 2]
        u = sc * (fx * (X[:, 0] / Z) + cx)
        v = sc * (fy * (X[:, 1] / Z) + cy)
        dp = d * Z if mistake == "dz" else d / Z
        bad_d = ~(np.isfinite(d) & (d > 0) & np.isfinite(c) & (c > 0))
        bad_z = ~bad_d & (~(Z > dtype(MIN_Z)) | ~np.isfinite(u) | ~np.isfinite(v) | ~np.isfinite(dp) | ~np.isfinite(cam).all())
        Rr = dtype(np.float32(R))
        far = ~bad_d & ~bad_z & ((u < -Rr) | (u > dtype(W - 1) + Rr) | (v < -Rr) | (v > dtype(H - 1) + Rr))
    cls[bad_d], cls[bad_z], cls[far] = 2, 3, 4
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = u, v, dp, c
    rec[bad_d | bad_z, :3] = np.nan
    rec[cls != 0, 3] = 0
    return rec, cls, np.where(bad_d, np.nan, Z).astype(dtype)


def prior_weight(prior, weight, relative, dtype=np.float64):
    """pw as the kernel forms it: ``weight``, or ``weight / prior^2`` (in float32 for the float32 form); 0 stays 0"""
    if weight == 0:
        return dtype(0)
    if not relative:
        return dtype(np.float32(weight))
    p = dtype(np.float32(prior))
    with np.errstate(all="ignore"):
        return dtype(np.float32(weight)) / (p * p)


def regress(records, prior, pw, R, H, W, dtype=np.float64, mistake=None):
    """records [K,4] (rows of weight 0 or NaN weight contribute nothing) -> dict(invdepth [H,W], weight [H,W], smax [H,W]:
    the largest s_k over the contributing records, -inf without one), all in ``dtype``"""
    assert mistake is None or mistake in REGRESS_MISTAKES
    rec = np.asarray(records).astype(dtype).reshape(-1, 4)
    rec = rec[rec[:, 3] > 0]
    gy, gx = np.meshgrid(np.arange(H, dtype=dtype), np.arange(W, dtype=dtype), indexing="ij")
    S0, S1 = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
    smax = np.full((H, W), -np.inf, dtype)
    one, zero = dtype(1), dtype(0)
    Rr = dtype(np.float32(R))
    inv_r2 = one / (Rr * Rr)
    for u, v, dp, c in rec:
        dx, dy = gx - u, gy - v
        r2 = dx * dx + dy * dy
        s = one - (r2 * inv_r2 if dtype == np.float32 else r2 / (Rr * Rr))
        t = np.maximum(s, zero)
        w = c * (t if mistake == "unsquared" else t * t)
        S0 += w
        S1 += w * dp
        np.maximum(smax, s, out=smax)
    pw, pr = dtype(pw), dtype(np.float32(prior))
    with np.errstate(all="ignore"):
        den = S0 if mistake == "noprior_den" else pw + S0
        val = ((pw * pr if pw > 0 else zero) + S1) / den
        nodata = pr if (pw > 0 and np.isfinite(pw)) else dtype(np.nan)
        out = np.where(S0 == 0, nodata, val).astype(dtype)
        if pw != 0 and not (pw > 0 and np.isfinite(pw)):
            out[:] = np.nan
    return dict(invdepth=out, weight=S0, smax=smax)


# ------------------------------------------------------------------------------------------------------------ the checks
def compare_records(rec_gpu, poses, patches, intr, cam, ids, M, H, W, R, scale=1.0, conf=None, conf_is_variance=False):
    """the GPU test's check of the records of one call against float64: u, v by georef.bound(PIXEL_FLOOR x largest
    |coordinate|, env), d' by the same with the largest d'; env = the float32 restatement's own error.  The rejected sets
    (weight 0) have to agree except where float64's Z' is within Z_MARGIN of MIN_Z."""
    args = (poses, patches, intr, cam, ids, M, H, W, R, scale, conf, conf_is_variance)
    r64, c64, z64 = project(*args, dtype=np.float64)
    r32, c32, _ = project(*args, dtype=np.float32)
    out = np.asarray(rec_gpu, np.float64).reshape(-1, 4)
    live_g, live_64, live_32 = out[:, 3] > 0, c64 == 0, c32 == 0
    with np.errstate(invalid="ignore"):
        edge = np.abs(z64 - MIN_Z) < Z_MARGIN
    sets_ok = bool(((live_g == live_64) | edge).all())
    keep, k32 = live_g & live_64, live_32 & live_64
    res = dict(sets_ok=sets_ok, n_live=int(keep.sum()))
    ok = sets_ok
    for name, cols in (("uv", slice(0, 2)), ("d", slice(2, 3)), ("c", slice(3, 4))):
        err = float(np.abs(out[keep, cols] - r64[keep, cols]).max()) if keep.any() else 0.0
        env = float(np.abs(r32[k32, cols].astype(np.float64) - r64[k32, cols]).max()) if k32.any() else 0.0
        big = float(np.abs(r64[live_64, cols]).max()) if live_64.any() else 1.0
        floor = georef.PIXEL_FLOOR * (max(1.0, big) if name == "uv" else big)
        res[name] = dict(err=err, env=env, floor=floor, bound=georef.bound(floor, env))
        ok = ok and np.isfinite(err) and err <= res[name]["bound"]
    res["ok"] = bool(ok)
    return res


def compare_map(inv_gpu, wgt_gpu, records, prior, pw, R, H, W):
    """the check of a map with pw > 0 against the float64 regression of the call's OWN records: floor MAP_FLOOR x the
    largest d' (and the prior), env = the float32 restatement against float64; the weight likewise, relative to its largest
    entry"""
    r64 = regress(records, prior, pw, R, H, W, np.float64)
    r32 = regress(records, prior, pw, R, H, W, np.float32)
    rec = np.asarray(records, np.float64).reshape(-1, 4)
    live = rec[:, 3] > 0
    big_d = max(float(rec[live, 2].max()) if live.any() else 0.0, abs(float(prior)))
    big_w = float(r64["weight"].max())
    res, ok = {}, True
    for name, out, scale in (("invdepth", inv_gpu, big_d), ("weight", wgt_gpu, big_w)):
        out = np.asarray(out, np.float64)
        nan_ok = bool(np.array_equal(np.isnan(out), np.isnan(r64[name])))
        fin = np.isfinite(r64[name]) & np.isfinite(out)
        err = float(np.abs(out - r64[name])[fin].max()) if fin.any() else 0.0
        f32 = np.isfinite(r64[name]) & np.isfinite(r32[name])
        env = float(np.abs(r32[name].astype(np.float64) - r64[name])[f32].max()) if f32.any() else 0.0
        floor = MAP_FLOOR * scale
        res[name] = dict(err=err, env=env, floor=floor, bound=georef.bound(floor, env), nan_ok=nan_ok)
        ok = ok and nan_ok and err <= res[name]["bound"]
    res["ok"] = bool(ok)
    return res
