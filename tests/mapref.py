"""Float64 restatement of the map with its uncertainty (include/ramp_hip.h ``ramp_ba_map_covariance`` and
``ramp_map_select``), numpy only, on top of ``covref.covariance`` (cov = S^-1, Q, the E rows, depth_var).

From the joint inverse of the damped system the step is solved with, for patch k with E row e_k:

    cov(xi, z_k) = -Q_k S^-1 e_k                      (pose-depth), c = its six rows of the patch's source frame i
    X_w = R' (r / d - t),  r = ((x - cx) / fx, (y - cy) / fy, 1),  T_i = (t, R) world-to-camera, intrinsics row 0
    J_p = R' [ -I | [r / d]x ]   (left perturbation T <- Exp(xi) T, xi = (translation, rotation))
    J_d = -R' r / d^2            (d <- d + z)
    Sigma_k = J_p cov_ii J_p' + depth_var_k J_d J_d' + (J_p c) J_d' + J_d (J_p c)'

and Sigma_k = depth_var_k J_d J_d', c = 0 where frame i is not a free pose.  ``dtype=np.float32`` runs the same statements
in float32 on covref's float32 result: its distance from float64 is the rounding envelope of the GPU test.  The keyword
switches of ``map_covariance`` break the restatement on purpose (tests/test_mapref_cpu.py)."""
import numpy as np

import covref

FLOOR, CAP = covref.FLOOR, 5e-3
SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))        # point_cov's six entries: xx, xy, xz, yy, yz, zz


def quat_R(q):
    """rotation matrix of the unit quaternion (x, y, z, w)"""
    x, y, z, w = q / np.sqrt(np.sum(q * q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], q.dtype)


def skew(p):
    return np.array([[0, -p[2], p[1]], [p[2], 0, -p[0]], [-p[1], p[0], 0]], p.dtype)


def point_of(R, t, ray, d):
    """X_w = R' (ray / d - t)"""
    return R.T @ (ray / d - t)


def jacobians(R, ray, d, right=False, swap=False, jd_no_d2=False, t=None):
    """J_p [3, 6], J_d [3] of ``point_of`` -- the keywords are the mutations"""
    T = ray.dtype.type
    pc = ray / d
    if right:                   # T <- T Exp(xi): X_w <- (I - [phi]x)(X_w - tau)
        Jp = np.concatenate([-np.eye(3, dtype=T), skew(point_of(R, t, ray, d))], 1)
    else:
        Jp = R.T @ np.concatenate([-np.eye(3, dtype=T), skew(pc)], 1)
    if swap:
        Jp = np.concatenate([Jp[:, 3:], Jp[:, :3]], 1)
    Jd = -(R.T @ ray) / (T(1) if jd_no_d2 else d * d)
    return Jp.astype(T), Jd.astype(T)


def se3_exp(xi):
    """(dR, dt) of Exp(xi), xi = (tau, phi), float64"""
    tau, phi = xi[:3], xi[3:]
    th = np.sqrt(phi @ phi)
    K = skew(phi)
    if th < 1e-12:
        return np.eye(3) + K, tau + 0.5 * K @ tau
    a, b, c = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
    return np.eye(3) + a * K + b * K @ K, (np.eye(3) + b * K + c * K @ K) @ tau


def _sources(s):
    """per sorted unique patch: its source frame (the ii of its factors) and its valid-factor count needs the gate"""
    kk, ii = np.asarray(s["kk"], np.int64), np.asarray(s["ii"], np.int64)
    uk, first = np.unique(kk, return_index=True)
    return uk, ii[first]


def map_covariance(s, t0, t1, dtype=np.float64, cross=1.0, right=False, swap=False, jd_no_d2=False, ref=None):
    """dict(point [n_patches, 3], point_cov [n_patches, 6], pose_depth_cov [n_patches, 6] (NaN where a patch has no factor),
    n_obs [n_patches] (0 there), uk, cov: covref.covariance's dict) in ``dtype``.  Mutations: ``cross`` scales the pose-depth
    term (0: dropped, -1: the opposite sign), ``right``: right instead of left perturbation, ``swap``: rotation and
    translation columns exchanged, ``jd_no_d2``: J_d without the 1 / d^2."""
    T = dtype
    r = ref if ref is not None else covref.covariance(s, t0, t1, T)
    cov, Q, Em, dv = r["cov"], r["Q"], r["E"], r["depth_var"]
    uk, src = _sources(s)
    assert np.array_equal(uk, r["uk"])
    npat = np.asarray(s["patches"]).shape[0]
    poses, pat = np.asarray(s["poses"], T), np.asarray(s["patches"], T)
    fx, fy, cx, cy = np.asarray(s["intr"], T).reshape(-1, 4)[0]
    point = np.full((npat, 3), np.nan, T)
    pcov = np.full((npat, 6), np.nan, T)
    pdc = np.full((npat, 6), np.nan, T)
    n_obs = np.zeros(npat, np.int32)
    np.add.at(n_obs, np.asarray(s["kk"], np.int64), r["valid"].astype(np.int32))
    SE = (cov @ Em).astype(T) if t1 > t0 else None
    for g, (k, i) in enumerate(zip(uk, src)):
        R, t = quat_R(poses[i, 3:]), poses[i, :3]
        d = pat[k, 2, 1, 1]
        ray = np.array([(pat[k, 0, 1, 1] - cx) / fx, (pat[k, 1, 1, 1] - cy) / fy, 1], T)
        point[k] = point_of(R, t, ray, d)
        Jp, Jd = jacobians(R, ray, d, right=right, swap=swap, jd_no_d2=jd_no_d2, t=t)
        S = (np.outer(Jd, Jd) * dv[k]).astype(T)
        c = np.zeros(6, T)
        if t0 <= i < t1:
            a = 6 * (i - t0)
            c = (T(cross) * (-Q[g] * SE[a:a + 6, g])).astype(T)
            m = Jp @ c
            S = (S + Jp @ cov[a:a + 6, a:a + 6] @ Jp.T + np.outer(m, Jd) + np.outer(Jd, m)).astype(T)
        pcov[k] = [S[x, y] for x, y in SYM]
        pdc[k] = c
    return dict(point=point, point_cov=pcov, pose_depth_cov=pdc, n_obs=n_obs, uk=uk, src=src, cov=r)


def errors(out_pcov, out_pdc, ref64):
    """point_cov: the largest entry difference per point over that point's float64 trace, maximised over the points;
    pose_depth_cov: the largest difference norm over the largest float64 norm of the case (no free source frame: every entry
    must be zero -- any difference is infinite)"""
    uk = ref64["uk"]
    p64, c64 = ref64["point_cov"][uk], ref64["pose_depth_cov"][uk]
    po, co = np.asarray(out_pcov, np.float64)[uk], np.asarray(out_pdc, np.float64)[uk]
    tr = p64[:, 0] + p64[:, 3] + p64[:, 5]
    e_p = float((np.abs(po - p64).max(1) / tr).max())
    dn, cn = np.linalg.norm(co - c64, axis=1).max(), np.linalg.norm(c64, axis=1).max()
    e_c = float(dn / cn) if cn > 0 else (0.0 if dn == 0 else np.inf)
    return dict(point_cov=e_p, pose_depth_cov=e_c)


def compare(out_pcov, out_pdc, ref64, ref32, floor=FLOOR, cap=CAP):
    """covref.compare's rule on the map's two error figures: error against float64 <= max(floor, 4 x the float32
    restatement's own error), and that envelope itself <= cap.  Returns (ok, report): report[name] = (error, bound, envelope)"""
    e, env = errors(out_pcov, out_pdc, ref64), errors(ref32["point_cov"], ref32["pose_depth_cov"], ref64)
    rep, ok = {}, True
    for k in ("point_cov", "pose_depth_cov"):
        bound = max(floor, 4 * env[k])
        rep[k] = (e[k], bound, env[k])
        ok = ok and bool(np.isfinite(e[k])) and e[k] <= bound and env[k] <= cap
    return ok, rep


def select(point_cov, depth_var, d, n_obs, max_sigma=None, max_rel_depth_sigma=None, min_obs=0):
    """ramp_map_select in numpy, float32 statement for statement: the ascending indices of the points with six finite
    covariance entries, sqrt((xx + yy) + zz) <= max_sigma, sqrt(depth_var) / d <= max_rel_depth_sigma and n_obs >= min_obs;
    None / +inf (min_obs: 0) switches a criterion off"""
    pc = np.asarray(point_cov, np.float32).reshape(-1, 6)
    dv, d, n_obs = np.asarray(depth_var, np.float32), np.asarray(d, np.float32), np.asarray(n_obs)
    inf = np.float32(np.inf)
    ms = inf if max_sigma is None else np.float32(max_sigma)
    mr = inf if max_rel_depth_sigma is None else np.float32(max_rel_depth_sigma)
    with np.errstate(all="ignore"):
        fin = np.isfinite(pc).all(1)
        sig = np.sqrt((pc[:, 0] + pc[:, 3]) + pc[:, 5])
        rel = np.sqrt(dv) / d
        hit = fin & ((ms == inf) | (sig <= ms)) & ((mr == inf) | (rel <= mr)) & ((min_obs <= 0) | (n_obs >= min_obs))
    return np.nonzero(hit)[0].astype(np.int32)
