"""Numpy restatement of the IMU entries (include/ramp_hip.h ``ramp_imu_preintegrate`` / ``ramp_imu_align``) -- TEST
INFRASTRUCTURE ONLY.  It does NOT share the kernel's structure: rotations are 3 x 3 matrices (the kernel composes
quaternions), the sub-intervals of an interval are composed one after the other from the left (the kernel reduces chunks of 64
by a shuffle tree), the breakpoints come from ``searchsorted``, the sums run in index order and the systems are solved by
``numpy.linalg.solve``.  Every function takes ``ft``: ``numpy.float64`` is the reference the GPU tests hold the kernels to,
``numpy.longdouble`` (80-bit where the platform has it) the yardstick that measures the float64 restatement's own error; the
yardstick forms an interval's product by pairwise halving over whole arrays, which is quick and rounds log m times.

``mistake=`` names one deliberate error; tests/test_imuref_cpu.py shows that each moves a quantity the GPU tests check."""
import numpy as np

BAD_ORDER, GYRO_FAILED, SCALE_FAILED, FEW_TRIPLES, SINGULAR, BAD_SCALE = 1, 2, 4, 8, 16, 32
SMALL = 1e-4               # theta^2 below which Exp and Jr use their series
MISTAKES = ("euler_rate", "operands_exchanged", "j_sign", "j_no_transpose", "dp_from_updated_dv", "end_sample_twice",
            "rbc_transposed", "no_lever_arm", "gravity_sign", "dt1_for_both", "quaternion_unnormalised")


# ------------------------------------------------------------------------------------------------ SO(3)
def hat(p):
    z = p.dtype.type(0)
    return np.array([[z, -p[2], p[1]], [p[2], z, -p[0]], [-p[1], p[0], z]], dtype=p.dtype)


def _coeffs(th2):
    """(sin th / th, (1 - cos th) / th^2, (th - sin th) / th^3) for th^2 in its own dtype"""
    ft = th2.dtype.type
    if th2 < ft(SMALL):
        a = 1 - th2 / 6 * (1 - th2 / 20 * (1 - th2 / 42 * (1 - th2 / 72)))
        b = ft(0.5) * (1 - th2 / 12 * (1 - th2 / 30 * (1 - th2 / 56 * (1 - th2 / 90))))
        c = (1 - th2 / 20 * (1 - th2 / 42 * (1 - th2 / 72 * (1 - th2 / 110)))) / 6
        return a, b, c
    th = np.sqrt(th2)
    s, h = np.sin(th), np.sin(th / 2)
    return s / th, 2 * h * h / th2, (th - s) / (th2 * th)


def so3_exp(phi):
    a, b, _ = _coeffs(phi @ phi)
    K = hat(phi)
    return np.eye(3, dtype=phi.dtype) + a * K + b * (K @ K)


def so3_jr(phi):
    _, b, c = _coeffs(phi @ phi)
    K = hat(phi)
    return np.eye(3, dtype=phi.dtype) - b * K + c * (K @ K)


def so3_log(R):
    """through the unit quaternion: accurate for the small residual rotations of the gyro step"""
    q = quat_from_R(R)
    n = np.sqrt(q[:3] @ q[:3])
    if n == 0:
        return 2 * q[:3] / q[3]
    return 2 * np.arctan2(n, q[3]) / n * q[:3]


def quat_from_R(R):
    """xyzw with w >= 0 (Shepperd: the largest of the four squares is the pivot)"""
    ft = R.dtype.type
    t = np.array([R[0, 0], R[1, 1], R[2, 2], R[0, 0] + R[1, 1] + R[2, 2]])
    i = int(np.argmax(t))
    if i == 3:
        w = np.sqrt(1 + t[3]) / 2
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        j, k = (i + 1) % 3, (i + 2) % 3
        x = np.sqrt(1 + 2 * t[i] - t[3]) / 2
        q = np.zeros(4, dtype=R.dtype)
        q[i], q[j], q[k], q[3] = x, (R[j, i] + R[i, j]) / (4 * x), (R[k, i] + R[i, k]) / (4 * x), (R[k, j] - R[j, k]) / (4 * x)
    q = q.astype(R.dtype)
    q = q / np.sqrt(q @ q)
    return -q if q[3] < ft(0) else q


def R_from_quat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=q.dtype)


# ------------------------------------------------------------------------------------------------ elements
def element(w, a, dt, mistake=None):
    """(Exp(w dt), a dt, 1/2 a dt^2, dt, -Jr(w dt) dt)"""
    phi = w * dt
    J = -so3_jr(phi) * dt
    if mistake == "j_sign":
        J = -J
    dv = a * dt
    return so3_exp(phi), dv, dv * (dt / 2), dt, J


def compose(e1, e2, mistake=None):
    if mistake == "operands_exchanged":
        e1, e2 = e2, e1
    R1, v1, p1, t1, J1 = e1
    R2, v2, p2, t2, J2 = e2
    v = v1 + R1 @ v2
    p = p1 + (v if mistake == "dp_from_updated_dv" else v1) * t2 + R1 @ p2
    J = (R2 if mistake == "j_no_transpose" else R2.T) @ J1 + J2
    return R1 @ R2, v, p, t1 + t2, J


def _elements_batch(w, a, dt):
    """``element`` for m sub-intervals at once: (R [m,3,3], dv [m,3], dp [m,3], dt [m], J [m,3,3])"""
    ft = dt.dtype.type
    phi = w * dt[:, None]
    th2 = np.sum(phi * phi, axis=1)
    small = th2 < ft(SMALL)
    x = np.where(small, th2, ft(0))
    sa = 1 - x / 6 * (1 - x / 20 * (1 - x / 42 * (1 - x / 72)))
    sb = ft(0.5) * (1 - x / 12 * (1 - x / 30 * (1 - x / 56 * (1 - x / 90))))
    sc = (1 - x / 20 * (1 - x / 42 * (1 - x / 72 * (1 - x / 110)))) / 6
    big = np.where(small, ft(1), th2)
    th = np.sqrt(big)
    sn, h = np.sin(th), np.sin(th / 2)
    ca, cb, cc = np.where(small, sa, sn / th), np.where(small, sb, 2 * h * h / big), np.where(small, sc, (th - sn) / (big * th))
    K = np.zeros((len(dt), 3, 3), dt.dtype)
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -phi[:, 2], phi[:, 1], phi[:, 2], -phi[:, 0], -phi[:, 1], phi[:, 0]
    K2, I = K @ K, np.eye(3, dtype=dt.dtype)
    R = I + ca[:, None, None] * K + cb[:, None, None] * K2
    J = -(I - cb[:, None, None] * K + cc[:, None, None] * K2) * dt[:, None, None]
    dv = a * dt[:, None]
    return R, dv, dv * (dt[:, None] / 2), dt, J


def _product_tree(e):
    """the ordered product of a batch of elements by pairwise halving: the longdouble yardstick's order (its rounding grows
    with log m; the float64 reference composes one after the other)"""
    R, v, p, t, J = e
    mv = lambda A, x: (A @ x[..., None])[..., 0]
    while len(t) > 1:
        if len(t) % 2:
            I, z = np.eye(3, dtype=R.dtype)[None], np.zeros((1, 3), R.dtype)
            R, v, p, t, J = (np.concatenate([R, I]), np.concatenate([v, z]), np.concatenate([p, z]), np.concatenate([t, t[:1] * 0]),
                             np.concatenate([J, I * 0]))
        R1, v1, p1, t1, J1, R2, v2, p2, t2, J2 = R[0::2], v[0::2], p[0::2], t[0::2], J[0::2], R[1::2], v[1::2], p[1::2], t[1::2], J[1::2]
        R, v, p, t, J = (R1 @ R2, v1 + mv(R1, v2), p1 + v1 * t2[:, None] + mv(R1, p2), t1 + t2,
                         np.swapaxes(R2, 1, 2) @ J1 + J2)
    return R[0], v[0], p[0], t[0], J[0]


def identity(ft):
    return np.eye(3, dtype=ft), np.zeros(3, ft), np.zeros(3, ft), ft(0), np.zeros((3, 3), ft)


def preintegrate_interval(tau, gyro, accel, T0, T1, bias_g, bias_a, max_gap=np.inf, ft=np.float64, mistake=None):
    """the 24-word record of [T0, T1] (NaN when the interval is not covered) and why: '' covered, 'dt' or 'uncovered'"""
    nan = np.full(24, np.nan, ft)
    if not (np.isfinite(np.asarray(bias_g, np.float64)).all() and np.isfinite(np.asarray(bias_a, np.float64)).all()):
        return nan, "uncovered"                          # (a failed gyro step's NaN bias: nothing is integrated with it)
    if not T1 > T0:
        return nan, "dt"
    N = len(tau)
    if not (tau[0] <= T0 and T1 <= tau[N - 1]):
        return nan, "uncovered"
    lo, hi = int(np.searchsorted(tau, T0, "right")), int(np.searchsorted(tau, T1, "left"))    # the samples strictly inside
    touched = slice(lo - 1, hi + 1)
    if not (np.isfinite(gyro[touched]).all() and np.isfinite(accel[touched]).all()):
        return nan, "uncovered"
    if (np.diff(tau[touched]) > max_gap).any():
        return nan, "uncovered"
    tl, g, a = tau.astype(ft), gyro.astype(ft), accel.astype(ft)
    bg, ba = np.asarray(bias_g, ft), np.asarray(bias_a, ft)

    def at(i, u):                                        # the measurement at u in (tau[i], tau[i + 1]]; a sample's own at its time
        if u == tl[i]:
            return g[i], a[i]
        if u == tl[i + 1]:
            return g[i + 1], a[i + 1]
        al = (u - tl[i]) / (tl[i + 1] - tl[i])
        return g[i] + al * (g[i + 1] - g[i]), a[i] + al * (a[i + 1] - a[i])

    u = np.concatenate([[ft(T0)], tl[lo:hi], [ft(T1)]])
    g0, a0 = at(lo - 1, ft(T0))
    g1, a1 = at(hi - 1, ft(T1))
    gs, as_ = np.vstack([g0[None], g[lo:hi], g1[None]]), np.vstack([a0[None], a[lo:hi], a1[None]])
    m = len(u) - 1
    acc = None
    half = ft(0.5)
    if ft is np.longdouble and mistake is None:
        acc = _product_tree(_elements_batch(half * (gs[:-1] + gs[1:]) - bg, half * (as_[:-1] + as_[1:]) - ba, np.diff(u)))
        m_loop = 0
    else:
        m_loop = m
    for j in range(m_loop):
        dt = u[j + 1] - u[j]
        if mistake == "euler_rate":
            w, f = gs[j] - bg, as_[j] - ba
        else:
            w, f = half * (gs[j] + gs[j + 1]) - bg, half * (as_[j] + as_[j + 1]) - ba
        e = element(w, f, dt, mistake)
        acc = e if acc is None else compose(acc, e, mistake)
        if mistake == "end_sample_twice" and j == m - 1 and tl[hi] == T1:      # (the sample on the end taken as a step of its own)
            acc = compose(acc, e, mistake)
    R, v, p, t, J = acc
    return np.concatenate([[t, ft(m)], quat_from_R(R), v, p, J.reshape(-1), np.zeros(3, ft)]).astype(ft), ""


def check_order(tau, times):
    bad = lambda x: (not np.isfinite(x).all()) or bool((np.diff(x) < 0).any())
    return bad(np.asarray(tau)) or bad(np.asarray(times))


def preintegrate(tau, gyro, accel, times, bias_g=None, bias_a=None, stride=1, max_gap=np.inf, ft=np.float64, mistake=None):
    """-> (preint [K - 1, 24], status int32 [8])"""
    tau, times = np.asarray(tau, np.float64), np.asarray(times, np.float64)
    gyro, accel = np.asarray(gyro).reshape(-1, 3), np.asarray(accel).reshape(-1, 3)
    bias_g = np.zeros(3) if bias_g is None else bias_g
    bias_a = np.zeros(3) if bias_a is None else bias_a
    used = times[::stride]
    K = len(used)
    status = np.zeros(8, np.int32)
    status[1], status[2] = len(tau), K - 1
    out = np.full((K - 1, 24), np.nan, ft)
    if check_order(tau, times):
        status[0] |= BAD_ORDER
        status[3] = K - 1
        return out, status
    for k in range(K - 1):
        out[k], why = preintegrate_interval(tau, gyro, accel, used[k], used[k + 1], bias_g, bias_a, max_gap, ft, mistake)
        status[3] += why == "uncovered"
        status[4] += why == "dt"
    return out, status


# ------------------------------------------------------------------------------------------------ alignment
def _bodies(knots, stride, R_bc, p_bc, ft, mistake=None):
    """(R_wb [K,3,3], pbar [K,3], c [K,3]) of the knots used"""
    kn = np.asarray(knots, np.float32)[::stride].astype(ft)
    Rbc, pbc = np.asarray(R_bc, ft).reshape(3, 3), np.asarray(p_bc, ft).reshape(3)
    if mistake == "rbc_transposed":
        Rbc = Rbc.T
    if mistake == "no_lever_arm":
        pbc = pbc * 0
    Rwb, c = [], []
    for row in kn:
        q = row[3:7]
        if mistake != "quaternion_unnormalised":
            q = q / np.sqrt(q @ q)
        Rwc = R_from_quat(q)
        Rwb.append(Rwc @ Rbc.T)
        c.append(Rwc @ (-(Rbc.T @ pbc)))
    return np.array(Rwb, ft), kn[:, :3].copy(), np.array(c, ft)


def _covered(pre):
    return np.isfinite(pre[:, 0])


def gyro_system(pre, Rwb, ft=np.float64):
    """(H [3,3], b [3], the number of intervals) of one Gauss-Newton step"""
    H, b, n = np.zeros((3, 3), ft), np.zeros(3, ft), 0
    for k in np.nonzero(_covered(pre))[0]:
        dR, J = R_from_quat(pre[k, 2:6]), pre[k, 12:21].reshape(3, 3)
        r = so3_log(dR.T @ Rwb[k].T @ Rwb[k + 1])
        H, b, n = H + J.T @ J, b + J.T @ r, n + 1
    return H, b, n


def triple_rows(pre, Rwb, pbar, c, j, mistake=None):
    """(A [3,4], rhs [3]) of the triple of knots j, j + 1, j + 2"""
    ft = pre.dtype.type
    t1, t2 = pre[j, 0], pre[j + 1, 0]
    if mistake == "dt1_for_both":
        t2 = t1
    dv1, dp1, dp2 = pre[j, 6:9], pre[j, 9:12], pre[j + 1, 9:12]
    A = np.zeros((3, 4), ft)
    A[:, 0] = (pbar[j + 2] - pbar[j + 1]) / t2 - (pbar[j + 1] - pbar[j]) / t1
    A[:, 1:] = (ft(0.5) if mistake == "gravity_sign" else ft(-0.5)) * (t1 + t2) * np.eye(3, dtype=ft)
    rhs = (Rwb[j + 1] @ dp2) / t2 - (Rwb[j] @ dp1) / t1 + Rwb[j] @ dv1 - (c[j + 2] - c[j + 1]) / t2 + (c[j + 1] - c[j]) / t1
    return A, rhs


def scale_system(pre, Rwb, pbar, c, mistake=None):
    """(N [4,4], y [4], the triples used) in index order"""
    ft = pre.dtype.type
    N, y, used = np.zeros((4, 4), ft), np.zeros(4, ft), []
    cov = _covered(pre)
    for j in range(len(pre) - 1):
        if cov[j] and cov[j + 1]:
            A, rhs = triple_rows(pre, Rwb, pbar, c, j, mistake)
            N, y = N + A.T @ A, y + A.T @ rhs
            used.append(j)
    return N, y, used


def tangent_basis(gh):
    e = np.zeros(3, gh.dtype)
    e[int(np.argmin(np.abs(gh)))] = 1            # (argmin: the first on ties)
    b1 = np.cross(gh, e)
    b1 = b1 / np.sqrt(b1 @ b1)
    return b1, np.cross(gh, b1)


def solve_scale(N, y, gravity_norm=0.0):
    """x = (s, g) from the normal equations alone: the free solve, then with a norm exactly four tangent refinements"""
    x = np.linalg.solve(N.astype(np.float64), y.astype(np.float64)).astype(N.dtype) if N.dtype != np.longdouble else _solve_ld(N, y)
    if gravity_norm > 0:
        ft = N.dtype.type
        G = ft(gravity_norm)
        gh = x[1:] / np.sqrt(x[1:] @ x[1:])
        for _ in range(4):
            b1, b2 = tangent_basis(gh)
            P = np.zeros((4, 3), N.dtype)
            P[0, 0], P[1:, 1], P[1:, 2] = 1, b1, b2
            x0 = np.concatenate([[ft(0)], G * gh])
            M, r = P.T @ N @ P, P.T @ (y - N @ x0)
            z = np.linalg.solve(M.astype(np.float64), r.astype(np.float64)).astype(N.dtype) if N.dtype != np.longdouble else _solve_ld(M, r)
            g = G * gh + z[1] * b1 + z[2] * b2
            gh = g / np.sqrt(g @ g)
            x = np.concatenate([[z[0]], G * gh])
    return x


def _solve_ld(A, b):
    """Gaussian elimination with partial pivoting in the arrays' own precision (numpy.linalg has no longdouble)"""
    A, b = A.copy(), b.copy()
    n = len(b)
    for i in range(n):
        p = i + int(np.argmax(np.abs(A[i:, i])))
        A[[i, p]], b[[i, p]] = A[[p, i]], b[[p, i]]
        for r in range(i + 1, n):
            f = A[r, i] / A[i, i]
            A[r, i:], b[r] = A[r, i:] - f * A[i, i:], b[r] - f * b[i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def velocities(pre, Rwb, pbar, c, x, used, mistake=None):
    """(velocity [K,3], residual [K-2], rms)"""
    ft = pre.dtype.type
    K = len(pbar)
    s, g = x[0], x[1:]
    p = s * pbar + c
    vel, res = np.full((K, 3), np.nan, ft), np.full(max(K - 2, 0), np.nan, ft)
    cov = _covered(pre)
    for k in range(K - 1):
        if cov[k]:
            t = pre[k, 0]
            vel[k] = (p[k + 1] - p[k] - ft(0.5) * g * (t * t) - Rwb[k] @ pre[k, 9:12]) / t
    if K >= 2 and cov[K - 2]:
        vel[K - 1] = vel[K - 2] + g * pre[K - 2, 0] + Rwb[K - 2] @ pre[K - 2, 6:9]
    for j in used:
        A, rhs = triple_rows(pre, Rwb, pbar, c, j, mistake)
        d = A @ x - rhs
        res[j] = np.sqrt(d @ d)
    rms = np.sqrt(np.sum(res[used] ** 2) / len(used)) if used else ft(np.nan)
    return vel, res, rms


def align(tau, gyro, accel, knots, times, R_bc=None, p_bc=None, bias_g=None, bias_a=None, stride=1, max_gap=np.inf,
          gravity_norm=0.0, gyro_steps=1, ft=np.float64, mistake=None, bias_g1=None):
    """the whole of ramp_imu_align -> dict(result [16], normal [32], velocity, residual, preint, status).  ``bias_g1``: skip the
    gyro stage's solve and integrate the second time with this bias (the device's own), H and b still formed."""
    with np.errstate(all="ignore"):                           # (the overflow case computes with inf and NaN on purpose)
        return _align(tau, gyro, accel, knots, times, R_bc, p_bc, bias_g, bias_a, stride, max_gap, gravity_norm, gyro_steps, ft,
                      mistake, bias_g1)


def _align(tau, gyro, accel, knots, times, R_bc, p_bc, bias_g, bias_a, stride, max_gap, gravity_norm, gyro_steps, ft, mistake, bias_g1):
    R_bc = np.eye(3) if R_bc is None else R_bc
    p_bc = np.zeros(3) if p_bc is None else p_bc
    bg = np.zeros(3, ft) if bias_g is None else np.asarray(bias_g, ft)
    ba = np.zeros(3, ft) if bias_a is None else np.asarray(bias_a, ft)
    Rwb, pbar, c = _bodies(knots, stride, R_bc, p_bc, ft, mistake)
    K = len(pbar)
    nan = ft(np.nan)
    result, normal = np.zeros(16, ft), np.full(32, np.nan, ft)
    bits, n_gyro = 0, 0
    H, b = np.full((3, 3), nan), np.full(3, nan)
    for step in range(gyro_steps):
        pre, status = preintegrate(tau, gyro, accel, times, bg, ba, stride, max_gap, ft, mistake)
        H, b, n = gyro_system(pre, Rwb, ft)
        if step == 0:
            n_gyro = n
        ok = n >= 1 and np.isfinite(H).all() and np.isfinite(b).all()
        if ok:
            try:
                np.linalg.cholesky(H.astype(np.float64))
                delta = _solve_ld(H, b)
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            bits |= GYRO_FAILED
            bg = np.full(3, nan)
            break
        bg = bg + delta
    if bias_g1 is not None:
        bg = np.asarray(bias_g1, ft)
    pre, status = preintegrate(tau, gyro, accel, times, bg, ba, stride, max_gap, ft, mistake)
    N, y, used = scale_system(pre, Rwb, pbar, c, mistake)
    x, cond = np.full(4, nan), nan
    if len(used) < 2:
        bits |= SCALE_FAILED | FEW_TRIPLES
    elif not (np.isfinite(N).all() and np.isfinite(y).all()):
        bits |= SCALE_FAILED | SINGULAR
    else:
        try:
            L = np.linalg.cholesky(N.astype(np.float64))
            d = np.diag(L) ** 2
            cond = ft(d.max() / d.min())
            x = solve_scale(N, y, gravity_norm)
            if not x[0] > 0:
                bits |= SCALE_FAILED | BAD_SCALE
        except np.linalg.LinAlgError:
            bits |= SCALE_FAILED | SINGULAR
    if bits & SCALE_FAILED:
        x, cond = np.full(4, nan), nan
        vel, res, rms = np.full((K, 3), nan), np.full(max(K - 2, 0), nan), nan
    else:
        vel, res, rms = velocities(pre, Rwb, pbar, c, x, used, mistake)
    result[0], result[1:4], result[4:7], result[7], result[8] = x[0], x[1:], bg, rms, cond
    normal[:16], normal[16:20], normal[20:29], normal[29:32] = N.reshape(-1), y, H.reshape(-1), b
    status = status.copy()
    status[0] |= bits
    status[5], status[6] = n_gyro, len(used)
    return dict(result=result, normal=normal, velocity=vel, residual=res, preint=pre, status=status, scale=x[0], gravity=x[1:],
                bias_g=bg)


# ------------------------------------------------------------------------------------------------ the analytic scene
G_TRUE = 9.80665 * np.array([0.3, -0.2, -9.79]) / np.linalg.norm([0.3, -0.2, -9.79])
BIAS_TRUE = np.array([0.01, -0.02, 0.015])
SCALE_TRUE = 3.7
P_BC = np.array([0.05, 0.02, -0.01])


def _f64_exp(phi):
    return so3_exp(np.asarray(phi, np.float64))


R_BC = _f64_exp([0.1, -0.05, 1.5])


def body(t):
    """(position, rotation, body rate, specific force) of the scene at time t, closed forms"""
    t = float(t)
    p2 = np.array([-1.5 * 0.81 * np.sin(0.9 * t), -0.49 * np.cos(0.7 * t), -0.6 * 1.69 * np.sin(1.3 * t + 0.4)])
    pos = np.array([1.5 * np.sin(0.9 * t), np.cos(0.7 * t) + 0.2 * t, 0.6 * np.sin(1.3 * t + 0.4)])
    phi = np.array([0.4 * np.sin(0.8 * t), 0.3 * np.sin(1.1 * t + 1), 0.5 * np.sin(0.5 * t)])
    dphi = np.array([0.32 * np.cos(0.8 * t), 0.33 * np.cos(1.1 * t + 1), 0.25 * np.cos(0.5 * t)])
    R = so3_exp(phi)
    return pos, R, so3_jr(phi) @ dphi, R.T @ (p2 - G_TRUE)


_scene_cache = {}


def knots_at(times):
    """the scene's camera poses at ``times`` with their translations divided by SCALE_TRUE, fp32 [T,7]"""
    knots = np.zeros((len(times), 7))
    for k, t in enumerate(times):
        pos, R, _, _ = body(t)
        knots[k, :3] = (pos + R @ P_BC) / SCALE_TRUE
        knots[k, 3:] = quat_from_R(R @ R_BC)
    return knots.astype(np.float32)


def scene(mirror=False, on_samples=False):
    """dict(tau, gyro, accel, knots, times) -- 200 Hz samples on [0, 12), 20 Hz frames on [0.5, 11.5), the knots camera poses
    with their translations divided by SCALE_TRUE, fp32.  ``mirror``: the knots' translations negated (s < 0).  ``on_samples``:
    the frames' time stamps are every tenth sample's, so that a sample lies exactly on each end of every interval."""
    if "base" not in _scene_cache:
        tau = 0.00123 + np.arange(int(12 * 200)) / 200.0
        tau = tau[tau < 12.0]
        gyro, accel = np.zeros((len(tau), 3)), np.zeros((len(tau), 3))
        for i, t in enumerate(tau):
            _, _, w, f = body(t)
            gyro[i], accel[i] = w + BIAS_TRUE, f
        _scene_cache["base"] = dict(tau=tau, gyro=gyro, accel=accel)
    key = "on" if on_samples else "off"
    if key not in _scene_cache:
        times = _scene_cache["base"]["tau"][100:2300:10].copy() if on_samples else 0.5 + np.arange(int(11 * 20)) / 20.0
        _scene_cache[key] = dict(knots=knots_at(times), times=times)
    s = {k: v.copy() for k, v in {**_scene_cache["base"], **_scene_cache[key]}.items()}
    if mirror:
        s["knots"][:, :3] *= -1
    return s


EXTR = dict(R_bc=R_BC, p_bc=P_BC)
IRREGULAR = [i for i in range(60) if i % 3 != 1]          # 40 of the scene's frames: intervals of two lengths in turn


def cases():
    """The failure cases the GPU test runs and the CPU test pins: name -> (keywords of ``align``, the expected status words
    [0, 2, 3, 4, 5, 6]: bits, intervals, uncovered, dt <= 0, gyro intervals, triples)."""
    out = {}
    sc = lambda **kw: {**scene(), **EXTR, **kw}
    short = lambda a, b: {k: (v[a:b] if k in ("knots", "times") else v) for k, v in sc().items()}
    s = sc()
    s["tau"][1200] = s["tau"][1198]
    out["tau_decreasing"] = (s, [BAD_ORDER | GYRO_FAILED | SCALE_FAILED | FEW_TRIPLES, 219, 219, 0, 0, 0])
    s = sc()
    s["times"][7] = np.nan
    out["times_nan"] = (s, [BAD_ORDER | GYRO_FAILED | SCALE_FAILED | FEW_TRIPLES, 219, 219, 0, 0, 0])
    s = sc()
    s["accel"][1000, 1] = np.nan                      # tau 5.00123: inside [5.0, 5.05] and the first sample behind [4.95, 5.0]
    out["nan_sample"] = (s, [0, 219, 2, 0, 217, 215])
    s = sc()
    keep = np.ones(len(s["tau"]), bool)
    keep[1001:1021] = False                           # a hole of 0.105 s: the intervals from 5.0 to 5.15 touch it
    s = {k: (v[keep] if k in ("tau", "gyro", "accel") else v) for k, v in s.items()}
    out["gap"] = ({**s, "max_gap": 0.02}, [0, 219, 3, 0, 216, 214])
    s = sc()
    cut = slice(120, 2200)                            # samples on [0.60123, 10.99623]: the 3 intervals that start before and the
    s = {k: (v[cut] if k in ("tau", "gyro", "accel") else v) for k, v in s.items()}      # 10 that end after (11.0 .. 11.45)
    out["uncovered_ends"] = (s, [0, 219, 3 + 10, 0, 206, 205])
    s = sc()
    s["times"][50] = s["times"][49]
    s["knots"][50] = s["knots"][49]
    out["dt_zero"] = (s, [0, 219, 0, 1, 218, 216])
    out["K2"] = (short(10, 12), [SCALE_FAILED | FEW_TRIPLES, 1, 0, 0, 1, 0])
    out["K3"] = (short(10, 13), [SCALE_FAILED | FEW_TRIPLES, 2, 0, 0, 2, 1])
    s = sc(R_bc=np.eye(3), p_bc=np.zeros(3))
    s["knots"][:] = np.array([0.25, -0.5, 1.0, 0, 0, 0, 1], np.float32)
    s["gyro"][:], s["accel"][:] = 0.0, -G_TRUE
    out["stationary"] = (s, [SCALE_FAILED | SINGULAR, 219, 0, 0, 219, 218])
    s = sc()
    s["gyro"][:] = 1e300                              # finite samples whose rotation overflows: the records' dt stays finite, H does
    out["gyro_overflow"] = (s, [GYRO_FAILED | SCALE_FAILED | FEW_TRIPLES, 219, 219, 0, 219, 0])      # not; then the NaN bias
    out["mirrored"] = ({**scene(mirror=True), **EXTR}, [SCALE_FAILED | BAD_SCALE, 219, 0, 0, 219, 218])
    return out


def bound(env, m, field):
    """the per-field bound of the GPU tests: max(4 env, 16 m 2^-53 max(1, max|field|))"""
    top = np.nanmax(np.abs(np.asarray(field, np.float64))) if np.size(field) else 0.0
    return max(4 * float(env), 16 * m * 2.0 ** -53 * max(1.0, float(top)))
