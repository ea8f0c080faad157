"""Numpy restatement of ``ramp_imu_propagate`` (include/ramp_hip.h) -- TEST INFRASTRUCTURE ONLY.  It shares none of the
kernel's structure: rotations are 3 x 3 matrices, the prefix products are ONE plain loop from the left over
``imuref.element`` / ``imuref.compose`` (the kernel scans chunks, tiles and a chain), the break index comes from a loop over
the rows.  ``ft``: ``numpy.float64`` is the reference the GPU test holds the kernel to, ``numpy.longdouble`` the yardstick that
measures the float64 restatement's own error.

``mistake=`` names one deliberate error; tests/test_propref_cpu.py shows that each moves a checked row."""
import numpy as np

import imuref as ir

BAD_ORDER, BAD_ANCHOR, NO_START = 1, 64, 128
ANCHOR_WORDS = 24
MISTAKES = ("g_negated", "no_v0_dt", "no_half", "rbc_transposed", "no_lever_arm", "times_s", "bias_kept",
            "t0_not_interpolated", "compose_no_t2", "qbc_wrong_side")


def make_anchor(t0, pbar0, q_wc0, v0, s, g, bias_g):
    return np.concatenate([[t0], pbar0, q_wc0, v0, [s], g, bias_g, np.zeros(6)]).astype(np.float64)


def quat_mul(a, b):
    """xyzw.  Not poseref.qmul: y and z are summed in another order here (last-bit differences), and this module needs no oracle"""
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def break_index(tau, gyro, accel, t0, max_gap):
    """the first row behind the anchor that dead reckoning does not reach, or N"""
    fin = np.isfinite(gyro).all(axis=1) & np.isfinite(accel).all(axis=1)
    for i in range(1, len(tau)):
        if tau[i] > t0 and (not fin[i] or not fin[i - 1] or tau[i] - tau[i - 1] > max_gap):
            return i
    return len(tau)


def propagate(tau, gyro, accel, anchor, R_bc=None, p_bc=None, bias_a=None, max_gap=np.inf, horizon=np.inf, ft=np.float64,
              mistake=None):
    """-> dict(state [N,16], poses64 [N,7] (the stated formula in ``ft``), poses fp32, times [N], status int32 [8],
    m [N]: the number of elements of positive length in front of each row)"""
    with np.errstate(all="ignore"):
        return _propagate(tau, gyro, accel, anchor, R_bc, p_bc, bias_a, max_gap, horizon, ft, mistake)


def _propagate(tau, gyro, accel, anchor, R_bc, p_bc, bias_a, max_gap, horizon, ft, mistake):
    tau, anchor = np.asarray(tau, np.float64), np.asarray(anchor, np.float64)
    gyro, accel = np.asarray(gyro).reshape(-1, 3), np.asarray(accel).reshape(-1, 3)
    N = len(tau)
    status = np.zeros(8, np.int32)
    status[1] = N
    state, poses, times = np.full((N, 16), np.nan, ft), np.full((N, 7), np.nan, ft), np.full(N, np.nan)
    m = np.zeros(N, np.int64)
    t0 = anchor[0]
    if not np.isfinite(tau).all() or (np.diff(tau) < 0).any():
        status[0] |= BAD_ORDER
    if not np.isfinite(anchor[:18]).all() or not anchor[11] > 0:
        status[0] |= BAD_ANCHOR
    if tau[0] > t0:
        status[0] |= NO_START
    out = dict(state=state, poses64=poses, poses=poses.astype(np.float32), times=times, status=status, m=m)
    if status[0]:
        return out
    Rbc = np.eye(3, dtype=ft) if R_bc is None else np.asarray(R_bc, ft).reshape(3, 3)
    pbc = np.zeros(3, ft) if p_bc is None else np.asarray(p_bc, ft).reshape(3)
    if mistake == "rbc_transposed":
        Rbc = Rbc.T
    if mistake == "no_lever_arm":
        pbc = pbc * 0
    ba = np.zeros(3, ft) if bias_a is None else np.asarray(bias_a, ft)
    A = anchor.astype(ft)
    pbar0, q, v0, s, g, bg = A[1:4], A[4:8], A[8:11], A[11], A[12:15], A[15:18]
    if mistake == "bias_kept":
        bg = bg * 0
    Rwc0 = ir.R_from_quat(q / np.sqrt(q @ q))
    R0 = Rwc0 @ Rbc.T
    p0 = s * pbar0 - R0 @ pbc
    tl, gy, ac = tau.astype(ft), gyro.astype(ft), accel.astype(ft)
    T0, half = ft(t0), ft(0.5)
    b = break_index(tau, gyro, accel, t0, max_gap)
    times[:] = np.maximum(tau, t0)
    acc, count = ir.identity(ft), 0
    for i in range(N):
        if i >= 1 and tau[i] > t0 and i < b:
            u0, g0, a0, g1, a1 = tl[i - 1], gy[i - 1], ac[i - 1], gy[i], ac[i]
            if tau[i - 1] < t0:
                u0 = T0
                if mistake != "t0_not_interpolated":
                    al = (T0 - tl[i - 1]) / (tl[i] - tl[i - 1])
                    g0, a0 = g0 + al * (g1 - g0), a0 + al * (a1 - a0)
            dt = tl[i] - u0
            if dt > 0:
                e = ir.element(half * (g0 + g1) - bg, half * (a0 + a1) - ba, dt)
                if mistake == "compose_no_t2":
                    R1, v1, p1, t1, J1 = acc
                    acc = (R1 @ e[0], v1 + R1 @ e[1], p1 + v1 + R1 @ e[2], t1 + e[3], J1)
                else:
                    acc = ir.compose(acc, e)
                count += 1
        m[i] = count
        if tau[i] <= t0:
            status[2] += 1
        elif i >= b:
            status[4] += 1
            continue
        elif acc[3] > horizon:
            status[5] += 1
            continue
        else:
            status[3] += 1
        dR, dv, dp, dt = acc[0], acc[1], acc[2], acc[3]
        gg = -g if mistake == "g_negated" else g
        hh = ft(1) if mistake == "no_half" else half
        Rwb = R0 @ dR
        v = (v0 + gg * dt) + R0 @ dv
        p = ((p0 + (0 if mistake == "no_v0_dt" else v0 * dt)) + hh * gg * (dt * dt)) + R0 @ dp
        state[i, 0], state[i, 1:5], state[i, 5:8], state[i, 8:11], state[i, 11:] = dt, ir.quat_from_R(Rwb), v, p, 0
        tr = p + Rwb @ pbc
        poses[i, :3] = tr * s if mistake == "times_s" else tr / s
        if mistake == "qbc_wrong_side":
            qc = quat_mul(ir.quat_from_R(Rbc), ir.quat_from_R(Rwb))
            poses[i, 3:] = qc / np.sqrt(qc @ qc)
        else:
            poses[i, 3:] = ir.quat_from_R(Rwb @ Rbc)
    out["poses"] = poses.astype(np.float32)
    return out


def scene_anchor(t0, ft=np.float64):
    """the analytic scene's true state at t0 as an anchor: the camera's pose with its translation divided by SCALE_TRUE, the
    body's velocity by a central difference of the closed-form position (h = 1e-5: error 1e-10, far below what is checked)"""
    pos, R, _, _ = ir.body(t0)
    h = 1e-5
    v0 = (ir.body(t0 + h)[0] - ir.body(t0 - h)[0]) / (2 * h)
    return make_anchor(t0, (pos + R @ ir.P_BC) / ir.SCALE_TRUE, ir.quat_from_R(R @ ir.R_BC), v0, ir.SCALE_TRUE, ir.G_TRUE, ir.BIAS_TRUE)


def cases():
    """The failure cases the GPU test runs and the CPU test pins: name -> (keywords of ``propagate``, the expected status words
    [0, 2, 3, 4, 5]: bits, held, propagated, cut off, beyond the horizon, the expected NaN rows as a slice or None for all)."""
    s = ir.scene()
    i0 = 1000                                             # tau 5.00123; the anchor lies between samples 999 and 1000
    t0 = 5.0
    base = lambda **kw: {**dict(tau=s["tau"][800:1300].copy(), gyro=s["gyro"][800:1300].copy(), accel=s["accel"][800:1300].copy(),
                                anchor=scene_anchor(t0), R_bc=ir.R_BC, p_bc=ir.P_BC), **kw}
    k0 = i0 - 800                                         # the first row behind the anchor: 200 held, 300 behind
    out, ALL = {}, slice(0, 500)

    def edit(f, **kw):
        c = base(**kw)
        f(c)
        return c
    def set_(key, idx, val):
        def f(c):
            c[key][idx] = val
        return f
    out["clean"] = (base(), [0, 200, 300, 0, 0], slice(0, 0))
    out["tau_decreasing"] = (edit(set_("tau", 100, s["tau"][898])), [BAD_ORDER, 0, 0, 0, 0], ALL)
    out["tau_nan"] = (edit(set_("tau", 7, np.nan)), [BAD_ORDER, 0, 0, 0, 0], ALL)
    out["anchor_nan"] = (edit(set_("anchor", 9, np.nan)), [BAD_ANCHOR, 0, 0, 0, 0], ALL)
    out["s_zero"] = (edit(set_("anchor", 11, 0.0)), [BAD_ANCHOR, 0, 0, 0, 0], ALL)
    out["s_negative"] = (edit(set_("anchor", 11, -3.7)), [BAD_ANCHOR, 0, 0, 0, 0], ALL)
    out["no_start"] = (edit(set_("anchor", 0, 3.9)), [NO_START, 0, 0, 0, 0], ALL)
    out["nan_before_anchor"] = (edit(set_("gyro", (k0 - 2, 1), np.nan)), [0, 200, 300, 0, 0], slice(0, 0))
    out["nan_at_i0"] = (edit(set_("accel", (k0, 2), np.nan)), [0, 200, 0, 300, 0], slice(k0, 500))
    out["nan_at_i0_plus_3"] = (edit(set_("gyro", (k0 + 3, 0), np.inf)), [0, 200, 3, 297, 0], slice(k0 + 3, 500))
    keep = np.ones(500, bool)
    keep[100:110] = False                                 # a hole of 0.055 s before the anchor: ignored
    c = base(max_gap=0.02)
    out["gap_before_anchor"] = ({**c, "tau": c["tau"][keep], "gyro": c["gyro"][keep], "accel": c["accel"][keep]},
                                [0, 190, 300, 0, 0], slice(0, 0))
    keep = np.ones(500, bool)
    keep[k0 + 50:k0 + 60] = False
    out["gap_after_anchor"] = ({**c, "tau": c["tau"][keep], "gyro": c["gyro"][keep], "accel": c["accel"][keep]},
                               [0, 200, 50, 240, 0], slice(k0 + 50, 490))
    out["horizon"] = (base(horizon=0.5), [0, 200, 100, 0, 200], slice(k0 + 100, 500))      # tau[k0 + 99] - t0 = 0.49623
    out["break_and_horizon"] = (edit(set_("gyro", (k0 + 150, 0), np.nan), horizon=0.5), [0, 200, 100, 150, 50], slice(k0 + 100, 500))
    return out
