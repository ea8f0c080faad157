"""Numpy restatement of the time surface (include/ramp_hip.h ``ramp_time_surface``) and of the localisation against the event
map (``ramp_point_map_localize_eval``, ``ramp_point_map_localize``) -- TEST INFRASTRUCTURE ONLY.

(a) ``last_stamps``: the per-pixel max of the time stamps with the counters; ``raw_surface`` in float32 (the header's
    statements, numpy's own exp) and float64 (the reference); ``binomial``: the passes in exact fp32 (numpy rounds every
    operation and fuses nothing), which the GPU is held to bit for bit from its own ``raw``.
(b) ``sample``: the bilinear sample and the interpolant's derivative in fp32 from given u, v; ``slot_terms``: the per-slot
    row, weight and sums in float64 from given records; ``evaluate``: the whole evaluation (projection from
    ``renderref.project``).  ``evaluate_records``: the sums from a call's OWN records.
(c) ``Machine``: the state machine of the header, plain Python floats and ``math.sqrt`` -- one IEEE double operation per
    operation written, in the header's order --, driven by any ``evaluate(pose_f32) -> (cost, H[21], b[6], in_reach, status0)``.
(d) the ``mistake`` keywords break the restatement on purpose (tests/test_localizeref_cpu.py: each has to be rejected by the
    inputs the GPU tests use, which are built here).
"""
import math

import numpy as np

import alignref
import pointmapref as pm
import poseref
import renderref as rr

H, W, K, CAM, VOXEL = rr.H, rr.W, rr.K, rr.CAM, rr.VOXEL
ITERS, CONVERGED, STALLED, SINGULAR, FEW, BUDGET = 1, 2, 3, 4, 5, 6
REASONS = {0: "running", ITERS: "iters", CONVERGED: "converged", STALLED: "stalled", SINGULAR: "singular", FEW: "few", BUDGET: "budget"}
REJECTS = 8
BAD_CAMERA = 1
MISTAKES = ("w2c", "fxfy", "gugv", "right", "trunc", "late", "min", "drop_out", "huber_inv", "halve")
ABSENT, FILTERED, REJECTED, OUT, IN = range(5)
MARGIN = 1e-2
f32 = np.float32


# ------------------------------------------------------------------------------------------------------- time surface
def last_stamps(x, y, t, t_ref, h, w, last_in=None, mistake=None):
    """-> (last float64 [h,w], NaN: no event; counters [seen, not finite, outside, late, used, pixels])"""
    x, y, t = np.asarray(x, f32).reshape(-1), np.asarray(y, f32).reshape(-1), np.asarray(t, np.float64).reshape(-1)
    last = np.full((h, w), np.nan)
    if last_in is not None:
        li = np.asarray(last_in, np.float64)
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(li) & (li <= t_ref)
        last[ok] = li[ok]
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(x) | ~np.isfinite(y) | ~np.isfinite(t)
        px, py = (np.trunc(x), np.trunc(y)) if mistake == "trunc" else (np.rint(x), np.rint(y))
        outside = ~bad & ~((px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1))
        late = ~bad & ~outside & (np.zeros(len(t), bool) if mistake == "late" else ~(t <= t_ref))
    used = ~bad & ~outside & ~late
    for i in np.flatnonzero(used):
        at = (int(py[i]), int(px[i]))
        cur = last[at]
        if np.isnan(cur) or ((t[i] < cur) if mistake == "min" else (t[i] > cur)):
            last[at] = t[i]
    return last, [len(t), int(bad.sum()), int(outside.sum()), int(late.sum()), int(used.sum()), int((~np.isnan(last)).sum())]


def raw_surface(last, t_ref, tau, negate=True, dtype=f32):
    """float32: expf(float32((last - t_ref) / tau)) with the quotient in float64, 0 without a time stamp, 1 - raw when negated;
    float64: the same formula without the roundings"""
    with np.errstate(all="ignore"):
        q = (np.asarray(last, np.float64) - np.float64(t_ref)) / np.float64(tau)
        raw = np.where(np.isnan(last), dtype(0), np.exp(np.where(np.isnan(last), 0, q).astype(dtype)))
    raw = (dtype(1) - raw) if negate else raw
    return raw.astype(dtype)


def _blur_axis(a, axis):
    idx = lambda k: np.clip(np.arange(a.shape[axis]) + k, 0, a.shape[axis] - 1)
    t = [np.take(a, idx(k), axis) for k in (-2, -1, 0, 1, 2)]
    return ((((f32(1) * t[0] + f32(4) * t[1]) + f32(6) * t[2]) + f32(4) * t[3]) + f32(1) * t[4]) * f32(0.0625)


def binomial(img, passes):
    """``passes`` of the separable (1, 4, 6, 4, 1) / 16, rows then columns, edges replicated: exact fp32"""
    a = np.asarray(img, f32)
    with np.errstate(all="ignore"):
        for _ in range(passes):
            a = _blur_axis(_blur_axis(a, 1), 0)
    return a


def time_surface(x, y, t, t_ref, tau, h, w, smooth=2, last_in=None, negate=True, mistake=None):
    last, ctr = last_stamps(x, y, t, t_ref, h, w, last_in, mistake)
    raw = raw_surface(last, t_ref, tau, negate)
    return dict(surface=binomial(raw, smooth), raw=raw, last_t=last, status=np.array([0] + ctr + [0], np.int32))


# --------------------------------------------------------------------------------------------------------- evaluation
def reach(u, v, h, w):
    with np.errstate(all="ignore"):
        x0, y0 = np.floor(u).astype(np.float64), np.floor(v).astype(np.float64)
        return (x0 >= 0) & (x0 < w - 1) & (y0 >= 0) & (y0 < h - 1)


def sample(surface, u, v, mistake=None):
    """fp32 (r, gu, gv) at (u, v) in reach, the header's statements"""
    S = np.asarray(surface, f32)
    u, v = np.asarray(u, f32), np.asarray(v, f32)
    x0, y0 = np.floor(u), np.floor(v)
    ax, ay = u - x0, v - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    s00, s10, s01, s11 = S[iy, ix], S[iy, ix + 1], S[iy + 1, ix], S[iy + 1, ix + 1]
    bx, by = f32(1) - ax, f32(1) - ay
    with np.errstate(all="ignore"):
        r = by * (bx * s00 + ax * s10) + ay * (bx * s01 + ax * s11)
        gu = by * (s10 - s00) + ay * (s11 - s01)
        gv = bx * (s01 - s00) + ax * (s11 - s10)
    return (r, gv, gu) if mistake == "gugv" else (r, gu, gv)


def huber(r, k, mistake=None):
    """-> (rho, w), float64"""
    r = np.asarray(r, np.float64)
    ar = np.abs(r)
    with np.errstate(all="ignore"):
        out = (k > 0) & (ar > k)
        w = np.where(out, (ar / k) if mistake == "huber_inv" else (k / ar), 1.0)
        rho = np.where(out, (2.0 * k) * ar - k * k, r * r)
    return rho, w


TRI = [(p, q) for p in range(6) for q in range(p, 6)]


def rows(gu, gv, Xc, Kc, mistake=None):
    """J [n,6] float64 from the fp32 words"""
    k = np.asarray(Kc, f32).astype(np.float64)
    if mistake == "fxfy":
        k = k[[1, 0, 2, 3]]
    X, Y, z = (np.asarray(Xc, f32)[:, i].astype(np.float64) for i in range(3))
    gx, gy = np.asarray(gu, f32).astype(np.float64) * k[0], np.asarray(gv, f32).astype(np.float64) * k[1]
    with np.errstate(all="ignore"):
        J0, J1 = gx / z, gy / z
        J2 = -(gx * X + gy * Y) / (z * z)
        return np.stack([J0, J1, J2, Y * J2 - z * J1, z * J0 - X * J2, X * J1 - Y * J0], 1)


def slot_terms(r, gu, gv, Xc, Kc, k, mistake=None):
    """the per-slot terms in float64 -> (terms [n, 28]: 21 of H, 6 of b, rho)"""
    J = rows(gu, gv, Xc, Kc, mistake)
    rd = np.asarray(r, f32).astype(np.float64)
    rho, w = huber(rd, k, mistake)
    with np.errstate(all="ignore"):
        wj = w[:, None] * J
        return np.concatenate([np.stack([wj[:, p] * J[:, q] for p, q in TRI], 1), wj * rd[:, None], rho[:, None]], 1)


def full(h21):
    A = np.zeros((6, 6))
    for i, (p, q) in enumerate(TRI):
        A[p, q] = A[q, p] = h21[i]
    return A


def _sums(kind, terms, k, mistake=None):
    """the 32 words from the slots' kinds and the terms of the slots in reach (float64 sums in numpy's order)"""
    sums = np.zeros(32)
    sums[:28] = terms.sum(0) if len(terms) else 0.0
    n_out = int(((kind == REJECTED) | (kind == OUT)).sum())
    if mistake != "drop_out":
        sums[27] += n_out * float(huber(1.0, k)[0])
    sums[28], sums[29] = (kind == IN).sum(), (kind == IN).sum() + n_out
    return sums


def evaluate(tab, voxel, cam, Kc, surface, min_points=1, min_views=1, k=0.0, mistake=None, dtype=f32):
    """the whole evaluation -> dict(sums [32], cost, H [21], b [6], in_reach, status [8], records [S,8], kind [S], terms).
    ``dtype=np.float64``: the projection in float64 (the reference of Xc and of the slots' kinds)"""
    S = len(tab["key"])
    if rr.bad_camera(cam, Kc):
        return dict(sums=np.full(32, np.nan), cost=np.nan, H=np.full(21, np.nan), b=np.full(6, np.nan), in_reach=np.nan,
                    status=np.array([1] + [0] * 7, np.int32), records=np.full((S, 8), np.nan, f32), kind=np.full(S, ABSENT))
    h, w = np.asarray(surface).shape
    kind = rr.slot_kinds(tab, min_points, min_views)          # ABSENT, FILTERED or RENDERED (= takes part)
    part = kind == rr.RENDERED
    u, v, d, Xc = rr.project(rr.mean_points(tab, voxel), cam, Kc, dtype, "w2c" if mistake == "w2c" else None)
    rej = part & rr.rejected(u, v, d, Xc)
    inr = part & ~rej & reach(np.where(rej, 0, u), np.where(rej, 0, v), h, w)
    kind = np.where(~part, np.where(kind == rr.FILTERED, FILTERED, ABSENT), np.where(rej, REJECTED, np.where(inr, IN, OUT)))
    rec = np.full((S, 8), np.nan, dtype)
    rec[part, 5:8] = Xc[part]
    rec[part & ~rej, 0], rec[part & ~rej, 1] = u[part & ~rej], v[part & ~rej]
    at = np.flatnonzero(inr)
    r, gu, gv = sample(surface, u[at].astype(f32), v[at].astype(f32), mistake)
    rec[at, 2], rec[at, 3], rec[at, 4] = r, gu, gv
    if mistake == "right":
        terms = _right_terms(r, gu, gv, Xc[at].astype(f32), cam, Kc, k)
    else:
        terms = slot_terms(r, gu, gv, Xc[at].astype(f32), Kc, k, mistake)
    sums = _sums(kind, terms, k, mistake)
    status = np.array([0, (kind != ABSENT).sum(), (kind == FILTERED).sum(), (kind == REJECTED).sum(), (kind == OUT).sum(),
                       (kind == IN).sum(), 0, 0], np.int32)
    return dict(sums=sums, cost=sums[27], H=sums[:21], b=sums[21:27], in_reach=sums[28], status=status, records=rec, kind=kind, terms=terms)


def _right_terms(r, gu, gv, Xc, cam, Kc, k):
    """the deliberate mistake "right": rows for T <- T Exp(xi): the camera-frame row turned into the world frame"""
    J = rows(gu, gv, Xc, Kc)
    q = np.asarray(cam, f32).astype(np.float64)[3:]
    qi = q * np.array([-1.0, -1, -1, 1])
    c = np.asarray(cam, f32).astype(np.float64)[:3]
    Xw = poseref.qrot(q, Xc.astype(np.float64)) + c
    jw = poseref.qrot(q, J[:, :3])                                # dr/dXw
    Jr = np.concatenate([jw, np.cross(Xw, jw)], 1)
    rd = np.asarray(r, f32).astype(np.float64)
    rho, w = huber(rd, k)
    wj = w[:, None] * Jr
    return np.concatenate([np.stack([wj[:, p] * Jr[:, q_] for p, q_ in TRI], 1), wj * rd[:, None], rho[:, None]], 1)


def kinds_of_records(tab, records, min_points, min_views):
    """the slots' kinds from a call's own records"""
    kind = rr.slot_kinds(tab, min_points, min_views)
    part = kind == rr.RENDERED
    rec = np.asarray(records, f32)
    return np.where(~part, np.where(kind == rr.FILTERED, FILTERED, ABSENT),
                    np.where(np.isnan(rec[:, 0]), REJECTED, np.where(np.isnan(rec[:, 2]) & np.isnan(rec[:, 3]), OUT, IN)))


def evaluate_records(tab, records, Kc, surface, min_points=1, min_views=1, k=0.0):
    """From a call's OWN records: the kinds (by the reach test on the call's u, v), r, gu, gv by the fp32 emulator on the call's
    u, v, and the float64 sums of the per-slot terms formed from the call's r, gu, gv, Xc -> dict(kind, r, gu, gv (of the slots
    in reach), sums, abs_sums (the sums of the terms' magnitudes: the summation bound's scale), n [28] (the terms per word))"""
    rec = np.asarray(records, f32)
    h, w = np.asarray(surface).shape
    kind = rr.slot_kinds(tab, min_points, min_views)
    part = kind == rr.RENDERED
    rej = part & np.isnan(rec[:, 0])
    inr = part & ~rej & reach(np.where(rej, 0, rec[:, 0]), np.where(rej, 0, rec[:, 1]), h, w)
    kind = np.where(~part, np.where(kind == rr.FILTERED, FILTERED, ABSENT), np.where(rej, REJECTED, np.where(inr, IN, OUT)))
    at = np.flatnonzero(inr)
    r, gu, gv = sample(surface, rec[at, 0], rec[at, 1])
    terms = slot_terms(rec[at, 2], rec[at, 3], rec[at, 4], rec[at, 5:8], Kc, k)
    sums = _sums(kind, terms, k)
    n_out = int(((kind == REJECTED) | (kind == OUT)).sum())
    abs_sums = np.zeros(32)
    abs_sums[:28] = np.abs(terms).sum(0) if len(terms) else 0.0
    abs_sums[27] += n_out * abs(float(huber(1.0, k)[0]))
    n = np.full(28, len(at))                                  # the terms per word: the slots in reach; the cost also has n_out
    n[27] += n_out
    return dict(kind=kind, at=at, r=r, gu=gu, gv=gv, sums=sums, abs_sums=abs_sums, n=n)


def cost_at(tab, voxel, cam64, Kc, surface, k=0.0, **kw):
    """the restatement's own cost at a float64 pose (through its float32 words, as the device reads it)"""
    return float(evaluate(tab, voxel, np.asarray(cam64, np.float64).astype(f32), Kc, surface, k=k, **kw)["cost"])


# ------------------------------------------------------------------------------------------------------------ the loop
def retract(C, delta, mistake=None):
    """C' = C D^-1 for T' = D T, D = (R(dq), v), dq the Cayley map of w: plain floats, the header's order"""
    c0, c1, c2, ax, ay, az, aw = (float(v) for v in C)
    v0, v1, v2, w0, w1, w2 = (float(v) for v in delta)
    ww = (w0 * w0 + w1 * w1) + w2 * w2
    sc = math.sqrt(1.0 + ww / 4.0)
    bx, by, bz, bw = -((w0 / 2.0) / sc), -((w1 / 2.0) / sc), -((w2 / 2.0) / sc), 1.0 / sc
    qx = ((aw * bx + ax * bw) + ay * bz) - az * by
    qy = ((aw * by - ax * bz) + ay * bw) + az * bx
    qz = ((aw * bz + ax * by) - ay * bx) + az * bw
    qw = ((aw * bw - ax * bx) - ay * by) - az * bz
    nq = math.sqrt(((qx * qx + qy * qy) + qz * qz) + qw * qw)
    qx, qy, qz, qw = qx / nq, qy / nq, qz / nq, qw / nq
    u0, u1, u2 = qy * v2 - qz * v1, qz * v0 - qx * v2, qx * v1 - qy * v0
    u0, u1, u2 = u0 + u0, u1 + u1, u2 + u2
    return [c0 - ((v0 + qw * u0) + (qy * u2 - qz * u1)), c1 - ((v1 + qw * u1) + (qz * u0 - qx * u2)),
            c2 - ((v2 + qw * u2) + (qx * u1 - qy * u0)), qx, qy, qz, qw]


def _tri(i, j):
    return i * 6 - (i * (i - 1)) // 2 + (j - i)


class Machine:
    """the state of the header's definition, by its names; ``step(e, cost, H21, b, in_reach, status)`` behind every evaluation"""

    def __init__(self, cam0, lambda0=1e-3, min_step=1e-6, iters=10, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.cam = np.asarray(cam0, f32).reshape(7).copy()   # what the next evaluation reads
        self.cam_C = self.cam.copy()
        self.C = [float(v) for v in self.cam]
        self.lam, self.min_step, self.iters, self.mistake = float(lambda0), float(min_step), int(iters), mistake
        self.f = self.f0 = self.reach = 0.0
        self.H, self.b, self.trial = [0.0] * 21, [0.0] * 6, [0.0] * 7
        self.n_accepted = self.n_evals = self.rejects = self.reason = self.seen = 0
        self.history = [float("nan")] * self.iters
        self.status = [0] * 8

    def propose(self):
        H, b, lam = self.H, self.b, self.lam
        L = [[0.0] * 6 for _ in range(6)]
        for j in range(6):
            s = H[_tri(j, j)] + lam * H[_tri(j, j)]
            for k in range(j):
                s = s - L[j][k] * L[j][k]
            if not (s > 0.0 and s < float("inf")):
                self.reason = SINGULAR
                return
            L[j][j] = math.sqrt(s)
            for i in range(j + 1, 6):
                t = H[_tri(j, i)]
                for k in range(j):
                    t = t - L[i][k] * L[j][k]
                L[i][j] = t / L[j][j]
        y, delta = [0.0] * 6, [0.0] * 6
        for i in range(6):
            t = -b[i]
            for k in range(i):
                t = t - L[i][k] * y[k]
            y[i] = t / L[i][i]
        for i in range(5, -1, -1):
            t = y[i]
            for k in range(i + 1, 6):
                t = t - L[k][i] * delta[k]
            delta[i] = t / L[i][i]
        dd = 0.0
        for v in delta:
            dd = dd + v * v
        self.delta = delta
        if math.sqrt(dd) < self.min_step:
            self.reason = CONVERGED
            return
        self.trial = retract(self.C, delta)
        self.cam = alignref.f32(self.trial)

    def step(self, e, cost, H21, b, in_reach, status):
        if self.reason != 0:
            return
        cost, in_reach = float(cost), float(in_reach)
        self.n_evals += 1
        self.seen |= int(status[0])
        take = False
        if e == 0:
            self.f = self.f0 = cost
            take = True
            if in_reach < 6.0:
                self.reason = FEW
            elif self.iters == 0:
                self.reason = ITERS
        elif cost < self.f:
            self.C, self.f, take = list(self.trial), cost, True
            self.history[self.n_accepted] = cost
            self.n_accepted += 1
            self.lam = max(self.lam / 10.0, 1e-12)
            self.rejects = 0
            if self.n_accepted == self.iters:
                self.reason = ITERS
            elif in_reach < 6.0:
                self.reason = FEW
        else:
            self.lam = (self.lam * 0.5) if self.mistake == "halve" else (self.lam * 10.0)
            self.rejects += 1
            if self.rejects == REJECTS:
                self.reason = STALLED
        if take:
            self.H, self.b, self.reach = [float(v) for v in H21], [float(v) for v in b], in_reach
            self.status, self.cam_C = [int(w) for w in status], self.cam.copy()
        if self.reason == 0:
            self.propose()


def localize(evaluate_fn, cam0, lambda0=1e-3, min_step=1e-6, iters=10, max_evals=None, mistake=None):
    """drives the machine over ``evaluate_fn(pose_f32) -> (cost, H[21], b[6], in_reach, status[8])`` -> the outputs of
    ramp_point_map_localize as numpy arrays, by their names"""
    need = 1 + (REJECTS + 1) * int(iters)
    budget = need if max_evals is None or max_evals <= 0 else min(int(max_evals), need)
    m = Machine(cam0, lambda0, min_step, iters, mistake)
    for e in range(budget):
        if m.reason != 0:
            break                                             # (the device enqueues the rest as empty launches)
        out = evaluate_fn(m.cam.copy())
        m.step(e, *out)
    if m.reason == 0:
        m.reason = BUDGET
    no_pose = (m.n_accepted == 0 and m.reason in (FEW, SINGULAR)) or bool(m.seen & BAD_CAMERA)
    nan = float("nan")
    return dict(pose=np.full(7, nan) if no_pose else np.asarray(m.C, np.float64),
                pose_f32=np.full(7, nan, f32) if no_pose else m.cam_C,
                result=np.asarray([m.f, m.f0, m.lam, m.reach], np.float64), hessian=full(m.H), gradient=np.asarray(m.b, np.float64),
                history=np.asarray(m.history, np.float64), status=np.asarray(m.status, np.int32), reason=m.reason,
                info=np.asarray([m.reason, m.n_accepted, m.n_evals, m.rejects, m.seen, 0, 0, 0], np.int32), machine=m)


def ref_evaluator(tab, voxel, Kc, surface, k=0.0, mistake=None, **kw):
    """``evaluate`` as the callable ``localize`` drives"""
    def fn(pose32):
        o = evaluate(tab, voxel, pose32, Kc, surface, k=k, mistake=mistake, **kw)
        return o["cost"], o["H"], o["b"], o["in_reach"], o["status"]
    return fn


# -------------------------------------------------------------------------------------------------------------- inputs
def pose_distance(a, b):
    """(translation distance, rotation angle) between two camera-to-world poses, float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    qa, qb = a[3:] / np.linalg.norm(a[3:]), b[3:] / np.linalg.norm(b[3:])
    dq = poseref.qmul(qa * [-1, -1, -1, 1], qb)
    return float(np.linalg.norm(a[:3] - b[:3])), float(2 * math.atan2(np.linalg.norm(dq[:3]), abs(dq[3])))


def grid_margin(a):
    """the distance of every value from an integer"""
    a = np.asarray(a, np.float64)
    return np.abs(a - np.rint(a))


def half_margin(a):
    """the distance of every value from a rounding switch k + 0.5"""
    a = np.asarray(a, np.float64)
    return np.abs(a - np.floor(a) - 0.5)


def uv_margin(tab, voxel, cam, Kc, min_points=1, min_views=1):
    """the smallest distance of a participating, not rejected slot's float64 u, v from an integer (a cell boundary, and the
    reach test's switch)"""
    kind = rr.slot_kinds(tab, min_points, min_views)
    u, v, d, Xc = rr.project(rr.mean_points(tab, voxel), cam, Kc, np.float64)
    live = (kind == rr.RENDERED) & ~rr.rejected(u, v, d, Xc)
    with np.errstate(all="ignore"):
        m = np.minimum(grid_margin(u), grid_margin(v))[live]
    return float(m.min()) if len(m) else np.inf


def loc_cloud(N, seed=0, cam=CAM, Kc=K, voxel=VOXEL, views=(3, 4)):
    """``renderref.cloud_case`` with the voxels whose u or v lies within 2 MARGIN of an integer left out HERE -> inserts of
    exactly ``N`` voxels (the rejected ones, behind the camera and nearer than RAMP_WARP_MIN_Z, stay)"""
    if N == 0:
        return []
    if N <= 8:                                                # a few voxels, all inside the image: one to three points each
        rng = np.random.default_rng(400 + seed)
        M = 4 * N + 8
        p = pm.lift(rng.uniform(2, W - 3, M), rng.uniform(2, H - 3, M), 1.0 / rng.uniform(0.45, 4.0, M), cam, Kc, np.float64).astype(f32)
        per = rng.integers(1, 4, M)
        pts = np.repeat(p, per, 0) + rng.uniform(-0.02, 0.02, (per.sum(), 3)).astype(f32)
        ins = [(pts, rng.uniform(0.5, 4.0, len(pts)).astype(f32), views[0])]
    else:
        ins = rr.cloud_case(int(N * 1.2), seed=seed, cam=cam, Kc=Kc, voxel=voxel, views=(views[0],))
    (pts, conf, _), = ins
    tab = rr.table_of(ins, voxel)
    u, v, d, Xc = rr.project(rr.mean_points(tab, voxel), cam, Kc, np.float64)
    rej = rr.rejected(u, v, d, Xc)
    with np.errstate(all="ignore"):
        near = ~rej & (np.minimum(grid_margin(u), grid_margin(v)) < 2 * MARGIN)
    keys = np.r_[tab["key"][rej], tab["key"][~rej & ~near]][:N]
    assert len(keys) == N, (N, len(keys))
    sel = np.isin(pm.fixed(pts, conf, voxel)["key"], keys)
    pts, conf = pts[sel], conf[sel]
    cut = np.linspace(0, len(pts), len(views) + 1).astype(int)
    return [(pts[a:b], conf[a:b], view) for a, b, view in zip(cut[:-1], cut[1:], views)]


def surface_13x17(seed=0):
    """a smooth-ish random field in (0, 1) over the small image, for the evaluation's cases"""
    rng = np.random.default_rng(500 + seed)
    return binomial(rng.uniform(0, 1, (H, W)).astype(f32), 1)


def event_case(N, seed=0, h=H, w=W, t_ref=2.0):
    """events over the image and half a pixel around it, coordinates at least 2 MARGIN from a rounding switch, time stamps
    on both sides of t_ref and of zero"""
    rng = np.random.default_rng(700 + seed)
    x, y = rng.uniform(-1.2, w + 0.2, 3 * N + 8), rng.uniform(-1.2, h + 0.2, 3 * N + 8)
    ok = (half_margin(x.astype(f32)) >= 2 * MARGIN) & (half_margin(y.astype(f32)) >= 2 * MARGIN)
    x, y = x[ok][:N].astype(f32), y[ok][:N].astype(f32)
    assert len(x) == N
    t = rng.uniform(-1.0, t_ref + 0.4, N)
    return x, y, t


CONV = dict(h=48, w=64, K=np.array([40.0, 40.0, 31.5, 23.25], f32), voxel=0.02, t_ref=10.0, tau=0.05, smooth=2, n=288, blob=3,
            true=np.array([0.1, -0.05, 0.2, 0.02, -0.03, 0.01, 0.9993], np.float64),
            perturb=np.array([0.02, -0.015, 0.01, 0.008, -0.006, 0.01]), iters=20, huber=0.0)


_conv = {}


def convergence_scene():
    """-> dict(inserts, tab, voxel, K, h, w, events (x, y, t), t_ref, tau, smooth, surface (the restatement's), true, start
    (float32 [7]), iters).  A map of a few hundred voxels on two planes in front of the true pose, one point per voxel, in blobs of 3 x 3 pixels whose
    projections lie within 0.15 of a pixel's centre (isolated points leave the smoothed surface almost flat); events
    at the voxels' projections from the true pose, time stamps within tau / 5 before t_ref; the start is the true pose moved
    by ``CONV["perturb"]`` through ``retract``."""
    if _conv:
        return _conv
    s = CONV
    rng = np.random.default_rng(900)
    true = s["true"].copy()
    true[3:] /= np.linalg.norm(true[3:])
    true32 = true.astype(f32)
    b, nb = s["blob"], s["n"] // s["blob"] ** 2
    cu, cv = np.rint(rng.uniform(5, s["w"] - 6 - b, nb)), np.rint(rng.uniform(5, s["h"] - 6 - b, nb))
    g = np.arange(b, dtype=np.float64)
    n = nb * b * b
    uu = (cu[:, None, None] + g[None, :, None] + 0 * g[None, None, :]).reshape(-1) + 0.15 * rng.uniform(-1, 1, n)
    vv = (cv[:, None, None] + 0 * g[None, :, None] + g[None, None, :]).reshape(-1) + 0.15 * rng.uniform(-1, 1, n)
    z = np.repeat(np.where(np.arange(nb) % 2 == 0, 2.0, 3.5), b * b) + 0.1 * (uu / s["w"])      # two (slightly tilted) planes
    pts = pm.lift(uu, vv, 1.0 / z, true32, s["K"], np.float64).astype(f32)
    ins = [(pts, np.ones(n, f32), 1)]
    tab = rr.table_of(ins, s["voxel"])
    u, v, d, Xc = rr.project(rr.mean_points(tab, s["voxel"]), true32, s["K"], np.float64)
    ok = (half_margin(u.astype(f32)) >= 2 * MARGIN) & (half_margin(v.astype(f32)) >= 2 * MARGIN)
    x, y = u[ok].astype(f32), v[ok].astype(f32)
    t = s["t_ref"] - rng.uniform(0, s["tau"] / 5, len(x))
    surf = time_surface(x, y, t, s["t_ref"], s["tau"], s["h"], s["w"], s["smooth"])["surface"]
    start = alignref.f32(retract(list(true32.astype(np.float64)), s["perturb"]))
    _conv.update(inserts=ins, tab=tab, voxel=s["voxel"], K=s["K"], h=s["h"], w=s["w"], events=(x, y, t), t_ref=s["t_ref"], tau=s["tau"],
                 smooth=s["smooth"], surface=surf, true=true32, start=start, iters=s["iters"], huber=s["huber"])
    return _conv


def collinear_case():
    """six voxels on one line through the scene, all in reach of CAM"""
    z = np.linspace(1.0, 3.0, 6)
    uu, vv = 3.3 + 1.9 * np.arange(6), 2.7 + 1.3 * np.arange(6)
    p0, p1 = (pm.lift(uu[[i]], vv[[i]], 1.0 / z[[i]], CAM, K, np.float64)[0] for i in (0, 5))
    pts = np.stack([p0 + (p1 - p0) * s for s in np.linspace(0, 1, 6)]).astype(f32)
    return [(pts, np.ones(6, f32), 1)]
