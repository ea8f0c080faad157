"""float64 restatements of the pose-geometry and frame-bookkeeping operators -- TEST INFRASTRUCTURE ONLY.

Plain numpy in float64 over the oracle's ``se3_*_f64`` (the reference's SE3 formulas evaluated in double): what
``csrc/lie.hip`` and the frame launches of ``csrc/select.hip`` compute, stated once more without any of their structure
(no tiles, no strides, no reductions in a fixed order).  Inputs are taken as they are -- a test rounds them to float32
first, so the kernel and the restatement read the same numbers -- and everything is returned in float64.

The checks: ``bound(floor, env)`` is the one tolerance rule of tests/test_geometry_f64_gpu.py, ``Table`` collects
(measured, envelope, bound) per input bin, prints them and says which bins failed; ``same_bits`` compares words.
"""
import numpy as np

import oracle as orc
import poseref

ENV_FACTOR = 4.0             # as test_ba_matches_oracle: a device cosf / sinf / atanf a few ulp from the host's
# unit-scale floors of test_se3_ops_match_oracle, per operator
FLOOR = dict(exp=2e-6, inv=2e-6, mul=2e-6, log=5e-6, act4=5e-6, adj=1e-5, adjT=1e-5)
PIXEL_FLOOR = 1e-5           # x the largest coordinate, as test_transform_reproject_point_cloud
Z_CLAMP = 0.1                # ramp/projective_ops.py: proj() clamps Z at 0.1
Z_SKIP = 1e-2                # reproject has no clamp: elements with |Z| below this are left out of a comparison


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------- projective ops
def _unproject(patches, K):
    """patches [E,3,P,P] pixels + inverse depth, K [E,4] -> homogeneous points [E,P*P,4]"""
    E = patches.shape[0]
    x, y, d = (patches[:, c].reshape(E, -1) for c in range(3))
    return np.stack([(x - K[:, 2:3]) / K[:, 0:1], (y - K[:, 3:4]) / K[:, 1:2], np.ones_like(x), d], -1)


def _project(X1, K, clamp):
    Z = X1[..., 2]
    if clamp:
        Z = np.maximum(Z, Z_CLAMP)
    return np.stack([K[:, 0:1] * (X1[..., 0] / Z) + K[:, 2:3], K[:, 1:2] * (X1[..., 1] / Z) + K[:, 3:4]], 1)


def transform(poses, patches, intr, ii, jj, kk, tonly=False, want_z=False):
    """pops.transform (ramp/projective_ops.py:50-101) -> [1,E,2,P,P]: unproject with the intrinsics of frame i, move by
    G = T_j T_i^-1 (its rotation dropped with ``tonly``), project with the intrinsics of frame j, Z clamped at 0.1"""
    poses, patches, intr = f64(poses).reshape(-1, 7), f64(patches), f64(intr).reshape(-1, 4)
    P = patches.shape[-1]
    patches = patches.reshape(-1, 3, P, P)
    E = len(ii)
    if E == 0:
        return np.zeros((1, 0, 2, P, P))
    G = orc.se3_mul_f64(poses[jj], orc.se3_inv_f64(poses[ii]))
    if tonly:
        G[:, 3:] = [0, 0, 0, 1]
    X1 = orc.se3_act4_f64(G[:, None, :], _unproject(patches[kk], intr[ii]))
    out = _project(X1, intr[jj], clamp=True).reshape(1, E, 2, P, P)
    return (out, X1[..., 2].reshape(E, P, P)) if want_z else out


def reproject(poses, patches, intr, ii, jj, kk, want_z=False):
    """fastba's reproject (ramp/fastba/ba_cuda.cu:379-429) -> [1,E,2,P,P]: intrinsics row 0 for every frame, no clamp,
    quaternions as stored (not normalised)"""
    poses, patches, intr = f64(poses).reshape(-1, 7), f64(patches), f64(intr).reshape(-1, 4)
    P = patches.shape[-1]
    patches = patches.reshape(-1, 3, P, P)
    E = len(ii)
    if E == 0:
        return np.zeros((1, 0, 2, P, P))
    ti, qi, tj, qj = poses[ii, :3], poses[ii, 3:], poses[jj, :3], poses[jj, 3:]
    a, b = qj, qi * np.array([-1.0, -1.0, -1.0, 1.0])                       # q_ij = q_j q_i^-1
    qij = np.concatenate([a[:, 3:] * b[:, :3] + b[:, 3:] * a[:, :3] + np.cross(a[:, :3], b[:, :3]),
                          a[:, 3:] * b[:, 3:] - (a[:, :3] * b[:, :3]).sum(-1, keepdims=True)], -1)
    tij = tj - poseref.qrot(qij, ti)
    K0 = np.broadcast_to(intr[0], (E, 4))
    X0 = _unproject(patches[kk], K0)
    X1 = poseref.qrot(qij[:, None, :], X0[..., :3]) + tij[:, None, :] * X0[..., 3:]
    out = _project(X1, K0, clamp=False).reshape(1, E, 2, P, P)
    return (out, X1[..., 2].reshape(E, P, P)) if want_z else out


def point_cloud(poses, patches, intr, ix):
    """pops.point_cloud + Ramp_vo.py:308-310 -> [m,3]: the centre pixel of patch n, unprojected with the intrinsics of its
    frame ix[n], in world coordinates"""
    poses, patches, intr = f64(poses).reshape(-1, 7), f64(patches), f64(intr).reshape(-1, 4)
    P = patches.shape[-1]
    m = len(ix)
    c = patches.reshape(-1, 3, P, P)[:m, :, P // 2, P // 2]
    K = intr[ix]
    X0 = np.stack([(c[:, 0] - K[:, 2]) / K[:, 0], (c[:, 1] - K[:, 3]) / K[:, 1], np.ones(m), c[:, 2]], -1)
    Pw = orc.se3_act4_f64(orc.se3_inv_f64(poses[ix]), X0)
    return Pw[:, :3] / Pw[:, 3:]


def flow_mag(poses, patches, intr, ii, jj, kk, beta, xform=transform):
    """pops.flow_mag (ramp/projective_ops.py:108-118) -> [E,P,P]; ``xform`` lets a test evaluate the same statement over the
    fp32 oracle's transform (the envelope of the reference formulas)"""
    c0 = xform(poses, patches, intr, ii, ii, kk, False)[0]
    c1 = xform(poses, patches, intr, ii, jj, kk, False)[0]
    c2 = xform(poses, patches, intr, ii, jj, kk, True)[0]
    T = c0.dtype.type
    f1 = np.sqrt(((c1 - c0) ** 2).sum(1, dtype=c0.dtype))
    f2 = np.sqrt(((c2 - c0) ** 2).sum(1, dtype=c0.dtype))
    return T(beta) * f1 + (T(1) - T(beta)) * f2


def motionmag(poses, patches, intr, ii, jj, kk, keys, key, beta, xform=transform):
    """one direction of Ramp_vo.motionmag (ramp/Ramp_vo.py:227-243): the mean flow magnitude over the factors whose pair
    key equals ``key`` and their P*P pixels; NaN without such a factor"""
    sel = np.nonzero(np.asarray(keys) == key)[0]
    if len(sel) == 0:
        return float("nan")
    f = flow_mag(poses, patches, intr, ii[sel], jj[sel], kk[sel], beta, xform).astype(np.float64)
    return f.sum() / f.size


# ---------------------------------------------------------------------------------------------------------- motion model
def motion_model(poses, n, damping):
    """DAMPED_LINEAR (ramp/Ramp_vo.py:356-363): Exp(damping * Log(P[n-1] P[n-2]^-1)) P[n-1] -> [7]"""
    poses = f64(poses).reshape(-1, 7)
    P1, P2 = poses[n - 1:n], poses[n - 2:n - 1]
    xi = orc.se3_log_f64(orc.se3_mul_f64(P1, orc.se3_inv_f64(P2)))
    return orc.se3_mul_f64(orc.se3_exp_f64(float(damping) * xi), P1)[0]


def motion_model_f32(poses, n, damping):
    """the same statement over the fp32 oracle (the envelope of the reference's float formulas)"""
    poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
    P1, P2 = poses[n - 1:n], poses[n - 2:n - 1]
    xi = orc.se3_log(orc.se3_mul(P1, orc.se3_inv(P2)))
    return orc.se3_mul(orc.se3_exp(np.float32(damping) * xi), P1)[0]


def pose_err(a, b):
    """largest element difference of two poses / pose arrays, the quaternion compared up to its sign"""
    a, b = f64(a), f64(b)
    dq = np.minimum(np.abs(a[..., 3:] - b[..., 3:]).max(-1), np.abs(a[..., 3:] + b[..., 3:]).max(-1))
    dt = np.abs(a[..., :3] - b[..., :3]).max(-1)
    return float(np.maximum(dq, dt).max()) if dq.size else 0.0


# ------------------------------------------------------------------------------------------------------ exact bookkeeping
def shift_rows(buf, k, nrows, mod=0):
    """keyframe removal on one buffer [slots, ...]: rows k+1 .. nrows-1 move down by one; a ring buffer (mod > 0) holds row
    r in slot r % mod.  Returns a copy"""
    out = np.array(buf, copy=True)
    slot = (lambda r: r % mod) if mod else (lambda r: r)
    for r in range(k, nrows - 1):
        out[slot(r)] = out[slot(r + 1)]
    return out


def lower_median(x):
    """torch.median: the lower of the two middle values of an even count"""
    s = np.sort(np.asarray(x).reshape(-1))
    return s[(len(s) - 1) // 2]


def same_bits(a, b):
    """equality of two arrays as 32-bit words (NaN patterns compare by their bits)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------------------ the checks
def bound(floor, env):
    """the one tolerance rule: the project's unit-scale bound of the operator, or four envelopes of the reference's own
    float formulas against float64, whichever is larger"""
    return max(float(floor), ENV_FACTOR * float(env))


def max_err(out, ref, keep=None):
    d = np.abs(f64(out) - f64(ref))
    if keep is not None:
        d = d[keep]
    return float(d.max()) if d.size else 0.0


class Table:
    """(measured, envelope, bound) per bin: printed by the test, asserted once at the end so that a failing run still shows
    every figure"""

    def __init__(self, title):
        self.title, self.rows = title, []

    def add(self, name, err, env, floor):
        b = bound(floor, env)
        ok = bool(np.isfinite(err)) and err <= b
        self.rows.append((name, float(err), float(env), b, ok))
        return ok

    def failed(self):
        return [r[0] for r in self.rows if not r[4]]

    def show(self):
        print("\n%s" % self.title)
        print("  %-34s %10s %10s %10s  %6s" % ("bin", "measured", "envelope", "bound", "err/env"))
        for name, err, env, b, ok in self.rows:
            print("  %-34s %10.2e %10.2e %10.2e  %6s%s" % (name, err, env, b, ("%.2f" % (err / env)) if env > 0 else "-",
                                                         "" if ok else "   <-- FAILS"))


# ---------------------------------------------------------------------------------------------------------------- scenes
def geo_scene(seed, n_frames=8, M=40, E=257, H=120, W=160):
    """float32 scene for the projective operators: every frame has intrinsics of its own (fx, fy, cx, cy 10-30 % apart),
    inverse depths from 1e-6 to 1.2, the cameras advance along z by ~0.8 per frame, so that for an edge to an earlier
    frame a tenth of the patches (inverse depth 1.5-4) lie behind the target camera and another tenth (Z = 0.1 +- 0.1)
    straddle the clamp.  Edges: E random (i, j, k) with k a patch of frame i"""
    rng = np.random.default_rng(seed)
    xi = np.cumsum(rng.normal(0, [0.05, 0.03, 0.02, 0.02, 0.02, 0.02], (n_frames, 6)), 0)
    xi[:, 2] += 0.8 * np.arange(n_frames)
    poses = orc.se3_exp_f64(xi).astype(np.float32)
    base = np.array([W * 0.5, W * 0.5, W * 0.5, H * 0.5])
    intr = (base * (1.0 + rng.choice([-1, 1], (n_frames, 4)) * rng.uniform(0.10, 0.30, (n_frames, 4)))).astype(np.float32)
    n_p = n_frames * M
    gy, gx = np.meshgrid(np.arange(-1, 2), np.arange(-1, 2), indexing="ij")
    patches = np.zeros((n_p, 3, 3, 3), np.float32)
    patches[:, 0] = rng.uniform(8, W - 8, (n_p, 1, 1)) + gx
    patches[:, 1] = rng.uniform(8, H - 8, (n_p, 1, 1)) + gy
    d = np.exp(rng.uniform(np.log(1e-6), np.log(1.2), n_p))
    kind = rng.permutation(n_p) % 10
    d[kind == 0] = rng.uniform(1.5, 4.0, (kind == 0).sum())                 # behind an earlier camera
    d[kind == 1] = (0.9 + rng.uniform(-0.1, 0.1, (kind == 1).sum())) / 0.8  # at the clamp for the previous frame
    patches[:, 2] = d[:, None, None]
    kk = rng.integers(0, n_p, E).astype(np.int64)
    ii = kk // M
    jj = np.clip(ii + rng.integers(-3, 4, E), 0, n_frames - 1).astype(np.int64)
    return dict(poses=poses, patches=patches, intr=intr, ii=ii, jj=jj, kk=kk, n_frames=n_frames, M=M)


PAIR_MUL = 16                # pair keys are jj * PAIR_MUL + ii, as Ramp_vo's graph plan makes them


def mm_case(seed, i, j, n_ij, n_ji, n_other=96):
    """factors for the motion test on geo_scene(seed): n_ij factors i -> j, n_ji factors j -> i and n_other factors of
    other pairs whose target frame is 1 .. 6, shuffled.  With (i, j) = (0, 2) the key of j -> i is the first of the sorted
    unique keys, with (5, 7) the key of i -> j is the last"""
    s = geo_scene(seed)
    rng = np.random.default_rng(seed + 1000)
    M, n = s["M"], s["n_frames"]
    oi = rng.integers(0, n, n_other)
    oj = rng.integers(1, 7, n_other)
    clash = ((oi == i) & (oj == j)) | ((oi == j) & (oj == i))
    oj[clash] = 1 + (oj[clash] % 6)
    clash = ((oi == i) & (oj == j)) | ((oi == j) & (oj == i))
    oi[clash] = (oi[clash] + 1) % n
    ii = np.concatenate([np.full(n_ij, i), np.full(n_ji, j), oi]).astype(np.int64)
    jj = np.concatenate([np.full(n_ij, j), np.full(n_ji, i), oj]).astype(np.int64)
    kk = (ii * M + rng.integers(0, M, len(ii))).astype(np.int64)
    perm = rng.permutation(len(ii))
    ii, jj, kk = ii[perm], jj[perm], kk[perm]
    s.update(ii=ii, jj=jj, kk=kk, keys=jj * PAIR_MUL + ii, key_ij=j * PAIR_MUL + i, key_ji=i * PAIR_MUL + j)
    return s
