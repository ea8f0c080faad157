"""Numpy restatement of the event map (include/ramp_hip.h ``ramp_depth_points``, ``ramp_point_map_*``) -- TEST INFRASTRUCTURE ONLY.

(a) ``masked_median``: the lower median over the detected pixels of the clipped window, in the order of the floats' bits mapped
    to unsigned words (csrc/median.h) -- exact.  ``lift``: the statements of the header in float64 (the reference) or float32
    (the header's own rounding: bit for bit what the kernel computes, and the envelope of the GPU test's bound).
    ``depth_points``: the whole call.

(b) the voxel hash in integers: ``fixed`` (keys and fixed point per point), ``PointMapRef`` (``np.unique`` over the keys, integer
    sums with ``np.add.at``, the export).  ``slot`` is the table's hash.

(c) the ``mistake`` keywords break the restatement on purpose (tests/test_pointmapref_cpu.py: each has to be rejected by the
    inputs the GPU test uses, which are built here: ``depth_case``, ``map_points``).
"""
import numpy as np

import poseref

AXIS = 1 << 20
CONF_BITS = 16
H, W = 13, 17
K = np.array([16.0, 12.0, 8.5, 6.25], np.float32)
CAM = np.array([0.3, -0.2, 0.5, 0.18257419, -0.36514837, 0.54772256, 0.73029674], np.float32)       # camera to world
IDENTITY = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
FILTER_MISTAKES = ("upper_median", "unclipped", "support_no_centre")
LIFT_MISTAKES = ("w2c",)
MAP_MISTAKES = ("trunc", "xy_key", "view_nowrap")
MASKS = ("empty", "full", "one", "checker", "random")


def key32(a):
    """csrc/median.h's order-preserving map of a float32's bits to an unsigned word"""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def detected(inv, plane=None):
    inv = np.asarray(inv, np.float32)
    return (np.asarray(plane) >= 0) if plane is not None else (np.isfinite(inv) & (inv > 0))


def masked_median(inv, det, r, s, mistake=None):
    """-> (value float32 [H,W]: the filtered value of a detected pixel that is not isolated, NaN elsewhere; isolated bool)"""
    assert mistake is None or mistake in FILTER_MISTAKES
    inv = np.asarray(inv, np.float32)
    h, w = inv.shape
    keys = key32(inv)
    out = np.full((h, w), np.nan, np.float32)
    iso = np.zeros((h, w), bool)
    for v in range(h):
        for u in range(w):
            if not det[v, u]:
                continue
            if mistake == "unclipped":                     # the window wraps around instead of ending at the border
                ys, xs = np.arange(v - r, v + r + 1) % h, np.arange(u - r, u + r + 1) % w
            else:
                ys, xs = np.arange(max(v - r, 0), min(v + r, h - 1) + 1), np.arange(max(u - r, 0), min(u + r, w - 1) + 1)
            m = det[np.ix_(ys, xs)]
            n = int(m.sum())
            if (n - 1 if mistake == "support_no_centre" else n) < s:
                iso[v, u] = True
                continue
            vals, ks = inv[np.ix_(ys, xs)][m], keys[np.ix_(ys, xs)][m]
            order = np.argsort(ks, kind="stable")
            out[v, u] = vals[order[n // 2 if mistake == "upper_median" else (n - 1) // 2]]
    return out, iso


def lift(u, v, d, cam, Kc, dtype=np.float64, mistake=None):
    """world points [n,3] of pixels (u, v) with inverse depth d, in ``dtype`` (the inputs are the float32 words either way)"""
    assert mistake is None or mistake in LIFT_MISTAKES
    cam = np.asarray(cam, np.float32)
    if mistake == "w2c":
        cam = poseref.invert_pose(cam).astype(np.float32)
    c, k = cam.astype(dtype), np.asarray(Kc, np.float32).astype(dtype)
    with np.errstate(all="ignore"):
        z = dtype(1.0) / np.asarray(d, np.float32).astype(dtype)
        Xc = np.stack([((np.asarray(u).astype(dtype) - k[2]) / k[0]) * z, ((np.asarray(v).astype(dtype) - k[3]) / k[1]) * z, z], -1)
        return (poseref.qrot(c[3:], Xc) + c[:3]).astype(dtype)


def depth_points(inv, cam, Kc, plane=None, confidence=None, r=2, s=3, min_invdepth=0.0, mistake=None):
    """the whole call -> dict(filtered, pixel, conf, count, status [8], points32 (bit for bit), points64 (the reference))"""
    inv = np.asarray(inv, np.float32)
    h, w = inv.shape
    cam, Kc = np.asarray(cam, np.float32), np.asarray(Kc, np.float32)
    status = np.zeros(8, np.int32)
    nan = np.full((h, w), np.nan, np.float32)
    if not (np.isfinite(cam).all() and np.isfinite(Kc).all() and Kc[0] != 0 and Kc[1] != 0):
        status[0] = 1
        return dict(filtered=nan, pixel=np.zeros(0, np.int32), conf=np.zeros(0, np.float32), count=0, status=status,
                    points32=np.zeros((0, 3), np.float32), points64=np.zeros((0, 3)))
    det = detected(inv, plane)
    fm = mistake if mistake in FILTER_MISTAKES else None
    val, iso = masked_median(inv, det, r, s, fm)
    cand = det & ~iso
    vv, uu = np.mgrid[0:h, 0:w]
    lm = mistake if mistake in LIFT_MISTAKES else None
    with np.errstate(all="ignore"):
        ok = cand & np.isfinite(val) & (val > 0) & ~(val < np.float32(min_invdepth))
        p32 = lift(uu, vv, np.where(ok, val, np.float32(1)), cam, Kc, np.float32, lm)
    ok &= np.isfinite(p32).all(-1)
    pix = np.flatnonzero(ok.reshape(-1)).astype(np.int32)
    d = val.reshape(-1)[pix]
    u, v = pix % w, pix // w
    cf = np.ones(len(pix), np.float32) if confidence is None else np.asarray(confidence, np.float32).reshape(-1)[pix]
    status[1:5] = det.sum(), iso.sum(), (cand & ~ok).sum(), ok.sum()
    return dict(filtered=np.where(ok, val, np.float32(np.nan)).astype(np.float32), pixel=pix, conf=cf, count=len(pix), status=status,
                points32=lift(u, v, d, cam, Kc, np.float32, lm), points64=lift(u, v, d, cam, Kc, np.float64, lm))


# ------------------------------------------------------------------------------------------------------- the voxel hash
def fixed(points, conf, voxel, mistake=None):
    """per point -> dict(kind int [N]: 0 accumulated, 1 not finite, 2 out of range; key int64, q int64 [N,3], c int64)"""
    assert mistake is None or mistake in MAP_MISTAKES
    p = np.asarray(points, np.float32).reshape(-1, 3)
    cf = np.ones(len(p), np.float32) if conf is None else np.asarray(conf, np.float32).reshape(-1)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(p).all(1) | ~np.isfinite(cf) | (cf < 0)
        g = np.where(bad[:, None], 0.0, p.astype(np.float64)) / np.float64(voxel)
        i = np.trunc(g) if mistake == "trunc" else np.floor(g)
        outside = ~bad & ~(np.abs(i) < AXIS).all(1)
        i = np.where((bad | outside)[:, None], 0.0, i)
        q = np.rint((np.where((bad | outside)[:, None], 0.0, g) - i) * AXIS).astype(np.int64)
        c = np.rint(np.minimum(np.where(bad, 0.0, cf.astype(np.float64)), float(AXIS)) * (1 << CONF_BITS)).astype(np.int64)
    ii = i.astype(np.int64) + AXIS
    a, b = (1, 0) if mistake == "xy_key" else (0, 1)
    key = (ii[:, a] << 42) | (ii[:, b] << 21) | ii[:, 2]
    return dict(kind=np.where(bad, 1, np.where(outside, 2, 0)), key=key, q=q, c=c)


def make_key(ix, iy, iz):
    return ((int(ix) + AXIS) << 42) | ((int(iy) + AXIS) << 21) | (int(iz) + AXIS)


def slot(key, capacity):
    """the finaliser of splitmix64, masked"""
    m = (1 << 64) - 1
    z = int(key) & m
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m
    return (z ^ (z >> 31)) & (capacity - 1)


class PointMapRef:
    """the table without its capacity: every accumulated point is kept, the export groups them"""

    def __init__(self, voxel, mistake=None):
        self.voxel, self.mistake = float(voxel), mistake
        self.key, self.q, self.c, self.bit = [np.zeros(0, np.int64)], [np.zeros((0, 3), np.int64)], [np.zeros(0, np.int64)], [np.zeros(0, np.uint64)]

    def insert(self, points, conf=None, view=0):
        """-> the call's status words [1] .. [5] (no table: nothing is dropped-full)"""
        f = fixed(points, conf, self.voxel, self.mistake)
        ok = f["kind"] == 0
        bit = (1 << view) & ((1 << 64) - 1) if self.mistake == "view_nowrap" else 1 << (view & 63)
        self.key.append(f["key"][ok]); self.q.append(f["q"][ok]); self.c.append(f["c"][ok])
        self.bit.append(np.full(int(ok.sum()), bit, np.uint64))
        return np.array([0, len(ok), (f["kind"] == 1).sum(), (f["kind"] == 2).sum(), 0, ok.sum()], np.int32)

    def export(self, min_points=1, min_views=1, max_out=None):
        key, q, c, bit = (np.concatenate(v) for v in (self.key, self.q, self.c, self.bit))
        uk, inv = np.unique(key, return_inverse=True)
        n, sq, sc, views = np.zeros(len(uk), np.int64), np.zeros((len(uk), 3), np.int64), np.zeros(len(uk), np.int64), np.zeros(len(uk), np.uint64)
        np.add.at(n, inv, 1); np.add.at(sq, inv, q); np.add.at(sc, inv, c); np.bitwise_or.at(views, inv, bit)
        nv = np.array([bin(int(v)).count("1") for v in views], np.int32)
        keep = (n >= min_points) & (nv >= min_views)
        passing = int(keep.sum())
        keep = np.flatnonzero(keep)[:passing if max_out is None else max_out]
        uk, n, sq, sc, nv = uk[keep], n[keep], sq[keep], sc[keep], nv[keep]
        a, b = (1, 0) if self.mistake == "xy_key" else (0, 1)
        idx = np.stack([(uk >> 42) - AXIS, ((uk >> 21) & (2 * AXIS - 1)) - AXIS, (uk & (2 * AXIS - 1)) - AXIS], 1)[:, [a, b, 2]]
        pts = ((idx.astype(np.float64) + (sq.astype(np.float64) / n.astype(np.float64)[:, None]) * 2.0 ** -20) * self.voxel).astype(np.float32)
        return dict(points=pts, n=np.minimum(n, 2 ** 31 - 1).astype(np.int32), conf=(sc.astype(np.float64) * 2.0 ** -CONF_BITS).astype(np.float32),
                    n_views=nv, key=uk, count=len(uk), n_passing=passing, n_cut_off=passing - len(uk), n_occupied=len(np.unique(key)))


# ---------------------------------------------------------------------------------------------------------------- inputs
def depth_case(mask, seed=0, bad_values=True):
    """the GPU test's 13 x 17 inputs -> (invdepth, plane, confidence): inverse depths in (0.2, 1.4), a block of equal values,
    and (``bad_values``) a NaN, a zero and a negative value at detected pixels"""
    assert mask in MASKS
    rng = np.random.default_rng(100 + seed)
    inv = rng.uniform(0.2, 1.4, (H, W)).astype(np.float32)
    inv[2:6, 3:8] = np.float32(0.75)                       # equal values inside a window
    inv[8:, :4] = np.round(inv[8:, :4] * 4) / 4            # and ties between a few levels
    vv, uu = np.mgrid[0:H, 0:W]
    det = dict(empty=np.zeros((H, W), bool), full=np.ones((H, W), bool), one=(vv == 0) & (uu == W - 1),
               checker=(vv + uu) % 2 == 0, random=rng.uniform(size=(H, W)) < 0.45)[mask]
    if bad_values and mask in ("full", "checker", "random"):
        for (v, u), x in (((4, 4), np.nan), ((6, 10), 0.0), ((10, 12), -0.5), ((12, 16), np.inf)):
            inv[v, u] = x
    plane = np.where(det, rng.integers(0, 16, (H, W)), -1).astype(np.int32)
    conf = rng.uniform(1.0, 9.0, (H, W)).astype(np.float32)
    return inv, plane, conf


def map_points(n, seed=0, voxel=0.25, spread=3.0):
    """the GPU test's clouds: ``n`` points around the origin on both sides of every axis, confidences in (0, 4); the first
    few sit exactly on voxel boundaries and at voxel centres"""
    rng = np.random.default_rng(200 + seed)
    p = rng.uniform(-spread, spread, (n, 3)).astype(np.float32)
    special = np.array([[0, 0, 0], [voxel, -voxel, 2 * voxel], [-0.5 * voxel, 0.5 * voxel, -1.5 * voxel], [-1e-30, 1e-30, -voxel]], np.float32)
    p[:min(n, 4)] = special[:min(n, 4)]
    return p, rng.uniform(0.0, 4.0, n).astype(np.float32)
