"""Numpy restatement of the event map's renderer (include/ramp_hip.h ``ramp_point_map_render``) -- TEST INFRASTRUCTURE ONLY.

(a) a TABLE is a dict of per-slot arrays ``key`` (-1: empty), ``n``, ``sq`` [S,3], ``sc`` (int64) and ``views`` (uint64):
    ``table_from_ref`` builds one from a ``pointmapref.PointMapRef`` (slots in any order), ``table_from_buffer`` reads the
    device's own buffer.  ``mean_points``: the export's mean point, the float64 formula rounded to float32 (exact).
(b) ``project``: the header's statements in float32 (its own rounding, statement for statement: numpy rounds every operation
    and fuses nothing) or float64 (the reference).  ``footprint_radius``: the float64 rule.  ``zbuffer``: the exact discrete
    part -- largest bits of d', lowest key among equal bits.  ``render``: the whole call.  ``from_records``: the discrete
    part rebuilt from a call's OWN records, which is what the GPU is held to bit for bit.
(c) the ``mistake`` keywords break the restatement on purpose (tests/test_renderref_cpu.py: each has to be rejected by the
    inputs the GPU test uses, which are built here: ``cloud_case``, ``CASES``).
"""
import numpy as np

import pointmapref as pm
import poseref

MIN_Z = np.float32(0.2)                       # RAMP_WARP_MIN_Z
H, W = pm.H, pm.W                             # 13 x 17
K = pm.K
CAM = pm.CAM
VOXEL = 0.25
MISTAKES = ("w2c", "fxfy", "trunc", "half_up", "min_depth", "high_key", "unclipped", "ceil_rho", "view_nowrap", "fill_over")
ABSENT, FILTERED, REJECTED, OUTSIDE, RENDERED = range(5)


# ------------------------------------------------------------------------------------------------------------- tables
def table_from_ref(ref, capacity=None, order=None):
    """the accumulators of a PointMapRef, one slot per voxel in ``order`` (a permutation; None: ascending key), padded with
    empty slots up to ``capacity``"""
    key, q, c, bit = (np.concatenate(v) for v in (ref.key, ref.q, ref.c, ref.bit))
    uk, inv = np.unique(key, return_inverse=True)
    n, sq, sc, views = np.zeros(len(uk), np.int64), np.zeros((len(uk), 3), np.int64), np.zeros(len(uk), np.int64), np.zeros(len(uk), np.uint64)
    np.add.at(n, inv, 1); np.add.at(sq, inv, q); np.add.at(sc, inv, c); np.bitwise_or.at(views, inv, bit)
    if order is not None:
        uk, n, sq, sc, views = uk[order], n[order], sq[order], sc[order], views[order]
    pad = 0 if capacity is None else capacity - len(uk)
    assert pad >= 0
    return dict(key=np.r_[uk, np.full(pad, -1, np.int64)], n=np.r_[n, np.zeros(pad, np.int64)], sq=np.r_[sq, np.zeros((pad, 3), np.int64)],
                sc=np.r_[sc, np.zeros(pad, np.int64)], views=np.r_[views, np.zeros(pad, np.uint64)])


def table_from_buffer(raw, capacity):
    """the device's buffer (uint8, ramp_point_map_bytes(capacity) of them): a 64-byte header, then 8 words per slot"""
    words = np.ascontiguousarray(raw).view(np.int64)[8:8 + 8 * capacity].reshape(capacity, 8)
    return dict(key=words[:, 0].copy(), n=words[:, 1].copy(), sq=words[:, 2:5].copy(), sc=words[:, 5].copy(),
                views=words[:, 6].copy().view(np.uint64))


def popcount(views):
    return np.array([bin(int(v)).count("1") for v in views], np.int64)


def mean_points(tab, voxel):
    """float32((double(i_a) + (double(sq_a) / double(n)) * 2^-20) * voxel) per slot (an empty slot: zeros, never read)"""
    k = np.where(tab["key"] < 0, 0, tab["key"])
    idx = np.stack([(k >> 42) - pm.AXIS, ((k >> 21) & (2 * pm.AXIS - 1)) - pm.AXIS, (k & (2 * pm.AXIS - 1)) - pm.AXIS], 1)
    n = np.maximum(tab["n"], 1).astype(np.float64)[:, None]
    return ((idx.astype(np.float64) + (tab["sq"].astype(np.float64) / n) * 2.0 ** -20) * np.float64(voxel)).astype(np.float32)


# --------------------------------------------------------------------------------------------------------- continuous
def bad_camera(cam, Kc):
    cam, Kc = np.asarray(cam, np.float32), np.asarray(Kc, np.float32)
    return not (np.isfinite(cam).all() and np.isfinite(Kc).all() and Kc[0] != 0 and Kc[1] != 0)


def project(points, cam, Kc, dtype=np.float32, mistake=None):
    """-> (u, v, d', Xc) in ``dtype`` from the float32 words of the points, the pose and the intrinsics"""
    cam, k = np.asarray(cam, np.float32).astype(dtype), np.asarray(Kc, np.float32).astype(dtype)
    if mistake == "fxfy":
        k = k[[1, 0, 2, 3]]
    X = np.asarray(points, np.float32).astype(dtype).reshape(-1, 3)
    with np.errstate(all="ignore"):
        if mistake == "w2c":                                 # the pose taken as world-to-camera
            Xc = poseref.qrot(cam[3:], X) + cam[:3]
        else:
            Xc = poseref.qrot(cam[3:] * np.array([-1, -1, -1, 1], dtype), X - cam[:3])
        d = dtype(1.0) / Xc[:, 2]
        u, v = k[0] * (Xc[:, 0] * d) + k[2], k[1] * (Xc[:, 1] * d) + k[3]
    return u.astype(dtype), v.astype(dtype), d.astype(dtype), Xc.astype(dtype)


def rejected(u, v, d, Xc):
    with np.errstate(all="ignore"):
        return ~(Xc[:, 2] > Xc.dtype.type(MIN_Z)) | ~np.isfinite(Xc).all(1) | ~np.isfinite(u) | ~np.isfinite(v)


def footprint_rho(d, voxel, Kc):
    """rho = ((0.5 * voxel) * double(max(|fx|, |fy|))) * double(d'), float64"""
    k = np.asarray(Kc, np.float32)
    with np.errstate(all="ignore"):
        return ((0.5 * np.float64(voxel)) * np.float64(max(abs(k[0]), abs(k[1])))) * np.asarray(d).astype(np.float64)


def footprint_radius(d, voxel, Kc, radius, footprint=True, mistake=None):
    """r_p per slot: ``radius``, or min(radius, max(0, ceil(rho - 0.5)))"""
    d = np.asarray(d)
    if not footprint:
        return np.full(d.shape, radius, np.int64)
    rho = footprint_rho(d, voxel, Kc)
    with np.errstate(all="ignore"):
        e = np.ceil(rho) if mistake == "ceil_rho" else np.ceil(rho - 0.5)
    return np.where(~(e < radius), radius, np.where(e > 0, e, 0)).astype(np.int64)


def centre(u, mistake=None):
    u = np.asarray(u, np.float32)
    with np.errstate(all="ignore"):
        if mistake == "trunc":
            return np.trunc(u)
        if mistake == "half_up":
            return np.floor(u + np.float32(0.5))
        return np.rint(u)                                     # half to even, as rintf


def inside(px, py, r, h, w):
    """the square has a pixel inside the image -- in float64, before any integer"""
    px, py, r = px.astype(np.float64), py.astype(np.float64), r.astype(np.float64)
    return (px + r >= 0) & (px - r <= w - 1) & (py + r >= 0) & (py - r <= h - 1)


# ----------------------------------------------------------------------------------------------------------- discrete
def zbuffer(px, py, d, r, key, rendered, h, w, mistake=None):
    """exact -> (bits uint32 [h,w], 0: no winner; key int64 [h,w], -1: no winner).  Per pixel the largest bits of d' among the
    covering slots, among equal bits the lowest key"""
    bits_out, key_out = np.zeros(h * w, np.uint32), np.full(h * w, -1, np.int64)
    at = np.flatnonzero(rendered)
    if not len(at):
        return bits_out.reshape(h, w), key_out.reshape(h, w)
    x0, y0, rr, kk = px[at].astype(np.int64), py[at].astype(np.int64), r[at], key[at]
    bb = np.ascontiguousarray(d[at], np.float32).view(np.uint32).astype(np.int64)
    R = int(rr.max())
    pix, bits, keys = [], [], []
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            m = rr >= max(abs(dx), abs(dy))
            x, y = x0 + dx, y0 + dy
            if mistake == "unclipped":                        # the square wraps around instead of ending at the border
                x, y = x % w, y % h
            m = m & (x >= 0) & (x < w) & (y >= 0) & (y < h)
            pix.append((y * w + x)[m]); bits.append(bb[m]); keys.append(kk[m])
    pix, bits, keys = np.concatenate(pix), np.concatenate(bits), np.concatenate(keys)
    order = np.lexsort((-keys if mistake == "high_key" else keys, bits if mistake == "min_depth" else -bits, pix))
    pix, bits, keys = pix[order], bits[order], keys[order]
    first = np.r_[True, pix[1:] != pix[:-1]]
    bits_out[pix[first]], key_out[pix[first]] = bits[first].astype(np.uint32), keys[first]
    return bits_out.reshape(h, w), key_out.reshape(h, w)


def _image(tab, bits, keyim, kind, fill, h, w, records, mistake=None):
    """the outputs from the winners: invdepth, key, n, conf, status"""
    won = keyim >= 0
    slot_of = {int(k): i for i, k in enumerate(tab["key"]) if k >= 0}
    slot = np.array([slot_of[int(k)] if k >= 0 else 0 for k in keyim.reshape(-1)], np.int64).reshape(h, w)
    none = np.float32(np.nan) if fill is None else np.float32(fill)
    inv = np.where(won, bits.view(np.float32), none).astype(np.float32)
    if mistake == "fill_over" and fill is not None:
        inv = np.full((h, w), none, np.float32)
    n = np.where(won, np.minimum(tab["n"], 2 ** 31 - 1)[slot], 0).astype(np.int32)
    conf = np.where(won, (tab["sc"].astype(np.float64) * 2.0 ** -pm.CONF_BITS).astype(np.float32)[slot], np.float32(0)).astype(np.float32)
    status = np.array([0, (kind != ABSENT).sum(), (kind == FILTERED).sum(), (kind == REJECTED).sum(), (kind == OUTSIDE).sum(),
                       (kind == RENDERED).sum(), won.sum(), 0], np.int32)
    return dict(invdepth=inv, key=np.where(won, keyim, -1).astype(np.int64), n=n, conf=conf, status=status, records=records, kind=kind)


def _failed(tab, h, w):
    S = len(tab["key"])
    nan = np.full((h, w), np.nan, np.float32)
    return dict(invdepth=nan, key=np.full((h, w), -1, np.int64), n=np.zeros((h, w), np.int32), conf=nan.copy(),
                status=np.array([1, 0, 0, 0, 0, 0, 0, 0], np.int32), records=np.full((S, 4), np.nan, np.float32),
                kind=np.full(S, ABSENT))


def slot_kinds(tab, min_points, min_views):
    """ABSENT, FILTERED or (for now) RENDERED per slot: the export's conditions"""
    occupied = tab["key"] != -1
    passing = occupied & (tab["n"] >= min_points) & (popcount(tab["views"]) >= min_views)
    return np.where(passing, RENDERED, np.where(occupied, FILTERED, ABSENT))


def render(tab, voxel, cam, Kc, h, w, radius=2, footprint=True, min_points=1, min_views=1, fill=None, mistake=None, dtype=np.float32):
    """the whole call -> dict(invdepth, key, n, conf, status, records [S,4], kind [S]); ``dtype=np.float64``: the continuous
    part in float64 (records then float64: the reference of the GPU's records)"""
    assert mistake is None or mistake in MISTAKES
    if bad_camera(cam, Kc):
        return _failed(tab, h, w)
    kind = slot_kinds(tab, min_points, min_views)
    u, v, d, Xc = project(mean_points(tab, voxel), cam, Kc, dtype, mistake)
    kind = np.where((kind == RENDERED) & rejected(u, v, d, Xc), REJECTED, kind)
    live = kind == RENDERED
    r = footprint_radius(np.where(live, d, 1).astype(np.float32) if dtype == np.float32 else np.where(live, d, 1), voxel,
                         np.asarray(Kc, np.float32)[[1, 0, 2, 3]] if mistake == "fxfy" else Kc, radius, footprint, mistake)
    px, py = centre(np.where(live, u, 0), mistake), centre(np.where(live, v, 0), mistake)
    kind = np.where(live & ~inside(px, py, r, h, w), OUTSIDE, kind)
    row = (kind == RENDERED) | (kind == OUTSIDE)
    records = np.where(row[:, None], np.stack([u, v, d, r.astype(dtype)], 1), np.nan).astype(dtype)
    bits, keyim = zbuffer(px, py, d.astype(np.float32), r, tab["key"], kind == RENDERED, h, w, mistake)
    return _image(tab, bits, keyim, kind, fill, h, w, records, mistake)


def from_records(records, tab, h, w, min_points=1, min_views=1, fill=None):
    """The discrete part from a call's OWN records (float32 [S,4]: u, v, d', r_p; NaN rows: no record): centre pixels, the
    test against the image, the z-buffer, the winners' words and every status word.  A slot that passes the export's
    conditions and has no record was rejected."""
    records = np.asarray(records, np.float32)
    kind = slot_kinds(tab, min_points, min_views)
    row = ~np.isnan(records[:, 2])
    assert not (row & (kind != RENDERED)).any(), "a record for a slot that does not take part"
    kind = np.where((kind == RENDERED) & ~row, REJECTED, kind)
    live = kind == RENDERED
    u, v, d = (np.where(live, records[:, i], 0).astype(np.float32) for i in range(3))
    r = np.where(live, records[:, 3], 0).astype(np.int64)
    px, py = centre(u), centre(v)
    kind = np.where(live & ~inside(px, py, r, h, w), OUTSIDE, kind)
    bits, keyim = zbuffer(px, py, d, r, tab["key"], kind == RENDERED, h, w)
    return _image(tab, bits, keyim, kind, fill, h, w, records)


# -------------------------------------------------------------------------------------------------------------- inputs
RHO_MARGIN, PIXEL_MARGIN = 1e-3, 1e-2


def margins(tab, voxel, cam, Kc, radius=7, min_points=1, min_views=1):
    """the two conditions on a scene, over the slots that take part and are not rejected -> (the smallest distance of the
    float64 rho - 0.5 from an integer, among the slots whose r_p the radius does not cap; the smallest distance of u, v from a
    rounding switch k + 0.5)"""
    a, b = slot_margins(tab, voxel, cam, Kc, radius, min_points, min_views)
    return float(a.min()) if len(a) else np.inf, float(b.min()) if len(b) else np.inf


def slot_margins(tab, voxel, cam, Kc, radius=7, min_points=1, min_views=1):
    """``margins`` per slot (inf where a slot does not count)"""
    kind = slot_kinds(tab, min_points, min_views)
    u, v, d, Xc = project(mean_points(tab, voxel), cam, Kc, np.float64)
    live = (kind == RENDERED) & ~rejected(u, v, d, Xc)
    with np.errstate(all="ignore"):
        e = footprint_rho(d, voxel, Kc) - 0.5
        half = lambda a: np.abs(a - np.floor(a) - 0.5)
        a = np.where(live & (e < radius + 1), np.abs(e - np.rint(e)), np.inf)
        b = np.where(live, np.minimum(half(u), half(v)), np.inf)
    return a, b


def cloud_case(N, seed=0, cam=CAM, Kc=K, voxel=VOXEL, views=(3,)):
    """the GPU test's clouds: ``N`` voxels in front of the camera ``cam`` -- pixels over the
    image and a margin of 4 around it, depths 0.45 .. 12 (rho 4.4 .. 0.17 with fx = 16; 0.45 .. 4 for the small ones), a few behind the camera and a few below
    RAMP_WARP_MIN_Z -- one to three points per voxel, split over ``views``.  Voxels that miss a margin (``margins``) are
    left out HERE, so that no comparison has to leave anything out.  -> list of (points, conf, view) inserts"""
    rng = np.random.default_rng(300 + seed)
    M = N + 6 if N <= 2 else 3 * N
    uu, vv = rng.uniform(-4, W + 3, M), rng.uniform(-4, H + 3, M)
    z = rng.uniform(0.45, 4.0 if N <= 8 else 12.0, M)
    if N > 8:
        z[:4], z[4:8] = -1.5, rng.uniform(0.05, 0.19, 4)
    else:
        uu, vv = rng.uniform(2, W - 3, M), rng.uniform(2, H - 3, M)
    p = pm.lift(uu, vv, 1.0 / z, cam, Kc, np.float64).astype(np.float32)
    per = rng.integers(1, 4, M)
    pts = np.repeat(p, per, 0) + rng.uniform(-0.02, 0.02, (per.sum(), 3)).astype(np.float32)
    conf = rng.uniform(0.5, 4.0, len(pts)).astype(np.float32)
    ref = pm.PointMapRef(voxel)
    ref.insert(pts, conf)
    tab = table_from_ref(ref)
    f = pm.fixed(pts, conf, voxel)
    a, b = slot_margins(tab, voxel, cam, Kc)                  # voxel by voxel: a voxel left out takes all its points along
    keep_key = tab["key"][(a >= 2 * RHO_MARGIN) & (b >= 2 * PIXEL_MARGIN)]
    first = keep_key[np.isinf(b[np.isin(tab["key"], keep_key)])]        # the rejected voxels stay, the rest is drawn
    rest = np.setdiff1d(keep_key, first)
    keep_key = np.r_[first, rest[rng.permutation(len(rest))]][:N]
    sel = np.isin(f["key"], keep_key)
    pts, conf = pts[sel], conf[sel]
    cut = np.linspace(0, len(pts), len(views) + 1).astype(int)
    return [(pts[a:b], conf[a:b], view) for a, b, view in zip(cut[:-1], cut[1:], views)]


def table_of(inserts, voxel=VOXEL, capacity=None, order=None, mistake=None):
    ref = pm.PointMapRef(voxel, mistake if mistake == "view_nowrap" else None)
    for p, c, view in inserts:
        ref.insert(p, c, view)
    return table_from_ref(ref, capacity, order)


def tie_case(count, seed=0, cam=pm.IDENTITY, voxel=VOXEL):
    """``count`` voxels whose mean points project with EQUAL bits of d' onto one pixel of the identity camera: one point per
    voxel at the voxel's centre, all at the same z (voxel 0.25 and centres at odd multiples of 0.125 are exact in float32),
    inside a patch of the plane z = 64.125 that stays within a tenth of a pixel of (8, 6)"""
    side = int(np.ceil(np.sqrt(count)))
    i = np.arange(count)
    cells = np.stack([i % side - side // 2, i // side - side // 2, np.full(count, 256)], 1)
    return [(((cells + 0.5) * voxel).astype(np.float32), np.ones(count, np.float32), 1)]


TIE_K = np.array([0.05, 0.05, 8.0, 6.0], np.float32)          # 80 voxels of 0.25 at z = 64 span 0.016 pixels: one pixel


def view_case():
    """three voxels seen from views {0}, {63, 64} and {64}: 64 wraps onto 0, so popcounts 1, 2, 1 (without the wrap: 1, 1, 0)"""
    cells = np.array([[0, 0, 8], [4, 0, 8], [-4, 2, 8]], np.float64)
    p = ((cells + 0.5) * VOXEL).astype(np.float32)
    one = np.ones(1, np.float32)
    return [(p[0:1], one, 0), (p[1:2], one, 63), (p[1:3], np.ones(2, np.float32), 64)]


HALF_K = np.array([16.0, 16.0, 4.5, 6.5], np.float32)


def half_case():
    """one voxel whose mean point is ON the optical axis of the identity camera (a point at the voxel's corner x = y = 0): u = fx
    * (0 * d') + cx = cx and v = cy in every bit, so with HALF_K the point sits on two rounding switches, (4.5, 6.5) -> (4, 6)"""
    return [(np.float32([[0, 0, 2.1]]), np.ones(1, np.float32), 1)]


# the z-buffer cases of the GPU test: (radius, footprint); 7 is larger than half the image, and with footprint off a voxel at
# the image's centre covers all 13 rows
RADII = [(0, False), (1, False), (3, False), (7, False), (0, True), (1, True), (3, True), (7, True)]


def gpu_scenes(full=True):
    """every scene the GPU test renders -> (name, inserts, voxel, cam, intrinsics, keywords of ``render``); ``full=False``
    leaves out the radii sweep over the large cloud but for two of its cases"""
    for N in (0, 1, 2):
        yield "cloud %d" % N, (cloud_case(N, seed=N) if N else []), VOXEL, CAM, K, dict(radius=3, footprint=True)
    big = cloud_case(4099, seed=7, views=(3, 4))
    for radius, fp in (RADII if full else [(3, True), (7, False)]):
        yield "cloud 4099 r=%d fp=%d" % (radius, fp), big, VOXEL, CAM, K, dict(radius=radius, footprint=fp)
    yield "cloud 4099 min_points=2 min_views=2", big, VOXEL, CAM, K, dict(radius=2, footprint=True, min_points=2, min_views=2)
    for count in (1, 2, 4099):
        yield "tie %d" % count, tie_case(count), VOXEL, pm.IDENTITY, TIE_K, dict(radius=1, footprint=False)
    for mv in (1, 2, 3):
        yield "views min_views=%d" % mv, view_case(), VOXEL, pm.IDENTITY, K, dict(radius=1, footprint=False, min_views=mv)
    yield "half", half_case(), VOXEL, pm.IDENTITY, HALF_K, dict(radius=0, footprint=False)
    yield "fill", cloud_case(2, seed=2), VOXEL, CAM, K, dict(radius=1, footprint=True, fill=0.5)
