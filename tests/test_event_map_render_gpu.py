"""The event map's renderer on the GPU: ``ramp_point_map_render`` (csrc/maprender.hip) through the C entry point (every buffer
between canaries, tests/guarded.py), ``ops.PointMap.render`` and the tracker's ``event_map_depth`` / ``invdepth="event_map"``.

The table the renderer reads is read back from the device as it is (``renderref.table_from_buffer``), so every comparison is
per SLOT and nothing depends on how the hash placed the voxels.  The DISCRETE part -- centre pixels, clipping, the z-buffer
with its tie rule, the winners' words, every status word -- is held BIT FOR BIT to the emulator run on the call's own records
(``renderref.from_records``).  The CONTINUOUS part -- the records -- is held to float64 per slot by the bound rule of
test_geometry_f64_gpu.py, ``georef.bound(floor, env)`` with env the float32 restatement's own error against float64 and the
floor ``georef.PIXEL_FLOOR`` x the largest coordinate; ``r_p`` exactly (tests/test_renderref_cpu.py holds the scenes' float64
rho - 0.5 at least 1e-3 from an integer).  Images are 13 x 17, capacities 8 and 2^13.  Nothing here provokes a fault."""
import ctypes

import numpy as np
import pytest
import torch

import dsiref
import georef
import pointmapref as pm
import renderref as rr
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W, V = rr.H, rr.W, rr.VOXEL
P = lambda f: ctypes.c_void_p(f.address()) if isinstance(f, Flat) else (None if f is None else ctypes.c_void_p(f.data_ptr()))


def _stream():
    from rampvo_amd import _lib
    return _lib.stream()


class GMap:
    """a table on the device between canaries, filled through ramp_point_map_insert"""

    def __init__(self, inserts, capacity=1 << 13, voxel=V):
        from rampvo_amd import _lib
        self.L, self.cap, self.voxel = _lib.lib(), capacity, voxel
        self.buf = Flat(self.L.ramp_point_map_bytes(capacity), torch.uint8)
        assert self.L.ramp_point_map_clear(P(self.buf), capacity, _stream()) == 0
        status = torch.empty(8, dtype=torch.int32, device="cuda")
        for p, c, view in inserts:
            d_p, d_c = cu(np.asarray(p, np.float32).reshape(-1, 3)), None if c is None else cu(np.asarray(c, np.float32))
            assert self.L.ramp_point_map_insert(P(self.buf), capacity, P(d_p), P(d_c), len(d_p), None, voxel, view, P(status), _stream()) == 0
            torch.cuda.synchronize()
            assert status[4].item() == 0, "nothing is dropped"
        torch.cuda.synchronize()
        self.tab = rr.table_from_buffer(self.buf.t.cpu().numpy(), capacity)

    def render(self, cam=rr.CAM, Kc=rr.K, h=H, w=W, radius=2, footprint=True, min_points=1, min_views=1, fill=None, key=True, n=True,
               conf=True, records=True, expect=0, **over):
        """the C entry with every buffer between canaries -> numpy dict; ``fill``: None, or a number (uploaded as the device word)"""
        nbytes = self.L.ramp_point_map_render_ws_bytes(h, w)
        b = dict(invdepth=Flat((h, w), torch.float32), key=Flat((h, w), torch.int64), n=Flat((h, w), torch.int32), conf=Flat((h, w), torch.float32),
                 records=Flat((self.cap, 4), torch.float32), status=Flat(8, torch.int32), ws=Flat(nbytes, torch.uint8, rows=4))
        d_cam, d_K = cu(np.asarray(cam, np.float32)), cu(np.asarray(Kc, np.float32))
        d_fill = None if fill is None else cu(np.float32([fill]))
        torch.cuda.synchronize()
        before, table = {k: v.snapshot() for k, v in b.items()}, self.buf.snapshot()
        a = dict(p_map=P(self.buf), cap=self.cap, voxel=self.voxel, min_points=min_points, min_views=min_views, p_cam=P(d_cam), p_K=P(d_K),
                 H=h, W=w, radius=radius, footprint=1 if footprint else 0, p_fill=P(d_fill), p_invdepth=P(b["invdepth"]),
                 p_key=P(b["key"]) if key else None, p_n=P(b["n"]) if n else None, p_conf=P(b["conf"]) if conf else None,
                 p_records=P(b["records"]) if records else None, p_ws=P(b["ws"]), nbytes=nbytes, p_status=P(b["status"]))
        assert set(over) <= set(a), over
        a.update(over)
        rc = self.L.ramp_point_map_render(*a.values(), _stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, over)
        assert all(v.intact() for v in b.values()) and self.buf.unchanged(table), "the render does not write the map"
        if rc:
            assert all(v.unchanged(before[k]) for k, v in b.items()), "a refused call touches nothing"
            return None
        for k, used in (("key", key), ("n", n), ("conf", conf), ("records", records)):
            assert used or b[k].unchanged(before[k]), "an output that was not asked for is not written: " + k
        return {k: b[k].t.cpu().numpy() for k in ("invdepth", "key", "n", "conf", "records", "status")}


def _same_image(out, ref, name, optional=("key", "n", "conf")):
    assert out["status"].tolist() == ref["status"].tolist(), (name, out["status"], ref["status"])
    assert georef.same_bits(out["invdepth"], ref["invdepth"]), name
    for k in optional:
        assert (georef.same_bits(out[k], ref[k]) if k == "conf" else np.array_equal(out[k], ref[k])), (name, k)
    st = out["status"]
    assert st[2] + st[3] + st[4] + st[5] == st[1], name
    if "key" in optional:
        assert st[6] == (out["key"] >= 0).sum(), name


def _check(g, out, name, tab=None, cam=rr.CAM, Kc=rr.K, h=H, w=W, radius=2, footprint=True, min_points=1, min_views=1, fill=None):
    """the discrete part bit for bit against the emulator on the call's own records; the records against float64"""
    _same_image(out, rr.from_records(out["records"], g.tab, h, w, min_points, min_views, fill), name)
    kw = dict(radius=radius, footprint=footprint, min_points=min_points, min_views=min_views, fill=fill)
    r32, r64 = rr.render(g.tab, g.voxel, cam, Kc, h, w, **kw), rr.render(g.tab, g.voxel, cam, Kc, h, w, dtype=np.float64, **kw)
    row = ~np.isnan(out["records"][:, 2])
    assert np.array_equal(row, ~np.isnan(r64["records"][:, 2])), name + ": the same slots are rendered or outside"
    assert np.array_equal(out["records"][row, 3], r64["records"][row, 3]), name + ": r_p exact"
    if not row.any():
        return 0.0
    worst = 0.0
    for cols, what in (((0, 1), "uv"), ((2,), "d'")):
        got, r_32, r_64 = (a["records"][row][:, cols] for a in (out, r32, r64))
        err, env = georef.max_err(got, r_64), georef.max_err(r_32, r_64)
        floor = georef.PIXEL_FLOOR * max(1.0, float(np.abs(r_64).max()))
        print("render %s %s: err %.3g env %.3g bound %.3g err/bound %.3g" % (name, what, err, env, georef.bound(floor, env), err / georef.bound(floor, env)))
        if tab is not None:
            tab.add("%s %s" % (name, what), err, env, floor)
        assert err <= georef.bound(floor, env), (name, what, err, env, floor)
        worst = max(worst, err / georef.bound(floor, env))
    return worst


_maps = {}


def _scene_map(key, inserts, capacity=1 << 13):
    """one table per scene and session, shared and never written behind its inserts"""
    if key not in _maps:
        _maps[key] = GMap(inserts, capacity)
    return _maps[key]


SCENES = list(rr.gpu_scenes())


# ------------------------------------------------------------------------------------------------ 1. records, counts, z-buffer
@pytest.mark.parametrize("i", range(len(SCENES)), ids=[s[0] for s in SCENES])
def test_render_bits_and_records(i):
    name, inserts, voxel, cam, Kc, kw = SCENES[i]
    g = _scene_map(name.split(" r=")[0] if name.startswith("cloud 4099") else name, inserts)
    out = g.render(cam=cam, Kc=Kc, **kw)
    tab = georef.Table("render: records against float64")
    worst = _check(g, out, name, tab, cam=cam, Kc=Kc, **kw)
    print("render %s: status %s largest err / bound %.3f" % (name, out["status"].tolist(), worst))
    occupied = int((g.tab["key"] >= 0).sum())
    assert out["status"][1] == occupied and out["status"][0] == 0
    if name == "cloud 0":
        assert out["status"].tolist() == [0] * 8 and np.isnan(out["invdepth"]).all() and (out["key"] == -1).all()
    if name.startswith("tie "):
        assert out["status"][5] == occupied and out["status"][6] == 9 and (out["key"][out["key"] >= 0] == g.tab["key"][g.tab["key"] >= 0].min()).all()
    if name.startswith("views"):
        assert out["status"][2] == {1: 0, 2: 2, 3: 3}[kw["min_views"]]
    if name == "half":
        assert np.argwhere(out["key"] >= 0).tolist() == [[6, 4]] and out["records"][~np.isnan(out["records"][:, 0])][0, :2].tolist() == [4.5, 6.5]
    again = g.render(cam=cam, Kc=Kc, **kw)                     # a call repeats its bits
    for k in ("invdepth", "key", "n", "conf", "records", "status"):
        assert georef.same_bits(out[k].reshape(-1).view(np.int32), again[k].reshape(-1).view(np.int32)), k


def test_a_table_that_is_exactly_full_and_keys_that_share_one_hash_slot():
    cells = [(i - 4, i % 3 - 1, 8 + i) for i in range(8)]
    pts = ((np.asarray(cells, np.float64) + rng_unit(len(cells), 1)) * V).astype(np.float32)
    g = GMap([(pts, None, 0)], capacity=8)
    assert (g.tab["key"] >= 0).all()
    out = g.render(cam=pm.IDENTITY, radius=3)
    _check(g, out, "capacity 8", cam=pm.IDENTITY, radius=3)
    assert out["status"][1] == 8
    cap, cells, i = 1 << 13, [], 0
    while len(cells) < 40:
        if pm.slot(pm.make_key(i % 9 - 4, i // 9 % 7 - 3, 8 + i // 63), cap) == 5:
            cells.append((i % 9 - 4, i // 9 % 7 - 3, 8 + i // 63))
        i += 1
    pts = ((np.asarray(cells, np.float64) + rng_unit(40, 2)) * V).astype(np.float32)
    g = GMap([(pts, None, 0)], capacity=cap)
    assert (g.tab["key"][5:45] >= 0).all() and (g.tab["key"] >= 0).sum() == 40, "one probe chain of 40"
    out = g.render(cam=pm.IDENTITY, radius=2)
    _check(g, out, "one hash slot", cam=pm.IDENTITY, radius=2)
    assert out["status"][1] == 40 and out["status"][5] > 0


def rng_unit(n, seed):
    """positions inside a voxel, away from its faces"""
    return np.random.default_rng(seed).uniform(0.2, 0.8, (n, 3))


def test_one_insert_two_inserts_and_a_shuffled_insert_give_the_same_image():
    (p, c, view), = rr.cloud_case(4099, seed=7, views=(3,))
    perm = np.random.default_rng(12).permutation(len(p))
    half = len(p) // 3
    outs = [GMap(ins).render(radius=3, records=False) for ins in ([(p, c, 3)], [(p[:half], c[:half], 3), (p[half:], c[half:], 3)],
                                                                  [(p[perm], c[perm], 3)])]
    for o in outs[1:]:
        for k in ("invdepth", "key", "n", "conf", "status"):
            assert georef.same_bits(outs[0][k].reshape(-1).view(np.int32), o[k].reshape(-1).view(np.int32)), k
    assert outs[0]["status"][6] > 100


# ------------------------------------------------------------------------------------------------ 2. filtering and fill
def test_min_points_min_views_and_fill():
    name, inserts, voxel, cam, Kc, _ = SCENES[[s[0] for s in SCENES].index("cloud 4099 min_points=2 min_views=2")]
    g = _scene_map("cloud 4099", inserts)
    for kw in (dict(min_points=2), dict(min_views=2), dict(min_points=3, min_views=2), dict(min_points=0, min_views=0), dict(min_points=10 ** 6)):
        out = g.render(radius=2, **kw)
        _check(g, out, "filter %s" % kw, radius=2, **kw)
        assert (kw.get("min_points", 1) < 10 ** 6) == (out["status"][5] > 0)
    inserts = SCENES[2][1]                                     # two voxels: most pixels stay empty
    g = _scene_map("cloud 2", inserts)
    none, number = g.render(radius=0), g.render(radius=0, fill=0.5)
    _check(g, number, "fill 0.5", radius=0, fill=0.5)
    won = none["key"] >= 0
    assert 0 < won.sum() < H * W and np.isnan(none["invdepth"][~won]).all() and (number["invdepth"][~won] == 0.5).all()
    assert georef.same_bits(none["invdepth"][won], number["invdepth"][won]) and (none["n"][~won] == 0).all() and (none["conf"][~won] == 0).all()
    # through ops: None, a number, a device word
    from rampvo_amd import ops
    m = ops.PointMap(V, capacity=1 << 13)
    for p, c, view in inserts:
        m.insert(cu(p), cu(c), view=view)
    for fill in (None, 0.5, cu(np.float32([0.5]))):
        r = m.render(cu(rr.CAM), rr.K, H, W, radius=0, fill=fill)
        assert georef.same_bits(r["invdepth"].cpu().numpy(), (none if fill is None else number)["invdepth"])
        assert np.array_equal(r["key"].cpu().numpy(), none["key"]) and sorted(r) == ["conf", "invdepth", "key", "n", "status"]
    assert ops.point_map_render_status(r["status"]) == dict(zip(("bad_camera", "n_occupied", "n_filtered", "n_rejected", "n_outside",
                                                                 "n_rendered", "n_pixels"), [False] + none["status"][1:7].tolist()))
    empty = ops.PointMap(V, capacity=8)
    r = empty.render(cu(rr.CAM), rr.K, H, W, fill=0.25, want_records=True)
    assert (r["invdepth"] == 0.25).all() and r["status"].cpu().tolist() == [0] * 8 and (r["key"] == -1).all() and torch.isnan(r["records"]).all()


# ------------------------------------------------------------------------------------------------ 3. failures and conventions
def test_a_camera_that_is_not_finite_renders_nothing_plausible():
    g = _scene_map("cloud 2", SCENES[2][1])
    for word in range(11):
        for bad in (np.nan, np.inf):
            cam, Kc = rr.CAM.copy(), rr.K.copy()
            (cam if word < 7 else Kc)[word if word < 7 else word - 7] = bad
            out = g.render(cam=cam, Kc=Kc, fill=0.5)
            assert out["status"].tolist() == [1] + [0] * 7, word
            assert np.isnan(out["invdepth"]).all() and np.isnan(out["conf"]).all() and (out["key"] == -1).all() and (out["n"] == 0).all()
            assert np.isnan(out["records"]).all()
    for i in (0, 1):
        Kc = rr.K.copy()
        Kc[i] = 0
        assert g.render(Kc=Kc)["status"].tolist() == [1] + [0] * 7


def test_refusals_touch_nothing():
    from rampvo_amd import _lib
    g = _scene_map("cloud 2", SCENES[2][1])
    for over in (dict(H=0), dict(W=-1), dict(radius=-1), dict(radius=8), dict(cap=12), dict(cap=4), dict(cap=1 << 31), dict(voxel=0.0),
                 dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(min_points=-1), dict(min_views=-1), dict(p_map=None),
                 dict(p_cam=None), dict(p_K=None), dict(p_invdepth=None), dict(p_ws=None), dict(p_status=None),
                 dict(p_map=ctypes.c_void_p(g.buf.address() + 8))):
        g.render(expect=_lib.RAMP_EINVAL, **over)
    g.render(expect=_lib.RAMP_EUNSUPPORTED, H=1 << 16, W=1 << 15)
    g.render(expect=_lib.RAMP_EWORKSPACE, nbytes=_lib.lib().ramp_point_map_render_ws_bytes(H, W) - 1)


def test_every_optional_output_null_and_a_side_stream():
    from rampvo_amd import ops
    name, inserts = SCENES[3][0], SCENES[3][1]
    g = _scene_map("cloud 4099", inserts)
    full = g.render(radius=3)
    for leave in ("key", "n", "conf", "records"):
        out = g.render(radius=3, **{leave: False})
        _same_image(out, full, "without " + leave, optional=[k for k in ("key", "n", "conf") if k != leave])
    out = g.render(radius=3, key=False, n=False, conf=False, records=False)
    _same_image(out, full, "invdepth alone", optional=())
    side = torch.cuda.Stream()
    d = [(cu(p), cu(c), view) for p, c, view in inserts]
    cam = cu(rr.CAM)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        m = ops.PointMap(V, capacity=1 << 13)
        for p, c, view in d:
            m.insert(p, c, view=view)
        r = m.render(cam, rr.K, H, W, radius=3, want_records=True)
    side.synchronize()
    for k in ("invdepth", "key", "n", "conf", "status"):
        assert georef.same_bits(r[k].cpu().numpy().reshape(-1).view(np.int32), full[k].reshape(-1).view(np.int32)), k
    assert r["records"].shape == (1 << 13, 4)


# ------------------------------------------------------------------------------------------------ 4. consumers
def test_the_render_feeds_the_event_warp():
    """ops.event_warp samples the rendered map at the event's rounded pixel: with two knots at one pose the warp is the
    identity whatever the depth, and with a moving camera the events' shift follows the rendered depth"""
    from rampvo_amd import ops
    inserts = SCENES[3][1]
    m = ops.PointMap(V, capacity=1 << 13)
    for p, c, view in inserts:
        m.insert(cu(p), cu(c), view=view)
    r = m.render(cu(rr.CAM), rr.K, H, W, radius=3, fill=0.5)
    inv = r["invdepth"].cpu().numpy()
    vv, uu = np.mgrid[0:H, 0:W]
    x, y = uu.reshape(-1).astype(np.float32), vv.reshape(-1).astype(np.float32)
    t, p = np.full(H * W, 1.0), np.ones(H * W, np.int8)
    knots = np.array([[0, 0, 0, 0, 0, 0, 1], [0.1, 0, 0, 0, 0, 0, 1]], np.float32)
    out = ops.event_warp(cu(x), cu(y), cu(t), cu(p), cu(knots), cu(np.array([0.0, 1.0])), 0.0, cu(rr.K), r["invdepth"], H, W, want_xy=True)
    xy = out["xy"].cpu().numpy()
    # X' = (x - cx) / fx + 0.1 d, Z' = 1: the shift is fx * 0.1 * d of the pixel's own rendered depth
    shift = xy[:, 0] - x
    want = rr.K[0] * np.float32(0.1) * inv.reshape(-1)
    assert np.isfinite(xy).all() and np.abs(shift - want).max() < 1e-4, np.abs(shift - want).max()
    assert len(np.unique(inv)) > 10


def test_two_plane_scene_end_to_end():
    """dsiref.two_plane_scene through ops.event_dsi, ops.depth_points, ops.PointMap and its render, at the reference pose and at
    a second pose: every rendered pixel's key is the restatement's (the float32 statements on the device's own table), its
    depth lies within the bound rule of the float64 restatement, and the distance of the rendered depths from their plane --
    seen from the reference pose, where a plane of the sweep is z = 1 / d_k -- is the figure the restatement gives"""
    from rampvo_amd import ops
    s = dsiref.TWO_PLANE
    x, y, t, knots, times = dsiref.two_plane_scene()
    r = ops.event_dsi(cu(x), cu(y), cu(t), cu(knots), cu(times), s["t_ref"], cu(s["K"]), s["H"], s["W"], planes=s["D"], range=s["rng"],
                      min_votes=s["min_votes"])
    pts = ops.depth_points(r["invdepth"], cu(pm.IDENTITY), s["K"], plane=r["plane"], confidence=r["confidence"], median_radius=2, min_support=3)
    voxel, cap = 0.2, 1 << 12
    m = ops.PointMap(voxel, capacity=cap)
    m.insert(pts["points"], pts["conf"], count=pts["count"], view=0)
    tab = rr.table_from_buffer(m.buf.cpu().numpy(), cap)
    d, _ = dsiref.plane_depths(s["rng"], s["D"])
    za, zb = (1.0 / float(d[p]) for p in s["planes"])
    for name, cam in (("reference pose", pm.IDENTITY), ("second pose", np.float32([0.15, -0.05, 0.1, 0, 0.02, 0, 1]))):
        out = kit.host(m.render(cu(cam), s["K"], s["H"], s["W"], radius=2, want_records=True))
        kw = dict(radius=2, footprint=True)
        r32 = rr.render(tab, voxel, cam, s["K"], s["H"], s["W"], **kw)
        r64 = rr.render(tab, voxel, cam, s["K"], s["H"], s["W"], dtype=np.float64, **kw)
        _same_image(out, rr.from_records(out["records"], tab, s["H"], s["W"]), name)
        won = out["key"] >= 0
        assert won.sum() >= 25 and np.array_equal(out["key"], r32["key"]), name
        slot = {int(k): i for i, k in enumerate(tab["key"]) if k >= 0}
        d64 = np.array([r64["records"][slot[int(k)], 2] for k in out["key"][won]])
        d32 = np.array([r32["records"][slot[int(k)], 2] for k in out["key"][won]], np.float32)
        err, env = georef.max_err(out["invdepth"][won], d64), georef.max_err(d32, d64)
        floor = georef.PIXEL_FLOOR * max(1.0, float(np.abs(d64).max()))
        print("two planes, %s: %d pixels, depth err %.3g env %.3g bound %.3g" % (name, won.sum(), err, env, georef.bound(floor, env)))
        assert err <= georef.bound(floor, env)
        if name == "reference pose":
            off = lambda im, w: np.minimum(np.abs(1.0 / im[w].astype(np.float64) - za), np.abs(1.0 / im[w].astype(np.float64) - zb))
            got, want = off(out["invdepth"], won), off(r32["invdepth"], r32["key"] >= 0)
            print("two planes: largest distance of a rendered depth from its plane %.4f (restatement %.4f, voxel %.2f)" % (got.max(), want.max(), voxel))
            assert got.max() == want.max() and got.max() <= voxel


def _render_ask(slam, f, frame):
    """The small tracker's median inverse depth is about 4.3: a sweep around it puts the three stacked pixels at a depth of 0.13,
    below RAMP_WARP_MIN_Z, where the renderer rejects them as the event warp would (measured: 1 occupied, 1 rejected).  The
    sweep is therefore given the range (0.1, 1.5) -- depths of 0.67 and more -- and the voxel, 0.5, holds the three points (at a
    depth near 10.7) together, so that the default ``min_points = 2`` of ``invdepth="event_map"`` keeps them"""
    x, y, t, p = (v.clone() for v in kit.query_events(f))
    x[:400], y[:400], t[:400] = 100.0, 80.0, kit.tstamp(f)
    x[400:800], y[400:800], t[400:800] = 101.0, 80.0, kit.tstamp(f)
    x[800:1200], y[800:1200], t[800:1200] = 100.0, 81.0, kit.tstamp(f)
    slam.event_map(voxel=0.5, capacity=1 << 16)
    slam.event_map_insert(x, y, t, planes=24, range=(0.1, 1.5), min_votes=2.0, median_radius=1, min_support=2, as_tensor=True)
    res = {"tensor": kit.host(slam.event_map_depth(min_points=1, as_tensor=True))}
    res["resident_mid"] = kit.resident(slam)
    res["numpy"] = slam.event_map_depth(min_points=1, t_ref=kit.tstamp(f - 1), fill="median")
    by_default = slam.event_map_depth(fill="median", as_tensor=True)
    m, res["default_status"] = by_default["invdepth"], kit.host(by_default["status"])
    res["by_name"] = slam.compensate_events(x, y, t, p, invdepth="event_map", want_xy=True)
    res["by_map"] = slam.compensate_events(x, y, t, p, invdepth=m, want_xy=True)
    res["contrast"] = slam.event_contrast(x, y, t, p, invdepth="event_map")["variance"]
    res["contrast_map"] = slam.event_contrast(x, y, t, p, invdepth=m)["variance"]
    return res


def _check_render_answer(a):
    tz = a["tensor"]
    assert sorted(tz) == ["conf", "invdepth", "key", "n", "pose_status", "status"] and tz["invdepth"].shape == (240, 320)
    won = tz["key"] >= 0
    assert tz["status"][0] == 0 and tz["status"][6] == won.sum() > 0 and np.isnan(tz["invdepth"][~won]).all() and (tz["invdepth"][won] > 0).all()
    nb = a["numpy"]
    assert nb["status"][0] == 0 and np.isfinite(nb["invdepth"]).all() and nb["invdepth"].shape == (240, 320)
    print("tracker render: status %s, with the defaults %s" % (tz["status"].tolist(), a["default_status"].tolist()))
    assert a["default_status"][6] > 0, "the map the comparison below samples is not the median alone"
    kit.same(a["by_name"], a["by_map"], "compensate_events")
    kit.same(a["contrast"], a["contrast_map"], "event_contrast")


def test_tracker_event_map_depth_device_resident():
    """event_map_depth and invdepth="event_map" on a device-resident tracker: it stays resident and tracks the bits of a run
    that is never asked"""
    a, ctl = kit.run_resident(True, _render_ask), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_mid"] and a["resident_after"] and a["resident_at_end"]
    _check_render_answer(a)
    for f in (kit.T_QUERY + 1, kit.T_QUERY + 2):
        kit.same(a["state", f], ctl["state", f], "state %d" % f)


@torch.no_grad()
def test_tracker_event_map_depth_host_driven():
    """a host-driven tracker: event_map_depth equals PointMap.render fed by hand with the tracker's own pose; a query before a
    map raises"""
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    x, y, t, p = kit.query_events(f, 3000)
    x[:600], y[:600], t[:600] = cu(np.repeat(np.float32([100.0, 101.0, 100.0]), 200)), cu(np.repeat(np.float32([80.0, 80.0, 81.0]), 200)), kit.tstamp(f)
    with pytest.raises(RuntimeError, match="no event map yet"):
        slam.event_map_depth()
    with pytest.raises(RuntimeError, match="no event map yet"):
        slam.compensate_events(x, y, t, p, invdepth="event_map")
    slam.event_map_insert(x, y, t, planes=8, range=(0.1, 1.5), min_votes=1.5, median_radius=1, min_support=2)
    out = slam.event_map_depth(min_points=1)
    cam = slam.poses_at([kit.tstamp(f)], as_tensor=True)[0][0]
    ref = slam.event_map().render(cam, frame[2].cuda().float(), 240, 320, radius=2, min_points=1)
    assert out["status"][0] == 0 and out["status"][6] > 0
    for k in ("invdepth", "key", "n", "conf", "status"):
        assert georef.same_bits(out[k].reshape(-1).view(np.int32), ref[k].cpu().numpy().reshape(-1).view(np.int32)), k
    a = slam.compensate_events(x, y, t, p, invdepth="event_map", want_xy=True)
    m = slam.event_map_depth(fill="median", as_tensor=True)["invdepth"]
    kit.same(a, slam.compensate_events(x, y, t, p, invdepth=m, want_xy=True), "compensate_events")
    with pytest.raises(RuntimeError, match="'median'"):
        slam.event_map_depth(fill="mean")
    del slam
    kit.quiesce()
