"""The numpy restatement of the event map (tests/pointmapref.py) against closed forms, and every deliberate mistake of it
against the inputs the GPU test uses (tests/test_event_map_gpu.py compares the kernels with this restatement bit for bit: a
mistake the inputs do not reject would pass there too).  The new entry points are declared, exported and bound, and the
``ops`` wrappers refuse bad arguments without a GPU."""
import ctypes

import numpy as np
import pytest

import pointmapref as pm

V = 0.25


def _export_of(points, conf=None, voxel=V, **kw):
    m = pm.PointMapRef(voxel)
    m.insert(points, conf)
    return m.export(**kw)


# ------------------------------------------------------------------------------------------------------------ closed forms
def test_a_point_at_a_voxel_centre_exports_itself():
    for c in ([0.125, 0.375, -0.125], [-2.625, 100.125, 0.625]):
        e = _export_of([c])
        assert e["count"] == 1 and e["n"][0] == 1 and np.array_equal(e["points"][0], np.float32(c))


def test_a_point_on_a_voxel_boundary_belongs_to_the_upper_voxel():
    f = pm.fixed([[0.5, -0.5, 0.0]], None, V)
    assert f["key"][0] == pm.make_key(2, -2, 0) and np.array_equal(f["q"][0], [0, 0, 0])
    assert np.array_equal(_export_of([[0.5, -0.5, 0.0]])["points"][0], np.float32([0.5, -0.5, 0.0]))


def test_negative_coordinates_take_floor_not_truncation():
    f = pm.fixed([[-0.1, -0.25, -0.26]], None, V)
    assert f["key"][0] == pm.make_key(-1, -1, -2)
    assert pm.fixed([[-0.1, -0.25, -0.26]], None, V, "trunc")["key"][0] == pm.make_key(0, -1, -1)
    assert (f["q"] >= 0).all() and (f["q"] <= pm.AXIS).all()


def test_two_points_in_one_voxel_export_their_midpoint():
    a, b = np.float32([0.26, 0.30, -0.20]), np.float32([0.40, 0.48, -0.02])
    e = _export_of([a, b], [1.0, 2.5])
    mid = (a.astype(np.float64) + b.astype(np.float64)) / 2
    assert e["count"] == 1 and e["n"][0] == 2 and e["conf"][0] == np.float32(3.5)
    assert np.abs(e["points"][0] - mid).max() <= V * 2.0 ** -20 + 1e-7          # the fixed point's step and the float32 of the result


def test_range_ends_and_confidence_cap():
    edge = V * (pm.AXIS - 1)
    f = pm.fixed([[edge, -edge, 0], [V * pm.AXIS, 0, 0], [0, -V * pm.AXIS - V, 0], [0, -V * pm.AXIS, 0], [np.nan, 0, 0], [0, 0, np.inf]],
                 [1, 1, 1, 1, 1, 1], V)
    assert f["kind"].tolist() == [0, 2, 2, 2, 1, 1]
    f = pm.fixed([[0, 0, 0]] * 4, [-1e-3, np.nan, 3e6, 0.5], V)
    assert f["kind"].tolist() == [1, 1, 0, 0] and f["c"][2] == 1 << 36 and f["c"][3] == 1 << 15


def test_identity_cam_with_unit_intrinsics():
    u, v, d = np.array([3, 0]), np.array([-2, 5]), np.float32([0.5, 4.0])
    for dt in (np.float64, np.float32):
        X = pm.lift(u, v, d, pm.IDENTITY, [1, 1, 0, 0], dt)
        assert X.dtype == dt and np.array_equal(X, np.array([[6, -4, 2], [0, 1.25, 0.25]], dt))


def test_lift_follows_the_camera_to_world_pose():
    """a quarter turn about z and a translation: the optical axis stays, x goes to y"""
    s = np.sqrt(0.5)
    X = pm.lift([2], [0], [1.0], [10, 20, 30, 0, 0, s, s], [1, 1, 0, 0])
    assert np.allclose(X, [[10, 22, 31]], atol=1e-6)


def test_a_3x3_window_at_a_corner_has_4_pixels():
    inv = np.arange(1, 13, dtype=np.float32).reshape(3, 4)
    det = np.ones((3, 4), bool)
    val, iso = pm.masked_median(inv, det, 1, 4)
    assert not iso.any() and val[0, 0] == 2 and val[2, 3] == 8 and val[1, 1] == 6          # {1,2,5,6} -> 2; {7,8,11,12} -> 8; 9 values -> 6
    assert pm.masked_median(inv, det, 1, 5)[1][[0, 0, 2, 2], [0, 3, 0, 3]].all()            # 4 < 5: the corners are isolated
    assert pm.masked_median(inv, det, 0, 1)[0].tolist() == inv.tolist()                    # r = 0: the pixel's own value


def test_the_median_reads_detected_pixels_only_and_orders_by_bits():
    inv = np.float32([[5, -0.0, 7], [np.nan, 0.0, 1], [9, 2, 3]])
    det = np.array([[0, 1, 0], [1, 1, 0], [0, 1, 1]], bool)
    val, iso = pm.masked_median(inv, det, 1, 1)
    assert val[1, 1] == 2 and not iso.any()                                            # (-0, +0, 2, 3, NaN) -> index 2
    assert val[0, 1] == 0 and not np.signbit(val[0, 1])                                # (-0, +0, NaN) -> index 1: +0, not -0
    assert val[2, 2] == 2                                                              # (+0, 2, 3) -> index 1
    assert pm.key32(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf, np.nan])).tolist() == sorted(pm.key32(np.float32([-np.inf, -1, -0.0, 0.0, 1, np.inf, np.nan])).tolist())


def test_status_words_add_up_and_a_bad_camera_lifts_nothing():
    inv, plane, conf = pm.depth_case("random")
    r = pm.depth_points(inv, pm.CAM, pm.K, plane, conf, 1, 4, 0.4)
    st = r["status"]
    assert st[0] == 0 and st[2] + st[3] + st[4] == st[1] == (plane >= 0).sum() and st[4] == r["count"] > 0 and st[2] > 0 and st[3] > 0
    assert np.array_equal(np.isfinite(r["filtered"]).reshape(-1).nonzero()[0], r["pixel"]) and (np.diff(r["pixel"]) > 0).all()
    assert np.abs(r["points32"] - r["points64"]).max() < 1e-5
    for cam, Kc in ((pm.CAM * np.float32(np.nan), pm.K), (pm.CAM, [16, 0, 8, 6]), (pm.CAM, [16, 12, np.inf, 6])):
        b = pm.depth_points(inv, cam, Kc, plane, conf)
        assert b["status"].tolist() == [1] + [0] * 7 and b["count"] == 0 and np.isnan(b["filtered"]).all()


def test_the_map_does_not_depend_on_order_or_split():
    p, c = pm.map_points(500)
    a, b, s = pm.PointMapRef(V), pm.PointMapRef(V), pm.PointMapRef(V)
    a.insert(p, c, 3)
    b.insert(p[:123], c[:123], 3); b.insert(p[123:], c[123:], 3)
    perm = np.random.default_rng(1).permutation(500)
    s.insert(p[perm], c[perm], 3)
    ea, eb, es = a.export(), b.export(), s.export()
    for k in ea:
        assert np.array_equal(ea[k], eb[k]) and np.array_equal(ea[k], es[k]), k
    assert (np.diff(ea["key"]) > 0).all() and ea["n"].sum() == 500
    cut = a.export(min_points=2, max_out=5)
    assert cut["count"] == 5 and cut["n_cut_off"] == cut["n_passing"] - 5 > 0 and (cut["n"] >= 2).all()
    assert np.array_equal(cut["key"], ea["key"][ea["n"] >= 2][:5])


def test_views_wrap_at_64():
    m = pm.PointMapRef(V)
    for view in (0, 63, 64):
        m.insert([[0.1, 0.1, 0.1]], None, view)
    e = m.export()
    assert e["n"][0] == 3 and e["n_views"][0] == 2 and m.export(min_views=3)["count"] == 0


def test_keys_that_share_a_slot_exist():
    keys = [pm.make_key(i, 0, 0) for i in range(64)]
    slots = [pm.slot(k, 8) for k in keys]
    assert set(slots) == set(range(8)) and max(slots.count(s) for s in range(8)) >= 4        # the hash spreads and collides
    assert pm.slot(0, 8) == 0 and all(0 <= pm.slot(k, 1 << 13) < 1 << 13 for k in keys)


# ------------------------------------------------------------------------------------------------------ deliberate mistakes
@pytest.mark.parametrize("mistake", pm.FILTER_MISTAKES + pm.LIFT_MISTAKES)
def test_depth_mistakes_are_rejected_by_the_gpu_tests_inputs(mistake):
    """what the GPU test compares bit for bit (filtered map, pixel, status) or against float64 (points) differs"""
    hit = 0
    for mask in ("full", "checker", "random"):
        inv, plane, conf = pm.depth_case(mask)
        for r, s in ((1, 3), (2, 3), (3, 49), (1, 9)):
            good = pm.depth_points(inv, pm.CAM, pm.K, plane, conf, r, s)
            bad = pm.depth_points(inv, pm.CAM, pm.K, plane, conf, r, s, mistake=mistake)
            if mistake in pm.LIFT_MISTAKES:
                hit += good["count"] > 0 and np.abs(bad["points64"] - good["points64"]).max() > 1e-2
            else:
                hit += not (np.array_equal(good["filtered"], bad["filtered"], equal_nan=True) and np.array_equal(good["status"], bad["status"]))
    assert hit >= 3, (mistake, hit)


@pytest.mark.parametrize("mistake", pm.MAP_MISTAKES)
def test_map_mistakes_are_rejected_by_the_gpu_tests_inputs(mistake):
    p, c = pm.map_points(4099)
    good, bad = pm.PointMapRef(V), pm.PointMapRef(V, mistake)
    for m in (good, bad):
        m.insert(p[:2000], c[:2000], 0); m.insert(p[2000:], c[2000:], 64)
    g, b = good.export(), bad.export()
    assert not all(g[k].shape == b[k].shape and np.array_equal(g[k], b[k]) for k in ("key", "points", "n", "n_views")), mistake


# ------------------------------------------------------------------------------------------------------------ entry points
def test_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, evaluate, ops
    from rampvo_amd.queries import TrackerQueries
    letter = {"p": ctypes.c_void_p, "i": ctypes.c_int, "z": ctypes.c_size_t, "d": ctypes.c_double, "f": ctypes.c_float, "l": ctypes.c_long}
    sig = lambda s: [letter[a] for a in s.replace(" ", "")]
    assert _lib.SIGNATURES["ramp_depth_points"] == (ctypes.c_int, sig("ppppp iiii f ppppp p z pp"))
    assert _lib.SIGNATURES["ramp_depth_points_ws_bytes"] == (ctypes.c_size_t, sig("ii"))
    assert _lib.SIGNATURES["ramp_point_map_bytes"] == (ctypes.c_size_t, sig("l"))
    assert _lib.SIGNATURES["ramp_point_map_clear"] == (ctypes.c_int, sig("plp"))
    assert _lib.SIGNATURES["ramp_point_map_insert"] == (ctypes.c_int, sig("pl pp i p d i pp"))
    assert _lib.SIGNATURES["ramp_point_map_export_ws_bytes"] == (ctypes.c_size_t, sig("l"))
    assert _lib.SIGNATURES["ramp_point_map_export"] == (ctypes.c_int, sig("pl d l ii pppppp p z pp"))
    assert _lib.RAMP_DEPTH_POINTS_BAD_CAMERA == 1
    L = _lib.lib()
    for cap in (8, 1 << 13, 1 << 30):
        assert L.ramp_point_map_bytes(cap) == 64 + 64 * cap and L.ramp_point_map_export_ws_bytes(cap) >= 24 * cap
    for cap in (0, 4, 9, -8, (1 << 30) + 1, 1 << 31):
        assert L.ramp_point_map_bytes(cap) == 0 and L.ramp_point_map_export_ws_bytes(cap) == 0
    assert L.ramp_depth_points_ws_bytes(13, 17) >= 12 * 13 * 17 and L.ramp_depth_points_ws_bytes(0, 17) == 0
    assert L.ramp_depth_points_ws_bytes(1 << 16, 1 << 15) == 0
    # refusals that need no device: the argument checks come before anything is launched
    status = (ctypes.c_int32 * 8)()
    p = ctypes.addressof(status)
    assert L.ramp_point_map_clear(None, 8, None) == _lib.RAMP_EINVAL and L.ramp_point_map_clear(p, 12, None) == _lib.RAMP_EINVAL
    assert L.ramp_point_map_insert(None, 8, p, None, 1, None, 0.1, 0, p, None) == _lib.RAMP_EINVAL
    assert L.ramp_depth_points(p, None, None, p, p, 4, 4, 4, 1, 0.0, p, p, p, None, p, p, 1 << 20, p, None) == _lib.RAMP_EINVAL
    assert list(status) == [0] * 8
    for f in (ops.depth_points, ops.depth_points_status, ops.PointMap, ops.point_map_status, ops.point_map_export_status,
              TrackerQueries.event_map, TrackerQueries.event_map_insert, TrackerQueries.event_map_points, evaluate.save_points_ply):
        assert callable(f)


def test_ops_refuse_on_the_cpu():
    import torch
    from rampvo_amd import ops
    inv, cam = torch.zeros(pm.H, pm.W), torch.tensor(pm.IDENTITY)
    call = lambda **kw: ops.depth_points(**{**dict(invdepth=inv, cam=cam, intrinsics=pm.K), **kw})
    for kw, match in ((dict(invdepth=inv[0]), "height, width"), (dict(plane=torch.zeros(3, 3, dtype=torch.int32)), "shape of invdepth"),
                      (dict(confidence=inv[:2]), "shape of invdepth"), (dict(median_radius=4), "0 .. 3"), (dict(median_radius=-1), "0 .. 3"),
                      (dict(min_support=0), "at least 1"), (dict(min_invdepth=-1.0), "not negative"),
                      (dict(min_invdepth=float("nan")), "not negative"), (dict(cam=cam[:6]), "7 numbers"), (dict(), "GPU only")):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
    for kw, match in ((dict(voxel=0.0), "finite and positive"), (dict(voxel=float("inf")), "finite and positive"),
                      (dict(voxel=0.1, capacity=12), "power of two"), (dict(voxel=0.1, capacity=4), "power of two"),
                      (dict(voxel=0.1, capacity=8, device="cpu"), "GPU only")):
        with pytest.raises(RuntimeError, match=match):
            ops.PointMap(**kw)


def test_save_points_ply(tmp_path):
    from rampvo_amd.evaluate import save_points_ply
    pts = np.arange(12, dtype=np.float32).reshape(4, 3)
    for scalar, words in ((None, 3), (np.float32([1, 2, 3, 4]), 4)):
        raw = open(save_points_ply(tmp_path / "a" / "m.ply", pts, scalar, name="conf"), "rb").read()
        head, body = raw.split(b"end_header\n")
        assert b"element vertex 4" in head and (b"property float conf" in head) == (scalar is not None)
        rows = np.frombuffer(body, "<f4").reshape(4, words)
        assert np.array_equal(rows[:, :3], pts) and (scalar is None or np.array_equal(rows[:, 3], scalar))
    with pytest.raises(RuntimeError, match="one number per point"):
        save_points_ply(tmp_path / "b.ply", pts, [1.0])
