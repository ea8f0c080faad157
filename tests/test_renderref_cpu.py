"""The numpy restatement of the event map's renderer (tests/renderref.py) held by closed forms and by deliberate mistakes, the
conditions on the scenes the GPU test renders (tests/test_event_map_render_gpu.py), and what of ``ramp_point_map_render``,
``ops.PointMap.render`` and the status table can be checked without a GPU."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import pointmapref as pm
import renderref as rr

I7 = pm.IDENTITY
V = rr.VOXEL


def _voxels(cells, view=1):
    """one point at the centre of each voxel (exact in float32 with voxel 0.25)"""
    return [(((np.asarray(cells, np.float64) + 0.5) * V).astype(np.float32), np.ones(len(cells), np.float32), view)]


def _render(cells, Kc, cam=I7, order=None, **kw):
    return rr.render(rr.table_of(_voxels(cells), order=order), V, cam, Kc, rr.H, rr.W, **kw)


# ------------------------------------------------------------------------------------------------------- closed forms
def test_a_point_on_the_optical_axis():
    """no voxel is cut by the axis (voxels end at multiples of the edge): the mean point is put on it through the table's
    sums"""
    tab = rr.table_of([(np.float32([[0.05, 0.05, 2.1], [0.0, 0.0, 2.1]]), None, 1)])
    tab["sq"][:, :2] = 0                                      # the fractions of x and y: the mean point is (0, 0, z)
    z = rr.mean_points(tab, V)[0, 2]
    for Kc in (np.float32([16, 12, 8.5, 6.25]), np.float32([16, 12, 7.5, 5.5]), np.float32([16, 12, 3.2, 9.8])):
        out = rr.render(tab, V, I7, Kc, rr.H, rr.W, radius=0)
        want = (int(np.rint(Kc[3])), int(np.rint(Kc[2])))
        assert out["status"].tolist() == [0, 1, 0, 0, 0, 1, 1, 0]
        assert np.argwhere(out["key"] >= 0).tolist() == [list(want)]
        assert out["invdepth"][want] == np.float32(1.0) / z and out["n"][want] == 2 and out["conf"][want] == 2.0
        assert out["records"][0].tolist() == [Kc[2], Kc[3], np.float32(1.0) / z, 0.0]
    assert int(np.rint(np.float32(8.5))) == 8 and int(np.rint(np.float32(7.5))) == 8          # (half to even, both ways)


def test_half_pixels_go_to_the_even_pixel():
    """u = k + 0.5 exactly: X / z = 1 / 16 with fx = 16 and cx = k"""
    cell = (2, 0, 8)                                          # centre (0.625, 0.125, 2.125)
    pts = rr.mean_points(rr.table_of(_voxels([cell])), V)[0]
    fx = np.float32(0.5) / (pts[0] * (np.float32(1) / pts[2]))
    for k in range(2, 9):
        Kc = np.float32([fx, fx, k, 4.0])
        out = _render([cell], Kc, radius=0)
        u = out["records"][0, 0]
        if u != np.float32(k + 0.5):                          # (fx is rounded: only the cases that land on the half exactly count)
            continue
        assert np.argwhere(out["key"] >= 0)[0, 1] == (k if k % 2 == 0 else k + 1)
    Kc = np.float32([fx, fx, 4, 4.0])
    assert _render([cell], Kc, radius=0)["records"][0, 0] == np.float32(4.5), "the case exists"
    Kc = np.float32([fx, fx, 5, 4.0])
    assert _render([cell], Kc, radius=0)["records"][0, 0] == np.float32(5.5), "on both sides"


def test_the_nearer_layer_hides_the_farther_inside_its_footprint_only():
    Kc = np.float32([16, 16, 8.0, 6.0])
    far = [(ix, iy, 16) for ix in range(-20, 20) for iy in range(-16, 16)]           # z = 4.125: a pixel is 0.258, about a voxel
    near = (0, 0, 8)                                                                 # z = 2.125, centre pixel (9, 7)
    both = _render(far + [near], Kc, radius=2, footprint=False)
    only = _render(far, Kc, radius=2, footprint=False)
    d_near = np.float32(1) / np.float32(2.125)
    hidden = both["invdepth"] == d_near
    assert hidden.sum() == 25 and hidden[5:10, 7:12].all()
    assert pm.key32(both["invdepth"][~hidden]).tolist() == pm.key32(only["invdepth"][~hidden]).tolist()
    assert np.array_equal(both["key"][~hidden], only["key"][~hidden]) and (only["key"] >= 0).all()
    assert (both["key"][hidden] == pm.make_key(*near)).all()


def test_equal_depths_the_lower_key_wins_in_any_order():
    Kc = rr.TIE_K
    cells = [(1, 0, 256), (0, 0, 256), (0, 1, 256)]
    lowest = min(pm.make_key(*c) for c in cells)
    for order in ([0, 1, 2], [2, 1, 0], [1, 2, 0]):
        out = _render(cells, Kc, order=order, radius=0)
        assert out["status"][5] == 3 and out["status"][6] == 1 and out["key"][6, 8] == lowest
        assert len(set(pm.key32(out["records"][:, 2]).tolist())) == 1


def test_the_footprint_rule():
    """projected edge = voxel * fx * d': at most 1 pixel -> r_p = 0, 3 pixels -> r_p = 1"""
    d = np.float32([0.25, 0.2, 0.75, 0.76, 1.25, 10.0])
    r = rr.footprint_radius(d, 0.25, np.float32([16, 12, 0, 0]), 7)                  # edges 1, 0.8, 3, 3.04, 5, 40 pixels
    assert r.tolist() == [0, 0, 1, 2, 2, 7]
    assert rr.footprint_radius(d, 0.25, np.float32([12, -16, 0, 0]), 2).tolist() == [0, 0, 1, 2, 2, 2]   # max(|fx|, |fy|); the cap
    assert rr.footprint_radius(d, 0.25, np.float32([16, 12, 0, 0]), 3, footprint=False).tolist() == [3] * 6


def test_a_square_over_a_corner_covers_its_inside_pixels_only():
    Kc = np.float32([16, 16, -1.0, -1.0])                     # a point on the axis lands on pixel (-1, -1)
    tab = rr.table_of(_voxels([(0, 0, 8)]))
    tab["sq"][:, :2] = 0
    out = rr.render(tab, V, I7, Kc, rr.H, rr.W, radius=3, footprint=False)
    assert np.argwhere(out["key"] >= 0).tolist() == [[y, x] for y in range(3) for x in range(3)]
    assert out["status"].tolist() == [0, 1, 0, 0, 0, 1, 9, 0]
    out = rr.render(tab, V, I7, np.float32([16, 16, -4.0, -1.0]), rr.H, rr.W, radius=3, footprint=False)
    assert out["status"].tolist() == [0, 1, 0, 0, 1, 0, 0, 0] and (out["key"] == -1).all() and out["records"][0, 3] == 3
    out = rr.render(tab, V, I7, np.float32([16, 16, 3e38, -1.0]), rr.H, rr.W, radius=3, footprint=False)      # a huge u is outside
    assert out["status"].tolist() == [0, 1, 0, 0, 1, 0, 0, 0]


def test_behind_the_camera_and_at_the_smallest_depth():
    Kc = np.float32([16, 16, 8.0, 6.0])
    voxel = 0.2                                               # float32(1 * 0.2) IS RAMP_WARP_MIN_Z
    tab = rr.table_of([(np.float32([[0.05, 0.05, -1.7], [0.05, 0.05, 0.3], [0.05, 0.05, 0.5]]), None, 1)], voxel=voxel)
    tab["sq"][:] = 0                                          # the mean points are the voxels' corners (0, 0, i * 0.2)
    z = rr.mean_points(tab, voxel)[:, 2]
    assert sorted(z.tolist()) == [float(np.float32(-1.8)), float(rr.MIN_Z), float(np.float32(0.4))]
    out = rr.render(tab, voxel, I7, Kc, rr.H, rr.W, radius=0)
    assert out["status"].tolist() == [0, 3, 0, 2, 0, 1, 1, 0] and np.isnan(out["records"][z < 0.3]).all()
    assert out["invdepth"][6, 8] == np.float32(1) / np.float32(0.4)


def test_a_camera_to_world_translation_shifts_the_image_the_right_way():
    """the camera moves to +x: the scene moves to the left in its image"""
    Kc = np.float32([16, 16, 8.0, 6.0])
    cell = (0, 0, 8)
    a = _render([cell], Kc, radius=0)
    b = _render([cell], Kc, cam=np.float32([0.25, 0, 0, 0, 0, 0, 1]), radius=0)
    (ya, xa), (yb, xb) = np.argwhere(a["key"] >= 0)[0], np.argwhere(b["key"] >= 0)[0]
    assert ya == yb and xb == xa - 2                          # 0.25 / 2.125 * 16 = 1.88 pixels


def test_a_bad_camera_gives_nothing_plausible():
    tab = rr.table_of(_voxels([(0, 0, 8)]))
    out = rr.render(tab, V, np.r_[np.float32(np.nan), I7[1:]], rr.K, rr.H, rr.W, fill=0.5)
    assert np.isnan(out["invdepth"]).all() and np.isnan(out["conf"]).all() and (out["key"] == -1).all() and (out["n"] == 0).all()
    assert out["status"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and np.isnan(out["records"]).all()


# --------------------------------------------------------------------------------------------- scenes and mistakes
@functools.lru_cache(None)
def _scenes():
    return list(rr.gpu_scenes(full=False))


@functools.lru_cache(None)
def _truth(i):
    name, inserts, voxel, cam, Kc, kw = _scenes()[i]
    return rr.render(rr.table_of(inserts, voxel), voxel, cam, Kc, rr.H, rr.W, **kw)


def _differs(a, b):
    return any(not np.array_equal(a[k], b[k], equal_nan=True) for k in ("invdepth", "key", "n", "status"))


@pytest.mark.parametrize("mistake", rr.MISTAKES)
def test_each_mistake_is_rejected_by_the_inputs_of_the_gpu_test(mistake):
    caught = []
    for i, (name, inserts, voxel, cam, Kc, kw) in enumerate(_scenes()):
        if not inserts:
            continue
        out = rr.render(rr.table_of(inserts, voxel, mistake=mistake), voxel, cam, Kc, rr.H, rr.W, mistake=mistake, **kw)
        if _differs(out, _truth(i)):
            caught.append(name)
    print(mistake, "rejected by", caught)
    assert caught, mistake


def test_the_scenes_keep_their_margins_and_their_sizes():
    """rho - 0.5 at least 1e-3 from an integer, u and v at least 1e-2 from a rounding switch, in float64, for every scene that
    is compared through its pixels (the tie scenes are made of equal depths ON one pixel: their margin is that of the
    patch, a tenth of a pixel)"""
    for name, inserts, voxel, cam, Kc, kw in rr.gpu_scenes():
        tab = rr.table_of(inserts, voxel) if inserts else rr.table_from_ref(pm.PointMapRef(voxel), 8)
        a, b = rr.margins(tab, voxel, cam, Kc)
        if name == "half":                                    # ON the switch on purpose, and exactly so in float32: u = cx, v = cy
            out = rr.render(tab, voxel, cam, Kc, rr.H, rr.W, **kw)
            assert b == 0.0 and out["records"][0, :2].tolist() == [4.5, 6.5] and np.argwhere(out["key"] >= 0).tolist() == [[6, 4]]
            continue
        assert a >= rr.RHO_MARGIN and b >= rr.PIXEL_MARGIN, (name, a, b)
        occupied = int((tab["key"] >= 0).sum())
        if name.startswith("cloud "):
            assert occupied == int(name.split()[1]), name
        if name.startswith("tie "):
            assert occupied == int(name.split()[1]) and len(set(pm.key32(_tie_depths(tab, cam, Kc)).tolist())) == 1
    kinds = _truth(3)["kind"]                                  # the large cloud holds every kind of slot but the filtered
    assert all((kinds == k).sum() >= 4 for k in (rr.REJECTED, rr.OUTSIDE, rr.RENDERED))
    out = _truth(5)
    assert out["status"][2] > 100 and out["status"][5] > 100   # min_points = 2, min_views = 2 filter many and leave many


def _tie_depths(tab, cam, Kc):
    return rr.project(rr.mean_points(tab, V), cam, Kc)[2]


def test_the_emulator_on_the_records_gives_the_render_and_float32_stays_near_float64():
    for i, (name, inserts, voxel, cam, Kc, kw) in enumerate(_scenes()):
        tab = rr.table_of(inserts, voxel) if inserts else rr.table_from_ref(pm.PointMapRef(voxel), 8)
        a = rr.render(tab, voxel, cam, Kc, rr.H, rr.W, **kw)
        kw2 = {k: v for k, v in kw.items() if k in ("min_points", "min_views", "fill")}
        b = rr.from_records(a["records"], tab, rr.H, rr.W, **kw2)
        for k in ("invdepth", "key", "n", "conf", "status"):
            assert np.array_equal(a[k], b[k], equal_nan=True), (name, k)
        c = rr.render(tab, voxel, cam, Kc, rr.H, rr.W, dtype=np.float64, **kw)
        assert np.array_equal(a["kind"], c["kind"]) and np.array_equal(a["records"][:, 3], c["records"][:, 3], equal_nan=True), name
        if len(tab["key"]) and np.isfinite(c["records"]).any():
            assert np.nanmax(np.abs(a["records"][:, :3] - c["records"][:, :3])) < 1e-4, name
        assert np.array_equal(a["key"], c["key"]), name          # (the margins at work: float64 lands on the same pixels)


def test_the_image_does_not_depend_on_the_order_of_the_slots():
    name, inserts, voxel, cam, Kc, kw = _scenes()[4]
    tab = rr.table_of(inserts, voxel)
    perm = np.random.default_rng(1).permutation(len(tab["key"]))
    out = rr.render(rr.table_of(inserts, voxel, order=perm, capacity=1 << 13), voxel, cam, Kc, rr.H, rr.W, **kw)
    assert not _differs(out, _truth(4)) and np.array_equal(out["conf"], _truth(4)["conf"])


# ------------------------------------------------------------------------------------------------------------ entry points
def test_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    letter = {"p": ctypes.c_void_p, "i": ctypes.c_int, "z": ctypes.c_size_t, "d": ctypes.c_double, "l": ctypes.c_long}
    sig = lambda s: [letter[a] for a in s.replace(" ", "")]
    assert _lib.SIGNATURES["ramp_point_map_render"] == (ctypes.c_int, sig("pl d l i pp iiii p ppppp p z pp"))
    assert _lib.SIGNATURES["ramp_point_map_render_ws_bytes"] == (ctypes.c_size_t, sig("ii"))
    assert _lib.RAMP_MAP_RENDER_BAD_CAMERA == _lib.RAMP_DEPTH_POINTS_BAD_CAMERA == 1 and np.float32(_lib.RAMP_WARP_MIN_Z) == rr.MIN_Z
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for h, w in ((1, 1), (13, 17), (480, 640), (1, (1 << 31) - 1)):
        assert L.ramp_point_map_render_ws_bytes(h, w) == up(4 * h * w) + up(8 * h * w)
    for h, w in ((0, 17), (13, -1), (1 << 16, 1 << 15), (1, 1 << 31)):
        assert L.ramp_point_map_render_ws_bytes(h, w) == 0
    # refusals that need no device: the argument checks come before anything is launched
    words = (ctypes.c_int32 * 512)()
    p = (ctypes.addressof(words) + 255) // 256 * 256
    call = lambda **o: L.ramp_point_map_render(*{**dict(map=p, cap=8, voxel=0.1, mp=1, mv=1, cam=p, K=p, H=4, W=4, radius=2, fp=1, fill=None,
                                                         inv=p, key=p, n=p, conf=p, rec=None, ws=p, nbytes=1 << 20, status=p, stream=None), **o}.values())
    for o in (dict(H=0), dict(W=0), dict(radius=-1), dict(radius=8), dict(cap=12), dict(cap=4), dict(cap=1 << 31), dict(voxel=0.0),
              dict(voxel=float("nan")), dict(voxel=float("inf")), dict(mp=-1), dict(mv=-1), dict(map=None), dict(cam=None), dict(K=None),
              dict(inv=None), dict(ws=None), dict(status=None), dict(map=p + 8), dict(ws=p + 64), dict(key=p + 4)):
        assert call(**o) == _lib.RAMP_EINVAL, o
    assert call(H=1 << 16, W=1 << 15) == _lib.RAMP_EUNSUPPORTED
    assert call(nbytes=L.ramp_point_map_render_ws_bytes(4, 4) - 1) == _lib.RAMP_EWORKSPACE
    assert all(v == 0 for v in words), "a refused call touches nothing"
    assert callable(ops.PointMap.render) and callable(ops.point_map_render_status) and callable(TrackerQueries.event_map_depth)


def test_the_status_decoder_and_its_row_of_the_table():
    from rampvo_amd import ops
    bits, names = ops._STATUS["point_map_render"]
    assert names == ("n_occupied", "n_filtered", "n_rejected", "n_outside", "n_rendered", "n_pixels")
    assert bits["bad_camera"] is ops._STATUS["depth_points"][0]["bad_camera"]          # one row: the same bit, the same text
    assert ops.point_map_render_status(torch.tensor([1, 9, 1, 2, 3, 3, 40, 0], dtype=torch.int32)) == dict(
        bad_camera=True, n_occupied=9, n_filtered=1, n_rejected=2, n_outside=3, n_rendered=3, n_pixels=40)
    assert ops.point_map_render_status(torch.zeros(8, dtype=torch.int32))["bad_camera"] is False
    assert ops.status_message("depth_points", "bad_camera", 1) == "the camera pose at t_ref is not finite"


def test_ops_refusals_need_no_gpu():
    from rampvo_amd import ops
    from rampvo_amd.queries import TrackerQueries
    m = ops.PointMap.__new__(ops.PointMap)                    # (the constructor allocates on the device)
    m.voxel, m.capacity, m.device = 0.25, 8, torch.device("cuda")
    cam, Kc = torch.zeros(7), [16, 12, 8.5, 6.25]
    for kw, text in ((dict(height=0), "at least one pixel"), (dict(width=-3), "at least one pixel"), (dict(height=1 << 16, width=1 << 15), "fewer than 2\\^31"),
                     (dict(radius=-1), "radius is 0 .. 7"), (dict(radius=8), "radius is 0 .. 7"), (dict(min_points=-1), "not negative"),
                     (dict(min_views=-1), "not negative"), (dict(cam=torch.zeros(6)), "7 numbers"), (dict(cam=[0] * 7), "7 numbers"),
                     (dict(fill=torch.zeros(2)), "one-element"), (dict(), "GPU only")):
        a = {**dict(cam=cam, intrinsics=Kc, height=13, width=17), **kw}
        with pytest.raises(RuntimeError, match=text):
            m.render(**a)
    q = TrackerQueries()
    with pytest.raises(RuntimeError, match="no event map yet"):
        q.event_map_depth()
