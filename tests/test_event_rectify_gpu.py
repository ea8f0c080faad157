"""Lens distortion on the GPU: ``ramp_event_rectify`` / ``ramp_image_rectify`` (csrc/rectify.hip) through ``ops.event_rectify``,
``ops.image_rectify`` and the tracker's ``set_camera`` / ``rectify_events`` / ``rectify_image`` / ``distorted=True``.

Coordinates are held to the rule of ``warpref.compare`` (``rectifyref.compare_events`` / ``compare_map``): over the rows valid in
both, the largest difference from the float64 restatement is at most ``georef.bound(PIXEL_FLOOR x largest |coordinate|, env)``,
env the float32 restatement's own error.  Validity agrees with float64's except next to the two thresholds
(``rectifyref.excused``): none excused on the ordinary cameras, at most 2 % on the strong one.  Pixel values are compared BIT FOR
BIT with the exact emulator (``rectifyref.sample``) fed the kernel's own map.  The sensor is 64 x 48.

The tracker tests run the small synthetic tracker of tests/trackerkit.py."""
import numpy as np
import pytest
import torch

import georef
import rectifyref as rr
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = rr.HS, rr.WS
NAMES = {rr.PINHOLE: "pinhole", rr.RADTAN: "radtan", rr.EQUIDISTANT: "equidistant"}
EVENT_CAMERAS = tuple(n for n in rr.CAMERAS if n != "strong_wide")
_cache = {}



def _camera(name):
    from rampvo_amd import ops
    c = rr.CAMERAS[name]
    return ops.camera(NAMES[c["model"]], c["raw"], c["coeffs"], new_intrinsics=c["new"], rotation=c["R"])


def _random_events(n=4099, seed=5, margin=0.5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-margin, W - 1 + margin, n).astype(np.float32), rng.uniform(-margin, H - 1 + margin, n).astype(np.float32)


def _gpu(x, y, name, h=H, w=W, want_valid=True):
    from rampvo_amd import ops
    r = ops.event_rectify(cu(x), cu(y), _camera(name), h, w, want_valid=want_valid)
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def _base(name):
    """the 4,099 random events of camera ``name`` once: (x, y, the kernel's result)"""
    if name not in _cache:
        x, y = _random_events()
        _cache[name] = (x, y, _gpu(x, y, name))
    return _cache[name]


def _show(title, name, c):
    print("\n%s  %-12s measured %.2e  envelope %.2e  bound %.2e  valid %d  excused %d" % (title, name, c["err"], c["env"], c["bound"],
                                                                                      c["n_valid"], c["n_excused"]))


def _check_events(title, name, x, y, r, h=H, w=W):
    """one call against the restatement: coordinates, validity with its caps, the status identity and every status word"""
    c = rr.compare_events(r["xy"], x, y, rr.CAMERAS[name], h, w)
    _show(title, name, c)
    assert c["ok"], (name, c["err"], c["bound"], c["n_unexcused"])
    assert c["n_excused"] <= (0.02 * len(x) if name == "strong" else 0), (name, c["n_excused"])
    s, ref = r["status"], c["r64"]["status"]
    valid = ~np.isnan(r["xy"]).any(-1)
    assert s[0] == 0 and s[1] == len(x) and s[2:7].sum() == s[1] and s[7] == 0
    assert s[2] == ref[2] and np.array_equal(r["valid"].astype(bool), valid) and s[5] + s[6] == valid.sum()
    if c["n_differ"] == 0:
        assert s[3] == ref[3] and s[4] == ref[4]
    px, py = r["xy"][valid, 0], r["xy"][valid, 1]
    inside = (px >= 0) & (px <= w - 1) & (py >= 0) & (py <= h - 1)           # the split of the kernel's own coordinates
    assert s[6] == inside.sum()
    q = c["r64"]["xy"]
    with np.errstate(invalid="ignore"):
        border = np.minimum(np.minimum(np.abs(q[:, 0]), np.abs(q[:, 0] - (w - 1))), np.minimum(np.abs(q[:, 1]), np.abs(q[:, 1] - (h - 1))))
    if c["n_differ"] == 0 and not (border <= c["bound"]).any():              # nobody on the border: every word is float64's
        assert np.array_equal(s, ref), (s, ref)
    return c


# ------------------------------------------------------------------------------------------------ 1. events
@pytest.mark.parametrize("name", EVENT_CAMERAS)
def test_every_pixel_of_the_sensor_on_both_paths(name):
    x, y = rr.sensor_grid()
    ri, rf = _gpu(x, y, name), _gpu(x.astype(np.float32), y.astype(np.float32), name)
    for k in ("xy", "status", "valid"):
        assert georef.same_bits(ri[k], rf[k]) if k == "xy" else np.array_equal(ri[k], rf[k]), k
    c = _check_events("every pixel", name, x, y, ri)
    if name == "strong":                                                     # the failure path: both classes are there
        assert ri["status"][3] > 500 and ri["status"][5] + ri["status"][6] > 2000
        assert np.isnan(ri["xy"][ri["valid"] == 0]).all() and not np.isnan(ri["xy"][ri["valid"] == 1]).any()
    else:
        assert c["n_differ"] == 0 and ri["status"][3] == 0 and ri["status"][4] == 0
    if name == "pinhole":
        assert np.array_equal(ri["xy"], np.stack([x, y], -1).astype(np.float32))


@pytest.mark.parametrize("name", EVENT_CAMERAS)
def test_random_sub_pixel_events(name):
    x, y, r = _base(name)
    _check_events("4,099 random", name, x, y, r)
    again = _gpu(x, y, name)                                                 # a call repeats its bits
    assert georef.same_bits(again["xy"], r["xy"]) and np.array_equal(again["status"], r["status"])


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65])
def test_a_rows_bits_do_not_depend_on_n_position_or_order(N):
    for name in ("strong", "fisheye280", "rotated"):
        x, y, r = _base(name)
        head = _gpu(x[:N], y[:N], name)
        assert georef.same_bits(head["xy"], r["xy"][:N]) and np.array_equal(head["valid"], r["valid"][:N])
        assert head["status"][1] == N and head["status"][2:7].sum() == N
        tail = _gpu(x[-N:], y[-N:], name)                                    # another position in the tile, another tile
        assert georef.same_bits(tail["xy"], r["xy"][-N:])
    perm = np.random.default_rng(N).permutation(len(x))
    shuffled = _gpu(x[perm], y[perm], name)
    assert georef.same_bits(shuffled["xy"], r["xy"][perm]) and np.array_equal(shuffled["status"], r["status"])


def test_second_trip_of_the_grid():
    from rampvo_amd import _lib
    n = _lib.lib().ramp_event_rectify_grid_events() + 1
    x, y, r = _base("strong")
    reps = -(-n // len(x))
    big = _gpu(np.tile(x, reps)[:n], np.tile(y, reps)[:n], "strong")
    assert georef.same_bits(big["xy"], np.tile(r["xy"], (reps, 1))[:n]) and np.array_equal(big["valid"], np.tile(r["valid"], reps)[:n])
    assert big["status"][1] == n and big["status"][2:7].sum() == n and big["status"][3] == (big["valid"] == 0).sum()


def test_nan_and_inf_coordinates():
    from rampvo_amd import ops
    x, y, r = _base("radtan346")
    x, y = x[:300].copy(), y[:300].copy()
    x[3], y[4], x[7], y[7], x[9] = np.nan, np.inf, -np.inf, np.nan, 3e38
    g = _gpu(x, y, "radtan346")
    bad = [3, 4, 7]
    assert np.isnan(g["xy"][bad]).all() and g["status"][2] == 3 and (g["valid"][bad] == 0).all()
    assert np.isnan(g["xy"][9]).all() and g["status"][3] + g["status"][4] == 1          # finite, but nothing to invert
    keep = np.setdiff1d(np.arange(300), bad + [9])
    assert georef.same_bits(g["xy"][keep], r["xy"][keep])
    s = ops.event_rectify_status(cu(g["status"]))
    assert s["n_events"] == 300 and s["n_not_finite"] == 3 and not s["bad_camera"]
    assert s["n_not_finite"] + s["n_not_invertible"] + s["n_behind"] + s["n_outside"] + s["n_inside"] == 300
    empty = ops.event_rectify(cu(x[:0]), cu(y[:0]), _camera("radtan346"), H, W, want_valid=True)
    assert empty["xy"].shape == (0, 2) and empty["status"].tolist() == [0] * 8


def test_events_behind_the_rectified_camera():
    """a rotation of 100 degrees about y: rays on one side of the sensor end up behind the rectified camera"""
    from rampvo_amd import ops
    cam = rr._cam(rr.PINHOLE, (64.0, 64.0, 31.5, 23.5), R=rr._rotation(0.0, 100.0, 0.0))
    x, y = rr.sensor_grid()
    r = ops.event_rectify(cu(x), cu(y), ops.camera("pinhole", cam["raw"], rotation=cam["R"]), H, W, want_valid=True)
    ref = rr.event_rectify(x, y, cam, H, W)
    assert ref["status"][rr.BEHIND] > 100 and np.array_equal(r["status"].cpu().numpy(), ref["status"])
    assert np.array_equal(r["valid"].cpu().numpy().astype(bool), ref["cls"] >= rr.OUTSIDE)


@pytest.mark.parametrize("word,value", [(rr.RAW, float("nan")), (rr.RAW + 1, 0.0), (rr.NEW, -1.0), (rr.MODEL, 7.0), (31, float("inf")),
                                        (rr.COEFFS + 1, float("nan"))])
def test_a_camera_record_that_cannot_be_used(word, value):
    from rampvo_amd import ops
    cam = _camera("radtan346")
    cam[word] = value
    x, y = _random_events(500)
    x[5] = np.nan
    r = ops.event_rectify(cu(x), cu(y), cam, H, W, want_valid=True)
    assert torch.isnan(r["xy"]).all() and not r["valid"].any()
    assert r["status"].tolist() == [1, 500, 1, 499, 0, 0, 0, 0] and ops.event_rectify_status(r["status"])["bad_camera"]
    img = ops.image_rectify(cu(np.full((2, H, W), 9, np.uint8)), cam, 47, 61, fill=-2.0, want_map=True, want_mask=True)
    assert (img["image"] == -2.0).all() and torch.isnan(img["map"]).all() and not img["mask"].any()
    assert img["status"].tolist() == [1, 47 * 61, 47 * 61, 0, 0, 0, 0, 0] and ops.image_rectify_status(img["status"])["bad_camera"]


def test_event_canaries_and_the_unaligned_store_path():
    """the C entry with guard words around xy_out and valid_out; an xy_out that is 8- but not 16-byte aligned takes the other
    store path and gives the same bits"""
    from rampvo_amd import _lib
    L = _lib.lib()
    x, y, r = _base("strong")
    dx, dy, cam = cu(x), cu(y), _camera("strong")
    for N in (len(x), 256, 255, 1):
        for shift in (0, 2):
            xy, va, st = Flat(2 * N, torch.float32, -7.0, shift=shift), Flat(N, torch.uint8, 0xA5), Flat(8, torch.int32, -7)
            assert xy.t.data_ptr() % 16 == 4 * shift and xy.t.data_ptr() % 8 == 0
            rc = L.ramp_event_rectify(_lib.ptr(dx), _lib.ptr(dy), N, _lib.ptr(cam), 0, H, W, _lib.ptr(xy.t), _lib.ptr(va.t),
                                      _lib.ptr(st.t), _lib.stream())
            torch.cuda.synchronize()
            assert rc == 0
            assert xy.intact() and va.intact() and st.intact()
            assert georef.same_bits(xy.t.cpu().numpy().reshape(N, 2), r["xy"][:N])
            assert np.array_equal(va.t.cpu().numpy(), r["valid"][:N]) and int(st.t[1]) == N


def test_invalid_arguments():
    from rampvo_amd import _lib
    L, EINVAL = _lib.lib(), -1
    x, y = _random_events(64)
    dx, dy, cam = cu(x), cu(y), _camera("radtan346")
    xy, st = torch.empty((65, 2), device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    p, s = _lib.ptr, _lib.stream()
    ev = lambda **k: L.ramp_event_rectify(k.get("x", p(dx)), p(dy), k.get("N", 64), k.get("cam", p(cam)), k.get("flags", 0),
                                          k.get("H", H), k.get("W", W), k.get("xy", p(xy)), None, k.get("st", p(st)), s)
    assert ev() == 0 and ev(N=0, x=None, xy=None) == 0                      # N == 0: nothing is launched, nothing is read
    for bad in (dict(N=-1), dict(H=0), dict(W=0), dict(flags=2), dict(flags=4), dict(x=None), dict(cam=None), dict(xy=None),
                dict(st=None), dict(xy=p(xy.reshape(-1)[1:]))):
        assert ev(**bad) == EINVAL, bad
    src, out = cu(np.zeros((1, H, W), np.float32)), torch.empty((1, H, W), device="cuda")
    m = torch.empty(H * W * 2 + 1, device="cuda")
    im = lambda **k: L.ramp_image_rectify(k.get("src", p(src)), k.get("C", 1), k.get("Hs", H), k.get("Ws", W), k.get("cam", p(cam)),
                                          k.get("flags", 0), k.get("norm", 0), 0.0, k.get("H", H), k.get("W", W), k.get("out", p(out)),
                                          k.get("map", None), None, k.get("st", p(st)), s)
    assert im() == 0
    for bad in (dict(C=0), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(flags=1), dict(norm=3), dict(norm=-1), dict(src=None),
                dict(cam=None), dict(out=None), dict(st=None), dict(map=p(m[1:]))):
        assert im(**bad) == EINVAL, bad
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. images
def _source(C, dtype, seed=3):
    rng = np.random.default_rng(seed)
    if dtype == np.uint8:
        return rng.integers(0, 256, (C, H, W)).astype(np.uint8)
    return (rng.uniform(-40.0, 300.0, (C, H, W))).astype(np.float32)


@pytest.mark.parametrize("name,size", [(n, (H, W)) for n in rr.CAMERAS] + [("radtan346", (47, 61)), ("strong_wide", (61, 77)),
                                                                         ("strong_wide", (64, 80)), ("newK", (47, 61))])
def test_image_map_and_values(name, size):
    """map_out against float64 by the bound rule; the values of uint8 and fp32 sources, 1 and 3 channels, all three value
    modes, bit for bit against the emulator on the kernel's own map; fill, mask and NaN map agree"""
    from rampvo_amd import ops
    cam, h, w = _camera(name), size[0], size[1]
    first = None
    for C, dtype in ((1, np.uint8), (3, np.uint8), (1, np.float32), (3, np.float32)):
        src = _source(C, dtype)
        for norm in (None, "half", "unit"):
            r = ops.image_rectify(cu(src), cam, h, w, normalize=norm, fill=-5.0, want_map=True, want_mask=True)
            m, out, mask, st = (r[k].cpu().numpy() for k in ("map", "image", "mask", "status"))
            if first is None:
                first = m
                c = rr.compare_map(m, rr.CAMERAS[name], H, W, h, w)
                _show("image map %dx%d" % (h, w), name, c)
                assert c["ok"] and c["n_excused"] <= (0.02 * h * w if name.startswith("strong") else 0), (name, c["err"], c["bound"])
                if c["n_excused"] == 0:                                      # the sampled set is float64's: so is its count
                    assert np.array_equal(~np.isnan(m).any(-1), c["r64"]["cls"] == rr.IM_SAMPLED)
                    assert np.array_equal(st[[1, 4]], c["r64"]["status"][[1, 4]])
                if name == "strong_wide":                                    # every class of pixel is there
                    assert st[2] > 20 and st[3] > 20 and st[4] > h * w // 2
            assert georef.same_bits(m, first)                                # the map does not depend on the source
            sampled = ~np.isnan(m).any(-1)
            assert np.array_equal(mask.astype(bool), sampled) and np.array_equal(np.isnan(m[..., 0]), np.isnan(m[..., 1]))
            assert st[0] == 0 and st[1] == h * w and st[4] == sampled.sum() and st[2] + st[3] + st[4] == st[1] and not st[5:].any()
            assert (out[:, ~sampled] == -5.0).all()
            assert georef.same_bits(out, rr.sample(src, m, norm, fill=-5.0)), (name, C, dtype, norm)
    flat = ops.image_rectify(cu(_source(1, np.uint8)[0]), cam, h, w)         # a 2-D source: a 2-D image, no map unless asked
    assert flat["image"].shape == (h, w) and flat["map"] is None and flat["mask"] is None


def test_pinhole_half_is_the_reference_normalisation():
    from rampvo_amd import ops
    src = _source(3, np.uint8, seed=8)
    r = ops.image_rectify(cu(src), _camera("pinhole"), H, W, normalize="half")
    want = 2 * (torch.from_numpy(src) / 255.0) - 0.5                         # normalize_image's else branch, torch CPU fp32
    assert want.dtype == torch.float32 and georef.same_bits(r["image"].cpu().numpy(), want.numpy())
    unit = ops.image_rectify(cu(src), _camera("pinhole"), H, W, normalize="unit")
    assert georef.same_bits(unit["image"].cpu().numpy(), (2 * (torch.from_numpy(src) / 255.0) - 1).numpy())
    assert ops.image_rectify_status(r["status"]) == dict(bad_camera=False, n_pixels=H * W, n_invalid=0, n_outside=0, n_sampled=H * W)


def test_image_canaries():
    from rampvo_amd import _lib
    L = _lib.lib()
    src, cam, h, w = cu(_source(3, np.uint8)), _camera("strong_wide"), 61, 77
    out, m = Flat(3 * h * w, torch.float32, -7.0), Flat(2 * h * w, torch.float32, -7.0)
    k, st = Flat(h * w, torch.uint8, 0xA5), Flat(8, torch.int32, -7)
    rc = L.ramp_image_rectify(_lib.ptr(src), 3, H, W, _lib.ptr(cam), _lib.RAMP_RECTIFY_SRC_U8, 1, 0.0, h, w, _lib.ptr(out.t),
                              _lib.ptr(m.t), _lib.ptr(k.t), _lib.ptr(st.t), _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert out.intact() and m.intact() and k.intact() and st.intact()
    assert not (out.t == -7.0).any() and int(st.t[1]) == h * w


# ------------------------------------------------------------------------------------------------ 3. round trip, consumers
@pytest.mark.parametrize("name", ("radtan346", "fisheye280", "rotated", "newK"))
def test_checkerboard_corners_come_back(name):
    """the corners of a rectified checkerboard, distorted with the float64 forward model, land on the corners again"""
    cam = rr.CAMERAS[name]
    v, u = np.meshgrid(np.arange(4.0, H - 4, 5.0), np.arange(4.0, W - 4, 5.0), indexing="ij")
    corners = np.stack([u.reshape(-1), v.reshape(-1)], -1)
    (fx, fy, cx, cy), k, R, (nfx, nfy, ncx, ncy) = rr._params(cam, np.float64)
    ray = R.T @ np.stack([(corners[:, 0] - ncx) / nfx, (corners[:, 1] - ncy) / nfy, np.ones(len(corners))])
    xd, yd, det = rr.distort(cam["model"], k, ray[0] / ray[2], ray[1] / ray[2])
    assert (det > 0.4).all()
    x, y = (fx * xd + cx).astype(np.float32), (fy * yd + cy).astype(np.float32)
    r = _gpu(x, y, name)
    assert r["valid"].all()
    env = float(np.abs(rr.event_rectify(x, y, cam, H, W, np.float32)["xy"].astype(np.float64)
                       - rr.event_rectify(x, y, cam, H, W, np.float64)["xy"]).max())
    # rounding the raw pixel to float32 moves it by up to 2^-19 (half an ulp of 64); the inverse magnifies that by at most
    # 1 / min(det) < 2.5 and by the ratio of the focal lengths (< 1.5 here)
    b = georef.bound(georef.PIXEL_FLOOR * W, env) + 2.5 * 1.5 * 2.0 ** -19
    err = float(np.abs(r["xy"] - corners).max())
    print("\nround trip  %-12s measured %.2e  envelope %.2e  bound %.2e" % (name, err, env, b))
    assert err <= b


def test_rectified_events_go_straight_into_the_voxel_grid():
    import voxelref
    from rampvo_amd import ops
    x, y, r = _base("strong")
    rng = np.random.default_rng(17)
    t = np.sort(rng.uniform(0.0, 1.0, len(x)))
    p = rng.choice([-1, 1], len(x)).astype(np.int8)
    rect = ops.event_rectify(cu(x), cu(y), _camera("strong"), H, W)
    xy = rect["xy"]
    g = ops.event_voxel_grid(xy[:, 0], xy[:, 1], cu(t), cu(p), H, W, num_bins=5, normalize=False, subpixel=True)
    xyh = xy.cpu().numpy()
    ref = voxelref.voxel_grid(xyh[:, 0], xyh[:, 1], t, p, H, W, 5, normalize=False, subpixel=True)
    n_nan = int(np.isnan(xyh).any(-1).sum())
    assert n_nan == int(rect["status"][3]) > 500 and int(g["status"][2]) == n_nan              # the NaN rows are counted
    assert georef.same_bits(g["grid"].cpu().numpy(), ref["grid"][0]) and np.array_equal(g["status"].cpu().numpy(), ref["status"])


# ------------------------------------------------------------------------------------------------ 4. tracker
SENSOR = dict(model="radtan", raw_intrinsics=(205.0, 204.0, 158.5, 121.5), coeffs=(-0.3, 0.1, 5e-4, -4e-4, 0.0))


def _raw_events(f, n_ev=5000):
    """raw integer pixels of a 320 x 240 sensor, as a sensor gives them (not trackerkit.query_events: integer coordinates)"""
    rng = np.random.default_rng(21)
    return (cu(rng.integers(0, 320, n_ev).astype(np.int32)), cu(rng.integers(0, 240, n_ev).astype(np.int32)),
            cu(np.sort(rng.uniform(100.0 + 0.5 * (f - 2), 100.0 + 0.5 * f, n_ev))), cu(rng.choice([-1, 1], n_ev).astype(np.int8)))


def _queries(slam, x, y, t, p):
    """the distorted=True forms against the parts they are made of -> dict of (got, want) pairs on the host"""
    from rampvo_amd import ops
    cam = ops.camera(new_intrinsics=slam.intrinsics_[0] * float(slam.RES), **SENSOR)
    rect = ops.event_rectify(x, y, cam, 240, 320, want_valid=True)
    rx, ry = rect["xy"][:, 0], rect["xy"][:, 1]
    res = {}
    want = slam.compensate_events(rx, ry, t, p, want_xy=True, as_tensor=True)
    want["rectify_status"] = rect["status"]
    res["compensate"] = (slam.compensate_events(x, y, t, p, want_xy=True, as_tensor=True, distorted=True), want)
    want = slam.event_contrast(rx, ry, t, p, as_tensor=True)
    want["rectify_status"] = rect["status"]
    res["contrast"] = (slam.event_contrast(x, y, t, p, as_tensor=True, distorted=True), want)
    want = ops.event_voxel_grid(rx, ry, t, p, 240, 320, num_bins=3, subpixel=True)
    want["rectify_status"] = rect["status"]
    res["voxel"] = (slam.event_voxel_grid(x, y, t, p, num_bins=3, as_tensor=True, distorted=True), want)
    res["rectify"] = (slam.rectify_events(x, y, as_tensor=True), rect)
    img = cu(np.random.default_rng(4).integers(0, 256, (3, 240, 320)).astype(np.uint8))
    want = ops.image_rectify(img, cam, 240, 320, normalize="half", want_mask=True)
    want.pop("map")
    res["image"] = (slam.rectify_image(img, as_tensor=True), want)
    return {k: (kit.host(a), kit.host(b)) for k, (a, b) in res.items()}


@torch.no_grad()
def test_tracker_distorted_queries_device_resident():
    slam = kit.tracker(True, True)
    res = {}
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if f == kit.T_QUERY:
            x, y, t, p = _raw_events(f)
            assert kit.resident(slam)
            before = kit.host(slam.compensate_events(x.float(), y.float(), t, p, want_xy=True, as_tensor=True))
            with pytest.raises(RuntimeError, match="set_camera"):
                slam.compensate_events(x, y, t, p, distorted=True)
            with pytest.raises(RuntimeError, match="set_camera"):
                slam.rectify_events(x, y)
            slam.set_camera(**SENSOR)
            after = kit.host(slam.compensate_events(x.float(), y.float(), t, p, want_xy=True, as_tensor=True))
            res = _queries(slam, x, y, t, p)
            aligned = slam.align_events(x, y, t, p, iters=1, distorted=True)
            assert kit.resident(slam)
    assert kit.resident(slam)
    kit.same(after, before, "distorted=False after set_camera")               # today's code path, untouched
    for k, (got, want) in res.items():
        kit.same(got, want, k)
    s = res["compensate"][0]
    assert s["rectify_status"][0] == 0 and s["rectify_status"][1] == 5000 and s["rectify_status"][6] > 1000
    assert s["status"][3] == s["rectify_status"][2:5].sum()                    # the rows without a solution: the warp's NaN count
    assert np.array_equal(aligned["rectify_status"], s["rectify_status"]) and np.isfinite(aligned["variance"])
    assert res["image"][0]["image"].shape == (3, 240, 320) and res["image"][0]["mask"].sum() > 10000
    del slam
    kit.quiesce()


@torch.no_grad()
def test_tracker_distorted_queries_host_driven():
    """a host-driven tracker: numpy in, numpy out, the same bits as the parts; a record that is not finite makes the numpy
    form raise"""
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    x, y, t, p = _raw_events(f, 1000)
    before = kit.host(slam.compensate_events(x.float(), y.float(), t, p, want_xy=True, as_tensor=True))
    with pytest.raises(RuntimeError, match="set_camera"):
        slam.event_voxel_grid(x, y, t, p, distorted=True)
    slam.set_camera(**SENSOR)
    kit.same(kit.host(slam.compensate_events(x.float(), y.float(), t, p, want_xy=True, as_tensor=True)), before, "distorted=False")
    for k, (got, want) in _queries(slam, x, y, t, p).items():
        kit.same(got, want, k)
    xh, yh, th, ph = (v.cpu().numpy() for v in (x, y, t, p))
    host = slam.compensate_events(xh, yh, th, ph, want_xy=True, distorted=True)      # numpy in (int32: the integer path), numpy out
    kit.same(host, kit.host(slam.compensate_events(x, y, t, p, want_xy=True, as_tensor=True, distorted=True)), "numpy form")
    assert sorted(slam.rectify_events(xh, yh)) == ["status", "valid", "xy"]
    slam.set_camera("radtan", (float("nan"), 204.0, 158.5, 121.5), SENSOR["coeffs"])
    with pytest.raises(RuntimeError, match="camera record"):
        slam.compensate_events(xh, yh, th, ph, distorted=True)
    with pytest.raises(RuntimeError, match="camera record"):
        slam.rectify_image(np.zeros((240, 320), np.uint8))
    del slam
    kit.quiesce()
