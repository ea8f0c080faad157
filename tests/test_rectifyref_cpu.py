"""The numpy restatement of the lens-distortion entries (tests/rectifyref.py) against closed forms and against deliberate
mistakes, the conditions on the test cameras, and ``evaluate.camera_from_kalibr``: what tests/test_event_rectify_gpu.py
compares the kernels with has to be right, has to have teeth, and its fixtures must not silently lose a class."""
import os
import re

import numpy as np
import pytest

import rectifyref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = rr.HS, rr.WS


def _events(seed=5, n=4099, margin=0.5):
    rng = np.random.default_rng(seed)
    return rng.uniform(-margin, W - 1 + margin, n).astype(np.float32), rng.uniform(-margin, H - 1 + margin, n).astype(np.float32)


def _round_trip(cam, x, y, mistake=None, min_det=0.0):
    """distort(undistort(p)) - p in raw pixels, float64, over the accepted events whose smallest determinant exceeds min_det"""
    (fx, fy, cx, cy), k, _, _ = rr._params(cam, np.float64)
    x, y = x.astype(np.float64), y.astype(np.float64)
    u = rr.undistort(cam["model"], k, (x - cx) / fx, (y - cy) / fy, fx, fy, mistake=mistake)
    xd, yd, _ = rr.distort(cam["model"], k, u["x"], u["y"])
    ok = u["ok"] & (u["detmin"] > min_det)
    return float(np.hypot(xd * fx + cx - x, yd * fy + cy - y)[ok].max()), int(ok.sum())


# ------------------------------------------------------------------------------------------------ 1. closed forms
def test_pinhole_is_the_identity_in_both_directions():
    cam = rr.CAMERAS["pinhole"]
    x, y = rr.sensor_grid()
    for T in (np.float64, np.float32):
        r = rr.event_rectify(x, y, cam, H, W, T)
        assert np.array_equal(r["xy"][:, 0], x.astype(T)) and np.array_equal(r["xy"][:, 1], y.astype(T))       # exact: dyadic numbers
        assert r["status"].tolist() == [0, H * W, 0, 0, 0, 0, H * W, 0]
        m = rr.image_map(cam, H, W, H, W, T)
        assert np.array_equal(m["map"][..., 0].reshape(-1), x.astype(T)) and np.array_equal(m["map"][..., 1].reshape(-1), y.astype(T))
        assert m["status"].tolist() == [0, H * W, 0, 0, H * W, 0, 0, 0]


def test_pure_k1_inverts_the_cubic():
    """xd = x (1 + k1 r^2) is radial: rd = r + k1 r^3, whose real root in [0, rd / (1 + k1 rd^2) ...] numpy finds"""
    k1 = -0.125                                                              # (dyadic: the record holds float32)
    cam = rr._cam(rr.RADTAN, (40.0, 40.0, 31.5, 23.5), (k1, 0, 0, 0, 0))
    x, y = _events(3, 500)
    r = rr.event_rectify(x, y, cam, H, W)
    assert (r["cls"] >= rr.OUTSIDE).all()
    xd, yd = (x.astype(np.float64) - 31.5) / 40.0, (y.astype(np.float64) - 23.5) / 40.0
    rd = np.hypot(xd, yd)
    for i in range(len(x)):
        roots = np.roots([k1, 0.0, 1.0, -rd[i]])
        real = roots[np.abs(roots.imag) < 1e-12].real
        ru = real[real >= 0].min()                                           # the principal branch: the smallest root
        for _ in range(2):                                                   # (the eigenvalue solver's 1e-8, polished)
            ru -= (k1 * ru ** 3 + ru - rd[i]) / (3 * k1 * ru ** 2 + 1)
        want = np.array([xd[i], yd[i]]) * (ru / rd[i]) * 40.0 + [31.5, 23.5]
        assert np.abs(r["xy"][i] - want).max() < 1e-9


@pytest.mark.parametrize("name", rr.ORDINARY + ("strong",))
def test_round_trip_in_float64(name):
    """distort(undistort(p)) = p to 1e-9 raw pixels (the strong camera: away from its fold, smallest determinant above 0.02)"""
    x, y = _events()
    err, n = _round_trip(rr.CAMERAS[name], x, y, min_det=0.02 if name == "strong" else 0.0)
    assert n > 3000 and err < 1e-9, (err, n)


def test_rotation_only_cameras():
    """a pinhole behind a rotation: the homography K' R K^-1, in both directions"""
    R = rr._rotation(3.0, -2.0, 4.0)
    cam = rr._cam(rr.PINHOLE, (50.0, 52.0, 30.0, 25.0), R=R, new=(45.0, 44.0, 33.0, 22.0))
    R32 = rr.record(cam)[rr.ROTATION:rr.ROTATION + 9].astype(np.float64).reshape(3, 3)
    K, Kn = np.array([[50.0, 0, 30.0], [0, 52.0, 25.0], [0, 0, 1]]), np.array([[45.0, 0, 33.0], [0, 44.0, 22.0], [0, 0, 1]])
    x, y = _events(7, 300)
    p = np.stack([x, y, np.ones_like(x)]).astype(np.float64)
    q = Kn @ R32 @ np.linalg.inv(K) @ p
    r = rr.event_rectify(x, y, cam, H, W)
    assert np.abs(r["xy"] - (q[:2] / q[2]).T).max() < 1e-10
    m = rr.image_map(cam, H, W, 40, 50)
    v, u = np.meshgrid(np.arange(40.0), np.arange(50.0), indexing="ij")
    s = K @ R32.T @ np.linalg.inv(Kn) @ np.stack([u.reshape(-1), v.reshape(-1), np.ones(2000)])
    assert np.abs(m["raw"].reshape(-1, 2) - (s[:2] / s[2]).T).max() < 1e-10
    # the two directions are inverse to each other
    back = rr.event_rectify(m["raw"][..., 0].reshape(-1), m["raw"][..., 1].reshape(-1), cam, 40, 50)
    assert np.abs(back["xy"] - np.stack([u.reshape(-1), v.reshape(-1)], -1)).max() < 1e-4      # (the events are read as float32)


def test_the_image_direction_inverts_the_event_direction():
    for name in rr.ORDINARY:
        cam = rr.CAMERAS[name]
        m = rr.image_map(cam, H, W, H, W)
        ok = m["cls"] == rr.IM_SAMPLED
        back = rr.event_rectify(m["map"][ok][:, 0], m["map"][ok][:, 1], cam, H, W)
        v, u = np.nonzero(ok)
        assert (back["cls"] >= rr.OUTSIDE).all() and np.abs(back["xy"] - np.stack([u, v], -1)).max() < 2e-4, name


def test_the_exact_emulator_against_plain_float64():
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, (3, H, W)).astype(np.uint8)
    m = rr.image_map(rr.CAMERAS["strong_wide"], H, W, 61, 77, np.float32)["map"].astype(np.float32)
    out = rr.sample(src, m, "half", fill=-3.0)
    ok = ~np.isnan(m).any(-1)
    assert (out[:, ~ok] == -3.0).all() and ok.any() and (~ok).any()
    xs, ys = m[ok][:, 0].astype(np.float64), m[ok][:, 1].astype(np.float64)
    x0, y0 = np.floor(xs).astype(int), np.floor(ys).astype(int)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    wx, wy = xs - x0, ys - y0
    s = src.astype(np.float64)
    val = (1 - wy) * ((1 - wx) * s[:, y0, x0] + wx * s[:, y0, x1]) + wy * ((1 - wx) * s[:, y1, x0] + wx * s[:, y1, x1])
    assert np.abs(out[:, ok] - (2 * val / 255 - 0.5)).max() < 1e-5
    # the last row and column: the clamped neighbour has weight 0
    edge = np.zeros((2, 2, 2), np.float32)
    edge[..., 0], edge[..., 1] = [[0, W - 1], [0, W - 1]], [[0, 0], [H - 1, H - 1]]
    assert np.array_equal(rr.sample(src, edge)[0], src[0][[0, 0, H - 1, H - 1], [0, W - 1, 0, W - 1]].reshape(2, 2).astype(np.float32))


# ------------------------------------------------------------------------------------------------ 2. the test cameras
def test_conditions_on_the_test_cameras():
    """what the GPU tests rely on, over every pixel and over the random events, in float64: the ordinary cameras have no
    invalid event and no invalid pixel and keep their determinant well above the margin; the strong camera has both classes
    in the event direction, its wide form in the image direction"""
    x, y = rr.sensor_grid()
    xr, yr = _events()
    for name in rr.ORDINARY:
        cam = rr.CAMERAS[name]
        for px, py in ((x, y), (xr, yr)):
            r = rr.event_rectify(px, py, cam, H, W)
            assert (r["cls"] >= rr.OUTSIDE).all() and np.nanmin(r["detmin"]) > 0.4 and not rr.excused(r).any(), name
        m = rr.image_map(cam, H, W, H, W)
        assert m["status"][rr.IM_INVALID] == 0 and m["status"][rr.IM_SAMPLED] > 2000 and m["det"].min() > 0.4, name
    assert rr.image_map(rr.CAMERAS["newK"], H, W, H, W)["status"][rr.IM_OUTSIDE] > 500
    for px, py in ((x, y), (xr, yr)):
        r = rr.event_rectify(px, py, rr.CAMERAS["strong"], H, W)
        assert r["status"][rr.NOT_INVERTIBLE] > 500 and r["status"][rr.OUTSIDE] + r["status"][rr.INSIDE] > 2000
        assert np.nanmin(r["detmin"]) < -0.5
    for size in ((61, 77), (64, 80)):
        m = rr.image_map(rr.CAMERAS["strong_wide"], H, W, *size)
        assert m["status"][rr.IM_INVALID] > 20 and m["status"][rr.IM_OUTSIDE] > 20 and m["status"][rr.IM_SAMPLED] > 4000
        assert m["det"].min() < -0.2


def test_the_reference_alone_meets_the_caps():
    """the float32 restatement against float64 by the GPU test's own rule: within the bound, no event of an ordinary camera
    excused, at most 2 % of the strong camera's"""
    x, y = rr.sensor_grid()
    xr, yr = _events()
    for name, cam in rr.CAMERAS.items():
        for px, py in ((x, y), (xr, yr)):
            r32 = rr.event_rectify(px, py, cam, H, W, np.float32)
            c = rr.compare_events(r32["xy"], px, py, cam, H, W)
            assert c["ok"] and c["n_unexcused"] == 0, (name, c["err"], c["bound"], c["n_unexcused"])
            cap = 0.02 * len(px) if name.startswith("strong") else 0
            assert c["n_excused"] <= cap and int(rr.excused(c["r64"]).sum()) <= cap, name
            assert 0 < c["env"] < 2e-4 or name == "pinhole"
        size = (61, 77) if name == "strong_wide" else (H, W)
        c = rr.compare_map(rr.image_map(cam, H, W, *size, np.float32)["map"], cam, H, W, *size)
        assert c["ok"] and c["n_excused"] <= 0.02 * size[0] * size[1], name


# ------------------------------------------------------------------------------------------------ 3. deliberate mistakes
def _rejected_by_events(name, mistake):
    x, y = _events()
    cam = rr.CAMERAS[name]
    bad = rr.event_rectify(x, y, cam, H, W, np.float64, mistake=mistake)
    return not rr.compare_events(bad["xy"], x, y, cam, H, W)["ok"]


def test_mistake_p1_p2_exchanged():
    assert _rejected_by_events("radtan346", "p1p2") and _rejected_by_events("strong", "p1p2")


def test_mistake_fx_fy_exchanged():
    assert _rejected_by_events("radtan346", "fxfy") and _rejected_by_events("equi640", "fxfy")
    cam = rr.CAMERAS["radtan346"]
    assert not rr.compare_map(rr.image_map(cam, H, W, H, W, mistake="fxfy")["map"], cam, H, W, H, W)["ok"]


def test_mistake_rotation_transposed():
    assert _rejected_by_events("rotated", "transpose")
    cam = rr.CAMERAS["rotated"]
    assert not rr.compare_map(rr.image_map(cam, H, W, H, W, mistake="transpose")["map"], cam, H, W, H, W)["ok"]


def test_mistake_one_newton_step_too_few():
    """seven steps pass the pixel bound everywhere -- only the 1e-9 round trip sees the missing step"""
    x, y = _events()
    err8, _ = _round_trip(rr.CAMERAS["strong"], x, y, min_det=0.02)
    err7, _ = _round_trip(rr.CAMERAS["strong"], x, y, mistake="iters", min_det=0.02)
    assert err8 < 1e-9 < err7, (err7, err8)


def test_mistake_determinant_test_dropped():
    """without it the strong camera yields rows that pass the residual test on the wrong branch"""
    x, y = rr.sensor_grid()
    cam = rr.CAMERAS["strong"]
    good, bad = rr.event_rectify(x, y, cam, H, W), rr.event_rectify(x, y, cam, H, W, mistake="nodet")
    wrong = (bad["cls"] >= rr.OUTSIDE) & (good["cls"] == rr.NOT_INVERTIBLE)
    clear = wrong & (good["detmin"] < -0.5)                                  # far beyond the fold, nothing to excuse
    assert clear.sum() > 0
    c = rr.compare_events(bad["xy"], x, y, cam, H, W)
    assert not c["ok"] and c["n_unexcused"] == (wrong & ~rr.excused(good)).sum() >= clear.sum()


def test_mistake_ratio_inverted():
    cam = rr.CAMERAS["fisheye280"]
    assert not rr.compare_map(rr.image_map(cam, H, W, H, W, mistake="ratio")["map"], cam, H, W, H, W)["ok"]
    (fx, fy, cx, cy), k, _, _ = rr._params(cam, np.float64)
    xd, yd, _ = rr.distort(cam["model"], k, np.array([0.3]), np.array([0.4]), mistake="ratio")
    good = rr.distort(cam["model"], k, np.array([0.3]), np.array([0.4]))
    assert abs(xd[0] - good[0][0]) > 0.01


def test_every_mistake_is_covered():
    src = open(os.path.abspath(__file__)).read()
    for m in rr.MISTAKES:
        assert re.search(r'mistake="%s"|, "%s"\)' % (m, m), src), m


# ------------------------------------------------------------------------------------------------ 4. the package's side
KALIBR = {"cam0": {"camera_model": "pinhole", "intrinsics": [250.0, 250.5, 172.2, 131.4], "distortion_model": "radtan",
                   "distortion_coeffs": [-0.38, 0.17, 4e-4, -6e-4], "resolution": [346, 260]},
          "cam1": {"camera_model": "pinhole", "intrinsics": [560.0, 561.0, 322.0, 236.0], "distortion_model": "equidistant",
                   "distortion_coeffs": [-0.035, 0.012, -0.006, 0.0012], "resolution": [640, 480]},
          "cam2": {"camera_model": "pinhole", "intrinsics": [320.0, 320.0, 320.0, 240.0], "resolution": [640, 480]},
          "cam3": {"camera_model": "omni", "intrinsics": [1.0, 320.0, 320.0, 320.0, 240.0], "distortion_model": "fov",
                   "distortion_coeffs": [0.9], "resolution": [640, 480]}}


def test_camera_from_kalibr():
    from rampvo_amd import evaluate
    c = evaluate.camera_from_kalibr(KALIBR)
    assert c == dict(model="radtan", raw_intrinsics=(250.0, 250.5, 172.2, 131.4), coeffs=(-0.38, 0.17, 4e-4, -6e-4),
                     resolution=(346, 260))
    c = evaluate.camera_from_kalibr(KALIBR, resize_to=(352, 264))            # set_global_params: c += (resize_to - resolution) / 2
    assert c["raw_intrinsics"] == (250.0, 250.5, 172.2 + 3.0, 131.4 + 2.0) and c["resolution"] == (346, 260)
    c = evaluate.camera_from_kalibr(KALIBR, "cam1", resize_to=(630, 470))
    assert c["model"] == "equidistant" and c["raw_intrinsics"] == (560.0, 561.0, 317.0, 231.0) and len(c["coeffs"]) == 4
    c = evaluate.camera_from_kalibr(KALIBR, "cam2")
    assert c["model"] == "pinhole" and c["coeffs"] == ()
    with pytest.raises(ValueError, match="fov"):
        evaluate.camera_from_kalibr(KALIBR, "cam3")
    with pytest.raises(ValueError, match="coefficients"):
        evaluate.camera_from_kalibr({"cam0": dict(KALIBR["cam0"], distortion_coeffs=[0.1])})


def test_camera_words_and_constants_mirror_the_header():
    from rampvo_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    for name in ("RAMP_CAMERA_WORDS", "RAMP_CAMERA_RAW", "RAMP_CAMERA_MODEL", "RAMP_CAMERA_COEFFS", "RAMP_CAMERA_ROTATION",
                 "RAMP_CAMERA_NEW", "RAMP_CAM_PINHOLE", "RAMP_CAM_RADTAN", "RAMP_CAM_EQUIDISTANT", "RAMP_RECTIFY_ITERS",
                 "RAMP_RECTIFY_XY_I32", "RAMP_RECTIFY_SRC_U8", "RAMP_RECTIFY_NORM_NONE", "RAMP_RECTIFY_NORM_HALF",
                 "RAMP_RECTIFY_NORM_UNIT", "RAMP_RECTIFY_BAD_CAMERA"):
        value = int(re.search(r"#define %s (\d+)" % name, header).group(1))
        assert getattr(_lib, name) == value, name
    assert float(re.search(r"#define RAMP_RECTIFY_TOL ([0-9.]+)f", header).group(1)) == _lib.RAMP_RECTIFY_TOL == rr.TOL
    assert (rr.WORDS, rr.RAW, rr.MODEL, rr.COEFFS, rr.ROTATION, rr.NEW, rr.ITERS) == (
        _lib.RAMP_CAMERA_WORDS, _lib.RAMP_CAMERA_RAW, _lib.RAMP_CAMERA_MODEL, _lib.RAMP_CAMERA_COEFFS, _lib.RAMP_CAMERA_ROTATION,
        _lib.RAMP_CAMERA_NEW, _lib.RAMP_RECTIFY_ITERS)
    names = {rr.PINHOLE: "pinhole", rr.RADTAN: "radtan", rr.EQUIDISTANT: "equidistant"}
    for name, cam in rr.CAMERAS.items():                                     # ops.camera's host part lays the record out as rectifyref does
        w = np.asarray(ops.camera_words(names[cam["model"]], cam["raw"], cam["coeffs"], cam["R"]), np.float32)
        w[rr.NEW:rr.NEW + 4] = rr.new_intrinsics(cam)
        assert np.array_equal(w, rr.record(cam)), name
    with pytest.raises(RuntimeError, match="model"):
        ops.camera_words("fov", (1, 1, 0, 0))
    with pytest.raises(RuntimeError, match="coefficients"):
        ops.camera_words("equidistant", (1, 1, 0, 0), (0.1, 0.2))
    lib = _lib.lib()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    for name in ("ramp_event_rectify", "ramp_image_rectify", "ramp_event_rectify_grid_events"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
