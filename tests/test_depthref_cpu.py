"""The numpy restatement of the inverse-depth map (tests/depthref.py) against closed forms, and its checks against deliberate
mistakes: what tests/test_invdepth_map_gpu.py compares the kernel with has to be right, and has to have teeth."""
import numpy as np
import pytest

import depthref
import georef
import oracle as orc

H, W = 24, 40
K4 = np.array([30.0, 20.0, 19.5, 11.25], np.float32)
IDENT = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)


def _patches(x, y, d):
    """patches [n,3,3,3] whose centre pixels are (x, y, d)"""
    x, y, d = (np.atleast_1d(np.asarray(a, np.float32)) for a in (x, y, d))
    p = np.zeros((len(x), 3, 3, 3), np.float32)
    p[:, 0], p[:, 1], p[:, 2] = x[:, None, None], y[:, None, None], d[:, None, None]
    return p


def _flat(x, y, d):
    """records of points seen from their own camera: (x, y, d, 1)"""
    n = len(np.atleast_1d(x))
    return depthref.project(np.repeat(IDENT[None], n, 0), _patches(x, y, d), K4, IDENT, np.arange(n), 1, H, W, 5.0)[0]


# ------------------------------------------------------------------------------------------------------------ closed forms
def test_one_point_without_a_prior():
    rec = _flat([12.0], [9.0], [0.7])
    assert np.allclose(rec, [[12.0, 9.0, 0.7, 1.0]], atol=1e-6)
    r = depthref.regress(rec, 0.0, 0.0, 5.0, H, W)
    gy, gx = np.mgrid[:H, :W]
    inside = (gx - 12.0) ** 2 + (gy - 9.0) ** 2 < 25.0
    assert np.isnan(r["invdepth"][~inside]).all() and not r["weight"][~inside].any()
    assert np.allclose(r["invdepth"][inside], 0.7, atol=1e-6) and (r["weight"][inside] > 0).all()
    assert abs(r["weight"][9, 12] - 1.0) < 1e-6 and abs(r["weight"][9, 15] - (1 - 9 / 25) ** 2) < 1e-6


def test_two_points_of_equal_weight_meet_half_way():
    rec = _flat([10.0, 14.0], [9.0, 9.0], [0.2, 0.8])
    r = depthref.regress(rec, 0.0, 0.0, 5.0, H, W)
    assert abs(r["invdepth"][9, 12] - 0.5) < 1e-6
    assert r["invdepth"][9, 11] < 0.5 < r["invdepth"][9, 13]


def test_the_prior_alone_gives_the_prior():
    for dtype in (np.float64, np.float32):
        r = depthref.regress(np.zeros((0, 4)), 0.3, 3.0, 5.0, H, W, dtype)
        assert (r["invdepth"] == dtype(np.float32(0.3))).all() and not r["weight"].any()
    # a point far from the pixel leaves the prior there, a point on it is drawn to the prior by the prior's weight
    r = depthref.regress(_flat([12.0], [9.0], [0.7]), 0.3, 1.0, 5.0, H, W)
    assert abs(r["invdepth"][0, 0] - np.float32(0.3)) < 1e-7 and abs(r["invdepth"][9, 12] - 0.5) < 1e-6
    # relative: pw = weight / prior^2
    assert abs(depthref.prior_weight(0.5, 2.0, True) - 8.0) < 1e-12 and depthref.prior_weight(0.5, 0.0, True) == 0
    assert np.isnan(depthref.regress(np.zeros((0, 4)), 0.0, depthref.prior_weight(0.0, 1.0, True), 5.0, H, W)["invdepth"]).all()


def test_forward_translation():
    """the camera moves forward by b (camera-to-world translation +b z): Z' = 1 - b d, d' = d / (1 - b d)"""
    b, d = 0.5, np.array([0.2, 0.8, 1.2], np.float32)
    cam = np.array([0, 0, b, 0, 0, 0, 1], np.float32)
    x, y = np.array([19.5, 25.0, 8.0], np.float32), np.array([11.25, 6.0, 20.0], np.float32)
    rec, cls, Z = depthref.project(np.repeat(IDENT[None], 3, 0), _patches(x, y, d), K4, cam, np.arange(3), 1, H, W, 1e3)
    dd = d.astype(np.float64)
    assert np.allclose(Z, 1 - b * dd, atol=1e-7) and np.allclose(rec[:, 2], dd / (1 - b * dd), atol=1e-7)
    assert np.allclose(rec[:, 0], (x - 19.5) / (1 - b * dd) + 19.5, atol=1e-5)       # the principal point stays, the rest spreads
    # past the point: Z' = 1 - 0.9 <= MIN_Z is rejected with weight 0, as the event warp rejects it
    rec, cls, _ = depthref.project(IDENT[None], _patches([5.0], [5.0], [1.8]), K4, cam, [0], 1, H, W, 1e3)
    assert cls.tolist() == [3] and rec[0, 3] == 0 and np.isnan(rec[0, :3]).all()


def test_the_source_camera_sees_its_own_patches_where_they_are():
    s = georef.geo_scene(3)
    M, scale = s["M"], 2.5
    ids = np.arange(2 * M, 3 * M)
    cam = orc.se3_inv_f64(s["poses"][2:3].astype(np.float64))[0]
    rec, cls, Z = depthref.project(s["poses"], s["patches"], s["intr"][0], cam, ids, M, 300, 400, 1e4, scale=scale)
    c = s["patches"][ids][:, :, 1, 1].astype(np.float64)
    assert (cls == 0).all() and np.abs(Z - 1).max() < 1e-6
    assert np.abs(rec[:, 0] - scale * c[:, 0]).max() < 1e-4 and np.abs(rec[:, 1] - scale * c[:, 1]).max() < 1e-4
    assert np.abs(rec[:, 2] - c[:, 2]).max() < 1e-6 and (rec[:, 3] == 1).all()


def test_classes_and_confidence():
    n = 7
    d = np.array([0.5, np.nan, 0.0, -1.0, 0.5, 0.5, 0.5], np.float32)
    conf = np.array([2.0, 1.0, 1.0, 1.0, 0.0, np.inf, 4.0], np.float32)
    x = np.array([5, 5, 5, 5, 5, 5, W + 20], np.float32)
    args = (np.repeat(IDENT[None], n, 0), _patches(x, np.full(n, 5.0), d), K4, IDENT, np.arange(n), 1, H, W, 5.0)
    rec, cls, _ = depthref.project(*args, conf=conf)
    assert cls.tolist() == [0, 2, 2, 2, 2, 2, 4] and rec[0, 3] == 2.0 and rec[6, 3] == 0 and abs(rec[6, 0] - (W + 20)) < 1e-5
    rec, cls, _ = depthref.project(*args, conf=conf, conf_is_variance=True)       # an infinite variance: no confidence
    assert cls.tolist() == [0, 2, 2, 2, 2, 2, 4] and rec[0, 3] == 0.5
    cam = IDENT.copy()
    cam[1] = np.nan
    assert depthref.project(*args[:3], cam, *args[4:])[1].tolist() == [3, 2, 2, 2, 3, 3, 3]


# --------------------------------------------------------------------------------------------------------------- convexity
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_every_pixel_lies_between_the_extremes(dtype):
    rng = np.random.default_rng(5)
    n = 90
    rec = np.stack([rng.uniform(-6, W + 5, n), rng.uniform(-6, H + 5, n), np.exp(rng.uniform(-4, 1, n)), rng.uniform(0.1, 9, n)], -1)
    for prior, pw in ((0.0, 0.0), (0.4, 0.7)):
        r = depthref.regress(rec, prior, pw, 6.0, H, W, dtype)
        fin = np.isfinite(r["invdepth"])
        lo, hi = min(rec[:, 2].min(), prior if pw else np.inf), max(rec[:, 2].max(), prior if pw else -np.inf)
        eps = 1e-12 if dtype == np.float64 else 1e-5
        assert fin.any() and (fin.all() or not pw)
        assert r["invdepth"][fin].min() >= lo * (1 - eps) and r["invdepth"][fin].max() <= hi * (1 + eps)
        assert np.array_equal(~fin, r["smax"] <= 0) or pw


# ------------------------------------------------------------------------------------------------------------------- teeth
def _scene():
    s = georef.geo_scene(11)
    cam = orc.se3_inv_f64(s["poses"][5:6].astype(np.float64))[0].astype(np.float32)
    cam[:3] += np.float32([0.05, -0.03, 0.1])
    return s, cam, np.arange(s["n_frames"] * s["M"])


@pytest.mark.parametrize("mistake", depthref.PROJECT_MISTAKES)
def test_projection_mistakes_are_rejected(mistake):
    s, cam, ids = _scene()
    args = (s["poses"], s["patches"], s["intr"][0], cam, ids, s["M"], 120, 160, 12.0, 0.75)
    good = depthref.project(*args, dtype=np.float32)[0]
    c = depthref.compare_records(good, *args)
    assert c["ok"] and c["n_live"] >= 64, c
    assert not depthref.compare_records(depthref.project(*args, dtype=np.float32, mistake=mistake)[0], *args)["ok"]


@pytest.mark.parametrize("mistake", depthref.REGRESS_MISTAKES)
def test_regression_mistakes_are_rejected(mistake):
    rng = np.random.default_rng(12)
    n = 65
    rec = np.stack([rng.uniform(-6, W + 5, n), rng.uniform(-6, H + 5, n), np.exp(rng.uniform(-3, 0.5, n)), rng.uniform(0.5, 2, n)],
                   -1).astype(np.float32)
    good = depthref.regress(rec, 0.4, 0.7, 6.0, H, W, np.float32)
    assert depthref.compare_map(good["invdepth"], good["weight"], rec, 0.4, 0.7, 6.0, H, W)["ok"]
    bad = depthref.regress(rec, 0.4, 0.7, 6.0, H, W, np.float32, mistake=mistake)
    assert not depthref.compare_map(bad["invdepth"], bad["weight"], rec, 0.4, 0.7, 6.0, H, W)["ok"]


def test_the_float64_formula_leaves_few_pixels_undecided():
    """the GPU test of pw = 0 leaves out the pixels whose largest s_k lies within 1e-4 of 0: at most 1 % may be left out"""
    for (h, w, R, n) in ((120, 160, 12.0, 64), (120, 160, 12.0, 257), (37, 53, 1.5, 257), (37, 53, 400.0, 64)):
        rng = np.random.default_rng(n)
        rec = np.stack([rng.uniform(-R, w - 1 + R, n), rng.uniform(-R, h - 1 + R, n), rng.uniform(0.1, 1, n), np.ones(n)], -1)
        smax = depthref.regress(rec.astype(np.float32), 0.0, 0.0, R, h, w)["smax"]
        assert (np.abs(smax) <= 1e-4).mean() < 0.002
