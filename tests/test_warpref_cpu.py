"""The numpy restatement of the event warp (tests/warpref.py) against closed forms, and its checks against deliberate
mistakes: what tests/test_event_warp_gpu.py compares the kernel with has to be right, and has to have teeth."""
import numpy as np
import pytest

import interpref
import warpref

H, W = 12, 20
K = np.array([16.0, 12.0, 9.5, 6.25], np.float32)


def _events(seed, n, lo=0.0, hi=1.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0, W - 1, n).astype(np.float32), rng.uniform(0, H - 1, n).astype(np.float32),
            rng.uniform(lo, hi, n), rng.choice([-1, 1], n).astype(np.int8))


def _rot_z(theta):
    return np.array([0, 0, 0, 0, 0, np.sin(theta / 2), np.cos(theta / 2)])


def test_zero_motion_returns_the_input():
    x, y, t, _ = _events(1, 50, 0, 3)
    pose = interpref.rand_pose(np.random.default_rng(2), 1)
    for knots, times in ((pose, [0.0]), (np.repeat(pose, 4, 0), [0.0, 1.0, 2.0, 3.0])):
        xy, z = warpref.warp(x, y, t, knots.astype(np.float32), times, 1.5, K, 0.7, H, W)
        assert np.abs(xy[:, 0] - x).max() < 1e-6 and np.abs(xy[:, 1] - y).max() < 1e-6 and np.abs(z - 1).max() < 1e-6


def test_rotation_about_the_optical_axis():
    theta = 0.3
    Ks = np.array([16.0, 16.0, 9.5, 6.25], np.float32)
    knots = np.stack([_rot_z(0.0), _rot_z(theta)]).astype(np.float32)
    x, y, _, _ = _events(3, 40)
    xy, _ = warpref.warp(x, y, np.ones(40), knots, [0.0, 1.0], 0.0, Ks, 0.0, H, W)
    # G = C(0)^-1 C(1) = Rz(theta): a point seen at t = 1 turns by +theta into the frame of t = 0
    c, s = np.cos(theta), np.sin(theta)
    ex = c * (x - 9.5) - s * (y - 6.25) + 9.5
    ey = s * (x - 9.5) + c * (y - 6.25) + 6.25
    assert np.abs(xy[:, 0] - ex).max() < 1e-5 and np.abs(xy[:, 1] - ey).max() < 1e-5
    # half way in time, half the angle (the geodesic)
    xy, _ = warpref.warp(x, y, np.full(40, 0.5), knots, [0.0, 1.0], 0.0, Ks, 0.0, H, W)
    c, s = np.cos(theta / 2), np.sin(theta / 2)
    assert np.abs(xy[:, 0] - (c * (x - 9.5) - s * (y - 6.25) + 9.5)).max() < 1e-5


def test_translation_gives_the_closed_form_disparity():
    b, d = 0.25, 0.8
    knots = np.array([[0, 0, 0, 0, 0, 0, 1], [b, 0, 0, 0, 0, 0, 1]], np.float32)
    x, y, _, _ = _events(4, 40)
    xy, z = warpref.warp(x, y, np.ones(40), knots, [0.0, 1.0], 0.0, K, d, H, W)
    # the camera moved by +b along x (camera-to-world): the point is at P + b in the frame of t = 0: disparity fx b d
    assert np.abs(xy[:, 0] - (x + K[0] * b * d)).max() < 1e-5 and np.abs(xy[:, 1] - y).max() < 1e-5
    # a depth map with one value per pixel is sampled at the rounded pixel
    dm = (0.1 + 0.01 * np.arange(H * W, dtype=np.float32)).reshape(H, W)
    xy, _ = warpref.warp(x, y, np.ones(40), knots, [0.0, 1.0], 0.0, K, dm, H, W)
    dd = dm[np.rint(y).astype(int), np.rint(x).astype(int)]
    assert np.abs(xy[:, 0] - (x + K[0] * b * dd)).max() < 1e-5
    # forward motion past the point: Z' = 1 - 0.9 < MIN_Z is rejected, Z' = 1 - 0.5 is kept
    knots = np.array([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1.0, 0, 0, 0, 1]], np.float32)
    xy, z = warpref.warp(x[:2], y[:2], [1.0, 1.0], knots, [0.0, 1.0], 0.0, K, np.float32(0.9), H, W)
    assert np.isnan(xy).all() and np.abs(z - 0.1).max() < 1e-6
    xy, _ = warpref.warp(x[:2], y[:2], [1.0, 1.0], knots, [0.0, 1.0], 0.0, K, np.float32(0.5), H, W)
    assert np.isfinite(xy).all()


def test_invalid_rows_and_bad_times():
    x, y, t, _ = _events(5, 6)
    knots, times = interpref.walk_scene(6, 3)
    for col in range(3):
        a = [x.copy(), y.copy(), t.copy()]
        a[col][2] = np.nan
        xy, _ = warpref.warp(a[0], a[1], a[2], knots, times, 1.0, K, 0.5, H, W)
        assert np.isnan(xy[2]).all() and np.isfinite(np.delete(xy, 2, 0)).all()
    xy, _ = warpref.warp(x, y, t, knots, times[::-1], 1.0, K, 0.5, H, W)
    assert np.isnan(xy).all()


def test_weights_sum_to_one_in_fixed_point():
    rng = np.random.default_rng(7)
    xy = np.stack([rng.uniform(0, W - 1.001, 4000), rng.uniform(0, H - 1.001, 4000)], -1).astype(np.float32)
    xy[:8] = [[0, 0], [3, 4.5], [3.5, 4], [W - 2, H - 2], [1e-9, 1 - 1e-8], [5.25, 5.75], [7.999999, 2.000001], [0.5, 0.5]]
    s = warpref.scatter(xy, np.ones(4000, np.int8), H, W)
    assert np.abs(s["weight_sum"] - (1 << 24)).max() <= 4
    assert s["n_contributed"] == 4000 and s["n_outside"] == 0
    assert np.abs(s["iwe"][1].sum() - 4000 * (1 << 24)) <= 4 * 4000
    # integer coordinates: exactly one neighbour, exactly 2^24
    s = warpref.scatter(np.array([[3, 4]], np.float32), [-1], H, W, bins=1)
    assert s["iwe"][0, 4, 3] == -(1 << 24) and np.abs(s["iwe"]).sum() == 2 << 24 and s["stack"][0, 4, 3] == -(1 << 24)


def test_neighbours_outside_the_image_are_dropped():
    xy = np.array([[W - 0.5, 3.0], [4.0, -0.25], [-1.5, 3.0], [np.nan, np.nan]], np.float32)
    s = warpref.scatter(xy, [1, 1, 1, 1], H, W)
    assert s["n_outside"] == 1 and s["n_contributed"] == 2
    assert s["iwe"][1, 3, W - 1] == 1 << 23 and s["iwe"][1, 0, 4] == 3 << 22 and s["iwe"][1].sum() == (1 << 23) + (3 << 22)


def test_finish():
    acc = np.array([3 << 23, -(3 << 23), 130 << 24, -(130 << 24), (1 << 24) - 1, -(1 << 24) + 1], np.int64)
    assert warpref.finish_i8(acc).tolist() == [1, -1, -126, 126, 0, 0]
    assert warpref.finish_f32(acc)[:4].tolist() == [1.5, -1.5, 130.0, -130.0]


@pytest.mark.parametrize("mistake", warpref.WARP_MISTAKES)
def test_warp_mistakes_are_rejected(mistake):
    knots, times = interpref.walk_scene(11, 5)
    x, y, t, _ = _events(12, 300, 0.0, 4.0)
    args = (x, y, t, knots, times, 2.0, K, 0.5, H, W)
    good = warpref.warp(*args, dtype=np.float32)[0]
    assert warpref.compare(good, *args)["ok"]
    assert not warpref.compare(warpref.warp(*args, mistake=mistake)[0], *args)["ok"]


@pytest.mark.parametrize("mistake", warpref.SCATTER_MISTAKES)
def test_scatter_mistakes_are_rejected(mistake):
    rng = np.random.default_rng(13)
    xy = np.stack([rng.uniform(-1, W, 200), rng.uniform(-1, H, 200)], -1).astype(np.float32)
    xy[0] = [-0.5, 3.0]                              # floor -1, truncation 0
    p = rng.choice([-1, 1], 200)
    good, bad = warpref.scatter(xy, p, H, W, bins=5), warpref.scatter(xy, p, H, W, bins=5, mistake=mistake)
    assert not (np.array_equal(good["iwe"], bad["iwe"]) and np.array_equal(good["stack"], bad["stack"]))
    assert not np.array_equal(warpref.finish_i8(good["stack"]), warpref.finish_i8(bad["stack"])) or mistake == "trunc"


def test_bins_follow_the_event_stack():
    assert warpref.bins_of(np.arange(7), 7, 5).tolist() == [int(np.float32(5 * i) / np.float32(7)) for i in range(7)]
    assert warpref.bins_of([2 ** 25 - 1], 2 ** 25, 5).tolist() == [4]      # float32(i) rounds up to N: capped
