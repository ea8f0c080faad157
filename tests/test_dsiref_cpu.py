"""The numpy restatement of the event plane sweep (tests/dsiref.py) against closed forms, the two-plane scene, and its checks
against deliberate mistakes: what tests/test_event_dsi_gpu.py compares the kernel with has to be right, and has to have teeth.
The new entry points are declared, exported and bound, and ``ops.event_dsi`` refuses bad arguments without a GPU."""
import ctypes

import numpy as np
import pytest

import dsiref
import interpref
import warpref

H, W = 12, 20
K = np.array([16.0, 12.0, 9.5, 6.25], np.float32)
KP = np.array([16.0, 8.0, 10.0, 6.0], np.float32)        # powers of two: (x - cx) / fx * fx + cx is exact
ID = [0, 0, 0, 0, 0, 0, 1]


def _rot_z(theta):
    return np.array([0, 0, 0, 0, 0, np.sin(theta / 2), np.cos(theta / 2)])


# ------------------------------------------------------------------------------------------------------------ closed forms
def test_plane_depths_are_uniform_in_inverse_depth():
    d, step = dsiref.plane_depths((0.25, 1.75), 16)
    assert step == 0.1 and d.dtype == np.float32 and d[0] == 0.25 and d[15] == 1.75
    assert np.array_equal(d, (0.25 + np.arange(16) * 0.1).astype(np.float32))
    d, step = dsiref.plane_depths((0.5, 0.25), 1)
    assert step == 0.0 and d.tolist() == [0.5]
    assert not dsiref.bad_range((0.0, 1.0), 2) and not dsiref.bad_range((0.5, 0.25), 1)
    for r, D in (((0.5, 0.5), 2), ((-0.1, 1.0), 2), ((np.nan, 1.0), 1), ((0.1, np.inf), 1), ((1.0, 0.5), 3)):
        assert dsiref.bad_range(r, D), (r, D)


def test_a_pure_rotation_votes_the_same_pixel_in_every_plane():
    knots = np.stack([_rot_z(0.0), _rot_z(0.3)]).astype(np.float32)
    rng = np.random.default_rng(1)
    x, y = rng.uniform(3, W - 4, 30).astype(np.float32), rng.uniform(3, H - 4, 30).astype(np.float32)
    c, _ = dsiref.coordinates(x, y, rng.uniform(0, 1, 30), knots, [0.0, 1.0], 0.0, K, (0.1, 3.0), 7, H, W)
    assert np.isfinite(c).all() and np.abs(c - c[:, :1]).max() == 0.0
    assert np.abs(c[:, 0] - np.stack([x, y], -1)).max() > 0.1       # (and the events did move)


def test_an_event_at_the_reference_time_votes_its_own_pixel_with_weight_one():
    knots = np.array([ID, [0.3, -0.2, 0.1, 0, 0, 0, 1]], np.float32)
    x, y = np.array([3.0, 3.25, 7.5], np.float32), np.array([4.0, 4.5, 2.0], np.float32)
    c, _ = dsiref.coordinates(x, y, [1.0, 1.0, 1.0], knots, [0.0, 1.0], 1.0, KP, (0.2, 2.0), 5, H, W, dtype=np.float32)
    assert np.array_equal(c, np.broadcast_to(np.stack([x, y], -1)[:, None], (3, 5, 2)))
    v = dsiref.votes(c[:1], H, W)
    assert (v["dsi"][:, 4, 3] == 1 << 24).all() and v["dsi"].sum() == 5 << 24        # one neighbour, exactly 2^24
    v = dsiref.votes(c[1:2], H, W)
    assert (v["dsi"].sum((1, 2)) == 1 << 24).all()                                    # split over four, exactly 2^24 in all
    assert v["dsi"][2, 4, 3] == 3 << 21 and v["dsi"][2, 5, 4] == 1 << 21 and np.count_nonzero(v["dsi"][2]) == 4
    assert v["n_voted"] == 1 and v["n_no_vote"] == 0


def test_one_plane():
    knots = np.array([ID, [0.25, 0, 0, 0, 0, 0, 1]], np.float32)
    x, y = np.array([5.0], np.float32), np.array([6.0], np.float32)
    c, _ = dsiref.coordinates(x, y, [1.0], knots, [0.0, 1.0], 0.0, K, (0.8, 0.1), 1, H, W)
    assert c.shape == (1, 1, 2) and abs(c[0, 0, 0] - (5.0 + 16 * 0.25 * np.float32(0.8))) < 1e-6          # disparity fx b d_lo
    r = dsiref.detect(dsiref.votes(c.astype(np.float32), H, W)["dsi"], (0.8, 0.1), 0.5)
    assert r["n_detected"] >= 1 and set(r["plane"].reshape(-1).tolist()) == {-1, 0}
    assert (r["invdepth"][r["detected"]] == np.float32(0.8)).all() and np.isnan(r["invdepth"][~r["detected"]]).all()


def test_a_point_on_a_plane_seen_from_two_poses_meets_itself_there_and_nowhere_else():
    rngd, D, k = (0.25, 1.75), 16, 6
    d, _ = dsiref.plane_depths(rngd, D)
    knots = np.array([[-0.3, 0, 0, 0, 0, 0, 1], ID, [0.3, 0, 0, 0, 0, 0, 1]], np.float32)
    Z = 1.0 / float(d[k])
    X, Y = 0.1 * Z, -0.05 * Z                                        # the point, in the camera at t_ref = 1 (the origin)
    x = np.array([16 * (X + 0.3) / Z + 9.5, 16 * (X - 0.3) / Z + 9.5], np.float32)
    y = np.array([12 * Y / Z + 6.25] * 2, np.float32)
    c, _ = dsiref.coordinates(x, y, [0.0, 2.0], knots, [0.0, 1.0, 2.0], 1.0, K, rngd, D, H, W)
    gap = np.abs(c[0] - c[1]).max(-1)
    assert gap[k] < 1e-5 and np.abs(c[0, k] - [16 * 0.1 + 9.5, 12 * -0.05 + 6.25]).max() < 1e-5
    assert (np.delete(gap, k) > 0.9).all()                           # a plane further: 2 fx b step = 0.96 pixels apart


def test_the_refinement_of_an_exact_parabola():
    D = 12
    col = lambda k0x4: np.array([10000 - (4 * k - k0x4) ** 2 for k in range(D)], np.int64)
    dsi = np.zeros((D, 2, 3), np.int64)
    dsi[:, 0, 0], dsi[:, 0, 1], dsi[:, 0, 2] = col(21), col(20), col(18)       # vertices 5.25, 5 and 4.5 (a tie: the lowest)
    dsi[:, 1, 0], dsi[:, 1, 1] = col(0), col(44)                               # the vertex on the first and on the last plane
    dsi[:, 1, 2] = 7                                                           # flat: den == 0
    r = dsiref.detect(dsi, (0.5, 1.6), 0.0)
    assert r["plane"].tolist() == [[5, 5, 4], [0, 11, 0]]
    want = [[0.5 + 5.25 * 0.1, 0.5 + 5 * 0.1, 0.5 + 4.5 * 0.1], [0.5, 0.5 + 11 * 0.1, 0.5]]
    assert np.abs(r["invdepth"] - np.array(want)).max() < 1e-6
    assert r["invdepth"][1, 0] == np.float32(0.5) and r["invdepth"][1, 2] == np.float32(0.5)


def test_the_box_window_is_clipped_at_a_corner():
    best = np.arange(1, 21, dtype=np.int64).reshape(4, 5)
    box, n_in = dsiref.box_sums(best, 1)
    assert box[0, 0] == 1 + 2 + 6 + 7 and n_in[0, 0] == 4 and n_in[0, 2] == 6 and n_in[1, 1] == 9
    assert box[3, 4] == 14 + 15 + 19 + 20 and box[1, 1] == best[:3, :3].sum()
    box, n_in = dsiref.box_sums(best, 15)
    assert (box == best.sum()).all() and (n_in == 20).all()
    # the corner pixel holds 12 votes, its three neighbours 0: the mean over the 4 pixels inside is 3, over 9 it is 1
    dsi = np.zeros((1, 4, 5), np.int64)
    dsi[0, 0, 0] = 12 << 24
    assert dsiref.detect(dsi, (1.0, 1.0), 1.0, 1, 8.5)["detected"][0, 0]
    assert not dsiref.detect(dsi, (1.0, 1.0), 1.0, 1, 9.5)["detected"][0, 0]
    assert dsiref.detect(dsi, (1.0, 1.0), 1.0, 1, 9.0)["detected"][0, 0]            # best == threshold: detected
    # a negative offset and no floor on the votes: the three pixels beside the corner miss (0 < 12 / 6 - 1, 0 < 12 / 9 - 1),
    # every pixel whose window is empty passes (0 >= 0 - 1)
    r = dsiref.detect(dsi, (1.0, 1.0), 0.0, 1, -1.0)
    assert r["n_detected"] == 17 and not r["detected"][0, 1] and not r["detected"][1, 0] and not r["detected"][1, 1]
    # the floor: 12 * 2^24 // 9 = 22369621 = llrint(4/3 * 2^24), so the diagonal pixel passes at -4/3 exactly (0 >= 0)
    assert dsiref.detect(dsi, (1.0, 1.0), 0.0, 1, -4.0 / 3.0)["detected"][1, 1]
    assert not dsiref.detect(dsi, (1.0, 1.0), 0.0, 1, -4.0 / 3.0 + 2.0 ** -23)["detected"][1, 1]


# ------------------------------------------------------------------------------------------------------- the two-plane scene
@pytest.fixture(scope="module")
def two_plane():
    s = dsiref.TWO_PLANE
    x, y, t, knots, times = dsiref.two_plane_scene()
    c32, _ = dsiref.coordinates(x, y, t, knots, times, s["t_ref"], s["K"], s["rng"], s["D"], s["H"], s["W"], dtype=np.float32)
    return x, y, t, knots, times, c32


def test_two_plane_scene_meets_its_conditions(two_plane):
    s = dsiref.TWO_PLANE
    c32 = two_plane[5]
    v = dsiref.votes(c32, s["H"], s["W"])
    r = dsiref.detect(v["dsi"], s["rng"], s["min_votes"])
    c = dsiref.two_plane_conditions(r["plane"])
    print("two-plane scene: %d detected, %d on plane 3, %d on plane 10" % (c["n"], c["on_a"], c["on_b"]))
    assert c["all_near"] and c["on_a"] >= 30 and c["on_b"] >= 30, c
    assert v["n_voted"] == 80 * 64


# ------------------------------------------------------------------------------------------------------------------- teeth
@pytest.mark.parametrize("mistake", dsiref.COORD_MISTAKES)
def test_coordinate_mistakes_are_rejected(mistake, two_plane):
    """on the GPU test's own inputs: beyond the coordinate bound, and the two-plane scene's conditions fail"""
    knots, times = interpref.walk_scene(11, 5)
    rng = np.random.default_rng(12)
    x, y, t = rng.uniform(0, W - 1, 257).astype(np.float32), rng.uniform(0, H - 1, 257).astype(np.float32), rng.uniform(0, 4, 257)
    args = (x, y, t, knots, times, 2.0, K, (0.2, 1.4), 16, H, W)
    assert dsiref.compare(dsiref.coordinates(*args, dtype=np.float32)[0], *args)["ok"]
    assert not dsiref.compare(dsiref.coordinates(*args, mistake=mistake)[0], *args)["ok"]
    s = dsiref.TWO_PLANE
    x, y, t, knots, times, _ = two_plane
    c, _ = dsiref.coordinates(x, y, t, knots, times, s["t_ref"], s["K"], s["rng"], s["D"], s["H"], s["W"], dtype=np.float32,
                              mistake=mistake)
    r = dsiref.detect(dsiref.votes(c, s["H"], s["W"])["dsi"], s["rng"], s["min_votes"])
    if mistake != "fxfy":                                            # (fx == fy in that scene)
        assert not dsiref.two_plane_conditions(r["plane"])["ok"]


def test_truncation_for_floor_is_rejected():
    rng = np.random.default_rng(13)
    c = np.stack([rng.uniform(-1, W, (200, 3)), rng.uniform(-1, H, (200, 3))], -1).astype(np.float32)
    c[0, 0] = [-0.5, 3.0]                                            # floor -1, truncation 0
    assert not np.array_equal(dsiref.votes(c, H, W)["dsi"], dsiref.votes(c, H, W, mistake="trunc")["dsi"])


def _detect_case():
    """accumulators on which every detection mistake shows: a tie of two planes, a pixel exactly at the threshold, a corner,
    an asymmetric peak"""
    dsi = np.zeros((5, 6, 7), np.int64)
    dsi[1, 2, 2] = dsi[3, 2, 2] = 40 << 24                           # a tie: plane 1
    dsi[2, 4, 4] = 32 << 24                                          # exactly min_votes
    dsi[:, 0, 0] = np.array([0, 10, 50, 30, 0]) << 24                # a corner; the peak leans to plane 3
    dsi[2, 5, 6] = 34 << 24                                          # the opposite corner: below the mean of its 4 pixels + 26
    return dsi


@pytest.mark.parametrize("mistake", dsiref.DETECT_MISTAKES)
def test_detection_mistakes_are_rejected(mistake):
    dsi = _detect_case()
    kw = dict(rng=(0.25, 1.25), min_votes=32.0, adaptive_radius=1, adaptive_offset=26.0)
    good, bad = dsiref.detect(dsi, **kw), dsiref.detect(dsi, mistake=mistake, **kw)
    assert good["plane"][2, 2] == 1 and good["detected"][4, 4] and good["detected"][0, 0] and good["n_detected"] == 3
    assert good["invdepth"][0, 0] > np.float32(0.75)
    same = all(np.array_equal(good[k], bad[k], equal_nan=True) for k in ("plane", "detected", "invdepth"))
    assert not same
    changed = dict(tie_high=bad["plane"][2, 2] == 3, gt=not bad["detected"][4, 4], area=bad["n_detected"] != good["n_detected"],
                   sign=bad["invdepth"][0, 0] < np.float32(0.75))
    assert changed[mistake]


# ------------------------------------------------------------------------------------------------------------ entry points
def test_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    letter = {"p": ctypes.c_void_p, "i": ctypes.c_int, "z": ctypes.c_size_t, "d": ctypes.c_double}
    res, argtypes = _lib.SIGNATURES["ramp_event_dsi"]
    assert res is ctypes.c_int and argtypes == [letter[a] for a in "ppp i pp i d pp iiii d i d pppppp p z pp".replace(" ", "")]
    assert _lib.SIGNATURES["ramp_event_dsi_ws_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert _lib.SIGNATURES["ramp_event_dsi_grid_events"] == (ctypes.c_long, [])
    assert _lib.RAMP_DSI_BAD_RANGE == 2
    L = _lib.lib()
    for name in ("ramp_event_dsi", "ramp_event_dsi_ws_bytes", "ramp_event_dsi_grid_events"):
        assert hasattr(L, name), name
    small, large = L.ramp_event_dsi_ws_bytes(2, 12, 20), L.ramp_event_dsi_ws_bytes(2, 24, 20)
    assert small % 16 == 0 and large - small == 12 * 20 * 16 and L.ramp_event_dsi_ws_bytes(0, 12, 20) == 0
    # the size by the layout's own arithmetic (segment rows, C(t_ref)^-1, counters, one flag per 256 segments, 16 bytes per pixel)
    for T in (1, 2, 5, 256, 257, 258, 4096, 4097):
        for h, w in ((24, 32), (1, 1), (13, 17)):
            S = max(T - 1, 1)
            assert L.ramp_event_dsi_ws_bytes(T, h, w) == 64 * S + 128 + (4 * ((S + 255) // 256) + 15) // 16 * 16 + 16 * h * w, (T, h, w)
    for T, h, w in ((-1, 13, 17), (5, 0, 32), (5, 24, 0), (5, -1, -1)):
        assert L.ramp_event_dsi_ws_bytes(T, h, w) == 0
    assert L.ramp_event_dsi_grid_events() == L.ramp_event_warp_grid_events()
    assert callable(ops.event_dsi) and callable(ops.event_dsi_status) and callable(TrackerQueries.event_depth)


def test_ops_event_dsi_refuses_on_the_cpu():
    import torch
    from rampvo_amd import ops
    x = torch.zeros(4)
    t = torch.zeros(4, dtype=torch.float64)
    knots, times = torch.tensor([ID, ID], dtype=torch.float32), torch.tensor([0.0, 1.0], dtype=torch.float64)
    call = lambda **kw: ops.event_dsi(**{**dict(x=x, y=x, t=t, knots=knots, times=times, t_ref=0.5, intrinsics=KP, height=H, width=W,
                                                planes=4, range=(0.1, 1.0), min_votes=1.0), **kw})
    for kw, match in ((dict(times=times[:1]), "time stamps"), (dict(t=t[:3]), "differ in length"), (dict(planes=0), "at least one"),
                      (dict(height=0), "at least one"), (dict(adaptive_radius=16), "0 .. 15"), (dict(adaptive_radius=-1), "0 .. 15"),
                      (dict(planes=1 << 24, height=16, width=8), "2\\^31"), (dict(), "GPU only")):
        with pytest.raises(RuntimeError, match=match):
            call(**kw)
