"""The restatement of the time surface and of the localisation against the event map (tests/localizeref.py), held by closed
forms, and each deliberate mistake rejected by the inputs the GPU tests use; the convergence scene's conditions; the entry
points, their refusals and the status decoders.  No GPU."""
import ctypes
import math

import numpy as np
import pytest
import torch

import localizeref as lr
import pointmapref as pm
import poseref
import renderref as rr
import scenes

f32 = np.float32
bits = lambda a: np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[np.asarray(a).dtype.itemsize])


# ------------------------------------------------------------------------------------------------------- closed forms
def test_an_event_at_t_ref_gives_zero_and_a_pixel_without_events_one():
    o = lr.time_surface([3.2], [4.9], [2.0], 2.0, 0.1, 8, 9, smooth=0)
    assert o["surface"][5, 3] == 0.0 and (np.delete(o["surface"].reshape(-1), 5 * 9 + 3) == 1.0).all()
    assert o["status"].tolist() == [0, 1, 0, 0, 0, 1, 1, 0]
    plain = lr.time_surface([3.2], [4.9], [2.0], 2.0, 0.1, 8, 9, smooth=0, negate=False)["surface"]
    assert plain[5, 3] == 1.0 and plain.sum() == 1.0
    late = lr.time_surface([3.2, 3.0], [4.9, 5.0], [2.0 - 0.1, np.nextafter(2.0, 3.0)], 2.0, 0.1, 8, 9, smooth=0)
    assert late["status"].tolist() == [0, 2, 0, 0, 1, 1, 1, 0] and late["surface"][5, 3] == f32(1) - np.exp(f32(-1))


def test_the_binomial_of_a_constant_and_of_an_impulse():
    # (constants of at most 20 significant bits: every partial sum k c, k <= 16, is then exact in fp32 in the order written)
    for c in (f32(0.3125), f32(1.0), f32(12345.0 / 65536.0), f32(1.0) - f32(2.0 ** -20)):
        assert (bits(lr.binomial(np.full((13, 17), c, f32), 8)) == bits(c)).all()
    img = np.zeros((13, 17), f32)
    img[6, 8] = 1
    taps = np.array([1, 4, 6, 4, 1], f32) / 16
    want = np.zeros((13, 17), f32)
    want[4:9, 6:11] = np.outer(taps, taps)
    assert np.array_equal(lr.binomial(img, 1), want)
    for shape in ((1, 1), (1, 17), (13, 1)):                  # replicated edges: a constant stays a constant
        assert (lr.binomial(np.full(shape, f32(0.7)), 3) == f32(0.7)).all()


def test_a_point_on_the_optical_axis_has_no_rotation_about_z_in_its_row():
    J = lr.rows(f32([0.3]), f32([-0.2]), f32([[0, 0, 2.5]]), rr.K)
    assert J[0, 5] == 0.0 and J[0, 0] != 0 and J[0, 3] != 0


def _cost64(tab, voxel, cam64, Kc, surface, k):
    """the restatement's cost with the projection in float64 at a float64 pose (smooth in the pose inside a cell)"""
    cam = np.asarray(cam64, np.float64)
    u, v, d, Xc = (a for a in _project64(rr.mean_points(tab, voxel), cam, Kc))
    S = np.asarray(surface, np.float64)
    x0, y0 = np.floor(u), np.floor(v)
    ax, ay, ix, iy = u - x0, v - y0, x0.astype(int), y0.astype(int)
    r = (1 - ay) * ((1 - ax) * S[iy, ix] + ax * S[iy, ix + 1]) + ay * ((1 - ax) * S[iy + 1, ix] + ax * S[iy + 1, ix + 1])
    return float(lr.huber(r, k)[0].sum()), r


def _project64(X, cam, Kc):
    k = np.asarray(Kc, np.float64)
    Xc = poseref.qrot(cam[3:] * np.array([-1.0, -1, -1, 1]), X.astype(np.float64) - cam[:3])
    d = 1.0 / Xc[:, 2]
    return k[0] * (Xc[:, 0] * d) + k[2], k[1] * (Xc[:, 1] * d) + k[3], d, Xc


def test_the_row_is_the_derivative_of_the_restatements_own_cost():
    """central differences of the float64 cost over the LEFT perturbation of the world-to-camera pose, six voxels in the interior"""
    ins = lr.loc_cloud(6, seed=6)
    tab, S = rr.table_of(ins), lr.surface_13x17(1)
    cam = lr.CAM.astype(np.float64)
    for k in (0.0, 0.4):
        u, v, d, Xc = _project64(rr.mean_points(tab, lr.VOXEL), cam, lr.K)
        r, gu, gv = (a.astype(np.float64) for a in lr.sample(S, u.astype(f32), v.astype(f32)))
        J = lr.rows(gu.astype(f32), gv.astype(f32), Xc.astype(f32), lr.K)
        rho, w = lr.huber(r, k)
        grad = 2 * ((w * r)[:, None] * J).sum(0)              # d sum rho / d xi = 2 sum w r J
        h = 1e-6
        for i in range(6):
            e = np.zeros(6)
            e[i] = h
            # T <- Exp(xi) T is C <- C Exp(xi)^-1: the retraction, exact to first order
            fp = _cost64(tab, lr.VOXEL, lr.retract(cam, e), lr.K, S, k)[0]
            fm = _cost64(tab, lr.VOXEL, lr.retract(cam, -e), lr.K, S, k)[0]
            assert abs((fp - fm) / (2 * h) - grad[i]) <= 2e-4 * max(1.0, abs(grad[i])), (k, i, (fp - fm) / (2 * h), grad[i])


def test_the_cayley_retraction_is_the_exponential_to_second_order_and_the_identity_at_zero():
    for C in ([0.3, -0.2, 0.5, 0, 0, 0, 1], [1, 2, 3, 1, 0, 0, 0], [-1, 0.25, 8, 0.5, 0.5, 0.5, 0.5]):
        out = lr.retract(C, [0.0] * 6)
        assert (bits(np.asarray(out)) == bits(np.asarray(C, np.float64))).all(), C
    xi = np.array([0.3, -0.2, 0.1, 0.2, -0.1, 0.15])
    errs = []
    for s in (1e-1, 1e-2):
        D = scenes.se3_exp_np(s * xi).astype(np.float64)      # (t, q) of Exp(xi)
        Di = poseref.invert_pose(D)
        got = np.asarray(lr.retract([0, 0, 0, 0, 0, 0, 1.0], s * xi))   # I D^-1
        errs.append(np.abs(got - Di * np.sign(Di[6]) * np.sign(got[6])).max())
    assert errs[0] < 2e-3 and errs[1] < errs[0] / 50, errs    # the difference is of third order in the step (float32 oracle floor)


def test_a_quadratic_bowl_is_solved_in_one_accepted_step_without_damping():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    Hm = A @ A.T + 6 * np.eye(6)
    x_star = 1e-3 * rng.normal(size=6)
    state = {"x": np.zeros(6)}

    def evaluate(pose32):                                     # a bowl over the step itself: the machine's linear algebra alone
        x = state["x"]
        cost = float((x - x_star) @ Hm @ (x - x_star))
        return cost, [Hm[p, q] for p, q in lr.TRI], list(Hm @ (x - x_star)), 100.0, [0] * 8

    m = lr.Machine(lr.CAM, lambda0=0.0, min_step=1e-12, iters=5)
    m.step(0, *evaluate(None))
    assert np.allclose(m.delta, x_star, rtol=1e-9, atol=1e-15)
    state["x"] = np.asarray(m.delta)
    m.step(1, *evaluate(None))
    assert m.n_accepted == 1 and m.f < 1e-20 and m.lam == 1e-12
    state["x"] = np.asarray(m.delta) + state["x"]
    assert np.linalg.norm(m.delta) < 1e-9


# ------------------------------------------------------------------------------------------------- deliberate mistakes
def _gpu_eval_inputs():
    ins = lr.loc_cloud(4099, seed=7)
    return rr.table_of(ins), lr.surface_13x17(0)


@pytest.mark.parametrize("mistake", lr.MISTAKES)
def test_each_mistake_is_rejected_by_the_inputs_of_the_gpu_tests(mistake):
    if mistake in ("trunc", "late", "min"):
        x, y, t = lr.event_case(4099, seed=1)
        a, b = lr.time_surface(x, y, t, 2.0, 0.5, lr.H, lr.W), lr.time_surface(x, y, t, 2.0, 0.5, lr.H, lr.W, mistake=mistake)
        assert not np.array_equal(a["surface"], b["surface"]) and not np.array_equal(a["last_t"], b["last_t"], equal_nan=True)
        return
    if mistake == "halve":
        s = lr.convergence_scene()
        fn = lr.ref_evaluator(s["tab"], s["voxel"], s["K"], s["surface"])
        a, b = lr.localize(fn, s["start"], iters=s["iters"]), lr.localize(fn, s["start"], iters=s["iters"], mistake="halve")
        assert a["info"][3] + a["info"][2] > a["info"][1] + 1, "the scene rejects at least one step"
        assert not np.array_equal(a["pose"], b["pose"], equal_nan=True) or a["info"].tolist() != b["info"].tolist()
        return
    tab, S = _gpu_eval_inputs()
    k = 0.5 if mistake == "huber_inv" else 0.0
    a, b = lr.evaluate(tab, lr.VOXEL, lr.CAM, lr.K, S, k=k), lr.evaluate(tab, lr.VOXEL, lr.CAM, lr.K, S, k=k, mistake=mistake)
    scale = np.abs(a["sums"][:28]).max()
    assert np.abs(a["sums"][:28] - b["sums"][:28]).max() > 1e-3 * scale, mistake


# ----------------------------------------------------------------------------------------------------------- margins
EVAL_TABLES = (0, 1, 2, 6, 4099)


def test_the_scenes_keep_their_margins_and_their_sizes():
    for N in EVAL_TABLES:
        tab = rr.table_of(lr.loc_cloud(N, seed=N))
        assert (tab["key"] >= 0).sum() == N and lr.uv_margin(tab, lr.VOXEL, lr.CAM, lr.K) >= lr.MARGIN, N
    tab = rr.table_of(lr.loc_cloud(4099, seed=7))
    o = lr.evaluate(tab, lr.VOXEL, lr.CAM, lr.K, lr.surface_13x17(0))
    assert o["status"][3] >= 8 and o["status"][4] > 100 and o["status"][5] > 100, o["status"]     # rejected, out of reach, in reach
    assert (rr.table_of(lr.loc_cloud(5, seed=5))["key"] >= 0).sum() == 5
    for N in (1, 2, 4099):
        x, y, t = lr.event_case(N, seed=N)
        assert min(lr.half_margin(x).min(), lr.half_margin(y).min()) >= lr.MARGIN
    s = lr.convergence_scene()
    assert min(lr.half_margin(s["events"][0]).min(), lr.half_margin(s["events"][1]).min()) >= lr.MARGIN
    assert s["h"] <= 64 and s["w"] <= 80 and 200 <= (s["tab"]["key"] >= 0).sum() <= 400


def test_the_emulator_on_the_records_gives_the_evaluation():
    tab, S = _gpu_eval_inputs()
    for k in (0.0, 0.5):
        o = lr.evaluate(tab, lr.VOXEL, lr.CAM, lr.K, S, k=k)
        e = lr.evaluate_records(tab, o["records"], lr.K, S, k=k)
        assert np.array_equal(e["kind"], o["kind"]) and np.array_equal(e["sums"], o["sums"])
        at = e["at"]
        assert np.array_equal(e["r"], o["records"][at, 2]) and np.array_equal(e["gu"], o["records"][at, 3])
        r = o["records"][at, 2]
        assert (np.abs(r) > 0.5).any() and (np.abs(r) < 0.5).any(), "residuals on both sides of the Huber threshold"


# ------------------------------------------------------------------------------------------------ the convergence scene
def test_the_convergence_scene_meets_its_conditions():
    s = lr.convergence_scene()
    fn = lr.ref_evaluator(s["tab"], s["voxel"], s["K"], s["surface"])
    out = lr.localize(fn, s["start"], iters=s["iters"])
    t0, r0 = lr.pose_distance(s["start"], s["true"])
    t1, r1 = lr.pose_distance(out["pose"], s["true"])
    print("convergence scene: %s after %d accepted steps and %d evaluations, cost %.4f -> %.4f, translation %.4f -> %.4f, rotation %.4f -> %.4f"
          % (lr.REASONS[out["reason"]], out["info"][1], out["info"][2], out["result"][1], out["result"][0], t0, t1, r0, r1))
    assert out["reason"] in (lr.ITERS, lr.CONVERGED)                       # (a)
    assert out["result"][0] < out["result"][1]                            # (b)
    assert t1 < 0.5 * t0 and r1 < 0.5 * r0                                # (c)
    assert np.all(np.diff(out["history"][:out["info"][1]]) < 0)


def test_the_machines_ends():
    s = lr.convergence_scene()
    fn = lr.ref_evaluator(s["tab"], s["voxel"], s["K"], s["surface"])
    assert lr.localize(fn, s["start"], iters=0)["reason"] == lr.ITERS
    full_run = lr.localize(fn, s["start"], iters=3)
    need = int(full_run["info"][2])
    assert lr.localize(fn, s["start"], iters=3, max_evals=need - 1)["reason"] == lr.BUDGET
    one = lr.localize(fn, s["start"], iters=3, max_evals=1)
    assert one["reason"] == lr.BUDGET and one["info"].tolist()[:3] == [lr.BUDGET, 0, 1] and np.array_equal(one["pose"], s["start"].astype(np.float64))
    few = rr.table_of(lr.loc_cloud(5, seed=5))
    out = lr.localize(lr.ref_evaluator(few, lr.VOXEL, lr.K, lr.surface_13x17(0)), lr.CAM)
    assert out["reason"] == lr.FEW and np.isnan(out["pose"]).all() and np.isnan(out["pose_f32"]).all()
    tab = rr.table_of(lr.loc_cloud(6, seed=6))
    flat = lr.localize(lr.ref_evaluator(tab, lr.VOXEL, lr.K, np.ones((lr.H, lr.W), f32)), lr.CAM)
    # a surface of all ones: b = 0 AND H = 0, so the first pivot is not positive -- the machine as written says SINGULAR
    assert flat["reason"] == lr.SINGULAR and np.isnan(flat["pose"]).all() and not flat["gradient"].any()
    nan = lr.localize(lr.ref_evaluator(tab, lr.VOXEL, lr.K, np.full((lr.H, lr.W), np.nan, f32)), lr.CAM)
    assert nan["reason"] == lr.SINGULAR and np.isnan(nan["result"][0]) and np.isnan(nan["pose"]).all()
    bad = lr.CAM.copy()
    bad[2] = np.inf
    out = lr.localize(lr.ref_evaluator(tab, lr.VOXEL, lr.K, lr.surface_13x17(0)), bad)
    assert out["info"][4] == 1 and np.isnan(out["pose"]).all()
    col = rr.table_of(lr.collinear_case())
    out = lr.localize(lr.ref_evaluator(col, lr.VOXEL, lr.K, lr.surface_13x17(0)), lr.CAM)
    assert lr.evaluate(col, lr.VOXEL, lr.CAM, lr.K, lr.surface_13x17(0))["status"][5] == 6 and out["reason"] != 0


# ---------------------------------------------------------------------------------------------------------- entry points
def test_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    letter = {"p": ctypes.c_void_p, "i": ctypes.c_int, "z": ctypes.c_size_t, "d": ctypes.c_double, "l": ctypes.c_long}
    sig = lambda s: [letter[a] for a in s.replace(" ", "")]
    S = _lib.SIGNATURES
    assert S["ramp_time_surface"] == (ctypes.c_int, sig("ppp l p dd iiii ppp p z pp"))
    assert S["ramp_time_surface_ws_bytes"] == (ctypes.c_size_t, sig("ii"))
    assert S["ramp_point_map_localize_eval"] == (ctypes.c_int, sig("pl d l i ppp ii d pp p z pp"))
    assert S["ramp_point_map_localize"] == (ctypes.c_int, sig("pl d l i ppp ii ddd ii pppppp pp p z p"))
    assert S["ramp_point_map_localize_ws_bytes"] == (ctypes.c_size_t, sig("li")) and S["ramp_point_map_localize_grid_slots"] == (ctypes.c_long, [])
    assert _lib.RAMP_MAP_LOCALIZE_BAD_CAMERA == _lib.RAMP_MAP_RENDER_BAD_CAMERA == 1 and _lib.RAMP_TIME_SURFACE_BAD_ARGS == 1
    assert (_lib.RAMP_LOCALIZE_ITERS, _lib.RAMP_LOCALIZE_CONVERGED, _lib.RAMP_LOCALIZE_STALLED, _lib.RAMP_LOCALIZE_SINGULAR,
            _lib.RAMP_LOCALIZE_FEW, _lib.RAMP_LOCALIZE_BUDGET, _lib.RAMP_LOCALIZE_REJECTS) == (lr.ITERS, lr.CONVERGED, lr.STALLED,
                                                                                               lr.SINGULAR, lr.FEW, lr.BUDGET, lr.REJECTS)
    L = _lib.lib()
    up = lambda v: (v + 255) // 256 * 256
    for h, w in ((1, 1), (13, 17), (480, 640), (1, (1 << 31) - 1)):
        assert L.ramp_time_surface_ws_bytes(h, w) == up(8 * h * w) + up(4 * h * w)
    for h, w in ((0, 17), (13, -1), (1 << 16, 1 << 15)):
        assert L.ramp_time_surface_ws_bytes(h, w) == 0
    slots = L.ramp_point_map_localize_grid_slots()
    assert slots > 0 and slots % 256 == 0
    fixed = L.ramp_point_map_localize_ws_bytes(8, 0)
    assert fixed >= slots // 256 * 32 * 8 and fixed % 256 == 0
    assert all(L.ramp_point_map_localize_ws_bytes(c, i) == fixed for c, i in ((1 << 13, 10), (1 << 30, _lib.RAMP_LOCALIZE_MAX_ITERS)))
    assert all(L.ramp_point_map_localize_ws_bytes(c, i) == 0 for c, i in ((12, 1), (4, 1), (8, -1), (8, _lib.RAMP_LOCALIZE_MAX_ITERS + 1)))
    # refusals that need no device: the argument checks come before anything is launched
    words = (ctypes.c_int32 * 512)()
    p = (ctypes.addressof(words) + 255) // 256 * 256
    ts = lambda **o: L.ramp_time_surface(*{**dict(x=p, y=p, t=p, N=4, last=None, t_ref=1.0, tau=0.1, H=4, W=4, smooth=2, flags=1, surface=p,
                                                  raw=None, last_out=None, ws=p, nbytes=1 << 20, status=p, stream=None), **o}.values())
    for o in (dict(N=-1), dict(H=0), dict(W=0), dict(smooth=-1), dict(smooth=9), dict(flags=2), dict(surface=None), dict(status=None),
              dict(ws=None), dict(x=None), dict(t=None), dict(ws=p + 64), dict(t=p + 4), dict(last=p + 4), dict(surface=p + 2)):
        assert ts(**o) == _lib.RAMP_EINVAL, o
    assert ts(H=1 << 16, W=1 << 15) == _lib.RAMP_EUNSUPPORTED
    assert ts(nbytes=L.ramp_time_surface_ws_bytes(4, 4) - 1) == _lib.RAMP_EWORKSPACE
    base = dict(map=p, cap=8, voxel=0.1, mp=1, mv=1, cam=p, K=p, surface=p, H=4, W=4, huber=0.0)
    ev = lambda **o: L.ramp_point_map_localize_eval(*{**base, **dict(sums=p, rec=None, ws=p, nbytes=1 << 20, status=p, stream=None), **o}.values())
    lo = lambda **o: L.ramp_point_map_localize(*{**base, **dict(lambda0=1e-3, min_step=1e-6, iters=3, max_evals=0, pose=p, pose32=p, result=p,
                                                                hessian=p, gradient=p, history=p, status=p, info=p, ws=p, nbytes=1 << 20,
                                                                stream=None), **o}.values())
    shared = (dict(H=1), dict(W=1), dict(cap=12), dict(cap=4), dict(cap=1 << 31), dict(voxel=0.0), dict(voxel=float("nan")),
              dict(voxel=float("inf")), dict(mp=-1), dict(mv=-1), dict(map=None), dict(cam=None), dict(K=None), dict(surface=None),
              dict(ws=None), dict(status=None), dict(map=p + 8), dict(ws=p + 64), dict(huber=float("nan")))
    for o in shared + (dict(sums=None), dict(sums=p + 4)):
        assert ev(**o) == _lib.RAMP_EINVAL, o
    for o in shared + (dict(iters=-1), dict(iters=_lib.RAMP_LOCALIZE_MAX_ITERS + 1), dict(lambda0=-1.0), dict(lambda0=float("nan")),
                       dict(min_step=float("inf")), dict(pose=None), dict(pose32=None), dict(result=None), dict(hessian=None),
                       dict(gradient=None), dict(history=None), dict(info=None), dict(pose=p + 4)):
        assert lo(**o) == _lib.RAMP_EINVAL, o
    for call in (ev, lo):
        assert call(H=1 << 16, W=1 << 15) == _lib.RAMP_EUNSUPPORTED and call(nbytes=fixed - 1) == _lib.RAMP_EWORKSPACE
    assert all(v == 0 for v in words), "a refused call touches nothing"
    assert all(callable(f) for f in (ops.time_surface, ops.time_surface_status, ops.PointMap.localize_eval, ops.PointMap.localize,
                                     ops.point_map_localize_status, ops.point_map_localize_info, TrackerQueries.event_map_localize))


def test_the_status_decoders_and_the_table():
    from rampvo_amd import ops
    bits_, names = ops._STATUS["point_map_localize"]
    assert names == ("n_occupied", "n_filtered", "n_rejected", "n_out_of_reach", "n_in_reach")
    assert bits_["bad_camera"] is ops._STATUS["depth_points"][0]["bad_camera"]          # one row: the same bit, the same text
    assert ops.point_map_localize_status(torch.tensor([1, 9, 1, 2, 3, 3, 0, 0], dtype=torch.int32)) == dict(
        bad_camera=True, n_occupied=9, n_filtered=1, n_rejected=2, n_out_of_reach=3, n_in_reach=3)
    assert ops.time_surface_status(torch.tensor([1, 9, 1, 2, 3, 3, 5, 0], dtype=torch.int32)) == dict(
        bad_args=True, n_events=9, n_not_finite=1, n_outside=2, n_late=3, n_used=3, n_pixels=5)
    assert ops.point_map_localize_info(torch.tensor([lr.FEW, 0, 1, 0, 1, 0, 0, 0], dtype=torch.int32)) == dict(
        reason="few", n_accepted=0, n_evals=1, rejects=0, seen=1, bad_camera=True)
    assert set(ops.LOCALIZE_REASONS.values()) == set(lr.REASONS.values())
    # the roles and the raise order are as they were: the new entries raise through the existing roles only
    assert ops.STATUS_ROLES == {"traj": "trajectory", "interp": "se3_interp", "cam": "invdepth_map", "voxel": "event_voxel",
                                "rectify": "event_rectify", "filter": "event_filter", "imu": "imu", "propagate": "imu_propagate",
                                "dsi": "event_dsi", "depth_points": "depth_points"}
    assert len(ops.STATUS_ORDER) == 16 and ops.STATUS_ORDER[-1] == ("depth_points", "bad_camera")
    assert "point_map_localize" not in ops.STATUS_ROLES.values() and "time_surface" not in ops.STATUS_ROLES.values()


def test_ops_refusals_need_no_gpu():
    from rampvo_amd import ops
    from rampvo_amd.queries import TrackerQueries
    m = ops.PointMap.__new__(ops.PointMap)                    # (the constructor allocates on the device)
    m.voxel, m.capacity, m.device = 0.25, 8, torch.device("cuda")
    S, cam, Kc = torch.ones(13, 17), torch.zeros(7), [16, 12, 8.5, 6.25]
    for fn in (m.localize_eval, m.localize):
        for kw, text in ((dict(surface=torch.ones(1, 17)), "2 x 2"), (dict(surface=torch.ones(17)), "2 x 2"), (dict(min_points=-1), "not negative"),
                         (dict(min_views=-1), "not negative"), (dict(cam=torch.zeros(6)), "7 numbers"), (dict(huber=float("nan")), "huber"),
                         (dict(), "GPU only")):
            with pytest.raises(RuntimeError, match=text):
                fn(**{**dict(surface=S, cam=cam, intrinsics=Kc), **kw})
    x = torch.zeros(4)
    for kw, text in ((dict(height=0), "at least one pixel"), (dict(smooth=9), "smooth is 0 .. 8"), (dict(smooth=-1), "smooth is 0 .. 8"),
                     (dict(height=1 << 16, width=1 << 15), "fewer than 2\\^31"), (dict(), "GPU only")):
        with pytest.raises(RuntimeError, match=text):
            ops.time_surface(**{**dict(x=x, y=x, t=x.double(), t_ref=1.0, tau=0.1, height=13, width=17), **kw})
    with pytest.raises(RuntimeError, match="no event map yet"):
        TrackerQueries().event_map_localize(x, x, x)


def test_the_host_log_inverts_the_exponential():
    """queries._se3_log_between(a, b) = Log(a^-1 b): xi back from a Exp(xi), small angles, angles near pi and a NaN pose"""
    from rampvo_amd.queries import _se3_log_between

    def exp64(xi):                                            # Rodrigues and V in float64, independent of the code under test
        v, w = np.asarray(xi[:3], np.float64), np.asarray(xi[3:], np.float64)
        th = np.linalg.norm(w)
        Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        A, B = (0.5 - th ** 2 / 24, 1 / 6 - th ** 2 / 120) if th < 1e-5 else ((1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3)
        q = np.r_[w * (0.5 - th ** 2 / 48 if th < 1e-5 else np.sin(th / 2) / th), np.cos(th / 2)]
        return np.r_[(np.eye(3) + A * Wx + B * Wx @ Wx) @ v, q]

    def compose(a, b):                                        # a b as (t, q)
        qa, qb = a[3:], b[3:]
        return np.r_[a[:3] + poseref.qrot(qa, b[None, :3])[0], poseref.qmul(qa, qb)]

    a = np.array([0.3, -0.2, 0.5, 0.18257419, -0.36514837, 0.54772256, 0.73029674])
    a[3:] /= np.linalg.norm(a[3:])
    axis = np.array([0.6, -0.48, 0.64])
    for scale in (0.0, 1e-9, 1e-6, 1e-3, 0.3, 2.0, np.pi - 1e-3, np.pi - 1e-7):
        xi = np.r_[[0.4, -0.1, 0.25], scale * axis]
        for base in (np.array([0, 0, 0, 0, 0, 0, 1.0]), a):
            got = _se3_log_between(base, compose(base, exp64(xi)))
            assert np.abs(got - xi).max() <= 1e-9 * max(1.0, scale) + (1e-6 if scale > 3.1415 else 0), (scale, got, xi)
    flipped = compose(a, exp64(np.r_[[0.4, -0.1, 0.25], 0.3 * axis]))
    flipped[3:] *= -1                                         # q and -q are one rotation
    assert np.abs(_se3_log_between(a, flipped) - np.r_[[0.4, -0.1, 0.25], 0.3 * axis]).max() <= 1e-9
    xi32 = np.float32([0.3, -0.2, 0.1, 0.2, -0.1, 0.15])     # and against the project's own exponential (float32)
    assert np.abs(_se3_log_between([0, 0, 0, 0, 0, 0, 1], scenes.se3_exp_np(xi32)) - xi32).max() <= 2e-6
    assert np.isnan(_se3_log_between(np.full(7, np.nan), a)).all() and np.isnan(_se3_log_between(a, np.full(7, np.nan))).all()
