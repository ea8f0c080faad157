"""Motion-compensated events on the GPU: ``ramp_event_warp`` (csrc/warp.hip) through ``ops.event_warp``, the float path of
``ops.event_stack`` and ``Ramp_vo.compensate_events``.

Coordinates are compared per event with the float64 restatement (tests/warpref.py ``compare``): the bound is
``georef.bound(PIXEL_FLOOR x largest |coordinate|, env)`` with env = the float32 restatement's own error against float64 on
the same inputs.  The splat is compared BIT FOR BIT with the exact emulator (``warpref.scatter``) applied to the kernel's
own ``xy``.  Images are 12 x 20 (not square), intrinsics (16, 12, 9.5, 6.25).

The tracker test runs the small synthetic tracker of tests/trackerkit.py, device resident and publishing pose records."""
import ctypes

import numpy as np
import pytest
import torch

import georef
import interpref
import trackerkit as kit
import warpref
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = 12, 20
K = np.array([16.0, 12.0, 9.5, 6.25], np.float32)


def _events(seed, n, t_lo, t_hi, margin=0.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-margin, W - 1 + margin, n).astype(np.float32), rng.uniform(-margin, H - 1 + margin, n).astype(np.float32),
            rng.uniform(t_lo, t_hi, n), rng.choice([-1, 1], n).astype(np.int8))


def _warp(x, y, t, p, knots, times, t_ref, invdepth, bins=0, stack=None, extrapolate=False, want_iwe=True, Kc=K):
    from rampvo_amd import ops
    d = cu(np.asarray(invdepth, np.float32)) if np.ndim(invdepth) == 2 else float(invdepth)
    r = ops.event_warp(cu(x), cu(y), cu(np.asarray(t, np.float64)), cu(p), cu(np.asarray(knots, np.float32)),
                       cu(np.asarray(times, np.float64)), t_ref, cu(Kc), d, H, W, num_bins=bins, extrapolate=extrapolate,
                       want_xy=True, want_iwe=want_iwe, stack=stack)
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check_splat(r, p, bins=0, stack=None, index=None):
    """iwe / stack of one call equal the emulator on the call's own xy, and the counters the emulator's"""
    s = warpref.scatter(r["xy"], p, H, W, bins=bins if stack else 0, index=index)
    if "iwe" in r:
        assert georef.same_bits(r["iwe"], warpref.finish_f32(s["iwe"]))
    if stack == "f32":
        assert georef.same_bits(r["stack"], warpref.finish_f32(s["stack"]))
    if stack == "i8":
        assert np.array_equal(r["stack"], warpref.finish_i8(s["stack"]))
    assert r["status"][5] == s["n_outside"] and r["status"][6] == s["n_contributed"] and r["status"][7] == 0
    assert r["status"][3:7].sum() == len(p)
    return s


# ------------------------------------------------------------------------------------------------ 1. float64, per event
def test_coordinates_against_float64():
    """walk scenes and pair scenes on both sides of LT_EPS, a segment of zero length, both depth modes, inside and outside
    the knots' range with and without extrapolation: (measured, envelope, bound) printed per scene"""
    tab = georef.Table("event_warp: warped coordinates against float64 (pixels)")
    dm = (0.2 + 0.003 * np.arange(H * W, dtype=np.float32)).reshape(H, W)      # a distinct value per pixel
    cases = []
    for T in (2, 5):
        knots, times = interpref.walk_scene(20 + T, T)
        cases.append(("walk T=%d scalar" % T, knots, times, 0.5 * times[-1], 0.5, False, (-0.5, times[-1] + 0.5)))
        cases.append(("walk T=%d map extrap" % T, knots, times, 0.25 * times[-1], dm, True, (-0.5, times[-1] + 0.5)))
    for angle in (1e-7, 1e-3, 1.0):
        knots, times = interpref.pair_scene(40, 3, angle, 0.1)
        cases.append(("pair angle %g" % angle, knots, times, 0.5, 0.8, False, (0.0, 1.0)))
        cases.append(("pair angle %g d=0" % angle, knots, times, 2.5, 0.0, False, (2.0, 3.0)))
    knots, times = interpref.walk_scene(50, 5)
    times = np.array([0.0, 1.0, 1.0, 2.0, 3.0])
    cases.append(("zero-length segment", knots, times, 1.0, dm, False, (0.0, 3.0)))
    ok = True
    for name, knots, times, t_ref, d, ex, (lo, hi) in cases:
        x, y, t, p = _events(len(name), 257, lo, hi)
        t[:4] = [times[0], times[-1], times[len(times) // 2], t_ref]
        r = _warp(x, y, t, p, knots, times, t_ref, d, extrapolate=ex)
        c = warpref.compare(r["xy"], x, y, t, knots, times, t_ref, K, d, H, W, extrapolate=ex)
        ok &= tab.add(name, c["err"], c["env"], c["floor"]) and c["nan_ok"] and c["n_valid"] >= 64
        assert c["nan_ok"], name
        assert r["status"][0] == 0 and r["status"][1] == (t < times[0]).sum() and r["status"][2] == (t > times[-1]).sum()
        _check_splat(r, p)
    tab.show()
    assert ok and not tab.failed(), tab.failed()


# ------------------------------------------------------------------------------------------------ 2. the splat, bit for bit
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("bins", [1, 5])
def test_splat_bits(N, bins):
    knots, times = interpref.walk_scene(3, 5)
    x, y, t, p = _events(N + bins, N, 0.0, 4.0, margin=2.0)
    for stack in ("f32", "i8"):
        r = _warp(x, y, t, p, knots, times, 2.0, 0.4, bins=bins, stack=stack)
        _check_splat(r, p, bins, stack)


@pytest.mark.parametrize("T", [1, 2, 5, "lds+1"])
def test_knot_counts(T):
    from rampvo_amd import _lib
    T = _lib.lib().ramp_se3_interp_lds_knots() + 1 if T == "lds+1" else T
    knots, times = interpref.walk_scene(4, T, step=(0.002,) * 6) if T > 5 else interpref.walk_scene(4, T)
    x, y, t, p = _events(T, 257, -1.0, times[-1] + 1.0)
    r = _warp(x, y, t, p, knots, times, 0.5 * times[-1], 0.5, bins=5, stack="i8")
    c = warpref.compare(r["xy"], x, y, t, knots, times, 0.5 * times[-1], K, 0.5, H, W)
    print("T=%d: err %.2e env %.2e bound %.2e" % (T, c["err"], c["env"], c["bound"]))
    assert c["ok"], c
    _check_splat(r, p, 5, "i8")


def test_second_trip_of_the_grid_and_unaligned_arrays():
    """one event more than a full grid covers in one trip; the same events from arrays that are not 16-byte aligned (the
    scalar staging path) give the same bits"""
    from rampvo_amd import _lib, ops
    N = _lib.lib().ramp_event_warp_grid_events() + 1
    knots, times = interpref.walk_scene(5, 5)
    x, y, t, p = _events(6, N + 1, 0.0, 4.0, margin=1.0)
    r = _warp(x[1:], y[1:], t[1:], p[1:], knots, times, 2.0, 0.4, bins=5, stack="f32")
    _check_splat(r, p[1:], 5, "f32")
    xs, ys, ts, ps = cu(x)[1:], cu(y)[1:], cu(t)[1:], cu(p)[1:]
    assert xs.data_ptr() % 16 and xs.is_contiguous()
    q = ops.event_warp(xs, ys, ts, ps, cu(knots), cu(times), 2.0, cu(K), 0.4, H, W, num_bins=5, want_xy=True, stack="f32")
    for k in ("xy", "iwe", "stack", "status"):
        assert georef.same_bits(q[k].cpu().numpy(), r[k]), k


def test_order_of_the_events_does_not_matter():
    knots, times = interpref.walk_scene(7, 5)
    x, y, t, p = _events(8, 4099, 0.0, 4.0, margin=1.0)
    a = _warp(x, y, t, p, knots, times, 2.0, 0.4, bins=1, stack="f32")
    perm = np.random.default_rng(9).permutation(len(x))
    b = _warp(x[perm], y[perm], t[perm], p[perm], knots, times, 2.0, 0.4, bins=1, stack="f32")
    assert georef.same_bits(a["xy"][perm], b["xy"])
    for k in ("iwe", "stack", "status"):
        assert georef.same_bits(a[k], b[k]), k
    c = _warp(x, y, t, p, knots, times, 2.0, 0.4, bins=1, stack="f32")      # and a call repeats its bits
    assert georef.same_bits(a["iwe"], c["iwe"]) and georef.same_bits(a["stack"], c["stack"])


# ------------------------------------------------------------------------------------------------ 3. identity
def test_identity_equals_the_integer_event_stack():
    """integer-valued float coordinates, one knot (C(t) = C(t_ref) in every bit: G is the exact identity) and intrinsics
    whose round trip (x - cx) / fx * fx + cx is exact (powers of two): stack_i8 equals ops.event_stack of the integer
    coordinates, 140 events on one pixel included (the int8 wraps); so does the float path of ops.event_stack"""
    from rampvo_amd import ops
    rng = np.random.default_rng(10)
    N = 700
    xi, yi = rng.integers(-1, W + 1, N), rng.integers(-1, H + 1, N)
    p = rng.choice([-1, 1], N).astype(np.int8)
    xi[:140], yi[:140], p[:140] = 7, 5, 1
    xi[140:280], yi[140:280], p[140:280] = 8, 5, -1
    ref = ops.event_stack(cu(xi), cu(yi), cu(p), H, W, num_bins=5, as_float=False).cpu().numpy()
    assert ref.min() < -100 and ref.max() > 100                 # (140 and -140 wrapped to -116 and 116)
    knots = interpref.rand_pose(np.random.default_rng(11), 1).astype(np.float32)
    Kp = np.array([16.0, 8.0, 10.0, 6.0], np.float32)
    r = _warp(xi.astype(np.float32), yi.astype(np.float32), rng.uniform(-1, 1, N), p, knots, [0.0], 0.25, 0.0, bins=5,
              stack="i8", Kc=Kp)
    assert np.array_equal(r["xy"], np.stack([xi, yi], -1).astype(np.float32))
    assert np.array_equal(r["stack"], ref)
    f = ops.event_stack(cu(xi.astype(np.float32)), cu(yi.astype(np.float32)), cu(p), H, W, num_bins=5, as_float=False)
    assert np.array_equal(f.cpu().numpy(), ref)
    # fractional coordinates through the float path: the emulator's bits
    x, y, _, _ = _events(12, N, 0, 1, margin=1.5)
    f = ops.event_stack(cu(x), cu(y), cu(p), H, W, num_bins=5, as_float=False).cpu().numpy()
    assert np.array_equal(f, warpref.finish_i8(warpref.scatter(np.stack([x, y], -1), p, H, W, bins=5)["stack"]))


# ------------------------------------------------------------------------------------------------ 4. edges
def test_neighbours_outside_the_image_and_the_z_test():
    Kp = np.array([16.0, 8.0, 10.0, 6.0], np.float32)
    knots = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    x = np.array([W - 0.5, 4.0, -1.5, 3.25], np.float32)
    y = np.array([3.0, -0.25, 3.0, 4.5], np.float32)
    p = np.array([1, -1, 1, -1], np.int8)
    r = _warp(x, y, np.zeros(4), p, knots, [0.0], 0.0, 0.0, Kc=Kp)
    assert np.array_equal(r["xy"], np.stack([x, y], -1))
    assert r["status"].tolist() == [0, 0, 0, 0, 0, 1, 3, 0]
    assert r["iwe"][1, 3, W - 1] == 0.5 and r["iwe"][0, 0, 4] == -0.75 and r["iwe"][1].sum() == 0.5 + 0.75 + 1.0
    _check_splat(r, p)
    # the camera moves forward by 1: Z' = 1 - d; d = 0.9 fails the test (Z' = 0.1 <= 0.2), d = 0.5 passes
    knots = np.array([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1.0, 0, 0, 0, 1]], np.float32)
    dm = np.full((H, W), 0.5, np.float32)
    dm[4, 3] = 0.9
    r = _warp(x[3:], y[3:] - 0.25, [1.0], p[3:], knots, [0.0, 1.0], 0.0, dm)
    assert np.isnan(r["xy"]).all() and r["status"].tolist() == [0, 0, 0, 0, 1, 0, 0, 0] and not r["iwe"].any()
    r = _warp(x[3:] + 1, y[3:] - 0.25, [1.0], p[3:], knots, [0.0, 1.0], 0.0, dm)
    assert np.isfinite(r["xy"]).all() and r["status"][4] == 0


@pytest.mark.parametrize("col", [0, 1, 2])
def test_an_event_that_is_not_finite(col):
    """NaN row, counted, and the other events' outputs are those of a call without that event"""
    knots, times = interpref.walk_scene(13, 5)
    x, y, t, p = _events(14, 130, 0.0, 4.0)
    a = [x.copy(), y.copy(), t.copy()]
    a[col][77] = [np.nan, np.inf, -np.inf][col]
    r = _warp(a[0], a[1], a[2], p, knots, times, 2.0, 0.4, bins=1, stack="f32")
    keep = np.arange(130) != 77
    q = _warp(x[keep], y[keep], t[keep], p[keep], knots, times, 2.0, 0.4, bins=1, stack="f32")
    assert np.isnan(r["xy"][77]).all() and r["status"][3] == 1 and q["status"][3] == 0
    assert georef.same_bits(r["xy"][keep], q["xy"])
    assert georef.same_bits(r["iwe"], q["iwe"]) and georef.same_bits(r["stack"], q["stack"])


def test_decreasing_times():
    knots, times = interpref.walk_scene(15, 5)
    x, y, t, p = _events(16, 65, -1.0, 5.0)
    x[3] = np.nan
    for stack in ("f32", "i8"):
        r = _warp(x, y, t, p, knots, times[::-1].copy(), 2.0, 0.4, bins=5, stack=stack)
        assert r["status"][0] == 1 and r["status"][3] == 1 and r["status"][4:].sum() == 0
        assert np.isnan(r["xy"]).all() and np.isnan(r["iwe"]).all()
        assert np.isnan(r["stack"]).all() if stack == "f32" else not r["stack"].any()


def test_extrapolation_outside_the_range():
    knots, times = interpref.walk_scene(17, 3)
    x, y, t, p = _events(18, 64, -1.0, 3.0)
    t[:32] = np.where(t[:32] < 1.0, t[:32] - 1.5, t[:32] + 1.5)      # half of them outside [0, 2]
    held = _warp(x, y, t, p, knots, times, 1.0, 0.3)
    moved = _warp(x, y, t, p, knots, times, 1.0, 0.3, extrapolate=True)
    for r, ex in ((held, False), (moved, True)):
        c = warpref.compare(r["xy"], x, y, t, knots, times, 1.0, K, 0.3, H, W, extrapolate=ex)
        assert c["ok"], c
        assert r["status"][1] == (t < 0).sum() and r["status"][2] == (t > 2).sum()
    out = (t < 0) | (t > 2)
    assert georef.same_bits(held["xy"][~out], moved["xy"][~out]) and not georef.same_bits(held["xy"][out], moved["xy"][out])


def test_arguments_and_canaries():
    """the C entry with guard words on both sides of every output and of the workspace; N == 0 launches and writes nothing;
    T < 1, H / W / bins < 1, no output, a t_ref that is not finite: RAMP_EINVAL; a short workspace: RAMP_EWORKSPACE"""
    from rampvo_amd import _lib
    L = _lib.lib()
    N, T, bins = 300, 5, 5
    knots, times = interpref.walk_scene(19, T)
    x, y, t, p = _events(20, N, -1.0, 5.0, margin=2.0)
    dx, dy, dt, dp, dk, dtm, dK = cu(x), cu(y), cu(t), cu(p), cu(knots), cu(times), cu(K)
    dd = torch.full((1,), 0.4, device="cuda")
    nbytes = L.ramp_event_warp_workspace_bytes(T, bins, H, W)
    assert nbytes % 8 == 0

    bufs = dict(xy=Flat(2 * N, torch.float32, -7.0), iwe=Flat(2 * H * W, torch.float32, -7.0),
                sf=Flat(bins * H * W, torch.float32, -7.0), s8=Flat(bins * H * W, torch.int8, 99),
                status=Flat(8, torch.int32, -7), ws=Flat(nbytes, torch.uint8, 0xA5))
    assert bufs["ws"].t.data_ptr() % 16 == 0

    def call(N=N, T=T, bins=bins, H_=H, W_=W, t_ref=2.0, outs=("xy", "iwe", "sf", "s8"), ws_bytes=nbytes, pol=dp, xy_off=0):
        o = lambda k: _lib.ptr(bufs[k].t) if k in outs else None
        xy_p = ctypes.c_void_p(bufs["xy"].t.data_ptr() + xy_off) if "xy" in outs else None
        rc = L.ramp_event_warp(_lib.ptr(dx), _lib.ptr(dy), _lib.ptr(dt), _lib.ptr(pol), N, _lib.ptr(dk), _lib.ptr(dtm), T, t_ref,
                               _lib.ptr(dK), _lib.ptr(dd), 0, bins, H_, W_, xy_p, o("iwe"), o("sf"), o("s8"),
                               _lib.ptr(bufs["ws"].t), ws_bytes, _lib.ptr(bufs["status"].t), _lib.stream())
        torch.cuda.synchronize()
        return rc

    before = {k: v.snapshot() for k, v in bufs.items()}
    assert call(N=0) == 0
    assert all(bufs[k].unchanged(before[k]) for k in bufs)                 # nothing written, status included
    for kw in (dict(T=0), dict(H_=0), dict(W_=0), dict(bins=0), dict(outs=()), dict(t_ref=float("nan")), dict(N=-1),
               dict(xy_off=4)):                                              # (xy_out rows are stored as float2)
        assert call(**kw) == -1, kw
    assert call(ws_bytes=nbytes - 8) == -3
    assert all(bufs[k].unchanged(before[k]) for k in bufs)
    assert call() == 0
    for k, b in bufs.items():
        assert b.intact(), k
    r = dict(xy=bufs["xy"].t.view(N, 2).cpu().numpy(), iwe=bufs["iwe"].t.view(2, H, W).cpu().numpy(),
             stack=bufs["sf"].t.view(bins, H, W).cpu().numpy(), status=bufs["status"].t.cpu().numpy())
    _check_splat(r, p, bins, "f32")
    r["stack"] = bufs["s8"].t.view(bins, H, W).cpu().numpy()
    _check_splat(r, p, bins, "i8")
    assert warpref.compare(r["xy"], x, y, t, knots, times, 2.0, K, 0.4, H, W)["ok"]
    # a polarity of 0 is read as -1 by the C entry itself
    p0 = p.copy()
    p0[p == -1] = 0
    assert (p0 == 0).sum() > 50 and call(pol=cu(p0)) == 0
    assert georef.same_bits(bufs["iwe"].t.view(2, H, W).cpu().numpy(), r["iwe"])
    assert np.array_equal(bufs["s8"].t.view(bins, H, W).cpu().numpy(), r["stack"])


# ------------------------------------------------------------------------------------------------ 5. tracker
@torch.no_grad()
def _run(query):
    from rampvo_amd import ops
    slam = kit.tracker(True, True)
    slam.pose_stream()
    res = {}
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        Kf = frame[2]
        if f == kit.T_QUERY and query:
            assert kit.resident(slam)
            x, y, t, p = kit.query_events(f)
            t[:100] = kit.tstamp(f)                                              # at the reference time: G is the identity
            out = slam.compensate_events(x, y, t, p, num_bins=3, stack="i8", want_xy=True, as_tensor=True)
            res["numpy"] = slam.compensate_events(x, y, t, p, num_bins=3, stack="i8", want_xy=True)
            res["resident_after"] = kit.resident(slam)
            # the same from the parts: poses_at's knots, the fed intrinsics, the median the next frame's patches start from
            knots, ts = slam.trajectory(as_tensor=True)
            n = slam.peek()["n"]
            med = torch.median(slam.patches_[n - 3:n, :, 2])
            ref = ops.event_warp(x, y, t, p, knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), Kf.cuda().float(), med, 240, 320,
                                 num_bins=3, want_xy=True, stack="i8")
            res["out"] = {k: v.cpu().numpy() for k, v in out.items()}
            res["xy_in"] = np.stack([x.cpu().numpy(), y.cpu().numpy()], -1)
            res["ref"] = {k: v.cpu().numpy() for k, v in ref.items()}
            res["med"] = float(med)
            res["still_resident"] = kit.resident(slam)
    n = slam.peek()["n"]
    res["final_resident"] = kit.resident(slam)
    res["poses"] = slam.poses_[:n].cpu().numpy()
    del slam
    kit.quiesce()
    return res


def test_tracker_compensate_events():
    """compensate_events equals ops.event_warp fed by trajectory()'s knots, the fed intrinsics and the tracker's own depth
    median; the tracker stays device resident and the frames behind the call give the poses of a run without it"""
    a, b = _run(True), _run(False)
    assert a["resident_after"] and a["still_resident"] and a["final_resident"] and b["final_resident"]
    assert a["med"] > 0
    for k in ("xy", "iwe", "stack", "status"):
        assert georef.same_bits(a["out"][k], a["ref"][k]), k
        assert isinstance(a["numpy"][k], np.ndarray) and georef.same_bits(a["numpy"][k], a["out"][k]), k      # as_tensor=False
    st = a["out"]["status"]
    assert st[0] == 0 and st[3] == 0 and st[6] >= 100 and st[3:7].sum() == 5000
    assert np.abs(a["out"]["xy"][:100] - a["xy_in"][:100]).max() < 1e-3     # (up to the unproject / project round trip)
    assert georef.same_bits(a["poses"], b["poses"])


@torch.no_grad()
def test_tracker_compensate_events_host_driven():
    """a host-driven tracker (no device-resident step): the numpy form of compensate_events equals ops.event_warp fed by
    trajectory()'s knots and the median of the last three keyframes' patches (ops.depth_median with the host's row count);
    frame time stamps that decrease make it raise"""
    from rampvo_amd import ops
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    Kf = frame[2]
    assert slam.is_initialized and slam._dev is None and f < kit.T_FRAMES - 1
    rng = np.random.default_rng(22)
    n_ev = 1000
    x, y = rng.uniform(0, 319, n_ev).astype(np.float32), rng.uniform(0, 239, n_ev).astype(np.float32)
    t = rng.uniform(100.0 + 0.5 * (f - 2), 100.0 + 0.5 * f, n_ev)
    p = rng.choice([-1, 1], n_ev).astype(np.int8)
    out = slam.compensate_events(x, y, t, p, want_xy=True)                      # numpy in, numpy out
    knots, ts = slam.trajectory(as_tensor=True)
    n = slam._n
    med = torch.median(slam.patches_[n - 3:n, :, 2])
    ref = ops.event_warp(cu(x), cu(y), cu(t), cu(p), knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), Kf.cuda().float(), med,
                         240, 320, want_xy=True)
    assert float(med) > 0 and sorted(out) == ["iwe", "status", "xy"]
    for k in out:
        assert isinstance(out[k], np.ndarray) and georef.same_bits(out[k], ref[k].cpu().numpy()), k
    assert out["status"][0] == 0 and out["status"][3:7].sum() == n_ev
    slam.tlist = slam.tlist[::-1]
    with pytest.raises(RuntimeError, match="time stamps decrease"):
        slam.compensate_events(x, y, t, p)
    del slam
    kit.quiesce()


# ------------------------------------------------------------------------------------------------ 6. the small entries
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5])
def test_depth_median_rows(n):
    """the median of rows n - 3 .. n - 1 with n read on the device; fewer than three rows: those there are; none: 0"""
    from rampvo_amd import ops
    rng = np.random.default_rng(30 + n)
    patches = cu(rng.uniform(0.1, 2.0, (6, 7, 3, 3, 3)).astype(np.float32))
    words = torch.tensor([99, n, 99], dtype=torch.int32, device="cuda")
    out = torch.full((3,), -7.0, device="cuda")
    ops.depth_median_rows(patches, words[1:], 3, out[1:])
    want = float(torch.median(patches[max(n - 3, 0):n, :, 2])) if n else 0.0
    assert out.cpu().tolist() == [-7.0, want, -7.0]


def test_event_warp_status():
    from rampvo_amd import ops
    knots, times = interpref.walk_scene(31, 3)
    x, y, t, p = _events(32, 65, -1.0, 3.0, margin=3.0)
    x[5] = np.nan
    r = ops.event_warp(cu(x), cu(y), cu(t), cu(p), cu(knots), cu(times), 1.0, cu(K), 0.3, H, W)
    s, w = ops.event_warp_status(r["status"]), r["status"].cpu().numpy()
    assert s == dict(bad_times=False, n_below=int((t < 0).sum()) - int(t[5] < 0), n_above=int((t > 2).sum()) - int(t[5] > 2),
                     n_not_finite=1, n_rejected=int(w[4]), n_outside=int(w[5]), n_contributed=int(w[6]))
    assert s["n_not_finite"] + s["n_rejected"] + s["n_outside"] + s["n_contributed"] == 65
    r = ops.event_warp(cu(x), cu(y), cu(t), cu(p), cu(knots), cu(times[::-1].copy()), 1.0, cu(K), 0.3, H, W)
    assert ops.event_warp_status(r["status"])["bad_times"]
