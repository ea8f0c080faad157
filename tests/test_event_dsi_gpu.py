"""Event multi-view stereo on the GPU: ``ramp_event_dsi`` (csrc/emvs.hip) through ``ops.event_dsi``, ``Ramp_vo.event_depth`` and
``compensate_events(invdepth="events")``.

Coordinates are compared per event and plane with the float64 restatement (tests/dsiref.py ``compare``): the bound is
``georef.bound(PIXEL_FLOOR x largest |coordinate|, env)`` with env = the float32 restatement's own error against float64 on the
same inputs.  The accumulators are compared BIT FOR BIT with the exact emulator (``dsiref.votes``) applied to the kernel's own
``coords``, the detection and the refinement with ``dsiref.detect`` applied to the kernel's own ``dsi``.  Images are 13 x 17 (no
tile divides them), intrinsics (16, 12, 8.5, 6.25).

The tracker tests run the small synthetic tracker of tests/trackerkit.py."""
import ctypes

import numpy as np
import pytest
import torch

import dsiref
import georef
import interpref
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = 13, 17
K = np.array([16.0, 12.0, 8.5, 6.25], np.float32)
RNG = (0.2, 1.4)


def _events(seed, n, t_lo, t_hi, margin=0.0):
    rng = np.random.default_rng(seed)
    return (rng.uniform(-margin, W - 1 + margin, n).astype(np.float32), rng.uniform(-margin, H - 1 + margin, n).astype(np.float32),
            rng.uniform(t_lo, t_hi, n))


def _dsi(x, y, t, knots, times, t_ref, D=16, rng=RNG, h=H, w=W, Kc=K, coords=True, **kw):
    from rampvo_amd import ops
    r = ops.event_dsi(cu(np.asarray(x, np.float32)), cu(np.asarray(y, np.float32)), cu(np.asarray(t, np.float64)),
                      cu(np.asarray(knots, np.float32)), cu(np.asarray(times, np.float64)), t_ref, cu(Kc), h, w, planes=D,
                      range=rng, want_coords=coords, **{"min_votes": 1.0, **kw})
    return {k: v.cpu().numpy() for k, v in r.items()}


def _check(r, rng=RNG, min_votes=1.0, adaptive_radius=0, adaptive_offset=0.0, fill=None):
    """one call against the emulators: dsi from the call's own coords, detection and refinement from its own dsi, the counters"""
    D, h, w = r["dsi"].shape
    v = dsiref.votes(r["coords"], h, w)
    assert np.array_equal(r["dsi"], v["dsi"])
    d = dsiref.detect(r["dsi"], rng, min_votes, adaptive_radius, adaptive_offset, fill)
    assert np.array_equal(r["plane"], d["plane"])
    assert georef.same_bits(r["confidence"], d["confidence"]) and georef.same_bits(r["invdepth"], d["invdepth"])
    st = r["status"]
    assert st[0] == 0 and st[4] == v["n_no_vote"] - st[3] and st[5] == v["n_voted"] and st[6] == d["n_detected"] and st[7] == 0
    assert st[3] + st[4] + st[5] == r["coords"].shape[0]
    return d


# ------------------------------------------------------------------------------------------------ 1. float64, per event and plane
def test_coordinates_against_float64():
    """walk scenes and pair scenes on both sides of LT_EPS, inside and outside the knots' range with and without
    extrapolation, ranges from 0 up: (measured, envelope, bound) printed per scene"""
    tab = georef.Table("event_dsi: projected coordinates against float64 (pixels)")
    cases = []
    for T in (2, 5):
        knots, times = interpref.walk_scene(20 + T, T)
        cases.append(("walk T=%d" % T, knots, times, 0.5 * times[-1], RNG, False, (-0.5, times[-1] + 0.5)))
        cases.append(("walk T=%d extrap d_lo=0" % T, knots, times, 0.25 * times[-1], (0.0, 2.5), True, (-0.5, times[-1] + 0.5)))
    for angle in (1e-7, 1e-3, 1.0):
        knots, times = interpref.pair_scene(40, 3, angle, 0.1)
        cases.append(("pair angle %g" % angle, knots, times, 0.5, (0.1, 3.0), False, (0.0, 1.0)))
    ok = True
    for name, knots, times, t_ref, rng, ex, (lo, hi) in cases:
        x, y, t = _events(len(name), 257, lo, hi)
        t[:4] = [times[0], times[-1], times[len(times) // 2], t_ref]
        r = _dsi(x, y, t, knots, times, t_ref, rng=rng, extrapolate=ex)
        c = dsiref.compare(r["coords"], x, y, t, knots, times, t_ref, K, rng, 16, H, W, extrapolate=ex)
        ok &= tab.add(name, c["err"], c["env"], c["floor"]) and c["nan_ok"] and c["n_valid"] >= 64 * 16
        assert c["nan_ok"], name
        assert r["status"][1] == (t < times[0]).sum() and r["status"][2] == (t > times[-1]).sum()
        _check(r, rng)
    tab.show()
    assert ok and not tab.failed(), tab.failed()


# ------------------------------------------------------------------------------------------------ 2. the accumulators, bit for bit
@pytest.mark.parametrize("N", [0, 1, 2, 4099])
@pytest.mark.parametrize("D", [1, 2, 16, 65])
def test_accumulator_bits(N, D):
    knots, times = interpref.walk_scene(3, 5)
    x, y, t = _events(N + D, N, 0.0, 4.0, margin=2.0)
    r = _dsi(x, y, t, knots, times, 2.0, D=D, rng=(0.2, 0.2 if D == 1 else 1.4))
    assert r["dsi"].shape == (D, H, W) and r["coords"].shape == (N, D, 2)
    d = _check(r, (0.2, 0.2 if D == 1 else 1.4))
    assert (N == 0) == (not r["dsi"].any()) and (N > 0 or (d["n_detected"] == 0 and np.isnan(r["invdepth"]).all()))


def test_second_trip_of_the_grid_and_unaligned_arrays():
    """one event more than a full grid covers in one trip; the same events from arrays that are not 16-byte aligned (the
    scalar staging path) give the same bits"""
    from rampvo_amd import _lib, ops
    N = _lib.lib().ramp_event_dsi_grid_events() + 1
    knots, times = interpref.walk_scene(5, 5)
    x, y, t = _events(6, N + 1, 0.0, 4.0, margin=1.0)
    r = _dsi(x[1:], y[1:], t[1:], knots, times, 2.0, D=2)
    _check(r)
    xs, ys, ts = cu(x)[1:], cu(y)[1:], cu(t)[1:]
    assert xs.data_ptr() % 16 and xs.is_contiguous()
    q = ops.event_dsi(xs, ys, ts, cu(knots), cu(times), 2.0, cu(K), H, W, planes=2, range=RNG, min_votes=1.0)
    for k in ("dsi", "invdepth", "confidence", "plane", "status"):
        assert np.array_equal(q[k].cpu().numpy(), r[k], equal_nan=True), k


def test_order_of_the_events_does_not_matter_and_a_call_repeats_its_bits():
    knots, times = interpref.walk_scene(7, 5)
    x, y, t = _events(8, 4099, 0.0, 4.0, margin=1.0)
    a = _dsi(x, y, t, knots, times, 2.0)
    perm = np.random.default_rng(9).permutation(len(x))
    b = _dsi(x[perm], y[perm], t[perm], knots, times, 2.0)
    c = _dsi(x, y, t, knots, times, 2.0)
    assert georef.same_bits(a["coords"][perm], b["coords"]) and georef.same_bits(a["coords"], c["coords"])
    for k in ("dsi", "invdepth", "confidence", "plane", "status"):
        assert np.array_equal(a[k], b[k], equal_nan=True) and np.array_equal(a[k], c[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------------ 3. detection and refinement
@pytest.mark.parametrize("radius,offset,min_votes", [(0, 0.0, 3.0), (1, 0.5, 3.0), (15, 0.25, 3.0), (1, -0.75, 1.0), (3, -1.0, 1.0)])
def test_detection_and_refinement(radius, offset, min_votes):
    """(with the negative offsets the floor on the votes is low enough for the adaptive threshold to decide)"""
    knots, times = interpref.walk_scene(10, 5)
    x, y, t = _events(11, 600, 0.0, 4.0, margin=1.0)
    x[:180], y[:180] = np.rint(x[:180]), np.rint(y[:180])            # whole pixels: votes of exactly 2^24, thresholds met exactly
    r = _dsi(x, y, t, knots, times, 2.0, min_votes=min_votes, adaptive_radius=radius, adaptive_offset=offset, fill=-1.0)
    d = _check(r, min_votes=min_votes, adaptive_radius=radius, adaptive_offset=offset, fill=-1.0)
    assert 0 < d["n_detected"] < H * W and (r["invdepth"][~d["detected"]] == -1.0).all()
    # invdepth is float32 of the float64 formula, written out once more from the kernel's own dsi
    yy, xx = np.nonzero(d["detected"])
    p = r["plane"][yy, xx]
    step = (float(np.float32(RNG[1])) - float(np.float32(RNG[0]))) / 15
    for i in range(len(p)):
        delta = 0.0
        if 0 < p[i] < 15:
            a, b, c = (int(v) for v in r["dsi"][p[i] - 1:p[i] + 2, yy[i], xx[i]])
            delta = (a - c) / (2.0 * (a - 2 * b + c)) if a - 2 * b + c else 0.0
        assert r["invdepth"][yy[i], xx[i]] == np.float32(float(np.float32(RNG[0])) + (p[i] + delta) * step)


def test_a_tie_goes_to_the_lowest_plane():
    """fx b = 4 pixels and planes 0.25, 0.5, 0.75: event A at t_ref votes pixel (8, 5) in every plane, B (2 pixels to the left,
    at t = 1) meets it in plane 1, C (3 to the left) in plane 2: planes 1 and 2 tie with two votes"""
    Kp = np.array([16.0, 8.0, 8.0, 6.0], np.float32)
    knots = np.array([[0, 0, 0, 0, 0, 0, 1], [0.25, 0, 0, 0, 0, 0, 1]], np.float32)
    r = _dsi([8.0, 6.0, 5.0], [5.0, 5.0, 5.0], [0.0, 1.0, 1.0], knots, [0.0, 1.0], 0.0, D=3, rng=(0.25, 0.75), Kc=Kp, min_votes=2.0)
    assert r["dsi"][:, 5, 8].tolist() == [1 << 24, 2 << 24, 2 << 24]
    assert r["plane"][5, 8] == 1 and r["status"][6] == 1 and r["confidence"][5, 8] == 2.0
    _check(r, (0.25, 0.75), min_votes=2.0)
    # one knot: every plane of every pixel ties: plane 0, no refinement, d_lo
    r = _dsi([8.0, 3.5], [5.0, 2.25], [0.0, 7.0], knots[:1], [0.0], 0.0, D=5, Kc=Kp, min_votes=0.0)
    assert (r["plane"] == 0).all() and georef.same_bits(r["invdepth"], np.full((H, W), RNG[0], np.float32))
    assert (r["dsi"] == r["dsi"][:1]).all() and r["dsi"][0].sum() == 2 << 24


# ------------------------------------------------------------------------------------------------ 4. the whole pipeline
def test_two_plane_scene_end_to_end():
    s = dsiref.TWO_PLANE
    x, y, t, knots, times = dsiref.two_plane_scene()
    r = _dsi(x, y, t, knots, times, s["t_ref"], D=s["D"], rng=s["rng"], h=s["H"], w=s["W"], Kc=s["K"], min_votes=s["min_votes"])
    c = dsiref.two_plane_conditions(r["plane"])
    print("two-plane scene: %d detected, %d on plane 3, %d on plane 10" % (c["n"], c["on_a"], c["on_b"]))
    assert c["all_near"] and c["on_a"] >= 30 and c["on_b"] >= 30, c
    _check(r, s["rng"], min_votes=s["min_votes"])
    d = dsiref.plane_depths(s["rng"], s["D"])[0]
    on = r["plane"] == 3
    assert np.abs(r["invdepth"][on] - d[3]).max() < 0.5 * 0.1        # (refined within half a plane of its own plane)


def test_fill_and_the_map_goes_into_event_warp():
    from rampvo_amd import ops
    knots, times = interpref.walk_scene(12, 5)
    x, y, t = _events(13, 500, 0.0, 4.0)
    nul = _dsi(x, y, t, knots, times, 2.0, min_votes=2.0)
    num = _dsi(x, y, t, knots, times, 2.0, min_votes=2.0, fill=0.625)
    dev = _dsi(x, y, t, knots, times, 2.0, min_votes=2.0, fill=torch.full((1,), 0.625, device="cuda"))
    miss = nul["plane"] < 0
    assert miss.any() and (~miss).any() and np.isnan(nul["invdepth"][miss]).all() and (num["invdepth"][miss] == 0.625).all()
    assert georef.same_bits(num["invdepth"], dev["invdepth"]) and georef.same_bits(num["invdepth"][~miss], nul["invdepth"][~miss])
    p = np.ones(500, np.int8)
    args = (cu(x), cu(y), cu(t), cu(p), cu(knots), cu(times), 2.0, cu(K))
    w = ops.event_warp(*args, cu(num["invdepth"]), H, W, want_xy=True)
    st = w["status"].cpu().numpy()
    assert st[0] == 0 and st[3] == 0 and st[3:7].sum() == 500 and st[6] > 250
    w = ops.event_warp(*args, cu(nul["invdepth"]), H, W, want_xy=True)        # NaN where nothing is detected: rejected, counted
    assert w["status"].cpu().numpy()[4] >= int(miss[np.rint(y).astype(int), np.rint(x).astype(int)].sum())


def test_status_words_and_the_two_bits():
    from rampvo_amd import ops
    knots, times = interpref.walk_scene(14, 3)
    x, y, t = _events(15, 130, -1.0, 3.0, margin=3.0)
    x[5], y[6], t[7] = np.nan, np.inf, -np.inf
    r = _dsi(x, y, t, knots, times, 1.0)
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(t)
    s = ops.event_dsi_status(cu(r["status"]))
    assert s["n_not_finite"] == 3 and s["n_below"] == (fin & (t < 0)).sum() and s["n_above"] == (fin & (t > 2)).sum()
    assert not s["bad_times"] and not s["bad_range"] and s["n_not_finite"] + s["n_no_vote"] + s["n_voted"] == 130
    assert np.isnan(r["coords"][[5, 6, 7]]).all()
    _check(r)
    # the other events' outputs are those of a call without the three
    q = _dsi(x[fin], y[fin], t[fin], knots, times, 1.0)
    assert georef.same_bits(r["coords"][fin], q["coords"]) and np.array_equal(r["dsi"], q["dsi"])
    # either bit: NaN / -1 / zero, [3] + [4] + [5] = N still
    for kw, bits in ((dict(times=times[::-1].copy()), 1), (dict(rng=(0.5, 0.5)), 2), (dict(rng=(-0.1, 1.0)), 2),
                     (dict(rng=(0.1, np.nan)), 2), (dict(rng=(np.inf, 1.0), times=times[::-1].copy()), 3)):
        b = _dsi(x, y, t, knots, kw.get("times", times), 1.0, rng=kw.get("rng", RNG), fill=0.5)
        assert b["status"][0] == bits and b["status"][3] == 3 and b["status"][4] == 127 and b["status"][5:].sum() == 0, kw
        assert np.isnan(b["invdepth"]).all() and np.isnan(b["confidence"]).all() and np.isnan(b["coords"]).all()
        assert (b["plane"] == -1).all() and not b["dsi"].any()
    s = ops.event_dsi_status(cu(b["status"]))
    assert s["bad_times"] and s["bad_range"]
    ok = _dsi(x, y, t, knots, times, 1.0, D=1, rng=(0.5, 0.25))                 # one plane: d_hi is not read against d_lo
    assert ok["status"][0] == 0


def test_a_plane_behind_the_z_test_for_some_events_only():
    """the camera moves forward by 1 between t = 0 and 1: Z' = 1 - d_k for an event at t = 1, so the planes with
    d_k >= 0.8 get no vote from it; an event at t_ref votes in every plane"""
    knots = np.array([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1.0, 0, 0, 0, 1]], np.float32)
    r = _dsi([4.0, 9.0, 9.5], [5.0, 6.0, 3.0], [0.0, 1.0, 1.0], knots, [0.0, 1.0], 0.0, D=8, rng=(0.25, 1.125))
    d = dsiref.plane_depths((0.25, 1.125), 8)[0]
    voted = ~np.isnan(r["coords"]).any(-1)
    assert voted[0].all() and np.array_equal(voted[1], 1.0 - d > 0.2 + 1e-4) and np.array_equal(voted[1], voted[2])
    assert 0 < voted[1].sum() < 8 and r["status"][3:6].tolist() == [0, 0, 3]
    _check(r, (0.25, 1.125))
    r = _dsi([9.0], [6.0], [1.0], knots, [0.0, 1.0], 0.0, D=4, rng=(0.85, 1.125))        # every plane behind: voted in no plane
    assert r["status"][3:7].tolist() == [0, 1, 0, 0] and not r["dsi"].any() and np.isnan(r["coords"]).all()


def test_extrapolation_outside_the_range():
    knots, times = interpref.walk_scene(17, 3)
    x, y, t = _events(18, 64, -1.0, 3.0)
    t[:32] = np.where(t[:32] < 1.0, t[:32] - 1.5, t[:32] + 1.5)      # half of them outside [0, 2]
    held, moved = _dsi(x, y, t, knots, times, 1.0), _dsi(x, y, t, knots, times, 1.0, extrapolate=True)
    for r, ex in ((held, False), (moved, True)):
        c = dsiref.compare(r["coords"], x, y, t, knots, times, 1.0, K, RNG, 16, H, W, extrapolate=ex)
        assert c["ok"], c
        assert r["status"][1] == (t < 0).sum() and r["status"][2] == (t > 2).sum()
        _check(r)
    out = (t < 0) | (t > 2)
    assert georef.same_bits(held["coords"][~out], moved["coords"][~out]) and not georef.same_bits(held["coords"][out], moved["coords"][out])


# ------------------------------------------------------------------------------------------------ 5. refusals and guards
def test_arguments_and_canaries():
    """the C entry with 64 guard rows on both sides of every output and of the workspace, on a side stream; the refusals
    touch nothing; the N * D cap returns its code without a launch (its events do not exist)"""
    from rampvo_amd import _lib
    L = _lib.lib()
    N, T, D = 300, 5, 7
    knots, times = interpref.walk_scene(19, T)
    x, y, t = _events(20, N, -1.0, 5.0, margin=2.0)
    dx, dy, dt, dk, dtm, dK = cu(x), cu(y), cu(t), cu(knots), cu(times), cu(K)
    drng, dfill = cu(np.asarray(RNG, np.float32)), torch.full((1,), 0.5, device="cuda")
    nbytes = L.ramp_event_dsi_ws_bytes(T, H, W)
    bufs = dict(dsi=Flat(D * H * W, torch.int64, rows=W), coords=Flat(N * D * 2, torch.float32, -7.0, rows=2 * D),
                inv=Flat(H * W, torch.float32, -7.0, rows=W), conf=Flat(H * W, torch.float32, -7.0, rows=W),
                plane=Flat(H * W, torch.int32, rows=W), status=Flat(8, torch.int32), ws=Flat(nbytes, torch.uint8, rows=16))
    assert bufs["ws"].t.data_ptr() % 16 == 0 and bufs["dsi"].t.data_ptr() % 8 == 0
    side = torch.cuda.Stream()

    def call(N=N, T=T, D=D, H_=H, W_=W, t_ref=2.0, r=1, min_votes=1.0, offset=0.0, flags=0, ws_bytes=nbytes, ex=dx, dsi_off=0,
             co_off=0, rng=drng):
        o = lambda k, off=0: ctypes.c_void_p(bufs[k].t.data_ptr() + off)
        with torch.cuda.stream(side):
            rc = L.ramp_event_dsi(_lib.ptr(ex), _lib.ptr(dy), _lib.ptr(dt), N, _lib.ptr(dk), _lib.ptr(dtm), T, t_ref, _lib.ptr(dK),
                                  _lib.ptr(rng), flags, D, H_, W_, min_votes, r, offset, _lib.ptr(dfill), o("dsi", dsi_off),
                                  o("coords", co_off), o("inv"), o("conf"), o("plane"), o("ws"), ws_bytes, o("status"),
                                  _lib.stream())
        torch.cuda.synchronize()
        return rc

    torch.cuda.synchronize()
    before = {k: v.snapshot() for k, v in bufs.items()}
    for kw in (dict(N=-1), dict(T=0), dict(H_=0), dict(W_=0), dict(D=0), dict(r=-1), dict(r=16), dict(t_ref=float("nan")),
               dict(min_votes=float("inf")), dict(offset=float("nan")), dict(flags=4), dict(ex=None), dict(rng=None),
               dict(dsi_off=4), dict(co_off=4)):
        assert call(**kw) == _lib.RAMP_EINVAL, kw
    assert call(N=1 << 30, D=1 << 8, H_=1, W_=1) == _lib.RAMP_EUNSUPPORTED          # N * D = 2^38
    assert call(D=1 << 15, H_=1 << 8, W_=1 << 8) == _lib.RAMP_EUNSUPPORTED          # D * H * W = 2^31
    assert call(ws_bytes=nbytes - 16) == _lib.RAMP_EWORKSPACE
    assert all(bufs[k].unchanged(before[k]) for k in bufs)
    assert call() == 0
    for k, b in bufs.items():
        assert b.intact(), k
    r = dict(dsi=bufs["dsi"].t.view(D, H, W), coords=bufs["coords"].t.view(N, D, 2), invdepth=bufs["inv"].t.view(H, W),
             confidence=bufs["conf"].t.view(H, W), plane=bufs["plane"].t.view(H, W), status=bufs["status"].t)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    _check(r, adaptive_radius=1, fill=0.5)
    assert dsiref.compare(r["coords"], x, y, t, knots, times, 2.0, K, RNG, D, H, W)["ok"]
    # no event: the DSI is zeroed, the detection runs, the fill everywhere; still inside the guards
    assert call(N=0, ex=None) == 0
    assert all(b.intact() for b in bufs.values())
    assert not bufs["dsi"].t.any() and (bufs["inv"].t == 0.5).all() and (bufs["plane"].t == -1).all()
    assert bufs["status"].t.cpu().tolist() == [0] * 8


# ------------------------------------------------------------------------------------------------ 6. tracker
def _ask(slam, f, frame):
    from rampvo_amd import ops
    x, y, t, p = (v.clone() for v in kit.query_events(f))
    x[:200], y[:200], t[:200] = 100.0, 80.0, kit.tstamp(f)          # at the reference time: 200 votes on one pixel of every plane
    out = slam.event_depth(x, y, t, planes=24, min_votes=2.0, as_tensor=True)
    res = {"resident_mid": kit.resident(slam)}
    knots, ts = slam.trajectory(as_tensor=True)
    n = slam.peek()["n"]
    med = torch.median(slam.patches_[n - 3:n, :, 2]).reshape(1)
    ref = ops.event_dsi(x, y, t, knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), frame[2].cuda().float(), 240, 320, planes=24,
                        range=torch.cat([med / 4.0, med * 4.0]), min_votes=2.0)
    res["out"], res["ref"], res["med"] = kit.host(out), kit.host(ref), float(med)
    res["numpy"] = slam.event_depth(x, y, t, planes=24, min_votes=2.0)
    # compensate_events(invdepth="events") = event_depth(fill="median"), then compensate_events(invdepth=that map)
    a = slam.compensate_events(x, y, t, p, invdepth="events", want_xy=True, as_tensor=True)
    m = slam.event_depth(x, y, t, fill="median", as_tensor=True)["invdepth"]
    b = slam.compensate_events(x, y, t, p, invdepth=m, want_xy=True, as_tensor=True)
    res["comp"], res["comp_ref"], res["map"] = kit.host(a), kit.host(b), kit.host(m)
    return res


def test_tracker_event_depth_device_resident():
    """event_depth equals ops.event_dsi fed by trajectory()'s knots, the fed intrinsics and the range around the tracker's own
    depth median; compensate_events(invdepth="events") equals its two steps; the tracker stays device resident and tracks
    the bits of a run that is never asked"""
    a, ctl = kit.run_resident(True, _ask), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_mid"] and a["resident_after"] and a["resident_at_end"]
    assert a["med"] > 0 and sorted(a["out"]) == ["confidence", "dsi", "invdepth", "plane", "range", "status"]
    for k in ("dsi", "invdepth", "confidence", "plane", "status"):
        assert np.array_equal(a["out"][k], a["ref"][k], equal_nan=True), k
        assert isinstance(a["numpy"][k], np.ndarray) and np.array_equal(a["numpy"][k], a["out"][k], equal_nan=True), k
    st = a["out"]["status"]
    assert st[0] == 0 and st[3] == 0 and st[5] >= 200 and st[3:6].sum() == 5000 and st[6] == (a["out"]["plane"] >= 0).sum() > 0
    assert a["out"]["plane"][80, 100] >= 0 and a["out"]["confidence"][80, 100] >= 199.0          # (200, up to the round trip's split)
    assert georef.same_bits(a["out"]["range"], np.array([a["med"] / 4.0, a["med"] * 4.0], np.float32))
    kit.same(a["comp"], a["comp_ref"], "compensate_events")
    assert np.isfinite(a["map"]).all() and (a["map"] == np.float32(a["med"])).any() and (a["map"] != np.float32(a["med"])).any()
    for f in (kit.T_QUERY + 1, kit.T_QUERY + 2):
        kit.same(a["state", f], ctl["state", f], "state %d" % f)


@torch.no_grad()
def test_tracker_event_depth_host_driven():
    """a host-driven tracker: the numpy form equals ops.event_dsi on the same inputs, compensate_events(invdepth="events")
    its two steps; an empty range and frame time stamps that decrease make the numpy form raise"""
    from rampvo_amd import ops
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    rng = np.random.default_rng(22)
    x, y = rng.uniform(0, 319, 1000).astype(np.float32), rng.uniform(0, 239, 1000).astype(np.float32)
    t = rng.uniform(kit.tstamp(f - 2), kit.tstamp(f), 1000)
    out = slam.event_depth(x, y, t, planes=8, range=(0.1, 1.5), min_votes=1.5, adaptive_radius=2, fill=0.25)
    knots, ts = slam.trajectory(as_tensor=True)
    ref = ops.event_dsi(cu(x), cu(y), cu(t), knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), frame[2].cuda().float(), 240, 320,
                        planes=8, range=(0.1, 1.5), min_votes=1.5, adaptive_radius=2, fill=0.25)
    for k in ("dsi", "invdepth", "confidence", "plane", "status"):
        assert isinstance(out[k], np.ndarray) and np.array_equal(out[k], ref[k].cpu().numpy(), equal_nan=True), k
    assert out["status"][0] == 0 and out["status"][3:6].sum() == 1000
    a = slam.compensate_events(x, y, t, np.ones(1000, np.int8), invdepth="events", want_xy=True)
    m = slam.event_depth(x, y, t, fill="median", as_tensor=True)["invdepth"]
    kit.same(a, slam.compensate_events(x, y, t, np.ones(1000, np.int8), invdepth=m, want_xy=True), "compensate_events")
    with pytest.raises(RuntimeError, match="range of inverse depths"):
        slam.event_depth(x, y, t, range=(0.5, 0.5))
    with pytest.raises(RuntimeError, match="'map' or 'events'"):
        slam.compensate_events(x, y, t, np.ones(1000, np.int8), invdepth="patches")
    slam.tlist = slam.tlist[::-1]
    with pytest.raises(RuntimeError, match="time stamps decrease"):
        slam.event_depth(x, y, t, range=(0.1, 1.5))
    del slam
    kit.quiesce()
