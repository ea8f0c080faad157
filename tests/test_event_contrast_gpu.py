"""Event contrast and its gradient on the GPU: ``ramp_event_contrast`` (csrc/contrast.hip) through ``ops.event_contrast``,
``ops.event_align`` and the tracker's ``event_contrast`` / ``align_events``.

Three references.  (1) ``ops.event_warp``: with a zero correction the image and the status words are its bits.  (2) The exact
emulator ``warpref.scatter`` on the kernel's own coordinates: the accumulators as integers, and from them the statistics as
exact rationals (Python integers and ``fractions.Fraction``).  (3) The float64 restatement tests/contrastref.py for the
gradient: per component ``|grad - float64| <= georef.bound(floor, env)``, env = the float32-geometry restatement's own error
against float64 on the same inputs, floor = 1e-5 x the sum of the absolute per-event terms of that component.

Images are 24 x 32 and 37 x 53 (not square, not multiples of a wave).  The tracker tests run the small synthetic tracker of
tests/trackerkit.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import contrastref
import georef
import interpref
import trackerkit as kit
import warpref
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

SIZES = {"24x32": (24, 32, np.array([30.0, 28.0, 15.5, 11.25], np.float32)),
         "37x53": (37, 53, np.array([44.0, 41.0, 26.25, 18.5], np.float32))}
THETA = np.array([0.3, -0.2, 0.15, 0.25, -0.3, 0.5, 0.2], np.float32)
_tab = {}



def _scene(seed, n, size="24x32", T=5, margin=1.5, depth="scalar", step=None):
    H, W, K = SIZES[size]
    rng = np.random.default_rng(seed)
    knots, times = interpref.walk_scene(seed + 100, T, **({"step": step} if step else {}))
    x = rng.uniform(-margin, W - 1 + margin, n).astype(np.float32)
    y = rng.uniform(-margin, H - 1 + margin, n).astype(np.float32)
    t = rng.uniform(times[0] - (0.2 if T > 1 else 1.0), times[-1] + (0.2 if T > 1 else 1.0), n)
    p = rng.choice([-1, 1], n).astype(np.int8)
    d = 0.5 if depth == "scalar" else (0.3 + 0.5 * rng.uniform(0, 1, (H, W))).astype(np.float32)
    return (x, y, t, p, knots, times, float(0.5 * (times[0] + times[-1])), K, d, H, W)


def _dev(args):
    x, y, t, p, knots, times, t_ref, K, d, H, W = args
    return (cu(x), cu(y), cu(np.asarray(t, np.float64)), cu(p), cu(np.asarray(knots, np.float32)), cu(np.asarray(times, np.float64)),
            t_ref, cu(K), cu(d) if np.ndim(d) == 2 else float(d), H, W)


def _contrast(args, **kw):
    from rampvo_amd import ops
    return {k: v.cpu().numpy() for k, v in ops.event_contrast(*_dev(args), **kw).items()}


def _warp(args, **kw):
    from rampvo_amd import ops
    return {k: v.cpu().numpy() for k, v in ops.event_warp(*_dev(args), want_xy=True, **kw).items()}


def _exact_stats(acc):
    """variance and sum of I^2 of one int64 accumulator plane as exact rationals (I = acc 2^-24)"""
    vals = [int(v) for v in acc.reshape(-1)]
    Pn, s1, s2 = len(vals), sum(vals), sum(v * v for v in vals)
    return Fraction(Pn * s2 - s1 * s1, Pn * Pn * (1 << 48)), Fraction(s2, 1 << 48), Fraction(s1, Pn * (1 << 24))


def _rel(value, exact):
    return abs(Fraction(float(value)) - exact) / exact if exact else abs(float(value))


def _check_against_the_warp(args, r, w, plane, N):
    """``r`` of ops.event_contrast (zero correction) against ``w`` of ops.event_warp on the same arguments: the image and
    the status bit for bit, the accumulators of the emulator on the warp's own coordinates as integers, the statistics
    against their exact rational values"""
    H, W = args[9], args[10]
    assert georef.same_bits(r["iwe"], w["iwe"]) and np.array_equal(r["status"], w["status"])
    s = warpref.scatter(w["xy"], args[3], H, W)
    assert georef.same_bits(r["iwe"], warpref.finish_f32(s["iwe"]))
    assert [int(v) for v in r["sums"]] == [int(s["iwe"][0].sum()), int(s["iwe"][1].sum())]
    var, s2, mean = _exact_stats(s["iwe"][plane])
    e_var, e_s2, e_mean = _rel(r["stats"][0], var), _rel(r["stats"][2], s2), _rel(r["stats"][1], mean)
    print("N=%d plane %d: variance %.17g, relative error of variance %.2e, of sum I^2 %.2e, of the mean %.2e"
          % (N, plane, r["stats"][0], e_var, e_s2, e_mean))
    assert e_var <= 1e-12 and e_s2 <= 1e-12 and e_mean <= 1e-12
    assert r["stats"][3] == H * W and not r["stats"][4:].any() and r["variance"] == r["stats"][0]
    assert r["status"][3:7].sum() == N and r["status"][6] == s["n_contributed"]


# --------------------------------------------------------------------- 1. zero correction and the exact emulator
@pytest.mark.parametrize("N", [1, 1023, 1025, 2 * 1024 + 7])
@pytest.mark.parametrize("size", ["24x32", "37x53"])
def test_zero_correction_equals_the_warp_and_the_emulator(N, size):
    args = _scene(N, N, size, depth="map" if N % 2 else "scalar")
    w = _warp(args)
    for signed in (True, False):
        for cor in (None, np.zeros(7, np.float32)):
            r = _contrast(args, correction=cor, signed=signed, want_iwe=True)
            _check_against_the_warp(args, r, w, 0 if signed else 1, N)
            assert np.isfinite(r["grad"]).all()


@pytest.mark.parametrize("T", [1, 2, 9, "lds+1"])
def test_knot_counts(T):
    from rampvo_amd import _lib
    T = _lib.lib().ramp_se3_interp_lds_knots() + 1 if T == "lds+1" else T
    args = _scene(40 + min(T, 10), 1025, "37x53", T=T, step=(0.002,) * 6 if T > 9 else None)
    w = _warp(args)
    r = _contrast(args, want_iwe=True)
    _check_against_the_warp(args, r, w, 0, 1025)
    c = contrastref.compare(_contrast(args, correction=THETA)["grad"], *args, theta=THETA)
    print("T=%d: err / bound" % T, c["err"] / c["bound"])
    assert c["ok"], c


def test_second_trip_of_the_grid_and_unaligned_arrays():
    """one event more than a full grid covers in one trip (the statistics of a nearly uniform image: the squares are centred
    before they are summed); the same events from arrays that are not 16-byte aligned (the scalar staging path) give the
    same bits, the gradient included (the same lanes see the same events)"""
    from rampvo_amd import _lib, ops
    N = _lib.lib().ramp_event_warp_grid_events() + 1
    x, y, t, p, knots, times, t_ref, K, d, H, W = _scene(6, N + 1, margin=1.0)
    args = (x[1:], y[1:], t[1:], p[1:], knots, times, t_ref, K, d, H, W)
    w = _warp(args)
    for signed in (True, False):
        r = _contrast(args, signed=signed, want_iwe=True)
        _check_against_the_warp(args, r, w, 0 if signed else 1, N)
    xs, ys, ts, ps = cu(x)[1:], cu(y)[1:], cu(t)[1:], cu(p)[1:]
    assert xs.data_ptr() % 16 and xs.is_contiguous()
    q = ops.event_contrast(xs, ys, ts, ps, cu(knots), cu(times), t_ref, cu(K), d, H, W, signed=False, want_iwe=True)
    for k in ("stats", "sums", "grad", "iwe", "status"):
        assert georef.same_bits(q[k].cpu().numpy(), r[k]) if r[k].dtype.kind == "f" else np.array_equal(q[k].cpu().numpy(), r[k]), k


# ------------------------------------------------------------------------------------------------ 2. order
def test_order_of_the_events():
    """a permutation leaves stats, sums and iwe in every bit and moves grad by at most 1e-12 x the sum of the absolute
    per-event terms; a second call repeats all bits"""
    args = _scene(8, 4099, "37x53")
    a = _contrast(args, correction=THETA, want_iwe=True)
    perm = np.random.default_rng(9).permutation(4099)
    b = _contrast(tuple(v[perm] for v in args[:4]) + args[4:], correction=THETA, want_iwe=True)
    c = _contrast(args, correction=THETA, want_iwe=True)
    for k in ("stats", "iwe", "grad"):
        assert georef.same_bits(a[k], c[k]), k
        if k != "grad":
            assert georef.same_bits(a[k], b[k]), k
    assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["status"], b["status"]) and np.array_equal(a["sums"], c["sums"])
    _, abs_terms = contrastref.gradient(*args, theta=THETA)
    print("grad moved by", np.abs(a["grad"] - b["grad"]) / abs_terms, "of the sum of the absolute terms")
    assert (np.abs(a["grad"] - b["grad"]) <= 1e-12 * abs_terms).all() and a["grad"].any()


# ------------------------------------------------------------------------------------------------ 3. gradient
GRAD_CASES = [("theta=0 signed scalar", None, True, "scalar", 1.5), ("theta=0 count map", None, False, "map", 1.5),
              ("theta signed scalar", THETA, True, "scalar", 1.5), ("theta signed map", THETA, True, "map", 1.5),
              ("theta count scalar", THETA, False, "scalar", 1.5), ("theta count map", THETA, False, "map", 1.5),
              ("theta count inside", THETA, False, "scalar", -4.0), ("theta signed border", THETA, True, "map", 3.0)]


def test_gradient_against_float64():
    """(measured, envelope, bound) per case and component; the largest measured / envelope ratios are printed last"""
    tab = georef.Table("event_contrast: gradient against float64 (per component)")
    names = ("v0", "v1", "v2", "w0", "w1", "w2", "lam")
    worst = held = 0.0
    for size in SIZES:
        for name, th, signed, depth, margin in GRAD_CASES:
            args = _scene(len(name) + len(size), 1500, size, margin=margin, depth=depth)
            r = _contrast(args, correction=th, signed=signed)
            c = contrastref.compare(r["grad"], *args, theta=th, signed=signed)
            for i in range(7):
                tab.add("%s %s %s" % (size, name, names[i]), c["err"][i], c["env"][i], c["floor"][i])
                if c["env"][i] > 0:
                    worst = max(worst, c["err"][i] / c["env"][i])
                    held = max(held, c["err"][i] / c["env"][i]) if 4.0 * c["env"][i] >= c["floor"][i] else held
            assert np.abs(c["ref"]).max() > 0 and r["status"][0] == 0
            v64 = contrastref.contrast(*args, theta=th, signed=signed)["variance"]
            assert abs(r["stats"][0] - v64) <= 1e-4 * v64              # (the fixed point and fp32 coordinates: a sanity check)
    tab.show()
    print("largest measured / envelope ratio: %.2f; over the rows whose bound is four envelopes and not the floor: %.2f" % (worst, held))
    assert not tab.failed(), tab.failed()


@pytest.mark.parametrize("mistake", contrastref.MISTAKES)
def test_the_gpu_comparison_rejects_the_mistake(mistake):
    """the kernel's gradient passes against the restatement and fails against the mistaken one by more than the bound: the
    comparison has teeth on the kernel's own output"""
    signed = mistake != "nomean"
    args = _scene(5, 1500)
    if "grad" not in _tab.setdefault(signed, {}):
        _tab[signed]["grad"] = _contrast(args, correction=THETA, signed=signed)["grad"]
    g = _tab[signed]["grad"]
    c = contrastref.compare(g, *args, theta=THETA, signed=signed)
    assert c["ok"], c
    bad, _ = contrastref.gradient(*args, theta=THETA, signed=signed, mistake=mistake)
    assert (np.abs(g - bad) > c["bound"]).any()


# ------------------------------------------------------------------------------------------------ 4. failures
def test_failure_behaviour():
    args = _scene(15, 300)
    x, y, t, p, knots, times, t_ref, K, d, H, W = args
    good = _contrast(args, correction=THETA, want_iwe=True)
    assert good["status"][0] == 0 and np.isfinite(good["stats"]).all() and good["stats"][0] > 0
    # decreasing knot times
    r = _contrast((x, y, t, p, knots, times[::-1].copy(), t_ref, K, d, H, W), correction=THETA, want_iwe=True)
    assert r["status"][0] == 1 and r["status"][4:].sum() == 0
    assert np.isnan(r["stats"][:3]).all() and np.isnan(r["grad"]).all() and np.isnan(r["iwe"]).all() and not r["sums"].any()
    # a NaN in the correction
    for i in (0, 4, 6):
        th = THETA.copy()
        th[i] = np.nan if i else np.inf
        r = _contrast(args, correction=th, want_iwe=True)
        assert r["status"][0] == 2 and r["status"][4:].sum() == 0
        assert np.isnan(r["stats"][:3]).all() and np.isnan(r["grad"]).all() and np.isnan(r["iwe"]).all() and not r["sums"].any()
    # a NaN event: counted, and the others' result is that of a call without it
    for col in range(3):
        a = [x.copy(), y.copy(), t.copy()]
        a[col][77] = [np.nan, np.inf, -np.inf][col]
        r = _contrast((a[0], a[1], a[2], p, knots, times, t_ref, K, d, H, W), correction=THETA, want_iwe=True)
        keep = np.arange(300) != 77
        q = _contrast((x[keep], y[keep], t[keep], p[keep], knots, times, t_ref, K, d, H, W), correction=THETA, want_iwe=True)
        assert r["status"][3] == 1 and q["status"][3] == 0
        assert georef.same_bits(r["stats"], q["stats"]) and georef.same_bits(r["iwe"], q["iwe"]) and np.array_equal(r["sums"], q["sums"])
        _, abs_terms = contrastref.gradient(*args, theta=THETA)
        assert (np.abs(r["grad"] - q["grad"]) <= 1e-12 * abs_terms).all()
    # every event rejected (behind the camera after a forward motion past the points): variance 0, gradient 0
    fwd = np.array([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1.0, 0, 0, 0, 1]], np.float32)
    r = _contrast((x, y, np.ones(300), p, fwd, np.array([0.0, 1.0]), 0.0, K, 0.9, H, W), want_iwe=True)
    assert r["status"].tolist() == [0, 0, 0, 0, 300, 0, 0, 0]
    assert not r["stats"][:3].any() and not r["grad"].any() and not r["iwe"].any() and not r["sums"].any()
    assert not np.signbit(r["stats"][0])
    # two coincident events of opposite polarity: variance 0 of the signed image
    two = (np.array([5.3, 5.3], np.float32), np.array([7.6, 7.6], np.float32), np.array([t_ref + 0.3] * 2), np.array([1, -1], np.int8))
    r = _contrast(two + (knots, times, t_ref, K, d, H, W), correction=THETA)
    assert r["stats"][0] == 0 and r["status"][6] == 2


def test_arguments_and_canaries():
    """the C entry with guard words on both sides of every output and of the workspace; N == 0 launches and writes nothing"""
    from rampvo_amd import _lib
    L = _lib.lib()
    N, T = 300, 5
    args = _scene(19, N)
    dx, dy, dt, dp, dk, dtm, t_ref, dK, _, H, W = _dev(args)
    dd = torch.full((1,), 0.5, device="cuda")
    dth = cu(THETA)
    nbytes = L.ramp_event_contrast_workspace_bytes(T, H, W)

    bufs = dict(iwe=Flat(2 * H * W, torch.float32, -7.0), sums=Flat(2, torch.int64, -7), stats=Flat(8, torch.float64, -7.0),
                grad=Flat(7, torch.float64, -7.0), status=Flat(8, torch.int32, -7), ws=Flat(nbytes, torch.uint8, 0xA5))
    assert bufs["ws"].t.data_ptr() % 16 == 0

    def call(N=N, ws_bytes=nbytes, flags=0, outs=("iwe", "grad")):
        o = lambda k: _lib.ptr(bufs[k].t) if k in outs else None
        rc = L.ramp_event_contrast(_lib.ptr(dx), _lib.ptr(dy), _lib.ptr(dt), _lib.ptr(dp), N, _lib.ptr(dk), _lib.ptr(dtm), T, t_ref,
                                   _lib.ptr(dK), _lib.ptr(dd), _lib.ptr(dth), flags, H, W, o("iwe"), _lib.ptr(bufs["sums"].t),
                                   _lib.ptr(bufs["stats"].t), o("grad"), _lib.ptr(bufs["ws"].t), ws_bytes,
                                   _lib.ptr(bufs["status"].t), _lib.stream())
        torch.cuda.synchronize()
        return rc

    before = {k: v.snapshot() for k, v in bufs.items()}
    assert call(N=0) == 0 and call(flags=_lib.RAMP_WARP_IDENTITY) == -1 and call(ws_bytes=nbytes - 8) == -3
    assert all(bufs[k].unchanged(before[k]) for k in bufs)                 # nothing written, status included
    assert call(outs=()) == 0                                                    # neither optional output
    assert bufs["iwe"].unchanged(before["iwe"]) and bufs["grad"].unchanged(before["grad"])
    stats_only = bufs["stats"].t.cpu().numpy().copy()
    assert call() == 0
    for k, b in bufs.items():
        assert b.intact(), k
    ref = _contrast(args, correction=THETA, want_iwe=True)
    assert georef.same_bits(bufs["stats"].t.cpu().numpy(), ref["stats"]) and georef.same_bits(stats_only, ref["stats"])
    assert georef.same_bits(bufs["grad"].t.cpu().numpy(), ref["grad"]) and georef.same_bits(bufs["iwe"].t.view(2, H, W).cpu().numpy(), ref["iwe"])
    assert np.array_equal(bufs["sums"].t.cpu().numpy(), ref["sums"]) and np.array_equal(bufs["status"].t.cpu().numpy(), ref["status"])


# ------------------------------------------------------------------------------------------------ 5. the line search
def test_event_align_on_the_dot_scene():
    """the accepted variances rise strictly and the result reaches 0.9 of what the float64 restatement's own search gains (the
    margin is for the fp32 geometry taking a different line-search path)"""
    from rampvo_amd import ops
    s = contrastref.align_scene()
    ref = contrastref.align(contrastref.evaluator(**s))
    r = ops.event_align(cu(s["x"]), cu(s["y"]), cu(s["t"]), cu(s["p"]), cu(s["knots"]), cu(s["times"]), s["t_ref"], cu(s["K"]),
                        s["invdepth"], s["H"], s["W"])
    print("variance0 %.6g -> %.6g in %d steps (restatement: %.6g -> %.6g in %d), correction %s"
          % (r["variance0"], r["variance"], len(r["history"]), ref["variance0"], ref["variance"], len(ref["history"]), r["correction"]))
    h = [r["variance0"]] + r["history"]
    assert len(h) > 1 and all(b > a for a, b in zip(h, h[1:])) and r["variance"] == h[-1]
    assert r["variance"] >= r["variance0"] + 0.9 * (ref["variance"] - ref["variance0"])
    assert not any(r["correction"][i] for i in (0, 1, 2, 6))


# ------------------------------------------------------------------------------------------------ 6. tracker
def _ask(slam, f, frame):
    from rampvo_amd import ops
    x, y, t, p = kit.query_events(f)
    res = {}
    out = slam.event_contrast(x, y, t, p, correction=THETA * 0.1, want_iwe=True, as_tensor=True)
    res["numpy"] = slam.event_contrast(x, y, t, p, correction=THETA * 0.1, want_iwe=True)
    res["map"] = kit.host(slam.event_contrast(x, y, t, p, invdepth="map", radius=kit.RADIUS, signed=False, as_tensor=True))
    res["align"] = slam.align_events(x, y, t, p, iters=2)
    knots, ts = slam.trajectory(as_tensor=True)
    n = slam.peek()["n"]
    med = torch.median(slam.patches_[n - 3:n, :, 2])
    K = frame[2].cuda().float()
    tdev = cu(np.asarray(ts, np.float64))
    ref = ops.event_contrast(x, y, t, p, knots, tdev, float(ts[-1]), K, med, 240, 320, correction=THETA * 0.1, want_iwe=True)
    res["align_ref"] = ops.event_align(x, y, t, p, knots, tdev, float(ts[-1]), K, med, 240, 320, iters=2)
    res["out"], res["ref"] = kit.host(out), kit.host(ref)
    return res


def test_tracker_event_contrast_and_align():
    """slam.event_contrast / align_events equal ops.event_contrast / event_align on trajectory(as_tensor=True), the fed
    intrinsics and the tracker's depth median, bit for bit; the same from a tracker on its own stream; the tracker stays device
    resident and ends with the pose bits of one never asked"""
    a, b, c = kit.run_resident(True, _ask), kit.run_resident("stream", _ask), kit.run_resident(True, None)
    for r in (a, b):
        assert r["resident_before"] and r["resident_after"] and r["resident_at_end"]
        kit.same(r["out"], r["ref"], "against ops.event_contrast")
        assert isinstance(r["numpy"]["variance"], float)
        kit.same({k: v for k, v in r["numpy"].items() if k != "variance"}, {k: v for k, v in r["out"].items() if k != "variance"},
                 "numpy form")
        kit.same(r["align"], r["align_ref"], "against ops.event_align")
        st = r["out"]["status"]
        assert st[0] == 0 and st[3:7].sum() == 5000 and r["out"]["stats"][0] > 0 and np.isfinite(r["out"]["grad"]).all()
        assert r["map"]["status"][0] == 0 and r["map"]["stats"][0] > 0
        assert r["align"]["variance"] >= r["align"]["variance0"]
    for k in ("out", "map", "align"):
        kit.same(b[k], a[k], "own stream: " + k)
    assert c["resident_at_end"]
    for f in (kit.T_QUERY + 1, kit.T_QUERY + 2):
        kit.same(a["state", f], c["state", f], "state of a tracker that is never asked, frame %d" % f)
        kit.same(b["state", f], c["state", f], "own stream, frame %d" % f)


@torch.no_grad()
def test_tracker_event_contrast_host_driven():
    from rampvo_amd import ops
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    x, y, t, p = (v.cpu().numpy() for v in kit.query_events(f, 1000))
    out = slam.event_contrast(x, y, t, p, correction=THETA * 0.1)                     # numpy in, numpy out
    al = slam.align_events(x, y, t, p, iters=2)
    knots, ts = slam.trajectory(as_tensor=True)
    med = torch.median(slam.patches_[slam._n - 3:slam._n, :, 2])
    K, tdev = frame[2].cuda().float(), cu(np.asarray(ts, np.float64))
    ref = ops.event_contrast(cu(x), cu(y), cu(t), cu(p), knots, tdev, float(ts[-1]), K, med, 240, 320, correction=THETA * 0.1)
    assert sorted(out) == ["grad", "stats", "status", "sums", "variance"] and out["variance"] == out["stats"][0] > 0
    for k in ("grad", "stats", "status", "sums"):
        assert isinstance(out[k], np.ndarray) and np.array_equal(out[k], ref[k].cpu().numpy()), k
    kit.same(al, ops.event_align(cu(x), cu(y), cu(t), cu(p), knots, tdev, float(ts[-1]), K, med, 240, 320, iters=2), "align")
    slam.tlist = slam.tlist[::-1]
    with pytest.raises(RuntimeError, match="time stamps decrease"):
        slam.event_contrast(x, y, t, p)
    with pytest.raises(RuntimeError, match="time stamps decrease"):
        slam.align_events(x, y, t, p, iters=1)
    del slam
    kit.quiesce()
