"""The numpy restatement of the event contrast (tests/contrastref.py) has to earn its place as the GPU test's reference: its
analytic gradient against finite differences in float64, closed forms, the comparison the GPU test uses against the mistakes
the definition invites, the line search on a scene it has to sharpen, and the new entry points' export.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import contrastref
import interpref
import warpref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 32
K = np.array([30.0, 28.0, 15.5, 11.25], np.float32)
THETA = np.array([0.3, -0.2, 0.15, 0.25, -0.3, 0.5, 0.2], np.float32)      # size 0.1 - 0.5


def scene(seed=1, n=1500, margin=1.5, depth="scalar"):
    """a walk of 5 knots, events over its range and over the image with a margin, so that some lie on the border (a neighbour
    outside the image: the mean's term of the gradient does not cancel)"""
    rng = np.random.default_rng(seed)
    knots, times = interpref.walk_scene(seed + 100, 5)
    x = rng.uniform(-margin, W - 1 + margin, n).astype(np.float32)
    y = rng.uniform(-margin, H - 1 + margin, n).astype(np.float32)
    t = rng.uniform(0.0, 4.0, n)
    p = rng.choice([-1, 1], n).astype(np.int8)
    d = 0.5 if depth == "scalar" else (0.3 + 0.5 * rng.uniform(0, 1, (H, W))).astype(np.float32)
    return (x, y, t, p, knots, times, 2.0, K, d, H, W)


@pytest.mark.parametrize("depth", ["scalar", "map"])
@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("at", ["zero", "theta"])
def test_gradient_against_finite_differences(at, signed, depth):
    """central differences of the float64 variance, h = 1e-6 or smaller (the variance is piecewise smooth in theta -- an event
    that crosses a pixel boundary changes its neighbours -- so both samples are taken with every event in the cell it has at
    theta): 1e-6 of the largest component (2e-9 measured at 1500 events)"""
    args = scene(2, depth=depth)
    th = np.zeros(7) if at == "zero" else THETA.astype(np.float64)
    g, _ = contrastref.gradient(*args, theta=th, signed=signed)
    fd = np.zeros(7)
    cells = lambda c: np.floor(np.nan_to_num(c["xy"], nan=-9.0))
    f = lambda v: contrastref.contrast(*args, theta=v, signed=signed)
    here = cells(f(th))
    for c in range(7):
        for h in (1e-6, 3e-7, 1e-7, 3e-8):            # f is piecewise smooth: both samples in the piece theta lies in
            e = np.zeros(7)
            e[c] = h
            lo, hi = f(th - e), f(th + e)
            if np.array_equal(cells(lo), here) and np.array_equal(cells(hi), here):
                break
        else:
            raise AssertionError("no step keeps every event in its pixel cell")
        fd[c] = (hi["variance"] - lo["variance"]) / (2 * h)
    print("analytic", g, "\nfinite differences", fd, "\nlargest difference / largest component", np.abs(g - fd).max() / np.abs(g).max())
    assert np.abs(g).max() > 0 and np.abs(g - fd).max() <= 1e-6 * np.abs(g).max()


def test_one_event_on_an_integer_pixel():
    knots = np.array([[0, 0, 0, 0, 0, 0, 1]], np.float32)
    c = contrastref.contrast([5.0], [7.0], [0.0], [1], knots, [0.0], 0.0, K, 0.0, H, W)
    Pn = H * W
    assert c["image"][7, 5] == 1.0 and c["image"].sum() == 1.0
    assert abs(c["mean"] - 1.0 / Pn) < 1e-18 and abs(c["variance"] - (1.0 / Pn - 1.0 / Pn ** 2)) < 1e-15 and c["sum_sq"] == 1.0
    # at an integer pixel the neighbour to the right carries weight 0: the x term is (0 - mu) - (1 - mu) = -1, times tau = 0
    g, a = contrastref.gradient([5.0], [7.0], [0.0], [1], knots, [0.0], 0.0, K, 0.0, H, W)
    assert not g.any() and not a.any()
    # the same event half a unit of time away from t_ref: dx'/dv_x = tau ds fx / Z = 0.5 * 0.4 * fx
    g, _ = contrastref.gradient([5.0], [7.0], [0.5], [1], knots, [0.0], 0.0, K, 0.4, H, W)
    assert abs(g[0] - (2.0 / Pn) * (-1.0) * 0.5 * float(np.float32(0.4)) * 30.0) < 1e-12


def test_two_coincident_events_of_opposite_polarity():
    knots, times = interpref.walk_scene(3, 3)
    c = contrastref.contrast([5.3, 5.3], [7.6, 7.6], [0.7, 0.7], [1, -1], knots, times, 1.0, K, 0.5, H, W, theta=THETA)
    assert c["variance"] == 0.0 and c["sum_sq"] == 0.0
    c = contrastref.contrast([5.3, 5.3], [7.6, 7.6], [0.7, 0.7], [1, -1], knots, times, 1.0, K, 0.5, H, W, theta=THETA, signed=False)
    assert c["variance"] > 0


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_zero_correction_reproduces_the_warp(dtype):
    args = scene(4, n=300, depth="map")
    x, y, t, p, knots, times, t_ref, Kc, d, _, _ = args
    x[7] = np.nan
    ref, _ = warpref.warp(x, y, t, knots, times, t_ref, Kc, d, H, W, dtype=dtype)
    for th in (None, np.zeros(7)):
        g = contrastref.geometry(x, y, t, knots, times, t_ref, Kc, d, H, W, theta=th, dtype=dtype)
        assert g["xy"].dtype == dtype and np.array_equal(g["xy"], ref, equal_nan=True)
    assert np.isnan(ref[7]).all() and np.isfinite(ref).all(-1).sum() > 200


@pytest.mark.parametrize("mistake", contrastref.MISTAKES)
def test_the_comparison_rejects_the_mistake(mistake):
    """the float32-geometry restatement passes the GPU test's comparison, every mistaken gradient fails it"""
    signed = mistake != "nomean"           # (the count image has the larger mean)
    args = scene(5)
    good, _ = contrastref.gradient(*args, theta=THETA, signed=signed, dtype=np.float32)
    c = contrastref.compare(good, *args, theta=THETA, signed=signed)
    assert c["ok"], c
    bad, _ = contrastref.gradient(*args, theta=THETA, signed=signed, mistake=mistake)
    c = contrastref.compare(bad, *args, theta=THETA, signed=signed)
    print(mistake, "err / bound", c["err"] / c["bound"])
    assert not c["ok"]


def test_failure_conventions_of_the_restatement():
    args = list(scene(6, n=50))
    args[5] = args[5][::-1].copy()
    c = contrastref.contrast(*args)
    assert np.isnan(c["xy"]).all() and c["variance"] == 0.0           # (the kernel answers NaN: the GPU test checks that)


def test_align_sharpens_the_dot_scene():
    """the accepted variances rise strictly and the final variance is at least twice the first: a condition on the scene"""
    s = contrastref.align_scene()
    ev = contrastref.evaluator(**s)
    r = contrastref.align(ev)
    print("variance0 %.6g final %.6g after %d steps, correction %s" % (r["variance0"], r["variance"], len(r["history"]), r["correction"]))
    h = [r["variance0"]] + r["history"]
    assert len(r["history"]) >= 3 and all(b > a for a, b in zip(h, h[1:]))
    assert r["variance"] >= 2.0 * r["variance0"]
    assert not r["correction"][[0, 1, 2, 6]].any()                    # only the rotation is free
    assert np.abs(r["correction"][3:6] - contrastref.ALIGN_RATE).max() < 0.05
    # and the library's own loop takes the same path when fed the same evaluations
    from rampvo_amd import ops
    q = ops.align_loop(lambda th: tuple(ev(np.asarray(th))), [0.0] * 7, (0, 0, 0, 1, 1, 1, 0), 0.05, 20)
    assert q["history"] == r["history"] and np.array_equal(np.asarray(q["correction"]), r["correction"])


def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_event_contrast", "ramp_event_contrast_workspace_bytes"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    for macro, val in (("RAMP_CONTRAST_UNSIGNED", _lib.RAMP_CONTRAST_UNSIGNED),
                       ("RAMP_CONTRAST_BAD_CORRECTION", _lib.RAMP_CONTRAST_BAD_CORRECTION)):
        assert re.search(r"#define %s %d\b" % (macro, val), header), macro
    assert _lib.RAMP_CONTRAST_UNSIGNED & (_lib.RAMP_INTERP_EXTRAPOLATE | _lib.RAMP_WARP_DEPTH_MAP | _lib.RAMP_WARP_IDENTITY) == 0
    n = lib.ramp_event_contrast_workspace_bytes(5, H, W)
    assert n % 8 == 0 and n > lib.ramp_event_warp_workspace_bytes(5, 1, H, W) - H * W * 8
    assert lib.ramp_event_contrast_workspace_bytes(5, 0, W) == 0
    for name in ("event_contrast", "event_align"):
        assert callable(getattr(ops, name))
    for name in ("event_contrast", "align_events"):
        assert callable(getattr(TrackerQueries, name))


def test_argument_checks_that_need_no_gpu():
    """RAMP_EINVAL before anything touches the device (the pointers are never read)"""
    from rampvo_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)

    def call(N=10, T=2, t_ref=0.0, flags=0, H_=H, W_=W, sums=q, stats=q, status=q, ws=q):
        return lib.ramp_event_contrast(q, q, q, q, N, q, q, T, t_ref, q, q, None, flags, H_, W_, None, sums, stats, None, ws, 0,
                                       status, None)

    for kw in (dict(N=-1), dict(T=0), dict(H_=0), dict(W_=0), dict(t_ref=float("nan")), dict(t_ref=float("inf")),
               dict(flags=_lib.RAMP_WARP_IDENTITY), dict(flags=32), dict(sums=None), dict(stats=None), dict(status=None),
               dict(ws=None), dict(ws=ctypes.c_void_p(q.value + 8))):
        assert call(**kw) == -1, kw
    assert call(N=0) == 0
    assert call() == -3                                               # a workspace of 0 bytes: RAMP_EWORKSPACE
