"""tests/cornerref.py -- the numpy restatement the GPU tests of ramp_event_corners compare against, bit for bit -- held to closed
forms painted through the state, and shown to tell each plausible mistake (cornerref.MISTAKES) from the definition on the very
streams the GPU tests use.  Then the entry points and the refusals that need no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import cornerref as cr
import georef

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = cr.H0, cr.W0
SENSORS = ((9, 9), (H, W))
T = cr.TICK


def one(h, w, state, centre=None, **kw):
    """one event at the sensor's centre (or ``centre`` = (x, y)) at t = 3 on the painted state -> (cls, arc)"""
    cx, cy = ((w - 1) // 2, (h - 1) // 2) if centre is None else centre
    o = cr.event_corners([cx], [cy], [3.0], h, w, last_t=state, **kw)
    assert o["status"][1] == 1 and o["status"][2:].sum() == 1 and o["status"][o["cls"][0]] == 1
    assert o["last_t"][cy, cx] == 3.0 and o["count"][0] == (o["cls"][0] == 7) and o["corner_count"].sum() == o["count"][0]
    return int(o["cls"][0]), o["arc"][0].tolist()


def centre(h, w):
    return (w - 1) // 2, (h - 1) // 2


# ------------------------------------------------------------------------------------------------ 1. closed forms
@pytest.mark.parametrize("h,w", SENSORS)
def test_inner_lengths(h, w):
    c = centre(h, w)
    for L, passes in ((2, False), (3, True), (6, True), (7, False)):
        cls, arc = one(h, w, cr.painted(h, w, c, inner=(5, L)))
        assert (cls, arc) == ((6, [5, L, 0, 0]) if passes else (5, [0, 0, 0, 0])), L      # (the outer circle is all NaN: no arc)


@pytest.mark.parametrize("h,w", SENSORS)
def test_outer_lengths(h, w):
    c = centre(h, w)
    for L, passes in ((3, False), (4, True), (8, True), (9, False)):
        cls, arc = one(h, w, cr.painted(h, w, c, inner=(0, 3), outer=(17, L)))
        assert (cls, arc) == ((7, [0, 3, 17, L]) if passes else (6, [0, 3, 0, 0])), L


@pytest.mark.parametrize("h,w", SENSORS)
def test_an_arc_that_wraps_reports_its_start(h, w):
    c = centre(h, w)
    assert one(h, w, cr.painted(h, w, c, inner=(14, 4), outer=(18, 5))) == (7, [14, 4, 18, 5])
    assert one(h, w, cr.painted(h, w, c, inner=(14, 4)), mistake="no_wraparound")[0] == 5
    assert one(h, w, cr.painted(h, w, c, inner=(2, 4)), mistake="circle_reversed") == (6, [10, 4, 0, 0])     # (k -> 15 - k: 2 .. 5 is 10 .. 13)


@pytest.mark.parametrize("h,w", SENSORS)
def test_ties_and_nan(h, w):
    c = centre(h, w)
    cx, cy = c
    s = cr.painted(h, w, c, inner=(2, 4))
    assert one(h, w, s)[0] == 6
    s[cy + cr.INNER[9][1], cx + cr.INNER[9][0]] = 2.0              # an off-arc value equal to the arc's
    assert one(h, w, s)[0] == 5 and one(h, w, s, mistake="ties_by_ge")[0] == 6
    assert one(h, w, cr.painted(h, w, c, inner=(2, 4), rest=2.0))[0] == 5                 # every value equal
    assert one(h, w, cr.painted(h, w, c, inner=(2, 4), rest=cr.NAN)) == (6, [2, 4, 0, 0])  # the rest all NaN: below every number
    assert one(h, w, cr.painted(h, w, c, inner=(2, 4), on=-1.0, rest=cr.NAN)) == (6, [2, 4, 0, 0])
    assert one(h, w, cr.painted(h, w, c, inner=(2, 4), on=-1.0, rest=cr.NAN), mistake="nan_is_zero")[0] == 5
    assert one(h, w, np.full((h, w), cr.NAN)) == (5, [0, 0, 0, 0])                          # everything NaN
    s = cr.painted(h, w, c, inner=(2, 4))
    s[cy + cr.INNER[3][1], cx + cr.INNER[3][0]] = cr.NAN            # a NaN on the arc: it splits it into runs of 1 and 2
    assert one(h, w, s)[0] == 5
    s = cr.painted(h, w, c, inner=(2, 7))
    s[cy + cr.INNER[5][1], cx + cr.INNER[5][0]] = cr.NAN            # ... runs of 3 and 3: still no arc, the values are not one run
    assert one(h, w, s)[0] == 5


@pytest.mark.parametrize("h,w", SENSORS)
def test_wide_accepts_the_complements_and_nothing_else(h, w):
    c = centre(h, w)
    for L in range(1, 16):
        s = cr.painted(h, w, c, inner=(11, L))
        assert (one(h, w, s)[0] >= 6) == (3 <= L <= 6), L
        assert (one(h, w, s, wide=True)[0] >= 6) == (3 <= L <= 6 or 10 <= L <= 13), L
    for L in range(1, 20):
        s = cr.painted(h, w, c, inner=(0, 3), outer=(3, L))
        assert (one(h, w, s)[0] == 7) == (4 <= L <= 8), L
        cls, arc = one(h, w, s, wide=True)
        assert (cls == 7) == (4 <= L <= 8 or 12 <= L <= 16) and arc == ([0, 3, 3, L] if cls == 7 else [0, 3, 0, 0]), L


def test_the_border_is_four_pixels():
    s = np.full((H, W), 1.0)
    for (x, y), border in (((3, 4), True), ((W - 4, 4), True), ((4, 4), False), ((W - 5, H - 5), False), ((4, 3), True), ((4, H - 4), True)):
        p = s if border else cr.painted(H, W, (x, y), inner=(0, 3), outer=(0, 4))
        cls, arc = one(H, W, p, centre=(x, y))
        assert (cls, arc) == ((4, [0, 0, 0, 0]) if border else (7, [0, 3, 0, 4])), (x, y)
    assert one(H, W, s, centre=(3, 4), mistake="border_3")[0] == 5
    for h, w in ((8, 40), (40, 8), (1, 1)):                         # a sensor of border pixels alone is valid
        o = cr.event_corners([w // 2], [h // 2], [1.0], h, w)
        assert o["cls"].tolist() == [4] and o["status"].tolist() == [0, 1, 0, 0, 1, 0, 0, 0]


@pytest.mark.parametrize("h,w", SENSORS)
def test_of_two_nested_arcs_the_shorter_is_reported(h, w):
    c = centre(h, w)
    cx, cy = c
    s = cr.painted(h, w, c, inner=(6, 6), outer=(10, 8))
    for k in (8, 9, 10):
        s[cy + cr.INNER[k][1], cx + cr.INNER[k][0]] = 2.5
    for k in (12, 13, 14, 15):
        s[cy + cr.OUTER[k][1], cx + cr.OUTER[k][0]] = 2.5
    assert one(h, w, s) == (7, [8, 3, 12, 4]) and one(h, w, s, mistake="largest_L_reported") == (7, [6, 6, 10, 8])
    assert one(h, w, s, inner=(4, 6), outer=(5, 8)) == (7, [6, 6, 10, 8])               # the shorter one is not allowed


def test_the_own_pixel_and_the_other_plane_take_no_part():
    c = centre(H, W)
    s = cr.painted(H, W, c, inner=(0, 3), outer=(0, 4))
    s[c[1], c[0]] = 2.75                                            # the event's own predecessor, above the rest
    assert one(H, W, s) == (7, [0, 3, 0, 4]) and one(H, W, s, mistake="own_predecessor_read")[0] == 5
    two = np.stack([s, np.full((H, W), cr.NAN)])
    for pol, cls in ((-1, 7), (1, 5)):
        o = cr.event_corners([c[0]], [c[1]], [3.0], H, W, p=[pol], last_t=two)
        assert o["cls"][0] == cls and o["last_t"][int(pol > 0), c[1], c[0]] == 3.0
    assert cr.event_corners([c[0]], [c[1]], [3.0], H, W, p=[1], last_t=two, mistake="polarity_not_split")["cls"][0] == 7
    assert cr.event_corners([c[0]], [c[1]], [3.0], H, W, last_t=s, mistake="state_ignored")["cls"][0] == 5
    late = s.copy()
    late[c[1], c[0]] = 3.5                                          # the event lies before its own state
    bad = cr.event_corners([c[0], 0], [c[1], -1], [3.0, 1.0], H, W, last_t=late)
    assert bad["status"].tolist() == [1, 2, 0, 1, 0, 0, 0, 0] and np.isnan(bad["last_t"]).all() and not bad["cls"].any()
    assert (bad["index"] == -1).all() and bad["count"][0] == 0 and not bad["arc"].any() and not bad["corner_count"].any()


# ------------------------------------------------------------------------------------------------ 2. the wedge streams
def test_every_wedge_stream_holds_every_class_and_the_set_every_length():
    inner, outer, wide_inner, wide_outer = set(), set(), 0, 0
    for name, x, y, t, p in cr.wedges():
        assert (np.diff(t) >= 0).all() and len(set(zip(x.tolist(), y.tolist()))) == len(x), name     # every pixel fires once
        o = cr.event_corners(x, y, t, H, W)
        assert o["status"][0] == 0 and (o["status"][4:] > 0).all() and o["status"][2:].sum() == len(x), (name, o["status"])
        corner = o["cls"] == 7
        inner |= set(o["arc"][corner, 1].tolist())
        outer |= set(o["arc"][corner, 3].tolist())
        assert np.array_equal(o["index"][:o["count"][0]], np.nonzero(corner)[0]) and (o["index"][o["count"][0]:] == -1).all()
        assert o["corner_count"].sum() == corner.sum() and (o["arc"][o["cls"] == 6, 1] > 0).all() and not o["arc"][o["cls"] <= 5].any()
        ow = cr.event_corners(x, y, t, H, W, wide=True)
        wide_inner, wide_outer = max(wide_inner, ow["arc"][:, 1].max()), max(wide_outer, ow["arc"][:, 3].max())
    assert inner == {3, 4, 5, 6} and outer == {4, 5, 6, 7, 8} and wide_inner >= 10 and wide_outer >= 12


def test_noise_alone_gives_no_corner():
    x, y, t, p = cr.noise(4099)
    s = cr.event_corners(x, y, t, H, W)["status"]
    assert s[7] == 0 and s[4] > 1000 and s[5] > 1000 and s[6] > 0 and s[2:].sum() == 4099


def test_the_streams_are_what_they_claim():
    x, y, t, p = cr.stream(4099)
    assert len(x) == 4099 and (np.diff(t) >= 0).all() and t[0] < 0 < t[-1] and (t == 0).any() and set(np.unique(p)) == {-1, 1}
    assert len(np.unique(t)) < 4099 and x.min() >= 0 and x.max() < W and y.min() >= 0 and y.max() < H
    for kw in (dict(), dict(p=p)):
        o = cr.event_corners(x, y, t, H, W, **kw)
        assert o["status"][0] == 0 and (o["status"][4:] > 20).all(), o["status"]
    both = cr.event_corners(x, y, t, H, W, p=p)
    assert {int(v > 0) for v in p[both["cls"] == 7]} == {0, 1}        # corners on either plane
    xd, yd, td, pd = cr.stream(4099, distinct=True)
    assert len(np.unique(td)) == 4099 and np.array_equal(xd, x) and (np.diff(td) > 0).all()
    perm = cr.shuffle_keeping_cells(xd, yd, pd, np.random.default_rng(2))
    assert sorted(perm.tolist()) == list(range(4099)) and (np.diff(td[perm]) < 0).sum() > 1000
    a, b = cr.event_corners(xd, yd, td, H, W, p=pd), cr.event_corners(xd[perm], yd[perm], td[perm], H, W, p=pd[perm])
    assert b["status"][0] == 0 and np.array_equal(b["cls"], a["cls"][perm]) and np.array_equal(b["arc"], a["arc"][perm])
    assert a["status"][7] > 20


def _differs(a, b):
    return not georef.same_bits(a["last_t"], b["last_t"]) or any(
        not np.array_equal(a[k], b[k]) for k in ("cls", "arc", "index", "count", "corner_count", "status"))


def _cases(mistake):
    """the streams the GPU test runs, as (arguments, keywords): the wedge streams plain, wide and with p, a wedge stream
    that starts below t = 0, the mixed stream whole and in two calls"""
    for name, x, y, t, p in cr.wedges():
        yield (x, y, t), dict()
        yield (x, y, t), dict(wide=True)
        yield (x, y, t), dict(p=p)
    name, x, y, t, p = cr.wedges(t0=-12 * T)[8]
    yield (x, y, t), dict()
    x, y, t, p = cr.stream(4099)
    yield (x, y, t), dict()
    yield (x, y, t), dict(p=p)
    a = cr.event_corners(x[:2049], y[:2049], t[:2049], H, W, p=p[:2049])
    yield (x[2049:], y[2049:], t[2049:]), dict(p=p[2049:], last_t=a["last_t"])


@pytest.mark.parametrize("mistake", cr.MISTAKES)
def test_the_streams_reject_each_mistake(mistake):
    rejected = [kw for args, kw in _cases(mistake)
                if _differs(cr.event_corners(*args, H, W, **kw), cr.event_corners(*args, H, W, mistake=mistake, **kw))]
    assert rejected
    if mistake == "circle_reversed":                                # only the arcs tell it apart
        for args, kw in _cases(mistake):
            a, b = cr.event_corners(*args, H, W, **kw), cr.event_corners(*args, H, W, mistake=mistake, **kw)
            assert np.array_equal(a["cls"], b["cls"]) and np.array_equal(a["index"], b["index"])


# ------------------------------------------------------------------------------------------------ 3. the C entries, ops
def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_event_corners", "ramp_event_corners_ws_bytes", "ramp_event_corners_grid_events"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert _lib.RAMP_CORNER_XY_I32 == 1 and _lib.RAMP_CORNER_WIDE == 2
    assert _lib.RAMP_CORNER_BAD_ORDER == _lib.RAMP_FILTER_BAD_ORDER == cr.BAD_ORDER
    assert ops._STATUS["event_corners"][0]["bad_order"] is ops._STATUS["event_filter"][0]["bad_order"]      # one row
    assert len(ops._STATUS["event_corners"][1]) == 7 and "event_corners" not in ops.STATUS_ROLES.values()
    assert lib.ramp_event_corners_grid_events() == lib.ramp_event_flow_grid_events()
    one_, two = lib.ramp_event_corners_ws_bytes(1000, H, W, 1), lib.ramp_event_corners_ws_bytes(1000, H, W, 2)
    assert one_ % 256 == 0 and 0 < two - one_ <= 4 * H * W + 256 and lib.ramp_event_corners_ws_bytes(1000, H, W, 3) == 0
    assert lib.ramp_event_corners_ws_bytes(1000, 1 << 15, 1 << 15, 1) == 0 and lib.ramp_event_corners_ws_bytes(0, 8, 8, 1) > 0
    assert all(callable(f) for f in (ops.event_corners, ops.event_corners_status, TrackerQueries.event_corners,
                                     TrackerQueries.reset_event_corners))
    assert "corner.hip" in open(os.path.join(ROOT, "rampvo_amd", "csrc", "Makefile")).read()
    # the circles of the header are the reference's, in its order
    block = header[header.index("ramp_event_corners: which events"):header.index("#define RAMP_CORNER_XY_I32")]
    pairs = [(int(a), int(b)) for a, b in re.findall(r"\((-?\d),(-?\d)\)", block)]
    assert tuple(pairs[:16]) == cr.INNER and tuple(pairs[16:36]) == cr.OUTER and len(pairs) == 36
    for ring, r2 in ((cr.INNER, (8, 10)), (cr.OUTER, (13, 17))):
        assert len(set(ring)) == len(ring) and all(r2[0] <= dx * dx + dy * dy <= r2[1] for dx, dy in ring)
        assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) == 1 for a, b in zip(ring, ring[1:] + ring[:1]))      # a closed chain


def test_argument_checks_that_need_no_gpu():
    """every refusal comes before anything touches the device (the pointers are never read)"""
    from rampvo_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd4, odd2 = ctypes.c_void_p(q.value + 4), ctypes.c_void_p(q.value + 2)

    def call(N=10, H=13, W=17, flags=0, inner=(3, 6), outer=(4, 8), p=None, last_in=None, last_out=None, cls=q, arc=None, index=None,
             count=None, corner_count=None, status=q, ws=q, x=q, t=q, ws_bytes=0):
        return lib.ramp_event_corners(x, q, t, p, N, H, W, flags, inner[0], inner[1], outer[0], outer[1], last_in, last_out, cls, arc,
                                      index, count, corner_count, status, ws, ws_bytes, None)

    for kw in (dict(N=-1), dict(H=0), dict(W=0), dict(flags=4), dict(flags=-1), dict(inner=(0, 6)), dict(inner=(7, 6)), dict(inner=(3, 16)),
               dict(outer=(0, 8)), dict(outer=(9, 8)), dict(outer=(4, 20)), dict(status=None), dict(cls=None), dict(x=None), dict(t=None),
               dict(ws=None), dict(index=q), dict(count=q), dict(last_in=odd4), dict(last_out=odd4), dict(status=odd2), dict(arc=odd2),
               dict(index=odd2, count=q), dict(index=q, count=odd2), dict(corner_count=odd2), dict(t=odd4),
               dict(ws=ctypes.c_void_p(q.value + 8))):
        assert call(**kw) == _lib.RAMP_EINVAL, kw
    full = lib.ramp_event_corners_ws_bytes(10, 13, 17, 1)
    assert call() == _lib.RAMP_EWORKSPACE and call(ws_bytes=full - 1) == _lib.RAMP_EWORKSPACE
    assert call(p=q, ws_bytes=full) == _lib.RAMP_EWORKSPACE          # two planes need more
    assert call(N=1 << 31) == _lib.RAMP_EUNSUPPORTED and call(H=1 << 15, W=1 << 15) == _lib.RAMP_EUNSUPPORTED
    for kw in (dict(flags=3), dict(inner=(1, 15), outer=(1, 19)), dict(inner=(4, 4)), dict(H=8, W=40), dict(index=q, count=q, arc=q)):
        assert call(**kw) == _lib.RAMP_EWORKSPACE, kw               # valid: refused only for the workspace it was not given


def test_ops_refusals_need_no_gpu():
    import torch
    from rampvo_amd import ops
    x = torch.zeros(4)
    good = dict(x=x, y=x, t=x.double(), height=13, width=17)
    for kw, text in ((dict(height=0), "positive"), (dict(inner=(0, 6)), "inner is"), (dict(inner=(3, 16)), "inner is"),
                     (dict(inner=(7, 6)), "inner is"), (dict(outer=(4, 20)), "outer is"), (dict(outer=5), "outer is a pair"),
                     (dict(inner=(3,)), "inner is a pair"), (dict(t=torch.zeros(3).double()), "differ in length"),
                     (dict(p=torch.zeros(3)), "differ in length"), (dict(last_t=torch.zeros(13, 17)), "float64"),
                     (dict(p=x, last_t=torch.zeros(13, 17).double()), r"\[2, height, width\]"), (dict(), "GPU only")):
        with pytest.raises(RuntimeError, match=text):
            ops.event_corners(**{**good, **kw})
    assert ops.event_corners_status(torch.tensor([1, 9, 1, 2, 3, 1, 1, 1], dtype=torch.int32)) == dict(
        bad_order=True, n_events=9, n_not_finite=1, n_outside=2, n_border=3, n_no_inner_arc=1, n_no_outer_arc=1, n_corners=1)
