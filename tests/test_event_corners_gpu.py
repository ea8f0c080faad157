"""ramp_event_corners (csrc/corner.hip) against tests/cornerref.py -- one sweep over a surface-of-active-events map and arcs tested
by brute force, restated in numpy without the kernel's sort, searches and threshold sets.  Everything is EXACT: cls, arc, index,
count, corner_count, the state and every status word, bit for bit.  No tolerance in this file: time stamps are only compared.

Most cases call the C entry directly, with a guard band in front of and behind every output, and launch twice."""
import ctypes

import numpy as np
import pytest
import torch

import cornerref as cr
import filterref as fr
import georef
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = cr.H0, cr.W0
KEYS = ("cls", "arc", "index", "count", "corner_count", "status")
_cache = {}


def stream(N, seed=3, distinct=False):
    if (N, seed, distinct) not in _cache:
        _cache[N, seed, distinct] = cr.stream(N, seed=seed, distinct=distinct)
    return _cache[N, seed, distinct]


def entry(x, y, t, p, N, h, w, flags, inner, outer, last_in, last_out, cls, arc, index, count, corner_count, status, ws, ws_bytes):
    from rampvo_amd import _lib
    q = lambda v: v if (v is None or isinstance(v, (int, ctypes.c_void_p))) else _lib.ptr(v)
    return _lib.lib().ramp_event_corners(q(x), q(y), q(t), q(p), N, h, w, flags, inner[0], inner[1], outer[0], outer[1], q(last_in),
                                         q(last_out), q(cls), q(arc), q(index), q(count), q(corner_count), q(status), q(ws), ws_bytes,
                                         _lib.stream())


def call(x, y, t, h=H, w=W, p=None, inner=(3, 6), outer=(4, 8), wide=False, last_t=None, inplace=False):
    """the C entry with every output requested and guarded, launched twice (the second launch's bits are the first's) -> the
    outputs on the host (N == 0 without a state: the last_t the entry leaves untouched is filled in as ops.event_corners does)"""
    from rampvo_amd import _lib
    x, y = np.asarray(x), np.asarray(y)
    integer = x.dtype.kind in "iu"
    xd, yd = (cu(v.astype(np.int32 if integer else np.float32)) for v in (x, y))
    td = cu(np.asarray(t, np.float64))
    N, S = len(td), 1 if p is None else 2
    pd = None if p is None else cu(np.asarray(p, np.int8) if N else np.zeros(1, np.int8))     # (N == 0: p not NULL says two planes)
    nbytes = _lib.lib().ramp_event_corners_ws_bytes(N, h, w, S)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    flags = (_lib.RAMP_CORNER_XY_I32 if integer else 0) | (_lib.RAMP_CORNER_WIDE if wide else 0)
    runs = []
    for _ in range(2):
        bufs = {k: Flat(n, d) for k, (n, d) in dict(cls=(N, torch.uint8), arc=(N * 4, torch.uint8), index=(N, torch.int32),
                                                    count=(1, torch.int32), corner_count=(h * w, torch.int32), status=(8, torch.int32),
                                                    last_t=(S * h * w, torch.float64)).items()}
        at = {k: ctypes.c_void_p(b.address()) for k, b in bufs.items()}          # (an empty view has no pointer)
        last_in = None
        if last_t is not None:
            if inplace:
                bufs["last_t"].t.copy_(cu(np.asarray(last_t, np.float64).reshape(-1)))
                last_in = at["last_t"]
            else:
                last_in = cu(np.asarray(last_t, np.float64))
        rc = entry(xd, yd, td, pd, N, h, w, flags, inner, outer, last_in, at["last_t"], at["cls"], at["arc"], at["index"], at["count"],
                   at["corner_count"], at["status"], ws, nbytes)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert b.intact(), "guard band of " + k
        res = {k: b.t.cpu().numpy() for k, b in bufs.items()}
        if N == 0 and last_t is None:
            assert (res["last_t"] == bufs["last_t"].canary).all()
            res["last_t"] = np.full(S * h * w, np.nan)
        res.update(arc=res["arc"].reshape(N, 4), corner_count=res["corner_count"].reshape(h, w),
                   last_t=res["last_t"].reshape((h, w) if p is None else (2, h, w)))
        runs.append(res)
    same(runs[1], runs[0], "second launch")
    return runs[0]


def same(got, ref, what=""):
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), "%s %s" % (what, k)
    assert got["last_t"].shape == ref["last_t"].shape and georef.same_bits(got["last_t"], ref["last_t"]), what + " last_t"
    assert got["status"][2:].sum() == got["status"][1] or got["status"][0] != 0


def check(x, y, t, h=H, w=W, what="", **kw):
    got = call(x, y, t, h, w, **kw)
    kw.pop("inplace", None)
    same(got, cr.event_corners(x, y, t, h, w, **kw), what)
    return got


# ------------------------------------------------------------------------------------------------ 1. sizes, paths, parameters
@pytest.mark.parametrize("N", (0, 1, 2, 4099))
def test_sizes(N):
    x, y, t, p = stream(4099)
    g = check(x[:N], y[:N], t[:N], p=p[:N])
    check(x[:N], y[:N], t[:N])
    if N == 4099:
        assert g["status"][0] == 0 and (g["status"][4:] > 20).all()


def test_second_trip():
    from rampvo_amd import _lib
    N = _lib.lib().ramp_event_corners_grid_events() + 1
    assert N == 2048 * 256 + 1
    x, y, t, p = stream(N)
    g = check(x, y, t, p=p)
    assert g["status"][1] == N and g["status"][7] > 100 and g["count"][0] == g["status"][7]


@pytest.mark.parametrize("h,w", ((9, 9), (H, W)))
def test_closed_forms(h, w):
    c = ((w - 1) // 2, (h - 1) // 2)
    states = [cr.painted(h, w, c, inner=(5, L)) for L in (2, 3, 6, 7)]
    states += [cr.painted(h, w, c, inner=(0, 3), outer=(17, L)) for L in (3, 4, 8, 9)]
    states += [cr.painted(h, w, c, inner=(14, 4), outer=(18, 5)), cr.painted(h, w, c, inner=(2, 4), rest=2.0),
               cr.painted(h, w, c, inner=(2, 4), outer=(1, 5), rest=np.nan), cr.painted(h, w, c, inner=(2, 4), on=-1.0, rest=np.nan),
               np.full((h, w), np.nan)]
    tie = cr.painted(h, w, c, inner=(2, 4))
    tie[c[1] + cr.INNER[9][1], c[0] + cr.INNER[9][0]] = 2.0
    hole = cr.painted(h, w, c, inner=(2, 7))
    hole[c[1] + cr.INNER[5][1], c[0] + cr.INNER[5][0]] = np.nan
    nested = cr.painted(h, w, c, inner=(6, 6), outer=(10, 8))
    for k in (8, 9, 10):
        nested[c[1] + cr.INNER[k][1], c[0] + cr.INNER[k][0]] = 2.5
    for k in (12, 13, 14, 15):
        nested[c[1] + cr.OUTER[k][1], c[0] + cr.OUTER[k][0]] = 2.5
    got = [check([c[0]], [c[1]], [3.0], h, w, last_t=s, what="state %d" % k) for k, s in enumerate(states + [tie, hole, nested])]
    assert [int(g["cls"][0]) for g in got] == [5, 6, 6, 5, 6, 7, 7, 6, 7, 5, 7, 6, 5, 5, 5, 7]
    assert got[8]["arc"][0].tolist() == [14, 4, 18, 5] and got[-1]["arc"][0].tolist() == [8, 3, 12, 4]
    assert check([c[0]], [c[1]], [3.0], h, w, last_t=nested, inner=(4, 6), outer=(5, 8))["arc"][0].tolist() == [6, 6, 10, 8]
    for L in range(1, 16):                                          # wide: the complements and nothing else
        g = check([c[0]], [c[1]], [3.0], h, w, last_t=cr.painted(h, w, c, inner=(11, L)), wide=True)
        assert (g["cls"][0] == 6) == (3 <= L <= 6 or 10 <= L <= 13), L
    for L in range(1, 20):
        g = check([c[0]], [c[1]], [3.0], h, w, last_t=cr.painted(h, w, c, inner=(0, 3), outer=(3, L)), wide=True)
        assert (g["cls"][0] == 7) == (4 <= L <= 8 or 12 <= L <= 16), L


@pytest.mark.parametrize("k", range(10))
def test_wedge_streams(k):
    name, x, y, t, p = cr.wedges()[k]
    g = check(x, y, t, what=name)
    assert (g["status"][4:] > 0).all() and g["count"][0] == g["status"][7]
    w = check(x, y, t, wide=True, what=name + " wide")
    assert w["status"][7] >= g["status"][7]
    check(x, y, t, p=p, what=name + " p")
    check(x, y, t, p=p, wide=True, what=name + " p wide")
    f = check(x.astype(np.float32), y.astype(np.float32), t, what=name + " integer-valued floats")
    same(f, g, "int32 against integer-valued floats")
    same(call(x + np.float32(0.75), y + np.float32(0.25), t), g, "fractions take no part")


def test_a_wedge_stream_below_zero():
    name, x, y, t, p = cr.wedges(t0=-12 * cr.TICK)[8]
    g = check(x, y, t)
    assert (t < 0).any() and (t == 0).any() and (t > 0).any() and g["status"][7] > 20


@pytest.mark.parametrize("kw", (dict(inner=(1, 15), outer=(1, 19)), dict(inner=(4, 4)), dict(inner=(1, 15), outer=(1, 19), wide=True),
                                dict(inner=(6, 6), outer=(8, 8))))
def test_arc_ranges(kw):
    x, y, t, p = stream(4099)
    g = check(x, y, t, **kw)
    assert g["status"][5] > 0 and g["status"][2:].sum() == 4099
    check(*cr.wedges()[8][1:4], **kw)


def test_border_sensors():
    rng = np.random.default_rng(11)
    N = 600
    t = np.sort(np.round(rng.uniform(0, 1, N) * 1024) / 1024)
    x, y = rng.integers(0, 9, N).astype(np.int32), rng.integers(0, 9, N).astype(np.int32)
    g = check(x, y, t, 9, 9)                                        # one interior pixel
    assert g["status"][4] + ((x == 4) & (y == 4)).sum() == N and g["status"][5] + g["status"][6] + g["status"][7] > 0
    for h, w in ((8, 40), (40, 8)):                                 # all border
        xs, ys = rng.integers(0, w, N).astype(np.int32), rng.integers(0, h, N).astype(np.int32)
        g = check(xs, ys, t, h, w, p=np.where(xs % 2, 1, -1))
        assert g["status"].tolist() == [0, N, 0, 0, N, 0, 0, 0] and np.isfinite(g["last_t"]).sum() > 100


def test_all_events_at_one_time_stamp():
    x, y, t, p = stream(4099)
    g = check(x, y, np.full(4099, 3.25), p=p)
    check(x, y, np.full(4099, 3.25))
    assert g["status"][0] == 0 and g["status"][5] > 1000              # (ties are broken by the index alone)


def test_long_segment():
    """one pixel holds 5,000 of 6,500 events and lies on its neighbours' circles: they search a segment of 5,000"""
    rng = np.random.default_rng(5)
    name, wx, wy, wt, wp = cr.wedges()[8]
    N = 6000
    x, y = rng.integers(0, W, N).astype(np.int32), rng.integers(0, H, N).astype(np.int32)
    big = rng.permutation(N)[:5000]
    x[big], y[big] = 21, 16                                         # three pixels right of the centre
    t = np.round(rng.uniform(0, 20, N)) / 1024
    x, y, t = np.concatenate([x, wx]), np.concatenate([y, wy]), np.concatenate([t, wt])
    order = np.argsort(t, kind="stable")
    g = check(x[order], y[order], t[order])
    assert g["status"][5] > 1000 and g["status"][7] > 0


def test_bad_events():
    rng = np.random.default_rng(8)
    x, y, t, p = (v.copy() for v in stream(4099))
    bad = rng.permutation(4099)[:240]
    x[bad[:30]], y[bad[30:60]], t[bad[60:90]] = np.nan, np.inf, np.nan
    t[bad[90:100]], x[bad[100:110]] = -np.inf, -np.inf
    x[bad[110:150]], x[bad[150:180]], y[bad[180:210]], y[bad[210:240]] = -1.0, float(W), -3.5, H + 0.5
    g = check(x, y, t, p=p)
    assert g["status"][2] == 110 and g["status"][3] == 130 and g["status"][7] > 20
    assert (g["cls"][bad[:110]] == 2).all() and (g["cls"][bad[110:]] == 3).all() and not g["arc"][bad].any()


# ------------------------------------------------------------------------------------------------ 2. state, order
@pytest.mark.parametrize("cut", (1, 4099 // 2, 4098))
def test_state_carry(cut):
    x, y, t, p = stream(4099)
    whole = call(x, y, t, p=p)
    a = check(x[:cut], y[:cut], t[:cut], p=p[:cut])
    b = check(x[cut:], y[cut:], t[cut:], p=p[cut:], last_t=a["last_t"])
    for k in ("cls", "arc"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    assert np.array_equal(a["status"][1:] + b["status"][1:], whole["status"][1:]) and georef.same_bits(b["last_t"], whole["last_t"])
    assert np.array_equal(a["corner_count"] + b["corner_count"], whole["corner_count"])


def test_state_in_place_and_the_empty_call():
    x, y, t, p = stream(4099)
    first = call(x[:2000], y[:2000], t[:2000], p=p[:2000])
    apart = check(x[2000:], y[2000:], t[2000:], p=p[2000:], last_t=first["last_t"])
    inplace = check(x[2000:], y[2000:], t[2000:], p=p[2000:], last_t=first["last_t"], inplace=True)
    same(inplace, apart, "last_t_out == last_t_in")
    for kw in (dict(), dict(inplace=True)):
        e = check(x[:0], y[:0], t[:0], p=p[:0], last_t=first["last_t"], **kw)
        assert georef.same_bits(e["last_t"], first["last_t"]) and not e["corner_count"].any() and not e["status"].any() and e["count"][0] == 0


def test_the_filters_and_the_flows_state_is_the_detectors_state():
    from rampvo_amd import ops
    x, y, t, _ = stream(4099)
    f = ops.event_filter(cu(x[:2000]), cu(y[:2000]), cu(t[:2000]), H, W)
    fl = ops.event_flow(cu(x[:2000]), cu(y[:2000]), cu(t[:2000]), H, W, window_dt=1.0)
    mine = call(x[:2000], y[:2000], t[:2000])["last_t"]
    whole = call(x, y, t)
    for state in (f["last_t"].cpu().numpy(), fl["last_t"].cpu().numpy()):
        assert georef.same_bits(state, mine)
        g = check(x[2000:], y[2000:], t[2000:], last_t=state)
        assert np.array_equal(g["cls"], whole["cls"][2000:]) and np.array_equal(g["arc"], whole["arc"][2000:])


def test_per_cell_sorted_globally_shuffled():
    x, y, t, p = stream(4099, distinct=True)
    perm = cr.shuffle_keeping_cells(x, y, p, np.random.default_rng(2))
    assert (np.diff(t[perm]) < 0).sum() > 1000
    a, g = call(x, y, t, p=p), check(x[perm], y[perm], t[perm], p=p[perm])
    assert g["status"][0] == 0 and a["status"][0] == 0 and a["status"][7] > 20
    assert np.array_equal(g["cls"], a["cls"][perm]) and np.array_equal(g["arc"], a["arc"][perm])
    assert np.array_equal(g["corner_count"], a["corner_count"]) and georef.same_bits(g["last_t"], a["last_t"])


def _bad_order_outputs(g, N, n2=0, n3=0):
    assert g["status"].tolist() == [1, N, n2, n3, 0, 0, 0, 0]
    assert not g["cls"].any() and not g["arc"].any() and (g["index"] == -1).all() and g["count"][0] == 0
    assert not g["corner_count"].any() and np.isnan(g["last_t"]).all()


def test_bad_order():
    x, y, t, p = (v.copy() for v in stream(4099))
    cellkey = (p > 0) * H * W + np.trunc(y).astype(int) * W + np.trunc(x).astype(int)
    x[5], t[5] = np.nan, 1.0
    at = [q for q in np.unique(cellkey) if (cellkey == q).sum() > 3]
    at = np.nonzero(cellkey == at[len(at) // 2])[0]
    at = at[at != 5]
    k = next(k for k in range(1, len(at)) if t[at[k]] > t[at[k - 1]])
    t[at[k]] = np.nextafter(t[at[k - 1]], -1.0)                    # one decrease within one cell
    _bad_order_outputs(check(x, y, t, p=p), 4099, n2=1)
    x, y, t, p = stream(4099)
    state = np.full((2, H, W), np.nan)
    q = int(cellkey[0])
    state.reshape(-1)[q] = np.nextafter(t[0], 1.0)                 # a first event before the state
    _bad_order_outputs(check(x, y, t, p=p, last_t=state), 4099)
    state.reshape(-1)[q] = t[0]
    assert check(x, y, t, p=p, last_t=state)["status"][0] == 0
    state.reshape(-1)[q] = np.nan
    other = q - H * W if q >= H * W else q + H * W
    state.reshape(-1)[other] = t[0] + 1.0                          # the other plane's state is not this cell's
    quiet = cellkey != other
    assert check(x[quiet], y[quiet], t[quiet], p=p[quiet], last_t=state)["status"][0] == 0


def test_integer_outputs():
    x, y, t, p = stream(4099)
    g = check(x, y, t, p=p)
    K = int(g["count"][0])
    assert K == g["status"][7] > 20 and np.array_equal(g["index"][:K], np.nonzero(g["cls"] == 7)[0]) and (g["index"][K:] == -1).all()
    pix = np.trunc(y).astype(int) * W + np.trunc(x).astype(int)
    assert np.array_equal(g["corner_count"].reshape(-1), np.bincount(pix[g["cls"] == 7], minlength=H * W))
    assert g["corner_count"].max() > 1
    nx, ny, nt, _ = cr.noise(4099)
    z = check(nx, ny, nt)                                           # noise alone: no corner at all
    assert z["count"][0] == 0 and (z["index"] == -1).all() and not z["corner_count"].any()


# ------------------------------------------------------------------------------------------------ 3. arguments
def test_every_refusal_touches_nothing():
    from rampvo_amd import _lib
    L = _lib.lib()
    N = 100
    x, y, t, p = (cu(v[:N]) for v in stream(4099))
    bufs = dict(cls=Flat(N, torch.uint8), arc=Flat(N * 4 + 4, torch.uint8), index=Flat(N + 1, torch.int32), count=Flat(2, torch.int32),
                corner_count=Flat(H * W + 1, torch.int32), status=Flat(9, torch.int32), last=Flat(2 * H * W + 1, torch.float64))
    nbytes = L.ramp_event_corners_ws_bytes(N, H, W, 2)
    assert nbytes > L.ramp_event_corners_ws_bytes(N, H, W, 1) > 0
    assert [L.ramp_event_corners_ws_bytes(*a) for a in ((-1, H, W, 1), (N, 0, W, 1), (N, H, W, 0), (N, H, W, 3), (N, 1 << 15, 1 << 15, 1))] == [0] * 5
    ws = Flat(nbytes, torch.uint8, rows=4)
    at = lambda k, off=0: ctypes.c_void_p(bufs[k].address() + off)
    good = dict(x=x, y=y, t=t, p=p, N=N, h=H, w=W, flags=0, inner=(3, 6), outer=(4, 8), last_in=at("last"), last_out=at("last"),
                cls=at("cls"), arc=at("arc"), index=at("index"), count=at("count"), corner_count=at("corner_count"),
                status=at("status"), ws=ctypes.c_void_p(ws.address()), ws_bytes=nbytes)
    snaps = {k: b.snapshot() for k, b in bufs.items()}
    ws_snap = ws.snapshot()
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4
    for change in (dict(N=-1), dict(h=0), dict(w=0), dict(flags=4), dict(flags=-1), dict(inner=(0, 6)), dict(inner=(7, 6)),
                   dict(inner=(3, 16)), dict(outer=(0, 8)), dict(outer=(9, 8)), dict(outer=(4, 20)), dict(status=None), dict(cls=None),
                   dict(x=None), dict(y=None), dict(t=None), dict(ws=None), dict(index=None), dict(count=None),
                   dict(last_in=at("last", 4)), dict(last_out=at("last", 4)), dict(status=at("status", 2)), dict(arc=at("arc", 2)),
                   dict(index=at("index", 2)), dict(count=at("count", 2)), dict(corner_count=at("corner_count", 2)),
                   dict(ws=ctypes.c_void_p(ws.address() + 8))):
        assert entry(**dict(good, **change)) == EINVAL, change
    assert entry(**dict(good, ws_bytes=nbytes - 1)) == EWORKSPACE
    assert entry(**dict(good, N=1 << 31)) == EUNSUPPORTED and entry(**dict(good, h=1 << 15, w=1 << 15)) == EUNSUPPORTED
    assert entry(**dict(good, h=(1 << 30), w=1)) == EUNSUPPORTED                 # 2 H W >= 2^31 - 1, with and without p
    torch.cuda.synchronize()
    assert all(b.unchanged(snaps[k]) for k, b in bufs.items()) and ws.unchanged(ws_snap)
    assert entry(**dict(good, flags=2)) == 0
    assert entry(**dict(good, arc=None, index=None, count=None, corner_count=None, last_in=None, last_out=None)) == 0
    assert entry(**dict(good, N=0, x=None, y=None, t=None, p=None, ws=None, ws_bytes=0, cls=None)) == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values())


# ------------------------------------------------------------------------------------------------ 4. the operator, streams
def _op(x, y, t, p=None, **kw):
    from rampvo_amd import ops
    if kw.get("last_t") is not None:
        kw["last_t"] = cu(np.asarray(kw["last_t"], np.float64))
    out = ops.event_corners(cu(x), cu(y), cu(t), H, W, p=None if p is None else cu(p), want_arc=True, want_map=True, **kw)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert out["corner"].dtype == np.bool_ and np.array_equal(out.pop("corner"), out["cls"] == 7)
    return out


def test_operator():
    from rampvo_amd import ops
    x, y, t, p = stream(4099)
    a = _op(x[:2000], y[:2000], t[:2000], p[:2000])
    same(a, cr.event_corners(x[:2000], y[:2000], t[:2000], H, W, p=p[:2000]), "ops first half")
    b = _op(x[2000:], y[2000:], t[2000:], p[2000:], last_t=a["last_t"], wide=True)
    same(b, cr.event_corners(x[2000:], y[2000:], t[2000:], H, W, p=p[2000:], last_t=a["last_t"], wide=True), "ops second half")
    same(_op(np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64), t, inner=(4, 5), outer=(5, 9)),
         cr.event_corners(np.trunc(x), np.trunc(y), t, H, W, inner=(4, 5), outer=(5, 9)), "integer tensors")
    same(_op(x[:0], y[:0], t[:0], p[:0]), cr.event_corners(x[:0], y[:0], t[:0], H, W, p=p[:0]), "empty")
    same(_op(x[:0], y[:0], t[:0], last_t=a["last_t"][0]), cr.event_corners(x[:0], y[:0], t[:0], H, W, last_t=a["last_t"][0]), "empty with a state")
    d = ops.event_corners(cu(x), cu(y), cu(t), H, W)                # the defaults: the published ranges, index and count
    assert sorted(d) == ["cls", "corner", "count", "index", "last_t", "status"]
    want = cr.event_corners(x, y, t, H, W)
    assert np.array_equal(d["index"].cpu().numpy(), want["index"]) and np.array_equal(d["status"].cpu().numpy(), want["status"])
    assert sorted(ops.event_corners(cu(x), cu(y), cu(t), H, W, want_index=False)) == ["cls", "corner", "last_t", "status"]
    s = ops.event_corners_status(cu(a["status"]))
    assert s == dict(bad_order=False, n_events=2000, n_not_finite=0, n_outside=0, n_border=int(a["status"][4]),
                     n_no_inner_arc=int(a["status"][5]), n_no_outer_arc=int(a["status"][6]), n_corners=int(a["status"][7]))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.event_corners(torch.zeros(3), torch.zeros(3), torch.zeros(3, dtype=torch.float64), H, W)


def test_own_stream():
    """inputs made on a side stream right before the call and overwritten right behind it, the results copied to the host on
    that stream: the bits of the default stream"""
    from rampvo_amd import ops
    x, y, t, p = stream(30011, seed=4)
    want = cr.event_corners(x, y, t, H, W, p=p)
    side = torch.cuda.Stream()
    hosts = [torch.from_numpy(v).pin_memory() for v in (x, y, t, p)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        xd, yd, td, pd = (v.to("cuda", non_blocking=True) for v in hosts)
        out = ops.event_corners(xd, yd, td, H, W, p=pd, want_arc=True, want_map=True)
        xd.fill_(float("nan")), yd.fill_(float("nan")), td.fill_(float("nan")), pd.fill_(0)
        host = {k: v.to("cpu", non_blocking=True) for k, v in out.items()}
        side.synchronize()
    same({k: v.numpy() for k, v in host.items()}, want, "side stream")
    assert want["status"][7] > 100


# ------------------------------------------------------------------------------------------------ 5. tracker
CORNERS = dict(want_arc=True, want_map=True)
TH, TW = 240, 320


def _events(f):
    """wedge runs and noise of the test stream, moved into the tracker's image, in the time of frame f"""
    x, y, t, p = stream(4099)
    return (np.trunc(x).astype(np.int32) + 100, np.trunc(y).astype(np.int32) + 100, 100.0 + 0.5 * (f - 2) + (t - t[0]), p)


def _tracker_queries(slam, f):
    xh, yh, th, ph = _events(f)
    x, y, t, p = cu(xh), cu(yh), cu(th), cu(ph)
    with pytest.raises(RuntimeError, match="unknown parameter"):
        slam.event_corners(x, y, t, window=1.0)
    with pytest.raises(RuntimeError, match="set_event_filter"):
        slam.event_corners(x, y, t, denoise=True)
    cut = 1500
    ref = cr.event_corners(xh, yh, th, TH, TW, p=ph)
    a = slam.event_corners(xh[:cut], yh[:cut], th[:cut], ph[:cut], **CORNERS)   # numpy in (int32: the integer path), numpy out
    b = kit.host(slam.event_corners(x[cut:], y[cut:], t[cut:], p[cut:], as_tensor=True, **CORNERS))
    for k in ("cls", "arc"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), ref[k]), k
    assert ref["status"][7] > 20 and np.array_equal(a["corner_count"] + b["corner_count"], ref["corner_count"])
    assert np.array_equal(np.concatenate([a["corner"], b["corner"]]), ref["cls"] == 7)
    assert georef.same_bits(b["last_t"], ref["last_t"]) and georef.same_bits(kit.host(slam._corner_state), ref["last_t"])
    assert slam._flow_state is None                                 # its own surface, not the flow's
    with pytest.raises(RuntimeError, match="decrease in time"):
        slam.event_corners(xh, yh, th, ph)                          # the same events again: they lie before the surface
    assert georef.same_bits(kit.host(slam._corner_state), ref["last_t"])        # ... which is left as it was
    with pytest.raises(RuntimeError, match="reset_event_corners"):
        slam.event_corners(xh, yh, th)                              # without p: another surface
    alone = slam.event_corners(xh, yh, th, ph, carry=False, **CORNERS)
    assert np.array_equal(alone["arc"], ref["arc"]) and np.array_equal(alone["index"], ref["index"])
    assert georef.same_bits(kit.host(slam._corner_state), ref["last_t"])
    slam.reset_event_corners()
    assert slam._corner_state is None
    # denoise=True: the filter's xy, NaN rows in class 2
    slam.set_event_filter(refractory=0.5 * cr.TICK)
    kept = fr.event_filter(xh, yh, th, TH, TW, refractory=0.5 * cr.TICK)
    want = cr.event_corners(kept["xy"][:, 0], kept["xy"][:, 1], th, TH, TW)
    d = slam.event_corners(x, y, t, denoise=True, carry=False, **CORNERS)
    assert np.array_equal(d["cls"], want["cls"]) and np.array_equal(d["arc"], want["arc"]) and np.array_equal(d["status"], want["status"])
    assert np.array_equal(d["filter_status"], kept["status"]) and d["status"][2] == 4099 - kept["status"][7] > 0
    assert slam._corner_state is None and slam._filter_state is None
    return dict(first=a, second=b, denoised=d)


def test_tracker_device_resident():
    a, c = kit.run_resident(True, lambda slam, f, frame: _tracker_queries(slam, f)), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_after"] and a["resident_at_end"] and c["resident_at_end"]
    kit.same(a["state", kit.T_QUERY + 1], c["state", kit.T_QUERY + 1], "the frame behind the queries")


@torch.no_grad()
def test_tracker_host_driven():
    slam = kit.tracker(False, True)
    frames = kit.frames()
    for f, frame in enumerate(frames):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    _tracker_queries(slam, f)
    kit.feed(slam, f + 1, frames[f + 1])
    assert slam._dev is None
    kit.drop(slam)
