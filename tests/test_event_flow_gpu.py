"""ramp_event_flow (csrc/flow.hip) against tests/flowref.py -- one sweep over a surface-of-active-events map and the header's
formulas, restated in numpy without the kernel's sort and searches.  Everything is EXACT: flow, cls, n_used, fit, flow_map,
map_index, the state and every status word, bit for bit.  No tolerance in this file: the definition fixes every rounding.

Most cases call the C entry directly, with a guard band in front of and behind every output, and launch twice."""
import ctypes

import numpy as np
import pytest
import torch

import filterref as fr
import flowref as fl
import georef
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = 13, 17
ALL = dict(fl.STREAM_PARAMS)
KEYS = ("flow", "cls", "n_used", "fit", "flow_map", "map_index", "last_t", "status")
_cache = {}


def stream(N, seed=3):
    if (N, seed) not in _cache:
        _cache[N, seed] = fl.stream(N, seed=seed)
    return _cache[N, seed]


def entry(x, y, t, p, N, h, w, flags, r, window_dt, min_points, refine, outlier_dt, max_speed, last_in, last_out, flow, cls,
          n_used, fit, flow_map, map_index, status, ws, ws_bytes):
    from rampvo_amd import _lib
    q = lambda v: v if (v is None or isinstance(v, (int, ctypes.c_void_p))) else _lib.ptr(v)
    return _lib.lib().ramp_event_flow(q(x), q(y), q(t), q(p), N, h, w, flags, r, window_dt, min_points, refine, outlier_dt,
                                      max_speed, q(last_in), q(last_out), q(flow), q(cls), q(n_used), q(fit), q(flow_map),
                                      q(map_index), q(status), q(ws), ws_bytes, _lib.stream())


def call(x, y, t, h=H, w=W, p=None, radius=2, window_dt=None, min_points=5, refine=1, outlier_dt=None, max_speed=float("inf"),
         last_t=None, inplace=False):
    """the C entry with every output requested and guarded, launched twice (the second launch's bits are the first's) -> the
    outputs on the host (N == 0 without a state: the last_t the entry leaves untouched is filled in as ops.event_flow does)"""
    from rampvo_amd import _lib
    x, y = np.asarray(x), np.asarray(y)
    integer = x.dtype.kind in "iu"
    xd, yd = (cu(v.astype(np.int32 if integer else np.float32)) for v in (x, y))
    td = cu(np.asarray(t, np.float64))
    N, S = len(td), 1 if p is None else 2
    pd = None if p is None else cu(np.asarray(p, np.int8) if N else np.zeros(1, np.int8))     # (N == 0: p not NULL says two planes)
    outlier_dt = window_dt / 4 if outlier_dt is None else outlier_dt
    nbytes = _lib.lib().ramp_event_flow_ws_bytes(N, h, w, S)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        bufs = {k: Flat(n, d) for k, (n, d) in dict(flow=(N * 2, torch.float32), cls=(N, torch.uint8), n_used=(N, torch.uint8),
                                                    fit=(N * 3, torch.float64), flow_map=(2 * h * w, torch.float32),
                                                    map_index=(h * w, torch.int32), status=(8, torch.int32),
                                                    last_t=(S * h * w, torch.float64)).items()}
        at = {k: ctypes.c_void_p(b.address()) for k, b in bufs.items()}          # (an empty view has no pointer)
        last_in = None
        if last_t is not None:
            if inplace:
                bufs["last_t"].t.copy_(cu(np.asarray(last_t, np.float64).reshape(-1)))
                last_in = at["last_t"]
            else:
                last_in = cu(np.asarray(last_t, np.float64))
        rc = entry(xd, yd, td, pd, N, h, w, _lib.RAMP_FLOW_XY_I32 if integer else 0, radius, window_dt, min_points, refine,
                   outlier_dt, max_speed, last_in, at["last_t"], at["flow"], at["cls"], at["n_used"], at["fit"], at["flow_map"],
                   at["map_index"], at["status"], ws, nbytes)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert b.intact(), "guard band of " + k
        res = {k: b.t.cpu().numpy() for k, b in bufs.items()}
        if N == 0 and last_t is None:
            assert (res["last_t"] == bufs["last_t"].canary).all()
            res["last_t"] = np.full(S * h * w, np.nan)
        res.update(flow=res["flow"].reshape(N, 2), fit=res["fit"].reshape(N, 3), flow_map=res["flow_map"].reshape(2, h, w),
                   map_index=res["map_index"].reshape(h, w), last_t=res["last_t"].reshape((h, w) if p is None else (2, h, w)))
        runs.append(res)
    same(runs[1], runs[0], "second launch")
    return runs[0]


def same(got, ref, what=""):
    for k in ("cls", "n_used", "map_index", "status"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), "%s %s" % (what, k)
    for k in ("flow", "fit", "flow_map", "last_t"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape and georef.same_bits(got[k], ref[k]), "%s %s" % (what, k)
    assert got["status"][2:].sum() == got["status"][1] or got["status"][0] != 0


def check(x, y, t, h=H, w=W, what="", **kw):
    got = call(x, y, t, h, w, **kw)
    kw.pop("inplace", None)
    same(got, fl.event_flow(x, y, t, h, w, **kw), what)
    return got


# ------------------------------------------------------------------------------------------------ 1. sizes, paths, parameters
@pytest.mark.parametrize("N", (0, 1, 2, 4099))
def test_sizes(N):
    x, y, t, p = stream(4099)
    g = check(x[:N], y[:N], t[:N], p=p[:N], **ALL)
    check(x[:N], y[:N], t[:N], **ALL)
    if N == 4099:
        assert g["status"][0] == 0 and g["status"][4] > 100 and g["status"][5] > 0 and g["status"][7] > 1000


def test_second_trip():
    from rampvo_amd import _lib
    N = _lib.lib().ramp_event_flow_grid_events() + 1
    assert N == 2048 * 256 + 1
    x, y, t, p = stream(N)
    g = check(x, y, t, p=p, radius=1, **ALL)
    assert g["status"][1] == N and g["status"][7] > 0.3 * N


@pytest.mark.parametrize("refine", (0, 1, 2))
@pytest.mark.parametrize("radius", (1, 2, 3))
def test_radius_and_refine(radius, refine):
    x, y, t, p = stream(4099)
    g = check(x, y, t, p=p, radius=radius, refine=refine, **ALL)
    assert g["status"][7] > 1000 and g["status"][4] > 0
    r0 = fl.event_flow(x, y, t, H, W, p=p, radius=radius, refine=0, **ALL)
    assert (refine == 0) == np.array_equal(g["n_used"], r0["n_used"])          # a pass that drops something


@pytest.mark.parametrize("radius", (1, 2, 3))
def test_min_points_at_both_ends(radius):
    x, y, t, p = stream(4099)
    lo = check(x, y, t, p=p, radius=radius, min_points=3, **ALL)
    hi = check(x, y, t, p=p, radius=radius, min_points=(2 * radius + 1) ** 2, **ALL)
    assert lo["status"][4] < hi["status"][4] and lo["status"][5] > 0


def test_int32_coordinates_and_integer_valued_floats():
    x, y, t, p = stream(4099)
    xi, yi = np.trunc(x).astype(np.int32), np.trunc(y).astype(np.int32)
    a = check(xi, yi, t, p=p, what="int32", **ALL)
    b = check(xi.astype(np.float32), yi.astype(np.float32), t, p=p, what="float", **ALL)
    same(a, b, "int32 against integer-valued floats")
    same(a, call(x, y, t, p=p, **ALL), "fractions take no part")


@pytest.mark.parametrize("diagonal", (False, True))
def test_closed_form_edges(diagonal):
    x, y, t = fl.edge(H, W, diagonal=diagonal, probe=(8, 6))
    g = check(x, y, t, window_dt=10.0, refine=0)
    i = int(np.nonzero((x == 8) & (y == 6))[0][0])
    want = (0.125, 0.125, 4.0, 4.0) if diagonal else (0.25, 0.0, 4.0, 0.0)
    assert (g["fit"][i, 0], g["fit"][i, 1], g["flow"][i, 0], g["flow"][i, 1]) == want and g["fit"][i, 2] == 0 and g["n_used"][i] == 15
    assert g["map_index"][6, 8] == i and tuple(g["flow_map"][:, 6, 8]) == want[2:]


def test_borders_corners_and_bad_events():
    rng = np.random.default_rng(8)
    x, y, t, p = (v.copy() for v in stream(4099))
    ring = rng.permutation(4099)[:1600]
    side = rng.integers(0, 4, 1600)
    x[ring] = np.where(side == 0, 0.5, np.where(side == 1, W - 0.5, x[ring]))
    y[ring] = np.where(side == 2, 0.5, np.where(side == 3, H - 0.5, y[ring]))
    for k, (cx, cy) in enumerate(((0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1))):
        x[ring[k::40][:30]], y[ring[k::40][:30]] = cx + 0.25, cy + 0.75
    bad = rng.permutation(4099)[:240]
    x[bad[:30]], y[bad[30:60]], t[bad[60:90]] = np.nan, np.inf, np.nan
    t[bad[90:100]], x[bad[100:110]] = -np.inf, -np.inf
    x[bad[110:150]], x[bad[150:180]], y[bad[180:210]], y[bad[210:240]] = -1.0, float(W), -3.5, H + 0.5
    for radius in (1, 3):
        g = check(x, y, t, p=p, radius=radius, min_points=3, **ALL)
        assert g["status"][2] == 110 and g["status"][3] == 130 and g["status"][7] > 500
        assert (g["cls"][bad[:110]] == 2).all() and (g["cls"][bad[110:]] == 3).all() and not g["n_used"][bad].any()
        corner = (np.trunc(x) == 0) & (np.trunc(y) == 0) & (g["cls"] >= 4)
        assert corner.sum() >= 20 and 1 < g["n_used"][corner].max() <= (radius + 1) ** 2      # the window clips


def test_a_sensor_of_one_row_is_collinear():
    rng = np.random.default_rng(17)
    N = 300
    x, y = rng.uniform(0, W, N).astype(np.float32), np.zeros(N, np.float32)
    t = np.sort(np.round(rng.uniform(0, 0.05, N) / fl.TICK) * fl.TICK)
    g = check(x, y, t, 1, W, window_dt=64 * fl.TICK, min_points=3)
    assert g["status"][5] > 50 and g["status"][6] == 0 and g["status"][7] == 0


def test_all_events_at_one_time_stamp():
    x, y, t, p = stream(4099)
    g = check(x, y, np.full(4099, 3.25), p=p, window_dt=0.0, outlier_dt=0.0)
    assert g["status"][6] > 1000 and g["status"][7] == 0                       # a surface of equal stamps is flat


def test_long_segment():
    """one pixel holds 5,000 of 6,000 events: its neighbours search a segment of 5,000"""
    rng = np.random.default_rng(5)
    N = 6000
    x, y = rng.uniform(0, W, N).astype(np.float32), rng.uniform(0, H, N).astype(np.float32)
    big = rng.permutation(N)[:5000]
    x[big], y[big] = 8.5, 6.5
    t = np.sort(np.round(rng.uniform(0, 1.0, N) / fl.TICK) * fl.TICK)
    g = check(x, y, t, radius=3, window_dt=4096 * fl.TICK)
    assert g["status"][7] > 1000


def test_max_speed_cuts():
    x, y, t, p = stream(4099)
    free = call(x, y, t, p=p, **ALL)
    speed = np.hypot(*free["flow"][free["cls"] == 7].astype(np.float64).T)
    cut = float(np.median(speed))
    g = check(x, y, t, p=p, max_speed=cut, **ALL)
    assert g["status"][6] > 1000 and g["status"][7] > 1000 and g["status"][6] + g["status"][7] == free["status"][6] + free["status"][7]


# ------------------------------------------------------------------------------------------------ 2. state, order
@pytest.mark.parametrize("cut", (1, 4099 // 2, 4098))
def test_state_carry(cut):
    x, y, t, p = stream(4099)
    whole = call(x, y, t, p=p, **ALL)
    a = check(x[:cut], y[:cut], t[:cut], p=p[:cut], **ALL)
    b = check(x[cut:], y[cut:], t[cut:], p=p[cut:], last_t=a["last_t"], **ALL)
    for k in ("flow", "fit"):
        assert georef.same_bits(np.concatenate([a[k], b[k]]), whole[k]), k
    for k in ("cls", "n_used"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    assert np.array_equal(a["status"][1:] + b["status"][1:], whole["status"][1:]) and georef.same_bits(b["last_t"], whole["last_t"])


def test_state_in_place_and_the_empty_call():
    x, y, t, p = stream(4099)
    first = call(x[:2000], y[:2000], t[:2000], p=p[:2000], **ALL)
    apart = check(x[2000:], y[2000:], t[2000:], p=p[2000:], last_t=first["last_t"], **ALL)
    inplace = check(x[2000:], y[2000:], t[2000:], p=p[2000:], last_t=first["last_t"], inplace=True, **ALL)
    same(inplace, apart, "last_t_out == last_t_in")
    for kw in (dict(), dict(inplace=True)):
        e = check(x[:0], y[:0], t[:0], p=p[:0], last_t=first["last_t"], **kw, **ALL)
        assert georef.same_bits(e["last_t"], first["last_t"]) and (e["map_index"] == -1).all() and not e["status"].any()


def test_the_filters_state_is_the_flows_state():
    from rampvo_amd import ops
    x, y, t, _ = stream(4099)
    f = ops.event_filter(cu(x[:2000]), cu(y[:2000]), cu(t[:2000]), H, W)
    state = f["last_t"].cpu().numpy()
    assert georef.same_bits(state, call(x[:2000], y[:2000], t[:2000], **ALL)["last_t"])
    g = check(x[2000:], y[2000:], t[2000:], last_t=state, **ALL)
    assert georef.same_bits(g["flow"], call(x, y, t, **ALL)["flow"][2000:])


def test_per_cell_sorted_globally_shuffled():
    x, y, t, p = stream(4099)
    perm = fl.shuffle_keeping_cells(x, y, p, np.random.default_rng(2))
    assert (np.diff(t[perm]) < 0).sum() > 1000
    a, g = call(x, y, t, p=p, **ALL), check(x[perm], y[perm], t[perm], p=p[perm], **ALL)
    assert g["status"][0] == 0 and a["status"][0] == 0
    # every event keeps its bits, except where a tie between two cells is now broken the other way
    _, inverse, counts = np.unique(t, return_inverse=True, return_counts=True)
    tie = counts[inverse] > 1
    assert 100 < tie.sum() < 3000
    for k in ("flow", "fit"):
        assert georef.same_bits(g[k][~tie[perm]], a[k][perm][~tie[perm]]), k


def _bad_order_outputs(g, N, n2=0, n3=0):
    assert g["status"].tolist() == [1, N, n2, n3, 0, 0, 0, 0]
    assert not g["cls"].any() and not g["n_used"].any() and (g["map_index"] == -1).all()
    assert all(np.isnan(g[k]).all() for k in ("flow", "fit", "flow_map", "last_t"))


def test_bad_order():
    x, y, t, p = (v.copy() for v in stream(4099))
    cellkey = (p > 0) * H * W + np.trunc(y).astype(int) * W + np.trunc(x).astype(int)
    x[5], t[5] = np.nan, 1.0
    at = np.nonzero(cellkey == cellkey[3000])[0]
    assert len(at) > 3 and t[at[2]] > t[at[1]]
    t[at[2]] = np.nextafter(t[at[1]], -1.0)                        # one decrease within one cell
    _bad_order_outputs(check(x, y, t, p=p, **ALL), 4099, n2=1)
    x, y, t, p = stream(4099)
    state = np.full((2, H, W), np.nan)
    q = int(cellkey[0])
    state.reshape(-1)[q] = np.nextafter(t[0], 1.0)                 # a first event before the state
    _bad_order_outputs(check(x, y, t, p=p, last_t=state, **ALL), 4099)
    state.reshape(-1)[q] = t[0]
    assert check(x, y, t, p=p, last_t=state, **ALL)["status"][0] == 0
    state.reshape(-1)[q] = np.nan
    state.reshape(-1)[q - H * W if q >= H * W else q + H * W] = t[0] + 1.0     # the other plane's state is not this cell's
    quiet = cellkey != (q - H * W if q >= H * W else q + H * W)
    assert check(x[quiet], y[quiet], t[quiet], p=p[quiet], last_t=state, **ALL)["status"][0] == 0


# ------------------------------------------------------------------------------------------------ 3. arguments
def test_every_refusal_touches_nothing():
    from rampvo_amd import _lib
    L = _lib.lib()
    N = 100
    x, y, t, p = (cu(v[:N]) for v in stream(4099))
    bufs = dict(flow=Flat(N * 2 + 2, torch.float32), cls=Flat(N, torch.uint8), n_used=Flat(N, torch.uint8), fit=Flat(N * 3 + 1, torch.float64),
                flow_map=Flat(2 * H * W + 1, torch.float32), map_index=Flat(H * W + 1, torch.int32), status=Flat(9, torch.int32),
                last=Flat(2 * H * W + 1, torch.float64))
    nbytes = L.ramp_event_flow_ws_bytes(N, H, W, 2)
    assert nbytes > L.ramp_event_flow_ws_bytes(N, H, W, 1) > 0
    assert [L.ramp_event_flow_ws_bytes(*a) for a in ((-1, H, W, 1), (N, 0, W, 1), (N, H, W, 0), (N, H, W, 3), (N, 1 << 15, 1 << 15, 1))] == [0] * 5
    ws = Flat(nbytes, torch.uint8, rows=4)
    at = lambda k, off=0: ctypes.c_void_p(bufs[k].address() + off)
    good = dict(x=x, y=y, t=t, p=p, N=N, h=H, w=W, flags=0, r=2, window_dt=1e-3, min_points=5, refine=1, outlier_dt=1e-4,
                max_speed=float("inf"), last_in=at("last"), last_out=at("last"), flow=at("flow"), cls=at("cls"), n_used=at("n_used"),
                fit=at("fit"), flow_map=at("flow_map"), map_index=at("map_index"), status=at("status"),
                ws=ctypes.c_void_p(ws.address()), ws_bytes=nbytes)
    snaps = {k: b.snapshot() for k, b in bufs.items()}
    ws_snap = ws.snapshot()
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4
    nan = float("nan")
    for change in (dict(N=-1), dict(h=0), dict(w=0), dict(flags=2), dict(flags=-1), dict(r=0), dict(r=4), dict(min_points=2),
                   dict(min_points=26), dict(r=1, min_points=10), dict(refine=-1), dict(refine=3), dict(window_dt=-1e-9),
                   dict(window_dt=nan), dict(outlier_dt=-1.0), dict(outlier_dt=nan), dict(max_speed=nan), dict(max_speed=0.0),
                   dict(max_speed=-1.0), dict(status=None), dict(flow=None), dict(x=None), dict(y=None), dict(t=None), dict(ws=None),
                   dict(flow_map=None), dict(map_index=None), dict(flow=at("flow", 4)), dict(fit=at("fit", 4)),
                   dict(last_in=at("last", 4)), dict(last_out=at("last", 4)), dict(status=at("status", 2)),
                   dict(flow_map=at("flow_map", 2)), dict(map_index=at("map_index", 2)), dict(ws=ctypes.c_void_p(ws.address() + 8))):
        assert entry(**dict(good, **change)) == EINVAL, change
    assert entry(**dict(good, ws_bytes=nbytes - 1)) == EWORKSPACE
    assert entry(**dict(good, N=1 << 31)) == EUNSUPPORTED and entry(**dict(good, h=1 << 15, w=1 << 15)) == EUNSUPPORTED
    assert entry(**dict(good, h=(1 << 30), w=1)) == EUNSUPPORTED                 # 2 H W >= 2^31 - 1, with and without p
    torch.cuda.synchronize()
    assert all(b.unchanged(snaps[k]) for k, b in bufs.items()) and ws.unchanged(ws_snap)
    assert entry(**dict(good, max_speed=float("inf"), window_dt=float("inf"))) == 0
    assert entry(**dict(good, N=0, x=None, y=None, t=None, p=None, ws=None, ws_bytes=0, flow=None)) == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values())


# ------------------------------------------------------------------------------------------------ 4. the operator, streams
def _op(x, y, t, p=None, **kw):
    from rampvo_amd import ops
    if kw.get("last_t") is not None:
        kw["last_t"] = cu(np.asarray(kw["last_t"], np.float64))
    out = ops.event_flow(cu(x), cu(y), cu(t), H, W, p=None if p is None else cu(p), want_map=True, want_fit=True, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_operator():
    from rampvo_amd import ops
    x, y, t, p = stream(4099)
    a = _op(x[:2000], y[:2000], t[:2000], p[:2000], **ALL)
    same(a, fl.event_flow(x[:2000], y[:2000], t[:2000], H, W, p=p[:2000], **ALL), "ops first half")
    b = _op(x[2000:], y[2000:], t[2000:], p[2000:], last_t=a["last_t"], **ALL)
    same(b, fl.event_flow(x[2000:], y[2000:], t[2000:], H, W, p=p[2000:], last_t=a["last_t"], **ALL), "ops second half")
    same(_op(np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64), t, **ALL), fl.event_flow(np.trunc(x), np.trunc(y), t, H, W, **ALL), "integer tensors")
    same(_op(x[:0], y[:0], t[:0], p[:0], **ALL), fl.event_flow(x[:0], y[:0], t[:0], H, W, p=p[:0], **ALL), "empty")
    same(_op(x[:0], y[:0], t[:0], last_t=a["last_t"][0], **ALL), fl.event_flow(x[:0], y[:0], t[:0], H, W, last_t=a["last_t"][0], **ALL), "empty with a state")
    # the defaults: radius 2, min_points 5, refine 1, outlier_dt = window_dt / 4, no speed limit
    d = ops.event_flow(cu(x), cu(y), cu(t), H, W, window_dt=ALL["window_dt"])
    assert sorted(d) == ["cls", "flow", "last_t", "n_used", "status"]
    want = fl.event_flow(x, y, t, H, W, window_dt=ALL["window_dt"])
    assert georef.same_bits(d["flow"].cpu().numpy(), want["flow"]) and np.array_equal(d["status"].cpu().numpy(), want["status"])
    s = ops.event_flow_status(cu(a["status"]))
    assert s == dict(bad_order=False, n_events=2000, n_not_finite=0, n_outside=0, n_few_points=int(a["status"][4]),
                     n_collinear=int(a["status"][5]), n_flat=int(a["status"][6]), n_valid=int(a["status"][7]))
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.event_flow(torch.zeros(3), torch.zeros(3), torch.zeros(3, dtype=torch.float64), H, W, window_dt=1.0)


def test_own_stream():
    """inputs made on a side stream right before the call and overwritten right behind it, the results copied to the host on
    that stream: the bits of the default stream"""
    from rampvo_amd import ops
    x, y, t, p = stream(30011, seed=4)
    want = fl.event_flow(x, y, t, H, W, p=p, **ALL)
    side = torch.cuda.Stream()
    hosts = [torch.from_numpy(v).pin_memory() for v in (x, y, t, p)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        xd, yd, td, pd = (v.to("cuda", non_blocking=True) for v in hosts)
        out = ops.event_flow(xd, yd, td, H, W, p=pd, want_map=True, want_fit=True, **ALL)
        xd.fill_(float("nan")), yd.fill_(float("nan")), td.fill_(float("nan")), pd.fill_(0)
        host = {k: v.to("cpu", non_blocking=True) for k, v in out.items()}
        side.synchronize()
    same({k: v.numpy() for k, v in host.items()}, want, "side stream")
    assert want["status"][7] > 10000


# ------------------------------------------------------------------------------------------------ 5. tracker
FLOW = dict(window_dt=0.05, radius=2, want_map=True, want_fit=True)


def _events(f, n_ev=4000):
    rng = np.random.default_rng(31)
    x, y = rng.integers(100, 130, n_ev).astype(np.int32), rng.integers(100, 120, n_ev).astype(np.int32)
    t = np.sort(rng.uniform(100.0 + 0.5 * (f - 2), 100.0 + 0.5 * f, n_ev))
    return x, y, t, rng.choice([-1, 1], n_ev).astype(np.int8)


def _tracker_queries(slam, f):
    xh, yh, th, ph = _events(f)
    x, y, t, p = cu(xh), cu(yh), cu(th), cu(ph)
    with pytest.raises(RuntimeError, match="unknown parameter"):
        slam.event_flow(x, y, t, window=1.0)
    with pytest.raises(RuntimeError, match="set_event_filter"):
        slam.event_flow(x, y, t, denoise=True, **FLOW)
    cut = 1500
    ref = fl.event_flow(xh, yh, th, 240, 320, p=ph, window_dt=0.05)
    a = slam.event_flow(xh[:cut], yh[:cut], th[:cut], ph[:cut], **FLOW)         # numpy in (int32: the integer path), numpy out
    b = kit.host(slam.event_flow(x[cut:], y[cut:], t[cut:], p[cut:], as_tensor=True, **FLOW))
    assert georef.same_bits(np.concatenate([a["flow"], b["flow"]]), ref["flow"]) and ref["status"][7] > 500
    assert georef.same_bits(np.concatenate([a["fit"], b["fit"]]), ref["fit"])
    assert georef.same_bits(b["last_t"], ref["last_t"]) and georef.same_bits(kit.host(slam._flow_state), ref["last_t"])
    with pytest.raises(RuntimeError, match="decrease in time"):
        slam.event_flow(xh, yh, th, ph, **FLOW)                                 # the same events again: they lie before the surface
    assert georef.same_bits(kit.host(slam._flow_state), ref["last_t"])          # ... which is left as it was
    with pytest.raises(RuntimeError, match="reset_event_flow"):
        slam.event_flow(xh, yh, th, **FLOW)                                     # without p: another surface
    alone = slam.event_flow(xh, yh, th, ph, carry=False, **FLOW)
    assert georef.same_bits(alone["flow"], ref["flow"]) and georef.same_bits(kit.host(slam._flow_state), ref["last_t"])
    slam.reset_event_flow()
    assert slam._flow_state is None
    # denoise=True: the filter's xy, NaN rows in class 2
    slam.set_event_filter(support_dt=0.02)
    kept = fr.event_filter(xh, yh, th, 240, 320, support_dt=0.02)
    want = fl.event_flow(kept["xy"][:, 0], kept["xy"][:, 1], th, 240, 320, window_dt=0.05)
    d = slam.event_flow(x, y, t, denoise=True, carry=False, **FLOW)
    assert georef.same_bits(d["flow"], want["flow"]) and np.array_equal(d["status"], want["status"])
    assert np.array_equal(d["filter_status"], kept["status"]) and d["status"][2] == 4000 - kept["status"][7] > 0
    assert slam._flow_state is None and slam._filter_state is None
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
