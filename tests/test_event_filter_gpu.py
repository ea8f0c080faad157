"""ramp_event_filter (csrc/filter.hip) against tests/filterref.py -- the textbook sequential filter over a last-time-stamp map,
restated in numpy without the kernel's sort and searches.  Everything is EXACT: keep, index, count, hot, every status word and
the state, bit for bit; xy is the input's bits or NaN; stats equals the restatement's doubles.  No tolerance in this file.

Most cases call the C entry directly, with a guard band in front of and behind every output."""
import ctypes

import numpy as np
import pytest
import torch

import filterref as fr
import georef
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = 13, 17
ALL = dict(fr.STREAM_PARAMS)
_cache = {}


def stream(N, seed=3):
    if (N, seed) not in _cache:
        _cache[N, seed] = fr.stream(N, seed=seed)
    return _cache[N, seed]


def entry(x, y, t, N, h, w, flags, support_dt, refractory, hot_count, hot_sigma, hot_in, last_in, last_out, keep, xy, index,
          count, hot, stats, status, ws, ws_bytes):
    from rampvo_amd import _lib
    p = lambda v: v if (v is None or isinstance(v, (int, ctypes.c_void_p))) else _lib.ptr(v)
    return _lib.lib().ramp_event_filter(p(x), p(y), p(t), N, h, w, flags, support_dt, refractory, hot_count, hot_sigma, p(hot_in),
                                        p(last_in), p(last_out), p(keep), p(xy), p(index), p(count), p(hot), p(stats), p(status),
                                        p(ws), ws_bytes, _lib.stream())


def call(x, y, t, h=H, w=W, support_dt=None, refractory=0.0, hot_count=0, hot_sigma=0.0, hot_mask=None, last_t=None,
         inplace=False):
    """the C entry with every output requested and guarded -> the outputs on the host (N == 0: what the entry left untouched is
    filled in as ops.event_filter fills it in)"""
    from rampvo_amd import _lib
    x, y = np.asarray(x), np.asarray(y)
    integer = x.dtype.kind in "iu"
    xd, yd = (cu(v.astype(np.int32 if integer else np.float32)) for v in (x, y))
    td = cu(np.asarray(t, np.float64))
    N = len(td)
    hot_in = None if hot_mask is None else cu((np.asarray(hot_mask) != 0).astype(np.uint8))
    bufs = {k: Flat(n, d) for k, (n, d) in dict(keep=(N, torch.uint8), xy=(N * 2, torch.float32), index=(N, torch.int32),
                                                count=(1, torch.int64), hot=(h * w, torch.uint8), stats=(4, torch.float64),
                                                status=(8, torch.int32), last_t=(h * w, torch.float64)).items()}
    o = {k: v.t for k, v in bufs.items()}
    at = {k: ctypes.c_void_p(b.address()) for k, b in bufs.items()}          # (an empty view has no pointer)
    last_in = None
    if last_t is not None:
        if inplace:
            o["last_t"].copy_(cu(np.asarray(last_t, np.float64).reshape(-1)))
            last_in = at["last_t"]
        else:
            last_in = cu(np.asarray(last_t, np.float64))
    nbytes = _lib.lib().ramp_event_filter_workspace_bytes(N, h, w)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    rc = entry(xd, yd, td, N, h, w, _lib.RAMP_FILTER_XY_I32 if integer else 0, -1.0 if support_dt is None else support_dt,
               refractory, hot_count, hot_sigma, hot_in, last_in, at["last_t"], at["keep"], at["xy"], at["index"], at["count"],
               at["hot"], at["stats"], at["status"], ws, nbytes)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.intact(), "guard band of " + k
    res = {k: v.cpu().numpy() for k, v in o.items()}
    if N == 0:                                                     # nothing launched: status, count, hot and stats are untouched
        for k in ("status", "count", "hot", "stats") + (() if last_t is not None else ("last_t",)):
            assert (res[k] == bufs[k].canary).all(), k
        res["status"][:], res["count"][:] = 0, 0
        res["hot"] = np.zeros(h * w, np.uint8) if hot_mask is None else (np.asarray(hot_mask) != 0).astype(np.uint8).reshape(-1)
        res["stats"] = np.array([0.0, np.nan, np.nan, np.nan])
        if last_t is None:
            res["last_t"] = np.full(h * w, np.nan)
    res.update(xy=res["xy"].reshape(N, 2), hot=res["hot"].reshape(h, w), last_t=res["last_t"].reshape(h, w), count=int(res["count"][0]))
    return res


def same(got, ref, what=""):
    for k in ("keep", "index", "hot", "status"):
        assert got[k].dtype == ref[k].dtype and np.array_equal(got[k], ref[k]), "%s %s" % (what, k)
    assert got["count"] == ref["count"], what + " count"
    assert georef.same_bits(got["xy"], ref["xy"]), what + " xy"
    assert georef.same_bits(got["stats"], ref["stats"]), "%s stats %s %s" % (what, got["stats"], ref["stats"])
    assert georef.same_bits(got["last_t"], ref["last_t"]), what + " last_t"
    assert got["status"][2:].sum() == got["status"][1] or got["status"][0] != 0


def check(x, y, t, h=H, w=W, what="", **kw):
    got = call(x, y, t, h, w, **kw)
    kw.pop("inplace", None)
    ref = fr.event_filter(x, y, t, h, w, **kw)
    same(got, ref, what)
    return got


# ------------------------------------------------------------------------------------------------ 1. sizes, paths, predicates
@pytest.mark.parametrize("N", (0, 1, 2, 4099))
def test_sizes(N):
    x, y, t = stream(4099)
    g = check(x[:N], y[:N], t[:N], **ALL)
    if N == 4099:
        assert (g["status"][4:] >= 0.05 * N).all() and g["status"][0] == 0      # every class is exercised


def test_second_trip():
    from rampvo_amd import _lib
    N = _lib.lib().ramp_event_filter_grid_events() + 1
    assert N == 2048 * 256 + 1
    g = check(*stream(N), **ALL)
    assert g["status"][1] == N and (g["status"][4:] >= 0.05 * N).all()


def test_64_by_48():
    rng = np.random.default_rng(12)
    N = 30000
    x, y, t = fr.stream(N, seed=6, H=48, W=64, hot_pixels=5)
    x[rng.choice(N, 40)] = 64.5                                    # outside
    g = check(x, y, t, 48, 64, support_dt=ALL["support_dt"] * 8, refractory=ALL["refractory"], hot_sigma=3.0)
    assert g["status"][3] > 0 and (g["status"][4:] > 300).all()


@pytest.mark.parametrize("h,w", ((1, 1), (1, 7)))
def test_degenerate_sensors(h, w):
    rng = np.random.default_rng(h * 10 + w)
    N = 300
    x, y = rng.uniform(0, w, N).astype(np.float32), rng.uniform(0, h, N).astype(np.float32)
    t = np.sort(np.round(rng.uniform(0, 0.05, N) / fr.STREAM_TICK) * fr.STREAM_TICK)
    g = check(x, y, t, h, w, support_dt=4 * fr.STREAM_TICK, refractory=2 * fr.STREAM_TICK)
    assert g["status"][5] > 0 and (g["status"][7] > 0) == (w > 1)              # 1 x 1: no neighbour, no support


def test_int32_coordinates_and_integer_valued_floats():
    x, y, t = stream(4099)
    xi, yi = np.trunc(x).astype(np.int32), np.trunc(y).astype(np.int32)
    a = check(xi, yi, t, what="int32", **ALL)
    b = check(xi.astype(np.float32), yi.astype(np.float32), t, what="float", **ALL)
    same(a, b, "int32 against integer-valued floats")
    c = call(x, y, t, **ALL)                                       # fractions change xy alone
    assert np.array_equal(a["keep"], c["keep"]) and not georef.same_bits(a["xy"], c["xy"])


PREDICATES = dict(activity=dict(support_dt=ALL["support_dt"]), refractory=dict(refractory=ALL["refractory"]),
                  hot_count=dict(hot_count=40), hot_sigma=dict(hot_sigma=2.5), hot_mask=dict(hot_mask="mask"), none={},
                  support_dt_zero=dict(support_dt=0.0), all=dict(ALL, hot_count=60, hot_mask="mask"))


@pytest.mark.parametrize("name", sorted(PREDICATES))
def test_predicates(name):
    kw = dict(PREDICATES[name])
    if kw.get("hot_mask") == "mask":
        kw["hot_mask"] = np.arange(H * W).reshape(H, W) % 7 == 0
    g = check(*stream(4099), **kw)
    s = g["status"]
    assert (s[4] > 0) == any(k.startswith("hot") for k in kw) and (s[5] > 0) == ("refractory" in kw) and (s[6] > 0) == ("support_dt" in kw)
    assert s[7] > 0 and np.isnan(g["stats"][3]) == ("hot_sigma" not in kw)


def test_long_segment():
    """one pixel holds 5,000 of 6,000 events and is not hot: its neighbours search a segment of 5,000"""
    rng = np.random.default_rng(5)
    N = 6000
    x, y = rng.uniform(0, W, N).astype(np.float32), rng.uniform(0, H, N).astype(np.float32)
    big = rng.permutation(N)[:5000]
    x[big], y[big] = 8.5, 6.5
    t = np.sort(np.round(rng.uniform(0, 1.0, N) / fr.STREAM_TICK) * fr.STREAM_TICK)
    g = check(x, y, t, support_dt=8 * fr.STREAM_TICK, refractory=fr.STREAM_TICK)
    assert g["hot"].sum() == 0 and g["status"][5] > 100 and g["status"][6] > 100 and g["status"][7] > 100


def test_all_events_at_one_time_stamp():
    x, y, t = stream(4099)
    g = check(x, y, np.full(4099, 3.25), support_dt=0.0, refractory=1.0)
    assert g["status"][5] > 0 and g["status"][6] > 0 and g["status"][7] > 0


def test_borders_corners_and_bad_events():
    rng = np.random.default_rng(8)
    x, y, t = (v.copy() for v in stream(4099))
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
    g = check(x, y, t, **ALL)
    assert g["status"][2] == 110 and g["status"][3] == 130 and (g["status"][4:] > 100).all()


# ------------------------------------------------------------------------------------------------ 2. state
@pytest.mark.parametrize("cut", (1, 4099 // 2, 4098))
def test_state_carry(cut):
    x, y, t = stream(4099)
    kw = dict(ALL, hot_sigma=0.0, hot_count=0)
    whole = call(x, y, t, **kw)
    a = check(x[:cut], y[:cut], t[:cut], **kw)
    b = check(x[cut:], y[cut:], t[cut:], last_t=a["last_t"], **kw)
    assert np.array_equal(np.concatenate([a["keep"], b["keep"]]), whole["keep"])
    assert georef.same_bits(np.concatenate([a["xy"], b["xy"]]), whole["xy"])
    assert np.array_equal(np.concatenate([a["index"][:a["count"]], b["index"][:b["count"]] + cut]), whole["index"][:whole["count"]])
    assert a["count"] + b["count"] == whole["count"] and (whole["index"][whole["count"]:] == -1).all()
    assert np.array_equal(a["status"][1:] + b["status"][1:], whole["status"][1:]) and whole["status"][0] == 0
    assert georef.same_bits(b["last_t"], whole["last_t"])
    assert np.array_equal(a["hot"], whole["hot"]) and whole["hot"].sum() == 0


def test_state_in_place_and_with_hot_pixels():
    x, y, t = stream(4099)
    first = call(x[:2000], y[:2000], t[:2000], **ALL)
    assert first["hot"].sum() > 0 and np.isnan(first["last_t"]).sum() >= first["hot"].sum()
    apart = check(x[2000:], y[2000:], t[2000:], last_t=first["last_t"], **ALL)
    inplace = check(x[2000:], y[2000:], t[2000:], last_t=first["last_t"], inplace=True, **ALL)
    same(inplace, apart, "last_t_out == last_t_in")
    # N == 0: the state is copied, or left where it is
    assert georef.same_bits(call(x[:0], y[:0], t[:0], last_t=first["last_t"], **ALL)["last_t"], first["last_t"])
    assert georef.same_bits(call(x[:0], y[:0], t[:0], last_t=first["last_t"], inplace=True, **ALL)["last_t"], first["last_t"])


def test_per_pixel_sorted_globally_shuffled():
    x, y, t = stream(4099)
    perm = fr.shuffle_keeping_pixels(x, y, np.random.default_rng(2))
    assert (np.diff(t[perm]) < 0).sum() > 1000
    g = check(x[perm], y[perm], t[perm], **ALL)
    assert g["status"][0] == 0 and (g["status"][4:] > 100).all()


def _bad_order_outputs(g, N, n2=0, n3=0):
    assert g["status"].tolist() == [1, N, n2, n3, 0, 0, 0, 0]
    assert not g["keep"].any() and g["count"] == 0 and (g["index"] == -1).all()
    assert np.isnan(g["xy"]).all() and np.isnan(g["last_t"]).all() and np.isnan(g["stats"]).all()


def test_bad_order():
    x, y, t = (v.copy() for v in stream(4099))
    pix = np.trunc(y).astype(int) * W + np.trunc(x).astype(int)
    x[5], t[5] = np.nan, 1.0
    at = np.nonzero(pix == pix[3000])[0]
    assert len(at) > 3 and t[at[2]] > t[at[1]]
    t[at[2]] = t[at[1]] - fr.STREAM_TICK                          # one decrease within one pixel
    _bad_order_outputs(check(x, y, t, **ALL), 4099, n2=1)
    x, y, t = stream(4099)
    state = np.full((H, W), np.nan)
    q = int(pix[0])
    state[q // W, q % W] = t[0] + fr.STREAM_TICK                   # a first event before the state
    _bad_order_outputs(check(x, y, t, last_t=state, **ALL), 4099)
    state[q // W, q % W] = t[0]
    assert check(x, y, t, last_t=state, **ALL)["status"][0] == 0


def test_a_call_repeats_its_bits():
    x, y, t = stream(30011, seed=4)
    a, b = call(x, y, t, **ALL), call(x, y, t, **ALL)
    same(a, b, "second call")
    assert a["status"][7] > 3000


# ------------------------------------------------------------------------------------------------ 3. arguments
def test_arguments():
    from rampvo_amd import _lib
    L = _lib.lib()
    N = 100
    x, y, t = (cu(v[:N]) for v in stream(4099))
    keep, xy, idx = (torch.empty(s, dtype=d, device="cuda") for s, d in ((N, torch.uint8), ((N + 1, 2), torch.float32), (N, torch.int32)))
    last, stats = torch.full((H * W + 1,), float("nan"), dtype=torch.float64, device="cuda"), torch.empty(5, dtype=torch.float64, device="cuda")
    status, count = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    nbytes = L.ramp_event_filter_workspace_bytes(N, H, W)
    assert nbytes > 0 and L.ramp_event_filter_workspace_bytes(-1, H, W) == 0 and L.ramp_event_filter_workspace_bytes(N, 0, W) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    good = dict(x=x, y=y, t=t, N=N, h=H, w=W, flags=0, support_dt=1e-3, refractory=0.0, hot_count=0, hot_sigma=0.0, hot_in=None,
                last_in=last[:H * W], last_out=last[:H * W], keep=keep, xy=xy[:N], index=idx, count=count, hot=None, stats=stats[:4],
                status=status, ws=ws, ws_bytes=nbytes)
    off = lambda v, nbytes_: ctypes.c_void_p(v.data_ptr() + nbytes_)
    assert entry(**good) == 0
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4
    for change in (dict(N=-1), dict(h=0), dict(w=0), dict(flags=2), dict(flags=-1), dict(keep=None), dict(status=None),
                   dict(x=None), dict(y=None), dict(t=None), dict(ws=None), dict(xy=off(xy, 4)), dict(last_in=off(last, 4)),
                   dict(last_out=off(last, 4)), dict(stats=off(stats, 4)), dict(refractory=-1e-9), dict(refractory=float("inf")),
                   dict(refractory=float("nan")), dict(support_dt=float("inf")), dict(support_dt=float("nan"))):
        assert entry(**dict(good, **change)) == EINVAL, change
    assert entry(**dict(good, support_dt=-5.0)) == 0               # negative: the activity test is off
    assert entry(**dict(good, ws_bytes=nbytes - 1)) == EWORKSPACE
    assert entry(**dict(good, N=1 << 31)) == EUNSUPPORTED and entry(**dict(good, h=1 << 16, w=(1 << 15))) == EUNSUPPORTED
    assert entry(**dict(good, h=2147483647, w=1)) == EUNSUPPORTED
    assert entry(**dict(good, N=0, x=None, y=None, t=None, ws=None, ws_bytes=0)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 4. the operator, streams, consumers
def _op(x, y, t, **kw):
    from rampvo_amd import ops
    for k in ("hot_mask", "last_t"):
        if kw.get(k) is not None:
            kw[k] = cu(np.asarray(kw[k], np.uint8 if k == "hot_mask" else np.float64))
    out = ops.event_filter(cu(x), cu(y), cu(t), H, W, want_index=True, **kw)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    res["count"] = int(res["count"][0])
    return res


def test_operator():
    from rampvo_amd import ops
    x, y, t = stream(4099)
    a = _op(x[:2000], y[:2000], t[:2000], **ALL)
    same(a, fr.event_filter(x[:2000], y[:2000], t[:2000], H, W, **ALL), "ops first half")
    b = _op(x[2000:], y[2000:], t[2000:], last_t=a["last_t"], **ALL)
    same(b, fr.event_filter(x[2000:], y[2000:], t[2000:], H, W, last_t=a["last_t"], **ALL), "ops second half")
    same(_op(np.trunc(x).astype(np.int64), np.trunc(y).astype(np.int64), t, **ALL),
         fr.event_filter(np.trunc(x), np.trunc(y), t, H, W, **ALL), "integer tensors")
    mask = np.arange(H * W).reshape(H, W) % 5 == 0
    same(_op(x[:0], y[:0], t[:0], hot_mask=mask, last_t=a["last_t"]), fr.event_filter(x[:0], y[:0], t[:0], H, W, hot_mask=mask, last_t=a["last_t"]), "empty")
    s = ops.event_filter_status(cu(a["status"]))
    assert s == dict(bad_order=False, n_events=2000, n_not_finite=0, n_outside=0, n_hot=int(a["status"][4]),
                     n_refractory=int(a["status"][5]), n_no_support=int(a["status"][6]), n_kept=a["count"])
    st = ops.event_filter_state(H, W)
    assert st.dtype == torch.float64 and tuple(st.shape) == (H, W) and bool(torch.isnan(st).all())
    lean = ops.event_filter(cu(x), cu(y), cu(t), H, W, want_xy=False, **ALL)
    assert lean["xy"] is None and lean["index"] is None and lean["count"] is None
    assert np.array_equal(lean["keep"].cpu().numpy(), fr.event_filter(x, y, t, H, W, **ALL)["keep"])
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.event_filter(torch.zeros(3), torch.zeros(3), torch.zeros(3, dtype=torch.float64), H, W)


def test_own_stream():
    """inputs made on a side stream right before the call and overwritten right behind it, the results copied to the host on
    that stream: the bits of the default stream"""
    from rampvo_amd import ops
    x, y, t = stream(30011, seed=4)
    want = fr.event_filter(x, y, t, H, W, **ALL)
    side = torch.cuda.Stream()
    xh, yh, th = (torch.from_numpy(v).pin_memory() for v in (x, y, t))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        xd, yd, td = (v.to("cuda", non_blocking=True) for v in (xh, yh, th))
        out = ops.event_filter(xd, yd, td, H, W, want_index=True, **ALL)
        xd.fill_(float("nan")), yd.fill_(float("nan")), td.fill_(float("nan"))
        host = {k: v.to("cpu", non_blocking=True) for k, v in out.items()}
        side.synchronize()
    got = {k: v.numpy() for k, v in host.items()}
    got["count"] = int(got["count"][0])
    same(got, want, "side stream")


def test_consumers_skip_and_count_the_nan_rows():
    from rampvo_amd import ops
    x, y, t = stream(4099)
    p = np.random.default_rng(1).choice([-1, 1], 4099).astype(np.int8)
    xd, yd, td, pd = cu(x), cu(y), cu(t), cu(p)
    f = ops.event_filter(xd, yd, td, H, W, want_index=True, **ALL)
    K = int(f["count"])
    idx = f["index"][:K].long()
    assert 500 < K < 4099 - 500
    a = ops.event_voxel_grid(f["xy"][:, 0], f["xy"][:, 1], td, pd, H, W, num_bins=3, normalize=False, subpixel=True)
    # (the slice's time range is that of its first and last event by position: keep them in the compacted list)
    ends = torch.tensor([0, 4098], device="cuda")
    sel = torch.unique(torch.cat([idx, ends]), sorted=True)
    xs, ys = xd[sel].clone(), yd[sel].clone()
    drop = ~f["keep"][sel].bool()
    xs[drop], ys[drop] = float("nan"), float("nan")
    b = ops.event_voxel_grid(xs, ys, td[sel], pd[sel], H, W, num_bins=3, normalize=False, subpixel=True)
    assert georef.same_bits(a["grid"].cpu().numpy(), b["grid"].cpu().numpy()) and float(a["grid"].abs().sum()) > 0
    assert int(a["status"][2]) == 4099 - K and int(a["status"][1]) == 4099
    cam = ops.camera("radtan", (20.0, 20.0, 8.0, 6.0), (-0.05, 0.01, 0.0, 0.0))
    # one bin: no time range, the compacted events as they are
    a1 = ops.event_voxel_grid(f["xy"][:, 0], f["xy"][:, 1], td, pd, H, W, num_bins=1, normalize=False, subpixel=True)
    b1 = ops.event_voxel_grid(xd[idx], yd[idx], td[idx], pd[idx], H, W, num_bins=1, normalize=False, subpixel=True)
    assert georef.same_bits(a1["grid"].cpu().numpy(), b1["grid"].cpu().numpy()) and int(b1["status"][1]) == K
    r = ops.event_rectify(f["xy"][:, 0], f["xy"][:, 1], cam, H, W)
    assert int(r["status"][2]) == 4099 - K and int(r["status"][1]) == 4099


# ------------------------------------------------------------------------------------------------ 5. tracker
PARAMS = dict(support_dt=0.02, refractory=1e-4, hot_count=20)


def _events(f, n_ev=4000):
    rng = np.random.default_rng(31)
    x, y = rng.integers(100, 160, n_ev).astype(np.int32), rng.integers(100, 140, n_ev).astype(np.int32)
    x[:200], y[:200] = 7, 9                                        # a hot pixel
    t = np.sort(rng.uniform(100.0 + 0.5 * (f - 2), 100.0 + 0.5 * f, n_ev))
    return x, y, t, rng.choice([-1, 1], n_ev).astype(np.int8)


def _tracker_queries(slam, f):
    """everything the tracker tests assert, asked between two frames"""
    from rampvo_amd import ops
    xh, yh, th, ph = _events(f)
    x, y, t, p = cu(xh), cu(yh), cu(th), cu(ph)
    xf, yf = x.float(), y.float()
    before = kit.host(dict(v=slam.event_voxel_grid(xf, yf, t, p, num_bins=3, as_tensor=True),
                           c=slam.compensate_events(xf, yf, t, p, want_xy=True, as_tensor=True)))
    for ask in (lambda: slam.event_voxel_grid(x, y, t, p, denoise=True), lambda: slam.compensate_events(x, y, t, p, denoise=True),
                lambda: slam.event_contrast(x, y, t, p, denoise=True), lambda: slam.align_events(x, y, t, p, iters=1, denoise=True),
                lambda: slam.filter_events(x, y, t)):
        with pytest.raises(RuntimeError, match="set_event_filter"):
            ask()
    with pytest.raises(RuntimeError, match="unknown parameter"):
        slam.set_event_filter(support=1.0)
    slam.set_event_filter(**PARAMS)
    after = kit.host(dict(v=slam.event_voxel_grid(xf, yf, t, p, num_bins=3, as_tensor=True),
                          c=slam.compensate_events(xf, yf, t, p, want_xy=True, as_tensor=True)))
    kit.same(after, before, "denoise=False after set_event_filter")
    # filter_events carries the state across two calls
    cut = 1500
    ref = fr.event_filter(xh, yh, th, 240, 320, **PARAMS)
    a = slam.filter_events(xh[:cut], yh[:cut], th[:cut])                       # numpy in (int32: the integer path), numpy out
    b = kit.host(slam.filter_events(x[cut:], y[cut:], t[cut:], as_tensor=True))
    assert np.array_equal(np.concatenate([a["keep"], b["keep"]]), ref["keep"]) and ref["status"][4] == 200 and ref["status"][7] > 500
    assert georef.same_bits(b["last_t"], ref["last_t"]) and georef.same_bits(kit.host(slam._filter_state), ref["last_t"])
    with pytest.raises(RuntimeError, match="decrease in time"):
        slam.filter_events(xh, yh, th)                                         # the same events again: they lie before the state
    assert georef.same_bits(kit.host(slam._filter_state), ref["last_t"])       # ... which is left as it was
    slam.reset_event_filter()
    assert slam._filter_state is None
    # denoise=True: filtering by hand, then the query
    hand = ops.event_filter(x, y, t, 240, 320, **PARAMS)
    hx, hy = hand["xy"][:, 0], hand["xy"][:, 1]
    want = slam.event_voxel_grid(hx, hy, t, p, num_bins=3, as_tensor=True)
    want["filter_status"] = hand["status"]
    kit.same(kit.host(slam.event_voxel_grid(x, y, t, p, num_bins=3, as_tensor=True, denoise=True)), kit.host(want), "voxel")
    want = slam.compensate_events(hx, hy, t, p, want_xy=True, as_tensor=True)
    want["filter_status"] = hand["status"]
    got = kit.host(slam.compensate_events(x, y, t, p, want_xy=True, as_tensor=True, denoise=True))
    kit.same(got, kit.host(want), "compensate")
    assert got["status"][3] == 4000 - ref["status"][7]                         # the dropped events: the warp's NaN count
    host = slam.compensate_events(xh, yh, th, ph, want_xy=True, denoise=True)
    kit.same(host, got, "numpy form")
    c = slam.event_contrast(x, y, t, p, denoise=True)
    assert np.array_equal(c["filter_status"], ref["status"]) and np.isfinite(c["variance"])
    al = slam.align_events(x, y, t, p, iters=1, denoise=True)
    assert np.array_equal(al["filter_status"], ref["status"]) and np.isfinite(al["variance"])
    assert slam._filter_state is None                                          # the queries read the state, they do not advance it
    return dict(filter=b, compensate=got, contrast=c, host=host)


def test_tracker_device_resident():
    a, c = kit.run_resident(True, lambda slam, f, frame: _tracker_queries(slam, f)), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_after"] and a["resident_at_end"] and c["resident_at_end"]
    kit.same(a["state", kit.T_QUERY + 1], c["state", kit.T_QUERY + 1], "the frame behind the queries")


@torch.no_grad()
def _run_host_driven(query, ready):
    import contextlib
    slam = kit.tracker(False, ready)
    side = torch.cuda.Stream() if ready == "stream" else None
    frames, res = kit.frames(), None
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        for f, frame in enumerate(frames):
            kit.feed(slam, f, frame)
            if slam.is_initialized and slam._n >= 4:
                break
        assert slam.is_initialized and slam._dev is None
        if query:
            res = _tracker_queries(slam, f)
        kit.feed(slam, f + 1, frames[f + 1])
        n = slam._n
        state = dict(n=n, poses=slam.poses_[:n].cpu().numpy(), patches=slam.patches_[:n].cpu().numpy())
        assert slam._dev is None
    del slam
    kit.quiesce()
    return state, res


def test_tracker_host_driven_and_on_its_own_stream():
    (a, ra), (b, _), (c, rc) = _run_host_driven(True, False), _run_host_driven(False, False), _run_host_driven(True, "stream")
    kit.same(a, b, "the frame behind the queries")
    kit.same(c, a, "own stream: the frame behind the queries")
    kit.same(rc, ra, "own stream: the queries")
