"""ramp_event_landmarks (csrc/landmark.hip) against tests/landmarkref.py.

EXACT, bit for bit: lm_track, n_obs, count, ev_landmark, span, cls and every status word, NaN exactly where the definition says
NaN, the bad_times path, the refusals, a repeated launch, a shuffled stream, a side stream.

TO A BOUND: ``ev_ray`` against the float64 pose kit per observation, by the rule of test_event_warp_gpu.py:
georef.bound(PIXEL_FLOOR x the largest |word|, the fp32 formulas' own error).  ``point``, ``cov``, ``rms``, ``parallax`` and
``ev_residual`` against the restatement run on the call's OWN ``ev_ray`` (and the rotations of ``ops.se3_interp`` at the same
time stamps, which are the call's bits: the centres say so): one fp32 rounding of the result plus 64 n 2^-53 cond(H) scale
(landmarkref.compare).  Measured on MI355X: see the README's "Event landmarks".

Most cases call the C entry directly, with a guard band around every output, and launch twice."""
import ctypes

import numpy as np
import pytest
import torch

import cornerref as cr
import georef
import landmarkref as lr
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

_cases = {}
RATIOS = {}


def cases():
    if not _cases:
        _cases.update(lr.cases())
    return _cases


def entry(x, y, t, track, N, knots, times, T, K, flags, min_obs, refine, min_parallax, max_rms, sigma_px, max_landmarks, lm_track, point,
          cov, n_obs, cls, rms, parallax, span, count, index, residual, rays, status, ws, ws_bytes):
    from rampvo_amd import _lib
    q = lambda v: v if (v is None or isinstance(v, (int, ctypes.c_void_p))) else _lib.ptr(v)
    return _lib.lib().ramp_event_landmarks(q(x), q(y), q(t), q(track), N, q(knots), q(times), T, q(K), flags, min_obs, refine, min_parallax,
                                           max_rms, sigma_px, max_landmarks, q(lm_track), q(point), q(cov), q(n_obs), q(cls), q(rms),
                                           q(parallax), q(span), q(count), q(index), q(residual), q(rays), q(status), q(ws), ws_bytes,
                                           _lib.stream())


def outputs(N, L):
    return dict(track=(L, torch.int64), point=(L * 3, torch.float32), cov=(L * 6, torch.float32), n_obs=(L, torch.int32),
                cls=(L, torch.uint8), rms=(L, torch.float32), parallax=(L, torch.float32), span=(L * 2, torch.float64),
                count=(1, torch.int32), index=(N, torch.int32), residual=(N * 2, torch.float32), rays=(N * 6, torch.float32),
                status=(8, torch.int32))


def call(sc, min_obs=3, refine=2, min_parallax=0.02, max_rms=2.0, sigma_px=1.0, max_landmarks=None, extrapolate=False, optional=True):
    """the C entry with every output guarded, launched twice (the second launch's bits are the first's) -> the outputs on the
    host, the per-landmark ones cut to count; rows behind count still hold the canary"""
    from rampvo_amd import _lib
    xd, yd, td, kd = cu(sc["x"].astype(np.float32)), cu(sc["y"].astype(np.float32)), cu(sc["t"]), cu(sc["track"])
    knots, times, K = cu(sc["knots"]), cu(sc["times"]), cu(np.asarray(sc["K"], np.float32))
    N, T = len(sc["t"]), len(sc["times"])
    L = max(1, min(N, 2 ** 20)) if max_landmarks is None else max_landmarks
    nbytes = _lib.lib().ramp_event_landmarks_ws_bytes(N, T, L)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        bufs = {k: Flat(n, d) for k, (n, d) in outputs(N, L).items()}
        at = {k: ctypes.c_void_p(b.address()) for k, b in bufs.items()}
        opt = lambda k: at[k] if optional and N else None
        rc = entry(xd, yd, td, kd, N, knots, times, T, K, _lib.RAMP_INTERP_EXTRAPOLATE if extrapolate else 0, min_obs, refine, min_parallax,
                   max_rms, sigma_px, L, at["track"], at["point"], at["cov"], at["n_obs"], at["cls"], at["rms"], at["parallax"], at["span"],
                   at["count"], opt("index"), opt("residual"), opt("rays"), at["status"], ws, nbytes)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert b.intact(), "guard band of " + k
        res = {k: b.t.cpu().numpy() for k, b in bufs.items()}
        k = int(res["count"][0])
        assert 0 <= k <= L
        for name, width in (("track", 1), ("point", 3), ("cov", 6), ("n_obs", 1), ("cls", 1), ("rms", 1), ("parallax", 1), ("span", 2)):
            tail = res[name][k * width:]
            assert (tail == bufs[name].canary).all(), "rows behind count of " + name
            res[name] = res[name][:k * width].reshape((k, width) if width > 1 else (k,))
        if not (optional and N):
            for name in ("index", "residual", "rays"):
                assert (res.pop(name) == bufs[name].canary).all()
        else:
            res.update(residual=res["residual"].reshape(N, 2), rays=res["rays"].reshape(N, 6))
        runs.append(res)
    for k in runs[0]:
        assert georef.same_bits(runs[0][k], runs[1][k]) if runs[0][k].dtype.itemsize >= 4 else np.array_equal(runs[0][k], runs[1][k]), k
    return runs[0]


def quats(sc, extrapolate):
    """the rotations (and centres) of ops.se3_interp at the events' time stamps: the call's own bits"""
    from rampvo_amd import ops
    t = np.where(np.isfinite(sc["t"]), sc["t"], sc["times"][0])
    poses, _, _ = ops.se3_interp(cu(sc["knots"]), cu(sc["times"]), cu(t), extrapolate=extrapolate)
    return poses.cpu().numpy()


def check(sc, kw, what=""):
    got = call(sc, **kw)
    ex = kw.get("extrapolate", False)
    if not len(sc["t"]):
        ref = lr.event_landmarks(sc["x"], sc["y"], sc["t"], sc["track"], sc["knots"], sc["times"], sc["K"], want_cond=True, **kw)
        cmp = lr.compare(got, ref)
        assert not cmp["exact"] and not cmp["nan"] and not got["status"].any(), (what, cmp)
        return got, ref
    poses = quats(sc, ex)
    obs = lr.observations(sc["x"], sc["y"], sc["t"], sc["track"], sc["times"], ex) == 4
    if got["status"][0] == 0:
        assert georef.same_bits(got["rays"][obs, :3], poses[obs, :3]), what + ": the centres are ops.se3_interp's bits"
        assert np.isnan(got["rays"][~obs]).all() and np.isfinite(got["rays"][obs]).all()
        r64, _ = lr.event_rays(sc["x"], sc["y"], sc["t"], sc["knots"], sc["times"], sc["K"], ex, np.float64)
        r32, _ = lr.event_rays(sc["x"], sc["y"], sc["t"], sc["knots"], sc["times"], sc["K"], ex, np.float32)
        if obs.any():
            err, env = georef.max_err(got["rays"][obs], r64[obs]), georef.max_err(r32[obs], r64[obs])
            bound = georef.bound(georef.PIXEL_FLOOR * float(np.abs(r64[obs]).max()), env)
            print("%s: ev_ray err %.3g env %.3g bound %.3g" % (what, err, env, bound))
            assert err <= bound, (what, err, bound)
    ref = lr.event_landmarks(sc["x"], sc["y"], sc["t"], sc["track"], sc["knots"], sc["times"], sc["K"], rays=got["rays"],
                             quat=poses[:, 3:], want_cond=True, **kw)
    cmp = lr.compare(got, ref)
    RATIOS[what] = cmp["ratio"]
    print("%s: largest err / bound %.3g, classes %s" % (what, cmp["ratio"], np.bincount(ref["cls"], minlength=8).tolist()))
    assert not cmp["exact"] and not cmp["nan"], (what, cmp)
    assert cmp["ratio"] <= 1.0, (what, cmp["ratio"])
    assert got["status"][1:5].sum() == len(sc["t"]) or got["status"][0] != 0
    return got, ref


def take(sc, sel):
    return dict(sc, x=sc["x"][sel], y=sc["y"][sel], t=sc["t"][sel], track=sc["track"][sel])


# ------------------------------------------------------------------------------------------------ 1. sizes, paths, parameters
@pytest.mark.parametrize("name", list(lr.cases()))
def test_streams(name):
    """tracks of 1, 2, 3, 63, 64, 65, 129 and 5,000 observations; 1, 65 and 1,000 tracks; T = 1, 2, 9 and 4,097 knots (the LDS /
    global switch of the knot times); max_landmarks below the track count; refine 0, 1, 2, 4; extrapolate"""
    sc, kw = cases()[name]
    got, ref = check(sc, kw, name)
    if name == "edges T=9":
        assert sorted(ref["n_obs"].tolist()) == sorted(lr.EDGE_SIZES) and (ref["cls"] == 7).sum() == 6 and got["status"][7] == 6
    if name == "1000 tracks, cut":
        assert got["status"][5:].tolist() == [1000, 300, 700] and got["count"][0] == 700 and (got["index"] == -1).sum() > 0
    if name == "4097 knots":
        assert len(sc["times"]) == 4097 and got["status"][7] == 3


@pytest.mark.parametrize("N", (0, 1, 2, 4099))
def test_sizes(N):
    sc, kw = cases()["1000 tracks, cut"]
    sub = take(sc, slice(0, N))
    got, _ = check(sub, dict(kw, max_landmarks=None), "N=%d" % N)
    assert got["status"][4] == N
    bare = call(sub, optional=False, **dict(kw, max_landmarks=None))             # without the optional outputs: the same landmarks
    for k in bare:
        assert georef.same_bits(bare[k], got[k]) if got[k].dtype.itemsize >= 4 else np.array_equal(bare[k], got[k]), k


def test_no_tracks_and_second_trip():
    from rampvo_amd import _lib
    N = _lib.lib().ramp_event_landmarks_grid_events() + 1
    assert N == 2048 * 256 + 1
    sc, kw = cases()["65 tracks"]
    rep = np.arange(N) % len(sc["t"])
    big = take(sc, rep)
    big["t"] = np.where(np.isfinite(big["t"]), big["t"] + 1e-9 * (np.arange(N) // len(sc["t"])), big["t"])
    none = dict(big, track=np.full(N, -1, np.int64))
    got = call(none, **kw)
    assert got["status"].tolist() == [0, N, 0, 0, 0, 0, 0, 0] and got["count"][0] == 0 and (got["index"] == -1).all()
    assert np.isnan(got["rays"]).all() and np.isnan(got["residual"]).all()
    g, ref = check(big, dict(kw, max_landmarks=64), "second trip")
    assert g["status"][5] == 65 and g["status"][6] == 1 and ref["n_obs"].max() > 5000


def test_shuffled_across_tracks():
    """distinct time stamps: every per-landmark output keeps its bits under any order of the events"""
    sc, kw = cases()["edges T=9"]
    sc = dict(sc, t=np.where(np.isfinite(sc["t"]), sc["t"] + np.arange(len(sc["t"])) * 2.0 ** -30, sc["t"]))
    keep = np.isfinite(sc["t"])
    assert len(np.unique(sc["t"][keep])) == keep.sum()
    perm = np.random.default_rng(5).permutation(len(sc["t"]))
    a, b = call(sc, **kw), call(take(sc, perm), **kw)
    for k in ("track", "point", "cov", "n_obs", "cls", "rms", "parallax", "span", "count", "status"):
        assert georef.same_bits(a[k], b[k]) if a[k].dtype.itemsize >= 4 else np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["index"], a["index"][perm]) and georef.same_bits(b["residual"], a["residual"][perm])
    assert georef.same_bits(b["rays"], a["rays"][perm]) and a["status"][7] == 6


def test_bad_times():
    sc, kw = cases()["65 tracks"]
    N = len(sc["t"])
    for change in (lambda t: np.concatenate([t[:4], [t[3] - 0.25], t[5:]]), lambda t: np.concatenate([t[:4], [np.nan], t[5:]]),
                   lambda t: np.concatenate([t[:-1], [np.inf]])):
        bad = dict(sc, times=change(sc["times"]))
        got = call(bad, **kw)
        ref = lr.event_landmarks(bad["x"], bad["y"], bad["t"], bad["track"], bad["knots"], bad["times"], bad["K"], **kw)
        assert got["status"][0] == 1 and np.array_equal(got["status"], ref["status"]) and got["status"][4:].tolist() == [0, 0, 0, 0]
        assert got["count"][0] == 0 and (got["index"] == -1).all() and np.isnan(got["rays"]).all() and np.isnan(got["residual"]).all()
        assert got["status"][1:4].sum() <= N


# ------------------------------------------------------------------------------------------------ 2. arguments
def test_every_refusal_touches_nothing():
    from rampvo_amd import _lib
    L_ = _lib.lib()
    sc, kw = cases()["65 tracks"]
    N, T, L = 100, len(sc["times"]), 50
    x, y, t, track = cu(sc["x"][:N]), cu(sc["y"][:N]), cu(sc["t"][:N]), cu(sc["track"][:N])
    knots, times, K = cu(sc["knots"]), cu(sc["times"]), cu(sc["K"])
    bufs = {k: Flat(n + 2, d) for k, (n, d) in outputs(N, L).items()}
    nbytes = L_.ramp_event_landmarks_ws_bytes(N, T, L)
    assert nbytes > 0 and nbytes % 256 == 0
    assert [L_.ramp_event_landmarks_ws_bytes(*a) for a in ((-1, T, L), (N, 0, L), (N, T, 0), (1 << 31, T, L))] == [0] * 4
    ws = Flat(nbytes, torch.uint8, rows=4)
    at = lambda k, off=0: ctypes.c_void_p(bufs[k].address() + off)
    good = dict(x=x, y=y, t=t, track=track, N=N, knots=knots, times=times, T=T, K=K, flags=0, min_obs=3, refine=2, min_parallax=0.02,
                max_rms=2.0, sigma_px=1.0, max_landmarks=L, lm_track=at("track"), point=at("point"), cov=at("cov"), n_obs=at("n_obs"),
                cls=at("cls"), rms=at("rms"), parallax=at("parallax"), span=at("span"), count=at("count"), index=at("index"),
                residual=at("residual"), rays=at("rays"), status=at("status"), ws=ctypes.c_void_p(ws.address()), ws_bytes=nbytes)
    snaps = {k: b.snapshot() for k, b in bufs.items()}
    ws_snap = ws.snapshot()
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4
    nan, inf = float("nan"), float("inf")
    for change in (dict(N=-1), dict(T=0), dict(flags=2), dict(flags=-1), dict(min_obs=1), dict(refine=-1), dict(refine=5),
                   dict(min_parallax=-1.0), dict(min_parallax=nan), dict(max_rms=inf), dict(max_rms=-0.5), dict(sigma_px=nan),
                   dict(sigma_px=-1.0), dict(max_landmarks=0), dict(x=None), dict(y=None), dict(t=None), dict(track=None), dict(knots=None),
                   dict(times=None), dict(K=None), dict(ws=None), dict(lm_track=None), dict(point=None), dict(cov=None), dict(n_obs=None),
                   dict(cls=None), dict(rms=None), dict(parallax=None), dict(span=None), dict(count=None), dict(status=None),
                   dict(lm_track=at("track", 4)), dict(span=at("span", 4)), dict(point=at("point", 2)), dict(cov=at("cov", 2)),
                   dict(n_obs=at("n_obs", 2)), dict(rms=at("rms", 2)), dict(parallax=at("parallax", 2)), dict(count=at("count", 2)),
                   dict(index=at("index", 2)), dict(residual=at("residual", 2)), dict(rays=at("rays", 2)), dict(status=at("status", 2)),
                   dict(ws=ctypes.c_void_p(ws.address() + 8))):
        assert entry(**dict(good, **change)) == EINVAL, change
    assert entry(**dict(good, ws_bytes=nbytes - 1)) == EWORKSPACE and entry(**dict(good, N=1 << 31)) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert all(b.unchanged(snaps[k]) for k, b in bufs.items()) and ws.unchanged(ws_snap)
    assert entry(**good) == 0 and entry(**dict(good, index=None, residual=None, rays=None, flags=1, refine=0, min_parallax=0.0)) == 0
    assert entry(**dict(good, N=0, x=None, y=None, t=None, track=None, knots=None, times=None, K=None, ws=None, ws_bytes=0)) == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values())
    assert bufs["count"].t[0] == 0 and not bufs["status"].t[:8].any()


# ------------------------------------------------------------------------------------------------ 3. the operator, streams
def _op(sc, **kw):
    from rampvo_amd import ops
    out = ops.event_landmarks(cu(sc["x"]), cu(sc["y"]), cu(sc["t"]), cu(sc["track"]), cu(sc["knots"]), cu(sc["times"]), cu(sc["K"]), **kw)
    res = {k: v.cpu().numpy() for k, v in out.items()}
    k = int(res["count"][0])
    return {key: (v[:k] if key in lr.PER_LANDMARK else v) for key, v in res.items()}


def test_operator():
    from rampvo_amd import ops
    sc, kw = cases()["edges T=9"]
    direct = call(sc, **kw)
    got = _op(sc, want_index=True, want_residual=True, want_rays=True, **kw)
    for k in got:
        assert georef.same_bits(got[k], direct[k]) if got[k].dtype.itemsize >= 4 else np.array_equal(got[k], direct[k]), k
    d = ops.event_landmarks(cu(sc["x"]), cu(sc["y"]), cu(sc["t"]), cu(sc["track"]), cu(sc["knots"]), cu(sc["times"]), sc["K"].tolist())
    assert sorted(d) == ["cls", "count", "cov", "n_obs", "parallax", "point", "rms", "span", "status", "track"]
    assert d["point"].shape == (len(sc["t"]), 3) and d["count"].item() == 8
    s = ops.event_landmarks_status(cu(direct["status"]))
    assert s == dict(bad_times=False, n_no_track=332, n_not_finite=332, n_out_of_range=332, n_observations=5327, n_tracks=8, n_cut_off=0,
                     n_valid=6)
    empty = _op(take(sc, slice(0, 0)), want_index=True)
    assert empty["count"][0] == 0 and not empty["status"].any() and empty["index"].shape == (0,)
    # the map drops what is not valid by itself
    pm = ops.PointMap(0.05, capacity=1 << 10)
    c = d["cov"]
    st = ops.point_map_status(pm.insert(d["point"], conf=1.0 / (c[:, 0] + c[:, 3] + c[:, 5]), count=d["count"]))
    assert st["n_seen"] == 8 and st["n_not_finite"] == 2 and st["n_accumulated"] + st["n_out_of_range"] + st["n_dropped_full"] == 6
    assert st["n_accumulated"] > 0
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.event_landmarks(torch.zeros(3), torch.zeros(3), torch.zeros(3).double(), torch.zeros(3).long(), cu(sc["knots"]),
                            cu(sc["times"]), sc["K"])


def test_own_stream():
    from rampvo_amd import ops
    sc, kw = cases()["edges T=9"]
    want = call(sc, **kw)
    side = torch.cuda.Stream()
    hosts = [torch.from_numpy(np.ascontiguousarray(sc[k])).pin_memory() for k in ("x", "y", "t", "track", "knots", "times", "K")]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev = [v.to("cuda", non_blocking=True) for v in hosts]
        out = ops.event_landmarks(*dev, want_index=True, want_residual=True, want_rays=True, **kw)
        for v in dev[:3]:
            v.fill_(float("nan"))
        dev[3].fill_(-1)
        host = {k: v.to("cpu", non_blocking=True) for k, v in out.items()}
        side.synchronize()
    k = int(host["count"][0])
    for key, v in host.items():
        v = v.numpy()[:k] if key in lr.PER_LANDMARK else v.numpy()
        assert georef.same_bits(v, want[key]) if v.dtype.itemsize >= 4 else np.array_equal(v, want[key]), key


# ------------------------------------------------------------------------------------------------ 4. end to end
def test_moving_corner_end_to_end():
    """A corner fixed in space at X0, seen by a camera that translates sideways without turning (two knots: the geodesic is
    the straight line), rendered into one event per time step at its projection.  ops.event_corner_tracks links the truncated
    pixels into one track among noise, ops.event_landmarks triangulates the sub-pixel projections.  The bound of the closed
    form: the rays are off by at most the rule's ray bound e (in pixels: f e), a least-squares solution moves by at most
    |dr| / sigma_min(J) = sqrt(lambda_max(H^-1)) sqrt(2 n) f e, and lambda_max(H^-1) is that of the call's cov at sigma_px = 1."""
    from rampvo_amd import ops
    H, W, n = lr.H0, lr.W0, 40
    K = lr.K0
    X0 = np.array([0.2, -0.1, 5.0])
    times = np.array([0.0, 1.0])
    knots = np.zeros((2, 7), np.float32)
    knots[:, 6] = 1.0
    knots[0, 0], knots[1, 0] = -1.0, 1.0
    t = 0.0125 + 0.0245 * np.arange(n)
    c = np.stack([-1.0 + 2.0 * t, 0 * t, 0 * t], 1)
    px = (K[0] * (X0[0] - c[:, 0]) / X0[2] + K[2]).astype(np.float32)
    py = np.full(n, K[1] * X0[1] / X0[2] + K[3], np.float32)
    rng = np.random.default_rng(9)
    m = 60                                                   # noise: single events in the far corner, each a track of its own
    xa = np.concatenate([px, rng.uniform(0, 5, m).astype(np.float32)])
    ya = np.concatenate([py, rng.uniform(0, 5, m).astype(np.float32)])
    ta = np.concatenate([t, rng.uniform(0.0, 1.0, m)])
    order = np.argsort(ta, kind="stable")
    xa, ya, ta = xa[order], ya[order], ta[order]
    trk = ops.event_corner_tracks(cu(np.trunc(xa).astype(np.int32)), cu(np.trunc(ya).astype(np.int32)), cu(ta), H, W, radius=1, max_dt=0.03)
    track = trk["track"].cpu().numpy()
    mine = track[np.nonzero(order < n)[0]]
    assert (mine == mine[0]).all() and (track == mine[0]).sum() == n and trk["status"][0].item() == 0
    out = ops.event_landmarks(cu(xa), cu(ya), cu(ta), trk["track"], cu(knots), cu(times), cu(K), min_obs=3, refine=2, want_rays=True)
    k = int(out["count"].item())
    ids = out["track"][:k].cpu().numpy()
    l = int(np.nonzero(ids == mine[0])[0][0])
    assert out["cls"][l].item() == 7 and out["n_obs"][l].item() == n and out["status"][7].item() >= 1
    P, cov = out["point"][l].cpu().numpy().astype(np.float64), out["cov"][l].cpu().numpy().astype(np.float64)
    sc = dict(x=xa, y=ya, t=ta, knots=knots, times=times, K=K)
    r64, _ = lr.event_rays(xa, ya, ta, knots, times, K, False, np.float64)
    r32, _ = lr.event_rays(xa, ya, ta, knots, times, K, False, np.float32)
    e = georef.bound(georef.PIXEL_FLOOR * float(np.abs(r64).max()), georef.max_err(r32, r64))
    lam = float(np.linalg.eigvalsh(lr.sym(cov)).max())
    bound = np.sqrt(lam) * np.sqrt(2 * n) * float(K.max()) * e + 2.0 ** -23 * float(np.abs(X0).max())
    err = float(np.linalg.norm(P - X0))
    print("end to end: point %s, closed form %s, err %.3g, bound %.3g" % (P, X0, err, bound))
    assert err <= bound


TRACKS = dict(radius=3, max_dt=4 * cr.TICK)
LM = dict(min_parallax=0.0, max_rms=50.0, want_index=True, want_rays=True, want_residual=True)


def _tracker_queries(slam, f):
    from rampvo_amd import ops
    x, y, t, p = cr.stream(4099)
    xh, yh = np.trunc(x).astype(np.int32) + 100, np.trunc(y).astype(np.int32) + 100
    th = 100.0 + 0.5 * (f - 2) + (t - t[0])
    with pytest.raises(RuntimeError, match="unknown parameter"):
        slam.event_landmarks(xh, yh, th, window=1.0, max_dt=1.0)
    with pytest.raises(RuntimeError, match="max_dt is required"):
        slam.event_landmarks(xh, yh, th)
    a = slam.event_landmarks(xh, yh, th, p, carry=False, **LM, **TRACKS)
    b = kit.host(slam.event_landmarks(cu(xh), cu(yh), cu(th), cu(p), carry=False, as_tensor=True, **LM, **TRACKS))
    k = a["count"]
    assert isinstance(k, int) and k == b["count"][0] > 10 and slam._track_state is None
    same = lambda u, v: georef.same_bits(u, v) if u.dtype.itemsize >= 4 else np.array_equal(u, v)
    for key in ("lm_track", "point", "cov", "n_obs", "lm_cls", "rms", "parallax", "span"):
        assert same(a[key], b[key][:k]), key
    alone = slam.event_corner_tracks(xh, yh, th, p, carry=False, **TRACKS)
    assert np.array_equal(a["track"], alone["track"]) and np.array_equal(a["track_status"], alone["status"]) and np.array_equal(a["cls"], alone["cls"])
    # the operator on the tracker's own trajectory, time stamps and intrinsics: the query's bits
    knots, _ = slam.trajectory(as_tensor=True)
    d = kit.host(ops.event_landmarks(cu(xh.astype(np.float32)), cu(yh.astype(np.float32)), cu(th), cu(a["track"]), knots,
                                     slam._frame_times_dev(), slam.intrinsics_[0] * float(slam.RES), **LM))
    for key, mine in (("track", "lm_track"), ("cls", "lm_cls"), ("point", "point"), ("cov", "cov"), ("n_obs", "n_obs"), ("rms", "rms"),
                      ("parallax", "parallax"), ("span", "span")):
        assert same(d[key][:k], a[mine]), key
    for key in ("index", "residual", "rays", "status"):
        assert same(d[key], a[key]), key
    assert a["status"][0] == 0 and a["status"][1:5].sum() == 4099 and a["status"][4] > 100 and a["status"][5] == k
    obs = a["index"] >= 0
    assert np.isfinite(a["rays"][obs]).all() and np.isnan(a["rays"][a["track"] < 0]).all() and np.array_equal(a["n_obs"], np.bincount(a["index"][obs], minlength=k))
    # insert=True: the map then holds the valid landmarks' voxels
    c = slam.event_landmarks(xh, yh, th, p, carry=False, insert=True, **LM, **TRACKS)
    st = ops.point_map_status(cu(c["map_status"]))
    n_valid = int(c["status"][7])
    assert same(c["point"], a["point"]) and n_valid == (a["lm_cls"] == 7).sum()
    assert st["n_seen"] == k and st["n_not_finite"] == k - n_valid and st["n_accumulated"] + st["n_out_of_range"] + st["n_dropped_full"] == n_valid
    pts = slam.event_map_points(min_points=1)
    assert pts["count"] == st["n_occupied"] and pts["n"].sum() == st["n_accumulated"]
    return dict(landmarks={key: a[key] for key in ("lm_track", "point", "cov", "lm_cls", "status")})


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
