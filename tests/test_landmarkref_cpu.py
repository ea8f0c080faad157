"""tests/landmarkref.py, the numpy restatement of ramp_event_landmarks, held to closed forms that are exact in binary; the
generators of the GPU test hold what they claim (conditions, margins at every gate, the status identities); the streams of the
GPU test (landmarkref.cases) tell every mistake of landmarkref.MISTAKES from the definition; the entries are declared, exported
and bound, and every refusal of the entry and of the operator comes without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import landmarkref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I4 = np.array([0.0, 0.0, 0.0, 1.0])
K1 = np.array([1.0, 1.0, 0.0, 0.0], np.float32)
_refs = {}


def refs():
    """the restatement on every stream of the GPU test, once"""
    if not _refs:
        for name, (sc, kw) in lr.cases().items():
            _refs[name] = (sc, kw, run(sc, kw))
    return _refs


def run(sc, kw, **more):
    return lr.event_landmarks(sc["x"], sc["y"], sc["t"], sc["track"], sc["knots"], sc["times"], sc["K"], want_cond=True, **{**kw, **more})


def views(centres, quats, P, K=K1, ids=None, t=None):
    """the events of one point P seen from the given poses, as rays: exact where the projection is exact in binary"""
    centres, quats = np.asarray(centres, np.float64), np.asarray(quats, np.float64)
    n = len(centres)
    Y = lr.poseref.qrot(quats * np.array([-1.0, -1.0, -1.0, 1.0]), np.asarray(P, np.float64) - centres)
    x, y = K[0] * Y[:, 0] / Y[:, 2] + K[2], K[1] * Y[:, 1] / Y[:, 2] + K[3]
    f = np.stack([(x - K[2]) / K[0], (y - K[3]) / K[1], np.ones(n)], -1)
    rays = np.concatenate([centres, lr.poseref.qrot(quats, f)], 1).astype(np.float32)
    return dict(x=x.astype(np.float32), y=y.astype(np.float32), t=np.arange(n, dtype=np.float64) if t is None else t,
                track=np.zeros(n, np.int64) if ids is None else ids, rays=rays, quat=quats.astype(np.float32))


def solve(v, K=K1, times=None, **kw):
    times = np.array([v["t"].min(), v["t"].max() + 1.0]) if times is None else times
    return lr.event_landmarks(v["x"], v["y"], v["t"], v["track"], None, times, K, rays=v["rays"], quat=v["quat"], want_cond=True,
                              **{**dict(min_obs=2, min_parallax=0.0), **kw})


# ------------------------------------------------------------------------------------------------ 1. closed forms
def test_two_rays_that_meet_and_the_optical_axis():
    """two cameras at (-1, 0, 0) and (1, 0, 0) look along z at (0, 0, 4): pixels (1/4, 0) and (-1/4, 0), all exact in binary"""
    v = views([[-1, 0, 0], [1, 0, 0]], [I4, I4], [0, 0, 4])
    for refine in (0, 2):
        r = solve(v, refine=refine)
        assert r["cls"].tolist() == [7] and r["n_obs"].tolist() == [2] and r["count"][0] == 1
        assert np.allclose(r["point"][0], [0, 0, 4], atol=1e-15, rtol=0) and r["rms"][0] <= 1e-15
        assert np.abs(r["residual"]).max() <= 1e-15 and r["span"].tolist() == [[0.0, 1.0]]
    # a point on the optical axis of the first camera under a sideways translation
    v = views([[0, 0, 0], [0.5, 0, 0], [1, 0, 0]], [I4, I4, I4], [0, 0, 2])
    r = solve(v, refine=1)
    assert r["cls"][0] == 7 and np.allclose(r["point"][0], [0, 0, 2], atol=1e-15, rtol=0)
    assert np.isclose(r["parallax"][0], np.arctan(0.5), rtol=1e-15)


def test_refine_zero_is_the_midpoint_and_exact_data_does_not_move():
    rng = np.random.default_rng(1)
    v = views([[-1, 0, 0], [0, 0.5, 0], [1, 0, 0]], [I4, I4, I4], [0.25, -0.5, 4])
    v["y"] = v["y"] + np.array([0.25, 0.0, 0.0], np.float32)                 # inconsistent pixels; the rays stay: the midpoint is theirs
    a, b = solve(v, refine=0), solve(v, refine=2)
    assert np.allclose(a["point"][0], [0.25, -0.5, 4], atol=1e-14, rtol=0) and a["rms"][0] > 0.1
    assert np.abs(b["point"][0] - a["point"][0]).max() > 1e-3 and b["rms"][0] < a["rms"][0]
    v = views(rng.uniform(-1, 1, (5, 3)), [I4] * 5, [0.25, -0.5, 4])
    a, b = solve(v, refine=0), solve(v, refine=2)
    assert np.abs(b["point"][0] - a["point"][0]).max() <= 1e-6 and b["rms"][0] <= 1e-6       # (fp32 pixels and rays: exact to their rounding)


def test_the_classes():
    s = np.sqrt(0.5)
    turn = [0.0, s, 0.0, s]                                               # 90 degrees about y
    v = views([[0, 0, 0], [0, 0, 0]], [I4, turn], [0, 0, 4])
    v["rays"][1, 3:] = [1, 0, 0]                                          # the second camera looks along x: a pure rotation
    r = solve(v, min_parallax=2.0)                                      # the same pixel from a camera turned by 90 degrees
    assert solve(v)["cls"][0] != 2 and r["cls"][0] == 2 and r["parallax"][0] == np.pi / 2 and np.isnan(r["point"]).all() and np.isnan(r["cov"]).all()
    v = views([[-1, 0, 0], [1, 0, 0]], [I4, I4], [0, 0, 4])
    assert solve(v, min_obs=3)["cls"][0] == 1 and solve(v, min_obs=2)["cls"][0] == 7
    par = dict(v, rays=np.array([[-1, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, 1]], np.float32))
    r = solve(par)
    assert r["cls"][0] == 3 and np.isnan(r["rms"][0]) and np.isnan(r["residual"]).all() and r["parallax"][0] == 0.0
    back = [0.0, 1.0, 0.0, 0.0]                                           # 180 degrees about y: the camera looks away
    v = views([[-1, 0, 0], [1, 0, 0], [0, 0, 0]], [I4, I4, back], [0, 0, 4])
    r = solve(v, refine=0)
    assert r["cls"][0] == 4 and abs(r["zmin"][0] + 4.0) <= 1e-14 and np.isnan(r["point"]).all() and np.isfinite(r["rms"][0])
    v = views([[-1, 0, 0], [1, 0, 0]], [I4, I4], [0, 0, 4])
    v["y"] = v["y"] + np.array([0.5, -0.5], np.float32)
    assert solve(v, refine=0, max_rms=0.25)["cls"][0] == 5 and solve(v, refine=0, max_rms=1.0)["cls"][0] == 7


def test_covariance_of_a_symmetric_two_view_case():
    """cameras at (-b, 0, 0) and (b, 0, 0), the point at (0, 0, Z), f = 1: with a = 1 / Z and c = b / Z^2 the rows of J are
    (a, 0, -c), (0, a, 0), (a, 0, c), (0, a, 0): H = diag(2 a^2, 2 a^2, 2 c^2), cov = sigma^2 diag(Z^2 / 2, Z^2 / 2, Z^4 / (2 b^2))"""
    b, Z, sigma = 1.0, 4.0, 0.5
    r = solve(views([[-b, 0, 0], [b, 0, 0]], [I4, I4], [0, 0, Z]), sigma_px=sigma)
    want = sigma ** 2 * np.array([Z * Z / 2, 0, 0, Z * Z / 2, 0, Z ** 4 / (2 * b * b)])
    assert np.allclose(r["cov"][0], want, rtol=1e-14, atol=1e-14) and r["cond"][0] == pytest.approx(16.0)


def test_order_numbering_cut_and_status():
    v = views([[-1, 0, 0], [1, 0, 0], [-1, 0, 0], [1, 0, 0], [0, 0, 0]], [I4] * 5, [0, 0, 4],
              ids=np.array([9, 9, 2, 2, -1]), t=np.array([1.0, 0.0, 0.5, 0.5, 0.25]))
    r = solve(v)
    assert r["track"].tolist() == [2, 9] and r["index"].tolist() == [1, 1, 0, 0, -1] and r["span"].tolist() == [[0.5, 0.5], [0.0, 1.0]]
    assert r["status"].tolist() == [0, 1, 0, 0, 4, 2, 0, 2] and np.isnan(r["rays"][4]).all() and np.isnan(r["residual"][4]).all()
    cut = solve(v, max_landmarks=1)
    assert cut["track"].tolist() == [2] and cut["index"].tolist() == [-1, -1, 0, 0, -1] and cut["status"].tolist() == [0, 1, 0, 0, 4, 2, 1, 1]
    assert np.isnan(cut["residual"][:2]).all() and np.isfinite(cut["rays"][:2]).all()
    v["t"][0], v["x"][1] = 7.0, np.nan                                     # outside [0, 2], not finite
    r = solve(v, times=np.array([0.0, 2.0]))
    assert r["status"].tolist() == [0, 1, 1, 1, 2, 1, 0, 1] and r["track"].tolist() == [2]
    bad = lr.event_landmarks(v["x"], v["y"], v["t"], v["track"], None, np.array([1.0, 0.0]), K1, rays=v["rays"], quat=v["quat"])
    assert bad["status"].tolist() == [1, 1, 1, 3, 0, 0, 0, 0] and bad["count"][0] == 0 and (bad["index"] == -1).all()


# ------------------------------------------------------------------------------------------------ 2. the generators' claims
def test_generators_conditions_margins_and_identities():
    seen = np.zeros(8, int)
    sizes = set()
    for name, (sc, kw, r) in refs().items():
        st = r["status"]
        assert st[0] == 0 and st[1:5].sum() == len(sc["t"]) and st[5] - st[6] == r["count"][0] == len(r["cls"]), name
        assert st[7] == (r["cls"] == 7).sum() and st[4] >= r["n_obs"].sum() and (st[6] > 0 or st[4] == r["n_obs"].sum()), name
        seen += np.bincount(r["cls"], minlength=8)
        sizes |= set(r["n_obs"].tolist())
        valid = r["cls"] == 7
        assert (r["cond"][valid] <= 1e4).all(), name
        # every gate at least 100 bounds from its threshold: the bound of a float64 quantity q is 64 n 2^-53 cond |q|
        with np.errstate(invalid="ignore"):
            term = 100 * 64.0 * r["n_obs"] * lr.U * np.where(np.isfinite(r["cond"]), r["cond"], 1.0)
        p = dict(lr.PARAMS, **kw)
        reached = r["n_obs"] >= p["min_obs"]
        assert (np.abs(r["parallax"] - np.float32(p["min_parallax"]))[reached] > (term * r["parallax"] + 1e-13)[reached]).all(), name
        reached &= r["parallax"] >= np.float32(p["min_parallax"])
        assert (r["pivot"][reached] > 1e-9).all(), name                        # a pivot of the midpoint system, per observation
        assert (np.abs(r["zmin"] - lr.MIN_Z)[reached] > (term * np.maximum(np.abs(r["zmin"]), r["dist"]))[reached]).all(), name
        reached &= r["zmin"] > lr.MIN_Z
        assert (np.abs(r["rms"] - np.float32(p["max_rms"]))[reached] > (term * r["rms"])[reached]).all(), name
    assert seen[[1, 2, 5, 7]].all() and set(lr.EDGE_SIZES) <= sizes


# ------------------------------------------------------------------------------------------------ 3. deliberate mistakes
@pytest.mark.parametrize("mistake", lr.MISTAKES)
def test_every_mistake_is_rejected_by_the_gpu_tests_streams(mistake):
    """on at least one stream of the GPU test the mistaken restatement differs from the definition by an integer, a NaN pattern
    or more than 100 bounds"""
    hits = []
    for name, (sc, kw, good) in refs().items():
        if name == "1000 tracks, cut":
            continue                                                      # (the largest: the others decide)
        if mistake == "first_by_index":                                   # the order of the events in time is the order of their indices: shuffle
            perm = np.random.default_rng(3).permutation(len(sc["t"]))
            sc = dict(sc, x=sc["x"][perm], y=sc["y"][perm], t=sc["t"][perm], track=sc["track"][perm])
            good = run(sc, kw)
        wrong = run(sc, kw, mistake=mistake)
        cmp = lr.compare({k: good[k] for k in lr.EXACT + ("point", "cov", "rms", "parallax", "residual")}, wrong)
        if cmp["exact"] or cmp["nan"] or cmp["ratio"] > 100.0:
            hits.append(name)
    assert hits, mistake


# ------------------------------------------------------------------------------------------------ 4. the entry and the operator
def test_entries_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_event_landmarks", "ramp_event_landmarks_ws_bytes", "ramp_event_landmarks_grid_events"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["ramp_event_landmarks"][1]) == 32
    assert ops._STATUS["event_landmarks"][0]["bad_times"] is ops._STATUS["event_warp"][0]["bad_times"]           # one row
    assert ops._STATUS["event_landmarks"][1] == ("n_no_track", "n_not_finite", "n_out_of_range", "n_observations", "n_tracks", "n_cut_off",
                                                 "n_valid")
    assert "event_landmarks" not in ops.STATUS_ROLES.values() and len(ops.STATUS_ORDER) == 16
    assert lib.ramp_event_landmarks_grid_events() == lib.ramp_event_corner_tracks_grid_events()
    a, b = lib.ramp_event_landmarks_ws_bytes(1 << 16, 9, 10), lib.ramp_event_landmarks_ws_bytes(1 << 17, 9, 1 << 17)
    assert a % 256 == 0 and b > a > (8 + 8 + 4 + 4 + 4 + 4 + 4 + 48) << 16
    assert [lib.ramp_event_landmarks_ws_bytes(*q) for q in ((-1, 9, 1), (10, 0, 1), (10, 9, 0), (1 << 31, 9, 1))] == [0] * 4
    assert lib.ramp_event_landmarks_ws_bytes(0, 1, 1) > 0
    assert all(callable(f) for f in (ops.event_landmarks, ops.event_landmarks_status, TrackerQueries.event_landmarks))
    assert "landmark.hip" in open(os.path.join(ROOT, "rampvo_amd", "csrc", "Makefile")).read()
    assert lr.MIN_Z == pytest.approx(_lib.RAMP_WARP_MIN_Z) and lr.BAD_TIMES == _lib.RAMP_INTERP_BAD_TIMES


def test_argument_checks_that_need_no_gpu():
    """every refusal comes before anything touches the device (the pointers are never read)"""
    import torch
    from rampvo_amd import _lib, ops
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd4, odd2 = ctypes.c_void_p(q.value + 4), ctypes.c_void_p(q.value + 2)

    def call(N=10, T=9, flags=0, min_obs=3, refine=2, min_parallax=0.02, max_rms=2.0, sigma_px=1.0, L=5, ws_bytes=0, **ptrs):
        p = {k: q for k in ("x", "y", "t", "track", "knots", "times", "K", "lm_track", "point", "cov", "n_obs", "cls", "rms", "parallax", "span",
                            "count", "status", "ws")}
        p.update(index=None, residual=None, rays=None)
        p.update(ptrs)
        return lib.ramp_event_landmarks(p["x"], p["y"], p["t"], p["track"], N, p["knots"], p["times"], T, p["K"], flags, min_obs, refine,
                                        min_parallax, max_rms, sigma_px, L, p["lm_track"], p["point"], p["cov"], p["n_obs"], p["cls"], p["rms"],
                                        p["parallax"], p["span"], p["count"], p["index"], p["residual"], p["rays"], p["status"], p["ws"],
                                        ws_bytes, None)

    nan, inf = float("nan"), float("inf")
    for kw in (dict(N=-1), dict(T=0), dict(flags=2), dict(flags=-1), dict(min_obs=1), dict(refine=-1), dict(refine=5), dict(min_parallax=-1e-30),
               dict(min_parallax=nan), dict(max_rms=inf), dict(max_rms=-1.0), dict(sigma_px=nan), dict(sigma_px=-inf), dict(L=0),
               *[{k: None} for k in ("x", "y", "t", "track", "knots", "times", "K", "ws", "lm_track", "point", "cov", "n_obs", "cls", "rms",
                                     "parallax", "span", "count", "status")],
               *[{k: odd4} for k in ("lm_track", "span", "t", "track", "times")],
               *[{k: odd2} for k in ("x", "y", "knots", "K", "point", "cov", "n_obs", "rms", "parallax", "count", "index", "residual", "rays",
                                     "status")], dict(ws=ctypes.c_void_p(q.value + 8))):
        assert call(**kw) == _lib.RAMP_EINVAL, kw
    full = lib.ramp_event_landmarks_ws_bytes(10, 9, 5)
    assert call() == _lib.RAMP_EWORKSPACE and call(ws_bytes=full - 1) == _lib.RAMP_EWORKSPACE and call(N=1 << 31) == _lib.RAMP_EUNSUPPORTED
    assert call(cls=ctypes.c_void_p(q.value + 1), refine=0, min_parallax=0.0, flags=1) == _lib.RAMP_EWORKSPACE      # (allowed: refused later)
    x, tr = torch.zeros(4), torch.zeros(4, dtype=torch.int64)
    good = dict(x=x, y=x, t=x.double(), track=tr, knots=torch.zeros(2, 7), times=torch.zeros(2).double(), intrinsics=[1.0, 1.0, 0.0, 0.0])
    for kw, text in ((dict(min_obs=1), "min_obs"), (dict(min_obs=2.5), "min_obs"), (dict(refine=5), "refine"), (dict(refine=True), "refine"),
                     (dict(min_parallax=-1.0), "min_parallax is finite"), (dict(max_rms=inf), "max_rms is finite"),
                     (dict(sigma_px=nan), "sigma_px is finite"), (dict(max_landmarks=0), "max_landmarks"), (dict(track=tr.int()), "track is int64"),
                     (dict(y=torch.zeros(3)), "differ in length"), (dict(track=tr[:3]), "differ in length"),
                     (dict(times=torch.zeros(3).double()), "2 knots but 3 time stamps"), (dict(knots=torch.zeros(0, 7), times=torch.zeros(0).double()), "at least one knot"),
                     (dict(), "GPU only")):
        with pytest.raises(RuntimeError, match=text):
            ops.event_landmarks(**{**good, **kw})
    assert ops.event_landmarks_status(torch.tensor([1, 9, 1, 2, 3, 4, 1, 2], dtype=torch.int32)) == dict(
        bad_times=True, n_no_track=9, n_not_finite=1, n_out_of_range=2, n_observations=3, n_tracks=4, n_cut_off=1, n_valid=2)
