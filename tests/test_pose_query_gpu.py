"""Continuous-time pose queries on the GPU: ``ramp_se3_interp`` (csrc/interp.hip) through ``ops.se3_interp``,
``lietorch.interpolate``, ``Ramp_vo.poses_at`` and ``evaluate.resample_trajectory`` against the float64 restatement
(tests/interpref.py), every comparison by ``interpref.compare``: the bound is ``georef.bound(floor, env)`` with floor =
georef.FLOOR["log"] x max(1, largest |translation|) and env = the fp32 restatement's own error against float64.

The tracker tests run the small synthetic tracker of tests/trackerkit.py (keyframes are dropped while it is device resident
from frame 21 on, and the initialisation leaves delta chains of depth 6), device resident."""
import ctypes

import numpy as np
import pytest
import torch

import georef
import interpref
import trackerkit as kit
from trackerkit import T_FRAMES, T_QUERY, cu

pytestmark = pytest.mark.gpu

_cache = {}


def _interp(knots, times, query, extrapolate=False, twist=True, **kw):
    from rampvo_amd import ops
    out, tw, status = ops.se3_interp(cu(np.asarray(knots, np.float32)), cu(np.asarray(times, np.float64)),
                                     cu(np.asarray(query, np.float64)), extrapolate=extrapolate, twist=twist, **kw)
    return out.cpu().numpy(), (tw.cpu().numpy() if twist else None), status.cpu().numpy()


def _raw(knots, times, T, query, Q, flags, out_p, twist_p, status_p):
    """the C entry with explicit sizes and pointers; the workspace is sized by the library's own query (for max(T, 1))"""
    from rampvo_amd import _lib
    L = _lib.lib()
    nbytes = L.ramp_se3_interp_workspace_bytes(max(T, 1))
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    rc = L.ramp_se3_interp(_lib.ptr(knots), _lib.ptr(times), T, _lib.ptr(query), Q, flags, out_p, twist_p, _lib.ptr(ws), nbytes,
                           status_p, _lib.stream())
    torch.cuda.synchronize()
    return rc


# ------------------------------------------------------------------------------------------------ 1. float64, per bin
ANGLES = (1e-7, 1e-3, 1.0, 3.0, np.pi - 1e-3)       # both sides of LT_EPS = 1e-6 (alpha = 1e-6 takes every angle below it)
ALPHAS = (0.0, 1e-6, 0.5, 1.0)
N_SEG = 24


def test_against_float64_per_bin():
    """segment rotation x alpha x translation scale, 24 random segments per bin: poses and twists within georef.bound(floor,
    env); (measured, envelope, bound) printed per bin"""
    poses, twists = georef.Table("se3_interp: poses against float64"), georef.Table("se3_interp: twists x segment length")
    for scale in (1.0, 100.0):
        for ai, angle in enumerate(ANGLES):
            knots, times = interpref.pair_scene(100 + ai, N_SEG, angle, scale)
            query = np.concatenate([times[0::2] + a for a in ALPHAS])
            out, tw, status = _interp(knots, times, query)
            assert status.tolist() == [0, 0, 0, 0]
            for k, a in enumerate(ALPHAS):
                sel = slice(k * N_SEG, (k + 1) * N_SEG)
                r = interpref.compare(out[sel], knots, times, query[sel], twist=tw[sel])
                name = "angle %.3g alpha %g scale %g" % (angle, a, scale)
                poses.add(name, r["err"], r["env"], r["floor"])
                twists.add(name, r["tw_err"], r["tw_env"], r["floor"])
    poses.show()
    twists.show()
    assert not poses.failed() and not twists.failed(), (poses.failed(), twists.failed())


# ------------------------------------------------------------------------------------------------ 2. time arithmetic
@pytest.mark.parametrize("t0,dt", [(1.7e9, 1e-3), (1.7e15, 1000.0)], ids=["seconds", "microseconds"])
def test_time_arithmetic(t0, dt):
    """absolute stamps with a small spacing (1.7e9 + k 1e-3 s, 1.7e15 + k 1000 us), queries strictly inside the segments:
    alpha has to come from a float64 difference -- in fp32 the stamps of a segment are one number"""
    knots, times = interpref.walk_scene(21, 9, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2), t0=t0, dt=dt)
    frac = np.array([0.03, 0.37, 0.5, 0.91])
    query = (times[:-1, None] + frac[None] * np.diff(times)[:, None]).reshape(-1)
    assert ((query > times[0]) & (query < times[-1])).all() and not np.isin(query, times).any()
    out, tw, status = _interp(knots, times, query)
    r = interpref.compare(out, knots, times, query, twist=tw)
    print("poses: measured %.2e envelope %.2e bound %.2e; twists x dt: %.2e %.2e %.2e"
          % (r["err"], r["env"], r["bound"], r["tw_err"], r["tw_env"], r["tw_bound"]))
    assert status.tolist() == [0, 0, 0, 0] and r["ok"] and r["tw_ok"], r


# ------------------------------------------------------------------------------------------------ 3. shapes
CANARY = 12345.5


@pytest.mark.parametrize("T", [1, 2, 3, 9])
@pytest.mark.parametrize("Q", [1, 63, 64, 65, 257])
def test_shapes_between_canaries(Q, T):
    """out and twist sit between canary rows that must survive; a NULL twist pointer gives the same pose bits; so does the
    launch's other store form"""
    knots, times = interpref.walk_scene(30 + T, T, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2))
    rng = np.random.default_rng(Q * 16 + T)
    query = rng.uniform(times[0] - 0.5, times[-1] + 0.5, Q)
    k, t, q = cu(knots), cu(times), cu(query)
    pad = 8
    runs = []
    for flags, with_twist in ((0, True), (0, False), (2, True)):
        out = torch.full((Q + 2 * pad, 7), CANARY, device="cuda")
        tw = torch.full((Q + 2 * pad, 6), CANARY, device="cuda")
        status = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        rc = _raw(k, t, T, q, Q, flags, ctypes.c_void_p(out.data_ptr() + pad * 28),
                  ctypes.c_void_p(tw.data_ptr() + pad * 24) if with_twist else None, ctypes.c_void_p(status.data_ptr()))
        assert rc == 0
        o, w = out.cpu().numpy(), tw.cpu().numpy()
        assert (o[:pad] == CANARY).all() and (o[pad + Q:] == CANARY).all()
        assert (w[:pad] == CANARY).all() and (w[pad + Q:] == CANARY).all()
        if not with_twist:
            assert (w == CANARY).all()
        runs.append((o[pad:pad + Q], w[pad:pad + Q], status.cpu().numpy()))
    (o0, w0, s0), (o1, _, s1), (o2, w2, s2) = runs
    assert georef.same_bits(o0, o1) and georef.same_bits(o0, o2) and georef.same_bits(w0, w2)
    assert s0.tolist() == s1.tolist() == s2.tolist() == [0, int((query < times[0]).sum()), int((query > times[-1]).sum()), 0]
    r = interpref.compare(o0, knots, times, query, twist=w0)
    assert r["ok"] and r["tw_ok"], r
    if T == 1:
        assert georef.pose_err(o0, interpref.interpolate(knots, times, query)[0]) <= r["floor"] and not w0.any()


def test_empty_and_invalid_sizes():
    """Q == 0: RAMP_OK and nothing written, the status words included; T == 0: RAMP_EINVAL"""
    knots, times = interpref.walk_scene(3, 4)
    k, t, q = cu(knots), cu(times), cu(np.array([0.5, 1.5]))
    out = torch.full((2, 7), CANARY, device="cuda")
    status = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    assert _raw(k, t, 4, q, 0, 0, p(out), None, p(status)) == 0
    assert (out.cpu().numpy() == CANARY).all() and status.cpu().tolist() == [-7] * 4
    assert _raw(k, t, 0, q, 2, 0, p(out), None, p(status)) == -1
    assert _raw(k, t, 4, q, -1, 0, p(out), None, p(status)) == -1
    assert (out.cpu().numpy() == CANARY).all() and status.cpu().tolist() == [-7] * 4


# ------------------------------------------------------------------------------------------------ 4. search semantics
def test_queries_at_the_knot_times_and_repeated_stamps():
    knots, times = interpref.walk_scene(41, 9, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2), t0=-3.0, dt=0.75)
    out, tw, status = _interp(knots, times, times)
    r = interpref.compare(out, knots, times, times, twist=tw)
    assert status.tolist() == [0, 0, 0, 0] and r["ok"] and r["tw_ok"], r
    unit = knots.astype(np.float64)
    unit[:, 3:] /= np.linalg.norm(unit[:, 3:], axis=1, keepdims=True)
    assert georef.pose_err(out, unit) <= r["floor"]
    # repeated stamps: two interior pairs and the last pair; at a repeated stamp the UPPER knot of the pair answers
    rep = np.array([0.0, 1.0, 1.0, 2.0, 2.5, 2.5, 3.0, 4.0, 4.0])
    query = np.array([-1.0, 0.0, 0.5, 1.0, 1.5, 2.0, 2.25, 2.5, 2.75, 3.0, 3.5, 4.0, 4.5, np.nextafter(1.0, 0), np.nextafter(1.0, 2),
                      np.nextafter(4.0, 0)])
    for ex in (False, True):
        out, tw, status = _interp(knots, rep, query, extrapolate=ex)
        r = interpref.compare(out, knots, rep, query, extrapolate=ex, twist=tw)
        assert r["ok"] and r["tw_ok"], (ex, r)
        assert status.tolist() == [0, 1, 1, 0]
        for tq, kn in ((1.0, 2), (2.5, 5), (4.0, 8), (4.5, 8)):
            assert georef.pose_err(out[query == tq], unit[kn:kn + 1]) <= r["floor"], (ex, tq)
        assert not tw[query >= 4.0].any()           # (the clamped last segment has zero length: no twist)


def test_both_searches():
    """T small enough for the knot times to be staged in LDS, and T one above the staging limit (the search in global memory):
    knots on a smooth random walk, a few hundred queries, sorted and shuffled"""
    from rampvo_amd import _lib
    limit = _lib.lib().ramp_se3_interp_lds_knots()
    rng = np.random.default_rng(43)
    for T in (64, limit, limit + 1):
        if T not in _cache:
            _cache[T] = interpref.walk_scene(50, T, step=(0.02, 0.01, 0.02, 0.01, 0.01, 0.01), t0=10.0, dt=0.01)
        knots, times = _cache[T]
        query = np.sort(np.concatenate([rng.uniform(times[0] - 0.05, times[-1] + 0.05, 380), times[[0, 1, T // 2, T - 2, T - 1]],
                                        rng.choice(times, 15)]))
        out, tw, status = _interp(knots, times, query)
        r = interpref.compare(out, knots, times, query, twist=tw)
        print("T %5d: measured %.2e envelope %.2e bound %.2e" % (T, r["err"], r["env"], r["bound"]))
        assert r["ok"] and r["tw_ok"], (T, r)
        assert status.tolist() == [0, int((query < times[0]).sum()), int((query > times[-1]).sum()), 0]
        perm = rng.permutation(len(query))
        out_p, tw_p, _ = _interp(knots, times, query[perm])
        assert georef.same_bits(out_p, out[perm]) and georef.same_bits(tw_p, tw[perm]), T


# ------------------------------------------------------------------------------------------------ 5. range
@pytest.mark.parametrize("extrapolate", [False, True])
def test_range(extrapolate):
    knots, times = interpref.walk_scene(51, 6, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2), t0=2.0, dt=0.5)
    rng = np.random.default_rng(52)
    query = np.concatenate([rng.uniform(0.0, 2.0, 40), rng.uniform(2.0, 4.5, 50), rng.uniform(4.5, 6.5, 47), [2.0, 4.5]])
    out, tw, status = _interp(knots, times, query, extrapolate=extrapolate)
    r = interpref.compare(out, knots, times, query, extrapolate=extrapolate, twist=tw)
    print("extrapolate %s: measured %.2e envelope %.2e bound %.2e" % (extrapolate, r["err"], r["env"], r["bound"]))
    assert r["ok"] and r["tw_ok"], r
    assert status.tolist() == [0, int((query < times[0]).sum()), int((query > times[-1]).sum()), 0]
    unit = knots.astype(np.float64)
    unit[:, 3:] /= np.linalg.norm(unit[:, 3:], axis=1, keepdims=True)
    if not extrapolate:                             # the end poses are held
        assert georef.pose_err(out[query < 2.0], unit[:1]) <= r["floor"] and georef.pose_err(out[query > 4.5], unit[-1:]) <= r["floor"]
    else:
        assert georef.pose_err(out[:40], np.repeat(unit[:1], 40, 0)) > 100 * r["floor"]


# ------------------------------------------------------------------------------------------------ 6. failures
def test_failure_conventions():
    knots, times = interpref.walk_scene(61, 9, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2))
    rng = np.random.default_rng(62)
    query = rng.uniform(-0.5, 8.5, 64)
    good, good_tw, s0 = _interp(knots, times, query)
    for bad_value in (times[4] - 0.25, np.inf, np.nan):
        bad = times.copy()
        bad[5] = bad_value
        out, tw, status = _interp(knots, bad, query)
        assert status[0] & 1 and np.isnan(out).all() and np.isnan(tw).all(), bad_value
    qn = query.copy()
    qn[37] = np.nan
    out, tw, status = _interp(knots, times, qn)
    keep = np.arange(64) != 37
    assert np.isnan(out[37]).all() and np.isnan(tw[37]).all() and status[3] == 1 and status[0] == 0
    assert georef.same_bits(out[keep], good[keep]) and georef.same_bits(tw[keep], good_tw[keep])
    assert status[1] == (query[keep] < 0).sum() and status[2] == (query[keep] > 8).sum()


# ------------------------------------------------------------------------------------------------ 7. order independence
def test_order_independence():
    knots, times = interpref.walk_scene(71, 9, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2))
    rng = np.random.default_rng(72)
    query = rng.uniform(-0.5, 8.5, 257)
    query[256] = query[0]
    out, tw, _ = _interp(knots, times, query)
    assert georef.same_bits(out[0], out[256]) and georef.same_bits(tw[0], tw[256])
    perm = rng.permutation(257)
    out_p, tw_p, _ = _interp(knots, times, query[perm])
    assert georef.same_bits(out_p, out[perm]) and georef.same_bits(tw_p, tw[perm])
    one, _, _ = _interp(knots, times, query[100:101])             # ... nor on Q
    assert georef.same_bits(one[0], out[100])
    from rampvo_amd import lietorch
    X = lietorch.interpolate(lietorch.SE3(cu(knots)), cu(times), cu(query))
    assert isinstance(X, lietorch.SE3) and X.shape == (257,) and georef.same_bits(X.data.cpu().numpy(), out)


# ------------------------------------------------------------------------------------------------ 8. tracker
def _midpoints(ts):
    return 0.5 * (ts[:-1] + ts[1:])


@torch.no_grad()
def _run(kind):
    """kind: "queried" (device resident; trajectory() and poses_at() behind frame T_QUERY), "plain" (device resident, never
    asked), "host" (host driven, asked at the same frame).  The resident ones publish pose records and go on to frame 43"""
    if kind in _cache:
        return _cache[kind]
    resident = kind != "host"
    slam = kit.tracker(resident, resident)
    if resident:
        slam.pose_stream()
    res = {}
    for t, frame in enumerate(kit.frames()):
        kit.feed(slam, t, frame)
        if t == T_QUERY and kind != "plain":
            if resident:
                assert slam._dev is not None and slam._dev.active and slam.stats["settles"] == 0
            ts = np.array(slam.tlist, dtype=float)
            dev_poses, dev_tw, dev_status = slam.poses_at(torch.from_numpy(_midpoints(ts)).cuda(), twist=True, as_tensor=True)
            res["traj"], res["ts"] = slam.trajectory()
            res["at_knots"], _ = slam.poses_at(ts)
            res["at_mid"], res["tw_mid"] = slam.poses_at(_midpoints(ts), twist=True)
            res["at_mid_tensor"], res["status"] = dev_poses.cpu().numpy(), dev_status.cpu().numpy()
            res["outside"], _ = slam.poses_at([ts[0] - 1.0, ts[-1] + 1.0])
            if resident:
                res["resident_after"] = slam._dev.active and slam.stats["settles"] == 0
            else:
                break
    if resident:
        res["resident_frames"] = slam.stats["device_frames"]
        res["still_resident"] = slam._dev.active and slam.stats["settles"] == 0
        n = slam.peek()["n"]
        torch.cuda.synchronize()
        recs, lost = slam.poses_since(-1)
        res.update(n=n, recs=recs, lost=lost, poses=slam.poses_[:n].cpu().numpy(), patches=slam.patches_[:n].cpu().numpy())
    _cache[kind] = res
    kit.drop(slam)
    return res


def test_tracker_poses_at_the_frame_times_and_between():
    """poses_at(tlist) equals trajectory() within the floor; at the segment midpoints it equals the restatement over
    trajectory(); the tensor form gives the same bits; the tracker was resident before and is resident afterwards"""
    a = _run("queried")
    assert a["resident_after"] and a["still_resident"] and a["resident_frames"] >= 10
    assert any(r.dropped for r in a["recs"][:T_QUERY + 1]), "no keyframe was dropped before the query"
    traj, ts = a["traj"], a["ts"]
    assert traj.shape == (T_QUERY + 1, 7) and np.array_equal(ts, [kit.tstamp(t) for t in range(T_QUERY + 1)])
    floor = interpref.floor_of(traj)
    assert georef.pose_err(a["at_knots"], traj) <= floor
    mid = _midpoints(ts)
    r = interpref.compare(a["at_mid"], traj, ts, mid, twist=a["tw_mid"])
    print("midpoints: measured %.2e envelope %.2e bound %.2e; twists x dt %.2e %.2e %.2e"
          % (r["err"], r["env"], r["bound"], r["tw_err"], r["tw_env"], r["tw_bound"]))
    assert r["ok"] and r["tw_ok"], r
    assert georef.same_bits(a["at_mid_tensor"], a["at_mid"]) and a["status"].tolist() == [0, 0, 0, 0]
    assert georef.pose_err(a["outside"], traj[[0, -1]]) <= floor


def test_a_queried_tracker_tracks_the_same_bits():
    """the two frames behind the queries: poses, patches and pose records of the queried tracker are bit-equal to those of a
    tracker that was never asked"""
    a, c = _run("queried"), _run("plain")
    assert a["still_resident"] and c["still_resident"] and a["lost"] == c["lost"] == 0
    assert a["n"] == c["n"] and np.array_equal(a["poses"], c["poses"]) and np.array_equal(a["patches"], c["patches"])
    ra, rc = a["recs"], c["recs"]
    assert len(ra) == len(rc) == T_FRAMES
    for x, y in zip(ra[-2:], rc[-2:]):
        assert x.frame == y.frame >= T_QUERY + 1 and x.tstamp == y.tstamp and x.n == y.n and x.factors == y.factors
        assert x.status == y.status and x.dropped == y.dropped and x.delta == y.delta
        assert np.array_equal(x.pose, y.pose) and np.array_equal(x.pose_inv, y.pose_inv)


def test_the_host_driven_tracker_answers_the_same():
    a, b = _run("queried"), _run("host")
    floor = interpref.floor_of(a["traj"])
    assert georef.pose_err(b["at_mid"], a["at_mid"]) <= floor and georef.pose_err(b["at_knots"], a["at_knots"]) <= floor
    assert np.abs(b["tw_mid"] - a["tw_mid"]).max() * 0.5 <= floor


# ------------------------------------------------------------------------------------------------ 9. resampling
def test_resample_trajectory_at_three_times_the_frame_rate(tmp_path):
    from rampvo_amd import evaluate
    a = _run("queried")
    traj, ts = a["traj"], a["ts"]
    out, times = evaluate.resample_trajectory(traj, ts, 6.0)                # (the frames are 0.5 s apart)
    assert len(out) == 3 * T_QUERY + 1 and np.array_equal(times[0::3], ts)
    floor = interpref.floor_of(traj)
    assert georef.pose_err(out[0::3], traj) <= floor
    r = interpref.compare(out, traj, ts, times)
    print("resampled: measured %.2e envelope %.2e bound %.2e" % (r["err"], r["env"], r["bound"]))
    assert r["ok"], r
    path = evaluate.save_fixed_rate_trajectory(str(tmp_path / "fixed" / "traj_6hz.txt"), traj, ts, 6.0)
    rows = np.loadtxt(path)
    assert rows.shape == (len(out), 8) and np.array_equal(rows[:, 0], times)
    assert np.allclose(rows[:, 1:4], out[:, :3], rtol=0, atol=1e-12) and np.allclose(rows[:, 4:], out[:, [6, 3, 4, 5]], rtol=0, atol=1e-12)
