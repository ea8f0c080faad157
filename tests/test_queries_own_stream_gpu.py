"""Every query of rampvo_amd/queries.py on a tracker that runs on its OWN stream (``inputs_ready = "stream"``, the mode
``evaluate.run`` sets): the frames are produced on a side stream right before each call and overwritten right behind it, the
queries are asked from that side stream and their results copied to the host on it, with no device-wide synchronisation
between the frame and the last query.  In that mode every query reads the state on the tracker's stream and hands its
results across (queries.StateStream); tracking is bit-identical across ``inputs_ready`` modes (test_pipeline_gpu.py), so a
query asked at the same frame must return the same bits as on a tracker fed with ``inputs_ready = True`` / ``False`` -- whose
query paths the other query tests hold to their float64 restatements.  No tolerance anywhere in this file.

The tracker is the small synthetic one of the other query tests (240 x 320, 48 patches per frame, seed 77, the `wide` weights
with d_gain = 14.5, fp16 features)."""
import contextlib
import gc

import numpy as np
import pytest
import torch

import georef

pytestmark = pytest.mark.gpu

T_STREAM, T_FRAMES, T_QUERY = 46, 44, 41
RADIUS = 24.0
_cache = {}


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _frames():
    if "frames" not in _cache:
        from rampvo_amd.synthetic import SyntheticStream
        stream = SyntheticStream(240, 320, T_STREAM, seed=77, device="cuda")   # (the canvas depends on the stream's length)
        _cache["frames"] = [stream.frame(t) for t in range(T_FRAMES)]
        torch.cuda.synchronize()
    return _cache["frames"]


def _tracker(device_steps, ready):
    from rampvo_amd.config import make_cfg
    from rampvo_amd.Ramp_vo import Ramp_vo
    from rampvo_amd.synthetic import make_network
    torch.manual_seed(5)
    slam = Ramp_vo(make_cfg("default", PATCHES_PER_FRAME=48, MIXED_PRECISION=True), make_network("SingleScale", d_gain=14.5),
                   {"event_bias": True}, ht=240, wd=320)
    slam.device_steps, slam.inputs_ready = device_steps, ready
    return slam


def _quiesce():
    """(several trackers in one test: each is dropped -- with its hipGraphs -- at a quiescent point, test_pipeline_gpu.py)"""
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def _feed(slam, f, frame):
    """one frame; inputs_ready = "stream": its tensors are produced on the current stream right before the call and
    overwritten right behind it (test_pipeline_gpu.py), two intrinsics of three as device tensors"""
    im, ev, K, mask = frame
    if slam.inputs_ready != "stream":
        slam(100.0 + 0.5 * f, input_tensor=(ev, im, mask), intrinsics=K)
        return
    ev2, im2 = ev * 1.0, im * 1.0
    K2 = K.cuda() * 1.0 if f % 3 else K
    slam(100.0 + 0.5 * f, input_tensor=(ev2, im2, mask), intrinsics=K2)
    ev2.fill_(float("nan"))
    im2.fill_(float("nan"))
    if K2.is_cuda:
        K2.fill_(float("nan"))


def _host(v):
    if isinstance(v, torch.Tensor):
        return v.cpu().numpy()
    if isinstance(v, dict):
        return {k: _host(x) for k, x in v.items()}
    return v


def _mid(f):
    return 100.0 + 0.5 * (np.arange(f) + 0.5)


def _ask(slam, f):
    """the queries behind frame f on the current stream, in one fixed order; returns (what the tensor forms, uncertainty() and
    map() returned, copied to the host on the current stream behind the last query; what the numpy forms returned)"""
    mid = _mid(f)
    dev, host = {}, {}
    dev["trajectory"] = dict(poses=slam.trajectory(as_tensor=True)[0], traj_status=slam._traj_status)
    poses, twist, status = slam.poses_at(mid, twist=True, as_tensor=True)
    dev["poses_at"] = dict(poses=poses, twist=twist, status=status, traj_status=slam._traj_status)
    rng = np.random.default_rng(21)                            # (the events of test_invdepth_map_gpu.py::_run)
    n_ev = 5000
    x, y = cu(rng.uniform(0, 319, n_ev).astype(np.float32)), cu(rng.uniform(0, 239, n_ev).astype(np.float32))
    t = cu(rng.uniform(100.0 + 0.5 * (f - 2), 100.0 + 0.5 * f, n_ev))
    p = cu(rng.choice([-1, 1], n_ev).astype(np.int8))
    dev["events_median"] = slam.compensate_events(x, y, t, p, want_xy=True, as_tensor=True)
    dev["events_map"] = slam.compensate_events(x, y, t, p, invdepth="map", radius=RADIUS, want_xy=True, as_tensor=True)
    dev["invdepth_map"] = slam.invdepth_map(radius=RADIUS, as_tensor=True)
    dev["invdepth_map_uniform"] = slam.invdepth_map(radius=RADIUS, weights="uniform", prior_rel_sigma=0.5, as_tensor=True)
    dev["uncertainty"] = slam.uncertainty()
    dev["map"] = slam.map(min_obs=2)
    host["trajectory"] = dict(poses=slam.trajectory()[0])
    poses, twist = slam.poses_at(mid, twist=True)
    host["poses_at"] = dict(poses=poses, twist=twist)
    host["invdepth_map"] = slam.invdepth_map(radius=RADIUS)
    return _host(dev), host


def _same(a, b, path):
    """bit for bit: float arrays and numbers as words, integer arrays and everything else by value"""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), path
        for k in a:
            _same(a[k], b[k], path + "." + k)
    elif isinstance(a, np.ndarray) and a.dtype.kind == "f":
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and georef.same_bits(a, b), path
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b), path
    elif isinstance(a, float):
        assert georef.same_bits(np.float64(a), np.float64(b)), path
    else:
        assert type(a) is type(b) and a == b, path


KEYS = dict(trajectory=("poses", "traj_status"), poses_at=("poses", "twist", "status", "traj_status"),
            events_median=("status", "xy", "iwe"), events_map=("status", "xy", "iwe"),
            invdepth_map=("invdepth", "weight", "status", "pose_status"),
            invdepth_map_uniform=("invdepth", "weight", "status", "pose_status"),
            uncertainty=("frames", "cov", "pose_cov", "depth_var", "chi2", "n_valid", "dof", "sigma0_sq", "failed"),
            map=("index", "frame", "points", "point_cov", "colors", "depth_sigma_rel", "n_obs", "n_total", "chi2", "dof",
                 "sigma0_sq", "failed"))


def _resident(slam):
    return bool(slam._dev is not None and slam._dev.active and slam.stats["settles"] == 0)


@torch.no_grad()
def _run_resident(ready, query):
    slam = _tracker(True, ready)
    side = torch.cuda.Stream() if ready == "stream" else None
    res = {}
    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        for f, frame in enumerate(_frames()):
            _feed(slam, f, frame)
            if f == T_QUERY and query:
                res["resident_before"] = _resident(slam)
                res["dev"], res["host"] = _ask(slam, f)
                res["resident_after"] = _resident(slam)
            if f > T_QUERY:                                        # the state after frames 42 and 43
                n = slam.peek()["n"]
                res["state", f] = dict(n=n, poses=slam.poses_[:n].cpu().numpy(), patches=slam.patches_[:n].cpu().numpy())
        res["resident_at_end"] = _resident(slam)
    del slam
    _quiesce()
    return res


def test_queries_of_a_resident_tracker_on_its_own_stream():
    a, b, c = _run_resident(True, True), _run_resident("stream", True), _run_resident("stream", False)
    for r in (a, b):
        assert r["resident_before"] and r["resident_after"] and r["resident_at_end"]
        assert sorted(r["dev"]) == sorted(KEYS)
        for q, keys in KEYS.items():
            assert sorted(r["dev"][q]) == sorted(keys), q
        assert r["dev"]["events_median"]["status"][0] == 0 and r["dev"]["events_median"]["status"][3:7].sum() == 5000
        assert r["dev"]["map"]["index"].size > 0 and r["dev"]["uncertainty"]["n_valid"] > 0
        for q in r["host"]:                                        # the numpy forms: the same bits as the tensor forms
            _same(r["host"][q], {k: r["dev"][q][k] for k in r["host"][q]}, "numpy form of " + q)
    assert c["resident_at_end"]
    _same(b["dev"], a["dev"], "own stream")
    _same(b["host"], a["host"], "own stream, numpy forms")
    for f in (T_QUERY + 1, T_QUERY + 2):
        assert f < T_FRAMES and a["state", f]["n"] > 0
        _same(b["state", f], a["state", f], "state behind the queries, frame %d" % f)
        _same(b["state", f], c["state", f], "state of a tracker that is never asked, frame %d" % f)


@torch.no_grad()
def _run_host_driven(ready):
    """the numpy forms of queries 1, 2, 5, 6, 7, 8 in that order.  A host-driven query that reads the window joins the
    tracker's stream (the variance map, the uniform map, uncertainty() and map() do), after which the state lives on the
    caller's stream until the next frame: so one more frame is fed in front of each query behind the first joining one, and
    EVERY query of the own-stream tracker starts with work queued on the tracker's stream (``own``)"""
    slam = _tracker(False, ready)
    side = torch.cuda.Stream() if ready == "stream" else None
    frames, res, own = _frames(), {}, []

    def ask(name, query, feed):
        nonlocal f
        if feed:
            f += 1
            _feed(slam, f, frames[f])
        own.append(slam._main_used)
        res[name] = _host(query())

    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        for f, frame in enumerate(frames):
            _feed(slam, f, frame)
            if slam.is_initialized and slam._n >= 4:
                break
        assert slam.is_initialized and slam._dev is None and f < T_FRAMES - 4
        res["f"], mid = f, _mid(f)
        ask("trajectory", lambda: dict(poses=slam.trajectory()[0]), False)
        ask("poses_at", lambda: dict(zip(("poses", "twist"), slam.poses_at(mid, twist=True))), False)
        ask("invdepth_map", lambda: slam.invdepth_map(radius=RADIUS), False)
        ask("invdepth_map_uniform", lambda: slam.invdepth_map(radius=RADIUS, weights="uniform", prior_rel_sigma=0.5), True)
        ask("uncertainty", slam.uncertainty, True)
        ask("map", lambda: slam.map(min_obs=2), True)
        assert slam._dev is None and own == [ready == "stream"] * 6, own
    del slam, ask
    _quiesce()
    return res


def test_queries_of_a_host_driven_tracker_on_its_own_stream():
    a, b = _run_host_driven(False), _run_host_driven("stream")
    assert a["f"] == b["f"]
    assert sorted(a) == ["f", "invdepth_map", "invdepth_map_uniform", "map", "poses_at", "trajectory", "uncertainty"]
    for q in ("invdepth_map", "invdepth_map_uniform", "uncertainty", "map"):
        assert sorted(a[q]) == sorted(KEYS[q]), q
    assert a["invdepth_map"]["status"][5] > 0 and a["uncertainty"]["n_valid"] > 0 and a["map"]["index"].size > 0
    _same(b, a, "own stream")
