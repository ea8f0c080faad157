"""Every query of rampvo_amd/queries.py on a tracker that runs on its OWN stream (``inputs_ready = "stream"``, the mode
``evaluate.run`` sets): the frames are produced on a side stream right before each call and overwritten right behind it, the
queries are asked from that side stream and their results copied to the host on it, with no device-wide synchronisation
between the frame and the last query.  In that mode every query reads the state on the tracker's stream and hands its
results across (queries.StateStream); tracking is bit-identical across ``inputs_ready`` modes (test_pipeline_gpu.py), so a
query asked at the same frame must return the same bits as on a tracker fed with ``inputs_ready = True`` / ``False`` -- whose
query paths the other query tests hold to their float64 restatements.  No tolerance anywhere in this file.

The tracker, its frames and the resident run are those of tests/trackerkit.py."""
import contextlib

import numpy as np
import pytest
import torch

import trackerkit as kit
from trackerkit import RADIUS, T_FRAMES, T_QUERY

pytestmark = pytest.mark.gpu


def _mid(f):
    return 100.0 + 0.5 * (np.arange(f) + 0.5)


def _ask(slam, f, frame):
    """the queries behind frame f on the current stream, in one fixed order; returns (what the tensor forms, uncertainty() and
    map() returned, copied to the host on the current stream behind the last query; what the numpy forms returned)"""
    mid = _mid(f)
    dev, res = {}, {}
    dev["trajectory"] = dict(poses=slam.trajectory(as_tensor=True)[0], traj_status=slam._traj_status)
    poses, twist, status = slam.poses_at(mid, twist=True, as_tensor=True)
    dev["poses_at"] = dict(poses=poses, twist=twist, status=status, traj_status=slam._traj_status)
    x, y, t, p = kit.query_events(f)
    dev["events_median"] = slam.compensate_events(x, y, t, p, want_xy=True, as_tensor=True)
    dev["events_map"] = slam.compensate_events(x, y, t, p, invdepth="map", radius=RADIUS, want_xy=True, as_tensor=True)
    dev["invdepth_map"] = slam.invdepth_map(radius=RADIUS, as_tensor=True)
    dev["invdepth_map_uniform"] = slam.invdepth_map(radius=RADIUS, weights="uniform", prior_rel_sigma=0.5, as_tensor=True)
    dev["uncertainty"] = slam.uncertainty()
    dev["map"] = slam.map(min_obs=2)
    res["trajectory"] = dict(poses=slam.trajectory()[0])
    poses, twist = slam.poses_at(mid, twist=True)
    res["poses_at"] = dict(poses=poses, twist=twist)
    res["invdepth_map"] = slam.invdepth_map(radius=RADIUS)
    return dict(dev=kit.host(dev), host=res)


KEYS = dict(trajectory=("poses", "traj_status"), poses_at=("poses", "twist", "status", "traj_status"),
            events_median=("status", "xy", "iwe"), events_map=("status", "xy", "iwe"),
            invdepth_map=("invdepth", "weight", "status", "pose_status"),
            invdepth_map_uniform=("invdepth", "weight", "status", "pose_status"),
            uncertainty=("frames", "cov", "pose_cov", "depth_var", "chi2", "n_valid", "dof", "sigma0_sq", "failed"),
            map=("index", "frame", "points", "point_cov", "colors", "depth_sigma_rel", "n_obs", "n_total", "chi2", "dof",
                 "sigma0_sq", "failed"))


def test_queries_of_a_resident_tracker_on_its_own_stream():
    a, b, c = kit.run_resident(True, _ask), kit.run_resident("stream", _ask), kit.run_resident("stream", None)
    for r in (a, b):
        assert r["resident_before"] and r["resident_after"] and r["resident_at_end"]
        assert sorted(r["dev"]) == sorted(KEYS)
        for q, keys in KEYS.items():
            assert sorted(r["dev"][q]) == sorted(keys), q
        assert r["dev"]["events_median"]["status"][0] == 0 and r["dev"]["events_median"]["status"][3:7].sum() == 5000
        assert r["dev"]["map"]["index"].size > 0 and r["dev"]["uncertainty"]["n_valid"] > 0
        for q in r["host"]:                                        # the numpy forms: the same bits as the tensor forms
            kit.same(r["host"][q], {k: r["dev"][q][k] for k in r["host"][q]}, "numpy form of " + q)
    assert c["resident_at_end"]
    kit.same(b["dev"], a["dev"], "own stream")
    kit.same(b["host"], a["host"], "own stream, numpy forms")
    for f in (T_QUERY + 1, T_QUERY + 2):
        assert f < T_FRAMES and a["state", f]["n"] > 0
        kit.same(b["state", f], a["state", f], "state behind the queries, frame %d" % f)
        kit.same(b["state", f], c["state", f], "state of a tracker that is never asked, frame %d" % f)


@torch.no_grad()
def _run_host_driven(ready):
    """the numpy forms of queries 1, 2, 5, 6, 7, 8 in that order.  A host-driven query that reads the window joins the
    tracker's stream (the variance map, the uniform map, uncertainty() and map() do), after which the state lives on the
    caller's stream until the next frame: so one more frame is fed in front of each query behind the first joining one, and
    EVERY query of the own-stream tracker starts with work queued on the tracker's stream (``own``)"""
    slam = kit.tracker(False, ready)
    side = torch.cuda.Stream() if ready == "stream" else None
    frames, res, own = kit.frames(), {}, []

    def ask(name, query, feed):
        nonlocal f
        if feed:
            f += 1
            kit.feed(slam, f, frames[f])
        own.append(slam._main_used)
        res[name] = kit.host(query())

    with torch.cuda.stream(side) if side is not None else contextlib.nullcontext():
        for f, frame in enumerate(frames):
            kit.feed(slam, f, frame)
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
    kit.quiesce()
    return res


def test_queries_of_a_host_driven_tracker_on_its_own_stream():
    a, b = _run_host_driven(False), _run_host_driven("stream")
    assert a["f"] == b["f"]
    assert sorted(a) == ["f", "invdepth_map", "invdepth_map_uniform", "map", "poses_at", "trajectory", "uncertainty"]
    for q in ("invdepth_map", "invdepth_map_uniform", "uncertainty", "map"):
        assert sorted(a[q]) == sorted(KEYS[q]), q
    assert a["invdepth_map"]["status"][5] > 0 and a["uncertainty"]["n_valid"] > 0 and a["map"]["index"].size > 0
    kit.same(b, a, "own stream")
