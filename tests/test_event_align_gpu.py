"""The event alignment on the device: ``ramp_event_align`` (csrc/contrast.hip) through ``ops.event_align(resident=True)`` and
the tracker's ``align_events(resident=True)``.

The expected value is always the state machine of tests/alignref.py driven by ``ops.event_contrast`` read on the host, one
evaluation at a time -- never the resident result itself -- and the comparison is bit for bit: the contrast's statistics are
integer sums, its gradient repeats its bits for equal arguments, and the machine's own arithmetic is a handful of float64
operations in a fixed order.  Scenes: the dot scene of tests/contrastref.py (1,200 events, 37 x 53, T = 2) and a walk of 5 knots
with 4,099 events on 24 x 32 and a depth map (the recipe of test_event_contrast_gpu.py, restated here)."""

import numpy as np
import pytest
import torch

import alignref
import contrastref
import georef
import interpref
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

_memo = {}
OUTPUTS = ("correction", "correction_f32", "result", "grad", "history", "status", "info")



def dots():
    s = contrastref.align_scene()
    return (s["x"], s["y"], s["t"], s["p"], s["knots"], s["times"], s["t_ref"], s["K"], s["invdepth"], s["H"], s["W"])


def walk(seed=8, n=4099, T=5, margin=1.5):
    H, W, K = 24, 32, np.array([30.0, 28.0, 15.5, 11.25], np.float32)
    rng = np.random.default_rng(seed)
    knots, times = interpref.walk_scene(seed + 100, T)
    x = rng.uniform(-margin, W - 1 + margin, n).astype(np.float32)
    y = rng.uniform(-margin, H - 1 + margin, n).astype(np.float32)
    t = rng.uniform(times[0] - 0.2, times[-1] + 0.2, n)
    p = rng.choice([-1, 1], n).astype(np.int8)
    d = (0.3 + 0.5 * rng.uniform(0, 1, (H, W))).astype(np.float32)
    return (x, y, t, p, knots, times, float(0.5 * (times[0] + times[-1])), K, d, H, W)


SCENES = {"dots": dots, "walk": walk}
WALK_CALL = dict(free=(1, 1, 1, 1, 1, 1, 1), step=0.02, iters=5)


def dev(name, **change):
    """the device arguments of a scene, made once"""
    key = (name,) + tuple(sorted(change))
    if key not in _memo:
        x, y, t, p, knots, times, t_ref, K, d, H, W = SCENES[name]()
        if "reversed_times" in change:
            times = times[::-1].copy()
        if "empty" in change:
            x, y, t, p = x[:0], y[:0], t[:0], p[:0]
        _memo[key] = (cu(x), cu(y), cu(np.asarray(t, np.float64)), cu(p), cu(np.asarray(knots, np.float32)),
                      cu(np.asarray(times, np.float64)), t_ref, cu(K), cu(d) if np.ndim(d) == 2 else float(d), H, W)
    return _memo[key]


def evaluator(args, signed=True, extrapolate=False):
    """``evaluate`` for alignref over ops.event_contrast read on the host; one evaluation per distinct float32 correction"""
    from rampvo_amd import ops
    memo = _memo.setdefault(("ev", id(args), signed, extrapolate), {})

    def evaluate(theta32):
        key = np.asarray(theta32, np.float32).tobytes()
        if key not in memo:
            r = ops.event_contrast(*args, correction=torch.from_numpy(np.frombuffer(key, np.float32).copy()), signed=signed,
                                   extrapolate=extrapolate)
            memo[key] = (float(r["stats"][0].cpu()), r["grad"].cpu().numpy().tolist(), r["status"].cpu().numpy())
        return memo[key]
    return evaluate


def host(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def expected(args, signed=True, extrapolate=False, **kw):
    ref_kw = dict(kw)
    if ref_kw.get("correction") is not None:
        ref_kw["correction"] = alignref.f32(ref_kw["correction"]).astype(np.float64)         # (the start is read as float32)
    return alignref.align(evaluator(args, signed, extrapolate), **ref_kw)


def resident(args, **kw):
    from rampvo_amd import ops
    return host(ops.event_align(*args, resident=True, **kw))


def check(r, ref, what=""):
    """every output of the resident call against the machine, bit for bit"""
    print(what, "evals", ref["n_evals"], "accepted", ref["n_accepted"], alignref.REASONS[ref["reason"]], "variance", ref["variance0"],
          "->", ref["variance"], "| device info", r["info"].tolist())
    assert r["info"].tolist() == ref["info"].tolist(), what
    assert georef.same_bits(r["correction"], ref["correction"]) and georef.same_bits(r["correction_f32"], ref["correction_f32"]), what
    assert georef.same_bits(r["result"], np.array([ref["variance"], ref["variance0"], ref["length"], 0.0])), what
    assert georef.same_bits(r["variance"], np.float64(ref["variance"])) and georef.same_bits(r["variance0"], np.float64(ref["variance0"]))
    assert georef.same_bits(r["grad"], ref["grad"]) and georef.same_bits(r["history"], ref["history_full"]), what
    assert np.array_equal(r["status"], ref["status"]), what


def same_outputs(a, b, what=""):
    for k in OUTPUTS:
        assert georef.same_bits(a[k], b[k]) if a[k].dtype.kind == "f" else np.array_equal(a[k], b[k]), (what, k)


# ------------------------------------------------------------------------------------------------ 1. bit for bit
CASES = [("dots", name, kw) for name, kw in alignref.CALLS.items()] + [("walk", "walk", WALK_CALL)]


@pytest.mark.parametrize("scene,name,kw", CASES, ids=[c[1] for c in CASES])
def test_the_resident_loop_is_the_host_loop_bit_for_bit(scene, name, kw):
    from rampvo_amd import ops
    args = dev(scene)
    ref = expected(args, **kw)
    r = resident(args, **kw)
    check(r, ref, name)
    # the words of the evaluation at the result, from a fresh evaluation there
    again = ops.event_contrast(*args, correction=cu(r["correction_f32"]))
    assert np.array_equal(again["status"].cpu().numpy(), r["status"]) and georef.same_bits(again["stats"][:1].cpu().numpy(), r["result"][:1])
    assert georef.same_bits(again["grad"].cpu().numpy(), r["grad"])
    # and the host form of the same call
    h = ops.event_align(*args, **kw)
    assert georef.same_bits(np.asarray(h["correction"], np.float64), r["correction"])
    assert georef.same_bits(np.asarray(h["history"], np.float64), r["history"][:ref["n_accepted"]])
    assert georef.same_bits(np.float64(h["variance"]), r["variance"]) and georef.same_bits(np.float64(h["variance0"]), r["variance0"])
    assert len(h["history"]) == r["info"][1]


# ------------------------------------------------------------------------------------------------ 2. budget, the done word
def test_budgets():
    args = dev("dots")
    full = expected(args)
    need, cap = full["n_evals"], 1 + 9 * 20
    assert 10 < need < cap
    for budget in (1, 2, 10, need - 1, need, need + 1, cap + 1000):
        ref = expected(args, max_evals=budget)
        r = resident(args, max_evals=budget)
        check(r, ref, "max_evals=%d" % budget)
        assert (ref["reason"] == alignref.BUDGET) == (budget < need) and ref["n_evals"] == min(budget, need)
        if budget >= need:                           # behind the end of the search: empty launches, the same bits in every output
            same_outputs(r, resident(args), "budget %d against the full budget" % budget)
    ten = resident(args, max_evals=10)
    assert ten["correction"].tolist() == full["thetas"][9]


def test_event_contrast_around_an_alignment_on_the_same_workspace():
    from rampvo_amd import ops
    args = dev("walk")
    theta = np.array([0.3, -0.2, 0.15, 0.25, -0.3, 0.5, 0.2], np.float32)
    before = host(ops.event_contrast(*args, correction=theta, want_iwe=True))
    r = resident(args, max_evals=1 + 9 * 5, **WALK_CALL)
    after = host(ops.event_contrast(*args, correction=theta, want_iwe=True))
    assert r["info"][2] < 1 + 9 * 5                                          # (the done word was set: empty launches ran last)
    for k in before:
        assert georef.same_bits(before[k], after[k]) if before[k].dtype.kind == "f" else np.array_equal(before[k], after[k]), k
    assert before["status"][0] == 0 and before["stats"][0] > 0


def test_the_result_goes_straight_into_event_contrast():
    from rampvo_amd import ops
    args = dev("dots")
    r = ops.event_align(*args, resident=True, iters=6)
    c = ops.event_contrast(*args, correction=r["correction_f32"], want_iwe=True)
    assert georef.same_bits(c["variance"].cpu().numpy(), r["variance"].cpu().numpy()) and float(r["variance"]) > float(r["variance0"])
    assert georef.same_bits(c["grad"].cpu().numpy(), r["grad"].cpu().numpy()) and float(c["iwe"].abs().sum()) > 0
    info = ops.event_align_info(r["info"])
    assert info == dict(reason="iters", n_accepted=6, n_evals=int(r["info"][2]), halvings=0, seen=0, bad_times=False, bad_correction=False)


# ------------------------------------------------------------------------------------------------ 3. failures
def test_decreasing_knot_times():
    """FLAT after one evaluation, NaN variance, bit 0 in ``seen`` and in the status words -- with a budget of 5 as well: the
    evaluations behind the first never run, so nothing clears the bit"""
    args = dev("dots", reversed_times=True)
    for budget in (1, 5, None):
        r = resident(args, max_evals=budget)
        assert r["info"].tolist() == [alignref.FLAT, 0, 1, 0, 1, 0, 0, 0], budget
        assert np.isnan(r["variance"]) and np.isnan(r["variance0"]) and np.isnan(r["grad"]).all() and np.isnan(r["history"]).all()
        assert r["status"][0] == 1 and not r["correction"].any() and not r["correction_f32"].any()
        check(r, expected(args, max_evals=budget), "reversed times, budget %s" % budget)
    r = resident(args, iters=0)
    assert r["info"].tolist() == [alignref.ITERS, 0, 1, 0, 1, 0, 0, 0] and np.isnan(r["variance"])


def test_a_correction_that_is_not_finite():
    args = dev("dots")
    start = [0.0, 0.0, 0.0, float("nan"), 0.0, 0.0, 0.0]
    r = resident(args, correction=start)
    assert r["info"].tolist() == [alignref.FLAT, 0, 1, 0, 2, 0, 0, 0] and r["status"][0] == 2 and np.isnan(r["variance"])
    assert np.isnan(r["correction"][3]) and np.isnan(r["correction_f32"][3])
    check(r, expected(args, correction=start), "NaN start")


def test_a_step_that_overflows_float32():
    """step = 1e39: the first trials are infinite in float32 and rejected through BAD_CORRECTION; the lengths halve into range
    and the search goes on.  ``seen`` keeps bit 1, the final status is clean, and the host loop agrees"""
    from rampvo_amd import ops
    args = dev("dots")
    kw = dict(step=1e39, iters=2)
    ref = expected(args, **kw)
    r = resident(args, **kw)
    check(r, ref, "step=1e39")
    assert ref["seen"] & 2 and r["info"][4] & 2 and r["status"][0] == 0 and np.isfinite(r["variance"])
    h = ops.event_align(*args, **kw)
    assert georef.same_bits(np.asarray(h["correction"], np.float64), r["correction"])
    assert georef.same_bits(np.float64(h["variance"]), r["variance"]) and len(h["history"]) == r["info"][1]


# ------------------------------------------------------------------------------------------------ 4. edges
def test_no_events():
    """N == 0: the step kernel alone answers for the all-zero statistics, as the host loop over ops.event_contrast does"""
    from rampvo_amd import ops
    args = dev("dots", empty=True)
    start = [0.0, 0.0, 0.0, 0.5, 0.0, -0.25, 0.0]
    for kw in (dict(), dict(correction=start, iters=3), dict(iters=0)):
        r = resident(args, **kw)
        assert r["info"].tolist() == [alignref.ITERS if kw.get("iters") == 0 else alignref.FLAT, 0, 1, 0, 0, 0, 0, 0]
        assert r["variance"] == 0 and r["variance0"] == 0 and not r["grad"].any() and not r["status"].any()
        assert r["correction"].tolist() == kw.get("correction", [0.0] * 7) and np.isnan(r["history"]).all()
        check(r, expected(args, **kw), "N = 0")
        h = ops.event_align(*args, **kw)
        assert h["correction"] == r["correction"].tolist() and h["variance"] == 0 and h["history"] == []


@pytest.mark.parametrize("kw", [dict(iters=0), dict(signed=False, iters=4), dict(extrapolate=True, **WALK_CALL),
                                dict(extrapolate=False, signed=False, **WALK_CALL)], ids=["iters0", "unsigned", "extrapolate", "walk-unsigned"])
def test_edges(kw):
    args = dev("walk" if "extrapolate" in kw else "dots")
    ref = expected(args, **kw)
    r = resident(args, **kw)
    check(r, ref, str(kw))
    if kw.get("iters") == 0:
        assert r["info"].tolist()[:3] == [alignref.ITERS, 0, 1] and r["history"].shape == (0,) and r["variance"] == r["variance0"] > 0
    else:
        assert ref["n_accepted"] > 0
    if kw.get("extrapolate"):
        other = expected(args, **dict(kw, extrapolate=False))
        assert r["status"][1] + r["status"][2] > 0 and not georef.same_bits(other["grad"], ref["grad"])     # (events off the knots' range)


# ------------------------------------------------------------------------------------------------ 5. refusals, memory
def test_refusals_canaries_and_repeated_bits():
    """the C entry with guard words on both sides of every output and of the workspace; three calls repeat every bit"""
    from rampvo_amd import _lib
    L = _lib.lib()
    iters = 5
    dx, dy, dt, dp, dk, dtm, t_ref, dK, dd, H, W = dev("walk")
    T, N = dk.shape[0], dx.shape[0]
    nbytes = L.ramp_event_align_workspace_bytes(T, H, W)
    assert nbytes >= L.ramp_event_contrast_workspace_bytes(T, H, W) + 400 and nbytes % 8 == 0

    bufs = dict(correction=Flat(7, torch.float64, -7.0), correction_f32=Flat(7, torch.float32, -7.0),
                result=Flat(4, torch.float64, -7.0), grad=Flat(7, torch.float64, -7.0), history=Flat(iters, torch.float64, -7.0),
                status=Flat(8, torch.int32, -7), info=Flat(8, torch.int32, -7), ws=Flat(nbytes, torch.uint8, 0xA5))
    assert bufs["ws"].t.data_ptr() % 16 == 0
    P = _lib.ptr

    def call(N=N, ws_bytes=nbytes, flags=_lib.RAMP_WARP_DEPTH_MAP, free_mask=127, step=0.02, iters=iters, max_evals=1000, t_ref=t_ref,
             skip=None, cor=None):
        o = lambda k: None if k == skip else P(bufs[k].t)
        rc = L.ramp_event_align(P(dx), P(dy), P(dt), P(dp), N, P(dk), P(dtm), T, t_ref, P(dK), P(dd), cor, flags, H, W, free_mask,
                                step, iters, max_evals, o("correction"), o("correction_f32"), o("result"), o("grad"), o("history"),
                                o("status"), o("info"), o("ws"), ws_bytes, _lib.stream())
        torch.cuda.synchronize()
        return rc

    before = {k: v.snapshot() for k, v in bufs.items()}
    for kw in (dict(N=-1), dict(flags=_lib.RAMP_WARP_IDENTITY), dict(free_mask=128), dict(step=float("inf")), dict(step=float("nan")),
               dict(t_ref=float("nan")), dict(iters=-1), dict(iters=65537), dict(max_evals=0)) + tuple(dict(skip=k) for k in bufs):
        assert call(**kw) == -1, kw
    assert call(ws_bytes=nbytes - 8) == -3 and call(N=0, ws_bytes=nbytes - 8) == -3
    assert all(bufs[k].unchanged(before[k]) for k in bufs)                 # nothing written by a refused call
    ref = expected(dev("walk"), **WALK_CALL)
    runs = []
    for _ in range(3):
        for k in OUTPUTS:
            bufs[k].t.fill_(-7)
        assert call() == 0                                                       # (max_evals = 1000 is clamped to 1 + 9 * iters)
        for k, b in bufs.items():
            assert b.intact(), k
        runs.append({k: bufs[k].t.cpu().numpy().copy() for k in OUTPUTS})
        runs[-1]["variance"], runs[-1]["variance0"] = runs[-1]["result"][0], runs[-1]["result"][1]
        check(runs[-1], ref, "the C entry")
    same_outputs(runs[0], runs[1], "second call")
    same_outputs(runs[0], runs[2], "third call")


def test_a_side_stream():
    args = dev("dots")
    main = resident(args, iters=4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = resident(args, iters=4)
    torch.cuda.current_stream().wait_stream(side)
    same_outputs(main, other, "side stream")
    check(other, expected(args, iters=4), "side stream")


# ------------------------------------------------------------------------------------------------ 6. tracker
SENSOR = dict(model="radtan", raw_intrinsics=(205.0, 204.0, 158.5, 121.5), coeffs=(-0.3, 0.1, 5e-4, -4e-4, 0.0))
FILTER = dict(support_dt=0.02, refractory=1e-4, hot_count=20)
HOST_KEYS = ["correction", "history", "n_accepted", "n_evals", "reason", "variance", "variance0"]


def _raw_events(f, n_ev=4000):
    rng = np.random.default_rng(31)
    return (cu(rng.integers(100, 160, n_ev).astype(np.int32)), cu(rng.integers(100, 140, n_ev).astype(np.int32)),
            cu(np.sort(rng.uniform(100.0 + 0.5 * (f - 2), 100.0 + 0.5 * f, n_ev))), cu(rng.choice([-1, 1], n_ev).astype(np.int8)))


def _same_as_host_form(res, h, what):
    assert sorted(k for k in res if not k.endswith("_status")) == HOST_KEYS, what
    assert isinstance(res["correction"], list) and len(res["correction"]) == 7 and isinstance(res["variance"], float)
    assert georef.same_bits(np.asarray(res["correction"]), np.asarray(h["correction"], np.float64)), what
    assert georef.same_bits(np.asarray(res["history"]), np.asarray(h["history"], np.float64)) and len(res["history"]) == res["n_accepted"]
    assert georef.same_bits(np.float64(res["variance"]), np.float64(h["variance"])), what
    assert georef.same_bits(np.float64(res["variance0"]), np.float64(h["variance0"])), what


def _ask(slam, f, frame):
    from rampvo_amd import ops
    x, y, t, p = kit.query_events(f)
    res = {}
    out = slam.align_events(x, y, t, p, iters=2, as_tensor=True)
    res["read"] = slam.align_events(x, y, t, p, iters=2, resident=True)
    res["host"] = slam.align_events(x, y, t, p, iters=2)
    knots, ts = slam.trajectory(as_tensor=True)
    n = slam.peek()["n"]
    med = torch.median(slam.patches_[n - 3:n, :, 2])
    ref = ops.event_align(x, y, t, p, knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), frame[2].cuda().float(), med, 240, 320,
                          iters=2, resident=True)
    res["out"], res["ref"] = kit.host(out), kit.host(ref)
    xr, yr, tr, pr = _raw_events(f)
    slam.set_camera(**SENSOR)
    slam.set_event_filter(**FILTER)
    res["passed"] = slam.align_events(xr, yr, tr, pr, iters=1, distorted=True, denoise=True, resident=True)
    res["passed_host"] = slam.align_events(xr, yr, tr, pr, iters=1, distorted=True, denoise=True)
    res["passed_dev"] = kit.host(slam.align_events(xr, yr, tr, pr, iters=1, distorted=True, denoise=True, as_tensor=True))
    return res


def test_tracker_align_events_device_resident():
    """slam.align_events(resident=True) equals ops.event_align(resident=True) on trajectory(as_tensor=True), the fed intrinsics
    and the tracker's depth median, and the host form; the tracker stays device resident and ends with the pose bits of one never
    asked; distorted=True and denoise=True pass through"""
    a, c = kit.run_resident(True, _ask), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_after"] and a["resident_at_end"] and c["resident_at_end"]
    kit.same(a["out"], a["ref"], "against ops.event_align")
    assert sorted(a["out"]) == sorted(OUTPUTS + ("variance", "variance0"))
    _same_as_host_form(a["read"], a["host"], "one read")
    assert georef.same_bits(np.asarray(a["read"]["correction"]), a["out"]["correction"]) and a["read"]["n_evals"] == a["out"]["info"][2]
    assert a["read"]["reason"] in ("iters", "stalled") and a["read"]["variance"] >= a["read"]["variance0"] > 0
    _same_as_host_form(a["passed"], a["passed_host"], "distorted and denoised")
    for k in ("rectify_status", "filter_status"):
        assert np.array_equal(a["passed"][k], a["passed_host"][k]) and np.array_equal(a["passed"][k], a["passed_dev"][k]), k
    assert a["passed"]["filter_status"][7] > 500 and a["passed"]["rectify_status"][0] == 0
    for f in (kit.T_QUERY + 1, kit.T_QUERY + 2):
        kit.same(a["state", f], c["state", f], "state of a tracker that is never asked, frame %d" % f)


@torch.no_grad()
def test_tracker_align_events_host_driven():
    from rampvo_amd import ops
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    x, y, t, p = (v.cpu().numpy() for v in kit.query_events(f, 1000))
    res = slam.align_events(x, y, t, p, iters=2, resident=True)                       # numpy in, one read
    _same_as_host_form(res, slam.align_events(x, y, t, p, iters=2), "host driven")
    knots, ts = slam.trajectory(as_tensor=True)
    med = torch.median(slam.patches_[slam._n - 3:slam._n, :, 2])
    ref = ops.event_align(cu(x), cu(y), cu(t), cu(p), knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), frame[2].cuda().float(), med,
                          240, 320, iters=2, resident=True)
    kit.same(kit.host(slam.align_events(x, y, t, p, iters=2, as_tensor=True)), kit.host(ref), "against ops.event_align")
    slam.tlist = slam.tlist[::-1]
    with pytest.raises(RuntimeError, match="time stamps decrease"):
        slam.align_events(x, y, t, p, iters=1, resident=True)
    quiet = slam.align_events(x, y, t, p, iters=1, as_tensor=True)                    # nothing raised: the words say it
    assert int(quiet["info"][4]) & 1 and int(quiet["info"][0]) == alignref.FLAT and bool(torch.isnan(quiet["variance"]))
    del slam
    kit.quiesce()
