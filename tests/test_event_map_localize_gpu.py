"""Localisation against the event map on the GPU: ``ramp_point_map_localize_eval`` and ``ramp_point_map_localize``
(csrc/maplocalize.hip) through the C entry points (every buffer between canaries, tests/guarded.py), ``ops.PointMap.localize_eval``
/ ``localize`` and the tracker's ``event_map_localize``.

The table is read back from the device as it is, so every comparison is per SLOT.  ``records[:, :2]`` are the renderer's u, v bit
for bit; r, gu, gv are held bit for bit to the fp32 emulator on the call's own u, v and surface; Xc to float64 by the bound rule
of test_geometry_f64_gpu.py; the sums to the float64 sum of the emulator's per-slot terms formed from the call's own records
within the textbook bound (n - 1) 2^-53 sum |term| per word.  The loop is held BIT FOR BIT to ``localizeref.Machine`` driven by
``PointMap.localize_eval`` read on the host.  Nothing here provokes a fault."""
import ctypes

import numpy as np
import pytest
import torch

import georef
import localizeref as lr
import renderref as rr
import trackerkit as kit
from guarded import Flat
from test_event_map_render_gpu import GMap
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W, V = lr.H, lr.W, lr.VOXEL
P = lambda f: ctypes.c_void_p(f.address()) if isinstance(f, Flat) else (None if f is None else ctypes.c_void_p(f.data_ptr()))
bits = lambda a: np.ascontiguousarray(a).reshape(-1).view({4: np.uint32, 8: np.uint64}[np.asarray(a).dtype.itemsize])
SURF = lr.surface_13x17(0)


def evaluate(g, surface=SURF, cam=lr.CAM, Kc=lr.K, min_points=1, min_views=1, huber=0.0, records=True, expect=0, **over):
    """the C entry with every buffer between canaries -> numpy dict"""
    from rampvo_amd import _lib
    L = g.L
    h, w = surface.shape
    nbytes = L.ramp_point_map_localize_ws_bytes(g.cap, 0)
    b = dict(sums=Flat(32, torch.float64), records=Flat((g.cap, 8), torch.float32), status=Flat(8, torch.int32), ws=Flat(nbytes, torch.uint8, rows=4))
    d_cam, d_K, d_S = cu(np.asarray(cam, np.float32)), cu(np.asarray(Kc, np.float32)), cu(np.asarray(surface, np.float32))
    torch.cuda.synchronize()
    before, table = {k: v.snapshot() for k, v in b.items()}, g.buf.snapshot()
    a = dict(p_map=P(g.buf), cap=g.cap, voxel=g.voxel, min_points=min_points, min_views=min_views, p_cam=P(d_cam), p_K=P(d_K), p_surface=P(d_S),
             H=h, W=w, huber=huber, p_sums=P(b["sums"]), p_records=P(b["records"]) if records else None, p_ws=P(b["ws"]), nbytes=nbytes,
             p_status=P(b["status"]))
    assert set(over) <= set(a), over
    a.update(over)
    rc = L.ramp_point_map_localize_eval(*a.values(), _lib.stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, over)
    assert all(v.intact() for v in b.values()) and g.buf.unchanged(table), "the evaluation does not write the map"
    if rc:
        assert all(v.unchanged(before[k]) for k, v in b.items()), "a refused call touches nothing"
        return None
    assert records or b["records"].unchanged(before["records"])
    return {k: b[k].t.cpu().numpy() for k in ("sums", "records", "status")}


WORST = [0.0]


def check(g, out, name, surface=SURF, cam=lr.CAM, Kc=lr.K, min_points=1, min_views=1, huber=0.0):
    rec, st = out["records"], out["status"]
    e = lr.evaluate_records(g.tab, rec, Kc, surface, min_points, min_views, huber)
    kind = e["kind"]
    assert st.tolist() == [0, (kind != lr.ABSENT).sum(), (kind == lr.FILTERED).sum(), (kind == lr.REJECTED).sum(), (kind == lr.OUT).sum(),
                           (kind == lr.IN).sum(), 0, 0], (name, st)
    assert st[2] + st[3] + st[4] + st[5] == st[1] == (g.tab["key"] >= 0).sum(), name
    assert np.isnan(rec[kind <= lr.FILTERED]).all() and np.isnan(rec[kind == lr.REJECTED][:, :5]).all() and np.isnan(rec[kind == lr.OUT][:, 2:5]).all()
    assert not np.isnan(rec[kind >= lr.REJECTED][:, 5:]).any(), name
    at = e["at"]
    for col, what in ((2, "r"), (3, "gu"), (4, "gv")):        # bit for bit where the emulator's word is a number, NaN where it is NaN
        num = ~np.isnan(e[what])
        assert np.array_equal(bits(rec[at, col][num]), bits(e[what][num])) and np.isnan(rec[at, col][~num]).all(), (name, what)
    if np.isnan(surface).any():                               # a NaN pixel reaches the slots whose four neighbours hold it, no other
        x0, y0 = np.floor(rec[at, 0]).astype(int), np.floor(rec[at, 1]).astype(int)
        touched = np.isnan(surface[y0, x0]) | np.isnan(surface[y0, x0 + 1]) | np.isnan(surface[y0 + 1, x0]) | np.isnan(surface[y0 + 1, x0 + 1])
        assert touched.any() and not touched.all() and np.isnan(rec[at, 2][touched]).all(), name
        assert np.isfinite(rec[at, 2:5][~touched]).all(), name + ": slots away from the NaN pixel keep finite r, gu, gv"
    # the renderer's u, v, bit for bit
    ren = g.render(cam=cam, Kc=Kc, h=surface.shape[0], w=surface.shape[1], min_points=min_points, min_views=min_views)["records"]
    assert np.array_equal(bits(rec[:, :2]), bits(ren[:, :2])), name + ": the renderer's u, v"
    # Xc against float64, the kinds against the float64 restatement (the scenes keep their margins)
    r32, r64 = (lr.evaluate(g.tab, g.voxel, cam, Kc, surface, min_points, min_views, huber, dtype=t) for t in (np.float32, np.float64))
    assert np.array_equal(kind, r64["kind"]), name + ": the same slots are in reach"
    part = kind >= lr.REJECTED
    if part.any():
        err, env = georef.max_err(rec[part, 5:], r64["records"][part, 5:]), georef.max_err(r32["records"][part, 5:], r64["records"][part, 5:])
        floor = georef.PIXEL_FLOOR * max(1.0, float(np.abs(r64["records"][part, 5:]).max()))
        assert err <= georef.bound(floor, env), (name, err, env, floor)
    # the sums within the textbook bound of a float64 sum of n terms
    assert np.array_equal(out["sums"][28:], [st[5], st[3] + st[4] + st[5], 0, 0]), name
    if np.isnan(surface).any():
        assert np.isnan(out["sums"][27])
        return
    tol = np.maximum(e["n"] - 1, 0) * 2.0 ** -53 * e["abs_sums"][:28]
    diff = np.abs(out["sums"][:28] - e["sums"][:28])
    ratio = float(np.max(np.where(tol > 0, diff / np.where(tol > 0, tol, 1), np.where(diff > 0, np.inf, 0))))
    WORST[0] = max(WORST[0], ratio)
    print("localize eval %s: status %s, cost %.6g, largest |sum - float64 sum| / bound %.3g (so far %.3g)" % (name, st.tolist(), out["sums"][27], ratio, WORST[0]))
    assert (diff <= tol).all(), (name, diff, tol)


_maps = {}


def table(N, seed=None, capacity=1 << 13):
    key = (N, seed, capacity)
    if key not in _maps:
        _maps[key] = GMap(lr.loc_cloud(N, seed=N if seed is None else seed), capacity)
    return _maps[key]


# ------------------------------------------------------------------------------------------------ 1. the evaluation
@pytest.mark.parametrize("N,capacity", ((0, 8), (1, 8), (2, 8), (6, 8), (6, 1 << 13), (4099, 1 << 13)))
def test_evaluation_records_and_sums(N, capacity):
    g = table(N, 7 if N == 4099 else None, capacity)
    out = evaluate(g)
    check(g, out, "N=%d capacity=%d" % (N, capacity))
    if N == 0:
        assert not out["sums"].any() and not out["status"].any() and np.isnan(out["records"]).all()
    again = evaluate(g)                                        # a call repeats its bits
    for k in ("sums", "records", "status"):
        assert np.array_equal(bits(out[k]), bits(again[k])), k
    none = evaluate(g, records=False)
    assert np.array_equal(bits(out["sums"]), bits(none["sums"])) and np.array_equal(out["status"], none["status"])


def test_a_table_the_slot_loop_takes_two_trips_over():
    from rampvo_amd import _lib
    slots = _lib.lib().ramp_point_map_localize_grid_slots()
    cap = 1 << int(2 * slots - 1).bit_length()
    assert cap >= 2 * slots
    g = table(4099, 7, cap)
    out = evaluate(g)
    check(g, out, "two trips, capacity %d" % cap)
    assert (g.tab["key"][slots:] >= 0).any(), "voxels behind the first trip"
    assert out["status"][1] == 4099


def test_an_evaluation_on_a_side_stream():
    """the C entry and PointMap.localize_eval on a torch.cuda.Stream(): sums, records and status are the default stream's bits"""
    g = table(4099, 7)
    ref = evaluate(g, huber=0.5)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        out = evaluate(g, huber=0.5)                           # (_lib.stream() is the side stream here)
    side.synchronize()
    for k in ("sums", "records", "status"):
        assert np.array_equal(bits(out[k]), bits(ref[k])), k
    # through ops, on ONE table (another table's inserts may place a voxel in another slot, and move the sums' rounding)
    m = _ops_map(lr.loc_cloud(4099, seed=7))
    S, cam = cu(SURF), cu(lr.CAM)
    here = kit.host(m.localize_eval(S, cam, lr.K, huber=0.5, want_records=True))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = m.localize_eval(S, cam, lr.K, huber=0.5, want_records=True)
    side.synchronize()
    for k in ("sums", "records", "status", "cost", "hessian", "gradient", "in_reach"):
        assert np.array_equal(bits(r[k].cpu().numpy()), bits(here[k])), k
    assert here["status"].tolist() == ref["status"].tolist() and here["hessian"].shape == (6, 6)
    assert np.array_equal(bits(here["cost"]), bits(here["sums"][27])) and abs(here["cost"] - ref["sums"][27]) <= 1e-9 * ref["sums"][27]


def test_filters_huber_views_and_the_depth_limit():
    g = table(4099, 7)
    for kw in (dict(min_points=2), dict(min_views=2), dict(min_points=3, min_views=2), dict(min_points=0, min_views=0), dict(min_points=10 ** 6),
               dict(huber=0.5), dict(huber=0.05), dict(huber=5.0), dict(huber=-1.0)):
        out = evaluate(g, **kw)
        check(g, out, "%s" % kw, **kw)
    off, on = evaluate(g), evaluate(g, huber=0.5)
    assert on["sums"][27] < off["sums"][27] and np.array_equal(bits(evaluate(g, huber=5.0)["sums"]), bits(off["sums"]))
    assert off["status"][3] >= 8 and off["status"][4] > 100, "rejected (behind the camera, nearer than RAMP_WARP_MIN_Z) and out of reach"
    gv = GMap(rr.view_case())                                  # views 0, 63, 64: 64 wraps onto 0
    for mv, filtered in ((1, 0), (2, 2), (3, 3)):
        out = evaluate(gv, cam=rr.pm.IDENTITY, min_views=mv)
        check(gv, out, "views %d" % mv, cam=rr.pm.IDENTITY, min_views=mv)
        assert out["status"][2] == filtered
    # a voxel at exactly RAMP_WARP_MIN_Z is rejected, the next float32 above it is not (identity camera: z is the point's)
    # (voxel 0.2: the point z = float32(0.2) has the index 1 and the fraction 0, so its mean point is float32(1 * 0.2) again)
    gz = GMap([(np.float32([[0.01, 0.01, rr.MIN_Z], [0.3, 0.01, 0.6]]), None, 0)], voxel=0.2)
    zs = rr.mean_points(gz.tab, 0.2)[gz.tab["key"] >= 0][:, 2]
    assert (zs == rr.MIN_Z).sum() == 1 and (zs > rr.MIN_Z).sum() == 1, zs
    out = evaluate(gz, cam=rr.pm.IDENTITY)
    assert out["status"][1] == 2 and out["status"][3] == 1, out["status"]


def test_points_out_of_reach_on_each_border():
    """one voxel just outside and one just inside each border's last cell, through the identity camera"""
    Kc = np.float32([8.0, 8.0, 0.0, 0.0])
    z = 2.0
    uv = [(-0.3, 5.3), (0.3, 5.3), (W - 1.3, 5.3), (W - 0.7, 5.3), (5.3, -0.3), (5.3, 0.3), (5.3, H - 1.3), (5.3, H - 0.7)]
    pts = np.float32([[(u - Kc[2]) / Kc[0] * z, (v - Kc[3]) / Kc[1] * z, z] for u, v in uv])
    g = GMap([(pts, None, 0)], voxel=0.01)
    assert (g.tab["key"] >= 0).sum() == 8
    out = evaluate(g, cam=rr.pm.IDENTITY, Kc=Kc)
    check(g, out, "borders", cam=rr.pm.IDENTITY, Kc=Kc)
    assert out["status"].tolist() == [0, 8, 0, 0, 4, 4, 0, 0]
    assert out["sums"][27] >= 4.0, "a voxel out of reach keeps the residual 1"


def test_a_nan_pixel_a_bad_camera_and_the_refusals():
    from rampvo_amd import _lib
    g = table(4099, 7)
    S = SURF.copy()
    S[6, 8] = np.nan
    out = evaluate(g, surface=S)
    check(g, out, "one NaN pixel", surface=S)
    assert np.isnan(out["sums"][27]) and out["status"][0] == 0
    g2 = table(2)
    for word in range(11):
        for bad in (np.nan, np.inf):
            cam, Kc = lr.CAM.copy(), lr.K.copy()
            (cam if word < 7 else Kc)[word if word < 7 else word - 7] = bad
            out = evaluate(g2, cam=cam, Kc=Kc)
            assert out["status"].tolist() == [1] + [0] * 7 and np.isnan(out["sums"]).all() and np.isnan(out["records"]).all(), word
    for i in (0, 1):
        Kc = lr.K.copy()
        Kc[i] = 0
        assert evaluate(g2, Kc=Kc)["status"].tolist() == [1] + [0] * 7
    for over in (dict(H=1), dict(W=1), dict(cap=12), dict(cap=4), dict(cap=1 << 31), dict(voxel=0.0), dict(voxel=-1.0), dict(voxel=float("nan")),
                 dict(voxel=float("inf")), dict(min_points=-1), dict(min_views=-1), dict(p_map=None), dict(p_cam=None), dict(p_K=None),
                 dict(p_surface=None), dict(p_sums=None), dict(p_ws=None), dict(p_status=None), dict(huber=float("nan")),
                 dict(p_map=ctypes.c_void_p(g2.buf.address() + 8))):
        evaluate(g2, expect=_lib.RAMP_EINVAL, **over)
    evaluate(g2, expect=_lib.RAMP_EUNSUPPORTED, H=1 << 16, W=1 << 15)
    evaluate(g2, expect=_lib.RAMP_EWORKSPACE, nbytes=_lib.lib().ramp_point_map_localize_ws_bytes(g2.cap, 0) - 1)


# ------------------------------------------------------------------------------------------------ 2. the loop
def _ops_map(inserts, voxel=V, capacity=1 << 13):
    from rampvo_amd import ops
    m = ops.PointMap(voxel, capacity=capacity)
    for p, c, view in inserts:
        m.insert(cu(np.asarray(p, np.float32)), None if c is None else cu(np.asarray(c, np.float32)), view=view)
    return m


def _both(m, surface, cam, Kc, **kw):
    """(the device loop, the Machine driven by PointMap.localize_eval read on the host)"""
    S, loop_kw = cu(np.asarray(surface, np.float32)), {k: v for k, v in kw.items() if k in ("lambda0", "min_step", "iters", "max_evals")}
    ev_kw = {k: v for k, v in kw.items() if k not in loop_kw}
    dev = kit.host(m.localize(S, cu(np.asarray(cam, np.float32)), Kc, **kw))

    def fn(pose32):
        o = kit.host(m.localize_eval(S, cu(pose32), Kc, **ev_kw))
        return o["sums"][27], o["sums"][:21], o["sums"][21:27], o["sums"][28], o["status"]

    return dev, lr.localize(fn, np.asarray(cam, np.float32), **loop_kw)


def _same_loop(dev, ref, name):
    print("localize %s: reason %s, info %s, cost %.6g -> %.6g" % (name, lr.REASONS[int(dev["info"][0])], dev["info"].tolist(), dev["result"][1], dev["result"][0]))
    assert dev["info"].tolist() == ref["info"].tolist(), (name, dev["info"], ref["info"])
    for k in ("pose", "pose_f32", "result", "hessian", "gradient", "history"):
        assert np.array_equal(bits(dev[k]), bits(ref[k])), (name, k, dev[k], ref[k])
    assert dev["status"].tolist() == ref["status"].tolist(), name
    assert np.array_equal(bits(dev["cost"]), bits(ref["result"][0])) and np.array_equal(bits(dev["cost0"]), bits(ref["result"][1]))
    n = int(dev["info"][1])
    assert np.isnan(dev["history"][n:]).all() and not np.isnan(dev["history"][:n]).any()


def test_the_convergence_scene_ends_with_the_machines_bits():
    from rampvo_amd import ops
    s = lr.convergence_scene()
    m = _ops_map(s["inserts"], s["voxel"])
    x, y, t = s["events"]
    ts = ops.time_surface(cu(x), cu(y), cu(t), s["t_ref"], s["tau"], s["h"], s["w"], smooth=s["smooth"])
    surface = ts["surface"].cpu().numpy()
    dev, ref = _both(m, surface, s["start"], s["K"], iters=s["iters"])
    _same_loop(dev, ref, "convergence scene")
    t0, r0 = lr.pose_distance(s["start"], s["true"])
    t1, r1 = lr.pose_distance(dev["pose"], s["true"])
    print("convergence scene on the device: translation %.4f -> %.4f, rotation %.4f -> %.4f" % (t0, t1, r0, r1))
    assert int(dev["info"][0]) in (lr.ITERS, lr.CONVERGED) and dev["result"][0] < dev["result"][1] and t1 < 0.5 * t0 and r1 < 0.5 * r0
    need = int(dev["info"][2])
    # a start at the optimum, no step asked for, and budgets of 1, 2 and one below the need
    for name, cam, kw in (("at the optimum", dev["pose_f32"], dict(iters=3)), ("iters 0", s["start"], dict(iters=0)),
                          ("max_evals 1", s["start"], dict(iters=s["iters"], max_evals=1)), ("max_evals 2", s["start"], dict(iters=s["iters"], max_evals=2)),
                          ("one below the need", s["start"], dict(iters=s["iters"], max_evals=need - 1)), ("huber", s["start"], dict(iters=4, huber=0.6))):
        d, r = _both(m, surface, cam, s["K"], **kw)
        _same_loop(d, r, name)
        if name.startswith("max_evals") or name.startswith("one below"):
            assert int(d["info"][0]) == lr.BUDGET and int(d["info"][2]) == kw["max_evals"]
        if name == "iters 0":
            assert int(d["info"][0]) == lr.ITERS and np.array_equal(d["pose"], s["start"].astype(np.float64))
    side = torch.cuda.Stream()                                 # a side stream: the same bits
    S, c = cu(surface), cu(s["start"])
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = m.localize(S, c, s["K"], iters=s["iters"])
    side.synchronize()
    for k in ("pose", "result", "history", "info"):
        assert np.array_equal(bits(r[k].cpu().numpy()), bits(dev[k])), k


def test_the_ends_that_give_no_pose():
    """FEW, collinear points, a flat surface (H = 0 and b = 0: the machine as written says SINGULAR, not CONVERGED -- the first
    pivot is not positive), a NaN surface and a camera that is not finite"""
    few, six, col = _ops_map(lr.loc_cloud(5, seed=5)), _ops_map(lr.loc_cloud(6, seed=6)), _ops_map(lr.collinear_case())
    d, r = _both(few, SURF, lr.CAM, lr.K)
    _same_loop(d, r, "five voxels")
    assert int(d["info"][0]) == lr.FEW and np.isnan(d["pose"]).all() and np.isnan(d["pose_f32"]).all() and d["status"][5] == 5
    d, r = _both(col, SURF, lr.CAM, lr.K)
    _same_loop(d, r, "six collinear voxels")
    assert d["status"][5] == 6 or np.isnan(d["pose"]).all()
    d, r = _both(six, np.ones((H, W), np.float32), lr.CAM, lr.K)
    _same_loop(d, r, "a surface of all ones")
    assert not d["gradient"].any() and int(d["info"][0]) == lr.SINGULAR and np.isnan(d["pose"]).all()
    d, r = _both(six, np.full((H, W), np.nan, np.float32), lr.CAM, lr.K)
    _same_loop(d, r, "a NaN surface")
    assert np.isnan(d["pose"]).all() and np.isnan(d["result"][0])
    bad = lr.CAM.copy()
    bad[5] = np.nan
    d, r = _both(six, SURF, bad, lr.K)
    _same_loop(d, r, "a camera that is not finite")
    assert int(d["info"][4]) & 1 and np.isnan(d["pose"]).all() and np.isnan(d["pose_f32"]).all()


# ------------------------------------------------------------------------------------------------ 3. the tracker
def _localize_ask(slam, f, frame):
    x, y, t, p = (v.clone() for v in kit.query_events(f))
    x[:400], y[:400], t[:400] = 100.0, 80.0, kit.tstamp(f)
    x[400:800], y[400:800], t[400:800] = 101.0, 80.0, kit.tstamp(f)
    x[800:1200], y[800:1200], t[800:1200] = 100.0, 81.0, kit.tstamp(f)
    slam.event_map(voxel=0.5, capacity=1 << 16)
    slam.event_map_insert(x, y, t, planes=24, range=(0.1, 1.5), min_votes=2.0, median_radius=1, min_support=2, as_tensor=True)
    res = {"tensor": kit.host({k: v for k, v in slam.event_map_localize(x, y, t, min_points=1, as_tensor=True).items() if v is not None})}
    res["resident_mid"] = kit.resident(slam)
    res["numpy"] = slam.event_map_localize(x, y, t, min_points=1, t_ref=kit.tstamp(f - 1), tau=0.25)
    return res


def _check_answer(a):
    tz, nb = a["tensor"], a["numpy"]
    assert tz["pose"].shape == (7,) and tz["pose_prior"].shape == (7,) and tz["info"][2] >= 1 and tz["surface_status"][0] == 0
    print("tracker localize: info %s status %s; numpy reason %s counts %s" % (tz["info"].tolist(), tz["status"].tolist(), nb["reason"], nb["counts"]))
    assert nb["reason"] in lr.REASONS.values() and nb["reason"] != "running" and nb["delta"].shape == (6,) and nb["hessian"].shape == (6, 6)
    assert nb["counts"]["n_occupied"] >= 1 and not nb["counts"]["bad_camera"] and nb["surface_counts"]["n_events"] == 5000
    assert np.isnan(nb["pose"]).all() == np.isnan(nb["delta"]).all()


def test_tracker_event_map_localize_device_resident():
    """event_map_localize on a device-resident tracker: it stays resident and tracks the bits of a run that is never asked"""
    a, ctl = kit.run_resident(True, _localize_ask), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_mid"] and a["resident_after"] and a["resident_at_end"]
    _check_answer(a)
    for f in (kit.T_QUERY + 1, kit.T_QUERY + 2):
        kit.same(a["state", f], ctl["state", f], "state %d" % f)


@torch.no_grad()
def test_tracker_event_map_localize_host_driven():
    """a host-driven tracker: event_map_localize equals ops.time_surface and PointMap.localize fed by hand with the tracker's own
    pose; a query before a map raises; the state is not written"""
    from rampvo_amd import ops
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    x, y, t, p = kit.query_events(f, 3000)
    x[:600], y[:600], t[:600] = cu(np.repeat(np.float32([100.0, 101.0, 100.0]), 200)), cu(np.repeat(np.float32([80.0, 80.0, 81.0]), 200)), kit.tstamp(f)
    with pytest.raises(RuntimeError, match="no event map yet"):
        slam.event_map_localize(x, y, t)
    slam.event_map_insert(x, y, t, planes=8, range=(0.1, 1.5), min_votes=1.5, median_radius=1, min_support=2)
    poses, patches = slam.poses_.clone(), slam.patches_.clone()
    out = slam.event_map_localize(x, y, t, min_points=1, iters=3)
    cam = slam.poses_at([kit.tstamp(f)], as_tensor=True)[0][0]
    ts = ops.time_surface(x, y, t, kit.tstamp(f), kit.tstamp(f) - kit.tstamp(f - 1), 240, 320, smooth=2)
    ref = kit.host(slam.event_map().localize(ts["surface"], cam, frame[2].cuda().float(), min_points=1, iters=3))
    assert np.array_equal(bits(out["pose"]), bits(ref["pose"])) and np.array_equal(bits(np.float64(out["cost"])), bits(ref["result"][0]))
    assert out["reason"] == lr.REASONS[int(ref["info"][0])] and np.array_equal(bits(out["pose_prior"]), bits(cam.cpu().numpy()))
    assert torch.equal(poses, slam.poses_) and torch.equal(patches, slam.patches_), "nothing of the tracker is written"
    given = slam.event_map_localize(x, y, t, min_points=1, iters=3, cam=cam, as_tensor=True)
    assert given["pose_status"] is None and np.array_equal(bits(given["pose"].cpu().numpy()), bits(ref["pose"]))
    with pytest.raises(RuntimeError, match="tau is finite and positive"):
        slam.event_map_localize(x, y, t, tau=0.0)
    del slam
    kit.quiesce()
