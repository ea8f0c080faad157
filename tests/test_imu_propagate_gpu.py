"""ramp_imu_propagate (csrc/imu_propagate.hip) against tests/propref.py, the float64 numpy restatement that shares none of the
kernel's structure (matrices for quaternions, ONE sequential loop for the three-level scan).

Bounds.  Every field (dt, q_wb, v, p_wb) of every row of ``state`` is held to
    max(4 env, 16 max(m, 1) 2^-53 max(1, max|field|))                                               (imuref.bound)
env = the float64 restatement's distance from the same restatement in numpy.longdouble, m = the number of elements of positive
length in front of the row -- the terms of its product; a row at or before the anchor has none and is held with m = 1, the
row's own output arithmetic (tests/test_imu_align_gpu.py treats its sums alike).  q_wb is compared up to its sign.  ``poses``:
every component within one fp32 ulp of float32 of the stated formula evaluated in float64 by the restatement (the float64
bound is far below half an ulp: the two roundings differ only by straddling a boundary); rotations up to the sign.
``times_out`` is max(tau, t0) bit for bit.  The widths of the scan are 64 (chunk), 4,096 (tile: 64 chunks) and a chain over the
tiles, hence the sizes.  Every case prints its largest measured / bound ratio before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import georef
import imuref as ir
import propref as pr
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
FIELDS = dict(dt=(0, 1), q=(1, 5), v=(5, 8), p=(8, 11))
SIZES = (1, 2, 63, 64, 65, 4095, 4096, 4097, 4099, 8193)      # around the chunk and the tile; 2 tiles + 1: the chain runs
N_BIG = max(SIZES)
_cache = {}


def host_array(v, n):
    if v is None:
        return None
    return (ctypes.c_double * n)(*[float(x) for x in np.asarray(v, np.float64).reshape(-1)])


def c_propagate(tau, gyro, accel, anchor, R_bc=None, p_bc=None, bias_a=None, max_gap=np.inf, horizon=np.inf, want_times=True,
                want_state=True, rc_only=False, over=None):
    """the C entry with guarded outputs -> dict on the host (``rc_only``: the return code, and whether every buffer is untouched)"""
    from rampvo_amd import _lib
    f64 = np.asarray(gyro).dtype == np.float64
    td, gd, ad, an = cu(np.asarray(tau, np.float64)), cu(np.asarray(gyro)), cu(np.asarray(accel)), cu(np.asarray(anchor, np.float64))
    N = len(td)
    shapes = dict(poses=((N, 7), torch.float32, 7), times=((N,), torch.float64, 1), state=((N, 16), torch.float64, 16),
                  status=((8,), torch.int32, 1))
    bufs = {k: Flat(s, d, rows=r) for k, (s, d, r) in shapes.items()}
    ext = None if R_bc is None and p_bc is None else host_array(np.concatenate([np.asarray(R_bc, np.float64).reshape(-1),
                                                                              np.asarray(p_bc, np.float64).reshape(-1)]), 12)
    nbytes = _lib.lib().ramp_imu_propagate_workspace_bytes(N)
    bufs["ws"] = Flat(max(nbytes, 16) // 8, torch.float64, rows=2)
    fresh = {k: b.snapshot() for k, b in bufs.items()}
    args = dict(tau=_lib.ptr(td), gyro=_lib.ptr(gd), accel=_lib.ptr(ad), N=N, anchor=_lib.ptr(an), ext=ext, ba=host_array(bias_a, 3),
                max_gap=float(max_gap), horizon=float(horizon), flags=_lib.RAMP_IMU_F64 if f64 else 0, poses=_lib.ptr(bufs["poses"].t),
                times=_lib.ptr(bufs["times"].t) if want_times else None, state=_lib.ptr(bufs["state"].t) if want_state else None,
                status=_lib.ptr(bufs["status"].t), ws=_lib.ptr(bufs["ws"].t), nbytes=nbytes)
    args.update(over or {})
    order = ("tau", "gyro", "accel", "N", "anchor", "ext", "ba", "max_gap", "horizon", "flags", "poses", "times", "state", "status",
             "ws", "nbytes")
    rc = _lib.lib().ramp_imu_propagate(*[args[k] for k in order], _lib.stream())
    torch.cuda.synchronize()
    whole = lambda k: bufs[k].unchanged(fresh[k])
    if rc_only:
        return rc, all(whole(k) for k in shapes)
    assert rc == 0
    out = {k: bufs[k].t.cpu().numpy() for k in shapes}
    for k, b in bufs.items():
        assert b.intact(), k
    if not want_times:
        assert whole("times")
    if not want_state:
        assert whole("state")
    return out


def check_rows(got, ref64, refld, label):
    """every row and field of ``state`` by the rule above, ``poses`` to one fp32 ulp, ``times`` bit for bit -> the ratios"""
    n = len(got["state"])
    st, r64, rld, m = got["state"], ref64["state"][:n], refld["state"][:n].astype(np.float64), np.maximum(ref64["m"][:n], 1)
    dead = np.isnan(r64[:, 0])
    assert np.array_equal(np.isnan(st).all(axis=1), dead) and np.array_equal(np.isnan(st).any(axis=1), dead), label
    assert (st[~dead, 11:] == 0).all(), label
    worst = {}
    live = ~dead
    for name, (lo, hi) in FIELDS.items():
        g, r, l = st[live, lo:hi], r64[live, lo:hi], rld[live, lo:hi]
        err = np.abs(g - r)
        if name == "q":
            err = np.minimum(err, np.abs(g + r))
        env = np.abs(r - l).max(axis=1)
        bnd = np.maximum(4 * env, 16 * m[live] * EPS * np.maximum(1.0, np.abs(r).max(axis=1)))
        worst[name] = float((err.max(axis=1) / bnd).max()) if live.any() else 0.0
    want = ref64["poses"][:n]                                               # float32 of the formula in float64
    ulp = np.spacing(np.abs(want[live]))
    err = np.abs(got["poses"][live] - want[live])
    err[:, 3:] = np.minimum(err[:, 3:], np.abs(got["poses"][live] + want[live])[:, 3:])
    worst["poses_ulp"] = float((err / ulp).max()) if live.any() else 0.0
    assert np.isnan(got["poses"][dead]).all(), label
    print(label, "measured / bound per field:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (label, worst)
    assert georef.same_bits(got["times"], ref64["times"][:n]), label
    return worst


# ------------------------------------------------------------------------------------------------ 1. rows at every width
def size_case(held, dtype):
    """N_BIG jittered samples with ``held`` of them strictly before the anchor (0: the first sample lies exactly on t0), a
    duplicated tau behind the anchor; the two restatements, computed once"""
    key = ("size", held, np.dtype(dtype).name)
    if key not in _cache:
        rng = np.random.default_rng(100 + held)
        tau = np.cumsum(rng.uniform(0.003, 0.007, N_BIG)) + 2.0
        tau[held + 21] = tau[held + 20]                                     # a sub-interval of length 0
        gyro = (rng.normal(size=(N_BIG, 3)) * 0.8).astype(dtype)
        accel = (rng.normal(size=(N_BIG, 3)) * 3 + [0, 0, 9.8]).astype(dtype)
        t0 = tau[0] if held == 0 else 0.25 * tau[held - 1] + 0.75 * tau[held]
        q = rng.normal(size=4)
        anchor = pr.make_anchor(t0, rng.normal(size=3), q / np.linalg.norm(q) * 1.0001, rng.normal(size=3), 2.5, ir.G_TRUE,
                                [0.02, -0.01, 0.03])
        kw = dict(tau=tau, gyro=gyro, accel=accel, anchor=anchor, R_bc=ir.R_BC, p_bc=ir.P_BC, bias_a=[0.1, -0.2, 0.05])
        _cache[key] = (kw, pr.propagate(**kw), pr.propagate(**kw, ft=np.longdouble))
    return _cache[key]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("held", [0, 1, 70])
def test_rows_at_every_width(held, dtype):
    kw, r64, rld = size_case(held, dtype)
    cut = lambda n: {k: (v[:n] if k in ("tau", "gyro", "accel") else v) for k, v in kw.items()}
    big = c_propagate(**cut(N_BIG))
    n_held = max(held, 1)
    assert list(big["status"]) == [0, N_BIG, n_held, N_BIG - n_held, 0, 0, 0, 0]
    worst = {}
    for n in SIZES:
        got = big if n == N_BIG else c_propagate(**cut(n))
        h = min(n, n_held)                                                  # n <= held: t0 >= tau[-1], every row is held
        assert list(got["status"]) == [0, n, h, n - h, 0, 0, 0, 0], n
        w = check_rows(got, r64, rld, "held %d %s N %d" % (held, np.dtype(dtype).name, n))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        # the order of the tree: the first n rows of the larger call are this call's, bit for bit
        for k in ("state", "poses", "times"):
            assert georef.same_bits(got[k], big[k][:n]), (k, n)
    print("held %d %s, largest measured / bound:" % (held, np.dtype(dtype).name), {k: round(v, 4) for k, v in worst.items()})
    again = c_propagate(**cut(N_BIG))
    assert all(georef.same_bits(big[k], again[k]) for k in big)             # a call repeats its bits


def test_side_stream_and_the_wrapper():
    from rampvo_amd import ops
    kw, _, _ = size_case(70, np.float32)
    want = c_propagate(**kw)
    dev = {k: cu(kw[k]) for k in ("tau", "gyro", "accel", "anchor")}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = ops.imu_propagate(dev["tau"], dev["gyro"], dev["accel"], dev["anchor"], R_bc=ir.R_BC, p_bc=ir.P_BC,
                                bias_a=kw["bias_a"], want_state=True)
        lean = ops.imu_propagate(dev["tau"], dev["gyro"], dev["accel"], dev["anchor"], R_bc=ir.R_BC, p_bc=ir.P_BC, bias_a=kw["bias_a"])
        with pytest.raises(RuntimeError, match="host value"):
            ops.imu_propagate(dev["tau"], dev["gyro"], dev["accel"], dev["anchor"], R_bc=cu(ir.R_BC))
    side.synchronize()
    for k in want:
        assert georef.same_bits(out[k].cpu().numpy(), want[k]), k
    assert "state" not in lean and georef.same_bits(lean["poses"].cpu().numpy(), want["poses"])
    assert ops.imu_propagate_status(out["status"]) == dict(bad_order=False, bad_anchor=False, no_start=False, n_samples=N_BIG,
                                                           n_held=70, n_propagated=N_BIG - 70, n_cut_off=0, n_beyond_horizon=0)
    with pytest.raises(RuntimeError, match="24 float64 words"):
        ops.imu_propagate(dev["tau"], dev["gyro"], dev["accel"], dev["anchor"][:20])


# ------------------------------------------------------------------------------------------------ 2. the large case
def test_2_to_the_20_samples_against_the_one_interval_walk():
    """no sequential reference at this size: the last row's (dt, dR, dv, dp), recovered from ``state`` and the anchor, against
    ramp_imu_preintegrate of the single interval [t0, tau[-1]] -- the one-wave walk, tested on its own -- within the two
    kernels' bounds summed: 2 x 16 N 2^-53 max(1, max|field|)"""
    from rampvo_amd import ops
    rng = np.random.default_rng(31)
    N = 2 ** 20 + 1
    tau = np.arange(N) / 1000.0
    t = tau[:, None]
    gyro = (0.4 * np.sin(t * [0.7, 1.1, 0.5]) + 0.01 * rng.normal(size=(N, 3))).astype(np.float32)
    accel = (np.array([0.0, 0.0, 9.8]) + np.sin(t * [1.3, 0.9, 0.4]) + 0.05 * rng.normal(size=(N, 3))).astype(np.float32)
    t0 = 0.5 * (tau[0] + tau[1])
    bias = [0.02, -0.01, 0.03]
    anchor = pr.make_anchor(t0, [0.5, -1.0, 2.0], ir.quat_from_R(ir.so3_exp(np.array([0.3, -0.4, 0.2]))), [0.4, 0.1, -0.3], 2.0,
                            ir.G_TRUE, bias)
    td, gd, ad, an = cu(tau), cu(gyro), cu(accel), cu(anchor)
    out = ops.imu_propagate(td, gd, ad, an, want_state=True)
    small = ops.imu_propagate(td[:8193], gd[:8193], ad[:8193], an, want_state=True)
    pre, pst = ops.imu_preintegrate(td, gd, ad, cu(np.array([t0, tau[-1]])), bias_g=bias)
    assert ops.imu_propagate_status(out["status"])["n_propagated"] == N - 1
    for k in ("state", "poses", "times"):                                   # the first 8,193 rows: the N = 8,193 call's bits
        a, b = out[k][:8193].contiguous(), small[k].contiguous()
        assert torch.equal(a.view(torch.int64 if a.dtype == torch.float64 else torch.int32),
                           b.view(torch.int64 if b.dtype == torch.float64 else torch.int32)), k
    st, rec = out["state"][-1].cpu().numpy(), pre[0].cpu().numpy()
    assert rec[1] == N - 1 and np.isfinite(st).all()
    R0 = ir.R_from_quat(anchor[4:8] / np.linalg.norm(anchor[4:8]))
    p0, v0, g, dt = anchor[11] * anchor[1:4], anchor[8:11], anchor[12:15], st[0]
    got = dict(dt=np.array([dt]), q=ir.quat_from_R(R0.T @ ir.R_from_quat(st[1:5])), dv=R0.T @ (st[5:8] - v0 - g * dt),
               dp=R0.T @ (st[8:11] - p0 - v0 * dt - 0.5 * g * dt * dt))
    ref = dict(dt=rec[0:1], q=rec[2:6], dv=rec[6:9], dp=rec[9:12])
    # recovering dv and dp subtracts v0 + g dt and p0 + v0 dt + 1/2 g dt^2 from the row: the bound is on the ROW's own field
    field = dict(dt=ref["dt"], q=ref["q"], dv=st[5:8], dp=st[8:11])
    worst = {k: float(np.abs(got[k] - ref[k]).max() / (2 * ir.bound(0.0, N, field[k]))) for k in got}
    print("2^20 + 1 samples, last row measured / bound:", {k: round(v, 5) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), worst


# ------------------------------------------------------------------------------------------------ 3. status words and bits
@pytest.mark.parametrize("name", sorted(pr.cases()))
def test_failure_cases(name):
    kw, want, nan_rows = pr.cases()[name]
    out = c_propagate(**kw)
    st, N = out["status"], len(kw["tau"])
    assert [int(st[i]) for i in (0, 2, 3, 4, 5)] == want and st[1] == N and st[6] == 0 and st[7] == 0
    expect = np.zeros(N, bool)
    expect[nan_rows] = True
    for k in ("state", "poses"):
        assert np.array_equal(np.isnan(out[k]).all(axis=1), expect) and np.array_equal(np.isnan(out[k]).any(axis=1), expect), k
    if st[0]:
        assert np.isnan(out["times"]).all()
    else:
        assert st[2] + st[3] + st[4] + st[5] == st[1]
        check_rows(out, pr.propagate(**kw), pr.propagate(**kw, ft=np.longdouble), name)
    lean = c_propagate(**kw, want_times=False, want_state=False)            # NULL times_out and state
    assert georef.same_bits(lean["poses"], out["poses"]) and np.array_equal(lean["status"], st)


def test_refusals_touch_nothing():
    kw = pr.cases()["clean"][0]
    EINVAL, EWORKSPACE = -1, -3
    for over in (dict(N=0), dict(flags=2), dict(max_gap=0.0), dict(max_gap=float("nan")), dict(horizon=0.0), dict(horizon=float("nan")),
                 dict(horizon=-1.0), dict(tau=None), dict(gyro=None), dict(anchor=None), dict(poses=None), dict(status=None),
                 dict(ws=None), dict(ba=host_array([np.inf, 0, 0], 3)), dict(ext=host_array([np.inf] * 12, 12)),
                 dict(ext=host_array(np.concatenate([1.001 * ir.R_BC.reshape(-1), ir.P_BC]), 12)),
                 dict(ext=host_array(np.concatenate([(ir.R_BC * [1, 1, -1]).reshape(-1), ir.P_BC]), 12))):
        assert c_propagate(**kw, rc_only=True, over=over) == (EINVAL, True), over
    assert c_propagate(**kw, rc_only=True, over=dict(nbytes=64)) == (EWORKSPACE, True)


# ------------------------------------------------------------------------------------------------ 4. the chain
def _pose_error(row, t):
    """(translation distance in the tracker's unit, rotation angle) of a camera-to-world row from the scene's true pose at t"""
    true = ir.knots_at([t])[0].astype(np.float64)
    dR = ir.R_from_quat(true[3:] / np.linalg.norm(true[3:])).T @ ir.R_from_quat(row[3:].astype(np.float64) / np.linalg.norm(row[3:]))
    return float(np.linalg.norm(row[:3] - true[:3])), float(np.linalg.norm(ir.so3_log(dR)))


def test_alignment_anchor_propagation_on_the_scene():
    """align the scene's first 100 frames, anchor on the 100th, propagate through the samples behind it: the pose predicted at
    the 110th frame's time is closer to the truth than the held end pose and than the last segment's screw motion continued"""
    from rampvo_amd import ops
    s = ir.scene()
    knots, times = cu(s["knots"][:100]), cu(s["times"][:100])
    tau, gyro, accel = cu(s["tau"]), cu(s["gyro"]), cu(s["accel"])
    al = ops.imu_align(tau, gyro, accel, knots, times, R_bc=ir.R_BC, p_bc=ir.P_BC, gravity_norm=9.80665)
    anchor = ops.imu_anchor(al, knots, times)
    a = anchor.cpu().numpy()
    assert a.shape == (24,) and a[0] == s["times"][99] and (a[18:] == 0).all()
    assert georef.same_bits(a[1:8], s["knots"][99].astype(np.float64)) and georef.same_bits(a[8:11], al["velocity"][99].cpu().numpy())
    assert georef.same_bits(a[11:18], al["result"][:7].cpu().numpy())
    out = ops.imu_propagate(tau, gyro, accel, anchor, R_bc=ir.R_BC, p_bc=ir.P_BC, horizon=1.0)
    st = ops.imu_propagate_status(out["status"])
    assert not (st["bad_order"] or st["bad_anchor"] or st["no_start"]) and st["n_cut_off"] == 0 and st["n_beyond_horizon"] > 0
    tq = float(s["times"][109])
    q = cu(np.array([tq]))
    pred, _, pst = ops.se3_interp(out["poses"][:1200], out["times"][:1200], q)          # (rows within the horizon)
    held, _, _ = ops.se3_interp(knots, times, q)
    extra, _, _ = ops.se3_interp(knots, times, q, extrapolate=True)
    assert int(pst[0]) == 0
    e_imu, e_held, e_extra = (_pose_error(x.cpu().numpy()[0], tq) for x in (pred, held, extra))
    print("pose error 0.5 s ahead (translation, rotation): imu", e_imu, "held", e_held, "extrapolated", e_extra)
    assert e_imu[0] < e_held[0] and e_imu[0] < e_extra[0] and e_imu[1] < e_held[1] and e_imu[1] < e_extra[1]
    # poses, times are knots for the event warp
    n = 256
    rng = np.random.default_rng(3)
    ev_t = cu(np.sort(rng.uniform(s["times"][99], tq, n)))
    xs, ys = cu(rng.uniform(0, 63, n).astype(np.float32)), cu(rng.uniform(0, 47, n).astype(np.float32))
    warp = ops.event_warp(xs, ys, ev_t, cu(np.ones(n, np.int8)), out["poses"][:1200], out["times"][:1200], tq,
                          cu(np.array([60.0, 60.0, 32.0, 24.0], np.float32)), 0.5, 48, 64)
    assert int(warp["status"][0]) & 1 == 0


# ------------------------------------------------------------------------------------------------ 5. tracker
def _tracker_query(slam, f):
    from rampvo_amd import ops
    tau, gyro, accel = kit.imu_samples(f)
    with pytest.raises(RuntimeError, match="set_imu"):
        slam.propagate_imu(tau, gyro, accel)
    slam.set_imu(R_bc=ir.R_BC, p_bc=ir.P_BC, bias_g=[0.01, 0.0, -0.01], bias_a=[0.1, 0.0, 0.0])
    got = kit.host(slam.propagate_imu(cu(tau), cu(gyro), cu(accel), as_tensor=True, want_state=True))
    knots, tst = slam.trajectory(as_tensor=True)
    tdev = cu(np.asarray(tst, np.float64))
    al = ops.imu_align(cu(tau), cu(gyro), cu(accel), knots, tdev, R_bc=ir.R_BC, p_bc=ir.P_BC, bias_g=[0.01, 0.0, -0.01],
                       bias_a=[0.1, 0.0, 0.0], gravity_norm=9.80665)
    want = ops.imu_propagate(cu(tau), cu(gyro), cu(accel), ops.imu_anchor(al, knots, tdev), R_bc=ir.R_BC, p_bc=ir.P_BC,
                             bias_a=[0.1, 0.0, 0.0], want_state=True)
    want["align"] = al
    kit.same(got, kit.host(want), "propagate_imu")
    n_held = int((tau <= tst[-1]).sum())
    assert got["status"][1] == len(tau) and (got["status"][0] != 0 or got["status"][2] == n_held)
    # align= reuse: the device dict of align_imu(as_tensor=True)
    reuse = slam.propagate_imu(cu(tau), cu(gyro), cu(accel), align=slam.align_imu(cu(tau), cu(gyro), cu(accel), as_tensor=True),
                               as_tensor=True, want_state=True)
    for k in ("poses", "times", "state", "status"):
        assert georef.same_bits(reuse[k].cpu().numpy(), got[k]), k
    with pytest.raises(RuntimeError, match="align="):
        slam.propagate_imu(tau, gyro, accel, align=slam.align_imu(cu(tau), cu(gyro), cu(accel), stride=2, as_tensor=True))
    if got["status"][0] or got["align"]["status"][0]:
        with pytest.raises(RuntimeError, match="propagate_imu"):
            slam.propagate_imu(tau, gyro, accel)
    else:
        host = slam.propagate_imu(tau, gyro, accel, want_state=True)
        assert georef.same_bits(host["poses"], got["poses"]) and georef.same_bits(host["align"]["velocity"], got["align"]["velocity"])


@torch.no_grad()
def test_tracker_device_resident():
    slam = kit.tracker(True, True)
    for f, frame in enumerate(kit.frames()[:kit.T_QUERY + 2]):
        kit.feed(slam, f, frame)
        if f == kit.T_QUERY:
            assert kit.resident(slam)
            _tracker_query(slam, f)
            assert kit.resident(slam)                                      # the device-resident tracker is still resident
    assert kit.resident(slam)
    del slam
    kit.quiesce()


@torch.no_grad()
def test_tracker_host_driven():
    slam = kit.tracker(False, False)
    frames = kit.frames()
    for f, frame in enumerate(frames):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    _tracker_query(slam, f)
    kit.feed(slam, f + 1, frames[f + 1])
    assert slam._dev is None
    del slam
    kit.quiesce()
