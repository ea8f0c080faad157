"""ramp_imu_preintegrate / ramp_imu_align (csrc/imu.hip) against tests/imuref.py, the float64 numpy restatement that shares
none of the kernel's structure (matrices for quaternions, a sequential composition for the shuffle tree, searchsorted,
numpy.linalg.solve).

Bounds.  A field of a record, a word of ``normal``, a velocity or a residual is held to
    max(4 env, 16 m 2^-53 max(1, max|field|))                                                       (imuref.bound)
env = the float64 restatement's own distance from the same restatement in numpy.longdouble, m = the record's sub-interval
count (the number of terms of a sum): the worst-case linear growth of a few roundings per composition.  ``bias_g1``, ``s``
and ``g`` are held to numpy.linalg.solve on the CALL'S OWN ``normal`` words within 64 cond 2^-53 relative, the textbook bound
of a backward-stable Cholesky solve, cond = numpy.linalg.cond of those words; the same bound with a gravity norm, where the
reference is the restatement's four refinements on those words.  A velocity is held by the per-record rule with the m of the
record it is formed from and its own three components as the field, a residual with the larger m of its triple's two records,
the rms with m = the number of triples; env is the distance of the float64 restatement of these from the longdouble one, both
fed the call's own x and bias.  Every case prints its largest measured / bound ratio before it asserts."""
import ctypes

import numpy as np
import pytest
import torch

import georef
import imuref as ir
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
FIELDS = dict(dt=(0, 1), m=(1, 2), q=(2, 6), dv=(6, 9), dp=(9, 12), J=(12, 21), pad=(21, 24))
_cache = {}


def host_triple(v, n=3):
    if v is None:
        return None
    return (ctypes.c_double * n)(*[float(x) for x in np.asarray(v, np.float64).reshape(-1)])


def c_preintegrate(tau, gyro, accel, times, bias_g=None, bias_a=None, stride=1, max_gap=np.inf, rc_only=False, over=None):
    """the C entry with guarded outputs -> (preint, status) on the host"""
    from rampvo_amd import _lib
    f64 = np.asarray(gyro).dtype == np.float64
    td, gd, ad, tt = cu(np.asarray(tau, np.float64)), cu(np.asarray(gyro)), cu(np.asarray(accel)), cu(np.asarray(times, np.float64))
    T = len(tt)
    K = (T - 1) // stride + 1
    pre, st = Flat((max(K - 1, 1), 24), torch.float64, rows=24), Flat(8, torch.int32)
    bg, ba = host_triple(bias_g), host_triple(bias_a)
    args = dict(tau=_lib.ptr(td), gyro=_lib.ptr(gd), accel=_lib.ptr(ad), N=len(td), times=_lib.ptr(tt), T=T, stride=stride, bg=bg,
                ba=ba, max_gap=float(max_gap), flags=_lib.RAMP_IMU_F64 if f64 else 0, preint=_lib.ptr(pre.t), status=_lib.ptr(st.t))
    args.update(over or {})
    rc = _lib.lib().ramp_imu_preintegrate(*[args[k] for k in ("tau", "gyro", "accel", "N", "times", "T", "stride", "bg", "ba",
                                                              "max_gap", "flags", "preint", "status")], _lib.stream())
    if rc_only:
        return rc
    assert rc == 0
    out = pre.t.cpu().numpy(), st.t.cpu().numpy()
    assert pre.intact() and st.intact()
    return out


def c_align(tau, gyro, accel, knots, times, R_bc=None, p_bc=None, bias_g=None, bias_a=None, stride=1, max_gap=np.inf,
            gravity_norm=0.0, gyro_steps=1, rc_only=False, over=None):
    """the C entry with every output requested and guarded -> dict on the host"""
    from rampvo_amd import _lib
    f64 = np.asarray(gyro).dtype == np.float64
    td, gd, ad = cu(np.asarray(tau, np.float64)), cu(np.asarray(gyro)), cu(np.asarray(accel))
    kd, tt = cu(np.asarray(knots, np.float32)), cu(np.asarray(times, np.float64))
    T = len(tt)
    K = (T - 1) // stride + 1
    shapes = dict(result=((16,), 1), normal=((32,), 1), velocity=((K, 3), 3), residual=((max(K - 2, 0),), 1), preint=((K - 1, 24), 24))
    bufs = {k: Flat(s, torch.float64, rows=r) for k, (s, r) in shapes.items()}
    bufs["status"] = Flat(8, torch.int32)
    at = {k: ctypes.c_void_p(b.address()) for k, b in bufs.items()}
    ext = None if R_bc is None and p_bc is None else host_triple(np.concatenate([np.asarray(R_bc, np.float64).reshape(-1),
                                                                                np.asarray(p_bc, np.float64).reshape(-1)]), 12)
    nbytes = _lib.lib().ramp_imu_workspace_bytes(len(td), K)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    bg, ba = host_triple(bias_g), host_triple(bias_a)
    args = dict(tau=_lib.ptr(td), gyro=_lib.ptr(gd), accel=_lib.ptr(ad), N=len(td), knots=_lib.ptr(kd), times=_lib.ptr(tt), T=T,
                stride=stride, ext=ext, bg=bg, ba=ba, max_gap=float(max_gap), G=float(gravity_norm), steps=gyro_steps,
                flags=_lib.RAMP_IMU_F64 if f64 else 0, result=at["result"], normal=at["normal"], velocity=at["velocity"],
                residual=at["residual"] if K > 2 else None, preint=at["preint"], status=at["status"], ws=_lib.ptr(ws), nbytes=nbytes)
    args.update(over or {})
    order = ("tau", "gyro", "accel", "N", "knots", "times", "T", "stride", "ext", "bg", "ba", "max_gap", "G", "steps", "flags",
             "result", "normal", "velocity", "residual", "preint", "status", "ws", "nbytes")
    rc = _lib.lib().ramp_imu_align(*[args[k] for k in order], _lib.stream())
    if rc_only:
        return rc
    assert rc == 0
    out = {k: b.t.cpu().numpy() for k, b in bufs.items()}
    for k, b in bufs.items():
        assert b.intact(), k
    return out


def check_records(got, ref64, refld, label):
    """per record and field: |got - ref64| <= bound(env, m, field); NaN records NaN everywhere; -> the largest ratio per field"""
    worst = {}
    assert got.shape == ref64.shape
    for k in range(len(got)):
        if not np.isfinite(ref64[k, 0]):
            assert np.isnan(got[k]).all(), (label, k)
            continue
        m = ref64[k, 1]
        assert got[k, 1] == m and (got[k, 21:] == 0).all(), (label, k)
        for name, (lo, hi) in FIELDS.items():
            if name in ("m", "pad"):
                continue
            env = np.abs(ref64[k, lo:hi] - refld[k, lo:hi].astype(np.float64)).max()
            ratio = np.abs(got[k, lo:hi] - ref64[k, lo:hi]).max() / ir.bound(env, m, ref64[k, lo:hi])
            worst[name] = max(worst.get(name, 0.0), float(ratio))
    print(label, "measured / bound per field:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (label, worst)
    return worst


# ------------------------------------------------------------------------------------------------ 1. records
COUNTS = (1, 2, 63, 64, 65, 128, 129, 4099)


def count_case():
    """samples with jitter and intervals whose sub-interval counts are COUNTS, then one that ends on a sample and one with a
    sample on each end and a duplicated tau inside"""
    if "count" not in _cache:
        rng = np.random.default_rng(17)
        N = 4800
        tau = np.cumsum(rng.uniform(0.003, 0.007, N)) + 2.0
        gyro, accel = rng.normal(size=(N, 3)) * 1.5, rng.normal(size=(N, 3)) * 4 + [0, 0, 9.8]
        i, times = 5, []
        mid = lambda i: 0.5 * (tau[i] + tau[i + 1])
        times.append(mid(i))
        for m in COUNTS:
            i += m - 1 if m > 1 else 0
            times.append(mid(i) if m > 1 else 0.25 * tau[i] + 0.75 * tau[i + 1])
        times += [tau[4700], tau[4712]]
        tau, gyro, accel = np.insert(tau, 4705, tau[4705]), np.insert(gyro, 4705, gyro[4705], 0), np.insert(accel, 4705, accel[4705], 0)
        times = np.array(times)
        bg, ba = np.array([0.02, -0.01, 0.03]), np.array([0.1, -0.2, 0.05])
        refs = {}
        for dt in (np.float32, np.float64):
            g, a = gyro.astype(dt), accel.astype(dt)
            refs[dt] = (g, a, ir.preintegrate(tau, g, a, times, bg, ba)[0], ir.preintegrate(tau, g, a, times, bg, ba, ft=np.longdouble)[0])
        _cache["count"] = dict(tau=tau, times=times, bg=bg, ba=ba, refs=refs)
    return _cache["count"]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_records_at_every_chunk_shape(dtype):
    c = count_case()
    g, a, r64, rld = c["refs"][dtype]
    assert list(r64[:, 1]) == list(COUNTS) + [152, 13]                     # ... one that ends on a sample, one with a duplicate
    pre, st = c_preintegrate(c["tau"], g, a, c["times"], c["bg"], c["ba"])
    assert list(st) == [0, len(c["tau"]), 10, 0, 0, 0, 0, 0]
    check_records(pre, r64, rld, "counts %s" % np.dtype(dtype).name)
    again, _ = c_preintegrate(c["tau"], g, a, c["times"], c["bg"], c["ba"])
    assert georef.same_bits(pre, again)                                     # a call repeats its bits


@pytest.mark.parametrize("stride", [1, 2, 7])
def test_a_record_depends_on_its_own_interval_alone(stride):
    """each record of a strided call over the scene has the bits of the single-interval call over the same two time stamps"""
    s = ir.scene()
    times = s["times"][:43]
    pre, st = c_preintegrate(s["tau"], s["gyro"], s["accel"], times, ir.BIAS_TRUE, None, stride=stride)
    K = (len(times) - 1) // stride + 1
    assert pre.shape == (K - 1, 24) and st[2] == K - 1 and st[3] == 0
    for k in range(K - 1):
        one, _ = c_preintegrate(s["tau"], s["gyro"], s["accel"], times[[k * stride, (k + 1) * stride]], ir.BIAS_TRUE, None)
        assert georef.same_bits(one[0], pre[k]), (stride, k)
    ref = ir.preintegrate(s["tau"], s["gyro"], s["accel"], times, ir.BIAS_TRUE, None, stride=stride)[0]
    rld = ir.preintegrate(s["tau"], s["gyro"], s["accel"], times, ir.BIAS_TRUE, None, stride=stride, ft=np.longdouble)[0]
    check_records(pre, ref, rld, "stride %d" % stride)


def test_one_interval_over_65537_samples():
    rng = np.random.default_rng(23)
    N = 2 ** 16 + 3
    tau = np.arange(N) / 1000.0
    t = tau[:, None]
    gyro = (0.4 * np.sin(t * [0.7, 1.1, 0.5]) + 0.01 * rng.normal(size=(N, 3))).astype(np.float32)
    accel = (np.array([0.0, 0.0, 9.8]) + np.sin(t * [1.3, 0.9, 0.4]) + 0.05 * rng.normal(size=(N, 3))).astype(np.float32)
    times = np.array([0.5 * (tau[0] + tau[1]), 0.5 * (tau[N - 2] + tau[N - 1])])
    ref = ir.preintegrate(tau, gyro, accel, times)[0]
    rld = ir.preintegrate(tau, gyro, accel, times, ft=np.longdouble)[0]
    assert ref[0, 1] == 2 ** 16 + 2                                         # 2^16 + 1 samples inside
    pre, st = c_preintegrate(tau, gyro, accel, times)
    assert list(st) == [0, N, 1, 0, 0, 0, 0, 0]
    check_records(pre, ref, rld, "65537 samples")


# ------------------------------------------------------------------------------------------------ 2. alignment
def scene_run(key, **kw):
    if key not in _cache:
        args = {**ir.scene(), **ir.EXTR, **kw}
        _cache[key] = (args, c_align(**args))
    return _cache[key]


def check_sums(got, ref, status, label):
    worst = {}
    for name, (lo, hi, m) in dict(N=(0, 16, 3 * status[6]), y=(16, 20, 3 * status[6]), H=(20, 29, 3 * status[5]),
                                  b=(29, 32, 3 * status[5])).items():
        worst[name] = float(max(abs(g - r) / ir.bound(0.0, max(m, 1), [r]) for g, r in zip(got[lo:hi], ref[lo:hi])))     # per word
    print(label, "normal, measured / bound:", {k: round(v, 4) for k, v in worst.items()})
    assert all(v <= 1.0 for v in worst.values()), (label, worst)


def check_solves(out, gravity_norm, label):
    """bias step, s and g against numpy.linalg.solve on the call's own normal words"""
    nw, r = out["normal"], out["result"]
    N, y, H, b = nw[:16].reshape(4, 4), nw[16:20], nw[20:29].reshape(3, 3), nw[29:32]
    x = ir.solve_scale(N, y, gravity_norm)
    tol = 64 * np.linalg.cond(N) * EPS
    ratio = np.abs(r[:4] - x).max() / (tol * np.abs(x).max())
    print(label, "s, g measured / bound:", round(float(ratio), 4), "cond", np.linalg.cond(N), "pivot ratio", r[8])
    assert ratio <= 1.0
    L = np.linalg.cholesky(N)
    assert abs(r[8] / ((np.diag(L) ** 2).max() / (np.diag(L) ** 2).min()) - 1) < 1e-12
    return np.linalg.solve(H, b), 64 * np.linalg.cond(H) * EPS


@pytest.mark.parametrize("gravity_norm", [0.0, 9.80665])
def test_scene(gravity_norm):
    args, out = scene_run("scene%g" % gravity_norm, gravity_norm=gravity_norm)
    st = out["status"]
    assert list(st) == [0, 2400, 219, 0, 0, 219, 218, 0]
    # recovery, the figures of the CPU test
    assert np.abs(out["result"][4:7] - ir.BIAS_TRUE).max() < 1e-6
    assert abs(out["result"][0] / ir.SCALE_TRUE - 1) < 0.01 and np.abs(out["result"][1:4] - ir.G_TRUE).max() < 0.005
    if gravity_norm:
        assert abs(np.linalg.norm(out["result"][1:4]) - gravity_norm) < 8 * EPS * gravity_norm
    assert (out["result"][9:] == 0).all()
    # the gyro step against the solve on its own words; the first integration is the restatement's with the start bias
    delta, tol = check_solves(out, gravity_norm, "scene G=%g" % gravity_norm)
    assert np.abs(out["result"][4:7] - delta).max() <= tol * np.abs(delta).max()
    # the second integration against the restatement fed the device's own bias
    own = dict(args, bias_g1=out["result"][4:7])
    ref = ir.align(**own)
    rld = ir.preintegrate(args["tau"], args["gyro"], args["accel"], args["times"], out["result"][4:7], None, ft=np.longdouble)[0]
    check_records(out["preint"], ref["preint"], rld, "second integration")
    check_sums(out["normal"], ref["normal"], st, "scene")
    # velocity, residual and rms by the per-record rule: the record's own m, the field itself, env from the longdouble restatement
    x, used, ld = out["result"][:4], list(range(218)), np.longdouble
    vel, res, rms = ir.velocities(ref["preint"], *ir._bodies(args["knots"], 1, ir.R_BC, ir.P_BC, np.float64), x, used)
    vld, rsld, rmsld = ir.velocities(rld, *ir._bodies(args["knots"], 1, ir.R_BC, ir.P_BC, ld), x.astype(ld), used)
    m = ref["preint"][:, 1]
    rv = max(np.abs(out["velocity"][k] - vel[k]).max() / ir.bound(np.abs(vel[k] - vld[k].astype(np.float64)).max(), m[min(k, 218)], vel[k])
             for k in range(220))
    rr = max(abs(out["residual"][j] - res[j]) / ir.bound(abs(res[j] - float(rsld[j])), max(m[j], m[j + 1]), [res[j]]) for j in used)
    rm = abs(out["result"][7] - rms) / ir.bound(abs(rms - float(rmsld)), 218, [rms])
    print("velocity, residual, rms measured / bound:", round(float(rv), 4), round(float(rr), 4), round(float(rm), 4))
    assert rv <= 1.0 and rr <= 1.0 and rm <= 1.0
    again = c_align(**args)
    assert all(georef.same_bits(out[k], again[k]) for k in out)             # a call repeats its bits


def test_irregular_frames_float32_samples_and_strides():
    """intervals of two lengths, fp32 samples, two gyro steps; then the scene at stride 2 and 7"""
    s = ir.scene()
    args = {**s, **ir.EXTR, "knots": s["knots"][ir.IRREGULAR], "times": s["times"][ir.IRREGULAR],
            "gyro": s["gyro"].astype(np.float32), "accel": s["accel"].astype(np.float32), "gyro_steps": 2}
    out = c_align(**args)
    assert list(out["status"]) == [0, 2400, 39, 0, 0, 39, 38, 0]
    ref = ir.align(**args, bias_g1=out["result"][4:7])
    rld = ir.preintegrate(args["tau"], args["gyro"], args["accel"], args["times"], out["result"][4:7], None, ft=np.longdouble)[0]
    check_records(out["preint"], ref["preint"], rld, "irregular")
    check_sums(out["normal"], ref["normal"], out["status"], "irregular")
    check_solves(out, 0.0, "irregular")
    assert np.abs(out["result"][4:7] - ir.BIAS_TRUE).max() < 1e-5 and abs(out["result"][0] / ir.SCALE_TRUE - 1) < 0.02
    for stride in (2, 7):
        args = {**s, **ir.EXTR, "stride": stride}
        out = c_align(**args)
        K = 219 // stride + 1
        assert list(out["status"]) == [0, 2400, K - 1, 0, 0, K - 1, K - 2, 0]
        ref = ir.align(**args, bias_g1=out["result"][4:7])
        check_sums(out["normal"], ref["normal"], out["status"], "stride %d" % stride)
        check_solves(out, 0.0, "stride %d" % stride)
        assert out["velocity"].shape == (K, 3) and np.isfinite(out["velocity"]).all()


@pytest.mark.parametrize("name", sorted(ir.cases()))
def test_failure_cases(name):
    kw, want = ir.cases()[name]
    out = c_align(**kw)
    st = out["status"]
    assert [int(st[i]) for i in (0, 2, 3, 4, 5, 6)] == want and st[7] == 0 and st[1] == len(kw["tau"])
    assert st[3] + st[4] + np.isfinite(out["preint"][:, 0]).sum() == st[2]
    failed_scale, failed_gyro = bool(st[0] & ir.SCALE_FAILED), bool(st[0] & ir.GYRO_FAILED)
    for key in ("velocity", "residual"):
        assert np.isnan(out[key]).all() == failed_scale or out[key].size == 0, key
    assert np.isnan(out["result"][[0, 1, 2, 3, 7, 8]]).all() == failed_scale
    assert np.isnan(out["result"][4:7]).all() == failed_gyro
    if st[0] & ir.BAD_ORDER:
        assert np.isnan(out["preint"]).all() and np.isnan(out["result"][:9]).all()
    ref = ir.align(**kw, bias_g1=None if failed_gyro else out["result"][4:7])
    assert np.array_equal(np.isnan(out["preint"]), np.isnan(ref["preint"]))
    if not failed_gyro:
        assert np.abs(out["result"][4:7] - ref["bias_g"]).max() == 0        # (fed back: the same words)
        assert np.isfinite(out["result"][4:7]).all()                        # the bias stays valid when only the scale failed
        check_sums(out["normal"], ref["normal"], st, name)
    if not failed_scale:
        check_solves(out, 0.0, name)
        assert np.array_equal(np.isnan(out["velocity"]), np.isnan(ref["velocity"]))
        assert np.array_equal(np.isnan(out["residual"]), np.isnan(ref["residual"]))


def test_refusals():
    s = {**ir.scene(), **ir.EXTR}
    EINVAL, EWORKSPACE = -1, -3
    for over in (dict(N=0), dict(T=1), dict(stride=0), dict(stride=300), dict(flags=2), dict(max_gap=0.0), dict(max_gap=float("nan")),
                 dict(G=-1.0), dict(G=float("inf")), dict(steps=0), dict(steps=17), dict(tau=None), dict(knots=None), dict(result=None),
                 dict(status=None), dict(ws=None), dict(residual=None), dict(bg=host_triple([0, np.nan, 0])),
                 dict(ext=host_triple([np.inf] * 12, 12)), dict(ext=host_triple(np.concatenate([1.001 * ir.R_BC.reshape(-1), ir.P_BC]), 12)),
                 dict(ext=host_triple(np.concatenate([(ir.R_BC * [1, 1, -1]).reshape(-1), ir.P_BC]), 12)),      # scaled; a reflection
                 dict(ext=host_triple(np.concatenate([(ir.R_BC + [[0, 1e-4, 0]] * 3).reshape(-1), ir.P_BC]), 12))):
        assert c_align(**s, rc_only=True, over=over) == EINVAL, over
    assert c_align(**s, rc_only=True, over=dict(nbytes=64)) == EWORKSPACE
    for over in (dict(N=0), dict(T=1), dict(stride=0), dict(flags=4), dict(max_gap=-1.0), dict(preint=None), dict(status=None),
                 dict(gyro=None), dict(ba=host_triple([np.inf, 0, 0]))):
        assert c_preintegrate(s["tau"], s["gyro"], s["accel"], s["times"], rc_only=True, over=over) == EINVAL, over


def test_side_stream_and_the_wrappers():
    """ops.imu_align / ops.imu_preintegrate on a side stream give the bits of the C entry on the default stream"""
    from rampvo_amd import ops
    args, want = scene_run("scene9.80665", gravity_norm=9.80665)
    dev = {k: cu(args[k]) for k in ("tau", "gyro", "accel", "knots", "times")}
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        out = ops.imu_align(dev["tau"], dev["gyro"], dev["accel"], dev["knots"], dev["times"], R_bc=ir.R_BC, p_bc=ir.P_BC,
                            gravity_norm=9.80665, want_preint=True)
        with pytest.raises(RuntimeError, match="host value"):               # (a device tensor would have to be read back)
            ops.imu_preintegrate(dev["tau"], dev["gyro"], dev["accel"], dev["times"], bias_g=out["bias_g"])
        with pytest.raises(RuntimeError, match="host value"):
            ops.imu_align(dev["tau"], dev["gyro"], dev["accel"], dev["knots"], dev["times"], R_bc=cu(ir.R_BC))
        pre, st = ops.imu_preintegrate(dev["tau"], dev["gyro"], dev["accel"], dev["times"], bias_g=want["result"][4:7])
    side.synchronize()
    for k in want:
        assert georef.same_bits(out[k].cpu().numpy(), want[k]), k
    assert georef.same_bits(pre.cpu().numpy(), want["preint"])              # the same bias: the final integration's records
    assert out["scale"].data_ptr() == out["result"].data_ptr() and float(out["scale"]) == want["result"][0]
    d = ops.imu_status(out["status"])
    assert d == dict(bad_order=False, gyro_failed=False, scale_failed=False, few_triples=False, singular=False, bad_scale=False,
                     n_samples=2400, n_intervals=219, n_uncovered=0, n_dt_not_positive=0, n_gyro_intervals=219, n_triples=218)
    assert ops.imu_status(st)["n_gyro_intervals"] == 0


# ------------------------------------------------------------------------------------------------ 3. tracker
def _tracker_query(slam, f):
    from rampvo_amd import ops
    tau, gyro, accel = kit.imu_samples(f)
    with pytest.raises(RuntimeError, match="set_imu"):
        slam.align_imu(tau, gyro, accel)
    slam.set_imu(R_bc=ir.R_BC, p_bc=ir.P_BC, bias_g=[0.01, 0.0, -0.01])
    got = kit.host(slam.align_imu(cu(tau), cu(gyro), cu(accel), as_tensor=True, want_preint=True))
    knots, tst = slam.trajectory(as_tensor=True)
    want = kit.host(ops.imu_align(cu(tau), cu(gyro), cu(accel), knots, cu(np.asarray(tst, np.float64)), R_bc=ir.R_BC, p_bc=ir.P_BC,
                                  bias_g=[0.01, 0.0, -0.01], gravity_norm=9.80665, want_preint=True))
    kit.same(got, want, "align_imu")
    n = len(tst) - 1
    assert n >= 3 and list(got["status"][2:6]) == [n, 0, 0, n]              # every interval between two frames is covered
    if got["status"][0]:
        with pytest.raises(RuntimeError, match="align_imu"):
            slam.align_imu(tau, gyro, accel)
    else:
        host = slam.align_imu(tau, gyro, accel, want_preint=True)
        assert host["scale"] == got["result"][0] and georef.same_bits(host["velocity"], got["velocity"])
    return got


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
