"""The numpy restatement of the IMU entries (tests/imuref.py, include/ramp_hip.h ``ramp_imu_preintegrate`` / ``ramp_imu_align``)
has to earn its place before the GPU test trusts it: closed forms, the composition law, the bias Jacobian against a central
difference, recovery on the analytic scene, and eleven deliberate mistakes, each of which has to move a quantity the GPU test
checks by more than 100 of that quantity's bounds.  Also the status words the GPU test expects of every failure case, the
C ABI surface, the status check of the queries and ``evaluate.metric_trajectory``."""
import os
import re

import numpy as np
import pytest

import imuref as ir

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


def _grid(n=40, rate=200.0, t0=0.0):
    return t0 + np.arange(n) / rate


# ------------------------------------------------------------------------------------------------ closed forms
def test_constant_rate_and_acceleration_give_the_exact_preintegral():
    tau = _grid(41)
    w, a = np.array([0.7, -1.1, 0.4]), np.array([0.3, 9.0, -2.0])
    T0, T1 = 0.0123, 0.1871
    rec, why = ir.preintegrate_interval(tau, np.tile(w, (41, 1)), np.zeros((41, 3)), T0, T1, np.zeros(3), np.zeros(3))
    assert why == "" and rec[1] == 36
    dt = T1 - T0
    assert abs(rec[0] - dt) < 1e-15
    assert np.abs(ir.R_from_quat(rec[2:6]) - ir.so3_exp(w * dt)).max() < 1e-13
    assert np.abs(rec[12:21].reshape(3, 3) + ir.so3_jr(w * dt) * dt).max() < 1e-13        # constant rate: J = -Jr(w dt) dt
    rec, _ = ir.preintegrate_interval(tau, np.zeros((41, 3)), np.tile(a, (41, 1)), T0, T1, np.zeros(3), np.zeros(3))
    assert np.abs(rec[6:9] - a * dt).max() < 1e-13 and np.abs(rec[9:12] - 0.5 * a * dt * dt).max() < 1e-13
    assert np.abs(rec[2:6] - [0, 0, 0, 1]).max() == 0 and (rec[21:] == 0).all()
    # the biases are subtracted: a measurement equal to its bias integrates to the identity
    rec, _ = ir.preintegrate_interval(tau, np.tile(w, (41, 1)), np.tile(a, (41, 1)), T0, T1, w, a)
    assert np.abs(rec[6:12]).max() == 0 and np.abs(rec[2:6] - [0, 0, 0, 1]).max() == 0


def test_breakpoints_samples_on_the_ends_and_duplicates():
    tau = _grid(41)
    rng = np.random.default_rng(5)
    g, a = rng.normal(size=(41, 3)), rng.normal(size=(41, 3)) * 5
    z = np.zeros(3)
    m = lambda T0, T1, t=tau, gg=g, aa=a: ir.preintegrate_interval(t, gg, aa, T0, T1, z, z)[0]
    assert m(0.0101, 0.0149)[1] == 1 and m(0.0101, 0.0151)[1] == 2              # no sample inside; one
    assert m(tau[3], tau[9])[1] == 6                                             # a sample on each end is not repeated
    # a duplicated sample is a sub-interval of length 0, an identity: the same record but for the count
    t2, g2, a2 = np.insert(tau, 6, tau[6]), np.insert(g, 6, g[6], 0), np.insert(a, 6, a[6], 0)
    r1, r2 = m(tau[3], tau[9]), m(tau[3], tau[9], t2, g2, a2)
    assert r2[1] == 7 and np.array_equal(r1[[0] + list(range(2, 24))], r2[[0] + list(range(2, 24))])
    # not covered: before the first sample, behind the last, a NaN in a touched sample, a gap
    assert ir.preintegrate_interval(tau, g, a, -0.001, 0.05, z, z)[1] == "uncovered"
    assert ir.preintegrate_interval(tau, g, a, 0.15, 0.2001, z, z)[1] == "uncovered"
    assert ir.preintegrate_interval(tau, g, a, 0.05, 0.05, z, z)[1] == "dt"
    gn = g.copy()
    gn[12, 0] = np.nan                                                           # tau 0.06: the first sample behind [0.05, 0.057]
    assert ir.preintegrate_interval(tau, gn, a, 0.05, 0.057, z, z)[1] == "uncovered"
    assert ir.preintegrate_interval(tau, gn, a, 0.04, 0.052, z, z)[1] == ""
    assert ir.preintegrate_interval(tau, g, a, 0.05, 0.057, z, z, max_gap=0.004)[1] == "uncovered"


def _random_element(rng):
    return (ir.so3_exp(rng.normal(size=3)), rng.normal(size=3), rng.normal(size=3), abs(rng.normal()), rng.normal(size=(3, 3)))


def test_composition_is_associative():
    rng = np.random.default_rng(11)
    for _ in range(20):
        a, b, c = (_random_element(rng) for _ in range(3))
        left, right = ir.compose(ir.compose(a, b), c), ir.compose(a, ir.compose(b, c))
        for x, y in zip(left, right):
            assert np.abs(np.asarray(x) - np.asarray(y)).max() < 1e-13
        ident = ir.identity(np.float64)
        for x, y, z in zip(ir.compose(ident, a), a, ir.compose(a, ident)):
            assert np.array_equal(np.asarray(x), np.asarray(y)) and np.array_equal(np.asarray(z), np.asarray(y))


def test_bias_jacobian_against_a_central_difference():
    s = ir.scene()
    T0, T1, h = 3.0, 3.35, 1e-5
    at = lambda b: ir.preintegrate_interval(s["tau"], s["gyro"], s["accel"], T0, T1, b, np.zeros(3))[0]
    rec = at(ir.BIAS_TRUE)
    J = rec[12:21].reshape(3, 3)
    for i in range(3):
        e = np.zeros(3)
        e[i] = h
        Rm, Rp = ir.R_from_quat(at(ir.BIAS_TRUE - e)[2:6]), ir.R_from_quat(at(ir.BIAS_TRUE + e)[2:6])
        assert np.abs(ir.so3_log(Rm.T @ Rp) / (2 * h) - J[:, i]).max() < 1e-8
    # and the preintegral is the closed-form motion: the body's own rotation between the two times
    R0, R1 = ir.body(T0)[1], ir.body(T1)[1]
    assert np.abs(ir.so3_log(ir.R_from_quat(rec[2:6]).T @ R0.T @ R1)).max() < 1e-5


# ------------------------------------------------------------------------------------------------ the scene
_runs = {}


def run(key="free", **kw):
    if key not in _runs:
        _runs[key] = ir.align(**{**ir.scene(), **ir.EXTR, **kw})
    return _runs[key]


def test_scene_recovers_bias_scale_and_gravity():
    out = run()
    assert np.abs(out["bias_g"] - ir.BIAS_TRUE).max() < 1e-6
    assert abs(out["scale"] / ir.SCALE_TRUE - 1) < 0.01
    assert np.abs(out["gravity"] - ir.G_TRUE).max() < 0.005
    assert list(out["status"]) == [0, 2400, 219, 0, 0, 219, 218, 0]
    assert 5 < out["result"][8] < 20 and out["result"][7] < 1e-3                 # well conditioned; the rule's own residual
    # the velocities are the body's: d/dt of the closed-form position, to the rule's discretisation
    for k in (0, 100, 219):
        t = ir.scene()["times"][k]
        v = (ir.body(t + 1e-6)[0] - ir.body(t - 1e-6)[0]) / 2e-6
        assert np.abs(out["velocity"][k] - v).max() < 0.02
    # a second gyro step changes nothing a user would see, and stride 2 recovers the same quantities
    two = run("two", gyro_steps=2)
    assert np.abs(two["bias_g"] - out["bias_g"]).max() < 1e-7
    st2 = run("stride2", stride=2)
    assert abs(st2["scale"] / ir.SCALE_TRUE - 1) < 0.01 and st2["status"][2] == 109


def test_fixed_norm_refinement_returns_the_norm():
    out = run("fixed", gravity_norm=9.80665)
    assert abs(np.linalg.norm(out["gravity"]) - 9.80665) < 1e-14 * 9.80665 * 4
    assert abs(out["scale"] / ir.SCALE_TRUE - 1) < 0.01 and np.abs(out["gravity"] - ir.G_TRUE).max() < 0.005
    # the refinement is a descent of the same quadratic on the sphere: its cost is no lower than the free minimum's
    N, y = out["normal"][:16].reshape(4, 4), out["normal"][16:20]
    cost = lambda x: x @ N @ x - 2 * y @ x
    free = run()
    assert cost(out["result"][:4]) >= cost(free["result"][:4]) - 1e-12
    b1, b2 = ir.tangent_basis(np.array([0.0, 0.0, -1.0]))
    assert np.array_equal(b1, [0.0, -1.0, 0.0]) and np.array_equal(b2, [-1.0, 0.0, 0.0])    # e = x, the first axis on ties: -z cross x = -y


def test_longdouble_yardstick_is_closer_than_the_bounds():
    assert np.finfo(np.longdouble).eps < 1e-18                                   # the yardstick is extended precision
    s = ir.scene()
    p64, _ = ir.preintegrate(s["tau"], s["gyro"], s["accel"], s["times"][:12], ir.BIAS_TRUE)
    pld, _ = ir.preintegrate(s["tau"], s["gyro"], s["accel"], s["times"][:12], ir.BIAS_TRUE, ft=np.longdouble)
    env = np.abs(p64 - pld.astype(np.float64)).max()
    assert 0 < env < 16 * 11 * EPS                                               # the float64 restatement's own error: a few roundings


# ------------------------------------------------------------------------------------------------ mistakes
def _moved(ref, got):
    """the largest (difference / bound) over the quantities the GPU test checks, with env = 0: the second term of the bound"""
    worst = 0.0
    for name, (lo, hi) in dict(dt=(0, 1), q=(2, 6), dv=(6, 9), dp=(9, 12), J=(12, 21)).items():
        a, b = ref["preint"][:, lo:hi], got["preint"][:, lo:hi]
        for k in range(len(a)):
            if np.isfinite(a[k]).all():
                worst = max(worst, np.abs(a[k] - b[k]).max() / ir.bound(0.0, ref["preint"][k, 1], a[k]))
    terms = {"N": (0, 16, ref["status"][6] * 3), "y": (16, 20, ref["status"][6] * 3), "H": (20, 29, ref["status"][5] * 3),
             "b": (29, 32, ref["status"][5] * 3)}
    for name, (lo, hi, m) in terms.items():
        a, b = ref["normal"][lo:hi], got["normal"][lo:hi]
        worst = max(worst, np.abs(a - b).max() / ir.bound(0.0, m, a))
    return worst


@pytest.mark.parametrize("mistake", ir.MISTAKES)
def test_each_mistake_moves_a_checked_quantity(mistake):
    on = mistake == "end_sample_twice"                        # (shows only where a sample lies on a knot time)
    kw = dict(on_samples=True) if on else {}
    base = {**ir.scene(**kw), **ir.EXTR}
    base["knots"], base["times"] = base["knots"][ir.IRREGULAR], base["times"][ir.IRREGULAR]     # intervals of 0.1 and 0.05 s
    key = "mist_on" if on else "mist_off"
    if key not in _runs:
        _runs[key] = ir.align(**base)
    got = ir.align(**base, mistake=mistake)
    assert _moved(_runs[key], got) > 100, mistake


# ------------------------------------------------------------------------------------------------ status of every GPU case
@pytest.mark.parametrize("name", sorted(ir.cases()))
def test_status_words_of_the_failure_cases(name):
    kw, want = ir.cases()[name]
    out = ir.align(**kw)
    st = out["status"]
    assert [int(st[i]) for i in (0, 2, 3, 4, 5, 6)] == want and st[7] == 0 and st[1] == len(kw["tau"])
    assert st[3] + st[4] + np.isfinite(out["preint"][:, 0]).sum() == st[2]
    failed_scale, failed_gyro = bool(st[0] & ir.SCALE_FAILED), bool(st[0] & ir.GYRO_FAILED)
    assert np.isnan(out["result"][[0, 1, 2, 3, 7, 8]]).all() == failed_scale
    assert np.isnan(out["velocity"]).all() == failed_scale and np.isnan(out["bias_g"]).all() == failed_gyro
    if not failed_gyro:
        assert np.isfinite(out["bias_g"]).all()               # the bias stays valid when only the scale stage failed


# ------------------------------------------------------------------------------------------------ the surface
def test_c_abi_surface():
    from rampvo_amd import _lib, ops
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    for name in ("ramp_imu_preintegrate", "ramp_imu_align", "ramp_imu_workspace_bytes"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name, bit in dict(BAD_ORDER=ir.BAD_ORDER, GYRO_FAILED=ir.GYRO_FAILED, SCALE_FAILED=ir.SCALE_FAILED, FEW_TRIPLES=ir.FEW_TRIPLES,
                          SINGULAR=ir.SINGULAR, BAD_SCALE=ir.BAD_SCALE, PREINT_WORDS=24, F64=1).items():
        assert re.search(r"#define RAMP_IMU_%s %d\b" % (name, bit), header) and getattr(_lib, "RAMP_IMU_" + name) == bit
    assert lib.ramp_imu_workspace_bytes(1000, 2) >= 64 + 128 + 192 and lib.ramp_imu_workspace_bytes(0, 5) == 0
    assert set(ops._STATUS["imu"][0]) == {"bad_order", "gyro_failed", "scale_failed", "few_triples", "singular", "bad_scale"}
    assert len(ops._STATUS["imu"][1]) == 6


def test_queries_raise_on_the_imu_bits():
    import torch
    from rampvo_amd import queries
    word = lambda w: torch.tensor([w, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32)
    assert queries._check_status("q", imu=word(0)) is None
    for w, text in ((ir.BAD_ORDER, "decrease or are not finite"), (ir.GYRO_FAILED, "gyro bias step failed"),
                    (ir.SCALE_FAILED | ir.FEW_TRIPLES, "fewer than two triples"), (ir.SCALE_FAILED | ir.BAD_SCALE, "not positive"),
                    (ir.SCALE_FAILED | ir.SINGULAR, "singular")):
        with pytest.raises(RuntimeError, match=text):
            queries._check_status("q", imu=word(w))


def test_metric_trajectory():
    from rampvo_amd import evaluate
    rng = np.random.default_rng(2)
    poses = np.concatenate([rng.normal(size=(6, 3)), [ir.quat_from_R(ir.so3_exp(v)) for v in rng.normal(size=(6, 3))]], axis=1)
    g = np.array([0.3, -0.2, -9.79])
    out = evaluate.metric_trajectory(poses, dict(scale=2.5, gravity=g))
    # distances scale by s, the turned gravity points down, relative rotations are kept
    assert np.allclose(np.linalg.norm(out[1:, :3] - out[:-1, :3], axis=1), 2.5 * np.linalg.norm(poses[1:, :3] - poses[:-1, :3], axis=1))
    R = ir.R_from_quat(out[0, 3:]) @ ir.R_from_quat(poses[0, 3:]).T
    assert np.allclose(R @ g / np.linalg.norm(g), [0, 0, -1]) and np.allclose(R @ R.T, np.eye(3))
    assert np.allclose(out[:, :3], 2.5 * poses[:, :3] @ R.T)
    for k in range(6):
        assert np.allclose(ir.R_from_quat(out[k, 3:]), R @ ir.R_from_quat(poses[k, 3:]))
    same = evaluate.metric_trajectory(poses, dict(scale=1.0, gravity=[0, 0, -9.8]))
    assert np.allclose(same, poses)
    flip = evaluate.metric_trajectory(poses, dict(scale=1.0, gravity=[0, 0, 9.8]))
    assert np.allclose(np.abs(flip[:, 2]), np.abs(poses[:, 2])) and np.allclose(flip[:, 2], -poses[:, 2])
    with pytest.raises(RuntimeError, match="finite positive scale"):
        evaluate.metric_trajectory(poses, dict(scale=np.nan, gravity=g))
