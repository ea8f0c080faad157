"""The numpy restatement of the IMU propagation (tests/propref.py, include/ramp_hip.h ``ramp_imu_propagate``) has to earn its
place before the GPU test trusts it: closed forms, the analytic scene with the integration rule's own order of convergence, the
last row against ``imuref.preintegrate_interval``, the status words of every failure case the GPU test runs, and ten deliberate
mistakes, each of which has to move a checked row by more than 100 of its bounds.  Also the C ABI surface and the queries'
status check."""
import os
import re

import numpy as np
import pytest

import imuref as ir
import propref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.array([0.3, -0.2, -9.79])
Q0 = ir.quat_from_R(ir.so3_exp(np.array([0.3, -0.4, 0.2])))
P0, V0 = np.array([0.5, -1.0, 2.0]), np.array([0.4, 0.1, -0.3])


def _grid(n=121, rate=200.0, first=0.0):
    return first + np.arange(n) / rate


def _body_state(out, anchor, R_bc, p_bc):
    """(R0, p0) of the anchor as the definition forms them"""
    R0 = ir.R_from_quat(anchor[4:8] / np.linalg.norm(anchor[4:8])) @ np.asarray(R_bc).T
    return R0, anchor[11] * anchor[1:4] - R0 @ np.asarray(p_bc)


# ------------------------------------------------------------------------------------------------ closed forms
def test_free_fall():
    tau = _grid()
    t0 = 0.0123
    anchor = pr.make_anchor(t0, P0, Q0, V0, 2.0, G, np.zeros(3))
    out = pr.propagate(tau, np.zeros((121, 3)), np.zeros((121, 3)), anchor)
    assert list(out["status"]) == [0, 121, 3, 118, 0, 0, 0, 0]
    t = (np.maximum(tau, t0) - t0)[:, None]
    assert np.abs(out["state"][:, 0] - t[:, 0]).max() < 1e-15
    assert np.abs(out["state"][:, 8:11] - (2.0 * P0 + V0 * t + 0.5 * G * t * t)).max() < 1e-14
    assert np.abs(out["state"][:, 5:8] - (V0 + G * t)).max() < 1e-14
    assert np.abs(out["poses64"][:, :3] * 2.0 - out["state"][:, 8:11]).max() < 1e-15         # no lever arm: the camera is the body
    assert np.array_equal(out["times"], np.maximum(tau, t0)) and (out["state"][:, 11:] == 0).all()


def test_at_rest_every_row_is_the_anchor():
    tau = _grid()
    R = ir.R_from_quat(Q0)
    anchor = pr.make_anchor(0.2, P0, Q0, np.zeros(3), 1.5, G, np.zeros(3))
    out = pr.propagate(tau, np.zeros((121, 3)), np.tile(-R.T @ G, (121, 1)), anchor)
    assert np.abs(out["state"][:, 8:11] - 1.5 * P0).max() < 1e-14 and np.abs(out["state"][:, 5:8]).max() < 1e-14
    assert np.abs(out["poses64"] - np.concatenate([P0, Q0])).max() < 1e-14


def test_constant_rate_about_a_fixed_axis_and_the_lever_arm():
    tau = _grid()
    w, t0, s = np.array([0.7, -1.1, 0.4]), 0.0123, 3.0
    bias = np.array([0.01, -0.02, 0.015])
    anchor = pr.make_anchor(t0, P0, Q0, np.zeros(3), s, np.zeros(3), bias)
    out = pr.propagate(tau, np.tile(w + bias, (121, 1)), np.zeros((121, 3)), anchor, R_bc=ir.R_BC, p_bc=ir.P_BC)
    R0, p0 = _body_state(out, anchor, ir.R_BC, ir.P_BC)
    for i in (0, 3, 60, 120):
        Rwb = R0 @ ir.so3_exp(w * (max(tau[i], t0) - t0))
        assert np.abs(ir.R_from_quat(out["state"][i, 1:5]) - Rwb).max() < 1e-13
        assert np.abs(out["state"][i, 8:11] - p0).max() < 1e-14                             # pure rotation: the body stays
        assert np.abs(out["poses64"][i, :3] - (p0 + Rwb @ ir.P_BC) / s).max() < 1e-13       # ... and the camera goes round
        assert np.abs(ir.R_from_quat(out["poses64"][i, 3:]) - Rwb @ ir.R_BC).max() < 1e-13
    assert np.abs(out["poses64"][0, :3] - P0).max() < 1e-14                                 # a held row is the anchor's knot


# ------------------------------------------------------------------------------------------------ the analytic scene
def _scene_run(rate, t0=5.0, span=0.5, **kw):
    n = int(round((span + 0.02) * rate)) + 1
    tau = t0 - 0.01 + 0.00123 + np.arange(n) / rate
    gyro, accel = np.zeros((n, 3)), np.zeros((n, 3))
    for i, t in enumerate(tau):
        _, _, wv, f = ir.body(t)
        gyro[i], accel[i] = wv + ir.BIAS_TRUE, f
    out = pr.propagate(tau, gyro, accel, pr.scene_anchor(t0), R_bc=ir.R_BC, p_bc=ir.P_BC, **kw)
    i = int(np.searchsorted(tau, t0 + span, "right")) - 1
    pos, R, _, _ = ir.body(tau[i])
    return out, i, np.abs(out["state"][i, 8:11] - pos).max(), np.abs(ir.R_from_quat(out["state"][i, 1:5]) - R).max(), tau, gyro, accel


def test_scene_error_is_the_rules_own_discretisation():
    """Anchored on the true state, the only error is the integration rule's.  The rotation is the midpoint rule: second order,
    halving the sample spacing divides its error by about 4.  The element turns a sub-interval's `a dt` by the rotation at the
    sub-interval's START (`v1 + R1 v2`: the law of imu.hip, which the propagation takes word for word), which is first order in
    velocity and position: the error is about 1/2 (|a| |w| dt / 2) t^2 = 1/2 (10 x 0.5 x 0.0025) 0.25 = 1.6e-3 m at 200 Hz and
    halves with the spacing.  Measured: position 7.0e-4 -> 3.5e-4, rotation 2.5e-7 -> 6.3e-8."""
    out, i, ep, eR, _, _, _ = _scene_run(200.0)
    _, _, ep2, eR2, _, _, _ = _scene_run(400.0)
    print("position error after 0.5 s at 200 / 400 Hz:", ep, ep2, "rotation:", eR, eR2)
    assert ep < 1.6e-3 and eR < 1e-6
    assert 3.0 < eR / eR2 < 5.0                                                             # second order: about 4
    assert 1.7 < ep / ep2 < 2.3                                                             # first order: about 2


def test_last_row_is_the_preintegral_of_the_whole_span():
    out, _, _, _, tau, gyro, accel = _scene_run(200.0)
    anchor = pr.scene_anchor(5.0)
    rec, why = ir.preintegrate_interval(tau, gyro, accel, 5.0, tau[-1], ir.BIAS_TRUE, np.zeros(3))
    assert why == ""
    R0, p0 = _body_state(out, anchor, ir.R_BC, ir.P_BC)
    st = out["state"][-1]
    dt, v0, g = st[0], anchor[8:11], anchor[12:15]
    assert abs(dt - rec[0]) < 1e-15 and out["m"][-1] == rec[1]
    assert np.abs(R0.T @ ir.R_from_quat(st[1:5]) - ir.R_from_quat(rec[2:6])).max() < 1e-13
    assert np.abs(R0.T @ (st[5:8] - v0 - g * dt) - rec[6:9]).max() < 1e-13
    assert np.abs(R0.T @ (st[8:11] - p0 - v0 * dt - 0.5 * g * dt * dt) - rec[9:12]).max() < 1e-13


# ------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("name", sorted(pr.cases()))
def test_status_arithmetic_of_the_failure_cases(name):
    kw, want, nan_rows = pr.cases()[name]
    out = pr.propagate(**kw)
    st, N = out["status"], len(kw["tau"])
    assert [int(st[i]) for i in (0, 2, 3, 4, 5)] == want and st[1] == N and st[6] == 0 and st[7] == 0
    expect = np.zeros(N, bool)
    expect[nan_rows] = True
    assert np.array_equal(np.isnan(out["state"]).all(axis=1), expect) and np.array_equal(np.isnan(out["state"]).any(axis=1), expect)
    assert np.array_equal(np.isnan(out["poses"]).all(axis=1), expect)
    if st[0]:
        assert np.isnan(out["times"]).all()
    else:
        assert st[2] + st[3] + st[4] + st[5] == st[1]
        assert np.array_equal(out["times"], np.maximum(kw["tau"], kw["anchor"][0]))


# ------------------------------------------------------------------------------------------------ mistakes
def test_every_mistake_moves_a_checked_row_by_100_bounds():
    out, i, _, _, tau, gyro, accel = _scene_run(200.0)
    kw = dict(anchor=pr.scene_anchor(5.0), R_bc=ir.R_BC, p_bc=ir.P_BC)
    ld = pr.propagate(tau, gyro, accel, ft=np.longdouble, **kw)
    fields = dict(dt=(0, 1), q=(1, 5), v=(5, 8), p=(8, 11))
    assert len(pr.MISTAKES) == 10
    for mistake in pr.MISTAKES:
        bad = pr.propagate(tau, gyro, accel, mistake=mistake, **kw)
        moved = 0.0
        for lo, hi in fields.values():
            ref = out["state"][i, lo:hi]
            env = np.abs(ref - ld["state"][i, lo:hi].astype(np.float64)).max()
            moved = max(moved, np.abs(bad["state"][i, lo:hi] - ref).max() / ir.bound(env, out["m"][i], ref))
        ulp = np.spacing(np.abs(out["poses"][i]))
        dq = np.minimum(np.abs(bad["poses"][i, 3:] - out["poses"][i, 3:]), np.abs(bad["poses"][i, 3:] + out["poses"][i, 3:]))
        moved = max(moved, float((np.abs(bad["poses"][i, :3] - out["poses"][i, :3]) / ulp[:3]).max()), float((dq / ulp[3:]).max()))
        print(mistake, "moves row %d by %.3g bounds" % (i, moved))
        assert moved > 100, mistake


# ------------------------------------------------------------------------------------------------ the surface
def test_c_abi_surface():
    from rampvo_amd import _lib, ops
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    for name in ("ramp_imu_propagate", "ramp_imu_propagate_workspace_bytes"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    for name, value in dict(ANCHOR_WORDS=pr.ANCHOR_WORDS, BAD_ANCHOR=pr.BAD_ANCHOR, NO_START=pr.NO_START).items():
        assert re.search(r"#define RAMP_IMU_%s %d\b" % (name, value), header) and getattr(_lib, "RAMP_IMU_" + name) == value
    assert lib.ramp_imu_propagate_workspace_bytes(0) == 0
    assert lib.ramp_imu_propagate_workspace_bytes(4097) == 64 + (65 + 2) * 11 * 8           # 11 doubles per chunk and per tile
    assert set(ops._STATUS["imu_propagate"][0]) == {"bad_order", "bad_anchor", "no_start"}
    assert ops._STATUS["imu_propagate"][1] == ("n_samples", "n_held", "n_propagated", "n_cut_off", "n_beyond_horizon")
    assert len(ops._STATUS["imu"][1]) == 6 and "bad_anchor" not in ops._STATUS["imu"][0]     # the old entries' words are as they were
    for fn in (ops.imu_anchor, ops.imu_propagate, ops.imu_propagate_status):
        assert callable(fn)


def test_queries_raise_on_the_propagation_bits():
    import torch
    from rampvo_amd import queries
    word = lambda w: torch.tensor([w, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32)
    assert queries._check_status("q", imu=word(0), propagate=word(0)) is None
    for w, text in ((pr.BAD_ORDER, "decrease or are not finite"), (pr.BAD_ANCHOR, "anchor is not finite"),
                    (pr.NO_START, "at or before the anchor")):
        with pytest.raises(RuntimeError, match=text):
            queries._check_status("q", propagate=word(w))
    with pytest.raises(RuntimeError, match="gyro bias step failed"):                         # the alignment's bits come first
        queries._check_status("q", imu=word(ir.GYRO_FAILED), propagate=word(pr.BAD_ANCHOR))
    assert hasattr(queries.TrackerQueries, "propagate_imu")
