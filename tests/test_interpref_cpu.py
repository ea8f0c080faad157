"""The float64 restatement of the continuous-time pose query (tests/interpref.py) has to earn its place as the GPU test's
reference: the properties the definition promises (knots at their own times, one-parameter subgroup, inverses, the twist as
the curve's time derivative), the comparison the GPU test uses against the mistakes the definition invites, and the new entry
points' export.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import georef  # noqa: E402
import interpref  # noqa: E402
import oracle as orc  # noqa: E402


def _walk(T=9, seed=3, **kw):
    knots, times = interpref.walk_scene(seed, T, **kw)
    return knots.astype(np.float64), times


def test_knots_are_returned_at_their_own_times():
    """X(times[k]) = X[k] (unit quaternions): <= 1e-14, for distinct stamps and with the LAST pair repeated (the clamped
    zero-length segment: alpha = 1)"""
    knots, times = _walk()
    knots[:, 3:] /= np.linalg.norm(knots[:, 3:], axis=1, keepdims=True)
    out, _ = interpref.interpolate(knots, times, times)
    assert georef.pose_err(out, knots) <= 1e-14
    t2 = times.copy()
    t2[-1] = t2[-2]
    out, tw = interpref.interpolate(knots, t2, t2)
    assert georef.pose_err(out[:-2], knots[:-2]) <= 1e-14
    # both queries at the repeated stamp land on the upper knot of the pair; the zero-length segment has no twist
    assert georef.pose_err(out[-2:], knots[[-1, -1]]) <= 1e-14 and not tw[-2:].any()
    one, tw1 = interpref.interpolate(knots[:1], times[:1], np.array([-5.0, 0.0, 7.0]))
    assert georef.pose_err(one, np.repeat(knots[:1], 3, 0)) <= 1e-14 and not tw1.any()


def test_one_parameter_subgroup():
    """Exp(a xi) Exp(b xi) X = Exp((a + b) xi) X: moving on from X(t_a) by the same twist reaches X(t_a + t_b)"""
    knots, times = _walk(T=2)
    xi = orc.se3_log_f64(orc.se3_mul_f64(knots[1:2], orc.se3_inv_f64(knots[0:1])))
    for a, b in ((0.25, 0.5), (0.1, 0.9), (0.5, 0.7)):
        Xa, _ = interpref.interpolate(knots, times, np.array([a]), extrapolate=True)
        Xab, _ = interpref.interpolate(knots, times, np.array([a + b]), extrapolate=True)
        step = orc.se3_mul_f64(orc.se3_exp_f64(np.float64(np.float32(b)) * xi), Xa)
        assert georef.pose_err(step, Xab) <= 1e-7          # (alpha is rounded to fp32 once: a + b carries 6e-8)


def test_interpolating_inverses_gives_the_inverse():
    knots, times = _walk()
    q = np.linspace(times[0] - 0.5, times[-1] + 0.5, 41)
    for ex in (False, True):
        out, _ = interpref.interpolate(knots, times, q, extrapolate=ex)
        out_i, _ = interpref.interpolate(orc.se3_inv_f64(knots), times, q, extrapolate=ex)
        assert georef.pose_err(orc.se3_inv_f64(out_i), out) <= 1e-12


def test_twist_is_the_time_derivative_of_the_curve():
    """twist = d/dt Log(X(t + h) X(t - h)^-1) / 2h inside a segment (the left twist is constant there)"""
    knots, times = _walk(dt=0.25)
    q = times[:-1] + 0.4 * np.diff(times)
    h = 1e-3 * 0.25
    _, tw = interpref.interpolate(knots, times, q)
    Xp, _ = interpref.interpolate(knots, times, q + h)
    Xm, _ = interpref.interpolate(knots, times, q - h)
    fd = orc.se3_log_f64(orc.se3_mul_f64(Xp, orc.se3_inv_f64(Xm))) / (2 * h)
    assert np.abs(fd - tw).max() <= 1e-3 * max(1.0, np.abs(tw).max())      # (alpha's fp32 rounding, 6e-8 / 2e-3 relative, leads)


# ------------------------------------------------------------------------------------------- the comparison's teeth
def _case(mistake):
    """(knots, times, query, extrapolate) on which the mistake shows"""
    if mistake == "lower":                          # a repeated stamp in the interior whose two knots differ
        knots, times = interpref.walk_scene(5, 6, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2))
        times = np.array([0.0, 1.0, 1.0, 2.0, 3.0, 3.0])
        return knots, times, np.array([0.5, 1.0, 1.5, 3.0]), False
    if mistake == "alpha32":                        # absolute times near 1.7e9, 1 ms apart
        knots, times = interpref.walk_scene(6, 9, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2), t0=1.7e9, dt=1e-3)
        return knots, times, times[:-1] + 0.37 * np.diff(times), False
    if mistake == "noclamp":
        knots, times = interpref.walk_scene(7, 5, step=(0.3, 0.2, 0.3, 0.2, 0.2, 0.2))
        return knots, times, np.array([-2.0, -0.5, 1.5, 4.5, 7.0]), False
    knots, times = interpref.pair_scene(8, 8, 1.0, 1.0)         # 1 rad and a unit translation per segment
    return knots, times, np.repeat(times[0::2], 3) + np.tile([0.25, 0.5, 0.75], 8), False


@pytest.mark.parametrize("mistake", interpref.MISTAKES)
def test_the_comparison_rejects_the_mistake(mistake):
    """the restatement with one deliberate mistake, handed to ``interpref.compare`` as if it were the kernel's output: the
    check the GPU test uses has to say no -- and yes to the unbroken fp32 restatement on the same case"""
    knots, times, query, ex = _case(mistake)
    good, _ = interpref.interpolate(knots, times, query, ex, np.float32)
    res = interpref.compare(good, knots, times, query, ex)
    assert res["ok"], res
    wrong, _ = interpref.interpolate(knots, times, query, ex, np.float64, mistake=mistake)
    res = interpref.compare(wrong, knots, times, query, ex)
    print("%-8s err %.2e  env %.2e  bound %.2e" % (mistake, res["err"], res["env"], res["bound"]))
    assert not res["ok"] and res["err"] > 10 * res["bound"], res


def test_failure_conventions_of_the_restatement():
    knots, times = _walk()
    q = np.array([0.5, np.nan, 2.5])
    out, tw = interpref.interpolate(knots, times, q)
    assert np.isnan(out[1]).all() and np.isnan(tw[1]).all() and np.isfinite(out[[0, 2]]).all()
    bad = times.copy()
    bad[4] = bad[3] - 0.1
    out, tw = interpref.interpolate(knots, bad, q)
    assert np.isnan(out).all() and np.isnan(tw).all()
    res = interpref.compare(np.full((3, 7), np.nan), knots, bad, q)
    assert res["ok"]                                # all rows NaN is what the definition asks for
    assert not interpref.compare(np.zeros((3, 7)), knots, bad, q)["ok"]


def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_se3_interp", "ramp_se3_interp_workspace_bytes", "ramp_se3_interp_lds_knots"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert lib.ramp_se3_interp_workspace_bytes(1) == 64 and lib.ramp_se3_interp_workspace_bytes(9) == 8 * 64
    assert lib.ramp_se3_interp_lds_knots() >= 64
    for macro, val in (("RAMP_INTERP_EXTRAPOLATE", _lib.RAMP_INTERP_EXTRAPOLATE), ("RAMP_INTERP_ROW_STORES", _lib.RAMP_INTERP_ROW_STORES),
                       ("RAMP_INTERP_BAD_TIMES", _lib.RAMP_INTERP_BAD_TIMES)):
        assert re.search(r"#define %s %d\b" % (macro, val), header), macro
