"""The float64 restatement of the window's uncertainty (tests/covref.py) has to earn its place as the GPU tests' reference:
it is checked against the full (unreduced) normal equations, and the comparison the GPU tests use must reject the mistakes
the definition invites.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import covref  # noqa: E402
from oracle.make_golden_params import BA_PIN  # noqa: E402
from scenes import ba_pin_scene  # noqa: E402

_cache = {}


def _case(tag):
    if tag not in _cache:
        s = ba_pin_scene(**BA_PIN[tag])
        n = s["n_frames"]
        _cache[tag] = (s, 1, n, covref.covariance(s, 1, n, np.float64), covref.covariance(s, 1, n, np.float32))
    return _cache[tag]


@pytest.mark.parametrize("tag", ["w10", "w30"])
def test_schur_identity(tag):
    """H = [[B + D, E], [E', diag(C + lambda)]] with D the solver's damping: the pose block of H^-1 is cov, the diagonal of
    its depth block is depth_var, both to 1e-9 relative"""
    s, t0, t1, r, _ = _case(tag)
    n6, Mu = r["B"].shape[0], r["Mu"]
    H = np.zeros((n6 + Mu, n6 + Mu))
    H[:n6, :n6] = r["B"] + np.diag(r["D"])
    H[:n6, n6:] = r["E"]
    H[n6:, :n6] = r["E"].T
    H[n6:, n6:] = np.diag(r["C"] + float(np.asarray(s["lmbda"]).reshape(-1)[0]))
    Hi = np.linalg.inv(H)
    assert np.abs(Hi[:n6, :n6] - r["cov"]).max() <= 1e-9 * np.abs(r["cov"]).max()
    zz = np.diag(Hi)[n6:]
    assert (np.abs(zz - r["depth_var"][r["uk"]]) <= 1e-9 * zz).all()
    assert np.array_equal(r["cov"], r["cov"].T) or np.abs(r["cov"] - r["cov"].T).max() <= 1e-12 * np.abs(r["cov"]).max()


@pytest.mark.parametrize("tag", ["w10", "w30"])
def test_the_float32_envelope_is_small_and_the_right_answer_passes(tag):
    s, t0, t1, r64, r32 = _case(tag)
    ok, rep = covref.compare(r32["cov"], r32["depth_var"], r64, r32)
    print(tag, "cond(S) %.3g" % np.linalg.cond(r64["S"]), rep)
    assert ok, rep


@pytest.mark.parametrize("what", ["damping", "q_term", "ji_sign", "gate"])
@pytest.mark.parametrize("tag", ["w10", "w30"])
def test_the_comparison_has_teeth(tag, what):
    """each mistake, computed in float64 and rounded to float32 like a kernel's output, is rejected by covref.compare"""
    s, t0, t1, r64, r32 = _case(tag)
    if what == "gate":                      # one factor 200 px off: the reference gates it, the mistake keeps it
        s = dict(s, target=s["target"].copy())
        s["target"][7] += 200.0
        r64, r32 = covref.covariance(s, t0, t1, np.float64), covref.covariance(s, t0, t1, np.float32)
        assert not r64["valid"][7]
        bad = covref.covariance(s, t0, t1, np.float64, ungated_edge=7)
    else:
        kw = dict(damping=dict(damping=False), q_term=dict(q_term=False), ji_sign=dict(ji_sign=1.0))[what]
        bad = covref.covariance(s, t0, t1, np.float64, **kw)
    ok, rep = covref.compare(bad["cov"].astype(np.float32), bad["depth_var"].astype(np.float32), r64, r32)
    assert not ok, (what, rep)


def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_ba_covariance", "ramp_ba_covariance_workspace_bytes", "ramp_ba_covariance_planned",
                 "ramp_ba_covariance_planned_workspace_bytes", "ramp_track_uncertainty",
                 "ramp_track_uncertainty_workspace_bytes"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    # argument checks that need no GPU
    assert lib.ramp_ba_covariance(*([None] * 9), 4, 3, 2, 2, 1, 0, None, None, None, None, 0, None, None) == -1   # t1 < t0
    assert lib.ramp_ba_covariance(*([None] * 9), 4, 3, 40, 80, 1, 35, None, None, None, None, 0, None, None) == -4  # 34 free poses
    assert lib.ramp_track_uncertainty(None, 0, None, None, None, None, 0, None) == -1
    assert lib.ramp_ba_covariance_workspace_bytes(100, 11, 88, 1, 11) > lib.ramp_ba_workspace_bytes(100, 11, 88, 1, 11)
    from rampvo_amd import fastba
    from rampvo_amd.Ramp_vo import Ramp_vo
    assert callable(fastba.covariance) and callable(Ramp_vo.uncertainty)
