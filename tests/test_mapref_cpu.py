"""The float64 restatement of the map with its uncertainty (tests/mapref.py) has to earn its place as the GPU test's reference:
the pose-depth and depth blocks against the dense inverse of the full damped normal matrix, the two Jacobians against central
finite differences of the point function, the comparison the GPU test uses against the mistakes the definition invites, and
the numpy statement of the selection on hand-made inputs.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import covref  # noqa: E402
import mapref  # noqa: E402
from oracle.make_golden_params import BA_PIN  # noqa: E402
from scenes import ba_pin_scene  # noqa: E402

CASES = {"w10": 1, "w10_t4": 4}           # tag: t0 (both on BA_PIN["w10"])
_cache = {}


def _case(tag):
    if tag not in _cache:
        s = ba_pin_scene(**BA_PIN["w10"])
        s = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in s.items()}
        t0, n = CASES[tag], s["n_frames"]
        _cache[tag] = (s, t0, n, mapref.map_covariance(s, t0, n, np.float64), mapref.map_covariance(s, t0, n, np.float32))
    return _cache[tag]


@pytest.mark.parametrize("tag", list(CASES))
def test_cross_and_depth_blocks_equal_the_dense_inverse(tag):
    """H = [[B + D, E], [E', diag(C + lambda)]]: the pose-depth block of H^-1 is -Q_k S^-1 e_k (whose source-frame rows are
    pose_depth_cov), the diagonal of its depth block is depth_var -- 1e-9 relative (1e-13 measured)"""
    s, t0, t1, m64, _ = _case(tag)
    r = m64["cov"]
    n6, Mu = r["B"].shape[0], r["Mu"]
    H = np.zeros((n6 + Mu, n6 + Mu))
    H[:n6, :n6] = r["B"] + np.diag(r["D"])
    H[:n6, n6:] = r["E"]
    H[n6:, :n6] = r["E"].T
    H[n6:, n6:] = np.diag(r["C"] + float(np.asarray(s["lmbda"]).reshape(-1)[0]))
    Hi = np.linalg.inv(H)
    cross = Hi[:n6, n6:]
    scale = np.abs(cross).max()
    full = -r["Q"][None] * (r["cov"] @ r["E"])
    e_full = np.abs(cross - full).max() / scale
    n_free, e_c = 0, 0.0
    for g, (k, i) in enumerate(zip(m64["uk"], m64["src"])):
        if t0 <= i < t1:
            a = 6 * (i - t0)
            e_c = max(e_c, np.abs(cross[a:a + 6, g] - m64["pose_depth_cov"][k]).max() / scale)
            n_free += 1
        else:
            assert not m64["pose_depth_cov"][k].any()
    zz = np.diag(Hi)[n6:]
    e_z = (np.abs(zz - r["depth_var"][r["uk"]]) / zz).max()
    print(tag, "cross %.2e, source rows %.2e (%d free of %d), depth %.2e" % (e_full, e_c, n_free, Mu, e_z))
    assert n_free > 0 and (tag == "w10" or n_free < Mu)
    assert e_full <= 1e-9 and e_c <= 1e-9 and e_z <= 1e-9


def test_jacobians_equal_central_differences():
    """J_p under T <- Exp(xi) T and J_d under d <- d + z against central differences of the point function, float64, step 1e-6,
    1e-7 relative to the largest entry of the Jacobian"""
    s, _, _, m64, _ = _case("w10")
    poses, pat = np.asarray(s["poses"], np.float64), np.asarray(s["patches"], np.float64)
    fx, fy, cx, cy = np.asarray(s["intr"], np.float64).reshape(-1, 4)[0]
    h, worst = 1e-6, 0.0
    for k, i in list(zip(m64["uk"], m64["src"]))[::7]:
        R, t, d = mapref.quat_R(poses[i, 3:]), poses[i, :3], pat[k, 2, 1, 1]
        ray = np.array([(pat[k, 0, 1, 1] - cx) / fx, (pat[k, 1, 1, 1] - cy) / fy, 1.0])
        Jp, Jd = mapref.jacobians(R, ray, d)
        assert np.allclose(mapref.point_of(R, t, ray, d), m64["point"][k], rtol=0, atol=1e-12 * np.abs(m64["point"][k]).max())
        fd = np.zeros((3, 6))
        for c in range(6):
            xi = np.zeros(6)
            xi[c] = h
            (Ra, ta), (Rb, tb) = mapref.se3_exp(xi), mapref.se3_exp(-xi)
            fd[:, c] = (mapref.point_of(Ra @ R, Ra @ t + ta, ray, d) - mapref.point_of(Rb @ R, Rb @ t + tb, ray, d)) / (2 * h)
        fdd = (mapref.point_of(R, t, ray, d + h) - mapref.point_of(R, t, ray, d - h)) / (2 * h)
        worst = max(worst, np.abs(fd - Jp).max() / np.abs(Jp).max(), np.abs(fdd - Jd).max() / np.abs(Jd).max())
    print("largest relative difference %.2e" % worst)
    assert worst <= 1e-7


@pytest.mark.parametrize("tag", list(CASES))
def test_the_float32_envelope_is_small_and_the_right_answer_passes(tag):
    s, t0, t1, m64, m32 = _case(tag)
    ok, rep = mapref.compare(m32["point_cov"], m32["pose_depth_cov"], m64, m32)
    print(tag, rep)
    assert ok, rep
    assert np.array_equal(m64["n_obs"], m32["n_obs"]) and m64["n_obs"].sum() == m64["cov"]["n_valid"]


MUTATIONS = dict(cross_dropped=dict(cross=0.0), cross_sign=dict(cross=-1.0), right_perturbation=dict(right=True),
                 columns_exchanged=dict(swap=True), jd_without_d2=dict(jd_no_d2=True))


@pytest.mark.parametrize("what", list(MUTATIONS))
@pytest.mark.parametrize("tag", list(CASES))
def test_the_comparison_has_teeth(tag, what):
    """each mistake, computed in float64 and rounded to float32 like a kernel's output, is rejected by mapref.compare"""
    s, t0, t1, m64, m32 = _case(tag)
    bad = mapref.map_covariance(s, t0, t1, np.float64, ref=m64["cov"], **MUTATIONS[what])
    ok, rep = mapref.compare(bad["point_cov"].astype(np.float32), bad["pose_depth_cov"].astype(np.float32), m64, m32)
    print(tag, what, rep)
    assert not ok, (what, rep)
    if what in ("right_perturbation", "columns_exchanged", "jd_without_d2"):      # (point_cov alone has to catch these)
        assert rep["point_cov"][0] > rep["point_cov"][1], rep


def test_select_reference_on_hand_made_inputs():
    nan, inf = np.nan, np.inf
    one = [1.0, 0, 0, 1.0, 0, 1.0]                      # trace 3
    pc = np.array([one,                                 # 0 plain
                   [nan, 0, 0, 1, 0, 1],                # 1 NaN on the diagonal
                   [1, 0, inf, 1, 0, 1],                # 2 inf off the diagonal
                   [4.0, 0, 0, 0, 0, 0],                # 3 sigma == 2 exactly
                   one,                                 # 4 zero depth
                   one,                                 # 5 one observation
                   [9.0, 0, 0, 0, 0, 0],                # 6 sigma 3
                   one], np.float32)                    # 7 relative depth sigma == 0.5 exactly
    dv = np.array([0.01, 0.01, 0.01, 0.01, 0.01, 0.01, 0.01, 0.25], np.float32)
    d = np.array([1, 1, 1, 1, 0, 1, 1, 1], np.float32)
    n_obs = np.array([3, 3, 3, 3, 3, 1, 3, 3], np.int32)
    sel = lambda **kw: mapref.select(pc, dv, d, n_obs, **kw).tolist()
    assert sel() == [0, 3, 4, 5, 6, 7]                                  # only the six finite entries
    assert sel(max_sigma=inf, max_rel_depth_sigma=inf, min_obs=0) == sel()
    assert sel(max_sigma=2.0) == [0, 3, 4, 5, 7]                        # equal to the threshold passes
    assert sel(max_sigma=np.nextafter(np.float32(2.0), np.float32(0))) == [0, 4, 5, 7]
    assert sel(max_rel_depth_sigma=0.5) == [0, 3, 5, 6, 7]              # zero depth: inf never passes
    assert sel(max_rel_depth_sigma=0.4) == [0, 3, 5, 6]
    assert sel(min_obs=2) == [0, 3, 4, 6, 7]
    assert sel(max_sigma=2.0, max_rel_depth_sigma=0.4, min_obs=2) == [0, 3]
    assert sel(max_sigma=0.0) == []
    assert mapref.select(pc, np.full(8, nan, np.float32), d, n_obs, max_rel_depth_sigma=1e30).tolist() == []
    assert mapref.select(pc[:0], dv[:0], d[:0], n_obs[:0]).dtype == np.int32


def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_ba_map_covariance", "ramp_ba_map_covariance_workspace_bytes", "ramp_ba_map_covariance_planned",
                 "ramp_ba_map_covariance_planned_workspace_bytes", "ramp_track_map", "ramp_track_map_workspace_bytes",
                 "ramp_map_select"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    # argument checks that need no GPU
    assert lib.ramp_ba_map_covariance(*([None] * 9), 4, 3, 2, 2, 1, 0, *([None] * 7), None, 0, None, None) == -1
    assert lib.ramp_track_map(None, 0, *([None] * 7), None, 0, None) == -1
    assert lib.ramp_map_select(None, None, None, None, 4, 3, None, 0, 1.0, 1.0, 0, None, None, None) == -1
    assert (lib.ramp_ba_map_covariance_workspace_bytes(100, 11, 88, 1, 11)
            >= lib.ramp_ba_covariance_workspace_bytes(100, 11, 88, 1, 11))
    from rampvo_amd import evaluate, fastba, ops
    from rampvo_amd.Ramp_vo import Ramp_vo
    assert callable(fastba.map_covariance) and callable(ops.ba_map_covariance) and callable(Ramp_vo.map)
    assert callable(evaluate.save_map_ply)


def test_save_map_ply_round_trip(tmp_path):
    import torch
    from rampvo_amd import evaluate
    K = 5
    rng = np.random.default_rng(2)
    A = rng.normal(size=(K, 3, 3)).astype(np.float32)
    m = dict(points=torch.from_numpy(rng.normal(size=(K, 3)).astype(np.float32)),
             point_cov=torch.from_numpy(A @ A.transpose(0, 2, 1)),
             colors=torch.from_numpy(rng.integers(0, 255, (K, 3)).astype(np.uint8)))
    path = str(tmp_path / "map.ply")
    evaluate.save_map_ply(path, m, scale=2.0)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n")
    assert b"element vertex %d" % K in head and b"property float sigma" in head
    rec = np.frombuffer(body, np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3), ("sigma", "<f4")]))
    assert len(rec) == K and np.array_equal(rec["rgb"], m["colors"].numpy())
    assert np.allclose(rec["xyz"], 2.0 * m["points"].numpy(), rtol=1e-6)
    tr = np.trace(m["point_cov"].numpy(), axis1=1, axis2=2)
    assert np.allclose(rec["sigma"], 2.0 * np.sqrt(tr), rtol=1e-6)
    evaluate.save_map_ply(path, dict(points=m["points"][:0], point_cov=m["point_cov"][:0], colors=m["colors"][:0]))
    assert b"element vertex 0" in open(path, "rb").read()
