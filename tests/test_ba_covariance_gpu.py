"""Uncertainty of the window on the GPU: ``fastba.covariance`` (include/ramp_hip.h ``ramp_ba_covariance``) against the float64
restatement tests/covref.py, and ``Ramp_vo.uncertainty()`` device resident, host driven and against the operator.

Bounds (covref.compare): per output, error against float64 <= max(floor, 4 x the float32 restatement's own error) for that
case, and that envelope itself <= 5e-3.  cov is relative to its largest diagonal entry, the cov diagonal and depth_var per
entry.  floor = 1e-5 (covref.compare's docstring).  Float32 envelopes of the cases, measured on the CPU (cov / diagonal /
depth_var; cond(S)):

    n1      5.0e-7 / 9.3e-7 / 2.8e-7   (38)        w10     6.4e-4 / 6.4e-4 / 7.3e-4   (6.2e4)
    w10_t4  1.4e-5 / 1.4e-5 / 5.5e-6   (625)       w10_m7  3.1e-3 / 3.1e-3 / 3.0e-3   (5.8e4)
    w30     1.2e-3 / 1.3e-3 / 1.1e-3   (7.5e4)     w32     3.0e-4 / 3.8e-4 / 2.0e-4   (6.8e4; 33 frames, M = 4, seed 41)

Worst measured error / bound per case on MI355X: n1 0.35 (the floor decides: 3.5e-6 against 4 x 9.3e-7), w10 0.13, w30 0.18,
w32 0.16, w10_m7 0.10, w10_t4 0.37, w10_gated 0.60; chi2 at most 8e-7 from float64.

chi2 is held to E 2^-23 relative (the ordered-sum bound for positive terms), n_valid and Mu exactly.  Every case prints its
measured errors and the ratio to its bound before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import covref  # noqa: E402
import trackerkit as kit  # noqa: E402
from oracle.make_golden_params import BA_PIN  # noqa: E402
from scenes import ba_pin_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W32 = dict(seed=41, n_frames=33, M=4, lifetime=4)
CASES = {           # tag: (scene arguments, t0 as a function of the frame count)
    "n1": (BA_PIN["w10"], lambda n: n - 1),          # n6 = 6
    "w10": (BA_PIN["w10"], lambda n: 1),             # n6 = 60
    "w30": (BA_PIN["w30"], lambda n: 1),             # n6 = 180: LDS above 64 KB
    "w32": (W32, lambda n: 1),                       # n6 = 192: the whole LDS budget
    "w10_m7": (dict(BA_PIN["w10"], M=7), lambda n: 1),   # Mu no multiple of the waves per workgroup
    "w10_t4": (BA_PIN["w10"], lambda n: 4),          # source poses in front of t0 are fixed
    "w10_gated": (BA_PIN["w10"], lambda n: 1),       # 5 % of the targets 200 px away
}
_cache = {}


def _f32(s):
    return {k: (v.astype(np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v) for k, v in s.items()}


def scene(tag):
    """the scene rounded to float32 (what the GPU gets) and its window (t0, t1)"""
    kw, t0f = CASES[tag]
    s = _f32(ba_pin_scene(**kw))
    if tag == "w10_gated":
        rng = np.random.default_rng(5)
        far = rng.choice(len(s["ii"]), size=len(s["ii"]) // 20, replace=False)
        s["target"] = s["target"].copy()
        s["target"][far] += np.float32(200.0)
        s["far"] = far
    n = s["n_frames"]
    return s, t0f(n), n


def _case(tag):
    """scene(tag), its float64 result and its float32 envelope -- computed once"""
    if tag not in _cache:
        s, t0, n = scene(tag)
        _cache[tag] = (s, t0, n, covref.covariance(s, t0, n, np.float64), covref.covariance(s, t0, n, np.float32))
    return _cache[tag]


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run(s, t0, t1, info=None):
    from rampvo_amd import fastba
    poses, patches = _cu(s["poses"]), _cu(s["patches"])
    args = (poses, patches, _cu(s["intr"]), _cu(s["target"]), _cu(s["weight"]), _cu(s["lmbda"]), _cu(s["ii"]), _cu(s["jj"]),
            _cu(s["kk"]), t0, t1)
    cov, dv, st = fastba.covariance(*args, M=s["M"], info=info)
    return cov, dv, st, poses, patches, args


@pytest.mark.parametrize("tag", list(CASES))
def test_covariance_against_float64(tag):
    s, t0, t1, r64, r32 = _case(tag)
    info = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    cov, dv, st, poses, patches, args = _run(s, t0, t1, info)
    c, d = cov.cpu().numpy(), dv.cpu().numpy()
    ok, rep = covref.compare(c, d, r64, r32)
    chi_rel = abs(st["chi2"] - r64["chi2"]) / r64["chi2"]
    chi_bound = len(s["ii"]) * 2.0 ** -23
    print(tag, {k: "%.3g of %.3g (%.2f), envelope %.3g" % (v[0], v[1], v[0] / v[1], v[2]) for k, v in rep.items()},
          "chi2 %.3g of %.3g" % (chi_rel, chi_bound))
    assert int(info.cpu()) == 0 and not st["failed"]
    assert c.shape == (6 * (t1 - t0),) * 2 and d.shape == (s["patches"].shape[0],)
    assert ok, rep
    assert chi_rel <= chi_bound, (chi_rel, chi_bound)
    assert st["n_valid"] == r64["n_valid"] and st["Mu"] == r64["Mu"] and st["N"] == t1 - t0 and st["t0"] == t0
    if tag == "w10_gated":
        assert r64["n_valid"] == len(s["ii"]) - len(s["far"])           # the gate dropped exactly the moved targets
    assert np.array_equal(c, c.T), "cov is not symmetric bit for bit"
    written = np.isfinite(r64["depth_var"])
    q32 = np.full(d.shape, np.inf, np.float32)
    q32[r64["uk"]] = r32["Q"]
    assert (d[written] > 0).all() and (d[written] >= q32[written] * (1 - 2.0 ** -20)).all()   # (Q_k itself: a few ulp of C)
    assert np.isinf(d[~written]).all()
    # the inputs are only read; a second call gives the same bits
    assert np.array_equal(poses.cpu().numpy(), s["poses"]) and np.array_equal(patches.cpu().numpy(), s["patches"])
    from rampvo_amd import fastba
    cov2, dv2, st2 = fastba.covariance(*args, M=s["M"])
    assert torch.equal(cov, cov2) and torch.equal(dv, dv2) and st2 == st


def test_no_free_pose():
    s, _, n, _, _ = _case("w10")
    r64 = covref.covariance(s, n, n, np.float64)
    cov, dv, st, *_ = _run(s, n, n)
    d = dv.cpu().numpy()
    fin = np.isfinite(r64["depth_var"])
    assert cov.shape == (0, 0) and st["N"] == 0 and not st["failed"]
    assert np.abs(d[fin] / r64["depth_var"][fin] - 1).max() <= 1e-5 and np.isinf(d[~fin]).all()
    assert st["n_valid"] == r64["n_valid"] and abs(st["chi2"] / r64["chi2"] - 1) <= len(s["ii"]) * 2.0 ** -23


def test_every_factor_gated_gives_the_identity():
    """S = I: cov = I exactly, depth_var = 1 / lambda (to the division's rounding)"""
    s, t0, t1, _, _ = _case("w10")
    s = dict(s, target=s["target"] + np.float32(200.0))
    cov, dv, st, *_ = _run(s, t0, t1)
    d = dv.cpu().numpy()
    assert st["n_valid"] == 0 and st["chi2"] == 0.0 and not st["failed"]
    assert torch.equal(cov.cpu(), torch.eye(6 * (t1 - t0)))
    w = np.isfinite(d)
    assert w.sum() == st["Mu"] and np.abs(d[w] * np.float32(s["lmbda"][0]) - 1).max() <= 2.0 ** -22


def test_a_system_that_is_not_finite_gives_nan_and_the_info_bit():
    """one infinite confidence weight: an arithmetic outcome (no fault) -- NaN everywhere the call writes, bit 0, status OK"""
    s, t0, t1, r64, _ = _case("w10")
    s = dict(s, weight=s["weight"].copy())
    s["weight"][3, 0] = np.inf
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cov, dv, st, *_ = _run(s, t0, t1, info)
    d = dv.cpu().numpy()
    assert int(info.cpu()) & 1 and st["failed"]
    assert torch.isnan(cov).all()
    written = np.isfinite(r64["depth_var"])
    assert np.isnan(d[written]).all() and np.isinf(d[~written]).all()


# ----------------------------------------------------------------------------------------------------------- tracker
T_FRAMES = 30


def _snap(u):
    return dict(frames=list(u["frames"]), cov=u["cov"].cpu().numpy().copy(), depth_var=u["depth_var"].cpu().numpy().copy(),
                pose_cov=u["pose_cov"].cpu().numpy().copy(), chi2=u["chi2"], n_valid=u["n_valid"], dof=u["dof"],
                sigma0_sq=u["sigma0_sq"])


@torch.no_grad()
def _tracked(device_steps, query):
    key = ("trk", device_steps, query)
    if key not in _cache:
        slam = kit.tracker(device_steps, device_steps, **kit.COV_TRACKER)
        out = dict(dicts={}, resident={}, first_error=None)
        try:
            slam.uncertainty()
        except RuntimeError as e:
            out["first_error"] = str(e)
        for t, (im, ev, K, mask) in enumerate(kit.frames(*kit.COV_STREAM)):
            slam(float(t), input_tensor=(ev, im, mask), intrinsics=K)
            res = slam._dev is not None and slam._dev.active
            out["resident"][t] = bool(res)
            if query and t >= 1:
                try:
                    out["dicts"][t] = _snap(slam.uncertainty())
                except RuntimeError as e:          # (before the first update)
                    out["dicts"][t] = str(e)
                assert (slam._dev is not None and slam._dev.active) == res, "uncertainty() handed the state back"
        out["settles"] = slam.stats["settles"]
        out["device_frames"] = slam.stats["device_frames"]
        if query and device_steps:
            # the last dict against the operator on the tracker's own state, handed back afterwards
            slam.settle()
            from rampvo_amd import fastba
            n, W = slam.n, int(slam.cfg.OPTIMIZATION_WINDOW)
            rows = torch.from_numpy(np.asarray(slam._net_rows())).cuda()
            cov, dv, st = fastba.covariance(slam.poses_, slam.patches_, slam.intrinsics_, slam.last_target[0][rows],
                                            slam.last_weight[0][rows], slam.lmbda, slam.ii, slam.jj, slam.kk, max(n - W, 1), n)
            out["operator"] = dict(cov=cov.cpu().numpy(), depth_var=dv.cpu().numpy()[:n * slam.M].reshape(n, slam.M), stats=st,
                                   frames=list(range(max(n - W, 1), n)))
        traj, _ = slam.terminate()
        out["traj"], out["patches"] = traj, slam.patches_[:slam.n].cpu().numpy()
        del slam
        kit.quiesce()
        _cache[key] = out
    return _cache[key]


def _same(a, b):
    return (a["frames"] == b["frames"] and np.array_equal(a["cov"], b["cov"], equal_nan=True)
            and np.array_equal(a["depth_var"], b["depth_var"], equal_nan=True) and a["chi2"] == b["chi2"]
            and a["n_valid"] == b["n_valid"] and a["dof"] == b["dof"])


def test_a_queried_tracker_tracks_the_same_bits_and_stays_resident():
    a, b = _tracked(True, True), _tracked(True, False)
    assert a["first_error"] and "no update has run yet" in a["first_error"]
    assert sum(a["resident"].values()) > 10 and a["settles"] == 0 and a["resident"] == b["resident"]
    assert a["device_frames"] == b["device_frames"] > 10
    assert np.array_equal(a["traj"], b["traj"]) and np.array_equal(a["patches"], b["patches"])
    d = a["dicts"][T_FRAMES - 1]
    N = len(d["frames"])
    assert d["cov"].shape == (6 * N, 6 * N) and d["pose_cov"].shape == (N, 6, 6) and np.isfinite(d["cov"]).all()
    assert np.array_equal(d["cov"], d["cov"].T) and (np.diagonal(d["cov"]) > 0).all()
    assert np.array_equal(d["pose_cov"][N - 1], d["cov"][6 * N - 6:, 6 * N - 6:])
    assert d["sigma0_sq"] == d["chi2"] / max(d["dof"], 1) and d["n_valid"] > 0


def test_resident_and_host_driven_uncertainty_agree_bit_for_bit():
    a, c = _tracked(True, True), _tracked(False, True)
    assert c["device_frames"] == 0
    both = [t for t in a["dicts"] if isinstance(a["dicts"][t], dict) and isinstance(c["dicts"][t], dict)]
    res = [t for t in both if a["resident"][t]]
    assert len(res) > 10, (len(both), len(res))
    bad = [t for t in both if not _same(a["dicts"][t], c["dicts"][t])]
    assert not bad, bad


def test_the_dict_equals_the_operator_on_the_state_handed_back():
    a = _tracked(True, True)
    d, o = a["dicts"][T_FRAMES - 1], a["operator"]
    assert a["resident"][T_FRAMES - 1]
    assert d["frames"] == o["frames"] and np.array_equal(d["cov"], o["cov"])
    assert np.array_equal(d["depth_var"], o["depth_var"])
    assert d["chi2"] == o["stats"]["chi2"] and d["n_valid"] == o["stats"]["n_valid"]
