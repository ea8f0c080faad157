"""The map with its uncertainty on the GPU: ``fastba.map_covariance`` (include/ramp_hip.h ``ramp_ba_map_covariance``) against
the float64 restatement tests/mapref.py, ``ramp_map_select`` against its numpy statement exactly, and ``Ramp_vo.map()`` device
resident, host driven and against the operators.

Bounds (mapref.compare, the rule of covref.compare): per output, error against float64 <= max(1e-5, 4 x the float32
restatement's own error) for that case, and that envelope itself <= 5e-3.  point_cov: the largest entry difference per point
over that point's float64 trace, maximised over the points; pose_depth_cov: the largest difference norm over the largest
float64 norm of the case.  Float32 envelopes of the cases, measured on the CPU (point_cov / pose_depth_cov):

    n1      4.5e-7 / 6.2e-7      w10     7.2e-4 / 6.8e-4      w30     1.1e-3 / 1.2e-3
    w32     1.9e-4 / 2.2e-4      w10_m7  2.9e-3 / 3.1e-3      w10_t4  3.8e-6 / 1.4e-5

What each case is the smallest instance of:

    n1         n6 = 6; all but one source frame fixed, so rank-one covariances
    w10_t4     free and fixed source frames mixed; the block offset 6 (i - t0)
    w10_m7     Mu not a multiple of the waves per workgroup
    w10        n6 = 60
    w30        n6 = 180, lanes carrying three rows, the last partial
    w32        n6 = 192, the whole budget
    w10_gated  gated factors in n_obs

The measured error / bound ratios on MI355X are not recorded here yet: every case prints them.  n_obs is exact, ``point``
equals ``ramp_point_cloud``'s output bit for bit, and cov / depth_var / stats equal ``fastba.covariance``'s bit for bit.  Every
case prints its measured errors and the ratio to its bound before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import covref  # noqa: E402
import mapref  # noqa: E402
import trackerkit as kit  # noqa: E402
from oracle.make_golden_params import BA_PIN  # noqa: E402
from scenes import ba_pin_scene  # noqa: E402

pytestmark = pytest.mark.gpu

W32 = dict(seed=41, n_frames=33, M=4, lifetime=4)
CASES = {           # tag: (scene arguments, t0 as a function of the frame count) -- tests/test_ba_covariance_gpu.py's
    "n1": (BA_PIN["w10"], lambda n: n - 1),
    "w10_t4": (BA_PIN["w10"], lambda n: 4),
    "w10_m7": (dict(BA_PIN["w10"], M=7), lambda n: 1),
    "w10": (BA_PIN["w10"], lambda n: 1),
    "w30": (BA_PIN["w30"], lambda n: 1),
    "w32": (W32, lambda n: 1),
    "w10_gated": (BA_PIN["w10"], lambda n: 1),
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
        _cache[tag] = (s, t0, n, mapref.map_covariance(s, t0, n, np.float64), mapref.map_covariance(s, t0, n, np.float32))
    return _cache[tag]


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _args(s, t0, t1):
    return (_cu(s["poses"]), _cu(s["patches"]), _cu(s["intr"]), _cu(s["target"]), _cu(s["weight"]), _cu(s["lmbda"]),
            _cu(s["ii"]), _cu(s["jj"]), _cu(s["kk"]), t0, t1)


def _canaries(npat):
    return (torch.full((npat, 3), 7.5, device="cuda"), torch.full((npat, 6), -3.25, device="cuda"),
            torch.full((npat, 6), 11.0, device="cuda"), torch.full((npat,), -9, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("tag", list(CASES))
def test_map_covariance_against_float64(tag):
    from rampvo_amd import fastba, ops
    s, t0, t1, m64, m32 = _case(tag)
    args = _args(s, t0, t1)
    npat = s["patches"].shape[0]
    info = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    cov, dv, st, point, pcov, pdc, nobs = fastba.map_covariance(*args, M=s["M"], info=info, out=_canaries(npat))
    P, C, N = pcov.cpu().numpy(), pdc.cpu().numpy(), nobs.cpu().numpy()
    ok, rep = mapref.compare(P, C, m64, m32)
    print(tag, {k: "%.3g of %.3g (%.2f), envelope %.3g" % (v[0], v[1], v[0] / v[1], v[2]) for k, v in rep.items()})
    assert int(info.cpu()) == 0 and not st["failed"]
    assert ok, rep
    uk = m64["uk"]
    rest = np.setdiff1d(np.arange(npat), uk)
    assert np.array_equal(N[uk], m64["n_obs"][uk]), "n_obs"
    if tag == "w10_gated":
        assert N[uk].sum() == len(s["ii"]) - len(s["far"]) and (N[uk] < np.bincount(s["kk"], minlength=npat)[uk]).any()
    # a fixed source frame: zeros, and the rank-one form
    fixed = uk[(m64["src"] < t0) | (m64["src"] >= t1)]
    assert not C[fixed].any()
    if tag in ("n1", "w10_t4"):
        assert len(fixed) and len(fixed) < len(uk)
        S = P[fixed][:, [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(-1, 3, 3).astype(np.float64)
        ev = np.linalg.eigvalsh(S)
        # (nine float32 entries var (Jd_x Jd_y), two roundings each, none above the large eigenvalue: the perturbation
        # has Frobenius norm <= 3 x 2 x 2^-24 of it, 8 with the rounding of the eigenvalue itself)
        assert (np.abs(ev[:, :2]).max(1) <= 8 * 2.0 ** -24 * ev[:, 2]).all(), "not rank one"
    # patches without a factor keep the caller's values in all four outputs
    assert (point.cpu().numpy()[rest] == 7.5).all() and (P[rest] == -3.25).all() and (C[rest] == 11.0).all()
    assert (N[rest] == -9).all()
    # the point is ramp_point_cloud's, bit for bit (every intrinsics row is equal in these scenes)
    assert (s["intr"].reshape(-1, 4) == s["intr"].reshape(-1, 4)[0]).all()
    ix = np.zeros(npat, np.int64)
    ix[uk] = m64["src"]
    pts = ops.point_cloud(args[0], args[1], args[2], _cu(ix)).cpu().numpy()
    assert np.array_equal(point.cpu().numpy()[uk], pts[uk]), "point differs from ramp_point_cloud"
    assert np.isfinite(pts[uk]).all()
    assert np.abs(pts[uk] - m64["point"][uk]).max() <= 1e-5 * np.abs(m64["point"][uk]).max()
    # the covariance's own outputs are the same bits with and without the map
    cov0, dv0, st0 = fastba.covariance(*args, M=s["M"])
    assert torch.equal(cov, cov0) and torch.equal(dv, dv0) and st == st0
    # determinism, default fill, inputs only read
    out2 = fastba.map_covariance(*args, M=s["M"])
    assert torch.equal(out2[4][_cu(uk)], pcov[_cu(uk)]) and torch.equal(out2[5][_cu(uk)], pdc[_cu(uk)])
    assert torch.equal(out2[3][_cu(uk)], point[_cu(uk)]) and torch.equal(out2[0], cov) and torch.equal(out2[1], dv)
    if len(rest):
        assert torch.isnan(out2[4][_cu(rest)]).all() and not out2[6][_cu(rest)].any()
    assert np.array_equal(args[0].cpu().numpy(), s["poses"]) and np.array_equal(args[1].cpu().numpy(), s["patches"])


def test_patches_without_a_factor_keep_the_callers_values():
    """every fifth patch loses all its factors: canaries in all four outputs there, results everywhere else"""
    from rampvo_amd import fastba
    s, t0, t1, _, _ = _case("w10_t4")
    keep = s["kk"] % 5 != 0
    s = dict(s, **{k: s[k][keep] for k in ("ii", "jj", "kk", "target", "weight")})
    npat = s["patches"].shape[0]
    m64 = mapref.map_covariance(s, t0, t1, np.float64)
    cov, dv, st, point, pcov, pdc, nobs = fastba.map_covariance(*_args(s, t0, t1), M=s["M"], out=_canaries(npat))
    rest, uk = np.arange(0, npat, 5), m64["uk"]
    assert len(uk) == npat - len(rest) and st["Mu"] == len(uk)
    assert (point.cpu().numpy()[rest] == 7.5).all() and (pcov.cpu().numpy()[rest] == -3.25).all()
    assert (pdc.cpu().numpy()[rest] == 11.0).all() and (nobs.cpu().numpy()[rest] == -9).all()
    assert np.isinf(dv.cpu().numpy()[rest]).all()
    ok, rep = mapref.compare(pcov.cpu().numpy(), pdc.cpu().numpy(), m64, mapref.map_covariance(s, t0, t1, np.float32))
    assert ok, rep
    assert np.array_equal(nobs.cpu().numpy()[uk], m64["n_obs"][uk])


def test_no_free_pose_gives_rank_one_covariances_and_zero_cross_terms():
    """t1 == t0: every covariance is Q_k J_d J_d' and every pose_depth_cov entry is zero"""
    from rampvo_amd import fastba
    s, _, n, _, _ = _case("w10")
    m64 = mapref.map_covariance(s, n, n, np.float64)
    cov, dv, st, point, pcov, pdc, nobs = fastba.map_covariance(*_args(s, n, n), M=s["M"])
    uk = m64["uk"]
    P, C = pcov.cpu().numpy()[uk], pdc.cpu().numpy()[uk]
    assert cov.shape == (0, 0) and st["N"] == 0 and not st["failed"]
    assert not C.any()
    Q = m64["cov"]["Q"]
    assert np.abs(m64["cov"]["depth_var"][uk] - Q).max() == 0          # (the restatement: depth_var = Q_k there)
    tr = m64["point_cov"][uk][:, [0, 3, 5]].sum(1)
    err = (np.abs(P - m64["point_cov"][uk]).max(1) / tr).max()
    print("t1 == t0: point_cov %.3g of 1e-5" % err)
    assert err <= 1e-5
    assert np.array_equal(nobs.cpu().numpy(), m64["n_obs"])


def test_a_system_that_is_not_finite_gives_nan_covariances_and_finite_points():
    """the covariance test's non-finite scene (one infinite confidence weight): NaN point_cov / pose_depth_cov, bit 0 of
    info, point still finite"""
    from rampvo_amd import fastba
    s, t0, t1, m64, _ = _case("w10")
    s = dict(s, weight=s["weight"].copy())
    s["weight"][3, 0] = np.inf
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    cov, dv, st, point, pcov, pdc, nobs = fastba.map_covariance(*_args(s, t0, t1), M=s["M"], info=info)
    uk = _cu(m64["uk"])
    assert int(info.cpu()) & 1 and st["failed"]
    assert torch.isnan(pcov[uk]).all() and torch.isnan(pdc[uk]).all() and torch.isnan(cov).all()
    assert torch.isfinite(point[uk]).all()
    p64 = m64["point"][m64["uk"]]
    assert np.abs(point.cpu().numpy()[m64["uk"]] - p64).max() <= 1e-5 * np.abs(p64).max()
    assert np.array_equal(nobs.cpu().numpy(), m64["n_obs"])


# ------------------------------------------------------------------------------------------------------- ramp_map_select
def _select_inputs(n, seed):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, 3, 3)).astype(np.float32)
    S = A @ A.transpose(0, 2, 1) * np.float32(0.01)
    pc = np.stack([S[:, x, y] for x, y in mapref.SYM], 1).astype(np.float32)
    dv = (rng.uniform(0.001, 0.1, n) ** 2).astype(np.float32)
    patches = rng.uniform(0.2, 2.0, (n, 3, 3, 3)).astype(np.float32)
    n_obs = rng.integers(0, 6, n).astype(np.int32)
    return pc, dv, patches, n_obs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_map_select_equals_numpy_exactly(n):
    from rampvo_amd import ops
    pc, dv, patches, n_obs = _select_inputs(n, 100 + n)
    d = patches[:, 2, 1, 1]
    sig = np.sqrt((pc[:, 0] + pc[:, 3]) + pc[:, 5])
    rel = np.sqrt(dv) / d
    e = n // 2
    variants = {
        "everything": (pc, dv, patches, n_obs, dict()),
        "nothing": (pc, dv, patches, n_obs, dict(max_sigma=0.0)),
        "sigma alone": (pc, dv, patches, n_obs, dict(max_sigma=float(np.median(sig)))),
        "depth alone": (pc, dv, patches, n_obs, dict(max_rel_depth_sigma=float(np.median(rel)))),
        "obs alone": (pc, dv, patches, n_obs, dict(min_obs=3)),
        "all three": (pc, dv, patches, n_obs, dict(max_sigma=float(np.quantile(sig, 0.8)), min_obs=2,
                                                   max_rel_depth_sigma=float(np.quantile(rel, 0.8)))),
        "equal to the sigma threshold": (pc, dv, patches, n_obs, dict(max_sigma=float(sig[e]))),
        "equal to the depth threshold": (pc, dv, patches, n_obs, dict(max_rel_depth_sigma=float(rel[e]))),
    }
    bad = pc.copy()                                                     # NaN / inf rows and a zero depth
    bad[::3, 4] = np.nan
    bad[1::5, 0] = np.inf
    zp = patches.copy()
    zp[e, 2, 1, 1] = 0.0
    variants["nan rows"] = (bad, dv, patches, n_obs, dict())
    variants["nan rows and a zero depth"] = (bad, dv, zp, n_obs, dict(max_rel_depth_sigma=1e30, max_sigma=float(np.median(sig))))
    for name, (a, b, c, o, kw) in variants.items():
        ref = mapref.select(a, b, c[:, 2, 1, 1], o, **kw)
        index, count = ops.map_select(_cu(a), _cu(b), _cu(c), _cu(o), **kw)
        K, idx = int(count.cpu()), index.cpu().numpy()
        assert K == len(ref), (name, K, len(ref))
        assert np.array_equal(idx[:K], ref), name
        assert (idx[K:] == -1).all(), name + ": written behind the count"
    assert len(mapref.select(pc, dv, d, n_obs)) == n and len(mapref.select(pc, dv, d, n_obs, max_sigma=0.0)) == 0
    assert e in mapref.select(pc, dv, d, n_obs, max_sigma=float(sig[e]))
    # the device-side clip of n
    rows = torch.tensor([n // 4], dtype=torch.int32, device="cuda")
    index, count = ops.map_select(_cu(pc), _cu(dv), _cu(patches), _cu(n_obs), dyn_rows=rows, per_row=2)
    assert int(count.cpu()) == min(n, 2 * (n // 4)) and (index.cpu().numpy()[int(count.cpu()):] == -1).all()


# ----------------------------------------------------------------------------------------------------------- tracker
T_FRAMES = 30


TENSORS = ("index", "frame", "points", "point_cov", "colors", "depth_sigma_rel", "n_obs")
SCALARS = ("n_total", "chi2", "dof", "sigma0_sq", "failed")


def _snap(m):
    return dict({k: m[k].cpu().numpy().copy() for k in TENSORS}, **{k: m[k] for k in SCALARS})


@torch.no_grad()
def _tracked(device_steps, query):
    key = ("trk", device_steps, query)
    if key not in _cache:
        slam = kit.tracker(device_steps, device_steps, **kit.COV_TRACKER)
        out = dict(dicts={}, resident={}, first_error=None)
        try:
            slam.map()
        except RuntimeError as e:
            out["first_error"] = str(e)
        for t, (im, ev, K, mask) in enumerate(kit.frames(*kit.COV_STREAM)):
            slam(float(t), input_tensor=(ev, im, mask), intrinsics=K)
            res = slam._dev is not None and slam._dev.active
            out["resident"][t] = bool(res)
            if query and t >= 1:
                try:
                    out["dicts"][t] = _snap(slam.map())
                except RuntimeError as e:          # (before the first update)
                    out["dicts"][t] = str(e)
                assert (slam._dev is not None and slam._dev.active) == res, "map() handed the state back"
        if query:
            out["empty"] = _snap(slam.map(max_sigma=0))
            out["loose"] = _snap(slam.map(min_obs=0))
        out["settles"] = slam.stats["settles"]
        out["device_frames"] = slam.stats["device_frames"]
        if query and device_steps:
            # the last dict against the operators on the tracker's own state, handed back afterwards
            slam.settle()
            from rampvo_amd import fastba, ops
            from rampvo_amd import projective_ops as pops
            n, W, M = slam.n, int(slam.cfg.OPTIMIZATION_WINDOW), slam.M
            rows = torch.from_numpy(np.asarray(slam._net_rows())).cuda()
            o = fastba.map_covariance(slam.poses_, slam.patches_, slam.intrinsics_, slam.last_target[0][rows],
                                      slam.last_weight[0][rows], slam.lmbda, slam.ii, slam.jj, slam.kk, max(n - W, 1), n)
            index, count = ops.map_select(o[4], o[1], slam.patches_, o[6], min_obs=2, n=n * M)
            K = int(count.cpu())
            idx = index[:K].long()
            ixm = torch.arange(n * M, device="cuda") // M
            pts = pops.point_cloud(slam.poses_, slam.patches_.view(-1, 3, 3, 3)[:n * M], slam.intrinsics_, ixm)
            out["operator"] = dict(index=idx.cpu().numpy(), points=pts[idx].cpu().numpy(), point_cov=o[4][idx].cpu().numpy(),
                                   n_obs=o[6][idx].cpu().numpy(), colors=slam.colors_.view(-1, 3)[idx].cpu().numpy(),
                                   stats=o[2])
        traj, _ = slam.terminate()
        out["traj"], out["patches"] = traj, slam.patches_[:slam.n].cpu().numpy()
        del slam
        kit.quiesce()
        _cache[key] = out
    return _cache[key]


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in TENSORS) and all(a[k] == b[k] for k in SCALARS)


def test_a_tracker_queried_with_map_tracks_the_same_bits_and_stays_resident():
    a, b = _tracked(True, True), _tracked(True, False)
    assert a["first_error"] and "no update has run yet" in a["first_error"]
    assert sum(a["resident"].values()) > 10 and a["settles"] == 0 and a["resident"] == b["resident"]
    assert a["device_frames"] == b["device_frames"] > 10
    assert np.array_equal(a["traj"], b["traj"]) and np.array_equal(a["patches"], b["patches"])
    d = a["dicts"][T_FRAMES - 1]
    K = len(d["index"])
    assert 0 < K <= d["n_total"] and (np.diff(d["index"]) > 0).all() and np.array_equal(d["frame"], d["index"] // 16)
    assert d["points"].shape == (K, 3) and d["point_cov"].shape == (K, 3, 3) and d["colors"].shape == (K, 3)
    assert np.isfinite(d["points"]).all() and np.isfinite(d["point_cov"]).all() and (d["n_obs"] >= 2).all()
    assert np.array_equal(d["point_cov"], d["point_cov"].transpose(0, 2, 1))
    assert (np.linalg.eigvalsh(d["point_cov"].astype(np.float64))[:, 2] > 0).all() and (d["depth_sigma_rel"] > 0).all()
    assert d["sigma0_sq"] == d["chi2"] / max(d["dof"], 1) and not d["failed"]
    lo = a["loose"]
    assert len(lo["index"]) >= K and set(d["index"]) <= set(lo["index"])


def test_resident_and_host_driven_map_agree_bit_for_bit():
    a, c = _tracked(True, True), _tracked(False, True)
    assert c["device_frames"] == 0
    both = [t for t in a["dicts"] if isinstance(a["dicts"][t], dict) and isinstance(c["dicts"][t], dict)]
    res = [t for t in both if a["resident"][t]]
    assert len(res) > 10, (len(both), len(res))
    bad = [t for t in both if not _same(a["dicts"][t], c["dicts"][t])]
    assert not bad, bad


def test_the_dict_equals_the_operators_on_the_state_handed_back():
    a = _tracked(True, True)
    d, o = a["dicts"][T_FRAMES - 1], a["operator"]
    assert a["resident"][T_FRAMES - 1]
    assert np.array_equal(d["index"], o["index"]) and np.array_equal(d["points"], o["points"])
    assert np.array_equal(d["point_cov"].reshape(-1, 9)[:, [0, 1, 2, 4, 5, 8]], o["point_cov"])
    assert np.array_equal(d["n_obs"], o["n_obs"]) and np.array_equal(d["colors"], o["colors"])
    assert d["chi2"] == o["stats"]["chi2"] and d["n_total"] == o["stats"]["Mu"]


def test_max_sigma_zero_selects_nothing_with_well_formed_tensors():
    for dev in (True, False):
        e = _tracked(dev, True)["empty"]
        assert e["index"].shape == (0,) and e["frame"].shape == (0,) and e["points"].shape == (0, 3)
        assert e["point_cov"].shape == (0, 3, 3) and e["colors"].shape == (0, 3) and e["colors"].dtype == np.uint8
        assert e["depth_sigma_rel"].shape == (0,) and e["n_obs"].shape == (0,) and e["n_total"] > 0
