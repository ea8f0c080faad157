"""The inverse-depth map on the GPU: ``ramp_invdepth_map`` (csrc/depthmap.hip) through ``ops.invdepth_map``,
``Ramp_vo.invdepth_map`` and ``Ramp_vo.compensate_events(invdepth="map")``.

Records are compared per point with the float64 restatement (tests/depthref.py ``compare_records``): the bound is
``georef.bound(PIXEL_FLOOR x largest |coordinate|, env)`` with env = the float32 restatement's own error against float64.
Maps are compared with the float64 regression of the call's OWN records (``compare_map``: floor 1e-5 x the largest d').
Shapes: 120 x 160 and 37 x 53 (no tile and no vector width divides it); projections from ``georef.geo_scene``, regressions
from points drawn uniformly over the reach box and seen from their own camera.

The tracker tests run the small synthetic tracker of tests/trackerkit.py."""
import numpy as np
import pytest
import torch

import depthref
import georef
import oracle as orc
import trackerkit as kit
from guarded import Flat
from trackerkit import RADIUS, cu

pytestmark = pytest.mark.gpu

SHAPES = ((120, 160), (37, 53))
K4 = np.array([30.0, 20.0, 19.5, 11.25], np.float32)
IDENT = np.array([0, 0, 0, 0, 0, 0, 1], np.float32)
PRIOR, PW = 0.4, 0.7
_cache = {}


def _np(r):
    return {k: v.cpu().numpy() for k, v in r.items()}


def _stage():
    from rampvo_amd import _lib
    return _lib.lib().ramp_invdepth_map_stage_records()


def _status_ok(st, K=None):
    assert st[2] + st[3] + st[4] + st[5] == st[1] and st[7] == 0, st
    assert K is None or st[1] == K, st


def _points(seed, K, H, W, R):
    """K points uniform over the reach box, each seen from its own camera (identity poses, M = 1): u = x, v = y, d' = d up to
    the rounding of the unproject / project round trip"""
    rng = np.random.default_rng(seed)
    p = np.zeros((K, 3, 3, 3), np.float32)
    p[:, 0] = rng.uniform(-R, W - 1 + R, (K, 1, 1))
    p[:, 1] = rng.uniform(-R, H - 1 + R, (K, 1, 1))
    p[:, 2] = np.exp(rng.uniform(np.log(0.05), np.log(1.2), (K, 1, 1)))
    return np.repeat(IDENT[None], K, 0), p, rng.uniform(0.5, 2.0, K).astype(np.float32)


def _regress(poses, patches, conf, H, W, R, prior=PRIOR, pw=PW, **kw):
    from rampvo_amd import ops
    return _np(ops.invdepth_map(cu(poses), cu(patches), cu(K4), cu(IDENT), H, W, R, conf=None if conf is None else cu(conf),
                                prior=prior, prior_weight=pw, want_records=True, **kw))


def _geo():
    if "geo" not in _cache:
        s = georef.geo_scene(11)
        cam = orc.se3_inv_f64(s["poses"][5:6].astype(np.float64))[0].astype(np.float32)
        cam[:3] += np.float32([0.05, -0.03, 0.1])
        rng = np.random.default_rng(12)
        var = np.exp(rng.uniform(-6, 0, s["n_frames"] * s["M"])).astype(np.float32)
        _cache["geo"] = (s, cam, var)
    return _cache["geo"]


def _geo_call(H, W, R, scale, **kw):
    from rampvo_amd import ops
    s, cam, var = _geo()
    kw.setdefault("conf", cu(var))
    kw.setdefault("conf_is_variance", True)
    return _np(ops.invdepth_map(cu(s["poses"]), cu(s["patches"]), cu(s["intr"][0]), cu(cam), H, W, R, scale=scale, prior=PRIOR,
                                prior_weight=PW, want_records=True, **kw))


# ------------------------------------------------------------------------------------------------ 1. records, per point
def test_records_against_float64():
    """every patch of geo_scene projected into a camera between two frames: (measured, envelope, bound) printed per case"""
    s, cam, var = _geo()
    ids = np.arange(s["n_frames"] * s["M"])
    tab = georef.Table("invdepth_map: records against float64 (u, v in pixels; d' in inverse depth)")
    ok = True
    for (H, W), R in ((SHAPES[0], 12.0), (SHAPES[1], 1.5), (SHAPES[1], 400.0)):
        scale = W / 160.0
        r = _geo_call(H, W, R, scale)
        c = depthref.compare_records(r["records"], s["poses"], s["patches"], s["intr"][0], cam, ids, s["M"], H, W, R, scale,
                                     conf=var, conf_is_variance=True)
        for name in ("uv", "d", "c"):
            ok &= tab.add("%dx%d R=%g %s" % (H, W, R, name), c[name]["err"], c[name]["env"], c[name]["floor"])
        ok &= c["sets_ok"]
        _status_ok(r["status"], len(ids))
        assert r["status"][0] == 0 and r["status"][5] == (r["records"][:, 3] > 0).sum() and c["n_live"] >= 32
        cls = depthref.project(s["poses"], s["patches"], s["intr"][0], cam, ids, s["M"], H, W, R, scale, conf=var,
                               conf_is_variance=True)[1]
        assert r["status"][2] == (cls == 2).sum() and abs(int(r["status"][3]) - int((cls == 3).sum())) <= 2
    tab.show()
    assert ok and not tab.failed(), tab.failed()


# ------------------------------------------------------------------------------------------------ 2. the map, pw > 0
def _map_cases():
    cases = []
    for hw in SHAPES:
        cases += [(hw, K, 12.0) for K in (0, 1, 63, 64, 65, 257, "stage+37")]
        cases += [(hw, K, R) for K in (257, "stage+37") for R in (1.5, 400.0)]
    return cases


@pytest.mark.parametrize("hw,K,R", _map_cases())
def test_map_with_a_prior(hw, K, R):
    (H, W), K = hw, _stage() + 37 if K == "stage+37" else K
    poses, patches, conf = _points(K, K, H, W, R)
    r = _regress(poses, patches, conf, H, W, R)
    c = depthref.compare_map(r["invdepth"], r["weight"], r["records"], PRIOR, PW, R, H, W)
    for name in ("invdepth", "weight"):
        print("%dx%d K=%d R=%g %-8s err %.2e env %.2e bound %.2e" % (H, W, K, R, name, c[name]["err"], c[name]["env"],
                                                                     c[name]["bound"]))
    assert c["ok"], c
    _status_ok(r["status"], K)
    assert r["status"][0] == 0 and r["status"][6] == (r["weight"] == 0).sum() and np.isfinite(r["invdepth"]).all()
    assert r["records"].shape == (K, 4) and r["status"][5] == (r["records"][:, 3] > 0).sum()
    if K == 0:
        assert (r["invdepth"] == np.float32(PRIOR)).all() and not r["weight"].any()


# ------------------------------------------------------------------------------------------------ 3. the map, pw = 0
@pytest.mark.parametrize("hw,K,R", [(SHAPES[0], 64, 12.0), (SHAPES[0], 257, 12.0), (SHAPES[1], 257, 1.5), (SHAPES[1], 64, 400.0)])
def test_map_without_a_prior(hw, K, R):
    """no prior: a pixel inside a disc is finite, a pixel outside every disc is NaN with weight 0; pixels whose largest s_k
    (float64, the call's own records) lies within 1e-4 of 0 are left out"""
    H, W = hw
    poses, patches, conf = _points(100 + K, K, H, W, R)
    r = _regress(poses, patches, conf, H, W, R, prior=None, pw=0.0)
    smax = depthref.regress(r["records"], 0.0, 0.0, R, H, W)["smax"]
    inside, outside = smax > 1e-4, smax < -1e-4
    left_out = 1.0 - (inside | outside).mean()
    print("%dx%d K=%d R=%g: %.3f %% of the pixels left out" % (H, W, K, R, 100 * left_out))
    assert left_out <= 0.01
    assert np.isfinite(r["invdepth"][inside]).all() and (r["weight"][inside] > 0).all()
    assert np.isnan(r["invdepth"][outside]).all() and not r["weight"][outside].any()
    assert np.array_equal(np.isnan(r["invdepth"]), r["weight"] == 0) and r["status"][6] == np.isnan(r["invdepth"]).sum()
    live = r["records"][:, 3] > 0
    d = r["records"][live, 2]
    fin = np.isfinite(r["invdepth"])
    assert r["invdepth"][fin].min() >= d.min() * (1 - 1e-5) and r["invdepth"][fin].max() <= d.max() * (1 + 1e-5)
    _status_ok(r["status"], K)
    # an empty selection on a non-zero capacity: NaN everywhere, weight 0
    from rampvo_amd import ops
    e = _np(ops.invdepth_map(cu(poses), cu(patches), cu(K4), cu(IDENT), H, W, R, index=cu(np.arange(K, dtype=np.int32)),
                             count=torch.zeros(1, dtype=torch.int32, device="cuda")))
    assert np.isnan(e["invdepth"]).all() and not e["weight"].any() and e["status"].tolist() == [0, 0, 0, 0, 0, 0, H * W, 0]


# ------------------------------------------------------------------------------------------------ 4. repeatability
@pytest.mark.parametrize("hw", SHAPES)
def test_bits_repeat_and_ignore_what_reaches_no_pixel(hw):
    H, W = hw
    R, K = 12.0, _stage() + 37
    poses, patches, conf = _points(7, K, H, W, R)
    a = _regress(poses, patches, conf, H, W, R)
    b = _regress(poses, patches, conf, H, W, R)
    for k in ("invdepth", "weight", "records", "status"):
        assert georef.same_bits(a[k], b[k]), k
    # records out of reach (counted in [4]) and records in the corners of the reach box, farther than R from every pixel
    # (contributing by the count, w = 0 at every pixel), spread through the list so that the chunks shift
    extra = np.zeros((6, 3, 3, 3), np.float32)
    extra[:, 0] = np.float32([W + R + 40, -R - 3, 5, -0.9 * R, W - 1 + 0.9 * R, -0.8 * R]).reshape(6, 1, 1)
    extra[:, 1] = np.float32([5, 5, H + R + 9, -0.9 * R, H - 1 + 0.9 * R, H - 1 + 0.8 * R]).reshape(6, 1, 1)
    extra[:, 2] = 7.0
    at = np.sort(np.random.default_rng(8).integers(0, K, 6))
    p2, c2 = np.insert(patches, at, extra, 0), np.insert(conf, at, np.float32(5.0), 0)
    c = _regress(np.repeat(IDENT[None], K + 6, 0), p2, c2, H, W, R)
    assert georef.same_bits(a["invdepth"], c["invdepth"]) and georef.same_bits(a["weight"], c["weight"])
    assert c["status"][4] == a["status"][4] + 3 and c["status"][5] == a["status"][5] + 3 and c["status"][6] == a["status"][6]
    _status_ok(c["status"], K + 6)
    # another order of the points: within the bound of the comparison with float64
    perm = np.random.default_rng(9).permutation(K)
    d = _regress(poses, patches[perm], conf[perm], H, W, R)
    assert georef.same_bits(d["records"], a["records"][perm])
    cmp = depthref.compare_map(d["invdepth"], d["weight"], a["records"], PRIOR, PW, R, H, W)
    assert cmp["ok"], cmp
    assert np.abs(d["invdepth"].astype(np.float64) - a["invdepth"]).max() <= 2 * cmp["invdepth"]["bound"]


# ------------------------------------------------------------------------------------------------ 5. selection, clipping
def test_selection_and_clipping():
    from rampvo_amd import ops
    s, cam, var = _geo()
    H, W = SHAPES[0]
    M, n = s["M"], s["n_frames"] * s["M"]
    maps = ("invdepth", "weight")
    rng = np.random.default_rng(13)
    ids = rng.permutation(n)[:200].astype(np.int32)
    live = 150
    lst = np.concatenate([ids, np.int32([-5, n + 3])])                           # (behind the count: never read)
    a = _geo_call(H, W, 12.0, 1.0, index=cu(lst), count=cu(np.int32([live])))
    sel = ids[:live]
    dense = _np(ops.invdepth_map(cu(s["poses"][sel // M]), cu(s["patches"][sel]), cu(s["intr"][0]), cu(cam), H, W, 12.0,
                                 conf=cu(var[sel]), conf_is_variance=True, prior=PRIOR, prior_weight=PW, want_records=True))
    assert a["records"].shape == (202, 4) and not a["records"][live:].any() and a["status"][1] == live
    assert georef.same_bits(a["records"][:live], dense["records"])
    for k in maps + ("status",):
        assert georef.same_bits(a[k], dense[k]), k
    # no count: the whole list; an id outside the patches is a patch without a depth
    b = _geo_call(H, W, 12.0, 1.0, index=cu(lst))
    assert b["status"][1] == 202 and b["status"][2] >= 2 and b["records"][200:, 3].tolist() == [0, 0]
    _status_ok(b["status"], 202)
    # the row count on the device, and the newest rows of it
    words = cu(np.int32([99, 5, 99]))
    for last, lo in ((0, 0), (2, 3), (7, 0)):
        c = _geo_call(H, W, 12.0, 1.0, dyn_rows=words[1:], per_row=M, last_rows=last)
        ref = _np(ops.invdepth_map(cu(s["poses"][lo:5]), cu(s["patches"][lo * M:5 * M]), cu(s["intr"][0]), cu(cam), H, W, 12.0,
                                   conf=cu(var[lo * M:5 * M]), conf_is_variance=True, prior=PRIOR, prior_weight=PW,
                                   want_records=True))
        k = (5 - lo) * M
        assert c["status"][1] == k and georef.same_bits(c["records"][:k], ref["records"]) and not c["records"][k:].any()
        for m in maps + ("status",):
            assert georef.same_bits(c[m], ref[m]), (last, m)
    c = _geo_call(H, W, 12.0, 1.0, last_rows=3, per_row=M)                       # (the newest rows without a device count)
    assert c["status"][1] == 3 * M and c["records"].shape == (3 * M, 4)
    # the two flags equal their hand-formed equivalents
    full = _geo_call(H, W, 12.0, 1.0)
    hand = _geo_call(H, W, 12.0, 1.0, conf=cu(np.float32(1.0) / var), conf_is_variance=False)
    rel = _np(ops.invdepth_map(cu(s["poses"]), cu(s["patches"]), cu(s["intr"][0]), cu(cam), H, W, 12.0, conf=cu(var),
                               conf_is_variance=True, prior=PRIOR, prior_weight=PW, prior_relative=True, want_records=True))
    pw = float(np.float32(PW) / (np.float32(PRIOR) * np.float32(PRIOR)))
    absolute = _np(ops.invdepth_map(cu(s["poses"]), cu(s["patches"]), cu(s["intr"][0]), cu(cam), H, W, 12.0, conf=cu(var),
                                    conf_is_variance=True, prior=PRIOR, prior_weight=pw, want_records=True))
    for k in maps + ("records", "status"):
        assert georef.same_bits(full[k], hand[k]), k
        assert georef.same_bits(rel[k], absolute[k]), k
    assert not georef.same_bits(rel["invdepth"], full["invdepth"])


# ------------------------------------------------------------------------------------------------ 6. failure behaviour
def test_a_camera_that_is_not_finite_and_bad_patches():
    from rampvo_amd import ops
    H, W = SHAPES[1]
    poses, patches, conf = _points(14, 70, H, W, 12.0)
    for col, bad in ((1, np.nan), (5, np.inf)):
        cam = IDENT.copy()
        cam[col] = bad
        r = _np(ops.invdepth_map(cu(poses), cu(patches), cu(K4), cu(cam), H, W, 12.0, conf=cu(conf), prior=PRIOR, prior_weight=PW,
                                 want_records=True))
        assert r["status"][0] & 1 and ops.invdepth_map_status(cu(r["status"]))["bad_cam"]
        assert np.isnan(r["invdepth"]).all() and np.isnan(r["weight"]).all() and np.isnan(r["records"]).all()
        _status_ok(r["status"], 70)
        assert r["status"][5] == 0
    good = _regress(poses, patches, conf, H, W, 12.0)
    p2, c2 = patches.copy(), conf.copy()
    p2[3, 2], p2[10, 2], p2[11, 2] = np.nan, 0.0, -0.5
    c2[20], c2[21], c2[22] = 0.0, -1.0, np.nan
    r = _regress(poses, p2, c2, H, W, 12.0)
    rejected = [3, 10, 11, 20, 21, 22]
    assert r["status"][2] == 6 and good["status"][2] == 0 and not r["records"][rejected, 3].any()
    _status_ok(r["status"], 70)
    keep = np.setdiff1d(np.arange(70), rejected)
    q = _regress(poses[keep], p2[keep], c2[keep], H, W, 12.0)                    # the others: a call without those patches
    assert georef.same_bits(r["invdepth"], q["invdepth"]) and georef.same_bits(r["weight"], q["weight"])
    v = _regress(poses, patches, np.where(np.arange(70) == 4, np.inf, conf).astype(np.float32), H, W, 12.0, conf_is_variance=True)
    assert v["status"][2] == 1 and v["records"][4, 3] == 0                       # an infinite variance
    s = ops.invdepth_map_status(cu(r["status"]))
    assert s["n_bad_depth"] == 6 and s["n_considered"] == 70 and not s["bad_cam"]
    assert s["n_bad_depth"] + s["n_rejected"] + s["n_out_of_reach"] + s["n_contributing"] == 70
    # Z' at the threshold: the camera moves forward by 1, Z' = 1 - d
    cam = np.float32([0, 0, 1.0, 0, 0, 0, 1])
    pz = patches[:2].copy()
    pz[:, 0], pz[:, 1], pz[0, 2], pz[1, 2] = K4[2], K4[3], 0.9, 0.5
    r = _np(ops.invdepth_map(cu(poses[:2]), cu(pz), cu(K4), cu(cam), H, W, 12.0, want_records=True))
    assert r["status"].tolist()[:6] == [0, 2, 0, 1, 0, 1] and np.isnan(r["records"][0, :3]).all()
    assert np.allclose(r["records"][1], [K4[2], K4[3], 1.0, 1.0], atol=1e-5)


def test_arguments_and_canaries():
    """the C entry with guard words on both sides of every output and of the workspace; each bad argument: RAMP_EINVAL and
    nothing written; a short workspace: RAMP_EWORKSPACE; zero capacity runs the launches"""
    from rampvo_amd import _lib
    L = _lib.lib()
    H, W = SHAPES[1]
    K, R = 300, 12.0
    poses, patches, conf = _points(15, K, H, W, R)
    dpo, dpa, dco, dK, dcam = cu(poses), cu(patches), cu(conf), cu(K4), cu(IDENT)
    dprior = torch.full((1,), PRIOR, device="cuda")
    nbytes = L.ramp_invdepth_map_workspace_bytes(K)

    bufs = dict(inv=Flat(H * W, torch.float32, -7.0), wgt=Flat(H * W, torch.float32, -7.0),
                rec=Flat(4 * K, torch.float32, -7.0), status=Flat(8, torch.int32, -7), ws=Flat(nbytes, torch.uint8, 0xA5))
    assert bufs["ws"].t.data_ptr() % 16 == 0

    def call(n=K, M=1, P=3, scale=1.0, H_=H, W_=W, R_=R, pw=PW, flags=0, outs=("inv", "wgt", "rec"), ws_bytes=nbytes,
             prior=dprior, count=None, last_rows=0, per_row=0):
        o = lambda k: _lib.ptr(bufs[k].t) if k in outs else None
        rc = L.ramp_invdepth_map(_lib.ptr(dpo), _lib.ptr(dpa), _lib.ptr(dK), _lib.ptr(dcam), n, M, P, scale, None,
                                 _lib.ptr(count), 0, None, per_row, last_rows, _lib.ptr(dco), _lib.ptr(prior), pw, R_, flags, H_,
                                 W_, o("inv"), o("wgt"), o("rec"), _lib.ptr(bufs["ws"].t), ws_bytes,
                                 _lib.ptr(bufs["status"].t), _lib.stream())
        torch.cuda.synchronize()
        return rc

    before = {k: v.snapshot() for k, v in bufs.items()}
    inf, nan = float("inf"), float("nan")
    for kw in (dict(H_=0), dict(W_=0), dict(R_=0.0), dict(R_=-1.0), dict(R_=nan), dict(R_=inf), dict(pw=-0.5), dict(pw=nan),
               dict(pw=inf), dict(outs=()), dict(M=0), dict(P=0), dict(n=-1), dict(scale=0.0), dict(scale=nan), dict(flags=4),
               dict(prior=None), dict(count=dprior), dict(last_rows=2, per_row=0)):
        assert call(**kw) == -1, kw
    assert call(ws_bytes=nbytes - 16) == -3
    assert all(bufs[k].unchanged(before[k]) for k in bufs)                 # nothing written, status included
    assert call() == 0
    for k, b in bufs.items():
        assert b.intact(), k
    ref = _regress(poses, patches, conf, H, W, R)
    got = dict(invdepth=bufs["inv"].t.view(H, W), weight=bufs["wgt"].t.view(H, W), records=bufs["rec"].t.view(K, 4),
               status=bufs["status"].t)
    for k, v in got.items():
        assert georef.same_bits(v.cpu().numpy(), ref[k]), k
    # records alone: one launch less, [6] stays 0; a prior of weight 0 may be NULL
    assert call(outs=("rec",), prior=None, pw=0.0) == 0
    assert georef.same_bits(bufs["rec"].t.view(K, 4).cpu().numpy(), ref["records"])
    assert bufs["status"].t.cpu().tolist() == ref["status"].tolist()[:6] + [0, 0]
    # zero capacity: the launches run, the prior everywhere
    assert call(n=0) == 0
    assert (bufs["inv"].t == PRIOR).all() and not bufs["wgt"].t.any()
    assert bufs["status"].t.cpu().tolist() == [0, 0, 0, 0, 0, 0, H * W, 0]
    for k, b in bufs.items():
        assert b.intact(), k


# ------------------------------------------------------------------------------------------------ 7. tracker
def _from_parts(slam, n, t_now, want_records=True):
    """the two maps from the parts: the pose of poses_at, map()'s selection with the depth variance of the same query, the
    newest REMOVAL_WINDOW rows, the median of the last three frames' patches"""
    from rampvo_amd import ops
    cam = slam.poses_at([t_now], as_tensor=True)[0][0]
    index = slam.map(min_obs=2)["index"].to(torch.int32).contiguous()
    dvar = slam._window_query("test", with_map=True)[1]
    med = torch.median(slam.patches_[n - 3:n, :, 2])
    var = ops.invdepth_map(slam.poses_, slam.patches_, slam.intrinsics_[0], cam, 240, 320, RADIUS, scale=slam.RES, index=index,
                           conf=dvar, conf_is_variance=True, prior=med, prior_weight=1.0, prior_relative=True,
                           want_records=want_records)
    lo = max(n - int(slam.cfg.REMOVAL_WINDOW), 0)
    uni = ops.invdepth_map(slam.poses_[lo:n], slam.patches_[lo:n], slam.intrinsics_[0], cam, 240, 320, RADIUS, scale=slam.RES,
                           prior=med, prior_weight=4.0, want_records=want_records)
    return _np(var), _np(uni), float(med)


@torch.no_grad()
def _run(query):
    from rampvo_amd import ops
    slam = kit.tracker(True, True)
    slam.pose_stream()
    res = {}
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if f == kit.T_QUERY and query:
            res["resident_before"] = kit.resident(slam)
            var = slam.invdepth_map(radius=RADIUS, as_tensor=True)
            uni = slam.invdepth_map(radius=RADIUS, weights="uniform", prior_rel_sigma=0.5, as_tensor=True)
            res["numpy"] = slam.invdepth_map(radius=RADIUS)
            x, y, t, p = kit.query_events(f)
            comp = slam.compensate_events(x, y, t, p, invdepth="map", radius=RADIUS, want_xy=True, as_tensor=True)
            res["resident_after"] = kit.resident(slam)
            knots, ts = slam.trajectory(as_tensor=True)
            ref = ops.event_warp(x, y, t, p, knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), frame[2].cuda().float(),
                                 var["invdepth"], 240, 320, want_xy=True)
            res.update(var=_np(var), uni=_np(uni), comp=_np(comp), ref=_np(ref), n_query=slam.peek()["n"])
            res["parts_var"], res["parts_uni"], res["med"] = _from_parts(slam, slam.peek()["n"], kit.tstamp(f))
            res["still_resident"] = kit.resident(slam)
    n = slam.peek()["n"]
    res["final_resident"] = kit.resident(slam)
    res["poses"] = slam.poses_[:n].cpu().numpy()
    del slam
    kit.quiesce()
    return res


def test_tracker_invdepth_map():
    """Ramp_vo.invdepth_map equals ops.invdepth_map fed from the parts in both weight modes, compensate_events with the map
    equals ops.event_warp given that map, the tracker stays device resident and the frames behind the queries give the poses
    of a run without them"""
    a, b = _run(True), _run(False)
    assert a["resident_before"] and a["resident_after"] and a["still_resident"] and a["final_resident"] and b["final_resident"]
    assert a["med"] > 0
    for mode in ("var", "uni"):
        got, parts = a[mode], a["parts_" + mode]
        for k in ("invdepth", "weight"):
            assert georef.same_bits(got[k], parts[k]), (mode, k)
        assert got["status"].tolist() == parts["status"].tolist() and got["status"][0] == 0 and got["status"][5] >= 48
        _status_ok(got["status"])
        live = parts["records"][:, 3] > 0
        lo, hi = min(parts["records"][live, 2].min(), a["med"]), max(parts["records"][live, 2].max(), a["med"])
        assert np.isfinite(got["invdepth"]).all()
        assert got["invdepth"].min() >= lo * (1 - 1e-5) and got["invdepth"].max() <= hi * (1 + 1e-5)
        assert got["invdepth"].max() > got["invdepth"].min()                   # (relief: not one plane)
    assert a["uni"]["status"][1] == min(a["n_query"], 22) * 48                 # (the newest REMOVAL_WINDOW rows)
    for k in ("invdepth", "weight", "status", "pose_status"):
        assert isinstance(a["numpy"][k], np.ndarray) and georef.same_bits(a["numpy"][k], a["var"][k]), k      # as_tensor=False
    for k in ("xy", "iwe", "status"):
        assert georef.same_bits(a["comp"][k], a["ref"][k]), k
    assert a["comp"]["status"][0] == 0 and a["comp"]["status"][3:7].sum() == 5000
    assert georef.same_bits(a["poses"], b["poses"])


@torch.no_grad()
def test_tracker_invdepth_map_host_driven():
    """a host-driven tracker (no device-resident step): the numpy form of invdepth_map equals ops.invdepth_map fed from the
    parts in both weight modes; frame time stamps that decrease make it raise"""
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None and f < kit.T_FRAMES - 1
    var = slam.invdepth_map(radius=RADIUS)
    uni = slam.invdepth_map(radius=RADIUS, weights="uniform", prior_rel_sigma=0.5)
    parts_var, parts_uni, med = _from_parts(slam, slam._n, kit.tstamp(f), want_records=False)
    assert med > 0 and sorted(var) == ["invdepth", "pose_status", "status", "weight"]
    for got, parts in ((var, parts_var), (uni, parts_uni)):
        for k in ("invdepth", "weight", "status"):
            assert isinstance(got[k], np.ndarray) and georef.same_bits(got[k], parts[k]), k
        assert got["status"][0] == 0 and got["status"][5] > 0 and np.isfinite(got["invdepth"]).all()
        _status_ok(got["status"])
    assert uni["status"][1] == slam._n * 48
    with pytest.raises(RuntimeError, match="weights is"):
        slam.invdepth_map(weights="none")
    with pytest.raises(RuntimeError, match="invdepth is"):
        slam.compensate_events(np.zeros(1), np.zeros(1), np.full(1, 100.0), np.ones(1), invdepth="median")
    slam.tlist = slam.tlist[::-1]
    with pytest.raises(RuntimeError, match="time stamps decrease"):
        slam.invdepth_map(radius=RADIUS, weights="uniform")
    del slam
    kit.quiesce()
