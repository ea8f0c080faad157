"""The event map on the GPU: ``ramp_depth_points`` and ``ramp_point_map_*`` (csrc/evmap.hip) through the C entry points (every
buffer between canaries, tests/guarded.py), ``ops.depth_points`` / ``ops.PointMap`` and the tracker's ``event_map_insert`` /
``event_map_points``.

Everything but the world points is compared BIT FOR BIT with the restatement (tests/pointmapref.py): the filtered map, the
pixel list, the count, every status word, every word of the export.  The world points are compared with the float64 lift of
the call's own filtered depths by the bound rule of test_geometry_f64_gpu.py: ``georef.bound(FLOOR["act4"] x largest
|coordinate|, env)``, env = the float32 restatement's own error against float64.  Largest measured / bound on an MI355X: see
README "Event map".  Images are 13 x 17 (no tile divides them).  Nothing here provokes a fault: the full table ends by its probe
bound."""
import ctypes

import numpy as np
import pytest
import torch

import dsiref
import georef
import pointmapref as pm
import trackerkit as kit
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W, V = pm.H, pm.W, 0.25
P = lambda f: ctypes.c_void_p(f.address()) if isinstance(f, Flat) else (None if f is None else ctypes.c_void_p(f.data_ptr()))


def _stream():
    from rampvo_amd import _lib
    return _lib.stream()


def _depth_points(inv, cam=pm.CAM, Kc=pm.K, plane=None, conf=None, r=2, s=3, min_d=0.0, filtered=True, expect=0, **over):
    """the C entry with every buffer between canaries -> numpy dict (outputs cut to the count)"""
    from rampvo_amd import _lib
    L = _lib.lib()
    h, w = inv.shape
    nbytes = L.ramp_depth_points_ws_bytes(h, w)
    b = dict(points=Flat((h * w, 3), torch.float32), conf=Flat(h * w, torch.float32), pixel=Flat(h * w, torch.int32),
             filtered=Flat((h, w), torch.float32), count=Flat(1, torch.int32), status=Flat(8, torch.int32),
             ws=Flat(nbytes, torch.uint8, rows=4))
    d_inv, d_cam, d_K = cu(np.asarray(inv, np.float32)), cu(np.asarray(cam, np.float32)), cu(np.asarray(Kc, np.float32))
    d_plane, d_conf = None if plane is None else cu(plane.astype(np.int32)), None if conf is None else cu(conf.astype(np.float32))
    torch.cuda.synchronize()
    before = {k: v.snapshot() for k, v in b.items()}
    a = dict(p_inv=P(d_inv), p_plane=P(d_plane), p_conf=P(d_conf), p_cam=P(d_cam), p_K=P(d_K), H=h, W=w, r=r, s=s, min_d=min_d,
             p_points=P(b["points"]), p_oconf=P(b["conf"]), p_pixel=P(b["pixel"]), p_filtered=P(b["filtered"]) if filtered else None,
             p_count=P(b["count"]), p_ws=P(b["ws"]), nbytes=nbytes, p_status=P(b["status"]))
    assert set(over) <= set(a), over
    a.update(over)
    rc = L.ramp_depth_points(a["p_inv"], a["p_plane"], a["p_conf"], a["p_cam"], a["p_K"], a["H"], a["W"], a["r"], a["s"], a["min_d"],
                             a["p_points"], a["p_oconf"], a["p_pixel"], a["p_filtered"], a["p_count"], a["p_ws"], a["nbytes"], a["p_status"],
                             _stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, over)
    assert all(v.intact() for v in b.values())
    if rc:
        assert all(v.unchanged(before[k]) for k, v in b.items()), "a refused call touches nothing"
        return None
    k = int(b["count"].t.cpu())
    out = {n: b[n].t.cpu().numpy() for n in ("points", "conf", "pixel", "filtered", "status")}
    assert (out["pixel"][k:] == b["pixel"].canary).all() and (out["points"][k:] == b["points"].canary).all()
    return dict(points=out["points"][:k], conf=out["conf"][:k], pixel=out["pixel"][:k], filtered=out["filtered"], status=out["status"],
                count=k)


def _check_points(r, ref, tab=None, name=""):
    """bit for bit: filtered map, pixel, count, conf, status; the points against float64 by the bound rule"""
    assert r["count"] == ref["count"] and np.array_equal(r["pixel"], ref["pixel"])
    assert georef.same_bits(r["filtered"], ref["filtered"]) and georef.same_bits(r["conf"], ref["conf"])
    assert r["status"].tolist() == ref["status"].tolist()
    st = r["status"]
    assert st[2] + st[3] + st[4] == st[1] and st[4] == r["count"]
    if not r["count"]:
        return 0.0
    err, env = georef.max_err(r["points"], ref["points64"]), georef.max_err(ref["points32"], ref["points64"])
    floor = georef.FLOOR["act4"] * max(1.0, float(np.abs(ref["points64"]).max()))
    print("depth_points %s: err %.3g env %.3g bound %.3g ratio %.3g" % (name, err, env, georef.bound(floor, env), err / georef.bound(floor, env)))
    if tab is not None:
        tab.add(name, err, env, floor)
    assert err <= georef.bound(floor, env), (name, err, env, floor)
    return err / georef.bound(floor, env)


# ------------------------------------------------------------------------------------------------ 1. depth_points
@pytest.mark.parametrize("mask", pm.MASKS)
@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_depth_points_bits(mask, r):
    inv, plane, conf = pm.depth_case(mask, seed=r)
    for s in (1, 3, (2 * r + 1) ** 2):
        out = _depth_points(inv, plane=plane, conf=conf, r=r, s=s)
        _check_points(out, pm.depth_points(inv, pm.CAM, pm.K, plane, conf, r, s), name="%s r=%d s=%d" % (mask, r, s))
        if mask == "empty":
            assert out["count"] == 0 and out["status"].tolist() == [0] * 8 and np.isnan(out["filtered"]).all()
        if mask == "one":
            assert out["status"][1] == 1 and out["count"] == (1 if s == 1 else 0) and out["status"][2] == (0 if s == 1 else 1)
        if mask == "full" and r > 0 and s == (2 * r + 1) ** 2:                      # only the interior has a full window
            assert out["status"][2] == H * W - (H - 2 * r) * (W - 2 * r)


def test_plane_none_min_invdepth_and_no_optional_output():
    inv, _, conf = pm.depth_case("full", seed=9)
    n_bad = int((~(np.isfinite(inv) & (inv > 0))).sum())
    assert n_bad == 4
    for min_d, filtered in ((0.0, True), (0.5, True), (0.5, False), (3.0, True)):
        out = _depth_points(inv, conf=None, r=1, s=2, min_d=min_d, filtered=filtered)
        ref = pm.depth_points(inv, pm.CAM, pm.K, None, None, 1, 2, min_d)
        if not filtered:
            out["filtered"] = ref["filtered"]              # (not written: the canaries of the unused buffer are checked in the call)
        _check_points(out, ref, name="plane=None min=%g" % min_d)
        assert out["status"][1] == H * W - n_bad and (out["conf"] == 1.0).all()
        assert (min_d == 0.0) == (out["status"][3] == 0) and (min_d < 3.0 or out["count"] == 0)
    # with a plane map the NaN, zero, negative and infinite values ARE detected: they vote in the medians and are depth rejected
    inv, plane, conf = pm.depth_case("full", seed=9)
    out = _depth_points(inv, plane=plane, conf=conf, r=0, s=1)
    _check_points(out, pm.depth_points(inv, pm.CAM, pm.K, plane, conf, 0, 1), name="bad values r=0")
    assert out["status"][1] == H * W and out["status"][3] == 4


def test_a_camera_that_is_not_finite_lifts_nothing():
    inv, plane, conf = pm.depth_case("random")
    for cam, Kc in ((pm.CAM * np.float32(np.nan), pm.K), (np.r_[np.float32(np.inf), pm.CAM[1:]], pm.K), (pm.CAM, np.float32([16, 0, 8.5, 6.25])),
                    (pm.CAM, np.float32([16, 12, np.nan, 6.25]))):
        out = _depth_points(inv, cam=cam, Kc=Kc, plane=plane, conf=conf)
        assert out["count"] == 0 and out["status"].tolist() == [1] + [0] * 7 and np.isnan(out["filtered"]).all()


def test_points_against_float64_and_a_call_repeats_its_bits():
    """several poses and intrinsics; the largest measured / bound is printed (README "Event map")"""
    tab = georef.Table("depth_points: world points against float64")
    rng = np.random.default_rng(5)
    worst = 0.0
    for i in range(6):
        q = rng.normal(size=4)
        cam = np.r_[rng.uniform(-5, 5, 3) * 10.0 ** (i - 2), q / np.linalg.norm(q)].astype(np.float32)
        Kc = np.float32([16 * (i + 1), 12 * (i + 1), 8.5, 6.25])
        inv, plane, conf = pm.depth_case("random", seed=20 + i, bad_values=False)
        a = _depth_points(inv, cam=cam, Kc=Kc, plane=plane, conf=conf, r=2, s=3)
        worst = max(worst, _check_points(a, pm.depth_points(inv, cam, Kc, plane, conf, 2, 3), tab, "pose %d" % i))
        b = _depth_points(inv, cam=cam, Kc=Kc, plane=plane, conf=conf, r=2, s=3)
        assert georef.same_bits(a["points"], b["points"]) and a["count"] == b["count"] > 20
    tab.show()
    print("depth_points: largest measured / bound = %.3f" % worst)
    assert not tab.failed(), tab.failed()


def test_depth_points_refusals_touch_nothing():
    from rampvo_amd import _lib
    inv, plane, conf = pm.depth_case("random")
    for over in (dict(H=0), dict(W=-1), dict(r=-1), dict(r=4), dict(s=0), dict(min_d=-1.0), dict(min_d=float("nan")), dict(min_d=float("inf")),
                 dict(p_inv=None), dict(p_cam=None), dict(p_K=None), dict(p_points=None), dict(p_oconf=None), dict(p_pixel=None),
                 dict(p_count=None), dict(p_ws=None), dict(p_status=None)):
        _depth_points(inv, plane=plane, conf=conf, expect=_lib.RAMP_EINVAL, **over)
    _depth_points(inv, plane=plane, conf=conf, expect=_lib.RAMP_EUNSUPPORTED, H=1 << 16, W=1 << 15)
    nbytes = _lib.lib().ramp_depth_points_ws_bytes(H, W)
    _depth_points(inv, plane=plane, conf=conf, expect=_lib.RAMP_EWORKSPACE, nbytes=nbytes - 1)


def test_ops_depth_points_on_a_side_stream():
    from rampvo_amd import ops
    inv, plane, conf = pm.depth_case("checker", seed=3)
    ref = pm.depth_points(inv, pm.CAM, pm.K, plane, conf, 2, 3)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        r = ops.depth_points(cu(inv), cu(pm.CAM), pm.K, plane=cu(plane), confidence=cu(conf), want_filtered=True)
        st = ops.depth_points_status(r["status"])
    side.synchronize()
    k = int(r["count"].cpu())
    out = dict(points=r["points"][:k].cpu().numpy(), conf=r["conf"][:k].cpu().numpy(), pixel=r["pixel"][:k].cpu().numpy(),
               filtered=r["invdepth_filtered"].cpu().numpy(), status=r["status"].cpu().numpy(), count=k)
    _check_points(out, ref, name="ops, side stream")
    assert st == dict(bad_camera=False, n_detected=int(ref["status"][1]), n_isolated=int(ref["status"][2]),
                      n_depth_rejected=int(ref["status"][3]), n_lifted=k)


# ------------------------------------------------------------------------------------------------ 2. the voxel hash
class GMap:
    """the C entry points of the table with every buffer between canaries"""

    def __init__(self, capacity, voxel=V):
        from rampvo_amd import _lib
        self.L, self.cap, self.voxel = _lib.lib(), capacity, voxel
        self.buf = Flat(self.L.ramp_point_map_bytes(capacity), torch.uint8)
        self.clear()

    def clear(self):
        assert self.L.ramp_point_map_clear(P(self.buf), self.cap, _stream()) == 0

    def insert(self, points, conf=None, view=0, count=None, expect=0, **over):
        p = cu(np.asarray(points, np.float32).reshape(-1, 3))
        c = None if conf is None else cu(np.asarray(conf, np.float32))
        status = Flat(8, torch.int32)
        a = dict(p_map=P(self.buf), cap=self.cap, p_points=P(p) if len(p) else None, p_conf=P(c), n=len(p),
                 p_count=None if count is None else P(cu(np.int32([count]))), voxel=self.voxel, view=view, p_status=P(status))
        assert set(over) <= set(a), over
        a.update(over)
        rc = self.L.ramp_point_map_insert(a["p_map"], a["cap"], a["p_points"], a["p_conf"], a["n"], a["p_count"], a["voxel"], a["view"],
                                          a["p_status"], _stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, over)
        assert status.intact() and self.buf.intact()
        return status.t.cpu().numpy()

    def export(self, min_points=1, min_views=1, max_out=None, expect=0, **over):
        R = self.cap if max_out is None else max_out
        nbytes = self.L.ramp_point_map_export_ws_bytes(self.cap)
        b = dict(points=Flat((R, 3), torch.float32), n=Flat(R, torch.int32), conf=Flat(R, torch.float32), n_views=Flat(R, torch.int32),
                 key=Flat(R, torch.int64), count=Flat(1, torch.int32), status=Flat(8, torch.int32), ws=Flat(nbytes, torch.uint8, rows=4))
        torch.cuda.synchronize()
        before, table = {k: v.snapshot() for k, v in b.items()}, self.buf.snapshot()
        a = dict(p_map=P(self.buf), cap=self.cap, voxel=self.voxel, min_points=min_points, min_views=min_views, max_out=R,
                 nbytes=nbytes, **{"p_" + k: P(v) for k, v in b.items()})
        assert set(over) <= set(a), over
        a.update(over)
        rc = self.L.ramp_point_map_export(a["p_map"], a["cap"], a["voxel"], a["min_points"], a["min_views"], a["max_out"], a["p_points"],
                                          a["p_n"], a["p_conf"], a["p_n_views"], a["p_key"], a["p_count"], a["p_ws"], a["nbytes"],
                                          a["p_status"], _stream())
        torch.cuda.synchronize()
        assert rc == expect, (rc, over)
        assert all(v.intact() for v in b.values()) and self.buf.unchanged(table), "the export does not write the map"
        if rc:
            assert all(v.unchanged(before[k]) for k, v in b.items()), "a refused call touches nothing"
            return None
        k = int(b["count"].t.cpu())
        assert (b["key"].t[k:] == b["key"].canary).all()
        return {**{n: b[n].t[:k].cpu().numpy() for n in ("points", "n", "conf", "n_views", "key")}, "count": k,
                "status": b["status"].t.cpu().numpy()}


def _same_export(e, ref):
    assert e["count"] == ref["count"]
    assert np.array_equal(e["key"], ref["key"]) and np.array_equal(e["n"], ref["n"]) and np.array_equal(e["n_views"], ref["n_views"])
    assert georef.same_bits(e["points"], ref["points"]) and georef.same_bits(e["conf"], ref["conf"])
    assert e["status"].tolist() == [0, ref["n_passing"], ref["n_cut_off"], ref["n_occupied"], 0, 0, 0, 0]


@pytest.mark.parametrize("N", [0, 1, 2, 4099])
def test_insert_and_export_bits(N):
    p, c = pm.map_points(N, seed=N)
    if N > 100:
        p[5], c[6], c[7], p[8, 1] = np.nan, -1.0, np.inf, V * pm.AXIS                # three that are not finite, one out of range
    g, ref = GMap(1 << 13), pm.PointMapRef(V)
    st = g.insert(p, c, view=5)
    rs = ref.insert(p, c, view=5)
    occupied = ref.export()["n_occupied"] if N else 0
    assert st.tolist() == rs.tolist() + [occupied, 0] and st[1] == N and st[2:6].sum() == N
    if N:
        _same_export(g.export(), ref.export())
        assert N < 100 or (st[2] == 3 and st[3] == 1)
    else:
        e = g.export()
        assert e["count"] == 0 and e["status"].tolist() == [0] * 8


def test_no_confidence_counts_one_per_point():
    p, _ = pm.map_points(300, seed=2)
    g, ref = GMap(1 << 10), pm.PointMapRef(V)
    g.insert(p, None)
    ref.insert(p, None)
    e = g.export()
    _same_export(e, ref.export())
    assert np.array_equal(e["conf"], e["n"].astype(np.float32))


def _voxel_points(cells, per, seed):
    """``per`` points inside each voxel of ``cells`` (integer triples), away from the voxel's faces"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.float64).reshape(-1, 1, 3)
    return ((cells + rng.uniform(0.1, 0.9, (len(cells), per, 3))) * V).reshape(-1, 3).astype(np.float32)


def test_a_table_that_is_exactly_full():
    cells = [(i - 4, 2 * i, -i) for i in range(8)]
    p = _voxel_points(cells, 5, 1)
    g, ref = GMap(8), pm.PointMapRef(V)
    st = g.insert(p)
    ref.insert(p)
    assert st[4] == 0 and st[5] == 40 and st[6] == 8
    _same_export(g.export(), ref.export())


def test_a_table_that_overflows_drops_by_the_probe_bound():
    """9 voxels into 8 slots: the launch ends (every probe loop is bounded by the capacity), 8 voxels hold exactly the
    emulator's words, and the dropped points are those of the voxel that found no slot"""
    cells = [(i - 4, 2 * i, -i) for i in range(9)]
    per = [3, 4, 5, 6, 7, 8, 9, 10, 11]
    p = np.concatenate([_voxel_points([c], n, 10 + i) for i, (c, n) in enumerate(zip(cells, per))])
    g, ref = GMap(8), pm.PointMapRef(V)
    st = g.insert(p)
    ref.insert(p)
    e, r = g.export(), ref.export()
    assert st[6] == 8 and e["count"] == 8 and r["count"] == 9
    at = np.searchsorted(r["key"], e["key"])
    assert np.array_equal(r["key"][at], e["key"]) and np.array_equal(r["n"][at], e["n"])
    assert georef.same_bits(r["points"][at], e["points"]) and georef.same_bits(r["conf"][at], e["conf"])
    absent = np.setdiff1d(np.arange(9), at)
    assert len(absent) == 1 and st[4] == r["n"][absent[0]] and st[5] == len(p) - st[4] and st[1] == len(p)
    # a full table still takes the points of the voxels it holds, and drops every other point
    st = g.insert(_voxel_points([(100, 100, 100)], 70, 3))
    assert st[4] == 70 and st[5] == 0 and st[6] == 8
    present = [c for i, c in enumerate(cells) if make_key_of(c) in set(e["key"].tolist())]
    st = g.insert(_voxel_points(present[:2], 65, 4))
    assert st[4] == 0 and st[5] == 130 and st[6] == 8


def make_key_of(cell):
    return pm.make_key(*cell)


def test_4099_points_in_one_voxel():
    p = _voxel_points([(-3, 0, 7)], 4099, 5)
    c = np.random.default_rng(6).uniform(0, 4, 4099).astype(np.float32)
    g, ref = GMap(8), pm.PointMapRef(V)
    st = g.insert(p, c)
    ref.insert(p, c)
    e = g.export()
    _same_export(e, ref.export())
    assert st[5] == 4099 and st[6] == 1 and e["n"].tolist() == [4099] and e["key"].tolist() == [pm.make_key(-3, 0, 7)]


def test_keys_that_share_one_hash_slot():
    """40 voxels whose keys hash to slot 5 of 2^13: one probe chain of 40"""
    cap, cells = 1 << 13, []
    i = 0
    while len(cells) < 40:
        if pm.slot(pm.make_key(i, -i, 3), cap) == 5:
            cells.append((i, -i, 3))
        i += 1
    p = _voxel_points(cells, 3, 7)
    g, ref = GMap(cap), pm.PointMapRef(V)
    st = g.insert(p)
    ref.insert(p)
    assert st[5] == 120 and st[6] == 40
    _same_export(g.export(), ref.export())


def test_both_ends_of_the_range_and_one_voxel_beyond():
    """voxel 1.0: the float32 coordinates are exact.  Cells +-(2^20 - 1) are inside, +-2^20 outside (so is -2^20 itself)"""
    A = float(pm.AXIS)
    inside = np.float32([[A - 0.5, 0.5, 0.5], [-A + 1.5, 0.5, 0.5], [0.5, A - 1, -A + 1], [0.5, 0.5, -A + 1.25]])
    beyond = np.float32([[A, 0.5, 0.5], [0.5, -A - 0.5, 0.5], [0.5, 0.5, A + 1], [-A - 0.5, 0, 0], [3e38, 0, 0], [0, -A, 0]])
    g, ref = GMap(64, voxel=1.0), pm.PointMapRef(1.0)
    st = g.insert(np.concatenate([inside, beyond]))
    rs = ref.insert(np.concatenate([inside, beyond]))
    assert st[:6].tolist() == rs.tolist() and st[3] == 6 and st[5] == 4
    e = g.export()
    _same_export(e, ref.export())
    assert e["key"].min() == pm.make_key(-pm.AXIS + 1, 0, 0) and e["key"].max() == pm.make_key(pm.AXIS - 1, 0, 0)


def test_views_wrap_at_64():
    p = _voxel_points([(0, 0, 0), (1, 1, 1)], 2, 8)
    g, ref = GMap(16), pm.PointMapRef(V)
    for view, rows in ((0, slice(0, 4)), (63, slice(0, 2)), (64, slice(0, 4)), (2, slice(2, 4))):
        g.insert(p[rows], view=view)
        ref.insert(p[rows], view=view)
    e = g.export()
    _same_export(e, ref.export())
    assert sorted(e["n_views"].tolist()) == [2, 2]                 # {0, 63} (64 is 0 again) and {0, 2}
    _same_export(g.export(min_views=3), ref.export(min_views=3))
    from rampvo_amd import _lib
    g.insert(p, expect=_lib.RAMP_EINVAL, view=-1)


def test_one_insert_two_inserts_and_a_shuffled_insert_give_the_same_bits():
    p, c = pm.map_points(4099, seed=11)
    perm = np.random.default_rng(12).permutation(4099)
    a, b, s, ref = GMap(1 << 13), GMap(1 << 13), GMap(1 << 13), pm.PointMapRef(V)
    a.insert(p, c, view=9)
    b.insert(p[:1500], c[:1500], view=9); b.insert(p[1500:], c[1500:], view=9)
    s.insert(p[perm], c[perm], view=9)
    ref.insert(p, c, view=9)
    ea, eb, es = a.export(), b.export(), s.export()
    _same_export(ea, ref.export())
    for k in ("points", "n", "conf", "n_views", "key", "status"):
        assert np.array_equal(ea[k].view(np.int32), eb[k].view(np.int32)) and np.array_equal(ea[k].view(np.int32), es[k].view(np.int32)), k


def test_a_device_count_smaller_than_the_buffer():
    p, c = pm.map_points(1000, seed=13)
    p[700:] = np.nan                                         # behind the count: never read
    for count, live in ((600, 600), (0, 0), (-5, 0), (5000, 1000)):
        g, ref = GMap(1 << 12), pm.PointMapRef(V)
        st = g.insert(p, c, count=count)
        rs = ref.insert(p[:live], c[:live])
        assert st[:6].tolist() == rs.tolist() and st[1] == live
        if 0 < live <= 700:
            _same_export(g.export(), ref.export())


def test_min_points_min_views_and_a_max_out_that_cuts():
    p, c = pm.map_points(4099, seed=14, spread=1.5)
    g, ref = GMap(1 << 13), pm.PointMapRef(V)
    for view, rows in ((1, slice(0, 2500)), (2, slice(2500, 4099))):
        g.insert(p[rows], c[rows], view=view)
        ref.insert(p[rows], c[rows], view=view)
    for kw in (dict(min_points=3), dict(min_views=2), dict(min_points=4, min_views=2), dict(max_out=17), dict(min_points=2, max_out=1),
               dict(max_out=0), dict(min_points=10 ** 6), dict(min_points=0, min_views=0)):
        e, r = g.export(**kw), ref.export(**kw)
        _same_export(e, r)
    assert g.export(max_out=17)["status"][2] > 0 and g.export(min_views=2)["count"] > 0


def test_clear_and_repeated_calls():
    from rampvo_amd import ops
    p, c = pm.map_points(2000, seed=15)
    m = ops.PointMap(V, capacity=1 << 12)
    ref = pm.PointMapRef(V)
    exports = []
    for rep in range(3):
        st = ops.point_map_status(m.insert(cu(p), cu(c), view=rep))
        ref.insert(p, c, view=rep)
        assert st["n_seen"] == st["n_accumulated"] == 2000 and st["n_dropped_full"] == 0
        exports.append({k: v.cpu().numpy() for k, v in m.export().items()})
        again = {k: v.cpu().numpy() for k, v in m.export().items()}
        k = int(again["count"][0])
        assert all(np.array_equal(exports[-1][n][:k].view(np.int32), again[n][:k].view(np.int32)) for n in ("points", "n", "conf", "key"))
    r, k = ref.export(), int(exports[-1]["count"][0])
    assert k == r["count"] and np.array_equal(exports[-1]["key"][:k], r["key"]) and np.array_equal(exports[-1]["n"][:k], r["n"])
    assert georef.same_bits(exports[-1]["points"][:k], r["points"]) and (exports[-1]["n_views"][:k] == 3).all()
    assert ops.point_map_export_status(m.export(max_out=10)["status"]) == dict(n_passing=k, n_cut_off=k - 10, n_occupied=k)
    m.clear()
    e = m.export()
    assert int(e["count"].cpu()) == 0 and e["status"].cpu().tolist() == [0] * 8
    st = ops.point_map_status(m.insert(cu(p[:10]), None))
    assert st["n_occupied"] == len(np.unique(pm.fixed(p[:10], None, V)["key"]))


def test_the_map_on_a_side_stream():
    from rampvo_amd import ops
    p, c = pm.map_points(4099, seed=16)
    ref = pm.PointMapRef(V)
    ref.insert(p, c, view=1)
    side = torch.cuda.Stream()
    dp, dc = cu(p), cu(c)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        m = ops.PointMap(V, capacity=1 << 13)
        m.insert(dp, dc, view=1)
        e = m.export()
    side.synchronize()
    r, k = ref.export(), int(e["count"].cpu())
    assert k == r["count"] and np.array_equal(e["key"][:k].cpu().numpy(), r["key"])
    assert georef.same_bits(e["points"][:k].cpu().numpy(), r["points"]) and georef.same_bits(e["conf"][:k].cpu().numpy(), r["conf"])


def test_map_refusals_touch_nothing():
    from rampvo_amd import _lib
    p, c = pm.map_points(100, seed=17)
    g = GMap(64)
    g.insert(p, c)
    table = g.buf.snapshot()
    EINVAL = _lib.RAMP_EINVAL
    for over in (dict(p_map=None), dict(cap=63), dict(cap=4), dict(cap=1 << 31), dict(n=-1), dict(p_points=None), dict(voxel=0.0),
                 dict(voxel=-1.0), dict(voxel=float("nan")), dict(voxel=float("inf")), dict(p_status=None),
                 dict(p_map=ctypes.c_void_p(g.buf.address() + 8))):
        g.insert(p, c, expect=EINVAL, **over)
    g.insert(p, c, expect=EINVAL, view=-1)
    for over in (dict(p_map=None), dict(cap=48), dict(voxel=0.0), dict(p_points=None), dict(p_key=None), dict(p_count=None), dict(p_ws=None),
                 dict(p_status=None)):
        g.export(expect=EINVAL, **over)
    for kw in (dict(min_points=-1), dict(min_views=-1)):
        g.export(expect=EINVAL, **kw)
    g.export(expect=_lib.RAMP_EWORKSPACE, nbytes=_lib.lib().ramp_point_map_export_ws_bytes(64) - 1)
    assert g.L.ramp_point_map_clear(None, 64, _stream()) == EINVAL and g.L.ramp_point_map_clear(P(g.buf), 65, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert g.buf.unchanged(table)


# ------------------------------------------------------------------------------------------------ 3. end to end
def test_two_plane_scene_end_to_end():
    """dsiref.two_plane_scene through ops.event_dsi, ops.depth_points and ops.PointMap: every exported point lies within one
    voxel of one of the two planes.  The voxel, 0.2, is the depth that half a step of the sweep (0.05 in inverse depth: what the
    parabola can move a detection) spans at the far plane, 0.05 / 0.55^2 = 0.165, rounded up; the camera at t_ref is at the
    origin, so a plane of the sweep is z = 1 / d_k in the world.  The scene's points are single pixels: most detections are
    isolated and dropped, and so are the few that the sweep puts one plane off (they would lie 0.3 and more from their plane)"""
    from rampvo_amd import ops
    s = dsiref.TWO_PLANE
    x, y, t, knots, times = dsiref.two_plane_scene()
    r = ops.event_dsi(cu(x), cu(y), cu(t), cu(knots), cu(times), s["t_ref"], cu(s["K"]), s["H"], s["W"], planes=s["D"], range=s["rng"],
                      min_votes=s["min_votes"])
    assert dsiref.two_plane_conditions(r["plane"].cpu().numpy())["ok"]
    pts = ops.depth_points(r["invdepth"], cu(pm.IDENTITY), s["K"], plane=r["plane"], confidence=r["confidence"], median_radius=2,
                           min_support=3)
    voxel = 0.2
    m = ops.PointMap(voxel, capacity=1 << 12)
    st = ops.point_map_status(m.insert(pts["points"], pts["conf"], count=pts["count"], view=0))
    e = m.export()
    k = int(e["count"].cpu())
    z = e["points"][:k, 2].cpu().numpy().astype(np.float64)
    d, _ = dsiref.plane_depths(s["rng"], s["D"])
    za, zb = (1.0 / float(d[p]) for p in s["planes"])
    off = np.minimum(np.abs(z - za), np.abs(z - zb))
    print("two planes: %d points in %d voxels, largest distance to a plane %.4f (voxel %.2f)" % (st["n_accumulated"], k, off.max(), voxel))
    assert st["n_accumulated"] == int(pts["count"].cpu()) > 0 and st["n_dropped_full"] == 0 and k > 0
    assert (np.abs(z - za) <= voxel).any() and (np.abs(z - zb) <= voxel).any()           # both planes are in the map
    assert (off <= voxel).all(), off.max()


# ------------------------------------------------------------------------------------------------ 4. tracker
def _map_ask(slam, f, frame):
    x, y, t, _ = (v.clone() for v in kit.query_events(f))
    x[:400], y[:400], t[:400] = 100.0, 80.0, kit.tstamp(f)
    x[400:800], y[400:800], t[400:800] = 101.0, 80.0, kit.tstamp(f)
    x[800:1200], y[800:1200], t[800:1200] = 100.0, 81.0, kit.tstamp(f)
    pmap = slam.event_map(voxel=0.05, capacity=1 << 16)
    res = {"same_map": slam.event_map() is pmap}
    a = slam.event_map_insert(x, y, t, planes=24, min_votes=2.0, median_radius=1, min_support=2, as_tensor=True)
    res["resident_mid"] = kit.resident(slam)
    b = slam.event_map_insert(x, y, t, t_ref=kit.tstamp(f - 1), planes=24, min_votes=2.0, median_radius=1, min_support=2)
    res["tensor"], res["numpy"] = kit.host(a), b
    res["points"] = slam.event_map_points(min_points=1)
    res["points_t"] = kit.host(slam.event_map_points(min_points=1, as_tensor=True))
    res["counter"] = int(slam.counter)
    return res


def _check_map_answer(a):
    st = a["tensor"]
    assert a["same_map"] and sorted(st) == ["count", "depth_status", "map_status", "points_status", "pose_status"]
    assert st["depth_status"][0] == 0 and st["points_status"][0] == 0 and st["points_status"][4] == st["count"][0] == st["map_status"][1] > 0
    assert st["map_status"][2] == 0 and st["map_status"][4] == 0 and st["map_status"][5] + st["map_status"][3] == st["count"][0]
    nb = a["numpy"]
    assert nb["count"] == nb["points_status"]["n_lifted"] == nb["map_status"]["n_seen"] and not nb["points_status"]["bad_camera"]
    pts, pt = a["points"], a["points_t"]
    k = pts["count"]
    assert k == int(pt["count"][0]) > 0 and pts["points"].shape == (k, 3) and np.isfinite(pts["points"]).all()
    for n in ("points", "n", "conf", "n_views", "key"):
        assert np.array_equal(pts[n].view(np.int32), pt[n][:k].view(np.int32)), n
    assert pts["n"].sum() == st["map_status"][5] + nb["map_status"]["n_accumulated"] and (np.diff(pts["key"]) > 0).all()
    assert (pts["n_views"] == 1).all()                       # both inserts carry the same frame counter


def test_tracker_event_map_device_resident():
    """event_map_insert and event_map_points on a device-resident tracker: it stays resident and tracks the bits of a run that
    is never asked"""
    a, ctl = kit.run_resident(True, _map_ask), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_mid"] and a["resident_after"] and a["resident_at_end"]
    _check_map_answer(a)
    for f in (kit.T_QUERY + 1, kit.T_QUERY + 2):
        kit.same(a["state", f], ctl["state", f], "state %d" % f)


@torch.no_grad()
def test_tracker_event_map_host_driven_gives_the_same_bits_as_its_steps():
    """a host-driven tracker: the map equals ops.event_dsi -> ops.depth_points -> ops.PointMap fed by hand with the tracker's
    own trajectory; the default voxel is read from the depth median; queries before a map raise"""
    from rampvo_amd import ops
    slam = kit.tracker(False, False)
    with pytest.raises(RuntimeError, match="no event map yet"):
        slam.event_map_points()
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    rng = np.random.default_rng(23)
    x, y = rng.uniform(0, 319, 3000).astype(np.float32), rng.uniform(0, 239, 3000).astype(np.float32)
    t = rng.uniform(kit.tstamp(f - 2), kit.tstamp(f), 3000)
    x[:600], y[:600], t[:600] = np.repeat([100.0, 101.0, 100.0], 200), np.repeat([80.0, 80.0, 81.0], 200), kit.tstamp(f)
    n = slam._n
    med = float(torch.median(slam.patches_[n - 3:n, :, 2]))
    pmap = slam.event_map()
    assert pmap.voxel == 0.01 / med and pmap.capacity == 1 << 20
    out = slam.event_map_insert(x, y, t, planes=8, range=(0.1, 1.5), min_votes=1.5, median_radius=1, min_support=2)
    got = slam.event_map_points(min_points=1)
    knots, ts = slam.trajectory(as_tensor=True)
    dsi = ops.event_dsi(cu(x), cu(y), cu(t), knots, cu(np.asarray(ts, np.float64)), float(ts[-1]), frame[2].cuda().float(), 240, 320,
                        planes=8, range=(0.1, 1.5), min_votes=1.5)
    cam = slam.poses_at([float(ts[-1])], as_tensor=True)[0][0]
    pts = ops.depth_points(dsi["invdepth"], cam, frame[2].cuda().float(), plane=dsi["plane"], confidence=dsi["confidence"],
                           median_radius=1, min_support=2)
    ref = ops.PointMap(pmap.voxel, capacity=1 << 20)
    st = ops.point_map_status(ref.insert(pts["points"], pts["conf"], count=pts["count"], view=int(slam.counter)))
    e = ref.export()
    k = int(e["count"].cpu())
    assert out["map_status"] == st and out["count"] == st["n_seen"] > 0 and got["count"] == k > 0
    for name in ("points", "n", "conf", "n_views", "key"):
        assert np.array_equal(got[name].view(np.int32), e[name][:k].cpu().numpy().view(np.int32)), name
    with pytest.raises(RuntimeError, match="fill stays None"):
        slam.event_map_insert(x, y, t, fill=0.5)
    del slam, pmap, ref
    kit.quiesce()
