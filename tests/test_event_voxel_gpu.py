"""Event voxel grids on the GPU: ``ramp_event_voxel`` (csrc/voxel.hip) through ``ops.event_voxel_grid`` and
``Ramp_vo.event_voxel_grid``.

The accumulators, the raw grid, n, the sum and the mean are compared BIT FOR BIT with the exact integer emulator
(tests/voxelref.py ``voxel_grid``); std within a relative n x 2^-52 (a float64 sum of n terms in another order), every
normalised cell within one fp32 ulp.  Against the reference class's recorded output (tests/golden/event_voxel.npz) the
tolerance is the envelope rule of ``voxelref.compare``.  Images are 13 x 17 and 4 x 5.

The tracker tests run the small synthetic tracker of tests/trackerkit.py."""

import numpy as np
import pytest
import torch

import georef
import trackerkit as kit
import voxelref
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = 13, 17



def _events(seed, n, h=H, w=W, margin=1.0):
    """unsorted time stamps, the first and last by position inside their range; coordinates up to ``margin`` outside the image"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.0, n)
    if n > 1:
        t[0], t[-1] = 0.125, 0.875
    return (rng.uniform(-margin, w + margin, n).astype(np.float32), rng.uniform(-margin, h + margin, n).astype(np.float32), t,
            rng.choice([-1, 0, 1], n).astype(np.int8))


def _gpu(x, y, t, p, h, w, bins, offsets=None, normalize=True, subpixel=False):
    from rampvo_amd import ops
    r = ops.event_voxel_grid(cu(np.asarray(x, np.float32)), cu(np.asarray(y, np.float32)), cu(np.asarray(t, np.float64)),
                             cu(np.asarray(p, np.int8)), h, w, num_bins=bins,
                             offsets=None if offsets is None else cu(np.asarray(offsets, np.int64)), normalize=normalize,
                             subpixel=subpixel)
    r = {k: v.cpu().numpy() for k, v in r.items()}
    if offsets is None:
        r["grid"] = r["grid"][None]
    return r


def _within_one_ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    nan = np.isnan(b)
    return bool(np.array_equal(np.isnan(a), nan) and (np.abs(a.astype(np.float64) - b)[~nan] <= voxelref.ulp32(b)[~nan]).all())


def _check(x, y, t, p, h, w, bins, offsets=None, subpixel=False):
    """one event list, raw and normalised, against the emulator -> the emulator's result"""
    ref = voxelref.voxel_grid(x, y, t, p, h, w, bins, offsets=offsets, normalize=False, subpixel=subpixel)
    raw = _gpu(x, y, t, p, h, w, bins, offsets, False, subpixel)
    assert georef.same_bits(raw["grid"], ref["grid"])                       # float32(acc 2^-24): the accumulators
    assert np.array_equal(raw["status"], ref["status"]), (raw["status"], ref["status"])
    assert raw["status"][2:6].sum() == raw["status"][1] and not raw["status"][6:].any()
    nref, _ = voxelref.finish(ref["acc"], True, ref["failed"])
    nrm = _gpu(x, y, t, p, h, w, bins, offsets, True, subpixel)
    assert np.array_equal(nrm["status"], ref["status"])
    for st in (raw["stats"], nrm["stats"]):                                  # (n, mean, std, sum) in every mode
        assert georef.same_bits(st[:, [0, 1, 3]], ref["stats"][:, [0, 1, 3]])       # n and sum exact, the mean bit for bit
        n, sd, sd_ref = ref["stats"][:, 0], st[:, 2], ref["stats"][:, 2]
        assert np.array_equal(np.isnan(sd), np.isnan(sd_ref))
        ok = ~np.isnan(sd_ref)
        assert (np.abs(sd - sd_ref)[ok] <= n[ok] * 2.0 ** -52 * np.abs(sd_ref[ok])).all(), (sd, sd_ref)
    assert _within_one_ulp(nrm["grid"], nref)
    assert np.array_equal(nrm["grid"] == 0, nref == 0)
    return ref


# ------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("subpixel", [False, True])
@pytest.mark.parametrize("bins", [1, 2, 5])
@pytest.mark.parametrize("N", [0, 1, 2, 4099])
def test_grid_bits(N, bins, subpixel):
    x, y, t, p = _events(100 * N + bins, N)
    ref = _check(x, y, t, p, H, W, bins, subpixel=subpixel)
    if N == 4099:                                                            # (bins = 1: tn = 0 for every event, none without a bin)
        assert ref["status"][3] > 100 and (ref["status"][4] > 100) == (bins > 1) and ref["status"][5] > 2000


def test_second_trip_of_the_grid_and_unaligned_arrays():
    """one event more than a full grid covers in one trip; the same events from arrays that are not 16-byte aligned (the scalar
    staging path) give the same bits"""
    from rampvo_amd import _lib, ops
    N = _lib.lib().ramp_event_voxel_grid_events() + 1
    x, y, t, p = _events(3, N + 1)
    t[1] = 0.125
    _check(x[1:], y[1:], t[1:], p[1:], H, W, 5)
    xs, ys, ts, ps = cu(x)[1:], cu(y)[1:], cu(t)[1:], cu(p)[1:]
    assert xs.data_ptr() % 16 and xs.is_contiguous()
    a = ops.event_voxel_grid(xs, ys, ts, ps, H, W, subpixel=True)
    b = ops.event_voxel_grid(xs.clone(), ys.clone(), ts.clone(), ps.clone(), H, W, subpixel=True)
    for k in ("grid", "stats", "status"):
        assert georef.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()), k


@pytest.mark.parametrize("subpixel", [False, True])
def test_both_staging_paths_against_the_emulator(subpixel):
    """2 * 1024 + 1 events: two full tiles and a partial one.  From 16-byte aligned arrays the full tiles are staged with the
    16-byte loads; the same events as views one element into larger buffers take the scalar loop.  Each call gives the
    emulator's bits, and the two agree in every output and status word"""
    from rampvo_amd import ops
    x, y, t, p = _events(7, 2049 + 1)
    t[1] = 0.125
    ref = _check(x[1:], y[1:], t[1:], p[1:], H, W, 5, subpixel=subpixel)    # (uploads of their own: aligned)
    views = [cu(a)[1:] for a in (x, y, t, p)]
    assert all(v.data_ptr() % 16 and v.is_contiguous() for v in views)
    for normalize in (False, True):
        a = ops.event_voxel_grid(*views, H, W, num_bins=5, normalize=normalize, subpixel=subpixel)
        b = ops.event_voxel_grid(*(v.clone() for v in views), H, W, num_bins=5, normalize=normalize, subpixel=subpixel)
        for k in ("grid", "stats", "status"):
            assert georef.same_bits(a[k].cpu().numpy(), b[k].cpu().numpy()), (k, normalize)
        assert np.array_equal(a["status"].cpu().numpy(), ref["status"])
        if not normalize:
            assert georef.same_bits(a["grid"].cpu().numpy()[None], ref["grid"])


@pytest.mark.parametrize("subpixel", [False, True])
def test_order_of_the_events_does_not_matter(subpixel):
    """shuffled events give the same bits (the first and last stay in place: they define the time range); a call repeats them"""
    x, y, t, p = _events(4, 4099)
    perm = np.concatenate([[0], 1 + np.random.default_rng(5).permutation(4097), [4098]])
    a = _gpu(x, y, t, p, H, W, 5, subpixel=subpixel)
    b = _gpu(x[perm], y[perm], t[perm], p[perm], H, W, 5, subpixel=subpixel)
    c = _gpu(x, y, t, p, H, W, 5, subpixel=subpixel)
    for k in ("grid", "stats", "status"):
        assert georef.same_bits(a[k], b[k]) and georef.same_bits(a[k], c[k]), k


# ------------------------------------------------------------------------------------------------ 2. normalisation
def test_normalisation_conventions():
    # n = 1: the unbiased std is NaN, the mean is subtracted, the cell becomes 0
    r = _gpu([1], [2], [0.0], [1], 4, 5, 2)
    assert not r["grid"].any() and r["stats"][0, 0] == 1 and r["stats"][0, 1] == 1.0 and np.isnan(r["stats"][0, 2])
    # std = 0: two cells of the same value
    r = _gpu([1, 3], [2, 0], [0.0, 0.0], [1, 1], 4, 5, 2)
    assert not r["grid"].any() and r["stats"][0].tolist() == [2.0, 1.0, 0.0, 2.0]
    # n = 0: no event, and two events that cancel exactly
    for ev in (([], [], [], []), ([2.25, 2.75], [1.5, 1.25], [0.3, 0.3], [1, 0])):
        r = _gpu(*ev, 4, 5, 2)
        assert not r["grid"].any() and not r["stats"].any() and r["status"].tolist() == [0, len(ev[0]), 0, 0, 0, len(ev[0]), 0, 0]
    # +1 and -1: mean 0, unbiased std sqrt(2)
    r = _gpu([1, 3], [2, 0], [0.0, 0.0], [1, -1], 4, 5, 2)
    assert r["grid"][0, 0, 2, 1] == np.float32(1 / np.sqrt(2.0)) and r["grid"][0, 0, 0, 3] == -np.float32(1 / np.sqrt(2.0))
    # closed forms of the votes: tn = 1.25 puts 0.75 / 0.25 into bins 1 / 2; the last event lands wholly in the last bin
    r = _gpu([0, 2, 4], [0, 1, 3], [0.0, 1.25, 4.0], [1, 1, 1], 4, 5, 5, normalize=False)
    g = r["grid"][0]
    assert g[1, 1, 2] == 0.75 and g[2, 1, 2] == 0.25 and g[0, 0, 0] == 1.0 and g[4, 3, 4] == 1.0 and g.sum() == 3.0


# ------------------------------------------------------------------------------------------------ 3. the reference
@pytest.mark.parametrize("name", voxelref.CASES)
def test_against_the_reference_fixture(name):
    c = voxelref.load_case(name)
    e = c["events"]
    bins, h, w = (int(v) for v in c["shape"])
    for normalize in (False, True):
        r = _gpu(e[:, 1], e[:, 2], e[:, 0], e[:, 3], h, w, bins, normalize=normalize)
        q = voxelref.compare(r["grid"][0], c, normalize)
        print("%s normalize=%d: err %.3e, largest bound %.3e, worst err / bound %.3f" % (name, normalize, q["err"], q["bound"], q["worst"]))
        assert q["ok"], q
        assert r["stats"][0, 0] == (c["ref_raw"] != 0).sum() and r["status"][0] == 0


# ------------------------------------------------------------------------------------------------ 4. slices
def test_slices_equal_single_calls():
    """S = 3 with an empty middle slice equals three single calls, bit for bit"""
    x, y, t, p = _events(6, 600)
    off = [50, 300, 300, 580]                                                # (events in front of and behind the slices are not seen)
    for subpixel in (False, True):
        ref = _check(x, y, t, p, H, W, 5, offsets=off, subpixel=subpixel)
        assert ref["status"][1] == 530
        for normalize in (False, True):
            r = _gpu(x, y, t, p, H, W, 5, off, normalize, subpixel)
            assert not r["grid"][1].any() and not r["stats"][1].any()
            for s, (lo, hi) in enumerate(zip(off[:-1], off[1:])):
                q = _gpu(x[lo:hi], y[lo:hi], t[lo:hi], p[lo:hi], H, W, 5, None, normalize, subpixel)
                assert georef.same_bits(r["grid"][s], q["grid"][0]) and georef.same_bits(r["stats"][s], q["stats"][0]), s


def test_more_slices_than_the_lds_holds():
    """S + 1 offsets just above what the vote launch stages in LDS: the search in global memory; 4 x 5, 2 bins"""
    from rampvo_amd import _lib
    S = _lib.lib().ramp_event_voxel_lds_offsets()
    x, y, t, p = _events(7, 4099, 4, 5)
    rng = np.random.default_rng(8)
    off = np.sort(rng.integers(0, 4100, S + 1))
    off[:3] = 0                                                              # (empty slices at the front)
    _check(x, y, t, p, 4, 5, 2, offsets=off)
    _check(x, y, t, p, 4, 5, 2, offsets=off[:S], subpixel=True)              # and one fewer: the last chunk that fits the LDS


@pytest.mark.parametrize("off", [[0, 200, 100, 300], [-1, 100, 300], [0, 100, 301]])
def test_bad_offsets(off):
    x, y, t, p = _events(9, 300)
    r = _gpu(x, y, t, p, H, W, 5, offsets=off)
    assert r["status"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert np.isnan(r["grid"]).all() and np.isnan(r["stats"]).all()


def test_a_slice_whose_first_time_stamp_is_not_finite():
    x, y, t, p = _events(10, 300, margin=0.0)
    x, y = np.clip(x, 0, W - 0.5), np.clip(y, 0, H - 0.5)
    t[100] = np.inf
    off = [0, 100, 200, 300]
    ref = _check(x, y, t, p, H, W, 5, offsets=off)
    r = _gpu(x, y, t, p, H, W, 5, offsets=off)
    assert r["status"][0] == 2 and r["status"][2] == 1 and r["status"][4] >= 99
    assert np.isnan(r["grid"][1]).all() and np.isnan(r["stats"][1]).all()
    assert np.isfinite(r["grid"][[0, 2]]).all() and np.isfinite(r["stats"][[0, 2]]).all() and ref["failed"].tolist() == [False, True, False]


# ------------------------------------------------------------------------------------------------ 5. sub-pixel
def test_integer_coordinates_give_the_default_bits():
    x, y, t, p = _events(11, 4099, margin=2.0)
    x, y = np.trunc(x), np.trunc(y)                                          # (-2 .. W + 2: pixels outside on every side)
    for normalize in (False, True):
        a, b = _gpu(x, y, t, p, H, W, 5, normalize=normalize), _gpu(x, y, t, p, H, W, 5, normalize=normalize, subpixel=True)
        for k in ("grid", "stats", "status"):
            assert georef.same_bits(a[k], b[k]), k
    assert a["status"][3] > 100


def test_edge_neighbours_are_dropped():
    x = np.array([W - 0.5, 4.0, -1.5, 3.25, -0.5], np.float32)
    y = np.array([3.0, -0.25, 3.0, 4.5, H - 0.75], np.float32)
    r = _gpu(x, y, np.zeros(5), [1, 1, 1, 1, 1], H, W, 1, normalize=False, subpixel=True)
    g = r["grid"][0, 0]
    assert r["status"].tolist() == [0, 5, 0, 1, 0, 4, 0, 0]
    assert g[3, W - 1] == 0.5 and g[0, 4] == 0.75 and g[H - 1, 0] == 0.5 * 0.75 and g[4:6, 3:5].sum() == 1.0
    assert g.sum() == 0.5 + 0.75 + 0.375 + 1.0
    _check(x, y, np.zeros(5), [1, 1, 1, 1, 1], H, W, 1, subpixel=True)


def test_the_xy_of_the_event_warp_goes_straight_in():
    """event_warp(want_xy=True)'s coordinates, NaN rows included, as the sub-pixel grid's pixels: the NaN rows are counted in
    word 2 and the grid is the emulator's on those coordinates"""
    import interpref
    from rampvo_amd import ops
    knots, times = interpref.walk_scene(12, 5)
    rng = np.random.default_rng(13)
    n = 2000
    x, y = rng.uniform(0, W - 1, n).astype(np.float32), rng.uniform(0, H - 1, n).astype(np.float32)
    t = np.sort(rng.uniform(0.0, 4.0, n))
    p = rng.choice([-1, 1], n).astype(np.int8)
    x[::97] = np.nan                                                         # (rejected by the warp: NaN rows)
    K = cu(np.array([16.0, 12.0, 9.5, 6.25], np.float32))
    w = ops.event_warp(cu(x), cu(y), cu(t), cu(p), cu(knots), cu(times), 2.0, K, 0.4, H, W, want_xy=True, want_iwe=False)
    xy = w["xy"]
    r = ops.event_voxel_grid(xy[:, 0], xy[:, 1], cu(t), cu(p), H, W, subpixel=True)
    xyh = xy.cpu().numpy()
    n_nan = int(np.isnan(xyh).any(-1).sum())
    assert n_nan >= len(x[::97]) and int(r["status"][2]) == n_nan
    _check(xyh[:, 0], xyh[:, 1], t, p, H, W, 5, subpixel=True)
    ref = voxelref.voxel_grid(xyh[:, 0], xyh[:, 1], t, p, H, W, 5, subpixel=True)
    assert _within_one_ulp(r["grid"].cpu().numpy(), ref["grid"][0]) and np.array_equal(r["status"].cpu().numpy(), ref["status"])


# ------------------------------------------------------------------------------------------------ 6. status and memory
def test_status_words():
    from rampvo_amd import ops
    x, y, t, p = _events(14, 1000, margin=3.0)
    x[5], y[6], t[7], t[8] = np.nan, np.inf, np.nan, -np.inf
    ref = _check(x, y, t, p, H, W, 5)
    r = ops.event_voxel_grid(cu(x), cu(y), cu(t), cu(p), H, W)
    s = ops.event_voxel_status(r["status"])
    assert s == dict(bad_offsets=False, bad_times=False, n_events=1000, n_not_finite=4, n_outside=int(ref["status"][3]),
                     n_no_bin=int(ref["status"][4]), n_contributed=int(ref["status"][5]))
    assert s["n_outside"] > 100 and s["n_no_bin"] > 50 and s["n_not_finite"] + s["n_outside"] + s["n_no_bin"] + s["n_contributed"] == 1000
    off = ops.event_slices(1000, 300)
    assert off.dtype == torch.int64 and off.is_cuda and off.tolist() == [0, 300, 600, 900]       # (the partial slice is dropped)
    assert ops.event_voxel_grid(cu(x), cu(y), cu(t), cu(p), H, W, offsets=off)["grid"].shape == (3, 5, H, W)
    assert r["grid"].shape == (5, H, W)                                       # what the net takes as events[None, None]


def test_chunking_canaries_and_the_accumulators():
    """the C entry with guard words on both sides of every output and of the workspace: a workspace that holds one slice and
    one that holds all three give the same bits; the int64 accumulators in the workspace are the emulator's"""
    from rampvo_amd import _lib
    L = _lib.lib()
    N, S, bins = 900, 3, 5
    x, y, t, p = _events(15, N)
    off = np.array([0, 250, 250, 900], np.int64)
    dx, dy, dt, dp, doff = cu(x), cu(y), cu(t), cu(p), cu(off)
    one, three = (L.ramp_event_voxel_workspace_bytes(s, bins, H, W) for s in (1, 3))
    C = bins * H * W

    res = {}
    for nbytes in (one, three, three + 4096):
        bufs = dict(grid=Flat(S * C, torch.float32, -7.0), stats=Flat(4 * S, torch.float64, -7.0),
                    status=Flat(8, torch.int32, -7), ws=Flat(nbytes, torch.uint8, 0xA5))
        assert bufs["ws"].t.data_ptr() % 16 == 0
        for flags in (0, _lib.RAMP_VOXEL_NORMALIZE | _lib.RAMP_VOXEL_SUBPIXEL):
            rc = L.ramp_event_voxel(_lib.ptr(dx), _lib.ptr(dy), _lib.ptr(dt), _lib.ptr(dp), N, _lib.ptr(doff), S, bins, H, W, flags,
                                    _lib.ptr(bufs["grid"].t), _lib.ptr(bufs["stats"].t), _lib.ptr(bufs["status"].t),
                                    _lib.ptr(bufs["ws"].t), nbytes, _lib.stream())
            torch.cuda.synchronize()
            assert rc == 0
            for k, b in bufs.items():
                assert b.intact(), k
            res[nbytes, flags] = {k: bufs[k].t.cpu().numpy().copy() for k in ("grid", "stats", "status")}
        if nbytes == three:                                                  # all slices at once: counters, n and sum, accumulators
            words = bufs["ws"].t.cpu().numpy()
            acc = words[64 + 16 * S:64 + 16 * S + 8 * S * C].view(np.int64).reshape(S, bins, H, W)
            ref = voxelref.accumulate(x, y, t, p, H, W, bins, offsets=off, subpixel=True)
            assert np.array_equal(acc, ref["acc"])
            sums = words[64:64 + 16 * S].view(np.int64).reshape(S, 2)
            assert np.array_equal(sums[:, 0], (ref["acc"] != 0).sum((1, 2, 3))) and np.array_equal(sums[:, 1], ref["acc"].sum((1, 2, 3)))
    for flags in (0, _lib.RAMP_VOXEL_NORMALIZE | _lib.RAMP_VOXEL_SUBPIXEL):
        for k in ("grid", "stats", "status"):
            assert georef.same_bits(res[one, flags][k], res[three, flags][k]), k
            assert georef.same_bits(res[three + 4096, flags][k], res[three, flags][k]), k
    ref = voxelref.voxel_grid(x, y, t, p, H, W, bins, offsets=off, normalize=False)
    assert georef.same_bits(res[one, 0]["grid"].reshape(S, bins, H, W), ref["grid"])
    assert np.array_equal(res[one, 0]["status"], ref["status"])


# ------------------------------------------------------------------------------------------------ 7. tracker
def _tracker_events(f, n_ev=5000):
    x, y, t, p = kit.query_events(f, n_ev)
    return x, y, torch.sort(t).values, p


def _ask(slam, f, frame):
    from rampvo_amd import ops
    x, y, t, p = _tracker_events(f)
    off = ops.event_slices(5000, 2000)
    res = {}
    plain = slam.event_voxel_grid(x, y, t, p, offsets=off, as_tensor=True)
    comp = slam.event_voxel_grid(x, y, t, p, num_bins=3, compensate=True, as_tensor=True)
    res["numpy"] = slam.event_voxel_grid(x, y, t, p, num_bins=3, compensate=True)
    warp = slam.compensate_events(x, y, t, p, want_xy=True, want_iwe=False, as_tensor=True)
    ref = ops.event_voxel_grid(warp["xy"][:, 0], warp["xy"][:, 1], t, p, 240, 320, num_bins=3, subpixel=True)
    ref["warp_status"] = warp["status"]
    res["plain"], res["plain_ref"] = kit.host(plain), kit.host(ops.event_voxel_grid(x, y, t, p, 240, 320, offsets=off))
    res["comp"], res["comp_ref"] = kit.host(comp), kit.host(ref)
    return res


def test_tracker_event_voxel_grid():
    """slam.event_voxel_grid equals ops.event_voxel_grid at the tracker's image size; compensate=True equals
    compensate_events(want_xy) followed by the sub-pixel grid; the tracker stays device resident and ends with the pose bits
    of one never asked"""
    a, c = kit.run_resident(True, _ask), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_after"] and a["resident_at_end"] and c["resident_at_end"]
    kit.same(a["plain"], a["plain_ref"], "against ops.event_voxel_grid")
    kit.same(a["comp"], a["comp_ref"], "against compensate_events + the sub-pixel grid")
    kit.same(a["numpy"], a["comp"], "numpy form")
    assert a["plain"]["grid"].shape == (2, 5, 240, 320) and a["comp"]["grid"].shape == (3, 240, 320)
    assert a["plain"]["status"].tolist()[:2] == [0, 4000] and a["comp"]["status"][0] == 0 and a["comp"]["status"][5] > 2500
    assert a["comp"]["warp_status"][0] == 0 and a["comp"]["stats"][0, 0] > 1000 and np.isfinite(a["comp"]["grid"]).all()
    for f in (kit.T_QUERY + 1, kit.T_QUERY + 2):
        kit.same(a["state", f], c["state", f], "state of a tracker that is never asked, frame %d" % f)


@torch.no_grad()
def test_tracker_event_voxel_grid_host_driven():
    """a host-driven tracker: numpy in, numpy out, the same bits as the parts; bad offsets make the numpy form raise"""
    from rampvo_amd import ops
    slam = kit.tracker(False, False)
    for f, frame in enumerate(kit.frames()):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    x, y, t, p = (v.cpu().numpy() for v in _tracker_events(f, 1000))
    plain = slam.event_voxel_grid(x, y, t, p, normalize=False)
    comp = slam.event_voxel_grid(x, y, t, p, compensate=True)
    assert sorted(plain) == ["grid", "stats", "status"] and sorted(comp) == ["grid", "stats", "status", "warp_status"]
    kit.same(plain, kit.host(ops.event_voxel_grid(cu(x), cu(y), cu(t), cu(p), 240, 320, normalize=False)), "plain")
    warp = slam.compensate_events(cu(x), cu(y), cu(t), cu(p), want_xy=True, want_iwe=False, as_tensor=True)
    ref = ops.event_voxel_grid(warp["xy"][:, 0], warp["xy"][:, 1], cu(t), cu(p), 240, 320, subpixel=True)
    kit.same({k: comp[k] for k in ref}, kit.host(ref), "compensated")
    assert comp["status"][0] == 0 and comp["status"][5] > 500
    with pytest.raises(RuntimeError, match="slice offsets"):
        slam.event_voxel_grid(x, y, t, p, offsets=np.array([0, 600, 500]))
    slam.tlist = slam.tlist[::-1]
    with pytest.raises(RuntimeError, match="time stamps decrease"):
        slam.event_voxel_grid(x, y, t, p, compensate=True)
    del slam
    kit.quiesce()
