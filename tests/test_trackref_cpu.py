"""tests/trackref.py, the numpy restatement of ramp_event_corner_tracks, held to closed forms that are exact in binary, to
"pieces equal whole" and to saturation; the generators of the GPU test hold what they claim; the streams of the GPU test
(trackref.cases) tell every mistake of trackref.MISTAKES from the definition; the entries are declared, exported and bound, and
every refusal of the entry and of the operator comes without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import georef
import trackref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = tr.H0, tr.W0
_cases = {}


def cases():
    if not _cases:
        _cases.update({name: (args, kw) for name, args, kw in tr.cases()})
    return _cases


def run(x, y, t, h=H, w=W, **kw):
    return tr.event_corner_tracks(np.asarray(x), np.asarray(y), np.asarray(t, np.float64), h, w, **kw)


def differs(a, b):
    return any(not (georef.same_bits(a[k], b[k]) if a[k].dtype.kind == "f" else np.array_equal(a[k], b[k])) for k in tr.KEYS)


# ------------------------------------------------------------------------------------------------ 1. closed forms
@pytest.mark.parametrize("step,velocity", (((1, 0), (4.0, 0.0)), ((1, 1), (4.0, 4.0)), ((0, -1), (0.0, -4.0))))
def test_a_corner_stepping_one_pixel_per_quarter(step, velocity):
    k = 9
    x, y, t = 12 + step[0] * np.arange(k), 15 + step[1] * np.arange(k), 2.0 + 0.25 * np.arange(k)
    for r in (1, 3, 5):
        g = run(x, y, t, radius=r, max_dt=0.25, next_id=40)
        assert g["cls"].tolist() == [5] + [7] * (k - 1) and g["parent"].tolist() == [-1] + list(range(k - 1))
        assert (g["track"] == 40).all() and g["length"].tolist() == list(range(1, k + 1)) and g["next_id"][0] == 40 + k
        assert np.isnan(g["velocity"][0]).all() and (g["velocity"][1:] == np.float32(velocity)).all()
        assert (g["birth"] == [2.0, 12.0, 15.0]).all()
        s = tr.unpack_state(g["state"], W)
        assert np.isfinite(s["t"]).sum() == k and s["length"][y[-1], x[-1]] == k and s["track"][y[-1], x[-1]] == 40
        assert (s["t0"][y, x] == 2.0).all() and (s["x0"][y, x] == 12).all() and (s["y0"][y, x] == 15).all()
        assert g["status"].tolist() == [0, k, 0, 0, 0, 1, 0, k - 1]


def test_two_corners_further_apart_than_the_radius():
    x, y, t = np.array([5, 9, 6, 10]), np.array([5, 5, 5, 5]), np.array([0.0, 0.0, 0.25, 0.25])
    g = run(x, y, t, radius=3, max_dt=1.0)
    assert g["track"].tolist() == [0, 1, 0, 1] and g["parent"].tolist() == [-1, -1, 0, 1]
    g = run(x, y, t, radius=4, max_dt=1.0)                          # 4 pixels apart: one track (event 2 takes the nearer of two equal t')
    assert g["parent"].tolist() == [-1, 0, 0, 2] and g["track"].tolist() == [0, 0, 0, 0]


def test_the_gap_max_dt_links_and_the_next_float_does_not():
    max_dt = 0.3                                                    # (not exact in binary: the subtraction is what is compared)
    for t1 in (1.0, 1024.0):
        t2 = t1 + max_dt
        while t2 - t1 > max_dt:
            t2 = np.nextafter(t2, -np.inf)
        assert t2 - t1 <= max_dt < np.nextafter(t2, np.inf) - t1
        assert run([4, 5], [4, 4], [t1, t2], radius=1, max_dt=max_dt)["cls"].tolist() == [5, 7]
        assert run([4, 5], [4, 4], [t1, np.nextafter(t2, np.inf)], radius=1, max_dt=max_dt)["cls"].tolist() == [5, 5]
    assert run([4, 5], [4, 4], [0.0, 0.0], radius=1, max_dt=0.0)["cls"].tolist() == [5, 7]
    assert run([4, 5], [4, 4], [-1e300, 1e300], radius=1, max_dt=np.inf)["cls"].tolist() == [5, 7]


def test_the_tie_rule():
    # equal t' at two distances: the nearer; the newest first, whatever the distance
    g = run([10, 13, 12], [10, 10, 10], [1.0, 1.0, 2.0], radius=3, max_dt=5.0)
    assert g["parent"].tolist() == [-1, 0, 1]
    g = run([10, 13, 11], [10, 10, 10], [1.0, 1.0, 2.0], radius=3, max_dt=5.0)
    assert g["parent"].tolist() == [-1, 0, 0]
    g = run([10, 13, 11], [10, 10, 10], [1.0, 1.5, 2.0], radius=3, max_dt=5.0)
    assert g["parent"].tolist() == [-1, 0, 1]
    # equal t' at equal distance: the lowest j, rows first
    g = run([10, 12, 11], [10, 10, 10], [1.0, 1.0, 2.0], radius=1, max_dt=5.0)        # j = 3 (dx = -1) and j = 5 (dx = +1)
    assert g["parent"].tolist() == [-1, -1, 0]
    g = run([11, 10, 11], [11, 10, 10], [1.0, 1.0, 2.0], radius=1, max_dt=5.0)        # (0, +1): j = 7, (-1, 0): j = 3
    assert g["parent"].tolist() == [-1, 0, 1]
    g = run([11, 11, 11], [11, 9, 10], [1.0, 1.0, 2.0], radius=1, max_dt=5.0)         # (0, +1): j = 7, (0, -1): j = 1
    assert g["parent"].tolist() == [-1, -1, 1]
    # a state record and an event of this call compete on equal terms
    state = tr.empty_state(H, W)
    state[10, 10] = tr.pack_state(1.0, 7, 0.5, 2, 3, 4, W)
    g = run([12, 11], [10, 10], [1.0, 2.0], radius=1, max_dt=5.0, state=state, next_id=50)
    assert g["parent"].tolist() == [-1, -2] and g["track"].tolist() == [50, 7] and g["length"].tolist() == [1, 5]
    assert georef.same_bits(g["velocity"][1], np.array([(11 - 2) / 1.5, (10 - 3) / 1.5], np.float32))


def test_the_own_pixel_continues_a_track_and_the_planes_do_not_mix():
    g = run([7, 7, 7], [8, 8, 8], [1.0, 1.0, 3.0], radius=0, max_dt=2.0)
    assert g["parent"].tolist() == [-1, 0, 1] and g["length"].tolist() == [1, 2, 3] and np.isnan(g["velocity"][:2]).all()
    assert (g["velocity"][2] == 0).all()
    g = run([7, 8, 7, 8], [8, 8, 8, 8], [1.0, 2.0, 3.0, 4.0], p=[1, -1, 1, 0], radius=2, max_dt=9.0)
    assert g["parent"].tolist() == [-1, -1, 0, 1] and g["track"].tolist() == [0, 1, 0, 1] and g["state"].shape == (2, H, W, 4)
    assert run([7, 8, 7, 8], [8, 8, 8, 8], [1.0, 2.0, 3.0, 4.0], radius=2, max_dt=9.0)["parent"].tolist() == [-1, 0, 1, 2]


def test_the_window_is_clipped_at_a_corner_of_the_sensor():
    # the event at (0, 1): an unclipped window of radius 1 would run on to (W - 1, 0), the end of the row above
    g = run([W - 1, 0], [0, 1], [1.0, 2.0], radius=1, max_dt=5.0)
    assert g["parent"].tolist() == [-1, -1]
    g = run([W - 1, W - 2, 0, 1], [H - 1, H - 2, 0, 1], [1.0, 2.0, 3.0, 4.0], radius=5, max_dt=5.0)
    assert g["parent"].tolist() == [-1, 0, -1, 2]
    assert run([0, 0], [0, 0], [1.0, 1.0], h=1, w=1, radius=5, max_dt=0.0)["parent"].tolist() == [-1, 0]


def test_non_candidates_and_invalid_events_take_no_part():
    x, y, t = [5, 6, 6, np.nan, 40, 7], [5, 5, 5, 5, 5, 5], [1.0, 2.0, 2.5, 2.6, 2.7, 3.0]
    g = run(np.array(x, np.float32), y, t, corner=[1, 0, 255, 1, 1, 1], radius=1, max_dt=5.0)
    assert g["cls"].tolist() == [5, 4, 7, 2, 3, 7] and g["parent"].tolist() == [-1, -1, 0, -1, -1, 2]
    assert g["track"].tolist() == [0, -1, 0, -1, -1, 0] and g["length"].tolist() == [1, 0, 2, 0, 0, 3]
    assert np.isnan(g["birth"][[1, 3, 4]]).all() and np.isnan(g["velocity"][[1, 3, 4]]).all() and g["next_id"][0] == 6
    assert g["status"].tolist() == [0, 6, 1, 1, 1, 1, 0, 2]
    # the non-candidate's later time stamp at (6, 5) neither shows in the state nor breaks the order
    g = run([6, 6], [5, 5], [2.0, 1.0], corner=[0, 1], radius=1, max_dt=5.0)
    assert g["status"][0] == 0 and tr.unpack_state(g["state"], W)["t"][5, 6] == 1.0


def test_bad_order_and_the_empty_call():
    state = tr.empty_state(H, W)
    state[5, 6] = tr.pack_state(3.0, 7, 0.5, 2, 3, 4, W)
    for g in (run([6, 6], [5, 5], [2.0, 1.0], radius=1, max_dt=5.0, next_id=9), run([6], [5], [2.5], radius=1, max_dt=5.0, state=state, next_id=9)):
        n = len(g["cls"])
        assert g["status"].tolist() == [1, n, 0, 0, 0, 0, 0, 0] and not g["cls"].any() and not g["length"].any()
        assert (g["parent"] == -1).all() and (g["track"] == -1).all() and np.isnan(g["birth"]).all() and np.isnan(g["velocity"]).all()
        assert np.array_equal(g["state"], tr.empty_state(H, W)) and g["next_id"][0] == 9 + n
    e = run([], [], [], radius=1, max_dt=5.0, state=state, next_id=9)
    assert np.array_equal(e["state"], state) and e["next_id"][0] == 9 and not e["status"].any()


# ------------------------------------------------------------------------------------------------ 2. pieces, saturation
@pytest.mark.parametrize("cuts", ((1,), (2000,), (1000, 1001, 3000), (4098,)))
def test_pieces_equal_whole(cuts):
    x, y, t, p, c = tr.mixed(4099)
    kw = dict(radius=3, max_dt=6 * tr.TICK)
    whole = tr.event_corner_tracks(x, y, t, H, W, corner=c, p=p, **kw)
    parts = tr.in_pieces(x, y, t, H, W, cuts, corner=c, p=p, **kw)
    for k in ("track", "length", "birth", "velocity", "state", "next_id"):
        assert georef.same_bits(parts[k], whole[k]) if whole[k].dtype.kind == "f" else np.array_equal(parts[k], whole[k]), k
    # a link across a cut is class 6 and parent -2 in the pieces, class 7 and an index in the whole: nothing else differs
    across = parts["cls"] != whole["cls"]
    assert (parts["cls"][across] == 6).all() and (whole["cls"][across] == 7).all() and (parts["parent"][across] == -2).all()
    assert np.array_equal(parts["parent"][~across], whole["parent"][~across]) and (len(cuts) == 1 or across.sum() > 10)
    assert np.array_equal(parts["status"][:5], whole["status"][:5]) and parts["status"][5] == whole["status"][5]


def test_saturation():
    x, y, t, state = tr.saturating()
    g = run(x, y, t, radius=3, max_dt=1.0, state=state, next_id=100)
    assert g["cls"].tolist() == [6, 7] and g["length"].tolist() == [tr.LEN_MAX, tr.LEN_MAX] and g["track"].tolist() == [77, 77]
    s = tr.unpack_state(g["state"], W)
    assert s["length"][11, 14] == tr.LEN_MAX and s["length"][10, 12] == tr.LEN_MAX - 1 and (s["x0"][11, 14], s["y0"][11, 14]) == (3, 4)
    assert g["velocity"][1].tolist() == [np.float32(11 / 4.0), np.float32(7 / 4.0)]


# ------------------------------------------------------------------------------------------------ 3. the generators
def test_the_generators_hold_what_they_claim():
    for n in tr.CHAIN_LINKS:
        x, y, t = tr.chain(n)
        assert len(t) == n + 1 and (np.abs(np.diff(x)) + np.abs(np.diff(y)) == 1).all() and (np.diff(t) == 0.25).all()
        assert x.min() >= 2 and y.min() >= 2 and x.max() <= W - 3 and y.max() <= H - 3
        for r in (1, 2, 3):
            g = run(x, y, t, radius=r, max_dt=0.25)
            assert g["parent"].tolist() == list(range(-1, n)) and g["length"][-1] == n + 1 and (g["track"] == 0).all()
    assert max(tr.CHAIN_LINKS) > 2 ** 12 and len(np.unique(tr.chain(5000)[0] + 100 * tr.chain(5000)[1])) < 1200      # cells are revisited
    x, y, t = tr.stars(1250)
    g = run(x, y, t, radius=5, max_dt=4.5)
    assert np.array_equal(g["parent"], np.where(np.arange(6250) % 5 == 0, -1, np.arange(6250) // 5 * 5)) and (g["cls"] == 7).sum() == 5000
    assert (np.bincount(g["parent"][g["parent"] >= 0]).max() == 4) and g["length"].max() == 2
    x, y, t, p, c = tr.mixed(4099)
    assert (np.diff(t[np.isfinite(t)]) >= 0).all() and (np.diff(t) == 0).sum() > 100 and 0.6 < (c != 0).mean() < 0.9 and c.max() > 1
    classes = set()
    for name, (args, kw) in cases().items():
        g = tr.event_corner_tracks(*args, H, W, **kw)
        assert g["status"][0] == 0 and g["status"][2:].sum() == g["status"][1] == len(args[2]), name
        classes |= {k for k in range(2, 8) if g["status"][k] > 0}
        if name.startswith("mixed r=") or name == "mixed, second call":
            assert (g["status"][2:6] > 0).all() and g["status"][7] > 0, name
    assert classes == {2, 3, 4, 5, 6, 7}
    assert cases()["mixed, second call"][1]["next_id"] == 2000
    for name, wx, wy, wt, wp, wc in tr.wedge_masks():
        assert 10 < wc.sum() < len(wc) / 4, name
    perm = tr.cornerref.shuffle_keeping_cells(np.where(np.isfinite(x), x, 0), y, p, np.random.default_rng(2))
    assert (np.diff(t[perm][np.isfinite(t[perm])]) < 0).sum() > 500


# ------------------------------------------------------------------------------------------------ 4. the mistakes
@pytest.mark.parametrize("mistake", tr.MISTAKES)
def test_the_gpu_streams_reject_the_mistake(mistake):
    assert len(tr.MISTAKES) >= 10
    rejected = [name for name, (args, kw) in cases().items()
                if differs(tr.event_corner_tracks(*args, H, W, **kw), tr.event_corner_tracks(*args, H, W, mistake=mistake, **kw))]
    assert rejected, mistake


# ------------------------------------------------------------------------------------------------ 5. the C entries, ops
def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_event_corner_tracks", "ramp_event_corner_tracks_ws_bytes", "ramp_event_corner_tracks_grid_events"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert not any(n.startswith("ramp_event_corner_tracks") and n.endswith("_workspace_bytes") for n in _lib.SIGNATURES)
    assert _lib.RAMP_CORNER_TRACK_XY_I32 == 1 and _lib.RAMP_CORNER_TRACK_BAD_ORDER == _lib.RAMP_FILTER_BAD_ORDER == tr.BAD_ORDER
    assert ops._STATUS["event_corner_tracks"][0]["bad_order"] is ops._STATUS["event_filter"][0]["bad_order"]      # one row
    assert ops._STATUS["event_corner_tracks"][1] == ("n_events", "n_not_finite", "n_outside", "n_not_corner", "n_born", "n_carried",
                                                     "n_linked")
    assert "event_corner_tracks" not in ops.STATUS_ROLES.values() and len(ops.STATUS_ORDER) == 16
    assert lib.ramp_event_corner_tracks_grid_events() == lib.ramp_event_corners_grid_events()
    one_, two = lib.ramp_event_corner_tracks_ws_bytes(1000, H, W, 1), lib.ramp_event_corner_tracks_ws_bytes(1000, H, W, 2)
    assert one_ % 256 == 0 and 0 < two - one_ <= 4 * H * W + 256 and lib.ramp_event_corner_tracks_ws_bytes(1000, H, W, 3) == 0
    assert lib.ramp_event_corner_tracks_ws_bytes(1000, 1 << 15, 1 << 15, 1) == 0 and lib.ramp_event_corner_tracks_ws_bytes(0, 8, 8, 1) > 0
    # per event beyond the corners': the parents (4 bytes), the roots' records (24), the two jump buffers (8 each)
    more = lambda n: lib.ramp_event_corner_tracks_ws_bytes(n, H, W, 1) - lib.ramp_event_corners_ws_bytes(n, H, W, 1)
    assert more(1 << 16) == 44 << 16
    assert all(callable(f) for f in (ops.event_corner_tracks, ops.event_corner_tracks_status, ops.corner_track_state,
                                     TrackerQueries.event_corner_tracks, TrackerQueries.reset_event_corner_tracks))
    assert "cornertrack.hip" in open(os.path.join(ROOT, "rampvo_amd", "csrc", "Makefile")).read()


def test_argument_checks_that_need_no_gpu():
    """every refusal comes before anything touches the device (the pointers are never read)"""
    from rampvo_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    odd4, odd2 = ctypes.c_void_p(q.value + 4), ctypes.c_void_p(q.value + 2)

    def call(N=10, H=13, W=17, flags=0, rho=3, max_dt=1.0, p=None, corner=None, state_in=None, next_in=None, state_out=q, next_out=q,
             cls=q, parent=None, track=None, length=None, birth=None, velocity=None, status=q, ws=q, x=q, y=q, t=q, ws_bytes=0):
        return lib.ramp_event_corner_tracks(x, y, t, p, corner, N, H, W, flags, rho, max_dt, state_in, next_in, state_out, next_out,
                                            cls, parent, track, length, birth, velocity, status, ws, ws_bytes, None)

    for kw in (dict(N=-1), dict(H=0), dict(W=0), dict(flags=2), dict(flags=-1), dict(rho=-1), dict(rho=6), dict(max_dt=-1e-300),
               dict(max_dt=float("nan")), dict(max_dt=-float("inf")), dict(status=None), dict(cls=None), dict(state_out=None),
               dict(next_out=None), dict(x=None), dict(y=None), dict(t=None), dict(ws=None), dict(state_in=q), dict(next_in=q),
               dict(state_in=odd4, next_in=q), dict(state_in=q, next_in=odd4), dict(state_out=odd4), dict(next_out=odd4),
               dict(track=odd4), dict(birth=odd4), dict(status=odd2), dict(parent=odd2), dict(length=odd2), dict(velocity=odd2),
               dict(t=odd4), dict(x=odd2), dict(ws=ctypes.c_void_p(q.value + 8))):
        assert call(**kw) == _lib.RAMP_EINVAL, kw
    full = lib.ramp_event_corner_tracks_ws_bytes(10, 13, 17, 1)
    assert call() == _lib.RAMP_EWORKSPACE and call(ws_bytes=full - 1) == _lib.RAMP_EWORKSPACE
    assert call(p=q, ws_bytes=full) == _lib.RAMP_EWORKSPACE          # two planes need more
    assert call(N=1 << 31) == _lib.RAMP_EUNSUPPORTED and call(H=1 << 15, W=1 << 15) == _lib.RAMP_EUNSUPPORTED
    for kw in (dict(flags=1), dict(rho=0), dict(rho=5), dict(max_dt=0.0), dict(max_dt=float("inf")), dict(corner=odd2),
               dict(state_in=q, next_in=q, parent=q, track=q, length=q, birth=q, velocity=odd4)):
        assert call(**kw) == _lib.RAMP_EWORKSPACE, kw               # valid: refused only for the workspace it was not given


def test_ops_refusals_need_no_gpu():
    import torch
    from rampvo_amd import ops
    x = torch.zeros(4)
    state, nid = torch.zeros((13, 17, 4), dtype=torch.int64), torch.zeros(1, dtype=torch.int64)
    good = dict(x=x, y=x, t=x.double(), height=13, width=17, max_dt=1.0)
    for kw, text in ((dict(height=0), "positive"), (dict(radius=6), "radius is"), (dict(radius=-1), "radius is"), (dict(radius=1.5), "radius is"),
                     (dict(max_dt=None), "max_dt is required"), (dict(max_dt=-1.0), "max_dt is not"), (dict(max_dt=float("nan")), "max_dt is not"),
                     (dict(t=torch.zeros(3).double()), "differ in length"), (dict(p=torch.zeros(3)), "differ in length"),
                     (dict(corner=torch.zeros(5)), "differ in length"), (dict(state=state), "go together"), (dict(next_id=nid), "go together"),
                     (dict(state=state.double(), next_id=nid), "int64"), (dict(p=x, state=state, next_id=nid), r"\[2, height, width, 4\]"),
                     (dict(state=state, next_id=nid.int()), r"next_id is int64 \[1\]"), (dict(state=state, next_id=nid), "GPU only"),
                     (dict(), "GPU only")):
        with pytest.raises(RuntimeError, match=text):
            ops.event_corner_tracks(**{**good, **kw})
    assert ops.event_corner_tracks_status(torch.tensor([1, 9, 1, 2, 3, 1, 1, 1], dtype=torch.int32)) == dict(
        bad_order=True, n_events=9, n_not_finite=1, n_outside=2, n_not_corner=3, n_born=1, n_carried=1, n_linked=1)
    packed = tr.pack_state(np.array([[1.5, np.nan]]), np.array([[7, 0]]), np.array([[0.5, 0.0]]), np.array([[1, 0]]), np.array([[0, 0]]),
                           np.array([[tr.LEN_MAX, 0]]), 2)
    s = ops.corner_track_state(torch.from_numpy(packed))
    assert s["t"][0, 0] == 1.5 and torch.isnan(s["t"][0, 1]) and s["track"][0, 0] == 7 and s["t0"][0, 0] == 0.5
    assert (s["x0"][0, 0], s["y0"][0, 0], s["length"][0, 0]) == (1, 0, tr.LEN_MAX) and s["length"].dtype == torch.int32
    with pytest.raises(RuntimeError, match="int64"):
        ops.corner_track_state(torch.zeros((3, 3, 4)))
