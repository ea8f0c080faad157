"""ramp_event_corner_tracks (csrc/cornertrack.hip) against tests/trackref.py -- one sweep over a per-cell record map, restated in
numpy without the kernel's sort, searches and pointer jumping.  Everything is EXACT: cls, parent, track, length, birth, velocity,
the state, next_id and every status word, bit for bit.  No tolerance in this file.

Most cases call the C entry directly, with a guard band in front of and behind every output, and launch twice.

The issue's "star of 5,000 children on one root" cannot exist under the definition: two children of one parent must not see
each other (the newer one would take the older, which is newer than the parent), yet both lie in the parent's window, so with
distinct time stamps a parent has at most four children (the corners of its window).  ``trackref.stars`` is 1,250 such maximal
stars, 5,000 children in all, on cells that are used 1,250 times each; 5,000 lanes reading ONE root is the chain of 5,000."""
import ctypes

import numpy as np
import pytest
import torch

import cornerref as cr
import filterref as fr
import georef
import trackerkit as kit
import trackref as tr
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = tr.H0, tr.W0
_cases = {}


def cases():
    if not _cases:
        _cases.update({name: (args, kw) for name, args, kw in tr.cases()})
    return _cases


def entry(x, y, t, p, corner, N, h, w, flags, rho, max_dt, state_in, next_in, state_out, next_out, cls, parent, track, length, birth,
          velocity, status, ws, ws_bytes):
    from rampvo_amd import _lib
    q = lambda v: v if (v is None or isinstance(v, (int, ctypes.c_void_p))) else _lib.ptr(v)
    return _lib.lib().ramp_event_corner_tracks(q(x), q(y), q(t), q(p), q(corner), N, h, w, flags, rho, max_dt, q(state_in), q(next_in),
                                               q(state_out), q(next_out), q(cls), q(parent), q(track), q(length), q(birth),
                                               q(velocity), q(status), q(ws), ws_bytes, _lib.stream())


def call(x, y, t, h=H, w=W, corner=None, p=None, radius=3, max_dt=None, state=None, next_id=0, inplace=False):
    """the C entry with every output requested and guarded, launched twice (the second launch's bits are the first's) -> the
    outputs on the host (N == 0 without a state: what the entry leaves untouched is filled in as ops.event_corner_tracks does)"""
    from rampvo_amd import _lib
    x, y = np.asarray(x), np.asarray(y)
    integer = x.dtype.kind in "iu"
    xd, yd = (cu(v.astype(np.int32 if integer else np.float32)) for v in (x, y))
    td = cu(np.asarray(t, np.float64))
    N, S = len(td), 1 if p is None else 2
    pd = None if p is None else cu(np.asarray(p, np.int8) if N else np.zeros(1, np.int8))     # (N == 0: p not NULL says two planes)
    cd = None if corner is None else cu(np.asarray(corner, np.uint8) if N else np.zeros(1, np.uint8))
    nbytes = _lib.lib().ramp_event_corner_tracks_ws_bytes(N, h, w, S)
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        bufs = {k: Flat(n, d) for k, (n, d) in dict(cls=(N, torch.uint8), parent=(N, torch.int32), track=(N, torch.int64),
                                                    length=(N, torch.int32), birth=(N * 3, torch.float64), velocity=(N * 2, torch.float32),
                                                    status=(8, torch.int32), state=(S * h * w * 4, torch.int64),
                                                    next_id=(1, torch.int64)).items()}
        at = {k: ctypes.c_void_p(b.address()) for k, b in bufs.items()}          # (an empty view has no pointer)
        state_in = next_in = None
        if state is not None:
            if inplace:
                bufs["state"].t.copy_(cu(np.asarray(state, np.int64).reshape(-1)))
                bufs["next_id"].t.fill_(next_id)
                state_in, next_in = at["state"], at["next_id"]
            else:
                state_in, next_in = cu(np.asarray(state, np.int64)), cu(np.array([next_id], np.int64))
        rc = entry(xd, yd, td, pd, cd, N, h, w, _lib.RAMP_CORNER_TRACK_XY_I32 if integer else 0, radius, max_dt, state_in, next_in,
                   at["state"], at["next_id"], at["cls"], at["parent"], at["track"], at["length"], at["birth"], at["velocity"],
                   at["status"], ws, nbytes)
        assert rc == 0, rc
        torch.cuda.synchronize()
        for k, b in bufs.items():
            assert b.intact(), "guard band of " + k
        res = {k: b.t.cpu().numpy() for k, b in bufs.items()}
        if N == 0 and state is None:
            assert (res["state"] == bufs["state"].canary).all() and res["next_id"][0] == bufs["next_id"].canary
            res["state"], res["next_id"] = tr.empty_state(h, w, S).reshape(-1), np.zeros(1, np.int64)
        res.update(birth=res["birth"].reshape(N, 3), velocity=res["velocity"].reshape(N, 2),
                   state=res["state"].reshape((h, w, 4) if p is None else (2, h, w, 4)))
        runs.append(res)
    same(runs[1], runs[0], "second launch")
    return runs[0]


def same(got, ref, what=""):
    for k in tr.KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, "%s %s" % (what, k)
        assert georef.same_bits(got[k], ref[k]) if ref[k].dtype.kind == "f" else np.array_equal(got[k], ref[k]), "%s %s" % (what, k)
    assert got["status"][2:].sum() == got["status"][1] or got["status"][0] != 0


def check(x, y, t, h=H, w=W, what="", **kw):
    got = call(x, y, t, h, w, **kw)
    kw.pop("inplace", None)
    same(got, tr.event_corner_tracks(x, y, t, h, w, **kw), what)
    return got


# ------------------------------------------------------------------------------------------------ 1. sizes, paths, parameters
@pytest.mark.parametrize("N", (0, 1, 2, 4099))
def test_sizes(N):
    x, y, t, p, c = tr.mixed(4099, bad=False)
    g = check(x[:N], y[:N], t[:N], corner=c[:N], p=p[:N], radius=3, max_dt=6 * tr.TICK)
    check(x[:N], y[:N], t[:N], radius=3, max_dt=6 * tr.TICK)
    if N == 4099:
        assert g["status"][0] == 0 and g["status"][5] > 20 and g["status"][7] > 1000 and g["length"].max() > 20


def test_second_trip():
    from rampvo_amd import _lib
    N = _lib.lib().ramp_event_corner_tracks_grid_events() + 1
    assert N == 2048 * 256 + 1
    x, y, t, p, c = tr.mixed(N)
    g = check(x, y, t, corner=c, p=p, radius=1, max_dt=2 * tr.TICK)
    assert g["status"][1] == N and (g["status"][2:] != 0).sum() == 5 and (g["status"][[2, 3, 4, 5, 7]] > 100).all() and g["next_id"][0] == N


@pytest.mark.parametrize("name", [n for n, _, _ in tr.cases() if not n.startswith(("chain", "wedge", "stars"))])
def test_streams(name):
    """radius 0, 1, 3, 5; with and without p and corner; int32 and fp32; a second call on a state; one time stamp; events that
    are not finite; saturation"""
    args, kw = cases()[name]
    g = check(*args, what=name, **kw)
    assert g["status"][0] == 0
    if name == "saturation":
        assert g["length"].tolist() == [tr.LEN_MAX] * 2
    if name == "mixed, corner alone, integers":
        frac = lambda v, d: np.where(v >= 0, v + np.float32(d), v).astype(np.float32)      # (-1 + 0.5 would truncate onto the sensor)
        f = call(frac(args[0], 0.5), frac(args[1], 0.25), args[2], **kw)
        same(f, g, "fractions take no part")


@pytest.mark.parametrize("n", tr.CHAIN_LINKS)
def test_chains(n):
    """one chain of n links: the pointer-jumping round edges, in time order and shuffled across cells"""
    args, kw = cases()["chain %d" % n]
    g = check(*args, what="chain", **kw)
    assert g["length"][-1] == n + 1 and (g["track"] == 0).all() and g["status"].tolist() == [0, n + 1, 0, 0, 0, 1, 0, n]
    x, y, t = args
    perm = cr.shuffle_keeping_cells(x, y, np.zeros(len(x)), np.random.default_rng(n))
    s = check(x[perm], y[perm], t[perm], what="shuffled chain", **kw)
    assert np.array_equal(s["length"], g["length"][perm])
    assert (s["track"] == np.nonzero(perm == 0)[0][0]).all() and georef.same_bits(s["velocity"], g["velocity"][perm])


def test_stars():
    args, kw = cases()["stars"]
    g = check(*args, what="stars", **kw)
    assert g["status"].tolist() == [0, 6250, 0, 0, 0, 1250, 0, 5000] and g["length"].max() == 2


@pytest.mark.parametrize("k", range(10))
def test_wedge_streams_with_the_detectors_own_mask(k):
    from rampvo_amd import ops
    name, x, y, t, p = cr.wedges()[k]
    mask = ops.event_corners(cu(x), cu(y), cu(t), H, W)["corner"].cpu().numpy().astype(np.uint8)
    assert np.array_equal(mask, tr.wedge_masks()[k][5]) and mask.sum() > 10
    for key in ("wedge " + name, "wedge p " + name):
        args, kw = cases()[key]
        g = check(*args, what=key, **kw)
        assert g["status"][7] > 10 and g["length"].max() >= 5


def test_per_cell_sorted_globally_shuffled():
    x, y, t, p, c = tr.mixed(4099)
    t = np.where(np.isfinite(t), t + np.arange(4099) * 2.0 ** -36, t)          # distinct: no order across cells is left to the index
    keep = np.isfinite(x)
    perm = cr.shuffle_keeping_cells(np.where(keep, x, 0), y, p, np.random.default_rng(2))
    assert (np.diff(t[perm][np.isfinite(t[perm])]) < 0).sum() > 1000
    kw = dict(radius=3, max_dt=6 * tr.TICK)
    a, g = call(x, y, t, corner=c, p=p, **kw), check(x[perm], y[perm], t[perm], corner=c[perm], p=p[perm], **kw)
    assert g["status"][0] == 0 and a["status"][0] == 0 and a["status"][7] > 1000
    for k in ("cls", "length"):
        assert np.array_equal(g[k], a[k][perm]), k
    assert georef.same_bits(g["birth"], a["birth"][perm]) and georef.same_bits(g["velocity"], a["velocity"][perm])
    inv = np.argsort(perm)
    assert np.array_equal(g["parent"], np.where(a["parent"][perm] >= 0, inv[np.maximum(a["parent"][perm], 0)], a["parent"][perm]))
    assert np.array_equal(g["track"], np.where(a["track"][perm] >= 0, inv[np.maximum(a["track"][perm], 0)], -1))    # the id is the root's index


# ------------------------------------------------------------------------------------------------ 2. state, order
@pytest.mark.parametrize("cut", (1, 4099 // 2, 4098))
def test_state_across_two_calls_against_the_whole_stream(cut):
    x, y, t, p, c = tr.mixed(4099)
    kw = dict(radius=3, max_dt=6 * tr.TICK)
    whole = call(x, y, t, corner=c, p=p, **kw)
    a = check(x[:cut], y[:cut], t[:cut], corner=c[:cut], p=p[:cut], **kw)
    b = check(x[cut:], y[cut:], t[cut:], corner=c[cut:], p=p[cut:], state=a["state"], next_id=int(a["next_id"][0]), **kw)
    for k in ("track", "length"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    for k in ("birth", "velocity"):
        assert georef.same_bits(np.concatenate([a[k], b[k]]), whole[k]), k
    assert np.array_equal(b["state"], whole["state"]) and b["next_id"][0] == whole["next_id"][0] == 4099
    assert np.array_equal(a["status"][1:6] + b["status"][1:6], whole["status"][1:6])
    assert b["status"][6] + b["status"][7] + a["status"][7] == whole["status"][7]


def test_state_in_place_and_the_empty_call():
    x, y, t, p, c = tr.mixed(4099)
    kw = dict(radius=3, max_dt=6 * tr.TICK)
    first = call(x[:2000], y[:2000], t[:2000], corner=c[:2000], p=p[:2000], **kw)
    rest = dict(corner=c[2000:], p=p[2000:], state=first["state"], next_id=2000, **kw)
    apart = check(x[2000:], y[2000:], t[2000:], **rest)
    same(check(x[2000:], y[2000:], t[2000:], inplace=True, **rest), apart, "state_out == state_in")
    assert apart["status"][6] > 10
    for extra in (dict(), dict(inplace=True)):
        e = check(x[:0], y[:0], t[:0], corner=c[:0], p=p[:0], state=first["state"], next_id=2000, **kw, **extra)
        assert np.array_equal(e["state"], first["state"]) and e["next_id"][0] == 2000 and not e["status"].any()


def _bad_order_outputs(g, N, n2=0, n3=0, next_id=0):
    assert g["status"].tolist() == [1, N, n2, n3, 0, 0, 0, 0]
    assert not g["cls"].any() and not g["length"].any() and (g["parent"] == -1).all() and (g["track"] == -1).all()
    assert np.isnan(g["birth"]).all() and np.isnan(g["velocity"]).all() and g["next_id"][0] == next_id + N
    assert np.array_equal(g["state"], tr.empty_state(H, W, g["state"].ndim - 2).reshape(g["state"].shape))


def test_bad_order():
    x, y, t, p, c = (v.copy() for v in tr.mixed(4099, bad=False))
    kw = dict(radius=3, max_dt=6 * tr.TICK)
    cellkey = (p > 0) * H * W + np.trunc(y).astype(int) * W + np.trunc(x).astype(int)
    marked = np.nonzero(c != 0)[0]
    at = [q for q in np.unique(cellkey[marked]) if (cellkey[marked] == q).sum() > 3]
    at = marked[cellkey[marked] == at[len(at) // 2]]
    k = next(k for k in range(1, len(at)) if t[at[k]] > t[at[k - 1]])
    t[at[k]] = np.nextafter(t[at[k - 1]], -1.0)                    # one decrease within one cell, between two candidates
    _bad_order_outputs(check(x, y, t, corner=c, p=p, **kw), 4099)
    c2 = c.copy()
    c2[at[k]] = 0                                                   # the same decrease at an event that is no candidate: in order
    assert check(x, y, t, corner=c2, p=p, **kw)["status"][0] == 0
    x, y, t, p, c = tr.mixed(4099, bad=False)
    first = int(marked[0])
    state = tr.empty_state(H, W, 2)
    q = np.unravel_index(int(cellkey[first]), (2, H, W))
    state[q] = tr.pack_state(np.nextafter(t[first], 1.0), 5, 0.0, 1, 1, 3, W)      # a first candidate before its state
    _bad_order_outputs(check(x, y, t, corner=c, p=p, state=state, next_id=70, **kw), 4099, next_id=70)
    state[q] = tr.pack_state(t[first], 5, t[first] - 1.0, 1, 1, 3, W)
    g = check(x, y, t, corner=c, p=p, state=state, next_id=70, **kw)
    assert g["status"][0] == 0 and g["cls"][first] == 6 and g["track"][first] == 5 and g["length"][first] == 4


# ------------------------------------------------------------------------------------------------ 3. arguments
def test_every_refusal_touches_nothing():
    from rampvo_amd import _lib
    L = _lib.lib()
    N = 100
    x, y, t, p, c = (cu(v[:N]) for v in tr.mixed(4099, bad=False))
    bufs = dict(cls=Flat(N, torch.uint8), parent=Flat(N + 1, torch.int32), track=Flat(N + 1, torch.int64), length=Flat(N + 1, torch.int32),
                birth=Flat(3 * N + 1, torch.float64), velocity=Flat(2 * N + 1, torch.float32), status=Flat(9, torch.int32),
                state=Flat(2 * H * W * 4 + 1, torch.int64), next_id=Flat(2, torch.int64))
    nbytes = L.ramp_event_corner_tracks_ws_bytes(N, H, W, 2)
    assert nbytes > L.ramp_event_corner_tracks_ws_bytes(N, H, W, 1) > 0
    assert [L.ramp_event_corner_tracks_ws_bytes(*a) for a in ((-1, H, W, 1), (N, 0, W, 1), (N, H, W, 0), (N, H, W, 3), (N, 1 << 15, 1 << 15, 1))] == [0] * 5
    ws = Flat(nbytes, torch.uint8, rows=4)
    at = lambda k, off=0: ctypes.c_void_p(bufs[k].address() + off)
    good = dict(x=x, y=y, t=t, p=p, corner=c, N=N, h=H, w=W, flags=0, rho=3, max_dt=1.0, state_in=at("state"), next_in=at("next_id"),
                state_out=at("state"), next_out=at("next_id"), cls=at("cls"), parent=at("parent"), track=at("track"), length=at("length"),
                birth=at("birth"), velocity=at("velocity"), status=at("status"), ws=ctypes.c_void_p(ws.address()), ws_bytes=nbytes)
    snaps = {k: b.snapshot() for k, b in bufs.items()}
    ws_snap = ws.snapshot()
    EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -3, -4
    for change in (dict(N=-1), dict(h=0), dict(w=0), dict(flags=2), dict(flags=-1), dict(rho=-1), dict(rho=6), dict(max_dt=-1.0),
                   dict(max_dt=float("nan")), dict(status=None), dict(cls=None), dict(state_out=None), dict(next_out=None), dict(x=None),
                   dict(y=None), dict(t=None), dict(ws=None), dict(state_in=None), dict(next_in=None), dict(state_in=at("state", 4)),
                   dict(next_in=at("next_id", 4)), dict(state_out=at("state", 4)), dict(next_out=at("next_id", 4)),
                   dict(track=at("track", 4)), dict(birth=at("birth", 4)), dict(status=at("status", 2)), dict(parent=at("parent", 2)),
                   dict(length=at("length", 2)), dict(velocity=at("velocity", 2)), dict(ws=ctypes.c_void_p(ws.address() + 8))):
        assert entry(**dict(good, **change)) == EINVAL, change
    assert entry(**dict(good, ws_bytes=nbytes - 1)) == EWORKSPACE
    assert entry(**dict(good, N=1 << 31)) == EUNSUPPORTED and entry(**dict(good, h=1 << 15, w=1 << 15)) == EUNSUPPORTED
    assert entry(**dict(good, h=(1 << 30), w=1)) == EUNSUPPORTED                 # 2 H W >= 2^31 - 1, with and without p
    torch.cuda.synchronize()
    assert all(b.unchanged(snaps[k]) for k, b in bufs.items()) and ws.unchanged(ws_snap)
    # (the state holds the canary, whose word 0 is a NaN: no track yet)
    assert entry(**dict(good, flags=0, max_dt=float("inf"))) == 0
    assert entry(**dict(good, parent=None, track=None, length=None, birth=None, velocity=None, corner=None, state_in=None, next_in=None)) == 0
    assert entry(**dict(good, N=0, x=None, y=None, t=None, p=None, corner=None, ws=None, ws_bytes=0, cls=None, state_out=None, next_out=None)) == 0
    torch.cuda.synchronize()
    assert all(b.intact() for b in bufs.values())


# ------------------------------------------------------------------------------------------------ 4. the operator, streams
def _op(x, y, t, p=None, corner=None, **kw):
    from rampvo_amd import ops
    for k in ("state", "next_id"):
        if kw.get(k) is not None:
            kw[k] = cu(np.asarray(kw[k], np.int64))
    out = ops.event_corner_tracks(cu(x), cu(y), cu(t), H, W, p=None if p is None else cu(p), corner=None if corner is None else cu(corner),
                                  want_birth=True, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_operator():
    from rampvo_amd import ops
    x, y, t, p, c = tr.mixed(4099)
    kw = dict(radius=3, max_dt=6 * tr.TICK)
    a = _op(x[:2000], y[:2000], t[:2000], p[:2000], c[:2000], **kw)
    same(a, tr.event_corner_tracks(x[:2000], y[:2000], t[:2000], H, W, p=p[:2000], corner=c[:2000], **kw), "ops first half")
    b = _op(x[2000:], y[2000:], t[2000:], p[2000:], c[2000:] != 0, state=a["state"], next_id=a["next_id"], **kw)
    same(b, tr.event_corner_tracks(x[2000:], y[2000:], t[2000:], H, W, p=p[2000:], corner=c[2000:], state=a["state"], next_id=2000, **kw),
         "ops second half")
    same(_op(x[:0], y[:0], t[:0], p[:0], **kw), tr.event_corner_tracks(x[:0], y[:0], t[:0], H, W, p=p[:0], **kw), "empty")
    same(_op(x[:0], y[:0], t[:0], state=a["state"][0], next_id=a["next_id"], **kw),
         tr.event_corner_tracks(x[:0], y[:0], t[:0], H, W, state=a["state"][0], next_id=2000, **kw), "empty with a state")
    d = ops.event_corner_tracks(cu(x), cu(y), cu(t), H, W, max_dt=6 * tr.TICK)          # the defaults: radius 3, parent and velocity
    assert sorted(d) == ["cls", "length", "next_id", "parent", "state", "status", "track", "velocity"]
    want = tr.event_corner_tracks(x, y, t, H, W, radius=3, max_dt=6 * tr.TICK)
    assert np.array_equal(d["track"].cpu().numpy(), want["track"]) and georef.same_bits(d["velocity"].cpu().numpy(), want["velocity"])
    assert sorted(ops.event_corner_tracks(cu(x), cu(y), cu(t), H, W, max_dt=1.0, want_parent=False, want_velocity=False)) == [
        "cls", "length", "next_id", "state", "status", "track"]
    s = ops.event_corner_tracks_status(cu(a["status"]))
    assert s == dict(bad_order=False, n_events=2000, n_not_finite=int(a["status"][2]), n_outside=int(a["status"][3]),
                     n_not_corner=int(a["status"][4]), n_born=int(a["status"][5]), n_carried=0, n_linked=int(a["status"][7]))
    u, r = kit.host(ops.corner_track_state(cu(b["state"]))), tr.unpack_state(b["state"], W)
    assert sorted(u) == sorted(r) and all(u[k].dtype == r[k].dtype and georef.same_bits(u[k], r[k]) for k in r)
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.event_corner_tracks(torch.zeros(3), torch.zeros(3), torch.zeros(3, dtype=torch.float64), H, W, max_dt=1.0)


def test_own_stream():
    """inputs made on a side stream right before the call and overwritten right behind it, the results copied to the host on
    that stream: the bits of the default stream"""
    from rampvo_amd import ops
    x, y, t, p, c = tr.mixed(30011, seed=4)
    kw = dict(radius=2, max_dt=4 * tr.TICK)
    want = tr.event_corner_tracks(x, y, t, H, W, p=p, corner=c, **kw)
    side = torch.cuda.Stream()
    hosts = [torch.from_numpy(v).pin_memory() for v in (x, y, t, p, c)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        xd, yd, td, pd, cd = (v.to("cuda", non_blocking=True) for v in hosts)
        out = ops.event_corner_tracks(xd, yd, td, H, W, p=pd, corner=cd, want_birth=True, **kw)
        xd.fill_(float("nan")), yd.fill_(float("nan")), td.fill_(float("nan")), pd.fill_(0), cd.fill_(0)
        host = {k: v.to("cpu", non_blocking=True) for k, v in out.items()}
        side.synchronize()
    same({k: v.numpy() for k, v in host.items()}, want, "side stream")
    assert want["status"][7] > 10000


# ------------------------------------------------------------------------------------------------ 5. tracker
TRACKS = dict(radius=3, max_dt=4 * tr.TICK, want_birth=True, want_arc=True)
TH, TW = 240, 320


def _events(f):
    """wedge runs and noise of the detector's test stream, moved into the tracker's image, in the time of frame f"""
    x, y, t, p = cr.stream(4099)
    return (np.trunc(x).astype(np.int32) + 100, np.trunc(y).astype(np.int32) + 100, 100.0 + 0.5 * (f - 2) + (t - t[0]), p)


def _reference(xh, yh, th, ph=None, **kw):
    det = cr.event_corners(xh, yh, th, TH, TW, p=ph)
    return det, tr.event_corner_tracks(xh, yh, th, TH, TW, corner=det["cls"] == 7, p=ph, radius=3, max_dt=4 * tr.TICK, **kw)


def _tracker_queries(slam, f):
    xh, yh, th, ph = _events(f)
    x, y, t, p = cu(xh), cu(yh), cu(th), cu(ph)
    with pytest.raises(RuntimeError, match="unknown parameter"):
        slam.event_corner_tracks(x, y, t, window=1.0, max_dt=1.0)
    with pytest.raises(RuntimeError, match="max_dt is required"):
        slam.event_corner_tracks(x, y, t)
    with pytest.raises(RuntimeError, match="set_event_filter"):
        slam.event_corner_tracks(x, y, t, denoise=True, max_dt=1.0)
    assert slam._track_state is None
    cut = 1500
    det, ref = _reference(xh, yh, th, ph)
    a = slam.event_corner_tracks(xh[:cut], yh[:cut], th[:cut], ph[:cut], **TRACKS)   # numpy in (int32: the integer path), numpy out
    b = kit.host(slam.event_corner_tracks(x[cut:], y[cut:], t[cut:], p[cut:], as_tensor=True, **TRACKS))
    for k in ("track", "length"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), ref[k]), k
    for k in ("birth", "velocity"):
        assert georef.same_bits(np.concatenate([a[k], b[k]]), ref[k]), k
    assert np.array_equal(np.concatenate([a["corner_cls"], b["corner_cls"]]), det["cls"]) and ref["status"][7] > 20 and b["status"][6] > 0
    assert np.array_equal(np.concatenate([a["arc"], b["arc"]]), det["arc"]) and np.array_equal(a["corner"], det["cls"][:cut] == 7)
    assert np.array_equal(b["state"], ref["state"]) and b["next_id"][0] == 4099 and georef.same_bits(b["last_t"], det["last_t"])
    carried = [kit.host(v) for v in slam._track_state]
    assert georef.same_bits(carried[0], det["last_t"]) and np.array_equal(carried[1], ref["state"]) and carried[2][0] == 4099
    assert slam._corner_state is None and slam._flow_state is None   # its own surface, not the detector query's
    with pytest.raises(RuntimeError, match="decrease in time"):
        slam.event_corner_tracks(xh, yh, th, ph, **TRACKS)          # the same events again: they lie before the surface
    again = [kit.host(v) for v in slam._track_state]                       # ... and everything carried is left as it was
    assert georef.same_bits(again[0], carried[0]) and np.array_equal(again[1], carried[1]) and again[2][0] == 4099
    with pytest.raises(RuntimeError, match="reset_event_corner_tracks"):
        slam.event_corner_tracks(xh, yh, th, **TRACKS)              # without p: another surface
    alone = slam.event_corner_tracks(xh, yh, th, ph, carry=False, **TRACKS)
    assert np.array_equal(alone["track"], ref["track"]) and np.array_equal(alone["parent"], ref["parent"])
    assert np.array_equal(alone["status"], ref["status"]) and np.array_equal(alone["corner_status"], det["status"])
    slam.reset_event_corner_tracks()
    assert slam._track_state is None
    # denoise=True: the filter's xy, NaN rows in class 2
    slam.set_event_filter(refractory=0.5 * cr.TICK)
    kept = fr.event_filter(xh, yh, th, TH, TW, refractory=0.5 * cr.TICK)
    ddet, want = _reference(kept["xy"][:, 0], kept["xy"][:, 1], th)
    d = slam.event_corner_tracks(x, y, t, denoise=True, carry=False, **TRACKS)
    assert np.array_equal(d["cls"], want["cls"]) and np.array_equal(d["track"], want["track"]) and np.array_equal(d["status"], want["status"])
    assert np.array_equal(d["filter_status"], kept["status"]) and d["status"][2] == 4099 - kept["status"][7] > 0
    assert slam._track_state is None and slam._filter_state is None
    return dict(first=a, second=b, denoised=d)


def test_tracker_device_resident():
    a, c = kit.run_resident(True, lambda slam, f, frame: _tracker_queries(slam, f)), kit.run_resident(True, None)
    assert a["resident_before"] and a["resident_after"] and a["resident_at_end"] and c["resident_at_end"]
    kit.same(a["state", kit.T_QUERY + 1], c["state", kit.T_QUERY + 1], "the frame behind the queries")


@torch.no_grad()
def test_tracker_host_driven():
    slam = kit.tracker(False, True)
    frames = kit.frames()
    for f, frame in enumerate(frames):
        kit.feed(slam, f, frame)
        if slam.is_initialized and slam._n >= 4:
            break
    assert slam.is_initialized and slam._dev is None
    _tracker_queries(slam, f)
    kit.feed(slam, f + 1, frames[f + 1])
    assert slam._dev is None
    kit.drop(slam)
