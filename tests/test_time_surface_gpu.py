"""The time surface on the GPU: ``ramp_time_surface`` (csrc/timesurface.hip) through the C entry point (every buffer between
canaries, tests/guarded.py) and ``ops.time_surface``.

``last_t`` and every status word are held BIT FOR BIT to the restatement (tests/localizeref.py); ``surface`` bit for bit to the
fp32 emulator of the binomial run on the call's OWN ``raw``; ``raw`` -- the one place ``expf`` sits -- to the float64 restatement
by the bound rule of test_geometry_f64_gpu.py, ``georef.bound(floor, env)`` with env the float32 restatement's own error against
float64 and the floor ``georef.FLOOR["exp"]`` (values in [0, 1]).  Images are 13 x 17.  Nothing here provokes a fault."""
import ctypes

import numpy as np
import pytest
import torch

import georef
import localizeref as lr
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

H, W = lr.H, lr.W
T_REF, TAU = 2.0, 0.5
P = lambda f: ctypes.c_void_p(f.address()) if isinstance(f, Flat) else (None if f is None else ctypes.c_void_p(f.data_ptr()))
bits = lambda a: np.ascontiguousarray(a).reshape(-1).view({4: np.uint32, 8: np.uint64}[np.asarray(a).dtype.itemsize])


def surface(x, y, t, t_ref=T_REF, tau=TAU, h=H, w=W, smooth=2, negate=True, last=None, raw=True, last_out=True, expect=0, **over):
    """the C entry with every buffer between canaries -> numpy dict"""
    from rampvo_amd import _lib
    L = _lib.lib()
    n = len(x)
    nbytes = L.ramp_time_surface_ws_bytes(h, w)
    b = dict(surface=Flat((h, w), torch.float32), raw=Flat((h, w), torch.float32), last_t=Flat((h, w), torch.float64),
             status=Flat(8, torch.int32), ws=Flat(nbytes, torch.uint8, rows=4))
    d = [cu(np.asarray(x, np.float32)), cu(np.asarray(y, np.float32)), cu(np.asarray(t, np.float64))] if n else [None] * 3
    d_last = None if last is None else cu(np.asarray(last, np.float64))
    torch.cuda.synchronize()
    before = {k: v.snapshot() for k, v in b.items()}
    a = dict(p_x=P(d[0]), p_y=P(d[1]), p_t=P(d[2]), N=n, p_last=P(d_last), t_ref=t_ref, tau=tau, H=h, W=w, smooth=smooth,
             flags=1 if negate else 0, p_surface=P(b["surface"]), p_raw=P(b["raw"]) if raw else None,
             p_last_out=P(b["last_t"]) if last_out else None, p_ws=P(b["ws"]), nbytes=nbytes, p_status=P(b["status"]))
    assert set(over) <= set(a), over
    a.update(over)
    rc = L.ramp_time_surface(*a.values(), _lib.stream())
    torch.cuda.synchronize()
    assert rc == expect, (rc, over)
    assert all(v.intact() for v in b.values())
    if rc:
        assert all(v.unchanged(before[k]) for k, v in b.items()), "a refused call touches nothing"
        return None
    for k, used in (("raw", raw), ("last_t", last_out)):
        assert used or b[k].unchanged(before[k]), "an output that was not asked for is not written: " + k
    return {k: b[k].t.cpu().numpy() for k in ("surface", "raw", "last_t", "status")}


def check(out, x, y, t, name, t_ref=T_REF, tau=TAU, h=H, w=W, smooth=2, negate=True, last=None):
    last_ref, ctr = lr.last_stamps(x, y, t, t_ref, h, w, last)
    assert out["status"].tolist() == [0] + ctr + [0], (name, out["status"], ctr)
    st = out["status"]
    assert st[2] + st[3] + st[4] + st[5] == st[1] == len(x), name
    assert np.array_equal(bits(out["last_t"]), bits(last_ref)), name + ": last_t bit for bit"
    r32, r64 = lr.raw_surface(last_ref, t_ref, tau, negate), lr.raw_surface(last_ref, t_ref, tau, negate, np.float64)
    err, env = georef.max_err(out["raw"], r64), georef.max_err(r32, r64)
    print("time surface %s: raw err %.3g env %.3g bound %.3g" % (name, err, env, georef.bound(georef.FLOOR["exp"], env)))
    assert err <= georef.bound(georef.FLOOR["exp"], env), (name, err, env)
    none = np.isnan(last_ref)
    assert (out["raw"][none] == (1.0 if negate else 0.0)).all(), name
    assert np.array_equal(bits(out["surface"]), bits(lr.binomial(out["raw"], smooth))), name + ": the surface from the call's own raw"


@pytest.mark.parametrize("N", (0, 1, 2, 4099))
def test_last_stamps_raw_and_surface(N):
    x, y, t = lr.event_case(N, seed=N) if N else (np.zeros(0, np.float32),) * 2 + (np.zeros(0),)
    out = surface(x, y, t)
    check(out, x, y, t, "N=%d" % N)
    if N == 0:
        assert out["status"].tolist() == [0] * 8 and (out["surface"] == 1).all() and np.isnan(out["last_t"]).all()
    if N == 4099:
        assert out["status"][3] > 0 and out["status"][4] > 0 and out["status"][6] == H * W
        again = surface(x, y, t)                              # a call repeats its bits
        perm = np.random.default_rng(3).permutation(N)
        shuffled = surface(x[perm], y[perm], t[perm])
        half = N // 3
        first = surface(x[:half], y[:half], t[:half])
        chained = surface(x[half:], y[half:], t[half:], last=first["last_t"])
        for other, what in ((again, "again"), (shuffled, "shuffled")):
            for k in ("surface", "raw", "last_t", "status"):
                assert np.array_equal(bits(out[k]), bits(other[k])), (what, k)
        for k in ("surface", "raw", "last_t"):
            assert np.array_equal(bits(out[k]), bits(chained[k])), ("chained", k)
        check(chained, x[half:], y[half:], t[half:], "chained", last=first["last_t"])
        for smooth in (0, 1, 8):
            check(surface(x, y, t, smooth=smooth), x, y, t, "smooth=%d" % smooth, smooth=smooth)
        check(surface(x, y, t, negate=False), x, y, t, "not negated", negate=False)


def test_equal_negative_and_boundary_time_stamps_and_the_borders():
    after = np.nextafter(T_REF, 3.0)
    x = np.float32([3, 3, 3, 5, 5, 6, 7, 8, -0.4, -0.6, W - 0.6, W - 0.4, 2, 2, 2, 2])
    y = np.float32([4, 4, 4, 1, 1, 1, 1, 1, 3, 3, 3, 3, -0.4, -0.6, H - 0.6, H - 0.4])
    t = np.array([1.5, 1.5, 1.25, -3.0, -2.0, T_REF, after, np.inf, 1, 1, 1, 1, 1, 1, 1, 1.0])
    t[7], x[6] = 1.0, np.nan
    t = np.r_[t, [np.nan, np.inf, -np.inf]]
    x, y = np.r_[x, np.float32([1, 1, 1])], np.r_[y, np.float32([1, 1, 1])]
    x, y, t = np.r_[x, np.float32([9])], np.r_[y, np.float32([9])], np.r_[t, [after]]
    out = surface(x, y, t, smooth=0)
    check(out, x, y, t, "edges", smooth=0)
    assert out["last_t"][4, 3] == 1.5 and out["last_t"][1, 5] == -2.0 and out["last_t"][1, 6] == T_REF and out["surface"][1, 6] == 0.0
    assert np.isnan(out["last_t"][9, 9]) and out["status"].tolist()[1:6] == [len(x), 4, 4, 1, len(x) - 9]


@pytest.mark.parametrize("shape", ((1, 1), (1, 17), (13, 1)))
def test_thin_images(shape):
    h, w = shape
    rng = np.random.default_rng(5)
    n = 40
    x, y, t = rng.integers(0, w, n).astype(np.float32), rng.integers(0, h, n).astype(np.float32), rng.uniform(0, T_REF, n)
    for smooth in (0, 2, 8):
        check(surface(x, y, t, h=h, w=w, smooth=smooth), x, y, t, "%dx%d smooth=%d" % (h, w, smooth), h=h, w=w, smooth=smooth)


def test_the_filters_state_is_usable_as_it_is_and_a_side_stream():
    from rampvo_amd import ops
    x, y, t = lr.event_case(4099, seed=2)
    inside = (np.rint(x) >= 0) & (np.rint(x) < W) & (np.rint(y) >= 0) & (np.rint(y) < H)
    xi, yi = np.rint(x[inside]).astype(np.int32), np.rint(y[inside]).astype(np.int32)
    order = np.argsort(t[inside], kind="stable")
    xi, yi, ti = xi[order], yi[order], t[inside][order]
    cut = len(ti) // 2
    f = ops.event_filter(cu(xi[:cut]), cu(yi[:cut]), cu(ti[:cut]), H, W)          # no test is on: every event is kept
    a = ops.time_surface(cu(xi[cut:].astype(np.float32)), cu(yi[cut:].astype(np.float32)), cu(ti[cut:]), T_REF, TAU, H, W,
                         last_t=f["last_t"], want_raw=True, want_last_t=True)
    whole = surface(xi.astype(np.float32), yi.astype(np.float32), ti)
    for k in ("surface", "raw", "last_t"):
        assert np.array_equal(bits(a[k].cpu().numpy()), bits(whole[k])), k
    assert ops.time_surface_status(a["status"])["n_late"] == int((ti[cut:] > T_REF).sum())
    side = torch.cuda.Stream()
    d = cu(x), cu(y), cu(t)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        r = ops.time_surface(*d, T_REF, TAU, H, W, want_raw=True, want_last_t=True)
    side.synchronize()
    ref = surface(x, y, t)
    for k in ("surface", "raw", "last_t", "status"):
        assert np.array_equal(bits(r[k].cpu().numpy()), bits(ref[k])), k
    plain = ops.time_surface(*d, T_REF, TAU, H, W)
    assert plain["raw"] is None and plain["last_t"] is None and torch.equal(plain["surface"], r["surface"])


def test_bad_arguments_set_the_bit_and_refusals_touch_nothing():
    from rampvo_amd import _lib
    x, y, t = lr.event_case(64, seed=4)
    good = surface(x, y, t)
    for kw in (dict(t_ref=np.nan), dict(t_ref=np.inf), dict(tau=np.nan), dict(tau=np.inf), dict(tau=0.0), dict(tau=-1.0)):
        out = surface(x, y, t, **kw)
        assert out["status"][0] == 1 and np.isnan(out["surface"]).all() and np.isnan(out["raw"]).all(), kw
        if "tau" in kw:
            assert np.array_equal(bits(out["last_t"]), bits(good["last_t"])) and out["status"].tolist()[1:] == good["status"].tolist()[1:]
    for over in (dict(N=-1), dict(H=0), dict(W=-1), dict(smooth=-1), dict(smooth=9), dict(flags=2), dict(p_surface=None), dict(p_status=None),
                 dict(p_ws=None), dict(p_x=None), dict(p_y=None), dict(p_t=None)):
        surface(x, y, t, expect=_lib.RAMP_EINVAL, **over)
    surface(x, y, t, expect=_lib.RAMP_EUNSUPPORTED, H=1 << 16, W=1 << 15)
    surface(x, y, t, expect=_lib.RAMP_EWORKSPACE, nbytes=_lib.lib().ramp_time_surface_ws_bytes(H, W) - 1)
    only = surface(x, y, t, raw=False, last_out=False)
    assert np.array_equal(bits(only["surface"]), bits(good["surface"]))
