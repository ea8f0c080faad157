"""Numpy restatement of the event voxel grid (include/ramp_hip.h ``ramp_event_voxel``) -- TEST INFRASTRUCTURE ONLY.

Two parts, from the same per-event votes (``votes``: float64 up to ``ti``, numpy float32 for ``dts``, the two values and the
sub-pixel products -- the formats the reference class and the kernel use):

(a) ``grid64``: the votes summed in FLOAT64 and standardised in float64 -- what the reference class would give with an exact
    ``index_add_``.  The fixture records the reference's own error against this.

(b) ``accumulate`` / ``finish``: an EXACT emulator of the kernel: ``np.rint(np.ldexp(value, 24))`` to int64, ``np.add.at``;
    n and the sum as integers, the mean from them, the grid as the kernel converts it.  Integer sums have no order, so the
    accumulators, n, sum and mean are reproduced bit for bit; std is a float64 sum whose order differs from the kernel's.

``compare`` is the one tolerance rule of the CPU and the GPU test.  The ``mistake`` keywords break the restatement on purpose
(tests/test_voxelref_cpu.py: each has to be rejected by the comparison with the reference fixture).
"""
import os

import numpy as np

import splatref

FIX_BITS = 24
FIX = float(1 << FIX_BITS)
MISTAKES = ("minmax", "swap", "biased", "round", "allcells", "rightedge")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "event_voxel.npz")
CASES = ("random", "three", "onebin", "equal_times", "cancel")
BAD_OFFSETS, BAD_TIMES = 1, 2
f32 = np.float32


def votes(x, y, t, p, H, W, bins, subpixel=False, mistake=None):
    """the votes of ONE slice -> (bin, row, col, value float32) of every single contribution, and the status words 1 .. 5"""
    assert mistake is None or mistake in MISTAKES
    x, y = np.asarray(x, f32).reshape(-1), np.asarray(y, f32).reshape(-1)
    t = np.asarray(t, np.float64).reshape(-1)
    p = np.asarray(p).astype(np.int64).reshape(-1)
    pol = np.where(p == 0, -1, p).astype(f32)                 # (0 is read as -1)
    N = len(x)
    empty = (np.zeros(0, np.int64),) * 3 + (np.zeros(0, f32),)
    if N == 0:
        return empty, np.zeros(5, np.int64), True
    t_first, t_last = (t.min(), t.max()) if mistake == "minmax" else (t[0], t[-1])
    ok = bool(np.isfinite(t_first) and np.isfinite(t_last))
    with np.errstate(all="ignore"):
        dT = t_last - t_first
        dT = 1.0 if dT == 0 else dT
        tn = ((bins - 1) * (t - t_first)) / dT
        ti = np.floor(tn)
        dts = (tn - ti).astype(f32)
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(t)
    xs, ys = np.where(fin, x, 0).astype(f32), np.where(fin, y, 0).astype(f32)
    if subpixel:
        ix, wx, inx = splatref.axis(xs, W)
        iy, wy, iny = splatref.axis(ys, H)
        inside = ((inx[0] & (wx[0] != 0)) | (inx[1] & (wx[1] != 0))) & ((iny[0] & (wy[0] != 0)) | (iny[1] & (wy[1] != 0)))
    else:
        xt, yt = (np.rint(xs), np.rint(ys)) if mistake == "round" else (np.trunc(xs), np.trunc(ys))
        inside = (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
        ix, iy = np.where(inside, xt, 0).astype(np.int64), np.where(inside, yt, 0).astype(np.int64)
    with np.errstate(invalid="ignore"):
        in_bin = (ti >= 0) & (ti < bins) & ok
    voted = fin & inside & in_bin
    b = np.where(voted, ti, 0).astype(np.int64)
    vl, vr = (pol * (f32(1.0) - dts)).astype(f32), (pol * dts).astype(f32)
    if mistake == "swap":
        vl, vr = vr, vl
    right = voted & (b + 1 < bins)
    br = b + 1
    if mistake == "rightedge":                                 # (a right vote at ti + 1 == bins, folded into the last bin)
        right, br = voted, np.minimum(b + 1, bins - 1)
    out = [[], [], [], []]

    def put(mask, bb, yy, xx, val):
        for o, a in zip(out, (bb, yy, xx, val)):
            o.append(a[mask])

    if subpixel:
        for jy in range(2):
            for jx in range(2):
                w = (wx[jx] * wy[jy]).astype(f32)
                m = inx[jx] & iny[jy]
                put(voted & m, b, iy + jy, ix + jx, (w * vl).astype(f32))
                put(right & m, br, iy + jy, ix + jx, (w * vr).astype(f32))
    else:
        put(voted, b, iy, ix, vl)
        put(right, br, iy, ix, vr)
    words = np.array([N, (~fin).sum(), (fin & ~inside).sum(), (fin & inside & ~in_bin).sum(), voted.sum()], np.int64)
    return tuple(np.concatenate(o) for o in out), words, ok


def _slices(N, offsets):
    if offsets is None:
        return [(0, N)], False
    off = np.asarray(offsets, np.int64).reshape(-1)
    bad = bool((off < 0).any() or (off > N).any() or (np.diff(off) < 0).any())
    return list(zip(off[:-1].tolist(), off[1:].tolist())), bad


def accumulate(x, y, t, p, H, W, bins, offsets=None, subpixel=False, mistake=None):
    """the kernel's accumulators -> dict(acc int64 [S,bins,H,W], count int64 [S,bins,H,W] (contributions per cell), status
    int64 [8], failed bool [S]); bad offsets: every slice failed, no event read"""
    x, y, t, p = (np.asarray(a).reshape(-1) for a in (x, y, t, p))
    sl, bad = _slices(len(x), offsets)
    S = len(sl)
    acc, count = np.zeros((S, bins, H, W), np.int64), np.zeros((S, bins, H, W), np.int64)
    status, failed = np.zeros(8, np.int64), np.zeros(S, bool)
    if bad:
        status[0] = BAD_OFFSETS
        return dict(acc=acc, count=count, status=status, failed=~failed)
    for s, (lo, hi) in enumerate(sl):
        (b, yy, xx, v), words, ok = votes(x[lo:hi], y[lo:hi], t[lo:hi], p[lo:hi], H, W, bins, subpixel, mistake)
        c = np.rint(np.ldexp(v, FIX_BITS)).astype(np.int64)
        np.add.at(acc[s], (b, yy, xx), c)
        np.add.at(count[s], (b, yy, xx), 1)
        status[1:6] += words
        if not ok:
            status[0] |= BAD_TIMES
            failed[s] = True
    return dict(acc=acc, count=count, status=status, failed=failed)


def finish(acc, normalize, failed=None, mistake=None):
    """accumulators [S,bins,H,W] -> (grid float32, stats float64 [S,4] = n, mean, std, sum), as the kernel converts them"""
    S = acc.shape[0]
    grid, stats = np.zeros(acc.shape, f32), np.zeros((S, 4))
    for s in range(S):
        a = acc[s]
        if failed is not None and failed[s]:
            grid[s], stats[s] = np.nan, np.nan
            continue
        nz = np.ones(a.shape, bool) if mistake == "allcells" else a != 0
        n, total = int(nz.sum()), int(a[nz].sum())
        g = a.astype(np.float64) / FIX                          # (exact below 2^53)
        grid[s] = a.astype(f32) * f32(1.0 / FIX)                # int64 -> float32 rounds once
        if n == 0:
            continue
        mean = float(np.float64(total) / (np.float64(n) * FIX))
        with np.errstate(all="ignore"):
            var = np.sum((g[nz] - mean) ** 2) / np.float64(n if mistake == "biased" else n - 1)
            std = float(np.sqrt(var))
        stats[s] = (n, mean, std, np.float64(total) / FIX)
        if normalize:
            d = g - mean
            out = (d / std if std > 0 else d).astype(f32)
            grid[s] = np.where(nz, out, f32(0))
    return grid, stats


def voxel_grid(x, y, t, p, H, W, bins, offsets=None, normalize=True, subpixel=False, mistake=None):
    """the whole emulator -> dict(grid, stats, status, acc, count, failed)"""
    r = accumulate(x, y, t, p, H, W, bins, offsets, subpixel, mistake)
    r["grid"], r["stats"] = finish(r["acc"], normalize, r["failed"], mistake)
    return r


def grid64(x, y, t, p, H, W, bins, normalize=True, subpixel=False):
    """ONE slice in float64: the fp32 votes summed exactly enough, mean and unbiased std over the non-zero cells in float64 ->
    (grid float64 [bins,H,W], mean, std); mean = std = 0 without a non-zero cell"""
    (b, yy, xx, v), _, ok = votes(x, y, t, p, H, W, bins, subpixel)
    g = np.zeros((bins, H, W))
    np.add.at(g, (b, yy, xx), v.astype(np.float64))
    nz = g != 0
    mean = std = 0.0
    if nz.any():
        mean = float(g[nz].mean())
        with np.errstate(all="ignore"):
            std = float(g[nz].std(ddof=1))
        if normalize:
            g = np.where(nz, (g - mean) / std if std > 0 else g - mean, 0.0)
    return g, mean, std


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, f32))).astype(np.float64)


def bound_raw(count, ref, own_err):
    """the envelope rule per cell: four times the reference's own error against float64, or what the fixed point may add --
    2^-25 per contribution -- plus one fp32 ulp of the value, whichever is larger"""
    return np.maximum(4.0 * own_err, count * 2.0 ** -(FIX_BITS + 1) + ulp32(ref))


def bound_norm(count, ref, own_err, std):
    """the same for the standardised grid.  With e = count 2^-25 a cell's fixed-point error and E its maximum over the grid, the
    mean moves by at most E and the std by at most sqrt(n / (n - 1)) 2 E <= 3 E, so (g - mean) / std moves by at most
    (e + E + 3 E |out|) / std (std from the fixture; 1 where the fixture's std is not positive: the mean alone is subtracted)"""
    e = count * 2.0 ** -(FIX_BITS + 1)
    E = float(e.max()) if e.size else 0.0
    s = std if std > 0 else 1.0
    return np.maximum(4.0 * own_err, (e + E * (1.0 + 3.0 * np.abs(ref))) / s + ulp32(ref))


def compare(grid, case, normalize):
    """a grid [bins,H,W] against the fixture's case ``case`` (``load_case``): the reference class's output by the envelope rule
    -> dict(err, bound: the largest of each; worst: the largest err / bound; ok)"""
    ref = case["ref_norm" if normalize else "ref_raw"].astype(np.float64)
    own = case["err_norm" if normalize else "err_raw"]
    bnd = bound_norm(case["count"], ref, own, float(case["std"])) if normalize else bound_raw(case["count"], ref, own)
    err = np.abs(np.asarray(grid, np.float64) - ref)
    with np.errstate(invalid="ignore"):
        ok = bool((err <= bnd).all())                          # (a NaN fails)
    return dict(err=float(np.nanmax(err)), bound=float(bnd.max()), worst=float(np.nanmax(err / bnd)), ok=ok)


def load_case(name, path=GOLDEN):
    with np.load(path) as z:
        return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}


def masks_agree(case):
    """the condition on the fixture: the reference's non-zero mask, the float64 restatement's and the emulator's are one set"""
    e = case["events"]
    bins, H, W = (int(v) for v in case["shape"])
    t, x, y, p = e[:, 0], e[:, 1], e[:, 2], e[:, 3]
    g, _, _ = grid64(x, y, t, p, H, W, bins, normalize=False)
    acc = accumulate(x, y, t, p, H, W, bins)["acc"][0]
    m = case["ref_raw"] != 0
    return bool(np.array_equal(m, g != 0) and np.array_equal(m, acc != 0))
