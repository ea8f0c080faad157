"""What the event voxel grid costs: ramp_event_voxel (csrc/voxel.hip) against a torch restatement of the reference's pipeline
-- two ``index_add_`` into a flat fp32 grid, then mean and unbiased std over the non-zero cells -- on the same device.  ONE
process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  N = 2^22 events, 640 x 480, 5 bins, time-sorted, as ONE slice and as 32 slices of N / 32.  Legs (device events around the
  whole call: per chunk a memset and four launches):
    default / sub-pixel pixels  x  raw / normalised        -> eight fused legs and their eight torch legs
  The torch legs run the slices one after the other, as the loader does (evaluate.py:117-135); the sub-pixel torch leg splats
  the four bilinear neighbours with ``index_add_``.  Float atomics: its sums depend on the order of arrival.
  Printed per leg: median us, min, max, the ratio torch / fused, and the integer-atomic bytes per second of the fused call
  (16 B per event, 64 B sub-pixel: an upper bound, votes of zero and neighbours outside the image are not sent).

    python tools/event_voxel_cost.py [--events N] [--repeats R] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _torch_slice(x, y, t, p, bins, H, W, normalize, subpixel):
    """one slice the way the reference class computes it (fp32 ``index_add_``), restated with torch"""
    grid = torch.zeros(bins * H * W, dtype=torch.float32, device=x.device)
    dT = t[-1] - t[0]
    dT = torch.where(dT == 0, torch.ones_like(dT), dT)
    tn = (bins - 1) * (t - t[0]) / dT
    ti = torch.floor(tn)
    dts = (tn - ti).float()
    pol = p.float()
    tl = ti.long()
    left, right = (ti >= 0) & (ti < bins), (ti >= 0) & (ti + 1 < bins)
    if subpixel:
        fx, fy = torch.floor(x), torch.floor(y)
        wx, wy = x - fx, y - fy
        nb = [(fx.long() + jx, fy.long() + jy, (wx if jx else 1 - wx) * (wy if jy else 1 - wy)) for jy in (0, 1) for jx in (0, 1)]
    else:
        nb = [(x.long(), y.long(), None)]
    for ix, iy, w in nb:
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        at = ix + iy * W
        vl, vr = pol * (1.0 - dts), pol * dts
        if w is not None:
            vl, vr = w * vl, w * vr
        m = left & inside
        grid.index_add_(0, (at + tl * (W * H))[m], vl[m])
        m = right & inside
        grid.index_add_(0, (at + (tl + 1) * (W * H))[m], vr[m])
    if normalize:
        nz = grid != 0
        n = nz.sum()
        mean = torch.where(nz, grid, torch.zeros_like(grid)).sum() / n
        std = torch.sqrt(torch.where(nz, (grid - mean) ** 2, torch.zeros_like(grid)).sum() / (n - 1))
        grid = torch.where(nz, (grid - mean) / std, grid)           # (no host read: std > 0 is taken for granted here)
    return grid.view(bins, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1 << 22)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--slices", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--baseline-repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "event_voxel_cost.py measures on the GPU; there is nothing to report without one"
    from rampvo_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, H, W, bins, S = args.events, args.height, args.width, args.bins, args.slices
    g = torch.Generator(device="cpu").manual_seed(8)
    t = torch.sort(torch.rand(N, generator=g, dtype=torch.float64)).values.to(dev)
    x = (torch.rand(N, generator=g) * (W - 1)).to(dev)
    y = (torch.rand(N, generator=g) * (H - 1)).to(dev)
    p = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).to(torch.int8).to(dev)
    off = ops.event_slices(N, N // S, device=dev)
    bounds = off.cpu().tolist()

    def fused(slices, normalize, subpixel):
        return lambda: ops.event_voxel_grid(x, y, t, p, H, W, num_bins=bins, offsets=off if slices > 1 else None,
                                            normalize=normalize, subpixel=subpixel)["grid"]

    def base(slices, normalize, subpixel):
        cuts = list(zip(bounds[:-1], bounds[1:])) if slices > 1 else [(0, N)]
        return lambda: [_torch_slice(x[a:b], y[a:b], t[a:b], p[a:b], bins, H, W, normalize, subpixel) for a, b in cuts]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    keys = [(s, nrm, sub) for s in (1, S) for sub in (False, True) for nrm in (False, True)]
    name = lambda k: "%2d slice%s %-9s %-10s" % (k[0], " " if k[0] == 1 else "s", "sub-pixel" if k[2] else "default", "normalised" if k[1] else "raw")
    legs, bases = {k: fused(*k) for k in keys}, {k: base(*k) for k in keys}
    agree = {}
    for k in keys:                                      # (also the first warm-up round)
        a, b = legs[k](), torch.stack(bases[k]())
        agree[k] = float((a.reshape(b.shape) - b).abs().max() / b.abs().max())
    for fn in list(legs.values()) + list(bases.values()):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us, base_us = {k: [] for k in keys}, {k: [] for k in keys}
    for r in range(args.repeats):
        for k in keys:
            us[k].append(timed(legs[k]))
            if r < args.baseline_repeats:
                base_us[k].append(timed(bases[k]))
    out = {"N": N, "H": H, "W": W, "bins": bins, "slices": S, "repeats": args.repeats, "baseline_repeats": args.baseline_repeats,
           "device": torch.cuda.get_device_name(dev), "legs": {}}
    for k in keys:
        med, bmed = statistics.median(us[k]), statistics.median(base_us[k])
        out["legs"][name(k).strip()] = {
            "us_median": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1),
            "torch_us_median": round(bmed, 1), "torch_us_min": round(min(base_us[k]), 1), "torch_us_max": round(max(base_us[k]), 1),
            "torch_over_fused": round(bmed / med, 2), "atomic_GBps_upper": round(N * (64 if k[2] else 16) / med / 1e3, 1),
            "largest_difference_rel": agree[k]}
        print("%s %9.1f us (min %.1f, max %.1f)   torch %10.1f us (min %.1f, max %.1f) = %6.2f x   <= %6.1f GB/s of integer atomics   "
              "difference %.1e" % (name(k), med, min(us[k]), max(us[k]), bmed, min(base_us[k]), max(base_us[k]), bmed / med,
                                  out["legs"][name(k).strip()]["atomic_GBps_upper"], agree[k]))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
