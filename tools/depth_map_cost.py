"""What the inverse-depth map costs: ramp_invdepth_map (csrc/depthmap.hip) against a torch broadcast of the same formula, and
behind the tracker.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  kernel   640 x 480, K = REMOVAL_WINDOW x 96 = 2112 points uniform over the reach box, confidences 0.5 .. 2, a prior.  Legs
           (device events around the whole call: memset + two launches): R = 16, 64, 640 image pixels.  Printed per leg: median
           us, min, max, the pairs the regression evaluates after the cull (counted on the host from the call's own records and
           the kernel's tile and margin) against the K x H x W unculled pairs, and pairs per second.
           baseline: the same records regressed by torch in chunks of 64 records broadcast against the [H, W] grid (fp32, the
           same statement order); the ratio is quoted against THIS.
  tracker  two interleaved pairs of legs on BASELINE configs[1] (SingleScale 640 x 480, 96 patches, fp16 features):
             a / b   no query / invdepth_map(as_tensor=True) behind every frame; kf/s per leg, b / a, a's own spread
             c / d   compensate_events(2 10^5 device-resident events of the last two frames, as_tensor=True, iwe) with the
                     median / with invdepth="map"; kf/s per leg, d / c

    python tools/depth_map_cost.py [--part kernel|tracker|both] [--weights variance|uniform] [--repeats R] [--json out.json]
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

import tracker_legs as tl

TILE_W, TILE_H = 32, 16               # csrc/depthmap.hip: DM_TILE_W, DM_TILE_H (the pair count below models its cull)


def _baseline(rec, prior, pw, R, H, W, chunk=64):
    dev = rec.device
    gy, gx = torch.meshgrid(torch.arange(H, dtype=torch.float32, device=dev), torch.arange(W, dtype=torch.float32, device=dev),
                            indexing="ij")
    S0, S1 = torch.zeros((H, W), device=dev), torch.zeros((H, W), device=dev)
    inv_r2 = 1.0 / (R * R)
    for i in range(0, rec.shape[0], chunk):
        r = rec[i:i + chunk]
        dx, dy = gx[None] - r[:, 0, None, None], gy[None] - r[:, 1, None, None]
        t = torch.clamp(1.0 - (dx * dx + dy * dy) * inv_r2, min=0.0)
        w = r[:, 3, None, None] * (t * t)
        S0 += w.sum(0)
        S1 += (w * r[:, 2, None, None]).sum(0)
    return (pw * prior + S1) / (pw + S0), S0


def _culled_pairs(rec, R, H, W):
    """pairs the regress launch evaluates: per tile the records with weight > 0 inside the tile's box grown by R + margin"""
    grow = R + 0.001 * (R + H + W)
    r = rec[rec[:, 3] > 0].double()
    x0 = torch.arange(0, W, TILE_W, device=rec.device, dtype=torch.float64)
    y0 = torch.arange(0, H, TILE_H, device=rec.device, dtype=torch.float64)
    inx = (r[:, 0, None] >= x0[None] - grow) & (r[:, 0, None] <= x0[None] + TILE_W - 1 + grow)
    iny = (r[:, 1, None] >= y0[None] - grow) & (r[:, 1, None] <= y0[None] + TILE_H - 1 + grow)
    return int((inx.sum(1) * iny.sum(1)).sum()) * TILE_W * TILE_H


def kernel_part(args, dev):
    from rampvo_amd import ops
    H, W, K = args.height, args.width, args.points
    g = torch.Generator(device="cpu").manual_seed(8)
    ident = torch.tensor([0, 0, 0, 0, 0, 0, 1.0], device=dev)
    poses = ident.repeat(K, 1).contiguous()
    intr = torch.tensor([320.0, 320.0, 319.5, 239.5], device=dev)
    conf = (0.5 + 1.5 * torch.rand(K, generator=g)).to(dev)
    prior, pw = 0.4, 0.7

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    legs, base, info = {}, {}, {}
    for R in args.radii:
        patches = torch.zeros((K, 3, 3, 3))
        patches[:, 0] = (torch.rand(K, generator=g) * (W - 1 + 2 * R) - R)[:, None, None]
        patches[:, 1] = (torch.rand(K, generator=g) * (H - 1 + 2 * R) - R)[:, None, None]
        patches[:, 2] = (0.05 + 1.15 * torch.rand(K, generator=g))[:, None, None]
        patches = patches.to(dev)
        name = "R=%g" % R
        legs[name] = (lambda p=patches, R=R: ops.invdepth_map(poses, p, intr, ident, H, W, R, conf=conf, prior=prior,
                                                              prior_weight=pw))
        first = ops.invdepth_map(poses, patches, intr, ident, H, W, R, conf=conf, prior=prior, prior_weight=pw, want_records=True)
        rec = first["records"]
        base[name] = (lambda rec=rec, R=R: _baseline(rec, prior, pw, R, H, W))
        ref, ref_w = base[name]()
        again = legs[name]()
        info[name] = {"pairs_unculled": K * H * W, "pairs_culled": _culled_pairs(rec, R, H, W),
                      "vs_baseline_rel": float((first["invdepth"] - ref).abs().max() / ref.abs().max()),
                      "weight_vs_baseline_rel": float((first["weight"] - ref_w).abs().max() / ref_w.abs().max()),
                      "same_bits_twice": torch.equal(again["invdepth"].view(torch.int32), first["invdepth"].view(torch.int32))}
    for fn in list(legs.values()) + list(base.values()):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us, base_us = {k: [] for k in legs}, {k: [] for k in legs}
    for r in range(args.repeats):
        for k in legs:
            us[k].append(timed(legs[k]))
        if r < args.baseline_repeats:
            for k in legs:
                base_us[k].append(timed(base[k]))
    out = {"K": K, "H": H, "W": W, "repeats": args.repeats, "legs": {}}
    for k, v in us.items():
        med, bmed = statistics.median(v), statistics.median(base_us[k])
        out["legs"][k] = dict(info[k], us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                              baseline_us_median=round(bmed, 1), baseline_over_kernel=round(bmed / med, 2),
                              culled_share=round(info[k]["pairs_culled"] / info[k]["pairs_unculled"], 4),
                              Gpairs_per_s=round(info[k]["pairs_culled"] / med / 1e3, 2))
        print("%-6s %9.1f us (min %.1f, max %.1f)  %.3g of %.3g pairs (%.1f %%), %.1f Gpair/s;  torch %9.1f us = %.2f x;  "
              "largest difference / largest value %.1e, same bits twice: %s"
              % (k, med, min(v), max(v), info[k]["pairs_culled"], info[k]["pairs_unculled"], 100 * out["legs"][k]["culled_share"],
                 out["legs"][k]["Gpairs_per_s"], bmed, bmed / med, info[k]["vs_baseline_rel"], info[k]["same_bits_twice"]))
    return out


def tracker_part(args, dev):
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 4, warmup), dev)
    slam, n_ev = t.slam, args.tracker_events
    g = torch.Generator(device="cpu").manual_seed(9)
    ex = (torch.rand(n_ev, generator=g) * (args.width - 1)).to(dev)
    ey = (torch.rand(n_ev, generator=g) * (args.height - 1)).to(dev)
    ep = (torch.randint(0, 2, (n_ev,), generator=g) * 2 - 1).to(torch.int8).to(dev)
    frac = torch.sort(torch.rand(n_ev, generator=g, dtype=torch.float64)).values.to(dev)      # time-sorted, in the last two frames
    t.prime(args.prime, args.clock_warm)
    what = {"a": "no query", "b": "invdepth_map(weights=%r) per frame" % args.weights,
            "c": "compensate_events(%d events), median" % n_ev, "d": "compensate_events(%d events), invdepth='map'" % n_ev}
    last = {}

    def b():
        last["map"] = slam.invdepth_map(weights=args.weights, as_tensor=True)

    def c():
        last["median"] = slam.compensate_events(ex, ey, float(t.pos - 3) + 2.0 * frac, ep, as_tensor=True)

    def d():
        last["warp"] = slam.compensate_events(ex, ey, float(t.pos - 3) + 2.0 * frac, ep, invdepth="map", weights=args.weights,
                                              as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": b, "c": c, "d": d}, steps, warmup, repeats)
    out = {"workload": t.workload, "weights": args.weights, "events_per_frame": n_ev, "steps": steps, "repeats": repeats,
           "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, what)
    out["b_over_a"], out["d_over_c"] = tl.ratio(out["legs"], "b", "a"), tl.ratio(out["legs"], "d", "c")
    out["a_spread"] = tl.spread(out["legs"]["a"])
    out["last_map_status"] = last["map"]["status"].cpu().tolist()
    out["last_warp_status"] = {"median": last["median"]["status"].cpu().tolist(), "map": last["warp"]["status"].cpu().tolist()}
    print("b / a = %.4f, d / c = %.4f   (a's own spread, (max - min) / median: %.4f); last map status %s"
          % (out["b_over_a"], out["d_over_c"], out["a_spread"], out["last_map_status"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "tracker", "both"), default="both")
    ap.add_argument("--points", type=int, default=22 * 96)
    ap.add_argument("--radii", type=float, nargs="+", default=[16.0, 64.0, 640.0])
    ap.add_argument("--weights", choices=("variance", "uniform"), default="variance")
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--baseline-repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tracker-repeats", type=int, default=5)
    ap.add_argument("--tracker-warmup", type=int, default=20)
    ap.add_argument("--tracker-events", type=int, default=200000)
    ap.add_argument("--prime", type=int, default=70)
    ap.add_argument("--clock-warm", type=int, default=480)
    ap.add_argument("--patches", type=int, default=96)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "depth_map_cost.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {}
    if args.part in ("kernel", "both"):
        out["kernel"] = kernel_part(args, dev)
    if args.part in ("tracker", "both"):
        out["tracker"] = tracker_part(args, dev)
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
