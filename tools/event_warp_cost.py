"""What motion compensation costs: ramp_event_warp (csrc/warp.hip) against the unfused composition the library offered before
it.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  N = 2^22 events, T = 2000 knots, 640 x 480.  Legs (device events around the whole call: memset + three launches):
    iwe            image of warped events only, scalar depth, time-sorted events
    iwe+stack5     the same plus a 5-bin float stack
    iwe map        depth from an [H, W] map
    iwe shuffled   the events in random order
  baseline: ops.se3_interp ([N,7] poses through HBM) + torch unproject / transform / project + floor, four weights and
  index_put_(accumulate=True) into the two planes (float sums, order dependent); the ratio is quoted against THIS.
  Printed per leg: median us, min, max, and the atomic bytes per second of the fused call (64 B per event for iwe, 32 B for a
  stack: an upper bound, contributions of zero and neighbours outside the image are not sent).

  tracker  pose_query_cost.py's two interleaved legs on BASELINE configs[1]: no query / compensate_events(2 10^5 device-resident
           events of the last two frames, as_tensor=True, iwe) behind every frame; kf/s per leg, b / a, a's own spread.

    python tools/event_warp_cost.py [--part kernel|tracker|both] [--events N] [--repeats R] [--json out.json]
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


def _knots(T, dev):
    from rampvo_amd.lietorch import SE3
    g = torch.Generator(device="cpu").manual_seed(7)
    v = torch.cumsum(torch.randn(T, 6, generator=g) * 0.01, 0) + torch.randn(1, 6, generator=g) * 0.05
    xi = torch.cumsum(v * torch.tensor([0.005, 0.003, 0.004, 0.002, 0.003, 0.002]), 0)
    return SE3.exp(xi.to(dev)).data.contiguous(), (0.05 * torch.arange(T, dtype=torch.float64)).to(dev)


def _baseline(x, y, t, p, knots, times, t_ref, K, d, H, W):
    from rampvo_amd import ops
    from rampvo_amd.lietorch import SE3
    C, _, _ = ops.se3_interp(knots, times, t)
    Cr, _, _ = ops.se3_interp(knots, times, torch.tensor([t_ref], dtype=torch.float64, device=x.device))
    G = SE3(Cr).inv() * SE3(C)
    P = torch.stack([(x - K[2]) / K[0], (y - K[3]) / K[1], torch.ones_like(x), torch.full_like(x, d)], -1)
    X = G.act(P)
    xw, yw = K[0] * (X[:, 0] / X[:, 2]) + K[2], K[1] * (X[:, 1] / X[:, 2]) + K[3]
    ok = X[:, 2] > 0.2
    fx, fy = torch.floor(xw), torch.floor(yw)
    wx, wy = xw - fx, yw - fy
    iwe = torch.zeros((2, H * W), dtype=torch.float32, device=x.device)
    pf = p.float()
    for jy in (0, 1):
        for jx in (0, 1):
            ix, iy = fx.long() + jx, fy.long() + jy
            w = (wx if jx else 1 - wx) * (wy if jy else 1 - wy)
            m = ok & (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
            at = (iy * W + ix)[m]
            iwe[0].index_put_((at,), (w * pf)[m], accumulate=True)
            iwe[1].index_put_((at,), w[m], accumulate=True)
    return iwe.view(2, H, W)


def tracker_part(args, dev):
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 2, warmup), dev)
    n_ev = args.tracker_events
    g = torch.Generator(device="cpu").manual_seed(9)
    ex = (torch.rand(n_ev, generator=g) * (args.width - 1)).to(dev)
    ey = (torch.rand(n_ev, generator=g) * (args.height - 1)).to(dev)
    ep = (torch.randint(0, 2, (n_ev,), generator=g) * 2 - 1).to(torch.int8).to(dev)
    frac = torch.sort(torch.rand(n_ev, generator=g, dtype=torch.float64)).values.to(dev)      # time-sorted, in the last two frames
    t.prime(args.prime, args.clock_warm)
    last = [None]

    def query():
        last[0] = t.slam.compensate_events(ex, ey, float(t.pos - 3) + 2.0 * frac, ep, as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": query}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "steps": steps, "repeats": repeats, "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "compensate_events(%d events) per frame" % n_ev})
    out["b_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.spread(out["legs"]["a"])
    out["last_status"] = last[0]["status"].cpu().tolist()
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f); last status %s" % (out["b_over_a"], out["a_spread"], out["last_status"]))
    return out


def kernel_part(args, dev):
    from rampvo_amd import ops
    N, T, H, W = args.events, args.knots, args.height, args.width
    knots, times = _knots(T, dev)
    g = torch.Generator(device="cpu").manual_seed(8)
    t = torch.sort(torch.rand(N, generator=g, dtype=torch.float64) * float(times[-1])).values.to(dev)
    x = (torch.rand(N, generator=g) * (W - 1)).to(dev)
    y = (torch.rand(N, generator=g) * (H - 1)).to(dev)
    p = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).to(torch.int8).to(dev)
    perm = torch.randperm(N, generator=g).to(dev)
    xs, ys, ts, ps = x[perm].contiguous(), y[perm].contiguous(), t[perm].contiguous(), p[perm].contiguous()
    K = torch.tensor([320.0, 320.0, 319.5, 239.5], device=dev)
    dmap = (0.3 + 0.4 * torch.rand(H, W, generator=g)).to(dev)
    t_ref = float(times[-1]) * 0.5
    legs = {
        "iwe": lambda: ops.event_warp(x, y, t, p, knots, times, t_ref, K, 0.5, H, W),
        "iwe+stack5": lambda: ops.event_warp(x, y, t, p, knots, times, t_ref, K, 0.5, H, W, num_bins=5, stack="f32"),
        "iwe map": lambda: ops.event_warp(x, y, t, p, knots, times, t_ref, K, dmap, H, W),
        "iwe shuffled": lambda: ops.event_warp(xs, ys, ts, ps, knots, times, t_ref, K, 0.5, H, W),
    }
    atomic_bytes = {"iwe": 64, "iwe+stack5": 96, "iwe map": 64, "iwe shuffled": 64}
    base = lambda: _baseline(x, y, t, p, knots, times, t_ref, K, 0.5, H, W)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    fused, ref = legs["iwe"]()["iwe"], base()
    agree = float((fused - ref).abs().max() / ref.abs().max())
    same = torch.equal(legs["iwe shuffled"]()["iwe"].view(torch.int32), fused.view(torch.int32))
    for fn in list(legs.values()) + [base]:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us, base_us = {k: [] for k in legs}, []
    for r in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
        if r < args.baseline_repeats:
            base_us.append(timed(base))
    out = {"N": N, "T": T, "H": H, "W": W, "repeats": args.repeats, "iwe_vs_baseline_rel": agree, "shuffled_same_bits": same, "legs": {}}
    for k, v in us.items():
        med = statistics.median(v)
        out["legs"][k] = {"us_median": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                          "atomic_GBps_upper": round(N * atomic_bytes[k] / med / 1e3, 1)}
        print("%-13s %9.1f us (min %.1f, max %.1f)  <= %7.1f GB/s of integer atomics" % (k, med, min(v), max(v), out["legs"][k]["atomic_GBps_upper"]))
    med = statistics.median(base_us)
    out["baseline"] = {"us_median": round(med, 1), "us_min": round(min(base_us), 1), "us_max": round(max(base_us), 1),
                       "over_iwe": round(med / out["legs"]["iwe"]["us_median"], 2)}
    print("baseline      %9.1f us (min %.1f, max %.1f)  = %.2f x the fused iwe call" % (med, min(base_us), max(base_us), out["baseline"]["over_iwe"]))
    print("iwe against the baseline, largest difference / largest value: %.2e; shuffled events, same bits: %s" % (agree, same))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "tracker", "both"), default="both")
    ap.add_argument("--events", type=int, default=1 << 22)
    ap.add_argument("--knots", type=int, default=2000)
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
    assert torch.cuda.is_available(), "event_warp_cost.py measures on the GPU; there is nothing to report without one"
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
