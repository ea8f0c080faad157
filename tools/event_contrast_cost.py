"""What scoring the compensation costs: ramp_event_contrast (csrc/contrast.hip) beside ramp_event_warp's image leg.  ONE
process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.  Nothing here fixes a rate.

  N = 2^22 events, T = 2000 knots, 640 x 480 (the scene of tools/event_warp_cost.py).  Legs (device events around the whole
  call: memset + launches):
    contrast        statistics only (want_grad=False): segment, splat, finish, final
    contrast+grad   the gradient launch as well: a second pass over the events, gathers instead of atomics
    iwe             ops.event_warp's image of warped events, for scale
  Printed per leg: median us, min, max.

  tracker  pose_query_cost.py's two interleaved legs on BASELINE configs[1]: no query / event_contrast(2 10^5 device-resident
           events of the last two frames, as_tensor=True, with the gradient) behind every frame; kf/s per leg, b / a, a's spread.

    python tools/event_contrast_cost.py [--part kernel|tracker|both] [--events N] [--repeats R] [--json out.json]
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
from event_warp_cost import _knots


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
        last[0] = t.slam.event_contrast(ex, ey, float(t.pos - 3) + 2.0 * frac, ep, as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": query}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "steps": steps, "repeats": repeats, "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "event_contrast(%d events) per frame" % n_ev})
    out["b_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.spread(out["legs"]["a"])
    out["last_status"], out["last_variance"] = last[0]["status"].cpu().tolist(), float(last[0]["variance"])
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f); last status %s, variance %.6g"
          % (out["b_over_a"], out["a_spread"], out["last_status"], out["last_variance"]))
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
    K = torch.tensor([320.0, 320.0, 319.5, 239.5], device=dev)
    theta = torch.tensor([0.01, -0.02, 0.01, 0.02, -0.01, 0.03, 0.05], device=dev)
    t_ref = float(times[-1]) * 0.5
    legs = {
        "contrast": lambda: ops.event_contrast(x, y, t, p, knots, times, t_ref, K, 0.5, H, W, correction=theta, want_grad=False),
        "contrast+grad": lambda: ops.event_contrast(x, y, t, p, knots, times, t_ref, K, 0.5, H, W, correction=theta),
        "iwe": lambda: ops.event_warp(x, y, t, p, knots, times, t_ref, K, 0.5, H, W),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    same = torch.equal(ops.event_contrast(x, y, t, p, knots, times, t_ref, K, 0.5, H, W, want_iwe=True)["iwe"].view(torch.int32),
                       legs["iwe"]()["iwe"].view(torch.int32))
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
    out = {"N": N, "T": T, "H": H, "W": W, "repeats": args.repeats, "zero_correction_same_bits_as_warp": same, "legs": {}}
    for k, v in us.items():
        med = statistics.median(v)
        out["legs"][k] = {"us_median": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1)}
        print("%-14s %9.1f us (min %.1f, max %.1f)" % (k, med, min(v), max(v)))
    print("zero correction, the same image bits as ops.event_warp: %s" % same)
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
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tracker-repeats", type=int, default=5)
    ap.add_argument("--tracker-warmup", type=int, default=20)
    ap.add_argument("--tracker-events", type=int, default=200000)
    ap.add_argument("--prime", type=int, default=70)
    ap.add_argument("--clock-warm", type=int, default=480)
    ap.add_argument("--patches", type=int, default=96)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "event_contrast_cost.py measures on the GPU; there is nothing to report without one"
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
