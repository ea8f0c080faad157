"""What the event filter costs: ramp_event_filter (csrc/filter.hip) on a time-sorted stream, and how much of it is the library's
stable sort.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  kernel part: N = 2^22 time-sorted events of a 640 x 480 sensor (a moving edge, uniform noise, 16 hot pixels).  Legs (device
  events around the whole call):
    all three predicates           support_dt, refractory, hot_sigma; xy and index requested
    the activity test alone        support_dt; xy requested
    key + stable sort alone        the YARDSTICK: the same pixel keys formed with torch ops and ``torch.sort(stable=True)`` -- what a
                                   caller pays for the order alone, before any predicate
    one pixel with 2^20 events     the long-segment case: a quarter of the events sit on one pixel that is not hot (its
                                   neighbours search a segment of 2^20), all three predicates
  tracker part: configs[1] with ``filter_events`` of 2 10^5 events behind every frame (the state carried, the stamps advancing
  frame by frame), against no query.
  Printed per leg: median us (min - max) and events per second.  Nothing is asserted about these times.

    python tools/event_filter_cost.py [--part kernel|tracker|both] [--events N] [--repeats R] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

PARAMS = dict(support_dt=2.0e-3, refractory=2.0e-4, hot_sigma=4.0)


def make_stream(N, H, W, dev, seed=8, span=1.0):
    """time-sorted: half the events on an edge that sweeps the sensor, a little under half uniform noise, 1 / 64 on 16 hot pixels"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.sort(torch.rand(N, generator=g, dtype=torch.float64) * span).values
    kind = torch.rand(N, generator=g)
    x = torch.rand(N, generator=g) * W
    y = torch.rand(N, generator=g) * H
    edge = kind < 0.5
    x = torch.where(edge, (t / span).float() * (W - 1) + torch.randn(N, generator=g) * 0.5, x).clamp(0, W - 0.01)
    spots = torch.randint(0, H * W, (16,), generator=g)
    hot = kind > 1.0 - 1.0 / 64
    at = spots[torch.randint(0, 16, (N,), generator=g)]
    x = torch.where(hot, (at % W).float() + 0.5, x)
    y = torch.where(hot, (at // W).float() + 0.5, y)
    return x.to(dev), y.to(dev), t.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                      # us


def kernel_part(args, dev):
    from rampvo_amd import ops
    N, H, W = args.events, args.height, args.width
    x, y, t = make_stream(N, H, W, dev)
    xl, yl = x.clone(), y.clone()
    big = torch.randperm(N, generator=torch.Generator(device="cpu").manual_seed(3))[:N // 4].to(dev)
    xl[big], yl[big] = W // 2 + 0.5, H // 2 + 0.5

    def sort_alone():
        ok = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(t)
        xt, yt = torch.trunc(x), torch.trunc(y)
        ok = ok & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
        key = torch.where(ok, yt.int() * W + xt.int(), torch.full_like(xt, H * W, dtype=torch.int32))
        return torch.sort(key, stable=True)

    legs = {
        "all three predicates": lambda: ops.event_filter(x, y, t, H, W, want_index=True, **PARAMS),
        "the activity test alone": lambda: ops.event_filter(x, y, t, H, W, support_dt=PARAMS["support_dt"]),
        "key + stable sort alone (torch)": sort_alone,
        "one pixel with N / 4 events": lambda: ops.event_filter(xl, yl, t, H, W, want_index=True, **dict(PARAMS, hot_sigma=0.0)),
    }
    words = {k: ops.event_filter_status(fn()["status"]) for k, fn in legs.items() if "sort" not in k}     # (also a warm-up round)
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
    out = {"N": N, "H": H, "W": W, "repeats": args.repeats, "device": torch.cuda.get_device_name(dev), "params": PARAMS, "legs": {}}
    for k in legs:
        med = statistics.median(us[k])
        out["legs"][k] = {"us_median": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1),
                          "events_per_us": round(N / med, 1), "status": words.get(k)}
        print("%-34s %9.1f us (min %.1f, max %.1f)   %7.1f events / us   %s" % (k, med, min(us[k]), max(us[k]), N / med, words.get(k, "")))
    return out


def tracker_part(args, dev):
    import tracker_legs as tl
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 2, warmup), dev)
    n_ev, span = args.tracker_events, 0.05
    ex, ey, et = make_stream(n_ev, args.height, args.width, dev, seed=9, span=span)
    t.slam.set_event_filter(**PARAMS)
    t.prime(args.prime, args.clock_warm)
    last, calls = [None], [0]

    def query():
        last[0] = t.slam.filter_events(ex, ey, et + calls[0] * span, as_tensor=True)     # (the stream goes on: the state is carried)
        calls[0] += 1

    rates, _ = t.run_legs({"a": None, "b": query}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "steps": steps, "repeats": repeats, "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "filter_events(%d events) per frame" % n_ev})
    out["b_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.spread(out["legs"]["a"])
    out["last_status"] = last[0]["status"].cpu().tolist()
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f); last status %s" % (out["b_over_a"], out["a_spread"], out["last_status"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "tracker", "both"), default="both")
    ap.add_argument("--events", type=int, default=1 << 22)
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
    assert torch.cuda.is_available(), "event_filter_cost.py measures on the GPU; there is nothing to report without one"
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
