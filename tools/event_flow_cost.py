"""What the per-event optical flow costs: ramp_event_flow (csrc/flow.hip) on a time-sorted stream, against the event filter on
the same events and the stable sort alone.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and
a clock state.

  N = 2^22 time-sorted events of a 640 x 480 sensor, half of them on an edge that sweeps the sensor, the rest uniform noise
  (tools/event_filter_cost.py's stream without the hot pixels), a random polarity.  Legs (device events around the whole call):
    flow r = 1, 2, 3 x refine = 0, 1     without p
    flow r = 1, 2, 3, refine = 1         with p (two surfaces)
    ops.event_filter, activity test      the YARDSTICK: the same order stage plus 8 searches per event
    key + stable sort alone (torch)      the order alone
  Printed per leg: median us (min - max), events per us and the ratio to the filter call.  Nothing is asserted about these times.

    python tools/event_flow_cost.py [--events N] [--repeats R] [--json out.json]
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

WINDOW_DT = 4.0e-3           # at 2^22 events a second on 640 x 480 a pixel fires every 73 ms: the edge fills the window, the noise does not
SUPPORT_DT = 2.0e-3


def make_stream(N, H, W, dev, seed=8, span=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.sort(torch.rand(N, generator=g, dtype=torch.float64) * span).values
    kind = torch.rand(N, generator=g)
    x = torch.rand(N, generator=g) * W
    y = torch.rand(N, generator=g) * H
    x = torch.where(kind < 0.5, (t / span).float() * (W - 1) + torch.randn(N, generator=g) * 0.5, x).clamp(0, W - 0.01)
    p = (torch.randint(0, 2, (N,), generator=g) * 2 - 1).to(torch.int8)
    return x.to(dev), y.to(dev), t.to(dev), p.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1 << 22)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "event_flow_cost.py measures on the GPU; there is nothing to report without one"
    from rampvo_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, H, W = args.events, args.height, args.width
    x, y, t, p = make_stream(N, H, W, dev)

    def sort_alone():
        xt, yt = torch.trunc(x), torch.trunc(y)
        ok = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(t) & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
        return torch.sort(torch.where(ok, yt.int() * W + xt.int(), torch.full_like(xt, H * W, dtype=torch.int32)), stable=True)

    flow = lambda r, refine, pol: (lambda: ops.event_flow(x, y, t, H, W, p=p if pol else None, radius=r, refine=refine, window_dt=WINDOW_DT))
    legs = {"flow r=%d refine=%d" % (r, f): flow(r, f, False) for r in (1, 2, 3) for f in (0, 1)}
    legs.update({"flow r=%d refine=1 with p" % r: flow(r, 1, True) for r in (1, 2, 3)})
    FILTER = "event_filter, activity test"
    legs[FILTER] = lambda: ops.event_filter(x, y, t, H, W, support_dt=SUPPORT_DT)
    legs["key + stable sort alone (torch)"] = sort_alone
    words = {k: (ops.event_flow_status if k.startswith("flow") else ops.event_filter_status)(fn()["status"])
             for k, fn in legs.items() if "sort" not in k}                                               # (also a warm-up round)
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
    out = {"N": N, "H": H, "W": W, "repeats": args.repeats, "device": torch.cuda.get_device_name(dev), "window_dt": WINDOW_DT,
           "support_dt": SUPPORT_DT, "legs": {}}
    base = statistics.median(us[FILTER])
    for k in legs:
        med = statistics.median(us[k])
        out["legs"][k] = {"us_median": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1),
                          "events_per_us": round(N / med, 1), "over_filter": round(med / base, 3), "status": words.get(k)}
        print("%-34s %10.1f us (min %.1f, max %.1f)  %7.1f events / us  %6.2f x filter  %s"
              % (k, med, min(us[k]), max(us[k]), N / med, med / base, words.get(k, "")))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
