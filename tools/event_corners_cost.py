"""What event corner detection costs: ramp_event_corners (csrc/corner.hip) on a time-sorted stream, against the event flow at
r = 3 (the same order stage and 48 searches per event), the event filter and the stable sort alone.  ONE process, rounds
INTERLEAVED over the legs, so that everything shares a box and a clock state.

  N = 2^22 time-sorted events of a 640 x 480 sensor, half of them on the two edges of wedges that move across the sensor (each
  edge event lies where a wedge's boundary is at the event's time, so the surface behind an apex is a corner's), the rest
  uniform noise, a random polarity per wedge and per noise event.  Legs (device events around the whole call):
    corners                               without p, index and count
    corners with p                        two surfaces
    corners wide                          the Arc* acceptance
    corners with arc, index and the map   every output
    ops.event_flow r = 3, refine = 1      YARDSTICK: the same order stage, 48 searches per event and a plane fit
    ops.event_filter, activity test       YARDSTICK: the same order stage plus 8 searches per event
    key + stable sort alone (torch)       the order alone
  Printed per leg: median us (min - max), events per us and the ratio to the filter call.  Nothing is asserted about these times.

    python tools/event_corners_cost.py [--events N] [--repeats R] [--json out.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOW_DT = 4.0e-3
SUPPORT_DT = 2.0e-3
WEDGES = 64


def make_stream(N, H, W, dev, seed=8, span=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.sort(torch.rand(N, generator=g, dtype=torch.float64) * span).values
    tf = (t / span).float()
    # the wedges: an apex that starts anywhere and crosses a third of the sensor, a half opening angle of 27 to 45 degrees
    ang = torch.rand(WEDGES, generator=g) * 2 * math.pi
    half = torch.atan(0.5 + 0.5 * torch.rand(WEDGES, generator=g))
    x0, y0 = torch.rand(WEDGES, generator=g) * W, torch.rand(WEDGES, generator=g) * H
    pol = (torch.randint(0, 2, (WEDGES,), generator=g) * 2 - 1).to(torch.int8)
    j = torch.randint(0, WEDGES, (N,), generator=g)
    side = torch.randint(0, 2, (N,), generator=g).float() * 2 - 1
    s = torch.rand(N, generator=g) * 40.0                           # the distance from the apex along the edge, in pixels
    edge = ang[j] + math.pi + side * half[j]                        # the edges trail the apex
    ax, ay = x0[j] + tf * (W / 3.0) * torch.cos(ang[j]), y0[j] + tf * (W / 3.0) * torch.sin(ang[j])
    wx, wy = torch.remainder(ax + s * torch.cos(edge), W), torch.remainder(ay + s * torch.sin(edge), H)
    noise = torch.rand(N, generator=g) < 0.5
    x = torch.where(noise, torch.rand(N, generator=g) * W, wx).clamp(0, W - 0.01)
    y = torch.where(noise, torch.rand(N, generator=g) * H, wy).clamp(0, H - 0.01)
    p = torch.where(noise, (torch.randint(0, 2, (N,), generator=g) * 2 - 1).to(torch.int8), pol[j])
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
    assert torch.cuda.is_available(), "event_corners_cost.py measures on the GPU; there is nothing to report without one"
    from rampvo_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, H, W = args.events, args.height, args.width
    x, y, t, p = make_stream(N, H, W, dev)

    def sort_alone():
        xt, yt = torch.trunc(x), torch.trunc(y)
        ok = torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(t) & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
        return torch.sort(torch.where(ok, yt.int() * W + xt.int(), torch.full_like(xt, H * W, dtype=torch.int32)), stable=True)

    FILTER = "event_filter, activity test"
    legs = {"corners": lambda: ops.event_corners(x, y, t, H, W),
            "corners with p": lambda: ops.event_corners(x, y, t, H, W, p=p),
            "corners wide": lambda: ops.event_corners(x, y, t, H, W, wide=True),
            "corners with arc, index and the map": lambda: ops.event_corners(x, y, t, H, W, want_arc=True, want_map=True),
            "event_flow r=3 refine=1": lambda: ops.event_flow(x, y, t, H, W, radius=3, refine=1, window_dt=WINDOW_DT),
            FILTER: lambda: ops.event_filter(x, y, t, H, W, support_dt=SUPPORT_DT),
            "key + stable sort alone (torch)": sort_alone}
    decode = lambda k: ops.event_corners_status if k.startswith("corners") else (ops.event_flow_status if "flow" in k else ops.event_filter_status)
    words = {k: decode(k)(fn()["status"]) for k, fn in legs.items() if "sort" not in k}                  # (also a warm-up round)
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
        print("%-38s %10.1f us (min %.1f, max %.1f)  %7.1f events / us  %6.2f x filter  %s"
              % (k, med, min(us[k]), max(us[k]), N / med, med / base, words.get(k, "")))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
