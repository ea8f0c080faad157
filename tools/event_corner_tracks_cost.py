"""What linking corners into tracks costs: ramp_event_corner_tracks (csrc/cornertrack.hip) on the wedge stream of
tools/event_corners_cost.py, with the detector's own answer as the mask, against the detector and the stable sort alone.  ONE
process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  N = 2^22 time-sorted events of a 640 x 480 sensor (event_corners_cost.make_stream).  max_dt = 4 ms of a 1 s stream.
  Legs (device events around the whole call):
    tracks rho = 1, 3, 5                  the detector's corners as candidates, without p
    tracks rho = 1, 3, 5 with p           two planes
    tracks rho = 3, corner=None           every valid event a candidate: the most links the stream can give
    ops.event_corners                     YARDSTICK: the same order stage over every event, 16 + 20 searches per event
    key + stable sort alone (torch)       YARDSTICK: the same keys (a non-candidate takes the sentinel) through torch.sort
  Printed per leg: median us (min - max), events per us and the ratio to the detector's call.  Then, from one profiled call per
  tracks leg (torch.profiler, kernel times by name), the share of the pointer-jumping launches in the call's kernel time;
  "unmeasured" where the profiler gives no kernel times.  Nothing is asserted about these times.

    python tools/event_corner_tracks_cost.py [--events N] [--repeats R] [--json out.json]
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

from event_corners_cost import make_stream, timed  # noqa: E402

MAX_DT = 4.0e-3


def jump_share(fn):
    """(share of trk_jump_kernel in the kernel time of one call, the kernel time in us), or None without kernel times"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [(e.key, getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)) for e in prof.key_averages()]
    except Exception:                                               # (no profiler in this build: the share stays unmeasured)
        return None
    total = sum(us for _, us in rows)
    jump = sum(us for k, us in rows if "trk_jump_kernel" in k)
    return (jump / total, total) if total > 0 and jump > 0 else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1 << 22)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "event_corner_tracks_cost.py measures on the GPU; there is nothing to report without one"
    from rampvo_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, H, W = args.events, args.height, args.width
    x, y, t, p = make_stream(N, H, W, dev)
    corner = ops.event_corners(x, y, t, H, W, want_index=False)["corner"]
    corner_p = ops.event_corners(x, y, t, H, W, p=p, want_index=False)["corner"]

    def sort_alone():
        xt, yt = torch.trunc(x), torch.trunc(y)
        ok = corner & torch.isfinite(x) & torch.isfinite(y) & torch.isfinite(t) & (xt >= 0) & (xt <= W - 1) & (yt >= 0) & (yt <= H - 1)
        return torch.sort(torch.where(ok, yt.int() * W + xt.int(), torch.full_like(xt, H * W, dtype=torch.int32)), stable=True)

    DETECTOR = "event_corners"
    legs = {}
    for r in (1, 3, 5):
        legs["tracks rho=%d" % r] = lambda r=r: ops.event_corner_tracks(x, y, t, H, W, corner=corner, radius=r, max_dt=MAX_DT)
        legs["tracks rho=%d with p" % r] = lambda r=r: ops.event_corner_tracks(x, y, t, H, W, corner=corner_p, p=p, radius=r, max_dt=MAX_DT)
    legs["tracks rho=3 corner=None"] = lambda: ops.event_corner_tracks(x, y, t, H, W, radius=3, max_dt=MAX_DT)
    legs[DETECTOR] = lambda: ops.event_corners(x, y, t, H, W)
    legs["key + stable sort alone (torch)"] = sort_alone
    words = {k: ops.event_corner_tracks_status(fn()["status"]) for k, fn in legs.items() if k.startswith("tracks")}      # (also a warm-up round)
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
    out = {"N": N, "H": H, "W": W, "repeats": args.repeats, "device": torch.cuda.get_device_name(dev), "max_dt": MAX_DT, "legs": {}}
    base = statistics.median(us[DETECTOR])
    for k in legs:
        med = statistics.median(us[k])
        out["legs"][k] = {"us_median": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1),
                          "events_per_us": round(N / med, 1), "over_detector": round(med / base, 3), "status": words.get(k)}
        print("%-34s %10.1f us (min %.1f, max %.1f)  %7.1f events / us  %6.2f x detector  %s"
              % (k, med, min(us[k]), max(us[k]), N / med, med / base, words.get(k, "")))
    for k, fn in legs.items():
        if k.startswith("tracks"):
            share = jump_share(fn)
            out["legs"][k]["jump_share"] = None if share is None else round(share[0], 3)
            print("%-34s pointer jumping: %s" % (k, "unmeasured" if share is None else "%.1f %% of %.1f us of kernels" % (100 * share[0], share[1])))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
