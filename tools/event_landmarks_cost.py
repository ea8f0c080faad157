"""What triangulating corner tracks costs: ramp_event_landmarks (csrc/landmark.hip) on the wedge stream of
tools/event_corners_cost.py, with the tracks of ops.event_corner_tracks and a synthetic trajectory, against a torch restatement
on the same device.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  N = 2^22 time-sorted events of a 640 x 480 sensor (event_corners_cost.make_stream), the detector's corners linked with
  rho = 3 and max_dt = 4 ms; 2,000 knots over the stream: a camera that moves sideways and turns a little.
  Legs (device events around the whole call):
    landmarks refine = 0, refine = 2      ops.event_landmarks, min_parallax = 0
    torch restatement (midpoint)          YARDSTICK: torch.sort by (id, t), poses by ops.se3_interp, the midpoint sums through
                                          index_add_ in float64 and a batched torch.linalg.solve -- no refinement, no classes
    the two sorts alone (torch)           YARDSTICK: two stable torch.sort calls over the same keys
  Printed per leg: median us (min - max) and events per us; then the two sorts' share of the landmark call.  Nothing is
  asserted about these times.

    python tools/event_landmarks_cost.py [--events N] [--knots T] [--repeats R] [--json out.json]
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

from event_corners_cost import make_stream, timed  # noqa: E402

MAX_DT = 4.0e-3


def trajectory(T, t0, t1, dev):
    s = torch.linspace(0.0, 1.0, T, dtype=torch.float64, device=dev)
    yaw = -0.25 * (s - 0.5)
    knots = torch.stack([3.0 * s - 1.5, 0.4 * torch.sin(2.0 * s), 0.3 * s, torch.zeros_like(s), torch.sin(yaw / 2), torch.zeros_like(s),
                         torch.cos(yaw / 2)], 1)
    return knots.float().contiguous(), (t0 + (t1 - t0) * s).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--events", type=int, default=1 << 22)
    ap.add_argument("--knots", type=int, default=2000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "event_landmarks_cost.py measures on the GPU; there is nothing to report without one"
    from rampvo_amd import ops
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    N, H, W, T = args.events, args.height, args.width, args.knots
    x, y, t, p = make_stream(N, H, W, dev)
    corner = ops.event_corners(x, y, t, H, W, want_index=False)["corner"]
    track = ops.event_corner_tracks(x, y, t, H, W, corner=corner, radius=3, max_dt=MAX_DT)["track"]
    fin = t[torch.isfinite(t)]
    knots, times = trajectory(T, float(fin.min()), float(fin.max()), dev)
    K = torch.tensor([0.8 * W, 0.8 * W, W / 2.0, H / 2.0], dtype=torch.float32, device=dev)
    xf, yf = x.float(), y.float()
    none = torch.iinfo(torch.int64).max

    def keys():
        ok = (track >= 0) & torch.isfinite(xf) & torch.isfinite(yf) & torch.isfinite(t)
        return ok, torch.where(ok, track, torch.full_like(track, none))

    def sorts_alone():
        ok, ids = keys()
        o1 = torch.sort(torch.where(ok, t, torch.full_like(t, math.inf)), stable=True)[1]
        return torch.sort(ids[o1], stable=True)

    def restatement():
        ok, ids = keys()
        o1 = torch.sort(torch.where(ok, t, torch.full_like(t, math.inf)), stable=True)[1]
        sid, o2 = torch.sort(ids[o1], stable=True)
        order = o1[o2]
        n_obs = int(0) + ok.sum()                                      # (a device count: the restatement may slice by it)
        order, sid = order[:n_obs], sid[:n_obs]
        poses = ops.se3_interp(knots, times, t[order])[0].double()
        f = torch.stack([(xf[order] - K[2]) / K[0], (yf[order] - K[3]) / K[1], torch.ones_like(xf[order])], 1).double()
        q, c = poses[:, 3:], poses[:, :3]
        uv = 2.0 * torch.cross(q[:, :3], f, dim=1)
        d = f + q[:, 3:4] * uv + torch.cross(q[:, :3], uv, dim=1)
        u = d / d.norm(dim=1, keepdim=True)
        lm = torch.unique_consecutive(sid, return_inverse=True)[1]
        L = int(lm[-1]) + 1 if lm.numel() else 0
        M = torch.eye(3, dtype=torch.float64, device=dev)[None] - u[:, :, None] * u[:, None, :]
        A = torch.zeros((L, 3, 3), dtype=torch.float64, device=dev).index_add_(0, lm, M)
        b = torch.zeros((L, 3), dtype=torch.float64, device=dev).index_add_(0, lm, (M @ c[:, :, None])[:, :, 0])
        return torch.linalg.solve(A + 1e-12 * torch.eye(3, dtype=torch.float64, device=dev), b)

    legs = {"landmarks refine=%d" % r: (lambda r=r: ops.event_landmarks(xf, yf, t, track, knots, times, K, refine=r, min_parallax=0.0))
            for r in (0, 2)}
    legs["torch restatement (midpoint)"] = restatement
    legs["the two sorts alone (torch)"] = sorts_alone
    words = {k: ops.event_landmarks_status(fn()["status"]) for k, fn in legs.items() if k.startswith("landmarks")}
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
    out = {"N": N, "T": T, "repeats": args.repeats, "device": torch.cuda.get_device_name(dev), "legs": {}}
    for k in legs:
        med = statistics.median(us[k])
        out["legs"][k] = {"us_median": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1),
                          "events_per_us": round(N / med, 1), "status": words.get(k)}
        print("%-34s %10.1f us (min %.1f, max %.1f)  %7.1f events / us  %s" % (k, med, min(us[k]), max(us[k]), N / med, words.get(k, "")))
    sorts = statistics.median(us["the two sorts alone (torch)"])
    for k in legs:
        if k.startswith("landmarks"):
            out["legs"][k]["sorts_share"] = round(sorts / statistics.median(us[k]), 3)
            print("%-34s two stable torch sorts are %.0f %% of the call" % (k, 100 * out["legs"][k]["sorts_share"]))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
