"""What rendering the event map costs: ramp_point_map_render (csrc/maprender.hip) against a torch restatement on the same
device, against the table read alone, and behind the tracker.  ONE process, rounds INTERLEAVED over the legs, so that
everything shares a box and a clock state.

  kernel   The scene of tools/event_map_cost.py: capacity 2^22 holding about 2^18 voxels (2^20 points spread over a cube),
           seen at 640 x 480 from a camera four cube sides away.  Legs (device events around the whole call: the memset of the
           status words and the four launches):
             r0 / r3 / r0 fp / r3 fp   radius 0 and 3, footprint off and on
             empty                     the call on a cleared table of the same capacity: the two table reads alone
             clear                     the table's one launch (256 MiB): the yardstick of one pass over the table
           baseline, quoted against r0 and r3: export, the transform and projection of the exported points in torch, and one
           scatter_reduce_(amax) of the inverse depths per pixel of the footprint.
  tracker  BASELINE configs[1] (SingleScale 640 x 480, 96 patches, fp16 features), after a map has been built from three
           views: a / b / c / d = no query / compensate_events(invdepth=None) / compensate_events(invdepth="event_map") /
           compensate_events(invdepth="events") of 2 10^5 device-resident events behind every frame; kf/s per leg.

    timeout -k 10 600 python tools/event_map_render_cost.py --part kernel --json runs/event_map_render_kernel.json && \\
    timeout -k 10 1100 python tools/event_map_render_cost.py --part tracker --json runs/event_map_render_tracker.json
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


def _render_baseline(pmap, cam, K, H, W, radius):
    """export + transform / project + scatter_reduce_(amax): the depth image alone (no key, n or conf)"""
    e = pmap.export()
    k = int(e["count"].cpu())                                            # (torch needs the count on the host: part of its cost)
    X = e["points"][:k] - cam[:3]
    qv = -cam[3:6]
    uv = 2.0 * torch.cross(qv.expand_as(X), X, dim=-1)
    Xc = X + cam[6] * uv + torch.cross(qv.expand_as(X), uv, dim=-1)
    ok = Xc[:, 2] > 0.2
    d = 1.0 / Xc[ok, 2]
    px = torch.round(K[0] * Xc[ok, 0] * d + K[2]).long()
    py = torch.round(K[1] * Xc[ok, 1] * d + K[3]).long()
    img = torch.zeros(H * W, device=X.device)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            x, y = px + dx, py + dy
            m = (x >= 0) & (x < W) & (y >= 0) & (y < H)
            img.scatter_reduce_(0, (y * W + x)[m], d[m], "amax")
    return img.view(H, W)


def kernel_part(args, dev):
    from rampvo_amd import ops
    N, cap, H, W = args.points, args.capacity, args.height, args.width
    g = torch.Generator(device="cpu").manual_seed(8)
    voxel = 0.05
    side = round((1 << 18) ** (1.0 / 3.0)) * voxel                      # a cube of about 2^18 voxels
    spread = ((torch.rand((N, 3), generator=g) - 0.5) * side).to(dev)
    conf = (torch.rand(N, generator=g) * 4.0).to(dev)
    cam = torch.tensor([0.0, 0.0, -4.0 * side, 0.0, 0.0, 0.0, 1.0], device=dev)
    K = torch.tensor([320.0 * 4, 320.0 * 4, 319.5, 239.5], device=dev)   # the cube fills 320 pixels of the image's 640
    full, empty = ops.PointMap(voxel, capacity=cap), ops.PointMap(voxel, capacity=cap)
    full.insert(spread, conf)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    render = lambda m, r, fp: m.render(cam, K, H, W, radius=r, footprint=fp)
    legs = {"r0": (lambda: render(full, 0, False), 0), "r3": (lambda: render(full, 3, False), 3), "r0 fp": (lambda: render(full, 0, True), None),
            "r3 fp": (lambda: render(full, 3, True), None), "empty": (lambda: render(empty, 3, False), None), "clear": (empty.clear, None)}
    base = {0: lambda: _render_baseline(full, cam, K, H, W, 0), 3: lambda: _render_baseline(full, cam, K, H, W, 3)}
    info = {}
    for name, r, fp in (("r0", 0, False), ("r3", 3, False), ("r0 fp", 0, True), ("r3 fp", 3, True)):
        out = render(full, r, fp)
        info[name] = {"status": ops.point_map_render_status(out["status"])}
        if not fp:
            ref = base[r]()
            won = out["key"] >= 0
            info[name]["same_pixels_as_torch"] = bool(torch.equal(won, ref > 0))
            info[name]["largest_difference_from_torch"] = float((out["invdepth"][won] - ref[won]).abs().max())
    for fn, _ in legs.values():
        for _ in range(args.warmup):
            timed(fn)
    for fn in base.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us, base_us = {k: [] for k in legs}, {k: [] for k in base}
    for rep in range(args.repeats):
        for k, (fn, _) in legs.items():
            us[k].append(timed(fn))
        if rep < args.baseline_repeats:
            for k in base:
                base_us[k].append(timed(base[k]))
    out = {"points": N, "capacity": cap, "H": H, "W": W, "repeats": args.repeats, "baseline_repeats": args.baseline_repeats, "legs": {}, "info": info}
    for k, v in us.items():
        med = statistics.median(v)
        row = dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1))
        if legs[k][1] is not None:
            bmed = statistics.median(base_us[legs[k][1]])
            row.update(baseline_us_median=round(bmed, 1), baseline_over_kernel=round(bmed / med, 2))
        out["legs"][k] = row
        print("%-8s %10.1f us (min %.1f, max %.1f)%s" % (k, med, min(v), max(v), "" if "baseline_us_median" not in row else
                                                      ";  torch %10.1f us = %.2f x" % (row["baseline_us_median"], row["baseline_over_kernel"])))
    clear = out["legs"]["clear"]["us_median"]
    out["table_reads_per_call"] = 2
    out["empty_over_two_clears"] = round(out["legs"]["empty"]["us_median"] / (2 * clear), 2)
    # what the atomics add: the full table's call less the empty table's, per return-less atomic of each kind (every rendered
    # slot issues at most (2 r + 1)^2 of each)
    st = info["r3"]["status"]
    out["atomics_r3"] = {"rendered_slots": st["n_rendered"], "upper_bound_per_kind": st["n_rendered"] * 49,
                         "us_over_empty": round(out["legs"]["r3"]["us_median"] - out["legs"]["empty"]["us_median"], 1)}
    print("empty / (2 clears) = %.2f; r3 less empty: %.1f us for at most %d atomics of each kind"
          % (out["empty_over_two_clears"], out["atomics_r3"]["us_over_empty"], out["atomics_r3"]["upper_bound_per_kind"]))
    for k, v in info.items():
        print("%-8s %s" % (k, v))
    return out


def tracker_part(args, dev):
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 4, warmup), dev)
    slam, n_ev = t.slam, args.tracker_events
    g = torch.Generator(device="cpu").manual_seed(9)
    ex = (torch.rand(n_ev, generator=g) * (args.width - 1)).to(dev)
    ey = (torch.rand(n_ev, generator=g) * (args.height - 1)).to(dev)
    ep = torch.where(torch.rand(n_ev, generator=g) < 0.5, 1, -1).to(torch.int8).to(dev)
    frac = torch.sort(torch.rand(n_ev, generator=g, dtype=torch.float64)).values.to(dev)      # time-sorted, in the last two frames
    t.prime(args.prime, args.clock_warm)
    slam.event_map(capacity=args.tracker_capacity)
    for back in (6, 4, 2):                                               # the map: three views behind the newest frame
        slam.event_map_insert(ex, ey, float(t.pos - 1 - back) + 2.0 * frac, t_ref=float(t.pos - 1 - back + 2), planes=args.tracker_planes,
                              as_tensor=True)
    last = {}

    def ask(invdepth):
        def leg():
            last[str(invdepth)] = slam.compensate_events(ex, ey, float(t.pos - 3) + 2.0 * frac, ep, invdepth=invdepth, as_tensor=True)["status"]
        return leg

    what = {"a": "no query", "b": "compensate_events(invdepth=None)", "c": "compensate_events(invdepth='event_map')",
            "d": "compensate_events(invdepth='events')"}
    rates, _ = t.run_legs({"a": None, "b": ask(None), "c": ask("event_map"), "d": ask("events")}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "planes": args.tracker_planes, "steps": steps, "repeats": repeats,
           "frames_at_end": t.pos, "voxel": slam.event_map().voxel, "capacity": slam.event_map().capacity}
    out["legs"] = tl.summary(rates, what)
    for k in "bcd":
        out[k + "_over_a"] = tl.ratio(out["legs"], k, "a")
    out["a_spread"] = tl.spread(out["legs"]["a"])
    from rampvo_amd import ops
    out["render_status"] = ops.point_map_render_status(slam.event_map_depth(as_tensor=True)["status"])
    out["last_status"] = {k: v.cpu().tolist() for k, v in last.items()}
    print("b / a = %.4f  c / a = %.4f  d / a = %.4f   (a's own spread, (max - min) / median: %.4f); render %s"
          % (out["b_over_a"], out["c_over_a"], out["d_over_a"], out["a_spread"], out["render_status"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "tracker", "both"), default="kernel")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--capacity", type=int, default=1 << 22)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--baseline-repeats", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tracker-repeats", type=int, default=5)
    ap.add_argument("--tracker-warmup", type=int, default=20)
    ap.add_argument("--tracker-events", type=int, default=200000)
    ap.add_argument("--tracker-planes", type=int, default=64)
    ap.add_argument("--tracker-capacity", type=int, default=1 << 20)
    ap.add_argument("--prime", type=int, default=70)
    ap.add_argument("--clock-warm", type=int, default=480)
    ap.add_argument("--patches", type=int, default=96)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "event_map_render_cost.py measures on the GPU; there is nothing to report without one"
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
