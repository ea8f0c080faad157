"""What the event map costs: ramp_depth_points and ramp_point_map_* (csrc/evmap.hip) against torch restatements on the same
device, and behind the tracker.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  kernel   Legs (device events around the whole call: the memset of the status words and every launch):
             insert spread     2^20 points into capacity 2^22, spread over about 2^18 voxels
             insert 64 voxels  2^20 points into capacity 2^22, all inside 64 voxels (contention on 64 lines)
             depth_points      640 x 480, median_radius 2, min_support 3, a quarter of the pixels detected
             export            the table of the spread leg (2^22 slots: flag, radix sort, gather)
             clear             the table's one launch (256 MiB)
           Each insert leg starts from a cleared table (the clear is outside the timed region).
           baselines, each quoted against its own leg: insert -- floor / rint of the float64 coordinates,
           torch.unique(return_inverse=True) over the keys, index_add_ of the counts, fractions and confidences; depth_points --
           unfold of the masked map with +inf in the place of undetected pixels, sort, gather of the lower median, the lift and a
           boolean-mask compaction; export -- a boolean mask over the table's key words and torch.sort.
  tracker  BASELINE configs[1] (SingleScale 640 x 480, 96 patches, fp16 features): a / b = no query / event_map_insert of
           2 10^5 device-resident events of the last two frames behind every frame; kf/s per leg, b / a, a's own spread.

    timeout -k 10 600 python tools/event_map_cost.py --part kernel --json runs/event_map_kernel.json && \\
    timeout -k 10 900 python tools/event_map_cost.py --part tracker --json runs/event_map_tracker.json
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

AXIS = 1 << 20


def _insert_baseline(points, conf, voxel):
    g = points.double() / voxel
    i = torch.floor(g)
    q = torch.round((g - i) * AXIS).long()
    ii = i.long() + AXIS
    key = (ii[:, 0] << 42) | (ii[:, 1] << 21) | ii[:, 2]
    uk, inv = torch.unique(key, return_inverse=True)
    n = torch.zeros(uk.shape[0], dtype=torch.int64, device=points.device).index_add_(0, inv, torch.ones_like(inv))
    sq = torch.zeros((uk.shape[0], 3), dtype=torch.int64, device=points.device).index_add_(0, inv, q)
    sc = torch.zeros(uk.shape[0], dtype=torch.int64, device=points.device).index_add_(0, inv, torch.round(conf.double() * 65536.0).long())
    return uk, n, sq, sc


def _points_baseline(inv, plane, conf, cam, K, r, s):
    H, W = inv.shape
    det = plane >= 0
    pad = torch.nn.functional.pad(torch.where(det, inv, torch.full_like(inv, float("inf")))[None, None], (r, r, r, r), value=float("inf"))
    win = torch.nn.functional.unfold(pad, 2 * r + 1)[0]                      # [(2r+1)^2, H*W]
    n = torch.isfinite(win).sum(0)
    srt = torch.sort(win, 0).values
    med = srt.gather(0, ((n - 1).clamp(min=0) // 2)[None])[0]
    keep = det.reshape(-1) & (n >= s) & torch.isfinite(med) & (med > 0)
    v, u = torch.div(torch.arange(H * W, device=inv.device), W, rounding_mode="floor"), torch.arange(H * W, device=inv.device) % W
    z = 1.0 / med
    Xc = torch.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], -1)
    uv = 2.0 * torch.cross(cam[3:6].expand_as(Xc), Xc, dim=-1)
    Xw = Xc + cam[6] * uv + torch.cross(cam[3:6].expand_as(Xc), uv, dim=-1) + cam[:3]
    return Xw[keep], conf.reshape(-1)[keep], torch.nonzero(keep)


def _export_baseline(buf, capacity):
    words = buf[64:].view(torch.int64).view(capacity, 8)
    keep = (words[:, 0] != -1) & (words[:, 1] >= 1)
    key, order = torch.sort(words[:, 0][keep])
    rows = words[keep][order]
    return key, rows[:, 2:5].double() / rows[:, 1:2].double()


def kernel_part(args, dev):
    from rampvo_amd import ops
    N, cap, H, W = args.points, args.capacity, args.height, args.width
    g = torch.Generator(device="cpu").manual_seed(8)
    voxel = 0.05
    side = round((1 << 18) ** (1.0 / 3.0)) * voxel                      # a cube of about 2^18 voxels
    spread = ((torch.rand((N, 3), generator=g) - 0.5) * side).to(dev)
    tight = (torch.rand((N, 3), generator=g) * torch.tensor([4.0, 4.0, 4.0]) * voxel).to(dev)      # 4 x 4 x 4 voxels
    conf = (torch.rand(N, generator=g) * 4.0).to(dev)
    inv = (0.2 + 1.2 * torch.rand((H, W), generator=g)).to(dev)
    plane = torch.where(torch.rand((H, W), generator=g) < 0.25, 1, -1).to(torch.int32).to(dev)
    pconf = torch.ones((H, W), device=dev)
    cam = torch.tensor([0.3, -0.2, 0.5, 0.18257419, -0.36514837, 0.54772256, 0.73029674], device=dev)
    K = torch.tensor([320.0, 320.0, 319.5, 239.5], device=dev)
    table, full = ops.PointMap(voxel, capacity=cap), ops.PointMap(voxel, capacity=cap)
    full.insert(spread, conf)

    def timed(fn, before=None):
        if before is not None:
            before()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    legs = {"insert spread": (lambda: table.insert(spread, conf), table.clear, "insert spread"),
            "insert 64 voxels": (lambda: table.insert(tight, conf), table.clear, "insert 64 voxels"),
            "depth_points": (lambda: ops.depth_points(inv, cam, K, plane=plane, confidence=pconf, median_radius=2, min_support=3), None,
                             "depth_points"),
            "export": (lambda: full.export(), None, "export"),
            "clear": (table.clear, None, None)}
    base = {"insert spread": lambda: _insert_baseline(spread, conf, voxel), "insert 64 voxels": lambda: _insert_baseline(tight, conf, voxel),
            "depth_points": lambda: _points_baseline(inv, plane, pconf, cam, K, 2, 3), "export": lambda: _export_baseline(full.buf, cap)}
    info = {}
    for name, pts in (("insert spread", spread), ("insert 64 voxels", tight)):
        table.clear()
        st = ops.point_map_status(table.insert(pts, conf))
        uk, n, _, _ = base[name]()
        e = table.export()
        k = int(e["count"].cpu())
        info[name] = {"status": st, "voxels": k, "same_keys_as_torch": bool(k == uk.shape[0] and torch.equal(e["key"][:k], uk)),
                      "same_counts_as_torch": bool(k == uk.shape[0] and torch.equal(e["n"][:k].long(), n))}
    r = ops.depth_points(inv, cam, K, plane=plane, confidence=pconf, median_radius=2, min_support=3)
    bp = base["depth_points"]()
    k = int(r["count"].cpu())
    info["depth_points"] = {"status": ops.depth_points_status(r["status"]), "same_pixels_as_torch": bool(k == bp[2].shape[0] and torch.equal(r["pixel"][:k].long(), bp[2].reshape(-1))),
                            "largest_difference_from_torch": float((r["points"][:k] - bp[0]).abs().max()) if k == bp[0].shape[0] else None}
    for fn, before, _ in legs.values():
        for _ in range(args.warmup):
            timed(fn, before)
    for fn in base.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us, base_us = {k: [] for k in legs}, {k: [] for k in base}
    for rep in range(args.repeats):
        for k, (fn, before, _) in legs.items():
            us[k].append(timed(fn, before))
        if rep < args.baseline_repeats:
            for k in base:
                base_us[k].append(timed(base[k]))
    out = {"points": N, "capacity": cap, "H": H, "W": W, "repeats": args.repeats, "baseline_repeats": args.baseline_repeats, "legs": {}, "info": info}
    for k, v in us.items():
        med = statistics.median(v)
        row = dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1))
        if legs[k][2] is not None:
            bmed = statistics.median(base_us[legs[k][2]])
            row.update(baseline_us_median=round(bmed, 1), baseline_over_kernel=round(bmed / med, 2))
        out["legs"][k] = row
        print("%-18s %10.1f us (min %.1f, max %.1f)%s" % (k, med, min(v), max(v), "" if "baseline_us_median" not in row else
                                                        ";  torch %10.1f us = %.2f x" % (row["baseline_us_median"], row["baseline_over_kernel"])))
    for k, v in info.items():
        print("%-18s %s" % (k, v))
    return out


def tracker_part(args, dev):
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 2, warmup), dev)
    slam, n_ev = t.slam, args.tracker_events
    g = torch.Generator(device="cpu").manual_seed(9)
    ex = (torch.rand(n_ev, generator=g) * (args.width - 1)).to(dev)
    ey = (torch.rand(n_ev, generator=g) * (args.height - 1)).to(dev)
    frac = torch.sort(torch.rand(n_ev, generator=g, dtype=torch.float64)).values.to(dev)      # time-sorted, in the last two frames
    t.prime(args.prime, args.clock_warm)
    slam.event_map(capacity=args.tracker_capacity)
    what = {"a": "no query", "b": "event_map_insert(%d events, %d planes) per frame" % (n_ev, args.tracker_planes)}
    last = {}

    def b():
        last["st"] = slam.event_map_insert(ex, ey, float(t.pos - 3) + 2.0 * frac, planes=args.tracker_planes, as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": b}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "planes": args.tracker_planes, "steps": steps, "repeats": repeats,
           "frames_at_end": t.pos, "voxel": slam.event_map().voxel, "capacity": slam.event_map().capacity}
    out["legs"] = tl.summary(rates, what)
    out["b_over_a"] = tl.ratio(out["legs"], "b", "a")
    out["a_spread"] = tl.spread(out["legs"]["a"])
    out["last_status"] = {k: v.cpu().tolist() for k, v in last["st"].items()}
    out["map_points"] = int(slam.event_map_points(as_tensor=True)["count"].cpu())
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f); last status %s; voxels with two points %d"
          % (out["b_over_a"], out["a_spread"], out["last_status"], out["map_points"]))
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
    assert torch.cuda.is_available(), "event_map_cost.py measures on the GPU; there is nothing to report without one"
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
