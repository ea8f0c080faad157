"""What lens distortion costs: ramp_event_rectify / ramp_image_rectify (csrc/rectify.hip) against torch restatements on the same
device.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  events   N = 2^22 raw events of a 640 x 480 sensor, the fp32 and the int32 path, a radtan and an equidistant camera.  Baseline:
           the same fixed-count Newton written with torch ops (no validity bookkeeping beyond the final mask).  Printed per leg:
           median us, min, max, torch / fused, and the bytes per second of the fused call (8 B in, 8 B out per event).
  image    640 x 480 x 3 uint8 into 640 x 480.  Baseline: ``F.grid_sample`` (bilinear, align_corners) on a PRECOMPUTED grid plus
           the normalisation -- the map is free for the baseline, the kernel recomputes it on every call.
  tracker  pose_query_cost.py's two interleaved legs on BASELINE configs[1]: no query / rectify_events(2 10^5 device-resident raw
           events, as_tensor=True) behind every frame; kf/s per leg, b / a, a's own spread.

    python tools/event_rectify_cost.py [--part kernel|tracker|both] [--events N] [--repeats R] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if path not in sys.path:
        sys.path.insert(0, path)

RADTAN = dict(model="radtan", raw_intrinsics=(766.0, 768.0, 319.0, 233.0), coeffs=(-0.29, 0.11, -5e-4, 3e-4, -0.02))
EQUI = dict(model="equidistant", raw_intrinsics=(560.0, 561.0, 322.0, 236.0), coeffs=(-0.035, 0.012, -0.006, 0.0012))
ITERS = 8


def _torch_rectify(x, y, cam):
    """the kernel's inversion with torch ops: ITERS Newton steps, then the projection with the raw intrinsics"""
    fx, fy, cx, cy = cam["raw_intrinsics"]
    k = list(cam["coeffs"]) + [0.0]
    xd, yd = (x.float() - cx) / fx, (y.float() - cy) / fy
    if cam["model"] == "radtan":
        k1, k2, p1, p2, k3 = k[:5]
        u, v = xd.clone(), yd.clone()
        for _ in range(ITERS):
            uu, vv, uv = u * u, v * v, u * v
            r2 = uu + vv
            rad = 1 + r2 * (k1 + r2 * (k2 + r2 * k3))
            drad = k1 + r2 * (2 * k2 + r2 * 3 * k3)
            ex = u * rad + 2 * p1 * uv + p2 * (r2 + 2 * uu) - xd
            ey = v * rad + p1 * (r2 + 2 * vv) + 2 * p2 * uv - yd
            J11 = rad + 2 * uu * drad + 2 * p1 * v + 6 * p2 * u
            J12 = 2 * uv * drad + 2 * p1 * u + 2 * p2 * v
            J22 = rad + 2 * vv * drad + 6 * p1 * v + 2 * p2 * u
            det = J11 * J22 - J12 * J12
            u, v = u - (J22 * ex - J12 * ey) / det, v - (J11 * ey - J12 * ex) / det
    else:
        thd = torch.sqrt(xd * xd + yd * yd)
        th = thd.clone()
        for _ in range(ITERS):
            t2 = th * th
            f = th * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
            df = 1 + t2 * (3 * k[0] + t2 * (5 * k[1] + t2 * (7 * k[2] + t2 * 9 * k[3])))
            th = th - (f - thd) / df
        s = torch.where(thd > 0, torch.tan(th) / thd, torch.ones_like(thd))
        u, v = s * xd, s * yd
    return torch.stack([fx * u + cx, fy * v + cy], -1)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                      # us


def kernel_part(args, dev):
    import torch.nn.functional as F
    from rampvo_amd import ops
    N, H, W = args.events, args.height, args.width
    g = torch.Generator(device="cpu").manual_seed(8)
    xi = torch.randint(0, W, (N,), generator=g, dtype=torch.int32).to(dev)
    yi = torch.randint(0, H, (N,), generator=g, dtype=torch.int32).to(dev)
    xf, yf = xi.float() + 0.25, yi.float() + 0.25
    legs, bases, nbytes = {}, {}, {}
    for cname, cam in (("radtan", RADTAN), ("equidistant", EQUI)):
        rec = ops.camera(device=dev, **cam)
        for pname, (x, y, b_in) in (("fp32", (xf, yf, 8)), ("int32", (xi, yi, 8))):
            key = "events %-11s %-5s" % (cname, pname)
            legs[key] = (lambda x=x, y=y, rec=rec: ops.event_rectify(x, y, rec, H, W)["xy"])
            bases[key] = (lambda x=x, y=y, cam=cam: _torch_rectify(x, y, cam))
            nbytes[key] = N * (b_in + 8)
    img = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev)
    for cname, cam in (("radtan", RADTAN), ("equidistant", EQUI)):
        rec = ops.camera(device=dev, **cam)
        m = ops.image_rectify(img, rec, H, W, want_map=True)["map"]
        grid = torch.stack([2 * m[..., 0] / (W - 1) - 1, 2 * m[..., 1] / (H - 1) - 1], -1)[None]      # precomputed once
        key = "image  %-11s u8x3 " % cname
        legs[key] = (lambda rec=rec: ops.image_rectify(img, rec, H, W, normalize="half")["image"])
        bases[key] = (lambda grid=grid: 2 * (F.grid_sample(img[None].float(), grid, mode="bilinear", padding_mode="zeros",
                                                           align_corners=True)[0] / 255.0) - 0.5)
        nbytes[key] = 3 * H * W * (1 + 4)
    keys = list(legs)
    agree = {}
    for k in keys:                                      # (also the first warm-up round)
        a, b = legs[k](), bases[k]()
        ok = torch.isfinite(a) & torch.isfinite(b)
        agree[k] = float((a - b)[ok].abs().max())
    for fn in list(legs.values()) + list(bases.values()):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us, base_us = {k: [] for k in keys}, {k: [] for k in keys}
    for r in range(args.repeats):
        for k in keys:
            us[k].append(timed(legs[k]))
            if r < args.baseline_repeats:
                base_us[k].append(timed(bases[k]))
    out = {"N": N, "H": H, "W": W, "repeats": args.repeats, "baseline_repeats": args.baseline_repeats,
           "device": torch.cuda.get_device_name(dev), "legs": {}}
    for k in keys:
        med, bmed = statistics.median(us[k]), statistics.median(base_us[k])
        out["legs"][" ".join(k.split())] = {
            "us_median": round(med, 1), "us_min": round(min(us[k]), 1), "us_max": round(max(us[k]), 1),
            "torch_us_median": round(bmed, 1), "torch_us_min": round(min(base_us[k]), 1), "torch_us_max": round(max(base_us[k]), 1),
            "torch_over_fused": round(bmed / med, 2), "GBps": round(nbytes[k] / med / 1e3, 1), "largest_difference": agree[k]}
        print("%s %9.1f us (min %.1f, max %.1f)   torch %10.1f us (min %.1f, max %.1f) = %6.2f x   %7.1f GB/s   difference %.1e"
              % (k, med, min(us[k]), max(us[k]), bmed, min(base_us[k]), max(base_us[k]), bmed / med, nbytes[k] / med / 1e3, agree[k]))
    return out


def tracker_part(args, dev):
    import tracker_legs as tl
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 2, warmup), dev)
    n_ev = args.tracker_events
    g = torch.Generator(device="cpu").manual_seed(9)
    ex = torch.randint(0, args.width, (n_ev,), generator=g, dtype=torch.int32).to(dev)
    ey = torch.randint(0, args.height, (n_ev,), generator=g, dtype=torch.int32).to(dev)
    t.slam.set_camera(**RADTAN)
    t.prime(args.prime, args.clock_warm)
    last = [None]

    def query():
        last[0] = t.slam.rectify_events(ex, ey, as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": query}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "steps": steps, "repeats": repeats, "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "rectify_events(%d events) per frame" % n_ev})
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
    assert torch.cuda.is_available(), "event_rectify_cost.py measures on the GPU; there is nothing to report without one"
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
