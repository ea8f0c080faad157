"""What the event plane sweep costs: ramp_event_dsi (csrc/emvs.hip) against a torch restatement on the same device, and behind
the tracker.  ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.

  kernel   N = 2^20 events uniform over 640 x 480, T = 2000 knots on a smooth walk, time-sorted events over the knots' range,
           D = 32 and 128 planes.  Legs per D (device events around the whole call: memset + four launches):
             detect    min_votes = 4, adaptive_radius = 0
             adaptive  min_votes = 4, adaptive_radius = 5, adaptive_offset = 1
             memset    the D x H x W x 8 bytes of the DSI cleared by torch: what the call's one memset costs
           The entry always runs its four launches, so the vote alone is not a leg of this tool: it is the vote launch's
           row of a kernel trace of the same command (rocprofv3 --kernel-trace --stats -- python tools/event_dsi_cost.py ...).
           Printed per leg: median us, min, max, votes (events x planes) per second, the memset's share (D x H x W x 8 bytes).
           baseline: ops.se3_interp at the events' times, the warp geometry broadcast over the planes in chunks of events,
           index_put_(accumulate=True) of the four fixed-point weights into an int64 DSI, max over the planes; the ratio is
           quoted against THIS.  It is checked against the kernel once (the DSI's sums agree to rounding of the coordinates:
           the share of cells that differ is printed, not asserted).
  tracker  BASELINE configs[1] (SingleScale 640 x 480, 96 patches, fp16 features): a / b = no query / event_depth of 2 10^5
           device-resident events of the last two frames behind every frame; kf/s per leg, b / a, a's own spread.

    timeout -k 10 600 python tools/event_dsi_cost.py --part kernel --json runs/event_dsi_kernel.json && \\
    timeout -k 10 900 python tools/event_dsi_cost.py --part tracker --json runs/event_dsi_tracker.json
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

FIX = float(1 << 24)


def _walk(T, dev):
    """T camera-to-world knots on a smooth walk (small constant twist with a slow wobble), times 0 .. T - 1"""
    from rampvo_amd import ops
    g = torch.Generator(device="cpu").manual_seed(4)
    xi = (torch.tensor([2e-4, 1e-4, 1.5e-4, 1e-4, 2e-4, 1e-4]) * (1.0 + 0.3 * torch.randn(T, 6, generator=g))).to(dev)
    X = torch.zeros((T, 7), device=dev)
    X[:, 6] = 1.0
    inc = ops.se3_unary("ramp_se3_exp", xi, 6, 7)
    for k in range(1, T):                              # (once, outside every timed region)
        X[k] = ops.se3_binary("ramp_se3_mul", inc[k:k + 1], X[k - 1:k], 7, 7, 7)[0]
    return X.contiguous(), torch.arange(T, dtype=torch.float64, device=dev)


def _qrot(q, v):
    uv = 2.0 * torch.cross(q[..., :3], v, dim=-1)
    return v + q[..., 3:4] * uv + torch.cross(q[..., :3], uv, dim=-1)


def _qmul(a, b):
    return torch.cat([a[..., 3:] * b[..., :3] + b[..., 3:] * a[..., :3] + torch.cross(a[..., :3], b[..., :3], dim=-1),
                      a[..., 3:] * b[..., 3:] - (a[..., :3] * b[..., :3]).sum(-1, keepdim=True)], -1)


def _baseline(x, y, t, knots, times, t_ref, K, rng, D, H, W, chunk=1 << 16):
    """the same sweep in torch: poses per event by ops.se3_interp, planes by broadcasting, votes by index_put_"""
    from rampvo_amd import ops
    dev = x.device
    C, _, _ = ops.se3_interp(knots, times, t)
    Cr, _, _ = ops.se3_interp(knots, times, torch.tensor([t_ref], dtype=torch.float64, device=dev))
    qi = Cr[:, 3:] * torch.tensor([-1.0, -1.0, -1.0, 1.0], device=dev)
    fx, fy, cx, cy = (float(v) for v in K)
    d = (rng[0] + (rng[1] - rng[0]) * torch.arange(D, dtype=torch.float64, device=dev) / max(D - 1, 1)).float()
    dsi = torch.zeros(D * H * W, dtype=torch.int64, device=dev)
    plane = (torch.arange(D, device=dev) * (H * W))[None, :]
    for i in range(0, x.shape[0], chunk):
        xs, ys, Cs = x[i:i + chunk], y[i:i + chunk], C[i:i + chunk]
        n = xs.shape[0]
        q = _qmul(qi.expand(n, 4), Cs[:, 3:])
        tG = _qrot(qi.expand(n, 4), Cs[:, :3] - Cr[:, :3])
        R = _qrot(q, torch.stack([(xs - cx) / fx, (ys - cy) / fy, torch.ones_like(xs)], -1))
        Xp = R[:, None, :] + tG[:, None, :] * d[None, :, None]                       # [n, D, 3]
        Z = Xp[..., 2]
        xp, yp = fx * (Xp[..., 0] / Z) + cx, fy * (Xp[..., 1] / Z) + cy
        ok = (Z > 0.2) & torch.isfinite(xp) & torch.isfinite(yp)
        fxl, fyl = torch.floor(xp), torch.floor(yp)
        wx, wy = xp - fxl, yp - fyl
        for jy in (0, 1):
            for jx in (0, 1):
                px, py = fxl + jx, fyl + jy
                m = ok & (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)
                w = torch.round(((wx if jx else 1.0 - wx) * (wy if jy else 1.0 - wy)) * FIX).to(torch.int64)
                at = (plane + (py.clamp(0, H - 1).long() * W + px.clamp(0, W - 1).long()))[m]
                dsi.index_put_((at,), w[m], accumulate=True)
    dsi = dsi.view(D, H, W)
    best, arg = dsi.max(0)
    return dsi, best, arg


def kernel_part(args, dev):
    from rampvo_amd import ops
    H, W, N, T = args.height, args.width, args.events, args.knots
    g = torch.Generator(device="cpu").manual_seed(8)
    x = (torch.rand(N, generator=g) * (W - 1)).to(dev)
    y = (torch.rand(N, generator=g) * (H - 1)).to(dev)
    t = (torch.sort(torch.rand(N, generator=g, dtype=torch.float64)).values * (T - 1)).to(dev)
    knots, times = _walk(T, dev)
    K = torch.tensor([320.0, 320.0, 319.5, 239.5], device=dev)
    rng, t_ref = (0.1, 2.0), 0.5 * (T - 1)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    legs, base, info = {}, {}, {}
    for D in args.planes:
        call = lambda D=D, **kw: ops.event_dsi(x, y, t, knots, times, t_ref, K, H, W, planes=D, range=rng, **kw)
        scratch = torch.empty((D, H, W), dtype=torch.int64, device=dev)
        legs["D=%d memset" % D] = lambda scratch=scratch: scratch.zero_()
        legs["D=%d detect" % D] = lambda call=call: call(min_votes=4.0)
        legs["D=%d adaptive" % D] = lambda call=call: call(min_votes=4.0, adaptive_radius=5, adaptive_offset=1.0)
        base["D=%d" % D] = lambda D=D: _baseline(x, y, t, knots, times, t_ref, K.cpu().tolist(), rng, D, H, W)
        first, again = call(min_votes=4.0), call(min_votes=4.0)
        ref_dsi, _, ref_arg = base["D=%d" % D]()
        st = ops.event_dsi_status(first["status"])
        info["D=%d" % D] = {"status": st, "same_bits_twice": torch.equal(first["dsi"], again["dsi"]),
                            "cells_differing_from_torch": float((first["dsi"] != ref_dsi).float().mean()),
                            "votes_sum_rel_difference": float((first["dsi"].sum() - ref_dsi.sum()).abs().double() / ref_dsi.sum().double())}
        del first, again, ref_dsi, ref_arg
    for fn in list(legs.values()) + list(base.values()):
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    us, base_us = {k: [] for k in legs}, {k: [] for k in base}
    for r in range(args.repeats):
        for k in legs:
            us[k].append(timed(legs[k]))
        if r < args.baseline_repeats:
            for k in base:
                base_us[k].append(timed(base[k]))
    out = {"N": N, "T": T, "H": H, "W": W, "repeats": args.repeats, "legs": {}, "info": info}
    for k, v in us.items():
        D = int(k.split()[0][2:])
        med, bmed = statistics.median(v), statistics.median(base_us["D=%d" % D])
        out["legs"][k] = dict(us_median=round(med, 1), us_min=round(min(v), 1), us_max=round(max(v), 1),
                              Gvotes_per_s=round(N * D / med / 1e3, 2), dsi_bytes=D * H * W * 8,
                              baseline_us_median=round(bmed, 1), baseline_over_kernel=round(bmed / med, 2))
        print("%-16s %10.1f us (min %.1f, max %.1f)  %.2f Gvote/s, DSI %.0f MB;  torch %10.1f us = %.2f x"
              % (k, med, min(v), max(v), out["legs"][k]["Gvotes_per_s"], D * H * W * 8 / 1e6, bmed, bmed / med))
    for k, v in info.items():
        print("%-8s %s; same bits twice: %s; cells differing from torch %.2e, sum of votes rel. %.1e"
              % (k, v["status"], v["same_bits_twice"], v["cells_differing_from_torch"], v["votes_sum_rel_difference"]))
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
    what = {"a": "no query", "b": "event_depth(%d events, %d planes) per frame" % (n_ev, args.tracker_planes)}
    last = {}

    def b():
        last["depth"] = slam.event_depth(ex, ey, float(t.pos - 3) + 2.0 * frac, planes=args.tracker_planes, as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": b}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "planes": args.tracker_planes, "steps": steps, "repeats": repeats,
           "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, what)
    out["b_over_a"] = tl.ratio(out["legs"], "b", "a")
    out["a_spread"] = tl.spread(out["legs"]["a"])
    out["last_status"] = last["depth"]["status"].cpu().tolist()
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f); last status %s" % (out["b_over_a"], out["a_spread"], out["last_status"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "tracker", "both"), default="kernel")
    ap.add_argument("--events", type=int, default=1 << 20)
    ap.add_argument("--knots", type=int, default=2000)
    ap.add_argument("--planes", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--baseline-repeats", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tracker-repeats", type=int, default=5)
    ap.add_argument("--tracker-warmup", type=int, default=20)
    ap.add_argument("--tracker-events", type=int, default=200000)
    ap.add_argument("--tracker-planes", type=int, default=64)
    ap.add_argument("--prime", type=int, default=70)
    ap.add_argument("--clock-warm", type=int, default=480)
    ap.add_argument("--patches", type=int, default=96)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "event_dsi_cost.py measures on the GPU; there is nothing to report without one"
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
