"""What aligning the events costs: the host loop of ops.event_align beside the device loop (ramp_event_align, csrc/contrast.hip).
ONE process, rounds INTERLEAVED over the legs, so that everything shares a box and a clock state.  Nothing here fixes a ratio:
the yardstick is the host loop, and if the resident form loses on wall time at some size the table says so.

  kernel   dots under a constant rotation rate (the recipe of tests/contrastref.py align_scene(), scaled to 640 x 480), T = 2000
           identity knots, N = 2^18 and 2^22, the default call (rotation free, step 0.05, 20 accepted steps).  Legs:
    host            ops.event_align(resident=False): one synchronisation per evaluation; wall time
    resident full   resident=True, max_evals = 1 + 9 * iters: the evaluations behind the end of the search are empty launches
    resident exact  resident=True, max_evals = the evaluations the host loop needed
           For the resident legs: the host time of the call (its enqueue), the device time between two device events around
           it, and the wall time up to the result.  Median (min - max) over the rounds.

  tracker  tools/tracker_legs.py on BASELINE configs[1]: no query / align_events(resident=True, as_tensor=True, iters=5) /
           align_events(iters=5) in its host form, of 2 10^5 device-resident events of the last two frames behind every frame;
           kf/s per leg, ratios to the first, its own spread.

    python tools/event_align_cost.py [--part kernel|tracker|both] [--events N [N ...]] [--repeats R] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tracker_legs as tl

RATE = (0.15, -0.10, 0.30)


def dot_scene(N, T, H, W, dev, dots=4000):
    """events of sharp dots seen under the rotation rate RATE about t_ref = 0 (to first order: P = P0 - tau RATE x P0)"""
    g = torch.Generator(device="cpu").manual_seed(5)
    K = torch.tensor([0.5 * W, 0.5 * W, 0.5 * (W - 1), 0.5 * (H - 1)], dtype=torch.float64)
    u0 = 6 + torch.rand(dots, generator=g, dtype=torch.float64) * (W - 13)
    v0 = 6 + torch.rand(dots, generator=g, dtype=torch.float64) * (H - 13)
    pol = torch.randint(0, 2, (dots,), generator=g) * 2 - 1
    k = torch.randint(0, dots, (N,), generator=g)
    tau = torch.sort(torch.rand(N, generator=g, dtype=torch.float64) - 0.5).values
    P0 = torch.stack([(u0[k] - K[2]) / K[0], (v0[k] - K[3]) / K[1], torch.ones(N, dtype=torch.float64)], -1)
    w = torch.tensor(RATE, dtype=torch.float64).expand(N, 3)
    P = P0 - tau[:, None] * torch.linalg.cross(w, P0)
    x, y = K[0] * P[:, 0] / P[:, 2] + K[2], K[1] * P[:, 1] / P[:, 2] + K[3]
    knots = torch.zeros(T, 7)
    knots[:, 6] = 1.0
    times = torch.linspace(-1.0, 1.0, T, dtype=torch.float64)
    return (x.float().to(dev), y.float().to(dev), tau.to(dev), pol[k].to(torch.int8).to(dev), knots.to(dev), times.to(dev), 0.0,
            K.float().to(dev), 0.0, H, W)


def fmt(v):
    return "%10.1f (%.1f - %.1f)" % (statistics.median(v), min(v), max(v))


def kernel_part(args, dev):
    from rampvo_amd import ops
    out = []
    for N in args.events:
        scene = dot_scene(N, args.knots, args.height, args.width, dev)
        full = ops.event_align(*scene, resident=True)
        info = ops.event_align_info(full["info"])
        host = ops.event_align(*scene)
        same = host["correction"] == full["correction"].cpu().tolist() and host["variance"] == float(full["variance"])
        need = info["n_evals"]
        legs = {"host": lambda: ops.event_align(*scene), "resident full": lambda: ops.event_align(*scene, resident=True),
                "resident exact": lambda: ops.event_align(*scene, resident=True, max_evals=need)}

        def timed(fn):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            t1 = time.perf_counter()
            b.record()
            b.synchronize()
            t2 = time.perf_counter()
            return (t1 - t0) * 1e6, a.elapsed_time(b) * 1e3, (t2 - t0) * 1e6          # us: the call on the host, device, wall

        for fn in legs.values():
            for _ in range(args.warmup):
                fn()
        us = {k: [] for k in legs}
        for _ in range(args.repeats):
            for k, fn in legs.items():
                us[k].append(timed(fn))
        row = {"N": N, "T": args.knots, "H": args.height, "W": args.width, "repeats": args.repeats, "evaluations": need,
               "accepted": info["n_accepted"], "reason": info["reason"], "budget_full": 1 + 9 * 20,
               "variance0": float(full["variance0"]), "variance": float(full["variance"]), "host_loop_same_bits": same, "legs": {}}
        print("N = %d: %d evaluations, %d accepted (%s), variance %.6g -> %.6g; the host loop's bits: %s"
              % (N, need, info["n_accepted"], info["reason"], row["variance0"], row["variance"], same))
        print("%-15s %30s %30s %30s" % ("leg", "host time of the call, us", "device, us", "wall, us"))
        for k, v in us.items():
            cols = list(zip(*v))
            row["legs"][k] = {name: {"median": round(statistics.median(c), 1), "min": round(min(c), 1), "max": round(max(c), 1)}
                              for name, c in zip(("host_us", "device_us", "wall_us"), cols)}
            print("%-15s %30s %30s %30s" % (k, fmt(cols[0]), fmt(cols[1]), fmt(cols[2])))
        out.append(row)
    return out


def tracker_part(args, dev):
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 3, warmup), dev)
    n_ev = args.tracker_events
    g = torch.Generator(device="cpu").manual_seed(9)
    ex = (torch.rand(n_ev, generator=g) * (args.width - 1)).to(dev)
    ey = (torch.rand(n_ev, generator=g) * (args.height - 1)).to(dev)
    ep = (torch.randint(0, 2, (n_ev,), generator=g) * 2 - 1).to(torch.int8).to(dev)
    frac = torch.sort(torch.rand(n_ev, generator=g, dtype=torch.float64)).values.to(dev)      # time-sorted, in the last two frames
    t.prime(args.prime, args.clock_warm)
    last = [None, None]

    def resident():
        last[0] = t.slam.align_events(ex, ey, float(t.pos - 3) + 2.0 * frac, ep, iters=5, as_tensor=True)

    def host():
        last[1] = t.slam.align_events(ex, ey, float(t.pos - 3) + 2.0 * frac, ep, iters=5)

    rates, _ = t.run_legs({"a": None, "b": resident, "c": host}, steps, warmup, repeats)
    out = {"workload": t.workload, "events_per_frame": n_ev, "steps": steps, "repeats": repeats, "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "align_events(resident=True, iters=5, %d events) per frame" % n_ev,
                                     "c": "align_events(iters=5), the host loop, per frame"})
    out["b_over_a"], out["c_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.ratio(out["legs"], "c", "a"), tl.spread(out["legs"]["a"])
    from rampvo_amd import ops
    out["last_info"] = ops.event_align_info(last[0]["info"])
    print("b / a = %.4f, c / a = %.4f   (a's own spread, (max - min) / median: %.4f); last resident call: %s"
          % (out["b_over_a"], out["c_over_a"], out["a_spread"], out["last_info"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "tracker", "both"), default="both")
    ap.add_argument("--events", type=int, nargs="+", default=[1 << 18, 1 << 22])
    ap.add_argument("--knots", type=int, default=2000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--warmup", type=int, default=2)
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
    assert torch.cuda.is_available(), "event_align_cost.py measures on the GPU; there is nothing to report without one"
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
