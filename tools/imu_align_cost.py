"""What the IMU alignment costs (ramp_imu_preintegrate / ramp_imu_align, csrc/imu.hip).  ONE process, rounds INTERLEAVED over
the legs, so that everything shares a box and a clock state.  No figure here is a target.

  kernel   N = 2^20 samples at 1 kHz (smooth rates, fp32), T = 2000 identity-free knots over the same span, stride 1 and 10.  Legs:
    preintegrate     ops.imu_preintegrate alone
    align            ops.imu_align, gyro_steps = 1, a gravity norm: two integrations, two reductions, the velocities
    one interval     ops.imu_preintegrate over two time stamps that hold all samples: ONE wave walks 2^20 sub-intervals
           Device time between two device events around the call and the host time of the call; median (min - max).  The
           bytes the integration must read (tau, gyro, accel once) over the device time, against the part's HBM rate.

  tracker  tools/tracker_legs.py on BASELINE configs[1]: no query / align_imu(as_tensor=True) over the samples of the last
           frames behind every frame; kf/s per leg, the ratio, its own spread.

    python tools/imu_align_cost.py [--part kernel|tracker|both] [--samples N] [--knots T] [--repeats R] [--json out.json]
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

HBM_BYTES_PER_S = 8.0e12          # MI355X: 8 TB/s peak


def scene(N, T, dev):
    """smooth body rates and specific forces at 1 kHz; knots on a Lissajous curve with slowly turning rotations"""
    tau = torch.arange(N, dtype=torch.float64) / 1000.0
    t = tau[:, None]
    gyro = (0.4 * torch.sin(t * torch.tensor([0.7, 1.1, 0.5], dtype=torch.float64))).float()
    accel = (torch.tensor([0.0, 0.0, 9.8], dtype=torch.float64) + torch.sin(t * torch.tensor([1.3, 0.9, 0.4], dtype=torch.float64))).float()
    times = torch.linspace(float(tau[1]), float(tau[-2]), T, dtype=torch.float64)
    k = times[:, None]
    pos = torch.cat([torch.sin(0.9 * k), torch.cos(0.7 * k), 0.5 * torch.sin(1.3 * k)], 1)
    half = 0.25 * torch.sin(0.5 * k)
    quat = torch.cat([torch.zeros(T, 2, dtype=torch.float64), torch.sin(half), torch.cos(half)], 1)
    knots = torch.cat([pos, quat], 1).float()
    return tau.to(dev), gyro.to(dev), accel.to(dev), knots.to(dev), times.to(dev)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    fn()
    t1 = time.perf_counter()
    b.record()
    b.synchronize()
    return (t1 - t0) * 1e6, a.elapsed_time(b) * 1e3          # us: the call on the host, the device


def fmt(v):
    return "%10.1f (%.1f - %.1f)" % (statistics.median(v), min(v), max(v))


def kernel_part(args, dev):
    from rampvo_amd import ops
    tau, gyro, accel, knots, times = scene(args.samples, args.knots, dev)
    ends = times[[0, -1]].contiguous()
    legs = {}
    for stride in (1, 10):
        legs["preintegrate, stride %d" % stride] = lambda s=stride: ops.imu_preintegrate(tau, gyro, accel, times, stride=s)
        legs["align, stride %d" % stride] = lambda s=stride: ops.imu_align(tau, gyro, accel, knots, times, stride=s, gravity_norm=9.8)
    legs["one interval"] = lambda: ops.imu_preintegrate(tau, gyro, accel, ends)
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
    st = ops.imu_status(ops.imu_align(tau, gyro, accel, knots, times, gravity_norm=9.8)["status"])
    read = args.samples * (8 + 12 + 12)
    out = {"N": args.samples, "T": args.knots, "repeats": args.repeats, "status": st, "bytes_read_once": read, "legs": {}}
    print("N = %d, T = %d; status %s" % (args.samples, args.knots, st))
    print("%-26s %30s %30s %12s" % ("leg", "host time of the call, us", "device, us", "of HBM rate"))
    for k, v in us.items():
        host, devt = zip(*v)
        passes = 2 if k.startswith("align") else 1
        share = passes * read / (statistics.median(devt) * 1e-6) / HBM_BYTES_PER_S
        out["legs"][k] = {"host_us": round(statistics.median(host), 1), "device_us": round(statistics.median(devt), 1),
                          "device_min": round(min(devt), 1), "device_max": round(max(devt), 1), "hbm_share": round(share, 5)}
        print("%-26s %30s %30s %12.5f" % (k, fmt(host), fmt(devt), share))
    return out


def tracker_part(args, dev):
    import tracker_legs as tl
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width, tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 2, warmup), dev)
    per, span = 100, 8                                     # samples per frame interval; frames of samples behind every frame
    n = per * span
    g = torch.Generator(device="cpu").manual_seed(9)
    gyro = (0.2 * torch.randn(n, 3, generator=g)).to(dev)
    accel = (torch.randn(n, 3, generator=g) + torch.tensor([0.0, 0.0, 9.8])).to(dev)
    frac = (torch.arange(n, dtype=torch.float64) / per).to(dev)
    t.prime(args.prime, args.clock_warm)
    t.slam.set_imu()
    last = [None]

    def query():
        last[0] = t.slam.align_imu(float(t.pos - 1 - span) + 0.5 + frac, gyro, accel, as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": query}, steps, warmup, repeats)
    out = {"workload": t.workload, "samples_per_query": n, "steps": steps, "repeats": repeats, "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "align_imu(as_tensor=True), %d samples, per frame" % n})
    out["b_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.spread(out["legs"]["a"])
    from rampvo_amd import ops
    out["last_status"] = ops.imu_status(last[0]["status"])
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f); last call: %s" % (out["b_over_a"], out["a_spread"], out["last_status"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "tracker", "both"), default="both")
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--knots", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--json", default=None)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tracker-repeats", type=int, default=5)
    ap.add_argument("--tracker-warmup", type=int, default=20)
    ap.add_argument("--prime", type=int, default=70)
    ap.add_argument("--clock-warm", type=int, default=480)
    ap.add_argument("--patches", type=int, default=96)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "imu_align_cost.py measures on the GPU; there is nothing to report without one"
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
