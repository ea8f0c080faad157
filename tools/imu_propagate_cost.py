"""What the IMU propagation costs (ramp_imu_propagate, csrc/imu_propagate.hip).  ONE process, rounds INTERLEAVED over the legs,
so that everything shares a box and a clock state.  No figure here is a target.

  N = 2^20 samples at 1 kHz (smooth rates, fp32), the anchor between the first two samples.  Legs:
    poses            ops.imu_propagate: poses and times
    poses + state    ops.imu_propagate(want_state=True)
    one interval     ops.imu_preintegrate of the one interval [t0, tau[-1]]: ONE wave walks all samples -- the only way to the
                     last row without the scan, here for scale
  Device time between two device events around the call and the host time of the call; median (min - max).  The call's own
  bytes -- the samples read twice (the tile pass and the row pass), the outputs written once -- over the device time, against the
  part's HBM rate; the ratio of each leg to the one-interval walk.

    python tools/imu_propagate_cost.py [--samples N] [--repeats R] [--json out.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from imu_align_cost import HBM_BYTES_PER_S, fmt, scene, timed          # noqa: E402  (the same samples, clock and format)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "imu_propagate_cost.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    from rampvo_amd import ops
    N = args.samples
    tau, gyro, accel, _, _ = scene(N, 2, dev)
    t0 = 0.5 * (float(tau[0]) + float(tau[1]))
    bias = [0.02, -0.01, 0.03]
    anchor = torch.tensor([t0, 0.5, -1.0, 2.0, 0.0, 0.0, 0.0, 1.0, 0.4, 0.1, -0.3, 2.0, 0.3, -0.2, -9.79] + bias + [0.0] * 6,
                          dtype=torch.float64, device=dev)
    ends = torch.tensor([t0, float(tau[-1])], dtype=torch.float64, device=dev)
    legs = {"poses": lambda: ops.imu_propagate(tau, gyro, accel, anchor),
            "poses + state": lambda: ops.imu_propagate(tau, gyro, accel, anchor, want_state=True),
            "one interval": lambda: ops.imu_preintegrate(tau, gyro, accel, ends, bias_g=bias)}
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    us = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, fn in legs.items():
            us[k].append(timed(fn))
    st = ops.imu_propagate_status(ops.imu_propagate(tau, gyro, accel, anchor)["status"])
    read = N * (8 + 12 + 12)
    written = {"poses": N * (28 + 8), "poses + state": N * (28 + 8 + 128), "one interval": 24 * 8}
    walk = statistics.median([d for _, d in us["one interval"]])
    out = {"N": N, "repeats": args.repeats, "status": st, "legs": {}}
    print("N = %d; status %s" % (N, st))
    print("%-16s %30s %30s %12s %14s" % ("leg", "host time of the call, us", "device, us", "of HBM rate", "of one interval"))
    for k, v in us.items():
        host, devt = zip(*v)
        nbytes = (1 if k == "one interval" else 2) * read + written[k]
        med = statistics.median(devt)
        share = nbytes / (med * 1e-6) / HBM_BYTES_PER_S
        out["legs"][k] = {"host_us": round(statistics.median(host), 1), "device_us": round(med, 1), "device_min": round(min(devt), 1),
                          "device_max": round(max(devt), 1), "bytes": nbytes, "hbm_share": round(share, 5),
                          "of_one_interval": round(med / walk, 6)}
        print("%-16s %30s %30s %12.5f %14.6f" % (k, fmt(host), fmt(devt), share, med / walk))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
