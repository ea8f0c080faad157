"""What the localisation against the event map costs on the device: ``ops.time_surface``, one ``PointMap.localize_eval`` and one
``PointMap.localize`` (its 1 + 9 * iters evaluations enqueued whether or not the machine has stopped), as medians of interleaved
rounds timed with HIP events around each call.

    python tools/event_map_localize_cost.py [--capacity 22] [--voxels 250000] [--events 200000] [--rounds 11] [--iters 10]

Prints one JSON line.  The map is a random cloud in front of the camera; the solve's answer is not looked at."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) * 1e3                             # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--capacity", type=int, default=22, help="log2 of the table's slots")
    ap.add_argument("--voxels", type=int, default=250000)
    ap.add_argument("--events", type=int, default=200000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    from rampvo_amd import ops
    rng = np.random.default_rng(0)
    H, W = a.height, a.width
    K = [0.8 * W, 0.8 * W, W / 2 - 0.5, H / 2 - 0.5]
    z = rng.uniform(1.0, 8.0, a.voxels)
    u, v = rng.uniform(0, W - 1, a.voxels), rng.uniform(0, H - 1, a.voxels)
    pts = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1).astype(np.float32)
    m = ops.PointMap(0.01, capacity=1 << a.capacity)
    m.insert(torch.from_numpy(pts).cuda(), view=0)
    cam = torch.tensor([0.01, -0.01, 0.0, 0.0, 0.002, 0.0, 1.0], device="cuda")
    x = torch.from_numpy(rng.uniform(0, W - 1, a.events).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.uniform(0, H - 1, a.events).astype(np.float32)).cuda()
    t = torch.from_numpy(rng.uniform(0.0, 1.0, a.events)).cuda()
    st = torch.cuda.current_stream()
    surface = ops.time_surface(x, y, t, 1.0, 0.1, H, W)["surface"]
    legs = {"time_surface": lambda: ops.time_surface(x, y, t, 1.0, 0.1, H, W),
            "localize_eval": lambda: m.localize_eval(surface, cam, K),
            "localize": lambda: m.localize(surface, cam, K, iters=a.iters)}
    for fn in legs.values():                                   # warm-up: workspaces, code objects
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            times[k].append(timed(fn, st))
    info = ops.point_map_localize_info(m.localize(surface, cam, K, iters=a.iters)["info"])
    print(json.dumps(dict(capacity=1 << a.capacity, voxels=a.voxels, events=a.events, image=[H, W], iters=a.iters, rounds=a.rounds,
                          median_us={k: round(statistics.median(v), 1) for k, v in times.items()},
                          min_us={k: round(min(v), 1) for k, v in times.items()}, reason=info["reason"], n_evals=info["n_evals"])))


if __name__ == "__main__":
    main()
