"""What live poses cost, and what they replace: three legs over bench.py's flagship workload (BASELINE configs[1]: SingleScale,
640 x 480, 96 patches per frame, default windows, fp16 features, frames pipelined), in ONE process so that they share a box
and a clock state.

  a  no pose stream                       -- the tracker as bench.py times it
  b  pose_stream() + latest_pose() after every call
  c  reading slam.n and poses_[n - 1] after every call: the only way to a per-frame pose without the stream -- one
     hand-back (settle) per frame, every frame host driven

One tracker tracks one stream of frames: primed until the window is full, clock-warmed with untimed steady-state steps as
bench.py does, then the legs run INTERLEAVED, --repeats rounds of a, b, c with --steps frames each (--steps-c for leg c,
which is several times slower), every round synchronised at its start and end.  Printed: kf/s per leg as the median over
the rounds, the lowest and highest round, and every round.  Leg b's pose stream stays allocated once switched on; legs a
and c run with publishing switched off again (slam._pose_ring = None), so a's launches are exactly the ones of a tracker
that never had a stream.

    python tools/pose_stream_cost.py [--steps 200] [--repeats 5] [--json out.json]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--steps-c", type=int, default=24)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--prime", type=int, default=70)
    ap.add_argument("--clock-warm", type=int, default=480)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--patches", type=int, default=96)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from rampvo_amd.config import make_cfg
    from rampvo_amd.Ramp_vo import Ramp_vo
    from rampvo_amd.synthetic import SyntheticStream, make_network
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    slam = Ramp_vo(make_cfg("default", PATCHES_PER_FRAME=args.patches, MIXED_PRECISION=True), make_network("SingleScale", device=dev),
                   {"event_bias": True}, ht=args.height, wd=args.width, device=dev)
    slam.inputs_ready = True
    per_round = 2 * (args.steps + args.warmup) + args.steps_c + args.warmup
    total = args.prime + args.clock_warm + args.repeats * per_round
    stream = SyntheticStream(args.height, args.width, total + 1, seed=1234, device=dev)
    pos = [0]

    frames = [stream.frame(t) for t in range(total)]
    torch.cuda.synchronize()

    def step():                                       # every frame is resident before its call (inputs_ready = True)
        im, ev, K, mask = frames[pos[0]]
        slam(pos[0], input_tensor=(ev, im, mask), intrinsics=K)
        pos[0] += 1

    for _ in range(args.prime):
        step()
    assert slam.is_initialized and slam._dev is not None and slam._dev.active, "the tracker is not device resident"
    gc.collect()
    gc.freeze()
    for _ in range(args.clock_warm):
        step()
    torch.cuda.synchronize()
    ring = None
    rates = {"a": [], "b": [], "c": []}
    seen = {"b_polled": 0, "b_behind": []}

    def leg(name, n):
        nonlocal ring
        slam._pose_ring = ring if name == "b" else None
        if name == "b" and ring is None:
            ring = slam.pose_stream()
        for _ in range(args.warmup):                  # (behind leg c the tracker has to become device resident again)
            step()
        torch.cuda.synchronize()
        settles = slam.stats["settles"]
        tic = time.perf_counter()
        for _ in range(n):
            step()
            if name == "b":
                r = slam.latest_pose()
                seen["b_polled"] += r is not None
                if r is not None:
                    seen["b_behind"].append(pos[0] - 1 - r.frame)
            elif name == "c":
                n_kf = slam.n                         # hands the state back
                _ = slam.poses_[n_kf - 1].cpu()
        torch.cuda.synchronize()
        dt = time.perf_counter() - tic
        rates[name].append(n / dt)
        if name != "c":
            assert slam.stats["settles"] == settles, "leg %s was handed back" % name
        return slam.stats["settles"] - settles

    c_settles = 0
    for _ in range(args.repeats):
        leg("a", args.steps)
        leg("b", args.steps)
        c_settles += leg("c", args.steps_c)
    slam._pose_ring = None
    out = {"workload": "SingleScale %dx%d, %d patches, fp16 features, inputs_ready=True" % (args.width, args.height, args.patches),
           "steps": args.steps, "steps_c": args.steps_c, "repeats": args.repeats, "legs": {}}
    for name, what in (("a", "no pose stream"), ("b", "pose_stream() + latest_pose() per call"),
                       ("c", "slam.n + poses_[n - 1] per call (one hand-back per frame)")):
        v = rates[name]
        out["legs"][name] = {"what": what, "kf_per_s_median": round(statistics.median(v), 1), "min": round(min(v), 1),
                             "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}
        print("leg %s  %-58s %8.1f kf/s  (min %.1f, max %.1f; rounds %s)"
              % (name, what, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))
    a, b = out["legs"]["a"], out["legs"]["b"]
    out["b_over_a"] = round(b["kf_per_s_median"] / a["kf_per_s_median"], 4)
    out["a_spread"] = round((a["max"] - a["min"]) / a["kf_per_s_median"], 4)
    out["c_settles"] = c_settles
    if seen["b_behind"]:
        out["b_frames_behind_median"] = statistics.median(seen["b_behind"])
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f);  leg b's polls saw a record %d frames behind the call "
          "(median);  leg c: %d hand-backs" % (out["b_over_a"], out["a_spread"], out.get("b_frames_behind_median", -1), c_settles))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
