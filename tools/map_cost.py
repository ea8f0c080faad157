"""What Ramp_vo.map() costs beside Ramp_vo.uncertainty(): three legs over bench.py's flagship workload (BASELINE configs[1]: SingleScale, 640 x 480, 96
patches per frame, default windows, fp16 features, frames pipelined), in ONE process so that they share a box and a clock
state.

  a  no query                         -- the tracker as bench.py times it
  b  slam.uncertainty() after every call (one C call behind the frame, then the host waits for its 32 bytes of stats)
  c  slam.map() after every call (the same call with the map stage, the selection, then the host waits for the stats and
     the count and gathers the K selected points)

One tracker tracks one stream of frames: primed until the window is full, clock-warmed with untimed steady-state steps as
bench.py does, then the legs run INTERLEAVED, --repeats rounds of a, b, c with --steps frames each, every round synchronised at
its start and end.  Printed: kf/s per leg as the median over the rounds, the lowest and highest round, every round; the
tracker must stay device resident throughout (no hand-back in any leg).

    python tools/map_cost.py [--steps 200] [--repeats 5] [--json out.json]
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
    total = args.prime + args.clock_warm + args.repeats * 3 * (args.steps + args.warmup)
    stream = SyntheticStream(args.height, args.width, total + 1, seed=1234, device=dev)
    pos = [0]
    frames = [stream.frame(t) for t in range(total)]
    torch.cuda.synchronize()

    def step():
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
    rates = {"a": [], "b": [], "c": []}
    last = [None, None]

    def leg(name, n):
        for _ in range(args.warmup):
            step()
        torch.cuda.synchronize()
        settles = slam.stats["settles"]
        tic = time.perf_counter()
        for _ in range(n):
            step()
            if name == "b":
                last[0] = slam.uncertainty()
            elif name == "c":
                last[1] = slam.map()
        torch.cuda.synchronize()
        rates[name].append(n / (time.perf_counter() - tic))
        assert slam.stats["settles"] == settles and slam._dev.active, "leg %s was handed back" % name

    for _ in range(args.repeats):
        leg("a", args.steps)
        leg("b", args.steps)
        leg("c", args.steps)
    out = {"workload": "SingleScale %dx%d, %d patches, fp16 features, inputs_ready=True" % (args.width, args.height, args.patches),
           "steps": args.steps, "repeats": args.repeats, "legs": {}}
    for name, what in (("a", "no query"), ("b", "uncertainty() per call"), ("c", "map() per call")):
        v = rates[name]
        out["legs"][name] = {"what": what, "kf_per_s_median": round(statistics.median(v), 1), "min": round(min(v), 1),
                             "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}
        print("leg %s  %-28s %8.1f kf/s  (min %.1f, max %.1f; rounds %s)"
              % (name, what, statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))
    a, b, c = out["legs"]["a"], out["legs"]["b"], out["legs"]["c"]
    out["b_over_a"] = round(b["kf_per_s_median"] / a["kf_per_s_median"], 4)
    out["c_over_a"] = round(c["kf_per_s_median"] / a["kf_per_s_median"], 4)
    out["c_over_b"] = round(c["kf_per_s_median"] / b["kf_per_s_median"], 4)
    out["a_spread"] = round((a["max"] - a["min"]) / a["kf_per_s_median"], 4)
    u = last[0]
    out["last_query"] = {"N": len(u["frames"]), "n_valid": u["n_valid"], "dof": u["dof"], "sigma0_sq": u["sigma0_sq"]}
    m = last[1]
    out["last_map"] = {"K": int(m["index"].numel()), "n_total": m["n_total"], "sigma0_sq": m["sigma0_sq"],
                       "median_sigma": float(m["point_cov"].diagonal(dim1=1, dim2=2).sum(1).sqrt().median()) if m["index"].numel() else None}
    print("b / a = %.4f   c / a = %.4f   c / b = %.4f   (a's own spread, (max - min) / median: %.4f)"
          % (out["b_over_a"], out["c_over_a"], out["c_over_b"], out["a_spread"]))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
