"""What Ramp_vo.uncertainty() costs: two legs over bench.py's flagship workload (BASELINE configs[1]: SingleScale, 640 x 480, 96
patches per frame, default windows, fp16 features, frames pipelined), in ONE process so that they share a box and a clock
state.

  a  no query                         -- the tracker as bench.py times it
  b  slam.uncertainty() after every call (one C call behind the frame, then the host waits for its 32 bytes of stats)

One tracker tracks one stream of frames: primed until the window is full, clock-warmed with untimed steady-state steps as
bench.py does, then the legs run INTERLEAVED, --repeats rounds of a, b with --steps frames each, every round synchronised at
its start and end.  Printed: kf/s per leg as the median over the rounds, the lowest and highest round, every round; the
tracker must stay device resident throughout (no hand-back in either leg).

    python tools/uncertainty_cost.py [--steps 200] [--repeats 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tracker_legs as tl


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
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, args.repeats, [args.steps] * 2, args.warmup), dev)
    t.prime(args.prime, args.clock_warm)
    last = [None]

    def query():
        last[0] = t.slam.uncertainty()

    rates, _ = t.run_legs({"a": None, "b": query}, args.steps, args.warmup, args.repeats)
    out = {"workload": t.workload, "steps": args.steps, "repeats": args.repeats}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "uncertainty() per call"})
    out["b_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.spread(out["legs"]["a"])
    u = last[0]
    out["last_query"] = {"N": len(u["frames"]), "n_valid": u["n_valid"], "dof": u["dof"], "sigma0_sq": u["sigma0_sq"]}
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f)" % (out["b_over_a"], out["a_spread"]))
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    with torch.no_grad():
        main()
