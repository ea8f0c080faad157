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
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import tracker_legs as tl


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
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    steps = {"a": args.steps, "b": args.steps, "c": args.steps_c}
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, args.repeats, steps.values(), args.warmup), dev)
    slam = t.slam
    t.prime(args.prime, args.clock_warm)
    ring = [None]
    seen = {"b_polled": 0, "b_behind": []}

    def before(name):                                 # legs a and c run with publishing switched off again
        slam._pose_ring = ring[0] if name == "b" else None
        if name == "b" and ring[0] is None:
            ring[0] = slam.pose_stream()

    def b():
        r = slam.latest_pose()
        seen["b_polled"] += r is not None
        if r is not None:
            seen["b_behind"].append(t.pos - 1 - r.frame)

    def c():
        n_kf = slam.n                                 # hands the state back
        _ = slam.poses_[n_kf - 1].cpu()

    # (behind leg c the tracker has to become device resident again: the next leg's warm-up)
    rates, settled = t.run_legs({"a": None, "b": b, "c": c}, steps, args.warmup, args.repeats, before=before, hands_back=("c",))
    slam._pose_ring = None
    out = {"workload": t.workload, "steps": args.steps, "steps_c": args.steps_c, "repeats": args.repeats}
    out["legs"] = tl.summary(rates, {"a": "no pose stream", "b": "pose_stream() + latest_pose() per call",
                                     "c": "slam.n + poses_[n - 1] per call (one hand-back per frame)"})
    out["b_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.spread(out["legs"]["a"])
    c_settles = out["c_settles"] = settled["c"]
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
