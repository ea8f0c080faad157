"""The harness the query cost tools share (pose_stream_cost.py, uncertainty_cost.py, map_cost.py, pose_query_cost.py,
event_warp_cost.py, depth_map_cost.py): ONE tracker on bench.py's flagship workload (BASELINE configs[1]: SingleScale, fp16
features, frames pipelined) tracks ONE stream of frames held on the device; it is primed until the window is full and the
steady state device resident, clock-warmed with untimed steps as bench.py does, then the legs run INTERLEAVED -- `repeats`
rounds over all legs, every leg warmed up, synchronised at its start and end, and checked not to have handed the state
back.  A tool keeps its legs, its ratios and its argument parser; this module is imported by the tools only.
"""
import gc
import statistics
import time

import torch


def frames_needed(prime, clock_warm, repeats, steps, warmup):
    """frames a run consumes; steps: the timed frames of every leg of one round"""
    return prime + clock_warm + repeats * sum(n + warmup for n in steps)


class TrackerLegs:
    def __init__(self, patches, height, width, frames, dev):
        from rampvo_amd.config import make_cfg
        from rampvo_amd.Ramp_vo import Ramp_vo
        from rampvo_amd.synthetic import SyntheticStream, make_network
        torch.manual_seed(1234)
        self.slam = Ramp_vo(make_cfg("default", PATCHES_PER_FRAME=patches, MIXED_PRECISION=True),
                            make_network("SingleScale", device=dev), {"event_bias": True}, ht=height, wd=width, device=dev)
        self.slam.inputs_ready = True                 # every frame is resident before its call
        self.workload = "SingleScale %dx%d, %d patches, fp16 features, inputs_ready=True" % (width, height, patches)
        stream = SyntheticStream(height, width, frames + 1, seed=1234, device=dev)
        self.frames = [stream.frame(t) for t in range(frames)]
        self.pos = 0                                  # the next frame; the newest tracked one is pos - 1
        torch.cuda.synchronize()

    def step(self):
        im, ev, K, mask = self.frames[self.pos]
        self.slam(self.pos, input_tensor=(ev, im, mask), intrinsics=K)
        self.pos += 1

    def prime(self, prime, clock_warm):
        slam = self.slam
        for _ in range(prime):
            self.step()
        assert slam.is_initialized and slam._dev is not None and slam._dev.active, "the tracker is not device resident"
        gc.collect()
        gc.freeze()
        for _ in range(clock_warm):
            self.step()
        torch.cuda.synchronize()

    def run_legs(self, legs, steps, warmup, repeats, before=None, hands_back=()):
        """legs: name -> what runs behind every timed frame (a callable without arguments, or None); steps: timed frames per
        leg, one number or name -> number.  before(name) runs in front of a leg's warm-up; a leg named in hands_back may hand
        the state back to the host (its warm-up makes the tracker device resident again for the next leg).  Returns
        (name -> kf/s of every round, name -> hand-backs over all rounds)."""
        slam = self.slam
        rates, settled = {k: [] for k in legs}, {k: 0 for k in legs}
        for _ in range(repeats):
            for name, query in legs.items():
                n = steps[name] if isinstance(steps, dict) else steps
                if before is not None:
                    before(name)
                for _ in range(warmup):
                    self.step()
                torch.cuda.synchronize()
                settles = slam.stats["settles"]
                tic = time.perf_counter()
                for _ in range(n):
                    self.step()
                    if query is not None:
                        query()
                torch.cuda.synchronize()
                rates[name].append(n / (time.perf_counter() - tic))
                settled[name] += slam.stats["settles"] - settles
                if name not in hands_back:          # (with a hand-back leg among them the legs are held to the count alone)
                    assert slam.stats["settles"] == settles and (hands_back or slam._dev.active), "leg %s was handed back" % name
        return rates, settled


def summary(rates, what):
    """name -> {what, kf_per_s_median, min, max, rounds}, printed leg by leg"""
    out, width = {}, max(len(w) for w in what.values())
    for name, v in rates.items():
        out[name] = {"what": what[name], "kf_per_s_median": round(statistics.median(v), 1), "min": round(min(v), 1),
                     "max": round(max(v), 1), "rounds": [round(x, 1) for x in v]}
        print("leg %s  %-*s %8.1f kf/s  (min %.1f, max %.1f; rounds %s)"
              % (name, width, what[name], statistics.median(v), min(v), max(v), " ".join("%.1f" % x for x in v)))
    return out


def ratio(legs, num, den):
    return round(legs[num]["kf_per_s_median"] / legs[den]["kf_per_s_median"], 4)


def spread(leg):
    """(max - min) / median over a leg's rounds: how far identical legs differ on this box"""
    return round((leg["max"] - leg["min"]) / leg["kf_per_s_median"], 4)
