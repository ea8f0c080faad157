"""What a pose query costs: ramp_se3_interp (csrc/interp.hip) against the composition the library offered before it, and
Ramp_vo.poses_at behind every frame of the flagship workload.  ONE process, so that everything shares a box and a clock state.

  query    T = 2000 knots, Q = 2^24 queries.  Every variant of the call -- sorted / shuffled queries x without / with twist x
           the two store forms (tile through LDS, RAMP_INTERP_ROW_STORES) -- is timed with device events around the whole
           call (status memset + segment launch + query launch), warmed up, then --repeats rounds INTERLEAVED over the
           variants; printed: the median in us, min and max, and the fraction of the HBM roof on the compulsory bytes (8 B
           read + 28 B (+ 24 B) written per query; the knots do not count) against the 6.29 TB/s a float4 copy reaches on
           this part and against the 8.0 TB/s of its data sheet.
           baseline: the same poses from torch.searchsorted + the package's lietorch operators (the segments' increments
           precomputed once per call, as a caller would), same events; the ratio is quoted against THIS.
  tracker  uncertainty_cost.py's two interleaved legs on BASELINE configs[1]: no query / poses_at(10^5 device-resident
           times, as_tensor=True) behind every frame; kf/s per leg, b / a, a's own spread.

    python tools/pose_query_cost.py [--part query|tracker|both] [--json out.json]
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

HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def _knots(T, dev):
    from rampvo_amd.lietorch import SE3
    g = torch.Generator(device="cpu").manual_seed(7)
    v = torch.cumsum(torch.randn(T, 6, generator=g) * 0.01, 0) + torch.randn(1, 6, generator=g) * 0.05
    xi = torch.cumsum(v * torch.tensor([0.05, 0.03, 0.04, 0.02, 0.03, 0.02]), 0)
    return SE3.exp(xi.to(dev)).data.contiguous(), (0.05 * torch.arange(T, dtype=torch.float64)).to(dev)


def _baseline(knots, times, q):
    """the composition: searchsorted, a gather, the clamp in float64, then exp and mul launches with [Q,7] intermediates"""
    from rampvo_amd.lietorch import SE3
    T = knots.shape[0]
    xi = (SE3(knots[1:]) * SE3(knots[:-1]).inv()).log()
    s = (torch.searchsorted(times, q, right=True) - 1).clamp_(0, T - 2)
    t0 = times[s]
    alpha = ((q - t0) / (times[s + 1] - t0)).clamp_(0.0, 1.0).float()
    return (SE3.exp(alpha[:, None] * xi[s]) * SE3(knots[s])).data


def query_part(args, dev):
    from rampvo_amd import _lib
    L = _lib.lib()
    T, Q = args.knots, args.queries
    knots, times = _knots(T, dev)
    g = torch.Generator(device="cpu").manual_seed(8)
    u = torch.rand(Q, generator=g, dtype=torch.float64).to(dev) * float(times[-1])
    qs = {"sorted": torch.sort(u).values.contiguous(), "shuffled": u.contiguous()}
    out = torch.empty((Q, 7), dtype=torch.float32, device=dev)
    tw = torch.empty((Q, 6), dtype=torch.float32, device=dev)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    nbytes = L.ramp_se3_interp_workspace_bytes(T)
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev)
    variants = [(o, t, f) for o in ("sorted", "shuffled") for t in (False, True) for f in (0, _lib.RAMP_INTERP_ROW_STORES)]

    def call(order, twist, flags):
        _lib.check(L.ramp_se3_interp(_lib.ptr(knots), _lib.ptr(times), T, _lib.ptr(qs[order]), Q, flags, _lib.ptr(out),
                                     _lib.ptr(tw) if twist else None, _lib.ptr(ws), nbytes, _lib.ptr(status), _lib.stream()),
                   "ramp_se3_interp")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3                  # us

    # the two store forms give the same bits, and the kernel the baseline's poses within the fp32 formulas' noise
    call("sorted", True, 0)
    ref_o, ref_t = out.clone(), tw.clone()
    call("sorted", True, _lib.RAMP_INTERP_ROW_STORES)
    assert torch.equal(ref_o.view(torch.int32), out.view(torch.int32)) and torch.equal(ref_t.view(torch.int32), tw.view(torch.int32))
    base = _baseline(knots, times, qs["sorted"])
    dq = torch.minimum((base[:, 3:] - ref_o[:, 3:]).abs().amax(1), (base[:, 3:] + ref_o[:, 3:]).abs().amax(1))
    agree = max(float((base[:, :3] - ref_o[:, :3]).abs().max()), float(dq.max()))
    del ref_o, ref_t, base, dq
    for v in variants:
        for _ in range(args.warmup):
            call(*v)
    for _ in range(2):
        _baseline(knots, times, qs["sorted"])
    torch.cuda.synchronize()
    us = {v: [] for v in variants}
    base_us = {"sorted": [], "shuffled": []}
    for r in range(args.repeats):
        for v in variants:
            us[v].append(timed(lambda: call(*v)))
        if r < args.baseline_repeats:
            for o in base_us:
                base_us[o].append(timed(lambda: _baseline(knots, times, qs[o])))
    res = {"T": T, "Q": Q, "repeats": args.repeats, "agreement_with_baseline": agree, "variants": [], "baseline": {}}
    for (o, t, f), v in us.items():
        med, nb = statistics.median(v), Q * (8 + 28 + (24 if t else 0))
        row = {"queries": o, "twist": t, "stores": "row" if f else "lds", "us_median": round(med, 1), "us_min": round(min(v), 1),
               "us_max": round(max(v), 1), "GBps": round(nb / med / 1e3, 1), "of_measured_roof": round(nb / (med * 1e-6) / HBM_MEASURED, 3),
               "of_spec_roof": round(nb / (med * 1e-6) / HBM_SPEC, 3)}
        res["variants"].append(row)
        print("query  %-8s twist %-5s stores %-3s  %9.1f us (min %.1f, max %.1f)  %7.1f GB/s  %.3f of 6.29 TB/s, %.3f of 8.0 TB/s"
              % (o, t, row["stores"], med, min(v), max(v), row["GBps"], row["of_measured_roof"], row["of_spec_roof"]))
    for o, v in base_us.items():
        med = statistics.median(v)
        best = min(r["us_median"] for r in res["variants"] if r["queries"] == o and not r["twist"] and r["stores"] == "lds")
        res["baseline"][o] = {"us_median": round(med, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1),
                              "over_kernel": round(med / best, 2)}
        print("baseline %-8s (searchsorted + lietorch, no twist)  %9.1f us (min %.1f, max %.1f)  = %.2f x the kernel (lds stores)"
              % (o, med, min(v), max(v), med / best))
    print("largest difference kernel / baseline, sorted queries: %.2e" % agree)
    return res


def tracker_part(args, dev):
    steps, warmup, repeats = args.steps, args.tracker_warmup, args.tracker_repeats
    t = tl.TrackerLegs(args.patches, args.height, args.width,
                       tl.frames_needed(args.prime, args.clock_warm, repeats, [steps] * 2, warmup), dev)
    frac = torch.sort(torch.rand(args.tracker_queries, dtype=torch.float64, device=dev)).values
    t.prime(args.prime, args.clock_warm)
    last = [None]

    def query():
        last[0] = t.slam.poses_at(frac * float(t.pos - 1), as_tensor=True)

    rates, _ = t.run_legs({"a": None, "b": query}, steps, warmup, repeats)
    out = {"workload": t.workload, "queries_per_frame": args.tracker_queries, "steps": steps, "repeats": repeats,
           "frames_at_end": t.pos}
    out["legs"] = tl.summary(rates, {"a": "no query", "b": "poses_at(%d times) per call" % args.tracker_queries})
    out["b_over_a"], out["a_spread"] = tl.ratio(out["legs"], "b", "a"), tl.spread(out["legs"]["a"])
    out["last_status"] = last[0][2].cpu().tolist()
    print("b / a = %.4f   (a's own spread, (max - min) / median: %.4f)" % (out["b_over_a"], out["a_spread"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("query", "tracker", "both"), default="both")
    ap.add_argument("--knots", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1 << 24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--baseline-repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--tracker-repeats", type=int, default=5)
    ap.add_argument("--tracker-warmup", type=int, default=20)
    ap.add_argument("--tracker-queries", type=int, default=100000)
    ap.add_argument("--prime", type=int, default=70)
    ap.add_argument("--clock-warm", type=int, default=480)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--patches", type=int, default=96)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pose_query_cost.py measures on the GPU; there is nothing to report without one"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {}
    if args.part in ("query", "both"):
        out["query"] = query_part(args, dev)
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
