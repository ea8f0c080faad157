"""Record what the library's workspace size queries return: tests/golden/workspace_bytes.json.

    RAMP_HIP_LIB=/path/to/libramp_hip.so python tools/record_workspace_bytes.py [--out FILE] [--hipcub]

The sizes are ABI: a caller may have stored one.  The fixture is recorded from the library of the commit BEFORE a change to the
workspace code (build that commit in a copy of the tree and point RAMP_HIP_LIB at its library) and
tests/test_workspace_sizes_cpu.py holds the current library to it, value for value.  No GPU is needed: the queries are host
arithmetic.

Per query the file holds a list of [arguments, value].  The arguments sit on both sides of every boundary inside the sizes:
0, negative and 1; E around the 256-byte rows (255, 256, 257); T around one knot and around the 4096 knots staged in LDS; N
around the 64-sample chunk and the 4096-sample tile of the propagation; K of 2, 3, 5; voxel slices 1 and 3 at 5 x 13 x 17; the
bundle adjustment at the (100, 11, 88, 1, 11) problem of the CPU tests.

--hipcub records the four families whose size contains hipcub's temporary storage instead (ramp_group_by, ramp_neighbors,
ramp_event_filter, the unplanned bundle adjustment).  That term may differ between rocPRIM builds, so it is kept out of the
fixture; record it twice on one machine, before and after, and compare the two files.
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

E_EDGES = (-1, 0, 1, 255, 256, 257)
T_EDGES = (-1, 0, 1, 2, 5, 4095, 4096, 4097)
N_EDGES = (-1, 0, 1, 63, 64, 65, 1000, 4095, 4096, 4097)
K_EDGES = (-1, 0, 1, 2, 3, 5)
BA = (100, 11, 88, 1, 11)

CASES = {
    "ramp_group_by_small_workspace_bytes": list(itertools.product(E_EDGES, (-3, -1, 0, 1, 5, 62, 63, 64, 4096))),
    "ramp_track_plan_workspace_bytes": [(e, k, p) for e in E_EDGES for k, p in ((-1, -1), (0, 0), (1, 1), (30, 31), (31, 30),
                                                                                  (62, 62), (960, 121))],
    "ramp_track_ba_workspace_bytes": [(e, 11, 8, w, kc, ic) for e in E_EDGES for w in (0, 1, 10)
                                      for kc, ic in ((0, 0), (1, 1), (88, 121), (1000, 1000))] + [(100, 0, 8, 10, 88, 121)],
    "ramp_ba_planned_workspace_bytes": None,                      # (filled below: the three planned queries share their cases)
    "ramp_ba_covariance_planned_workspace_bytes": None,
    "ramp_ba_map_covariance_planned_workspace_bytes": None,
    "ramp_se3_interp_workspace_bytes": [(t,) for t in T_EDGES],
    "ramp_event_warp_workspace_bytes": [(t, b, h, w) for t in T_EDGES for b in (-1, 0, 1, 5)
                                        for h, w in ((24, 32), (1, 1), (13, 17), (0, 32), (24, 0), (-1, -1))],
    "ramp_event_contrast_workspace_bytes": [(t, h, w) for t in T_EDGES
                                            for h, w in ((24, 32), (1, 1), (13, 17), (0, 32), (24, 0), (-1, -1))],
    "ramp_event_align_workspace_bytes": [(t, h, w) for t in T_EDGES
                                         for h, w in ((24, 32), (1, 1), (13, 17), (0, 32), (24, 0), (-1, -1))],
    "ramp_event_voxel_workspace_bytes": [(s, 5, 13, 17) for s in (-1, 0, 1, 2, 3, 4096)]
                                        + [(s, b, h, w) for s in (1, 3) for b, h, w in ((0, 13, 17), (5, 0, 17), (5, 13, 0), (1, 1, 1),
                                                                                       (1, 16, 16), (1, 255, 257), (8, 260, 346))],
    "ramp_invdepth_map_workspace_bytes": [(k,) for k in (-1, 0, 1, 2, 3, 5, 255, 256, 257)],
    "ramp_imu_workspace_bytes": list(itertools.product(N_EDGES, K_EDGES + (256, 257, 258, 1000))),
    "ramp_imu_propagate_workspace_bytes": [(n,) for n in N_EDGES + (8191, 8192, 8193, 2147483647)],
    "ramp_event_topk_workspace_bytes": [(h, w) for h, w in ((-4, -4), (0, 0), (1, 1), (3, 3), (4, 4), (7, 9), (128, 160),
                                                            (255, 257), (260, 346))],
    "ramp_event_stack_workspace_bytes": [(b, h, w) for b in (0, 1, 5) for h, w in ((0, 0), (1, 1), (13, 17), (128, 160))],
}
_PLANNED = [BA + m for m in ((0, 0), (1, 1), (88, 121), (5, 7), (1000, 1000))] + \
           [(e, 11, 88, 1, t1, 88, 121) for e in E_EDGES for t1 in (0, 1, 2, 11)] + [(100, 1, 1, 0, 1, 1, 1), (100, 11, 88, 5, 5, 88, 121)]
for _name in ("ramp_ba_planned_workspace_bytes", "ramp_ba_covariance_planned_workspace_bytes",
              "ramp_ba_map_covariance_planned_workspace_bytes"):
    CASES[_name] = _PLANNED

_UNPLANNED = [BA] + [(e, 11, 88, 1, t1) for e in E_EDGES for t1 in (0, 1, 2, 11)]
HIPCUB_CASES = {
    "ramp_group_by_workspace_bytes": [(e,) for e in E_EDGES + (4099, 100000)],
    "ramp_neighbors_workspace_bytes": [(e,) for e in E_EDGES + (4099, 100000)],
    "ramp_event_filter_workspace_bytes": [(n, h, w) for n in (-1, 0, 1, 255, 256, 257, 4099, 100000)
                                          for h, w in ((13, 17), (1, 1), (0, 17), (260, 346))],
    "ramp_ba_workspace_bytes": _UNPLANNED,
    "ramp_ba_covariance_workspace_bytes": _UNPLANNED,
    "ramp_ba_map_covariance_workspace_bytes": _UNPLANNED,
}


def record(cases):
    from rampvo_amd import _lib
    lib = _lib.lib()
    return {name: [[list(args), int(getattr(lib, name)(*args))] for args in rows] for name, rows in cases.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--hipcub", action="store_true", help="the four families with hipcub's term (not the fixture)")
    args = ap.parse_args()
    out = args.out or os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")
    if args.hipcub and args.out is None:
        raise SystemExit("--hipcub writes no fixture: name a file with --out")
    recorded = record(HIPCUB_CASES if args.hipcub else CASES)
    with open(out, "w") as f:                                   # one query per line
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(name), json.dumps(rows, separators=(",", ":")))
                                   for name, rows in recorded.items()) + "\n}\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
