"""Write tests/golden/event_voxel.npz: the reference's own voxel-grid class (utils/transformers.py,
EventSequenceToVoxelGrid_Pytorch) run on the CPU over a handful of small event lists -- inputs and recorded outputs only.

    python tools/make_voxel_golden.py [--reference DIR] [--out FILE]

The class is imported from the reference checkout at run time (``RAMP_REFERENCE`` or --reference); nothing of it is in this
file.  Its module imports ``data`` (which pulls in h5py) for a type annotation only, so the module is loaded by path with a
stand-in ``data`` that has an ``Events`` attribute.

Per case ``NAME`` the file holds ``NAME/events`` float64 [N,4] (t, x, y, p), ``NAME/shape`` (bins, H, W), the reference's
output without and with normalisation (``ref_raw``, ``ref_norm``), the reference's own absolute error per cell against the
float64 restatement tests/voxelref.py ``grid64`` (``err_raw``, ``err_norm``), that restatement's ``mean`` and ``std``, and
``count``, the contributions per cell.

CONDITION, checked here and asserted again by tests/test_voxelref_cpu.py: in every case the reference's non-zero mask, the
float64 restatement's and the fixed-point emulator's are the same set of cells, and no non-empty cell of the random case lies
within 1e-4 of zero -- a near-cancelling cell would make mean and std differ for reasons that are no error of the kernel.  A
seed that fails is skipped for the next."""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import voxelref  # noqa: E402


def reference_class(ref_root):
    path = os.path.join(ref_root, "utils", "transformers.py")
    if not os.path.exists(path):
        raise SystemExit("no reference checkout at %s" % ref_root)
    stand_in = types.ModuleType("data")
    stand_in.Events = object
    had = sys.modules.get("data")
    sys.modules["data"] = stand_in
    try:
        spec = importlib.util.spec_from_file_location("reference_transformers", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if had is None:
            del sys.modules["data"]
        else:
            sys.modules["data"] = had
    return mod.EventSequenceToVoxelGrid_Pytorch


class Sequence:
    """what the reference class reads of an event sequence"""

    def __init__(self, events, H, W):
        self.features, self.image_height, self.image_width = events, H, W


def random_events(seed, n, H, W):
    """UNSORTED time stamps with events before the first and behind the last one by position (so that min / max differ from
    first / last and some events fall off either end), fractional float32 coordinates inside the image"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.0, 1.0, n)
    t[0], t[-1] = 0.125, 0.875
    x = rng.uniform(0, W, n).astype(np.float32).clip(0, np.nextafter(np.float32(W), np.float32(0)))
    y = rng.uniform(0, H, n).astype(np.float32).clip(0, np.nextafter(np.float32(H), np.float32(0)))
    p = rng.choice([0.0, 1.0], n)                              # (0 is read as -1)
    return np.stack([t, x.astype(np.float64), y.astype(np.float64), p], -1)


def cases(seed):
    c = {"random": (random_events(seed, 4099, 13, 17), 5, 13, 17)}
    c["three"] = (np.array([[0.0, 1.7, 2.2, 1], [0.25, 4.0, 0.0, 0], [1.0, 1.2, 2.9, 1]]), 2, 4, 5)
    c["onebin"] = (random_events(seed + 1, 50, 4, 5), 1, 4, 5)
    e = random_events(seed + 2, 20, 4, 5)
    e[:, 0] = 3.5
    c["equal_times"] = (e, 3, 4, 5)
    # events 1 and 2 cancel exactly: the same time stamp, the same pixel, opposite polarity
    c["cancel"] = (np.array([[0.0, 0.5, 0.5, 1], [0.3, 2.25, 1.5, 1], [0.3, 2.75, 1.25, 0], [0.6, 3.0, 3.0, 0], [1.0, 4.5, 3.9, 1]]),
                   2, 4, 5)
    return c


def record(cls, events, bins, H, W):
    out = {"events": events, "shape": np.array([bins, H, W], np.int64)}
    t, x, y, p = events[:, 0], events[:, 1], events[:, 2], events[:, 3]
    for key, normalize in (("raw", False), ("norm", True)):
        ref = cls(bins, gpu=False, normalize=normalize, forkserver=False)(Sequence(events.copy(), H, W)).numpy()
        g, mean, std = voxelref.grid64(x, y, t, p, H, W, bins, normalize=normalize)
        out["ref_" + key] = ref.astype(np.float32)
        out["err_" + key] = np.abs(ref.astype(np.float64) - g)
    out["mean"], out["std"] = np.float64(mean), np.float64(std)
    out["count"] = voxelref.accumulate(x, y, t, p, H, W, bins)["count"][0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("RAMP_REFERENCE"), required="RAMP_REFERENCE" not in os.environ)
    ap.add_argument("--out", default=voxelref.GOLDEN)
    ap.add_argument("--seed", type=int, default=2024)
    a = ap.parse_args()
    cls = reference_class(a.reference)
    for seed in range(a.seed, a.seed + 50):
        rec = {name: record(cls, *c) for name, c in cases(seed).items()}
        ok = all(voxelref.masks_agree(r) for r in rec.values())
        raw = rec["random"]["ref_raw"]
        ok = ok and float(np.abs(raw[raw != 0]).min()) >= 1e-4
        if ok:
            break
        print("seed %d: a near-cancelling cell or masks that differ -- next seed" % seed)
    else:
        raise SystemExit("no seed satisfies the mask condition")
    for name, r in rec.items():
        print("%-12s N=%5d  own error raw %.2e norm %.2e  mean %+.6f std %.6f  non-zero cells %d" % (
            name, len(r["events"]), r["err_raw"].max(), r["err_norm"].max(), r["mean"], r["std"], int((r["ref_raw"] != 0).sum())))
    np.savez_compressed(a.out, seed=np.int64(seed), **{"%s/%s" % (n, k): v for n, r in rec.items() for k, v in r.items()})
    print("seed %d -> %s (%d bytes)" % (seed, a.out, os.path.getsize(a.out)))


if __name__ == "__main__":
    main()
