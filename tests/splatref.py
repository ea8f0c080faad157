"""The bilinear splat of the numpy references -- TEST INFRASTRUCTURE ONLY, numpy only.  One axis of it (warp_axis of
csrc/warp_device.h) and the fixed-point weight of a neighbour (warp_fixed_weight), stated once.
"""
import numpy as np


def axis(v, n, dtype=np.float32, mistake=None):
    """-> (floor int64, 0 where no neighbour lies in the image; the weights (1 - w, w) in ``dtype`` -- None: the dtype of ``v``;
    whether the neighbours floor and floor + 1 lie in [0, n)).  ``mistake="trunc"`` rounds toward zero instead"""
    dtype = np.dtype(v.dtype if dtype is None else dtype).type
    fl = (np.trunc(v) if mistake == "trunc" else np.floor(v)).astype(dtype)
    w = (v - fl).astype(dtype)
    w0 = (dtype(1) - w).astype(dtype)
    in0 = (fl >= 0) & (fl <= n - 1)
    in1 = (fl >= -1) & (fl <= n - 2)
    return np.where(in0 | in1, fl, 0).astype(np.int64), (w0, w), (in0, in1)


def fixed_weight(wx, wy, bits):
    """the fp32 product of two weights times 2^bits, rounded to the nearest integer (halves to even) -> int64"""
    return np.rint(np.ldexp((wx * wy).astype(np.float32), bits)).astype(np.int64)
