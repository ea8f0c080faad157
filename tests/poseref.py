"""The pose kit of the numpy references -- TEST INFRASTRUCTURE ONLY.  What every restatement needs of a pose (t, q), q = (x, y, z, w),
stated once: the oracle's SE(3) operations by dtype, the rotation of a vector, the Hamilton product, the inverse.
"""
import numpy as np

import oracle as orc


def se3_ops(dtype):
    """-> (exp, log, inv, mul): ``orc.se3_*_f64`` for float64, else the fp32 oracle (the reference's float formulas), which
    reads its arguments as contiguous float32"""
    if dtype == np.float64:
        return orc.se3_exp_f64, orc.se3_log_f64, orc.se3_inv_f64, orc.se3_mul_f64
    f = lambda fn: (lambda *a: fn(*[np.ascontiguousarray(v, np.float32) for v in a]))
    return f(orc.se3_exp), f(orc.se3_log), f(orc.se3_inv), f(orc.se3_mul)


def qrot(q, v):
    """lietorch's rotation of v [..., 3] by the quaternion q [..., 4] or [4], taken as stored: uv = 2 q x v, (v + w uv) + q x uv,
    in the dtype of the inputs.  This is lt_qrot of csrc/ramp_device.h operation for operation -- a cross product's component is
    a_i b_j - a_j b_i, doubling is exact, numpy rounds every operation and fuses nothing -- so in float32 it gives the kernel's
    bits"""
    two = q.dtype.type(2)
    uv = two * np.cross(q[..., :3], v)
    return v + q[..., 3:4] * uv + np.cross(q[..., :3], uv)


def qmul(a, b):
    """the Hamilton product a b, xyzw, over leading axes"""
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz], -1)


def invert_pose(cam):
    """the inverse of (t, q), float64, unit q"""
    cam = np.asarray(cam, np.float64)
    qi = cam[3:] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([-qrot(qi, cam[:3]), qi])
