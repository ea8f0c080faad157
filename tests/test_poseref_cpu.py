"""The pose kit (tests/poseref.py) and the splat axis (tests/splatref.py) every numpy restatement is built on: against the
rotation-matrix form, against each other, and the axis flags against values written out by hand."""
import numpy as np

import mapref
import poseref
import splatref

TOL = 1e-14                  # unit scale: about 20 double operations at 2.2e-16 each


def _quats(seed, n=64):
    q = np.random.default_rng(seed).standard_normal((n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def test_qrot_is_the_rotation_matrix():
    q, v = _quats(1), np.random.default_rng(2).uniform(-1, 1, (64, 3))
    ref = np.stack([mapref.quat_R(qi) @ vi for qi, vi in zip(q, v)])
    assert np.abs(poseref.qrot(q, v) - ref).max() <= TOL
    assert np.abs(poseref.qrot(q[0], v) - v @ mapref.quat_R(q[0]).T).max() <= TOL          # one quaternion [4] over many vectors


def test_qmul_composes_rotations():
    a, b, v = _quats(3), _quats(4), np.random.default_rng(5).uniform(-1, 1, (64, 3))
    assert np.abs(poseref.qrot(poseref.qmul(a, b), v) - poseref.qrot(a, poseref.qrot(b, v))).max() <= TOL
    assert np.array_equal(poseref.qmul(a, b)[7], poseref.qmul(a[7], b[7]))


def test_float32_stays_float32():
    a, b = _quats(6).astype(np.float32), _quats(7).astype(np.float32)
    v = np.random.default_rng(8).uniform(-1, 1, (64, 3)).astype(np.float32)
    assert poseref.qrot(a, v).dtype == np.float32 and poseref.qmul(a, b).dtype == np.float32
    assert poseref.qrot(a.astype(np.float64), v.astype(np.float64)).dtype == np.float64


def test_invert_pose_composes_to_the_identity():
    t = np.random.default_rng(9).uniform(-1, 1, (64, 3))
    for ti, qi in zip(t, _quats(10)):
        inv = poseref.invert_pose(np.r_[ti, qi])
        for (t1, q1), (t2, q2) in (((ti, qi), (inv[:3], inv[3:])), ((inv[:3], inv[3:]), (ti, qi))):
            assert np.abs(t1 + poseref.qrot(q1, t2)).max() <= TOL
            assert np.abs(poseref.qmul(q1, q2) - [0, 0, 0, 1]).max() <= TOL


def test_se3_ops_by_dtype():
    xi = np.random.default_rng(11).uniform(-0.5, 0.5, (5, 6))
    for dtype in (np.float32, np.float64):
        exp, log, inv, mul = poseref.se3_ops(dtype)
        X = exp(xi.astype(dtype))
        outs = (X, log(X), inv(X), mul(X, inv(X)))
        assert all(np.asarray(o).dtype == dtype for o in outs)
        assert np.abs(np.asarray(outs[3]) - [0, 0, 0, 0, 0, 0, 1]).max() < (1e-6 if dtype == np.float32 else 1e-14)
    exp, _, inv, _ = poseref.se3_ops(np.float32)                 # float64 in: read as float32, float32 out
    assert np.asarray(inv(exp(xi))).dtype == np.float32


def test_axis_flags_by_hand():
    """n = 4: the smallest case in which every branch of in0 / in1 is taken"""
    f, n = np.float32, 4
    below, above = (lambda c: np.nextafter(f(c), f(-9))), (lambda c: np.nextafter(f(c), f(9)))
    v = np.array([-1.5, -1.0, -0.25, 0.0, 2.999, 3.0, 3.5,
                  below(-1), above(-1), below(0), above(0), below(n - 1), above(n - 1), below(n), above(n)], f)
    floor = [-2, -1, -1, 0, 2, 3, 3, -2, -1, -1, 0, 2, 3, 3, 4]
    in0 = [0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0]            # floor in [0, n)
    in1 = [0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0]            # floor + 1 in [0, n)
    i0, (w0, w), (a, b) = splatref.axis(v, n)
    assert a.tolist() == [bool(k) for k in in0] and b.tolist() == [bool(k) for k in in1]
    assert i0.dtype == np.int64 and i0.tolist() == [fl if (p or q) else 0 for fl, p, q in zip(floor, in0, in1)]
    assert w.dtype == w0.dtype == f and np.array_equal(w, v - np.array(floor, f)) and np.array_equal(w0, f(1) - w)
    assert w[:7].tolist() == [0.5, 0.0, 0.75, 0.0, float(f(2.999) - f(2)), 0.0, 0.5]
    # the dtype of the coordinates, and the deliberate mistake: -0.25 truncates to 0, both neighbours inside
    _, (w0, w), _ = splatref.axis(v.astype(np.float64), n, dtype=None)
    assert w.dtype == w0.dtype == np.float64
    i0, (_, w), (a, b) = splatref.axis(v, n, mistake="trunc")
    assert (i0[2], w[2], a[2], b[2]) == (0, -0.25, True, True)
    assert splatref.fixed_weight(f(0.5), f(0.75), 24) == 3 << 21 and splatref.fixed_weight(f(1), f(1), 24).dtype == np.int64
