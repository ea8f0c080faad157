"""The pose-geometry and frame-bookkeeping kernels (csrc/ramp_device.h, csrc/lie.hip, the frame launches of
csrc/select.hip), called through the C ABI, against float64 (tests/georef.py).

Bounds, stated once.  For every operator and every input bin the error is measured against float64 of the same
fp32-rounded inputs, and the bound is max(floor, 4 * env):
  floor  the unit-scale bound of test_se3_ops_match_oracle for that operator (2e-6 exp / inv / mul, 5e-6 log / act4,
         1e-5 adj / adjT) times max(1, |operands|); for pixel outputs 1e-5 of the largest coordinate, as
         test_transform_reproject_point_cloud;
  env    the fp32 oracle's (or the fp32 numpy restatement's) own worst error against float64 in that bin, computed here:
         the envelope of the reference's float formulas, never of the kernel.
The factor 4 is test_ba_matches_oracle's (a device cosf / sinf / atanf a few ulp from the host's).  The kernels keep the
reference's Jacobian coefficients, whose (1 - cos t) / t^2 cancels for rotations of 1e-6 .. 1e-2 rad: those bins of exp
and of the motion model are held to 4 * env like every other (DESIGN.md 2.1 says why the cancellation-free forms are out).  Every test prints (measured, envelope, bound) per
bin before it asserts; DESIGN.md 2.1 carries the envelope table.

Bookkeeping launches (multi_copy / store_rows, shift_rows, frame_begin, frame_commit, depth_median) are compared as
32-bit words, with canaries around everything they may write."""
import ctypes

import numpy as np
import pytest
import torch

import georef as gr
import oracle as orc
from trackerkit import cu
from rampvo_amd._lib import RAMP_EINVAL as EINVAL, RAMP_EUNSUPPORTED as EUNSUPPORTED

pytestmark = pytest.mark.gpu

CANARY = 0x7fc0beef                      # a NaN pattern: a write of any float shows, and so does a read that propagates


def _api():
    from rampvo_amd import _lib
    return _lib.lib(), _lib.ptr, _lib.stream


def _words(t):
    return t.cpu().numpy().view(np.int32) if t.element_size() == 4 else t.cpu().numpy()


def _canary(shape):
    return torch.full(shape, CANARY, dtype=torch.int32, device="cuda").view(torch.float32)


# ----------------------------------------------------------------------------------------------------------------- SE3
THETAS = [0.0, 1e-8, 5e-7, float(np.float32(1e-6)), 2e-6, 1e-5, 1e-4, 1e-3, 1e-2, 0.1, 1.0, 3.0, float(np.pi - 1e-3)]
TSCALES = [0.0, 1.0, 1e3]
NB = 513                                 # rows per bin, and the largest batch
SIZES = (0, 1, 255, 256, 257, 513)
OPS = {  # name: (input widths, output width)
    "exp": ((6,), 7), "log": ((7,), 6), "inv": ((7,), 7), "mul": ((7, 7), 7), "act4": ((7, 4), 4), "adj": ((7, 6), 6),
    "adjT": ((7, 6), 6)}


def _axes(rng, n):
    ax = rng.normal(size=(n, 3))
    ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ax[:6] = np.concatenate([np.eye(3), -np.eye(3)])          # axis-aligned: the computed angle is the bin's to one rounding
    return ax


@pytest.fixture(scope="module")
def se3_case():
    """every (rotation, translation scale) bin, NB rows each, as fp32; the float64 and the fp32-oracle results of every
    operator on them (computed once, shared, never written)"""
    rng = np.random.default_rng(11)
    bins = [(th, ts) for th in THETAS for ts in TSCALES]
    a, a2 = [], []
    for th, ts in bins:
        a.append(np.concatenate([ts * rng.normal(size=(NB, 3)), th * _axes(rng, NB)], 1))
        a2.append(np.concatenate([ts * rng.normal(size=(NB, 3)), th * _axes(rng, NB)[::-1]], 1))
    a = np.concatenate(a).astype(np.float32)
    X = orc.se3_exp_f64(a).astype(np.float32)
    Y = orc.se3_exp_f64(np.concatenate(a2)).astype(np.float32)
    # log reads q, -q, q / 2 and 2 q in turn (lt_load normalises)
    Xl = X.copy()
    Xl[:, 3:] *= np.array([1.0, -1.0, 0.5, 2.0], np.float32)[np.arange(len(X)) % 4, None]
    p = rng.normal(size=(len(X), 4)).astype(np.float32)
    b = rng.normal(size=(len(X), 6)).astype(np.float32)
    ins = {"exp": (a,), "log": (Xl,), "inv": (X,), "mul": (X, Y), "act4": (X, p), "adj": (X, b), "adjT": (X, b)}
    ref = {k: getattr(orc, "se3_%s_f64" % k)(*v) for k, v in ins.items()}
    f32 = {k: getattr(orc, "se3_%s" % k)(*v) for k, v in ins.items()}
    return dict(bins=bins, ins=ins, ref=ref, f32=f32)


def _se3_call(name, ins, n, out):
    """ramp_se3_<name> on the first n rows of ``ins`` into ``out`` (device tensors), through the C ABI"""
    L, ptr, stream = _api()
    rc = getattr(L, "ramp_se3_" + name)(*[ptr(t) for t in ins], ptr(out), int(n), stream())
    assert rc == 0, (name, n, rc)


@pytest.fixture(scope="module")
def se3_gpu(se3_case):
    """one launch per operator over every bin; one canary row behind the output"""
    out = {}
    for name, (_, dout) in OPS.items():
        ins = [cu(x) for x in se3_case["ins"][name]]
        n = ins[0].shape[0]
        o = _canary((n + 1, dout))
        _se3_call(name, ins, n, o)
        w = _words(o)
        assert (w[n] == CANARY).all(), name
        out[name] = (ins, o[:n].cpu().numpy())
    return out


@pytest.mark.parametrize("name", list(OPS))
def test_se3_op_against_float64_per_bin(se3_case, se3_gpu, name):
    c = se3_case
    got = se3_gpu[name][1]
    tab = gr.Table("ramp_se3_%s: error against float64 per (rotation, translation scale) bin, %d rows each" % (name, NB))
    assert np.isfinite(got).all()
    for k, (th, ts) in enumerate(c["bins"]):
        r = slice(k * NB, (k + 1) * NB)
        scale = max(1.0, max(float(np.abs(x[r]).max()) for x in c["ins"][name]))
        floor = gr.FLOOR[name] * scale
        tab.add("theta %.7g, |t| ~ %g" % (th, ts), gr.max_err(got[r], c["ref"][name][r]),
                gr.max_err(c["f32"][name][r], c["ref"][name][r]), floor)
    tab.show()
    assert not tab.failed(), tab.failed()


@pytest.mark.parametrize("name", list(OPS))
def test_se3_op_batch_sizes_and_launch_tail(se3_gpu, name):
    """n = 0, 1, 255, 256, 257, 513 rows (mixed bins): the rows of the full launch bit for bit, nothing behind row n"""
    ins, full = se3_gpu[name]
    dout = OPS[name][1]
    pick = torch.arange(NB, device="cuda") * len(THETAS) * len(TSCALES) % ins[0].shape[0]     # one row of many bins
    sub = [t[pick].contiguous() for t in ins]
    want = full[pick.cpu().numpy()]
    for n in SIZES:
        o = _canary((n + 1, dout))
        _se3_call(name, sub, n, o)
        w = _words(o)
        assert (w[n:] == CANARY).all(), (name, n)
        assert gr.same_bits(o[:n].cpu().numpy(), want[:n]), (name, n)


def test_se3_log_at_rotation_by_pi():
    """|w| < 1e-6 with both signs: lt_so3_log takes +-pi / |v|.  Compared as a rotation -- exp_f64(log) against the input,
    the quaternion up to its sign -- so that the test does not depend on which of +-pi the branch picks"""
    from rampvo_amd import ops
    rng = np.random.default_rng(12)
    tab = gr.Table("ramp_se3_log at rotation by pi: exp_f64(log(X)) against X")
    for ts in TSCALES:
        w = np.tile(np.array([0.0, 1e-9, 1e-7, 5e-7, 9e-7, -1e-9, -1e-7, -5e-7, -9e-7]), 57)[:NB]
        ax = _axes(rng, NB)
        X = np.concatenate([ts * rng.normal(size=(NB, 3)), ax * np.sqrt(1 - w * w)[:, None], w[:, None]], 1).astype(np.float32)
        assert (np.abs(X[:, 6]) < 1e-6).all()
        Xn = X.astype(np.float64)
        Xn[:, 3:] /= np.linalg.norm(Xn[:, 3:], axis=1, keepdims=True)
        got = ops.se3_unary("ramp_se3_log", cu(X), 7, 6).cpu().numpy()
        assert np.isfinite(got).all()
        ang = np.linalg.norm(got[:, 3:].astype(np.float64), axis=1)
        assert np.abs(ang - np.pi).max() < 1e-5
        err = gr.pose_err(orc.se3_exp_f64(got), Xn)
        env = gr.pose_err(orc.se3_exp_f64(orc.se3_log(X)), Xn)
        tab.add("|w| < 1e-6, |t| ~ %g" % ts, err, env, gr.FLOOR["log"] * max(1.0, float(np.abs(X).max())))
    tab.show()
    assert not tab.failed(), tab.failed()


# -------------------------------------------------------------------------------------- motion model, frame_begin / commit
MM_ROT = [0.0, 1e-5, 1e-4, 1e-3, 1e-2, 0.1]
MM_STEP = [0.0, 0.05, 1.0]
MM_DAMP = [0.0, 0.5, 1.0]
MM_DRAWS = 8


def _motion_cases():
    """(rot, step) bins x MM_DRAWS draws: three pose rows each -- P[n-2] random, P[n-1] = Exp([step u, rot v]) P[n-2], row n
    a canary -- as fp32"""
    rng = np.random.default_rng(13)
    bins = [(r, s) for r in MM_ROT for s in MM_STEP]
    rows = []
    for r, s in bins:
        P2 = orc.se3_exp_f64(np.concatenate([rng.normal(size=(MM_DRAWS, 3)), 0.5 * rng.normal(size=(MM_DRAWS, 3))], 1))
        u = rng.normal(size=(MM_DRAWS, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        P1 = orc.se3_mul_f64(orc.se3_exp_f64(np.concatenate([s * u, r * _axes(rng, MM_DRAWS + 6)[6:]], 1)), P2)
        rows.append(np.stack([P2, P1], 1))
    return bins, np.concatenate(rows).astype(np.float32)                 # [bins * draws, 2, 7]


@pytest.mark.parametrize("entry", ["ramp_motion_model", "ramp_frame_begin"])
def test_motion_model_against_float64(entry):
    L, ptr, stream = _api()
    bins, pairs = _motion_cases()
    C = len(pairs)
    tab = gr.Table("%s: DAMPED_LINEAR against float64 per (inter-frame rotation, step) bin, damping 0 / 0.5 / 1, %d draws"
                   % (entry, MM_DRAWS))
    errs, envs = np.zeros((C, 3)), np.zeros((C, 3))
    for di, damping in enumerate(MM_DAMP):
        buf = _canary((C, 4, 7))                                      # rows n-2, n-1, n and one canary row per case
        buf[:, :2] = cu(pairs)
        before = _words(buf)
        for c in range(C):
            base = ctypes.c_void_p(buf.data_ptr() + c * 4 * 7 * 4)
            if entry == "ramp_motion_model":
                rc = L.ramp_motion_model(base, 2, damping, stream())
            else:
                rc = L.ramp_frame_begin(base, 2, 1, damping, None, 0, None, 0, None, 0, stream())
            assert rc == 0
        after = _words(buf)
        assert np.array_equal(after[:, [0, 1, 3]], before[:, [0, 1, 3]])    # inputs and the row behind: untouched
        got = buf[:, 2].cpu().numpy()
        assert np.isfinite(got).all()
        for c in range(C):
            ref = gr.motion_model(pairs[c], 2, damping)
            errs[c, di] = gr.pose_err(got[c], ref)
            envs[c, di] = gr.pose_err(gr.motion_model_f32(pairs[c], 2, damping), ref)
    for k, (r, s) in enumerate(bins):
        sl = slice(k * MM_DRAWS, (k + 1) * MM_DRAWS)
        floor = gr.FLOOR["exp"] * max(1.0, float(np.abs(pairs[sl]).max()))
        tab.add("rotation %g, step %g" % (r, s), errs[sl].max(), envs[sl].max(), floor)
    tab.show()
    assert not tab.failed(), tab.failed()


@pytest.mark.parametrize("entry", ["ramp_motion_model", "ramp_frame_begin"])
def test_motion_model_of_a_stationary_camera(entry):
    """rows n-1 and n-2 bit-equal: Log of (nearly) the identity -- the result is finite and is row n-1 within the floor"""
    L, ptr, stream = _api()
    rng = np.random.default_rng(14)
    P = orc.se3_exp_f64(np.concatenate([rng.normal(size=(16, 3)), rng.normal(size=(16, 3))], 1)).astype(np.float32)
    P[0] = [0, 0, 0, 0, 0, 0, 1]
    for damping in MM_DAMP:
        buf = _canary((16, 4, 7))
        buf[:, 0] = cu(P)
        buf[:, 1] = cu(P)
        for c in range(16):
            base = ctypes.c_void_p(buf.data_ptr() + c * 4 * 7 * 4)
            rc = (L.ramp_motion_model(base, 2, damping, stream()) if entry == "ramp_motion_model" else
                  L.ramp_frame_begin(base, 2, 1, damping, None, 0, None, 0, None, 0, stream()))
            assert rc == 0
        got = buf[:, 2].cpu().numpy()
        assert np.isfinite(got).all()
        assert (_words(buf)[:, 3] == CANARY).all()
        for c in range(16):
            assert gr.pose_err(got[c], P[c]) <= gr.FLOOR["exp"] * max(1.0, float(np.abs(P[c]).max())), (damping, c)


def _frame_state(seed, N=8, M=8, P=3):
    """random words everywhere a frame launch may write; poses and patches are numbers (they are computed with)"""
    rng = np.random.default_rng(seed)
    rw = lambda *s: rng.integers(-2 ** 31, 2 ** 31, s, dtype=np.int64).astype(np.int32)
    xi = np.cumsum(rng.normal(0, [0.05, 0.03, 0.02, 1e-3, 1e-3, 1e-3], (N, 6)), 0)
    st = dict(poses=cu(orc.se3_exp_f64(xi).astype(np.float32)),
              tstamps=cu(rw(N, 2)).view(torch.int64).reshape(N), index_map=cu(rw(N + 1, 2)).view(torch.int64).reshape(N + 1),
              intrinsics=cu(rw(N, 4)).view(torch.float32),
              patches=cu(rng.normal(size=(N, M, 3, P, P)).astype(np.float32)),
              patches_new=cu(rng.normal(size=(M, 3, P, P)).astype(np.float32)))
    return st


def _snap(st):
    return {k: (v.cpu().numpy().copy() if not isinstance(v, list) else [x.cpu().numpy().copy() for x in v]) for k, v in st.items()}


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


@pytest.mark.parametrize("motion", [0, 1, 2])
@pytest.mark.parametrize("copy_k", [0, 1])
def test_frame_begin_writes_its_elements_and_nothing_else(motion, copy_k):
    from rampvo_amd import ops
    n = 5
    st = _frame_state(20 + motion)
    b = _snap(st)
    ops.frame_begin(st["poses"], n, motion, 0.5, st["tstamps"], 1234567890123, st["index_map"], 96, st["intrinsics"], copy_k)
    a = _snap(st)
    exp = {k: v.copy() for k, v in b.items()}
    exp["tstamps"][n] = 1234567890123
    exp["index_map"][n + 1] = 96
    if copy_k:
        exp["intrinsics"][n] = b["intrinsics"][n - 1]
    if motion == 2:
        exp["poses"][n] = b["poses"][n - 1]
    if motion == 1:
        ref = gr.motion_model(b["poses"], n, 0.5)
        assert gr.pose_err(a["poses"][n], ref) <= gr.bound(gr.FLOOR["exp"], gr.pose_err(gr.motion_model_f32(b["poses"], n, 0.5), ref))
        exp["poses"][n] = a["poses"][n]
    for k in exp:
        assert np.array_equal(_bits(a[k]), _bits(exp[k])), k


@pytest.mark.parametrize("median_frames", [0, 3])
@pytest.mark.parametrize("median_given", [False, True])
@pytest.mark.parametrize("n_copy", [0, 1, 6])
def test_frame_commit_is_its_three_launches_bit_for_bit(median_frames, median_given, n_copy):
    """ramp_frame_commit == ramp_frame_begin + ramp_depth_median_fill + store_rows (the new patch row included)"""
    from rampvo_amd import ops
    n, N = 5, 8
    motion, copy_k = (1, 1) if n_copy != 1 else (2, 0)
    rng = np.random.default_rng(30 + n_copy)
    row_words = [4, 1025, 3, 16388, 257, 1][:n_copy]                  # 16 B, 4100 B, 12 B, 64 KiB + 16 B, 1028 B, 4 B
    rows = [int(r) for r in rng.integers(0, N, n_copy)]

    def make():
        st = _frame_state(31)
        r2 = np.random.default_rng(32)
        rw = lambda *s: r2.integers(-2 ** 31, 2 ** 31, s, dtype=np.int64).astype(np.int32)
        st["srcs"] = [cu(rw(w)) for w in row_words]
        st["bufs"] = [cu(rw(N, w)) for w in row_words]
        return st

    A, B = make(), make()
    med = None
    if median_given:
        med = _canary((1,))
        if median_frames:
            ops.depth_median(A["patches"], n, median_frames, med)
    ops.frame_commit(A["poses"], n, motion, 0.5, A["tstamps"], 77, A["index_map"], 48, A["intrinsics"], copy_k, A["patches"],
                     median_frames, A["patches_new"], A["srcs"], list(zip(A["bufs"], rows)), median_dev=med)
    ops.frame_begin(B["poses"], n, motion, 0.5, B["tstamps"], 77, B["index_map"], 48, B["intrinsics"], copy_k)
    if median_frames:
        ops.depth_median_fill(B["patches"], n, median_frames, B["patches_new"])
    ops.store_rows([B["patches_new"]] + B["srcs"], [(B["patches"], n)] + list(zip(B["bufs"], rows)))
    a, b = _snap(A), _snap(B)
    for k in a:
        for x, y in zip(a[k] if isinstance(a[k], list) else [a[k]], b[k] if isinstance(b[k], list) else [b[k]]):
            assert np.array_equal(_bits(x), _bits(y)), k
    # and the launch did something: the new patch row is the (filled) new patches, the stored rows are the sources
    assert np.array_equal(_bits(a["patches"][n]), _bits(a["patches_new"]))
    if median_frames:
        m = gr.lower_median(_snap(_frame_state(31))["patches"][n - median_frames:n, :, 2])
        assert (a["patches_new"][:, 2] == m).all()
    for s_, bf, r in zip(a["srcs"], a["bufs"], rows):
        assert np.array_equal(bf[r], s_)


# ------------------------------------------------------------------------------------------------------------ motionmag
MM_SIZES = [(0, 257), (1, 256), (255, 1000), (256, 255), (257, 1), (1000, 0), (0, 0)]


@pytest.mark.parametrize("grouping", ["group_by", "group_by_small"])
def test_motionmag_against_float64(grouping):
    """both directions of the keyframe motion test over pair groupings made on the device: segments of 0 .. 1000 factors
    (the 256-stride loop and the reduction), the key as the first / the last of the unique keys or absent, beta 0 / 0.5 / 1,
    intrinsics of its own for every frame, points behind the target camera (the clamp)"""
    from rampvo_amd import ops
    tab = gr.Table("ramp_motionmag (%s): mean flow magnitude against float64 per (factors i->j, factors j->i, beta)" % grouping)
    f32 = lambda *x: orc.transform(*x)
    for c_i, (n_ij, n_ji) in enumerate(MM_SIZES):
        i, j = ((0, 2), (5, 7))[c_i % 2]
        c = gr.mm_case(40 + c_i, i, j, n_ij, n_ji)
        dev = [cu(c[k]) for k in ("poses", "patches", "intr", "ii", "jj", "kk")]
        keys = cu(c["keys"])
        if grouping == "group_by":
            g = ops.group_by(keys)
        else:
            g = ops.group_by_small(dev[4], dev[3], gr.PAIR_MUL, 0, gr.PAIR_MUL * c["n_frames"])
        G = int(g.ngroups.item())
        uk = g.ukeys[:G].cpu().numpy()
        assert np.array_equal(uk, np.unique(c["keys"]))
        if n_ji:
            assert uk[0] == c["key_ji"] if (i, j) == (0, 2) else True
        if n_ij and (i, j) == (5, 7):
            assert uk[-1] == c["key_ij"]
        a = (c["poses"], c["patches"], c["intr"], c["ii"], c["jj"], c["kk"], c["keys"])
        for beta in (0.0, 0.5, 1.0):
            got = ops.motionmag(*dev, g, c["key_ij"], c["key_ji"], beta=beta).cpu().numpy()
            for d, (key, cnt) in enumerate(((c["key_ij"], n_ij), (c["key_ji"], n_ji))):
                if cnt == 0:
                    assert np.isnan(got[d]), (n_ij, n_ji, beta, d)
                    continue
                ref = gr.motionmag(*a, key, beta)
                env = abs(gr.motionmag(*a, key, beta, xform=f32) - ref)
                sel = c["keys"] == key
                cmax = max(float(np.abs(gr.transform(*a[:3], c["ii"][sel], x, c["kk"][sel], t)).max())
                           for x, t in ((c["ii"][sel], False), (c["jj"][sel], False), (c["jj"][sel], True)))
                tab.add("%d / %d factors, beta %.1f, %s" % (n_ij, n_ji, beta, "i->j" if d == 0 else "j->i"),
                        abs(float(got[d]) - ref), env, gr.PIXEL_FLOOR * cmax)
        # a key below all and a key above all: no segment, NaN
        lo, hi = int(uk[0]) - 1, int(uk[-1]) + 1
        got = ops.motionmag(*dev, g, lo, hi, beta=0.5).cpu().numpy()
        assert np.isnan(got).all(), (n_ij, n_ji)
    tab.show()
    assert not tab.failed(), tab.failed()


# ------------------------------------------------------------------------------ transform / reproject / point_cloud
E_SIZES = (0, 1, 255, 256, 257)


def _pixel_row(tab, name, got, ref, f32, keep=None):
    cmax = float(np.abs(ref if keep is None else ref[keep]).max()) if ref.size else 1.0
    tab.add(name, gr.max_err(got, ref, keep), gr.max_err(f32, ref, keep), gr.PIXEL_FLOOR * cmax)


def test_transform_reproject_point_cloud_against_float64():
    """distinct intrinsics per frame (row i in, row j out; row 0 for reproject; row ix[n] for the point cloud), inverse
    depths down to 1e-6, points on both sides of the Z clamp and behind the camera, E / m across the launch tail"""
    L, ptr, stream = _api()
    tab = gr.Table("ramp_transform / ramp_reproject / ramp_point_cloud against float64, per size")
    for E in E_SIZES:
        s = gr.geo_scene(50 + E, E=E)
        a = (s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"])
        dev = [cu(x) for x in a]
        for tonly in (0, 1):
            out = _canary((E + 1, 2, 3, 3))
            assert L.ramp_transform(*[ptr(t) for t in dev], ptr(out), E, 3, tonly, stream()) == 0
            assert (_words(out)[E] == CANARY).all()
            if E:
                _pixel_row(tab, "transform E %d tonly %d" % (E, tonly), out[:E].cpu().numpy()[None], gr.transform(*a, bool(tonly)),
                           orc.transform(*a, bool(tonly)))
        out = _canary((E + 1, 2, 3, 3))
        assert L.ramp_reproject(*[ptr(t) for t in dev], ptr(out), E, 3, stream()) == 0
        assert (_words(out)[E] == CANARY).all()
        if E:
            ref, Z = gr.reproject(*a, want_z=True)
            keep = np.broadcast_to((np.abs(Z) >= gr.Z_SKIP)[None, :, None], ref.shape)
            assert 1.0 - keep.mean() <= 0.02, "more than 2 %% of the elements within %g of Z = 0" % gr.Z_SKIP
            _pixel_row(tab, "reproject E %d" % E, out[:E].cpu().numpy()[None], ref, orc.reproject(*a), keep)
        # the point cloud of the first m = E patches, each with a frame (pose and intrinsics row) drawn at random
        m = E
        ix = np.random.default_rng(60 + E).integers(0, s["n_frames"], m).astype(np.int64)
        out = _canary((m + 1, 3))
        assert L.ramp_point_cloud(ptr(dev[0]), ptr(dev[1]), ptr(dev[2]), ptr(cu(ix)), ptr(out), m, 3, stream()) == 0
        assert (_words(out)[m] == CANARY).all()
        if m:
            K, c = s["intr"][ix], s["patches"][:m, :, 1, 1]
            X0 = np.stack([(c[:, 0] - K[:, 2]) / K[:, 0], (c[:, 1] - K[:, 3]) / K[:, 1], np.ones(m, np.float32), c[:, 2]], -1)
            Pw = orc.se3_act4(orc.se3_inv(s["poses"][ix]), X0.astype(np.float32))
            _pixel_row(tab, "point_cloud m %d" % m, out[:m].cpu().numpy(), gr.point_cloud(s["poses"], s["patches"], s["intr"], ix),
                       Pw[:, :3] / Pw[:, 3:])
    tab.show()
    assert not tab.failed(), tab.failed()


# ------------------------------------------------------------------------------------------------------ exact bookkeeping
GUARD = 4                                # canary words in front of and behind every region (16 bytes: keeps the alignment)
MIB = 1 << 20


def _random_words(rng, n):
    w = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    w[::97] = np.int32(0x7fc00001)                           # NaN patterns: a copy through a float register keeps them
    w[5::193] = np.array(0xffc12345, np.uint32).view(np.int32)
    return w


class _Region:
    """n4 words at (16-byte aligned + off words) inside a random-filled device array with guards on both sides"""

    def __init__(self, rng, n4, off=0):
        self.n4, self.lo = n4, GUARD + off
        self.host = _random_words(rng, GUARD + off + n4 + GUARD + 4)
        self.dev = cu(self.host)
        assert self.dev.data_ptr() % 16 == 0

    @property
    def addr(self):
        return self.dev.data_ptr() + 4 * self.lo

    def words(self):
        return self.host[self.lo:self.lo + self.n4]


def _multi_copy(srcs, dsts, nbytes):
    L, ptr, stream = _api()
    n = len(srcs)
    return L.ramp_multi_copy((ctypes.c_void_p * n)(*[s.addr for s in srcs]), (ctypes.c_void_p * n)(*[d.addr for d in dsts]),
                             (ctypes.c_long * n)(*nbytes), n, stream())


def test_multi_copy_bit_for_bit():
    """ten buffers of unequal size in one call: 0 .. 4100 bytes and 2 MiB + 16 / + 4 (past the 512-block cap: both loops
    stride), 16-byte aligned pairs (uint4 path) and pairs offset by 4 bytes (word path); every word outside a destination
    keeps its value"""
    rng = np.random.default_rng(70)
    spec = [(0, 0, 0), (4, 0, 0), (12, 0, 0), (16, 0, 0), (4100, 0, 0), (2 * MIB + 16, 0, 0), (2 * MIB + 4, 0, 0),
            (4112, 1, 0), (16, 0, 1), (2 * MIB + 16, 1, 1)]                     # (bytes, source offset, destination offset) in words
    srcs = [_Region(rng, b // 4, so) for b, so, _ in spec]
    dsts = [_Region(rng, b // 4, do) for b, _, do in spec]
    assert _multi_copy(srcs, dsts, [b for b, _, _ in spec]) == 0
    for s, d, sp in zip(srcs, dsts, spec):
        exp = d.host.copy()
        exp[d.lo:d.lo + d.n4] = s.words()
        assert np.array_equal(d.dev.cpu().numpy(), exp), sp
        assert np.array_equal(s.dev.cpu().numpy(), s.host), sp
    # refused whole: eleven buffers, a size that is no multiple of 4 -- nothing is written
    srcs = [_Region(rng, 4) for _ in range(11)]
    dsts = [_Region(rng, 4) for _ in range(11)]
    assert _multi_copy(srcs, dsts, [16] * 11) == EINVAL
    assert _multi_copy(srcs[:3], dsts[:3], [16, 6, 16]) == EINVAL
    torch.cuda.synchronize()
    for d in dsts:
        assert np.array_equal(d.dev.cpu().numpy(), d.host)


def test_store_rows_bit_for_bit():
    """ops.store_rows (ramp_multi_copy on rows of contiguous buffers): rows of 4, 12, 16 and 4100 bytes"""
    from rampvo_amd import ops
    rng = np.random.default_rng(71)
    widths, R = [1, 3, 4, 1025], 6
    srcs = [cu(_random_words(rng, w)) for w in widths]
    bufs = [cu(_random_words(rng, R * w).reshape(R, w)) for w in widths]
    before = [b.cpu().numpy().copy() for b in bufs]
    rows = [5, 0, 3, 2]
    ops.store_rows(srcs, list(zip(bufs, rows)))
    for s, b, b0, r in zip(srcs, bufs, before, rows):
        b0[r] = s.cpu().numpy()
        assert np.array_equal(b.cpu().numpy(), b0)


def test_shift_rows_bit_for_bit():
    """plain and ring buffers in one call, rows of 4, 12, 1028 bytes and 1 MiB + 4 bytes (past the 1024-block cap: the column
    loop strides); k = 0, the middle, nrows - 2; k >= nrows - 1 moves nothing; the ring's live rows wrap across its modulus;
    rows below k, rows from nrows on and the guards keep their words"""
    L, ptr, stream = _api()
    rng = np.random.default_rng(72)
    nrows, slots, mod = 11, 13, 5
    spec = [(1, 0), (3, 0), (257, mod), (MIB // 4 + 1, 0), (3, mod)]           # (row words, ring modulus)
    host = [_random_words(rng, GUARD + (m or slots) * w + GUARD) for w, m in spec]
    n = len(spec)
    for k in (0, 5, nrows - 2, nrows - 1, nrows + 3):
        dev = [cu(h) for h in host]
        base = (ctypes.c_void_p * n)(*[d.data_ptr() + 4 * GUARD for d in dev])
        rb = (ctypes.c_long * n)(*[4 * w for w, _ in spec])
        md = (ctypes.c_int * n)(*[m for _, m in spec])
        assert L.ramp_shift_rows(base, rb, md, n, k, nrows, stream()) == 0
        for (w, m), h, d in zip(spec, host, dev):
            exp = h.copy()
            body = exp[GUARD:len(exp) - GUARD].reshape(-1, w)
            body[:] = gr.shift_rows(body, k, nrows, m)
            assert np.array_equal(d.cpu().numpy(), exp), (k, w, m)
            if k >= nrows - 1:
                assert np.array_equal(exp, h)
    assert L.ramp_shift_rows(base, rb, md, 11, 0, nrows, stream()) == EINVAL


@pytest.mark.parametrize("F,M,P", [(1, 1, 1), (1, 5, 3), (3, 8, 3), (1, 2, 1), (4, 1024, 1), (1, 4097, 1), (1, 8192, 1)])
def test_depth_median_is_the_lower_median(F, M, P):
    """ramp_depth_median == torch.median (the lower of the two middle values) of the depth plane: odd and even counts, ties,
    F = 1, negative values; F M P P = 4096 and the library's capacity of 8192 values are accepted"""
    from rampvo_amd import ops
    rng = np.random.default_rng(F * 1000 + M)
    for ties in (False, True):
        x = rng.normal(size=(F, M, 3, P, P)).astype(np.float32)
        if ties:
            x = np.round(x * 2) / 2
        out = _canary((1,))
        ops.depth_median(cu(x), F, F, out)
        want = torch.median(torch.from_numpy(x[:, :, 2].copy()))
        assert float(out.item()) == float(want) == float(gr.lower_median(x[:, :, 2])), (F, M, P, ties)


def test_depth_median_refuses_what_it_cannot_hold():
    """one value past the capacity (8192): the library's refusal code, the output as it was"""
    L, ptr, stream = _api()
    x = cu(np.random.default_rng(80).normal(size=(1, 8193, 3, 1, 1)).astype(np.float32))
    out = _canary((1,))
    assert L.ramp_depth_median(ptr(x), 1, 8193, 1, ptr(out), stream()) == EUNSUPPORTED
    torch.cuda.synchronize()
    assert (_words(out) == CANARY).all()
