"""CPU tests of tests/georef.py: the float64 restatements agree with the fp32 oracle at fp32 level, the scenes of the GPU
test have the properties it relies on, and the checks have teeth -- every mutation a geometry or bookkeeping kernel could
plausibly carry is rejected by the bound the GPU test applies, while the fp32 oracle's own result passes it."""
import numpy as np
import torch

import georef as gr
import oracle as orc
from scenes import ba_scene


def _rel(a, b, keep=None):
    return gr.max_err(a, b, keep) / float(np.abs(gr.f64(b) if keep is None else gr.f64(b)[keep]).max())


def test_restatements_match_the_oracle_on_ba_scene():
    s = ba_scene(seed=2, n_frames=7, M=9)
    s["patches"][5, 2] = 1e-3
    s["poses"][3, :3] += [0, 0, 9]                       # some points behind the camera -> the clamp is taken
    a = (s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"])
    for tonly in (False, True):
        assert _rel(orc.transform(*a, tonly), gr.transform(*a, tonly)) < 1e-5
    ref, Z = gr.reproject(*a, want_z=True)
    keep = np.broadcast_to((np.abs(Z) >= gr.Z_SKIP)[None, :, None], ref.shape)
    assert keep.mean() > 0.98
    assert _rel(orc.reproject(*a), ref, keep) < 1e-5
    X = s["poses"]
    rng = np.random.default_rng(0)
    p, b = rng.normal(size=(len(X), 4)).astype(np.float32), rng.normal(size=(len(X), 6)).astype(np.float32)
    xi = orc.se3_log(X)
    assert gr.max_err(xi, orc.se3_log_f64(X)) < 5e-6
    assert gr.max_err(orc.se3_exp(xi), orc.se3_exp_f64(xi)) < 2e-6
    assert gr.max_err(orc.se3_inv(X), orc.se3_inv_f64(X)) < 2e-6 * 10
    assert gr.max_err(orc.se3_mul(X, X[::-1]), orc.se3_mul_f64(X, X[::-1])) < 2e-6 * 10
    assert gr.max_err(orc.se3_act4(X, p), orc.se3_act4_f64(X, p)) < 5e-6 * 10
    assert gr.max_err(orc.se3_adj(X, b), orc.se3_adj_f64(X, b)) < 1e-5 * 10
    assert gr.max_err(orc.se3_adjT(X, b), orc.se3_adjT_f64(X, b)) < 1e-5 * 10
    # point cloud: the statement of test_transform_reproject_point_cloud in fp32
    m = s["n_frames"] * s["M"]
    ix = np.repeat(np.arange(s["n_frames"]), s["M"]).astype(np.int64)
    K, c = s["intr"][ix], s["patches"][:m, :, 1, 1]
    X0 = np.stack([(c[:, 0] - K[:, 2]) / K[:, 0], (c[:, 1] - K[:, 3]) / K[:, 1], np.ones(m), c[:, 2]], -1)
    Pw = orc.se3_act4(orc.se3_inv(X[ix]), X0.astype(np.float32))
    assert _rel(Pw[:, :3] / Pw[:, 3:], gr.point_cloud(X, s["patches"][:m], s["intr"], ix)) < 1e-5
    # motion model: fp32 oracle against float64 at a benign inter-frame rotation
    assert gr.pose_err(gr.motion_model_f32(X, 6, 0.5), gr.motion_model(X, 6, 0.5)) < 2e-6 * 10


def test_geo_scene_has_the_properties_the_gpu_test_relies_on():
    s = gr.geo_scene(7, E=257)
    a = (s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"])
    K = s["intr"].astype(np.float64)
    spread = np.abs(K[:, None] - K[None]) / K[None]
    off = ~np.eye(len(K), dtype=bool)
    assert spread[off].min() > 1e-3 and (np.abs(K / K.mean(0) - 1).max(0) > 0.1).all()      # every row its own
    assert s["patches"][:, 2].min() < 1e-5
    _, Z = gr.transform(*a, want_z=True)
    back = s["jj"] < s["ii"]
    assert 0.05 < (Z[back] < 0).mean() < 0.35                                  # behind the target camera
    assert ((Z > 0.0) & (Z < gr.Z_CLAMP)).sum() >= 9 and ((Z >= gr.Z_CLAMP) & (Z < 0.2)).sum() >= 9   # both sides
    _, Zr = gr.reproject(*a, want_z=True)
    assert (np.abs(Zr) < gr.Z_SKIP).mean() <= 0.02
    # ... and for every scene of test_transform_reproject_point_cloud_against_float64 (seed 50 + E)
    for E in (1, 255, 256, 257):
        g = gr.geo_scene(50 + E, E=E)
        _, Zr = gr.reproject(g["poses"], g["patches"], g["intr"], g["ii"], g["jj"], g["kk"], want_z=True)
        assert (np.abs(Zr) < gr.Z_SKIP).mean() <= 0.02, E
    # the motion-test case: the tested keys sit where the docstring says, a tenth or more of j -> i behind the camera
    for (i, j), where in (((0, 2), "first"), ((5, 7), "last")):
        c = gr.mm_case(7, i, j, 257, 255)
        uk = np.unique(c["keys"])
        assert (uk[0] == c["key_ji"]) if where == "first" else (uk[-1] == c["key_ij"])
        assert (c["keys"] == c["key_ij"]).sum() == 257 and (c["keys"] == c["key_ji"]).sum() == 255
        sel = c["keys"] == c["key_ji"]
        _, Zm = gr.transform(c["poses"], c["patches"], c["intr"], c["ii"][sel], c["jj"][sel], c["kk"][sel], want_z=True)
        assert 0.1 <= (Zm < 0).mean() < 0.5     # (two frames back: the patches placed at the clamp are behind it too)


def _transform_mutant(s, tonly, swap_rows=False, clamp=True):
    """georef.transform's statement with one defect: the intrinsics rows of frames i and j exchanged, or no Z clamp"""
    poses, patches, intr = gr.f64(s["poses"]), gr.f64(s["patches"]), gr.f64(s["intr"])
    ii, jj, kk = s["ii"], s["jj"], s["kk"]
    G = orc.se3_mul_f64(poses[jj], orc.se3_inv_f64(poses[ii]))
    if tonly:
        G[:, 3:] = [0, 0, 0, 1]
    Ki, Kj = (intr[jj], intr[ii]) if swap_rows else (intr[ii], intr[jj])
    X1 = orc.se3_act4_f64(G[:, None, :], gr._unproject(patches[kk], Ki))
    return gr._project(X1, Kj, clamp).reshape(1, len(ii), 2, 3, 3)


def _pixel_check(out, ref, f32):
    """the GPU test's rule for pixel outputs -> (accepted, err, bound)"""
    floor = gr.PIXEL_FLOOR * float(np.abs(ref).max())
    b = gr.bound(floor, gr.max_err(f32, ref))
    e = gr.max_err(out, ref)
    return e <= b, e, b


def test_projective_checks_reject_exchanged_intrinsics_and_a_dropped_clamp():
    s = gr.geo_scene(7, E=257)
    a = (s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"])
    for tonly in (False, True):
        ref = gr.transform(*a, tonly)
        f32 = orc.transform(*a, tonly)
        assert _pixel_check(f32, ref, f32)[0]
        assert _pixel_check(ref.astype(np.float32), ref, f32)[0]
        assert np.array_equal(_transform_mutant(s, tonly), ref)                  # the mutant maker without a defect
        for name, kw in (("rows i and j exchanged", dict(swap_rows=True)), ("clamp dropped", dict(clamp=False))):
            ok, e, b = _pixel_check(_transform_mutant(s, tonly, **kw), ref, f32)
            print("transform tonly=%d mutant %-24s error %.2e, bound %.2e" % (tonly, name, e, b))
            assert not ok, name
    # the point cloud read with the intrinsics of a neighbouring frame
    m = s["n_frames"] * s["M"]
    ix = np.repeat(np.arange(s["n_frames"]), s["M"]).astype(np.int64)
    ref = gr.point_cloud(s["poses"], s["patches"], s["intr"], ix)
    wrong = gr.point_cloud(s["poses"], s["patches"], np.roll(s["intr"], 1, 0), ix)
    assert gr.max_err(wrong, ref) > 100 * gr.PIXEL_FLOOR * np.abs(ref).max()


def test_motionmag_check_rejects_a_lost_edge_of_a_257_edge_segment():
    c = gr.mm_case(7, 5, 7, 257, 257)
    a = (c["poses"], c["patches"], c["intr"], c["ii"], c["jj"], c["kk"], c["keys"])
    f32 = lambda *x: orc.transform(*x)
    for key in (c["key_ij"], c["key_ji"]):
        for beta in (0.0, 0.5, 1.0):
            ref = gr.motionmag(*a, key, beta)
            env = abs(gr.motionmag(*a, key, beta, xform=f32) - ref)
            sel = c["keys"] == key
            cmax = max(float(np.abs(gr.transform(c["poses"], c["patches"], c["intr"], c["ii"][sel], x, c["kk"][sel], t)).max())
                       for x, t in ((c["ii"][sel], False), (c["jj"][sel], False), (c["jj"][sel], True)))
            b = gr.bound(gr.PIXEL_FLOOR * cmax, env)
            assert env <= b
            # the edge a 256-stride loop reaches last
            f = gr.flow_mag(*a[:3], c["ii"][sel], c["jj"][sel], c["kk"][sel], beta)
            assert f.shape[0] == 257 and abs(f.sum() / f.size - ref) < 1e-12
            mut = (f.sum() - f[256].sum()) / f.size                     # ... and still divides by the full count
            print("motionmag key %d beta %.1f: mean %.4f, one edge lost %.2e, bound %.2e" % (key, beta, ref, abs(mut - ref), b))
            assert abs(mut - ref) > b
    assert np.isnan(gr.motionmag(*a, -1, 0.5)) and np.isnan(gr.motionmag(*a, 1 << 20, 0.5))


def test_shift_rows_rejects_a_ring_slot_off_by_one():
    rng = np.random.default_rng(3)
    buf = rng.integers(-2 ** 31, 2 ** 31, (8, 3), dtype=np.int64).astype(np.int32)
    # plain: rows 3.. move down, row nrows-1 keeps its old content, rows below k and past nrows untouched
    out = gr.shift_rows(buf, 2, 6)
    assert np.array_equal(out[:2], buf[:2]) and np.array_equal(out[2:5], buf[3:6]) and np.array_equal(out[5:], buf[5:])
    # ring of 5 slots holding rows 7 .. 10 (slots 2, 3, 4, 0): the live rows wrap across the modulus
    ring = buf[:5]
    out = gr.shift_rows(ring, 8, 11, mod=5)
    exp = ring.copy()
    exp[3], exp[4] = ring[4], ring[0]
    assert gr.same_bits(out, exp)
    assert np.array_equal(out[[1, 2]], ring[[1, 2]])                 # a slot outside the live range, and row 7 below k
    off = ring.copy()                                                # the same loop with every ring slot one too far
    for r in range(8, 10):
        off[(r + 1) % 5] = off[(r + 2) % 5]
    assert not gr.same_bits(off, exp)
    assert gr.same_bits(gr.shift_rows(ring, 10, 11, mod=5), ring)   # k = nrows - 1: nothing moves
    nan = np.array([[0x7fc00001, 0x7fc00002]], np.uint32).view(np.float32)
    assert gr.same_bits(nan, nan.copy()) and not gr.same_bits(nan, nan[:, ::-1])


def test_lower_median_is_torch_median_and_rejects_the_upper_one():
    rng = np.random.default_rng(4)
    for n in (1, 2, 9, 10, 4096):
        x = rng.normal(size=n).astype(np.float32)
        x[: n // 3] = -10.0                                          # ties (below the median: the two middle values differ)
        assert gr.lower_median(x) == float(torch.median(torch.from_numpy(x)))
        if n % 2 == 0:
            assert np.sort(x)[n // 2] != gr.lower_median(x)          # the upper median is another number
    tie = np.array([3.0, 1.0, 2.0, 2.0, 0.0, 5.0], np.float32)       # the two middle values tie: either median is 2
    assert gr.lower_median(tie) == 2.0 == float(torch.median(torch.from_numpy(tie)))
