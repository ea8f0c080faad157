"""GPU parity tests: every HIP operator (called through the C ABI) against the CPU
oracle on the same seeded inputs.  Tolerances are stated per test; integer /
index outputs must match exactly."""
import os
import numpy as np
import pytest
import torch

import oracle as orc
from scenes import BA_ORACLE_CASES, ba_oracle_case, ba_scene, corr_case
from trackerkit import cu

pytestmark = pytest.mark.gpu


def rel_err(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-12))


# ---------------------------------------------------------------------- lietorch
def test_se3_ops_match_oracle():
    from rampvo_amd import ops
    rng = np.random.default_rng(0)
    a = (0.4 * rng.normal(size=(257, 6))).astype(np.float32)
    a[0] = 0  # identity / small-angle branches
    a[1, 3:] = 1e-7
    X = orc.se3_exp(a)
    Xg = ops.se3_unary("ramp_se3_exp", cu(a), 6, 7).cpu().numpy()
    assert np.abs(Xg - X).max() < 2e-6
    Y = orc.se3_exp((0.3 * rng.normal(size=(257, 6))).astype(np.float32))
    p = rng.normal(size=(257, 4)).astype(np.float32)
    b = rng.normal(size=(257, 6)).astype(np.float32)
    assert np.abs(ops.se3_unary("ramp_se3_log", cu(X), 7, 6).cpu().numpy() - orc.se3_log(X)).max() < 5e-6
    assert np.abs(ops.se3_unary("ramp_se3_inv", cu(X), 7, 7).cpu().numpy() - orc.se3_inv(X)).max() < 2e-6
    assert np.abs(ops.se3_binary("ramp_se3_mul", cu(X), cu(Y), 7, 7, 7).cpu().numpy() - orc.se3_mul(X, Y)).max() < 2e-6
    assert np.abs(ops.se3_binary("ramp_se3_act4", cu(X), cu(p), 7, 4, 4).cpu().numpy() - orc.se3_act4(X, p)).max() < 5e-6
    assert np.abs(ops.se3_binary("ramp_se3_adj", cu(X), cu(b), 7, 6, 6).cpu().numpy() - orc.se3_adj(X, b)).max() < 1e-5
    assert np.abs(ops.se3_binary("ramp_se3_adjT", cu(X), cu(b), 7, 6, 6).cpu().numpy() - orc.se3_adjT(X, b)).max() < 1e-5


def test_se3_class_identities():
    """the identities of the reference's ramp/lietorch/run_tests.py:16-52 at fp32"""
    from rampvo_amd.lietorch import SE3
    g = torch.Generator().manual_seed(1)
    a = (0.2 * torch.randn(2, 3, 4, 6, generator=g)).cuda()
    X = SE3.exp(a)
    assert (X.log() - a).abs().max() < 1e-5
    assert (X * X.inv()).log().abs().max() < 1e-5
    c = torch.randn(2, 3, 4, 6, generator=g).cuda()
    Y1 = X * SE3.exp(c)
    Y2 = SE3.exp(X.adj(c)) * X
    assert (Y1 * Y2.inv()).log().abs().max() < 2e-5
    Xs = SE3.exp(torch.randn(1, 6, generator=g).cuda())
    p = torch.randn(1, 3, generator=g).cuda()
    p1 = Xs.act(p)
    ph = torch.cat([p, torch.ones_like(p[..., :1])], -1)
    p2 = torch.matmul(Xs.matrix(), ph[..., None])[..., 0]
    assert (p1 - p2[..., :3]).abs().max() < 1e-5


# ----------------------------------------------------------------------- altcorr
@pytest.mark.parametrize("C,R,HW", [(128, 1, (30, 40)), (384, 0, (30, 40)), (3, 1, (30, 40)), (3, 0, (120, 160))])
@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_patchify_matches_oracle(C, R, HW, layout):
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NCHW, RAMP_NHWC
    rng = np.random.default_rng(C + R)
    H, W = HW
    M = 37
    net = rng.normal(size=(2, C, H, W)).astype(np.float32)
    coords = np.stack([rng.uniform(-3, W + 3, (2, M)), rng.uniform(-3, H + 3, (2, M))], -1).astype(np.float32)
    coords[0, 0] = [0.0, 0.0]
    coords[0, 1] = [W - 1, H - 1]
    coords[0, 2] = [5.0, 7.0]  # integral coordinates: dx = dy = 0
    ref = orc.patchify(net, coords, R)
    raw = orc.patchify_raw(net, coords, R)
    if layout == "nchw":
        out = ops.patchify(cu(net), cu(coords), R, True, RAMP_NCHW, RAMP_NCHW).cpu().numpy()
        outr = ops.patchify(cu(net), cu(coords), R, False, RAMP_NCHW, RAMP_NCHW).cpu().numpy()
    else:
        nh = cu(net.transpose(0, 2, 3, 1))
        out = ops.patchify(nh, cu(coords), R, True, RAMP_NHWC, RAMP_NHWC).permute(0, 1, 4, 2, 3).cpu().numpy()
        outr = ops.patchify(nh, cu(coords), R, False, RAMP_NHWC, RAMP_NCHW).cpu().numpy()
    assert np.array_equal(outr, raw)            # a gather: bit exact
    assert np.abs(out - ref).max() <= 1e-6     # same expression order; fp32 rounding only


@pytest.mark.parametrize("layout", ["nchw", "nhwc"])
def test_corr_matches_oracle(layout):
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NCHW, RAMP_NHWC
    fmap1, fmap2, coords, ii, jj = corr_case(seed=3)
    fmap2b = np.ascontiguousarray(fmap2[:, :, :, ::2, ::2])  # a second, coarser level
    ref0 = orc.corr(fmap1, fmap2, coords / 1, ii, jj, 3)[0]
    ref1 = orc.corr(fmap1, fmap2b, coords / 4, ii, jj, 3)[0]
    if layout == "nchw":
        out = ops.corr(cu(fmap1[0]), [cu(fmap2[0]), cu(fmap2b[0])], cu(coords[0]), cu(ii), cu(jj), 3,
                       (1.0, 4.0), RAMP_NCHW)
    else:
        out = ops.corr(cu(fmap1[0].transpose(0, 2, 3, 1)),
                       [cu(fmap2[0].transpose(0, 2, 3, 1)), cu(fmap2b[0].transpose(0, 2, 3, 1))],
                       cu(coords[0]), cu(ii), cu(jj), 3, (1.0, 4.0), RAMP_NHWC)
    out = out.cpu().numpy()
    assert out.shape == (coords.shape[1], 7, 7, 3, 3, 2)
    # dots are the same channel-ordered fmaf chain, the blend the same expression
    for lvl, ref in ((0, ref0), (1, ref1)):
        diff = np.abs(out[..., lvl] - ref)
        assert np.nanmax(diff) <= 1e-5, (lvl, np.nanmax(diff))
        assert np.array_equal(np.isnan(out[..., lvl]), np.isnan(ref))


def test_corr_f32_mfma_variant_matches_oracle():
    """opt-in fp32 MFMA kernel (RAMP_CORR_MFMA32): same values as the oracle to 1e-5 (its accumulation order
    is the MFMA's; the default fp32 kernel keeps the reference's order)"""
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC
    fmap1, fmap2, coords, ii, jj = corr_case(seed=3)
    fmap2b = np.ascontiguousarray(fmap2[:, :, :, ::2, ::2])
    ref0 = orc.corr(fmap1, fmap2, coords / 1, ii, jj, 3)[0]
    ref1 = orc.corr(fmap1, fmap2b, coords / 4, ii, jj, 3)[0]
    args = (cu(fmap1[0].transpose(0, 2, 3, 1)), [cu(fmap2[0].transpose(0, 2, 3, 1)), cu(fmap2b[0].transpose(0, 2, 3, 1))],
            cu(coords[0]), cu(ii), cu(jj), 3, (1.0, 4.0), RAMP_NHWC)
    out = ops.corr(*args, fast_f32=True).cpu().numpy()
    for lvl, ref in ((0, ref0), (1, ref1)):
        assert np.array_equal(np.isnan(out[..., lvl]), np.isnan(ref))
        assert np.nanmax(np.abs(out[..., lvl] - ref)) <= 1e-5 * max(1.0, np.nanmax(np.abs(ref)))
    base = ops.corr(*args, fast_f32=False).cpu().numpy()
    assert np.nanmax(np.abs(base - out)) <= 1e-5 * max(1.0, np.nanmax(np.abs(ref0)))


def test_corr_reference_signature_and_half():
    from rampvo_amd import altcorr
    fmap1, fmap2, coords, ii, jj = corr_case(seed=5, E=32, distort=False)
    ref = orc.corr(fmap1, fmap2, coords, ii, jj, 3)
    out = altcorr.corr(cu(fmap1), cu(fmap2), cu(coords), cu(ii), cu(jj), 3)
    assert out.shape == ref.shape
    assert np.nanmax(np.abs(out.cpu().numpy() - ref)) <= 1e-5
    # fp16 storage, fp32 accumulation (the reference accumulates in half: looser tolerance)
    outh = altcorr.corr(cu(fmap1).half(), cu(fmap2).half(), cu(coords), cu(ii), cu(jj), 3)
    assert outh.dtype == torch.float16
    refh = orc.corr(fmap1.astype(np.float16).astype(np.float32), fmap2.astype(np.float16).astype(np.float32),
                    coords, ii, jj, 3)
    ok = np.isfinite(refh)
    assert np.abs(outh.float().cpu().numpy()[ok] - refh[ok]).max() <= 2e-2 * np.abs(refh[ok]).max()


@pytest.mark.parametrize("wide", [False, True])
def test_corr_half_mfma_path_matches_oracle(wide):
    """fp16 channels-last features -> v_mfma_f32_16x16x32_f16 kernel (fp32 accumulation; the reference
    accumulates in half, so the oracle on fp16-rounded inputs is the tighter target): only the final
    rounding of the output to half separates the two.  wide: a third of the patches projected 1.7-2.4 px apart --
    union windows of 130-190 pixels, the upper range of the kernel's single-pass path"""
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC
    fmap1, fmap2, coords, ii, jj = corr_case(seed=8, E=64, wide=wide)
    if wide:
        fx = np.floor(coords[0, :, 0]).reshape(64, 9); fy = np.floor(coords[0, :, 1]).reshape(64, 9)
        area = (fx.max(1) - fx.min(1) + 8) * (fy.max(1) - fy.min(1) + 8)
        assert ((area > 128) & (area <= 192)).sum() >= 10
    fmap2b = np.ascontiguousarray(fmap2[:, :, :, ::2, ::2])
    h = lambda a: a.astype(np.float16).astype(np.float32)
    ref0 = orc.corr(h(fmap1), h(fmap2), coords / 1, ii, jj, 3)[0]
    ref1 = orc.corr(h(fmap1), h(fmap2b), coords / 4, ii, jj, 3)[0]
    out = ops.corr(cu(fmap1[0].transpose(0, 2, 3, 1)).half(),
                   [cu(fmap2[0].transpose(0, 2, 3, 1)).half(), cu(fmap2b[0].transpose(0, 2, 3, 1)).half()],
                   cu(coords[0]), cu(ii), cu(jj), 3, (1.0, 4.0), RAMP_NHWC)
    assert out.dtype == torch.float16
    out = out.float().cpu().numpy()
    for lvl, ref in ((0, ref0), (1, ref1)):
        ok = np.isfinite(ref)
        assert np.array_equal(np.isnan(out[..., lvl]), np.isnan(ref))
        assert np.abs(out[..., lvl][ok] - ref[ok]).max() <= 1.5e-3 * np.abs(ref[ok]).max()


@pytest.mark.parametrize("half", [False, True])
def test_corr_schedule_does_not_change_values(half):
    """ramp_corr_fwd_ordered: any edge permutation as the XCD schedule (E not a multiple of 8, so the
    padded tail of the grid is exercised) gives bit-identical output"""
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC
    fmap1, fmap2, coords, ii, jj = corr_case(seed=11, E=61)
    fmap2b = np.ascontiguousarray(fmap2[:, :, :, ::2, ::2])
    t = (lambda a: cu(a).half()) if half else cu
    args = (t(fmap1[0].transpose(0, 2, 3, 1)), [t(fmap2[0].transpose(0, 2, 3, 1)), t(fmap2b[0].transpose(0, 2, 3, 1))],
            cu(coords[0]), cu(ii), cu(jj), 3, (1.0, 4.0), RAMP_NHWC)
    base = ops.corr(*args)
    perm = torch.from_numpy(np.random.default_rng(0).permutation(61).astype(np.int32)).cuda()
    byjj = torch.argsort(cu(jj), stable=True).int()
    for order in (perm, byjj):
        out = ops.corr(*args, order=order)
        assert torch.equal(torch.nan_to_num(out.float(), nan=-7.0), torch.nan_to_num(base.float(), nan=-7.0))
    # padded rows (882 -> 896): same values, zero tail
    pad = ops.corr(*args, order=byjj, row_elems=896)
    assert pad.shape == (61, 896) and float(pad[:, 882:].abs().max()) == 0.0
    assert torch.equal(torch.nan_to_num(pad[:, :882].float(), nan=-7.0),
                       torch.nan_to_num(base.reshape(61, 882).float(), nan=-7.0))


def test_pyramid_pack_and_chunked_corr():
    """ramp_pyramid_pack: level 1 is a pure re-layout, level 4 the 4x4 mean (Ramp_vo.py:378-381);
    the MFMA correlation over the chunked maps is bit-identical to the NHWC one"""
    import torch.nn.functional as F
    from rampvo_amd import ops
    from rampvo_amd._lib import KPLANE, RAMP_NHWC, RAMP_NHWC32
    g = torch.Generator().manual_seed(5)
    N2, H, W, C = 3, 24, 32, 128
    maps = (torch.randn(N2, H, W, C, generator=g) * 0.5).half().cuda()
    l1 = torch.empty(N2, H, C // KPLANE, W, KPLANE, dtype=torch.half, device="cuda")
    l4 = torch.empty(N2, H // 4, C // KPLANE, W // 4, KPLANE, dtype=torch.half, device="cuda")
    for n in range(N2):
        ops.pyramid_pack(maps[n], l1[n], l4[n])
    unchunk = lambda t: t.permute(0, 1, 3, 2, 4).reshape(t.shape[0], t.shape[1], t.shape[3], C)
    assert torch.equal(unchunk(l1), maps)
    pooled = F.avg_pool2d(maps.float().permute(0, 3, 1, 2), 4, 4).permute(0, 2, 3, 1)
    got = unchunk(l4).float()
    assert (got - pooled).abs().max() <= 2.0 ** -11 * pooled.abs().max() * 1.01       # one fp16 rounding
    # correlation: same edges over both layouts
    rng = np.random.default_rng(4)
    E, M = 61, 12
    fmap1 = (torch.randn(M, 3, 3, C, generator=g) * 0.5).half().cuda()
    coords = np.stack([rng.uniform(-6, W + 6, (E, 3, 3)), rng.uniform(-6, H + 6, (E, 3, 3))], 1).astype(np.float32)
    coords[:20] = coords[:20, :, :1, :1] + np.arange(3, dtype=np.float32)[None, None, None, :]   # compact windows
    ii = torch.from_numpy(rng.integers(0, M, E)).cuda()
    jj = torch.from_numpy(rng.integers(0, N2, E)).cuda()
    pooled_h = unchunk(l4).contiguous()
    a = ops.corr(fmap1, [maps, pooled_h], cu(coords), ii, jj, 3, (1.0, 4.0), RAMP_NHWC)
    b = ops.corr(fmap1, [l1, l4], cu(coords), ii, jj, 3, (1.0, 4.0), RAMP_NHWC32)
    assert torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))
    assert a.float().abs().max() > 0


def test_pyramid_pack_fp32_and_chunked_fp32_corr():
    """fp32 features (round 6): ramp_pyramid_pack -> [H][8][W][16] planes, level 1 a pure re-layout, level 4 torch's
    avg_pool2d TO THE BIT ((ky, kx)-ordered sum x 1/16); corr_mfma_kernel<float> over the chunked planes is bit-identical to
    the same kernel over plain NHWC planes (the layout changes which bytes a load fetches together, never a value)"""
    import torch.nn.functional as F
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC, RAMP_NHWC32, kplane
    g = torch.Generator().manual_seed(6)
    N2, H, W, C = 3, 24, 32, 128
    kp = kplane(torch.float32)
    assert kp == 16
    maps = (torch.randn(N2, H, W, C, generator=g) * 0.5).cuda()
    l1 = torch.empty(N2, H, C // kp, W, kp, device="cuda")
    l4 = torch.empty(N2, H // 4, C // kp, W // 4, kp, device="cuda")
    for n in range(N2):
        ops.pyramid_pack(maps[n], l1[n], l4[n], split=False)
    unchunk = lambda t: t.permute(0, 1, 3, 2, 4).reshape(t.shape[0], t.shape[1], t.shape[3], C)
    assert torch.equal(unchunk(l1), maps)
    pooled = F.avg_pool2d(maps.permute(0, 3, 1, 2), 4, 4).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(unchunk(l4), pooled)
    rng = np.random.default_rng(4)
    E, M = 61, 12
    fmap1 = (torch.randn(M, 3, 3, C, generator=g) * 0.5).cuda()
    coords = np.stack([rng.uniform(-6, W + 6, (E, 3, 3)), rng.uniform(-6, H + 6, (E, 3, 3))], 1).astype(np.float32)
    coords[:20] = coords[:20, :, :1, :1] + np.arange(3, dtype=np.float32)[None, None, None, :]   # compact windows
    ii = torch.from_numpy(rng.integers(0, M, E)).cuda()
    jj = torch.from_numpy(rng.integers(0, N2, E)).cuda()
    a = ops.corr(fmap1, [maps, pooled], cu(coords), ii, jj, 3, (1.0, 4.0), RAMP_NHWC, fast_f32=True)
    b = ops.corr(fmap1, [l1, l4], cu(coords), ii, jj, 3, (1.0, 4.0), RAMP_NHWC32, fast_f32=True)
    assert torch.equal(torch.nan_to_num(a, nan=-7.0), torch.nan_to_num(b, nan=-7.0))
    ref = ops.corr(fmap1, [maps, pooled], cu(coords), ii, jj, 3, (1.0, 4.0), RAMP_NHWC, fast_f32=False)   # the fmaf chain
    assert (torch.nan_to_num(b) - torch.nan_to_num(ref)).abs().max() <= 1e-5 * max(1.0, float(torch.nan_to_num(ref).abs().max()))
    assert a.abs().max() > 0


def test_pyramid_pack_split_and_x2_corr_against_oracle():
    """fp32 features as split fp16 pairs (round 6, RAMP_CORR_X2; the tracker's default for MIXED_PRECISION off): the pack
    kernel writes exactly ops.pack_split's pairs (level 1 of the map, level 4 of torch's avg_pool2d), hi + lo 2^-11 is the
    value to 2^-22; corr_mfma_kernel<CorrX2> -- three f16 MFMA products per dot product -- agrees with the C oracle (the
    reference kernel's fmaf chain) and with corr_kernel<float> to 1e-5 of the volume's scale, as close as the fp32 MFMA
    kernel does (both errors printed), NaN pattern included; tiny, huge-ish and zero features included"""
    import torch.nn.functional as F
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC, RAMP_NHWC32
    fmap1, fmap2, coords, ii, jj = corr_case(seed=11, E=96, N2=5, H=32, W=48, wide=True)
    fmap2[0, 0, :, :4, :4] *= 1e-5                  # below the fp16 normal range: carried by the low parts
    fmap2[0, 1, :, 8:12, 8:12] *= 200.0
    fmap2[0, 2, :64, 16:20] = 0.0
    fmap1[0, :4] *= 3e-5
    maps = cu(np.ascontiguousarray(fmap2[0].transpose(0, 2, 3, 1)))                   # [N2, H, W, C]
    N2, H, W, C = maps.shape
    l1 = torch.empty(N2, H, 8, W, 16, device="cuda")
    l4 = torch.empty(N2, H // 4, 8, W // 4, 16, device="cuda")
    for n in range(N2):
        ops.pyramid_pack(maps[n], l1[n], l4[n], split=True)
    pooled = F.avg_pool2d(maps.permute(0, 3, 1, 2), 4, 4).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(l1.view(torch.int32), ops.pack_split(maps).view(torch.int32))
    assert torch.equal(l4.view(torch.int32), ops.pack_split(pooled).view(torch.int32))
    hi, lo = ops.unpack_split(l1)
    back = hi.double() + lo.double() * 2.0 ** -11
    assert float((back - maps.double()).abs().max() / maps.abs().max()) <= 2.0 ** -22
    # (below the fp16 normal range, 6.1e-5, a value is carried by its low part alone: 11 bits, <= 1.5e-8 absolute)
    assert float(((back - maps.double()).abs() - maps.double().abs() * 2.0 ** -22).max()) <= 1.5e-8
    f1 = cu(np.ascontiguousarray(fmap1[0].transpose(0, 2, 3, 1)))
    args = (cu(coords[0]), cu(ii), cu(jj), 3, (1.0, 4.0))
    x2 = ops.corr(f1, [l1, l4], *args, RAMP_NHWC32, fast_f32=2).cpu().numpy()
    chain = ops.corr(f1, [maps, pooled], *args, RAMP_NHWC, fast_f32=False).cpu().numpy()
    mf = ops.corr(f1, [maps, pooled], *args, RAMP_NHWC, fast_f32=True).cpu().numpy()
    pooled_nchw = pooled.permute(0, 3, 1, 2).cpu().numpy()[None]
    ref0 = orc.corr(fmap1, fmap2, coords / 1, ii, jj, 3)[0]
    ref1 = orc.corr(fmap1, pooled_nchw, coords / 4, ii, jj, 3)[0]
    assert x2.shape == (coords.shape[1], 7, 7, 3, 3, 2)
    for lvl, ref in ((0, ref0), (1, ref1)):
        scale = max(1.0, float(np.nanmax(np.abs(ref))))
        assert np.array_equal(np.isnan(x2[..., lvl]), np.isnan(ref))
        e_x2 = float(np.nanmax(np.abs(x2[..., lvl] - ref))) / scale
        e_mf = float(np.nanmax(np.abs(mf[..., lvl] - ref))) / scale
        print("level %d: x2 %.2e, fp32 MFMA %.2e of the scale %.1f from the oracle's fmaf chain" % (lvl, e_x2, e_mf, scale))
        assert e_x2 <= 1e-5, (lvl, e_x2)
    assert np.nanmax(np.abs(x2 - chain)) <= 1e-5 * max(1.0, float(np.nanmax(np.abs(chain))))
    assert np.nanmax(np.abs(x2)) > 0
    # padded rows + ring-buffer slots + a schedule, as the tracker calls it
    order = torch.argsort(cu(jj), stable=True).int()
    padded = ops.corr(f1, [l1, l4], *args, RAMP_NHWC32, fast_f32=2, order=order, row_elems=896)
    assert padded.shape == (coords.shape[1], 896) and float(padded[:, 882:].abs().max()) == 0.0
    assert torch.equal(torch.nan_to_num(padded[:, :882], nan=-7.0),
                       torch.nan_to_num(torch.from_numpy(x2).cuda().reshape(-1, 882), nan=-7.0))


@pytest.mark.parametrize("mode", ["f16", "x2", "f32"])
def test_correlation_at_the_benchmark_size_by_properties(mode):
    """The tracker's correlation launch at BASELINE configs[1]'s OWN size -- 40,000 factors, 36 ring slots of 120 x 160 x 128
    planes (+ the 4x4-mean level), 3 x 36 x 96 patch rows, padded output rows, ring-buffer modulo, a target-frame-major
    schedule -- where the oracle cannot follow factor by factor in seconds, through what does not depend on the size:
      * a random sample of 320 factors against the C oracle's restatement of the reference kernel (both levels);
      * the schedule (none, target-frame major, a random permutation) changes no bit;
      * features scaled by a power of two scale the volume by exactly that power (fp32 paths and the fp16 path's normal range);
      * permuting the factors permutes the rows; factors that see nothing of either plane give zero rows.
    mode: the three instantiations the tracker launches -- fp16 features (the shipped precision), fp32 features as two fp16
    parts (`x2`, the fp32 default), fp32 features on the fp32 matrix cores."""
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC32
    rng = np.random.default_rng(17)
    g = torch.Generator(device="cuda").manual_seed(17)
    E, M, slots, H, W = 40000, 96, 36, 120, 160
    f1 = torch.randn(3 * slots * M, 3, 3, 128, generator=g, device="cuda") * 0.5
    maps = torch.randn(slots, H, W, 128, generator=g, device="cuda") * 0.5
    # (no feature within a factor 64 of the fp16 normal-range limit: below it an operand changes class -- fp16 subnormal, or
    # the split's "low part only" rule -- and a scaled copy would not be the same operand scaled)
    keep = lambda t: torch.where(t.abs() < 2.0 ** -8, torch.full_like(t, 2.0 ** -8).copysign(t), t)
    f1, maps = keep(f1), keep(maps)
    jj = np.sort(rng.integers(100, 100 + 31, E)).astype(np.int64)
    kk = rng.integers(0, 9 * slots * M, E).astype(np.int64)                    # (taken modulo 3 slots M inside the kernel)
    cx, cy = rng.uniform(-4, W + 4, E), rng.uniform(-4, H + 4, E)
    sc = rng.choice([0.8, 1.0, 1.2, 1.45, 1.9, 6.0], E, p=[0.05, 0.53, 0.28, 0.10, 0.02, 0.02])
    d = np.arange(-1, 2, dtype=np.float64)
    x = cx[:, None, None] + sc[:, None, None] * d[None, None, :] + rng.normal(0, 0.05, (E, 3, 3))
    y = cy[:, None, None] + sc[:, None, None] * d[None, :, None] + rng.normal(0, 0.05, (E, 3, 3))
    coords_np = np.stack([x, y], 1).astype(np.float32)
    far = rng.random(E) < 0.3
    coords_np[far] += 5000.0                                                 # nothing in either plane
    coords = cu(coords_np)
    kkc, jjc = cu(kk), cu(jj)
    if mode == "f16":
        f1m, mm = f1.half(), maps.half()
    else:
        f1m, mm = f1, maps
    l1 = torch.empty(slots, H, 128 // (32 if mode == "f16" else 16), W, 32 if mode == "f16" else 16, dtype=mm.dtype, device="cuda")
    l4 = torch.empty(slots, H // 4, l1.shape[2], W // 4, l1.shape[4], dtype=mm.dtype, device="cuda")
    for n in range(slots):
        ops.pyramid_pack(mm[n], l1[n], l4[n], split=(mode == "x2"))
    fast = {"f16": None, "x2": 2, "f32": 1}[mode]
    kw = dict(row_elems=896, mod_ii=3 * slots * M, mod_jj=slots, fast_f32=fast)
    run = lambda a=f1m, c=coords, i=kkc, j=jjc, **k: ops.corr(a, [l1, l4], c, i, j, 3, (1.0, 4.0), RAMP_NHWC32, **dict(kw, **k))
    byjj = torch.argsort(jjc, stable=True).int()
    base = run(order=byjj)
    assert base.shape == (E, 896) and float(base[:, 882:].abs().max()) == 0.0
    same = lambda a, b: torch.equal(torch.nan_to_num(a.float(), nan=-7.0), torch.nan_to_num(b.float(), nan=-7.0))
    # --- schedule
    perm = torch.from_numpy(rng.permutation(E).astype(np.int32)).cuda()
    assert same(run(), base) and same(run(order=perm), base)
    # --- dead factors
    assert float(base[cu(far)].abs().max()) == 0.0 and float(base[cu(~far)].abs().max()) > 0
    # --- permuting the factors permutes the rows
    p2 = torch.from_numpy(rng.permutation(E)).cuda()
    assert same(run(c=coords[p2], i=kkc[p2], j=jjc[p2]), base[p2])
    # --- scaling by powers of two (the split of the x2 path and every rounding commute with it; fp16 outputs: normal range)
    for s_ in (4.0, 0.25):
        scaled = run(a=f1m * s_, order=byjj).float()
        want = base.float() * s_
        if mode == "f16":
            ok = (want.abs() >= 2.0 ** -12) & (want.abs() < 3.0e4) | (want == 0)
            assert torch.equal(scaled[ok], want[ok]) and float(ok.float().mean()) > 0.9
        else:
            assert torch.equal(scaled, want)
    # --- a sample against the oracle (the pooled level restated with torch's avg_pool2d, checked to the bit elsewhere)
    import torch.nn.functional as F
    pick = np.sort(rng.choice(np.nonzero(~far)[0], 320, replace=False))
    used = np.unique(jj[pick] % slots)
    remap = {int(u): k for k, u in enumerate(used)}
    m_used = mm[torch.from_numpy(used).cuda()].float()
    fm2 = m_used.permute(0, 3, 1, 2).contiguous()
    fm4 = F.avg_pool2d(fm2, 4, 4) if mode != "f16" else F.avg_pool2d(fm2, 4, 4).half().float()
    rows = (kk[pick] % (3 * slots * M)).astype(np.int64)
    f1s = f1m[torch.from_numpy(rows).cuda()].float().permute(0, 3, 1, 2).contiguous().cpu().numpy()[None]
    ii_s = np.arange(320, dtype=np.int64)
    jj_s = np.array([remap[int(v % slots)] for v in jj[pick]], dtype=np.int64)
    c_s = coords_np[pick][None]
    ref0 = orc.corr(f1s, fm2.cpu().numpy()[None], c_s, ii_s, jj_s, 3)[0]
    ref1 = orc.corr(f1s, fm4.cpu().numpy()[None], c_s / 4, ii_s, jj_s, 3)[0]
    got = base[torch.from_numpy(pick).cuda(), :882].float().cpu().numpy().reshape(320, 7, 7, 3, 3, 2)
    tol = 1.5e-3 if mode == "f16" else 1e-5
    for lvl, ref in ((0, ref0), (1, ref1)):
        assert np.array_equal(np.isnan(got[..., lvl]), np.isnan(ref))
        err = float(np.nanmax(np.abs(got[..., lvl] - ref))) / max(1.0, float(np.nanmax(np.abs(ref))))
        print("%s level %d: %.2e of the scale from the oracle on 320 sampled factors" % (mode, lvl, err))
        assert err <= tol, (mode, lvl, err)


def test_corr_matches_reference_call_site_golden():
    """G3 (tests/golden/corr.npz): what the reference's altcorr.corr python call site returned for both pyramid
    levels, stacked as Ramp_vo.corr stacks them (ramp/Ramp_vo.py:175-182)"""
    import pipeline_checks as pc
    from rampvo_amd import altcorr
    from rampvo_amd._lib import RAMP_NCHW
    g = pc.gold("corr.npz")
    f1, f2, coords, ii, jj = corr_case(seed=int(g["seed"]), E=int(g["E"]))
    f2b = g["fmap2_l1"].astype(np.float32)
    out = altcorr.corr_pyramid(cu(f1[0]), [cu(f2[0]), cu(f2b[0])], cu(coords[0]), cu(ii), cu(jj), 3, (1, 4), RAMP_NCHW)
    out = out.cpu().numpy()
    assert out.shape == g["out"].shape
    assert np.array_equal(np.isnan(out), np.isnan(g["out"]))
    assert np.nanmax(np.abs(out - g["out"])) <= 1e-5


@pytest.mark.parametrize("half", [False, True])
def test_corr_ring_buffer_modulo_matches_oracle_on_wrapped_indices(half):
    """Ramp_vo.corr's ring-buffer aliasing (reference Ramp_vo.py:178-179: ``ii % (M*mem)``, ``jj % mem``) is taken
    INSIDE the kernel (mod_ii / mod_jj of ramp_corr_fwd_ordered): edge indices beyond the buffers (kk up to 3x the
    patch slots, jj up to 3x the frame slots, as after > mem keyframes under precise.yaml) must read the wrapped
    slot -- compared with the oracle on pre-wrapped indices, fp32 (<= 1e-5) and the fp16 MFMA kernel
    (oracle on fp16-rounded inputs), plain and target-frame-major schedule, both output row formats"""
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC
    N1, N2, E = 40, 6, 93
    fmap1, fmap2, coords, ii, jj = corr_case(seed=21, E=E, N1=N1, N2=N2)
    rng = np.random.default_rng(5)
    ii_raw = (ii + N1 * rng.integers(0, 3, E)).astype(np.int64)
    jj_raw = (jj + N2 * rng.integers(0, 3, E)).astype(np.int64)
    assert ii_raw.max() >= N1 and jj_raw.max() >= N2 and np.array_equal(ii_raw % N1, ii)
    fmap2b = np.ascontiguousarray(fmap2[:, :, :, ::2, ::2])
    h = (lambda a: a.astype(np.float16).astype(np.float32)) if half else (lambda a: a)
    ref = np.stack([orc.corr(h(fmap1), h(fmap2), coords / 1, ii, jj, 3)[0],
                    orc.corr(h(fmap1), h(fmap2b), coords / 4, ii, jj, 3)[0]], -1)
    t = (lambda a: cu(a).half()) if half else cu
    args = (t(fmap1[0].transpose(0, 2, 3, 1)), [t(fmap2[0].transpose(0, 2, 3, 1)), t(fmap2b[0].transpose(0, 2, 3, 1))],
            cu(coords[0]), cu(ii_raw), cu(jj_raw), 3, (1.0, 4.0), RAMP_NHWC)
    byjj = torch.argsort(cu(jj_raw), stable=True).int()
    tol = 1.5e-3 * np.nanmax(np.abs(ref)) if half else 1e-5
    wrapped = ops.corr(*args[:3], cu(ii), cu(jj), *args[5:])           # the same edges, indices wrapped by the caller
    for order, row in ((None, 0), (byjj, 0), (byjj, 896)):
        out = ops.corr(*args, order=order, row_elems=row, mod_ii=N1, mod_jj=N2)
        if row:
            assert float(out[:, 882:].abs().max()) == 0.0
            out = out[:, :882]
        assert torch.equal(torch.nan_to_num(out.reshape(E, -1).float(), nan=-7.0),
                           torch.nan_to_num(wrapped.reshape(E, -1).float(), nan=-7.0))
        o = out.reshape(ref.shape).float().cpu().numpy()
        assert np.array_equal(np.isnan(o), np.isnan(ref))
        assert np.nanmax(np.abs(o - ref)) <= tol


# ---------------------------------------------------------------- projective ops
def test_transform_reproject_point_cloud():
    from rampvo_amd import ops
    s = ba_scene(seed=2, n_frames=7, M=9)
    s["patches"][5, 2] = 1e-3      # far point
    s["poses"][3, :3] += [0, 0, 9]  # pushes some points behind the camera -> Z clamp
    for tonly in (False, True):
        ref = orc.transform(s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"], tonly)
        out = ops.transform(cu(s["poses"]), cu(s["patches"]), cu(s["intr"]), cu(s["ii"]), cu(s["jj"]),
                            cu(s["kk"]), tonly).cpu().numpy()
        assert rel_err(out, ref) < 1e-5
    ref = orc.reproject(s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"])
    out = ops.reproject(cu(s["poses"]), cu(s["patches"]), cu(s["intr"]), cu(s["ii"]), cu(s["jj"]),
                        cu(s["kk"])).cpu().numpy()
    fin = np.isfinite(ref) & (np.abs(ref) < 1e6)
    assert np.abs(out[fin] - ref[fin]).max() / np.abs(ref[fin]).max() < 1e-5
    m = s["n_frames"] * s["M"]
    ix = np.repeat(np.arange(s["n_frames"]), s["M"]).astype(np.int64)
    Tinv = orc.se3_inv(s["poses"][ix])
    K = s["intr"][ix]
    c = s["patches"][:m, :, 1, 1]
    X0 = np.stack([(c[:, 0] - K[:, 2]) / K[:, 0], (c[:, 1] - K[:, 3]) / K[:, 1], np.ones(m), c[:, 2]], -1)
    Pw = orc.se3_act4(Tinv, X0.astype(np.float32))
    refpc = Pw[:, :3] / Pw[:, 3:]
    out = ops.point_cloud(cu(s["poses"]), cu(s["patches"][:m]), cu(s["intr"]), cu(ix)).cpu().numpy()
    assert rel_err(out, refpc) < 1e-5


# ------------------------------------------------------------------------- graph
def test_group_by_and_neighbors_exact():
    from rampvo_amd import ops
    rng = np.random.default_rng(4)
    E = 5000
    kk = rng.integers(0, 300, E).astype(np.int64)
    jj = rng.integers(0, 40, E).astype(np.int64)
    for bound in (0, 300):
        g = ops.group_by(cu(kk), bound)
        G = int(g.ngroups.item())
        uk, inv = np.unique(kk, return_inverse=True)
        assert G == len(uk)
        assert np.array_equal(g.ukeys[:G].cpu().numpy(), uk)
        assert np.array_equal(g.gid[:E].cpu().numpy(), inv)
        order = g.order[:E].cpu().numpy()
        assert np.array_equal(order, np.argsort(kk, kind="stable"))
        seg = g.seg_start[:G + 1].cpu().numpy()
        assert seg[0] == 0 and seg[-1] == E and np.all(np.diff(seg) == np.bincount(inv))
    rix, rjx = orc.neighbors(kk, jj)
    for kb, jb in ((0, 0), (300, 40)):
        ix, jx = ops.neighbors(cu(kk), cu(jj), kb, jb)
        assert np.array_equal(ix.cpu().numpy(), rix) and np.array_equal(jx.cpu().numpy(), rjx)


def test_group_by_small_and_neighbors_from_groups_exact():
    from rampvo_amd import ops
    rng = np.random.default_rng(14)
    E = 6000
    kk = (rng.integers(0, 260, E) + 1000).astype(np.int64)
    ii = kk // 13
    jj = (rng.integers(0, 30, E) + 70).astype(np.int64)
    g = ops.group_by_small(cu(kk), None, 1, 1000, 260, 300)
    uk, inv = np.unique(kk, return_inverse=True)
    G = int(g.ngroups.item())
    assert G == len(uk) and np.array_equal(g.ukeys[:G].cpu().numpy(), uk)
    assert np.array_equal(g.gid[:E].cpu().numpy(), inv)
    assert np.array_equal(g.order[:E].cpu().numpy(), np.argsort(kk, kind="stable"))
    seg = g.seg_start[:G + 1].cpu().numpy()
    assert seg[0] == 0 and seg[-1] == E and np.all(np.diff(seg) == np.bincount(inv))
    f_lo, f_hi = int(min(ii.min(), jj.min())), int(max(ii.max(), jj.max())) + 1
    W = f_hi - f_lo
    gp = ops.group_by_small(cu(ii), cu(jj), W, f_lo * W + f_lo, W * W, 0)
    key = ii * 4096 + jj
    uk2, inv2 = np.unique(key, return_inverse=True)
    assert int(gp.ngroups.item()) == len(uk2) and np.array_equal(gp.gid[:E].cpu().numpy(), inv2)
    assert np.array_equal(gp.order[:E].cpu().numpy(), np.argsort(key, kind="stable"))
    rix, rjx = orc.neighbors(kk, jj)
    ix, jx = ops.neighbors_from_groups(g, cu(jj), 300)
    assert np.array_equal(ix.cpu().numpy(), rix) and np.array_equal(jx.cpu().numpy(), rjx)


def test_ba_with_shared_plan_equals_self_grouped():
    from rampvo_amd import ops
    from rampvo_amd.net import GraphPlan
    s = ba_scene(seed=17, n_frames=9, M=14, lifetime=4, n_total_frames=16, far=True)
    outs = []
    for use_plan in (False, True):
        poses, patches = cu(s["poses"]), cu(s["patches"])
        plan = None
        if use_plan:
            plan = GraphPlan.build(cu(s["ii"]), cu(s["jj"]), cu(s["kk"]), max_kk=9 * 14, max_ij=81,
                                   kk_range=(0, 9 * 14), frame_range=(0, 9))
        ops.ba(poses, patches, cu(s["intr"]), cu(s["target"]), cu(s["weight"]), cu(s["lmbda"]), cu(s["ii"]),
               cu(s["jj"]), cu(s["kk"]), 3, 9, 2, plan=plan)
        outs.append((poses.cpu().numpy(), patches.cpu().numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_group_by_empty_and_single():
    from rampvo_amd import ops
    g = ops.group_by(torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert int(g.ngroups.item()) == 0
    g = ops.group_by(torch.full((17,), 5, dtype=torch.int64, device="cuda"), 6)
    assert int(g.ngroups.item()) == 1 and g.seg_start[:2].tolist() == [0, 17]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_segment_softmax_sum(dtype):
    from rampvo_amd import ops
    rng = np.random.default_rng(6)
    E, C = 3000, 384
    keys = rng.integers(0, 90, E).astype(np.int64) * 12345 + rng.integers(0, 3, E)
    fx = rng.normal(size=(E, C)).astype(np.float32)
    gx = (3 * rng.normal(size=(E, C))).astype(np.float32)
    if dtype == torch.float16:
        fx = fx.astype(np.float16).astype(np.float32)
        gx = gx.astype(np.float16).astype(np.float32)
    uk, inv = np.unique(keys, return_inverse=True)
    ref = orc.segment_softmax_sum(fx, gx, inv, len(uk))
    g = ops.group_by(cu(keys))
    y = ops.segment_softmax_sum(cu(fx).to(dtype), cu(gx).to(dtype), g, len(uk) + 5)
    out = y[:len(uk)].float().cpu().numpy()
    tol = 2e-6 if dtype == torch.float32 else 2e-3
    assert np.abs(out - ref).max() <= tol * max(1.0, np.abs(ref).max())
    assert torch.all(y[len(uk):] == 0)


# ---------------------------------------------------------------------------- BA
@pytest.mark.parametrize("case", BA_ORACLE_CASES)
def test_ba_matches_oracle(case):
    from rampvo_amd import ops
    s, (t0, t1) = ba_oracle_case(case)
    p_ref, pt_ref = s["poses"].copy(), s["patches"].copy()
    st = orc.ba(p_ref, pt_ref, s["intr"], s["target"], s["weight"], s["lmbda"], s["ii"], s["jj"], s["kk"], t0, t1, 2)
    assert st == 0
    poses, patches = cu(s["poses"]), cu(s["patches"])
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.ba(poses, patches, cu(s["intr"]), cu(s["target"]), cu(s["weight"]), cu(s["lmbda"]), cu(s["ii"]),
           cu(s["jj"]), cu(s["kk"]), t0, t1, 2, info)
    assert int(info.item()) == 0
    p, pt = poses.cpu().numpy(), patches.cpu().numpy()
    assert np.array_equal(p[:t0], s["poses"][:t0]) and np.array_equal(p[t1:], s["poses"][t1:])  # fixed poses untouched
    moved = np.abs(p_ref - s["poses"]).max()
    if t1 > t0:
        assert moved > 1e-4                                  # the problem is not degenerate
    # north-star tolerance: 1e-4 relative on fp32 poses / depths.  Problems with almost
    # no fixed poses ("all_free": gauge freedom) are ill-conditioned: there the fp32
    # oracle itself sits ~2e-4 from an fp64 evaluation of the same algorithm, so the
    # bound is widened to 4x that measured fp32 rounding envelope.
    p64, pt64 = orc.ba_f64(s["poses"], s["patches"], s["intr"], s["target"], s["weight"], s["lmbda"],
                           s["ii"], s["jj"], s["kk"], t0, t1, 2)
    env_p, env_d = np.abs(p_ref - p64).max(), np.abs(pt_ref - pt64).max()
    tol_p = max(1e-4 * max(1.0, np.abs(p_ref).max()), 4 * env_p)
    tol_d = max(1e-4 * max(1.0, np.abs(pt_ref[:, 2]).max()), 4 * env_d)
    if case in ("window", "structure_only", "big_window", "full_window"):
        assert 4 * env_p < 1e-4 and 4 * env_d < 1e-4   # well conditioned: the plain 1e-4 bound applies
    assert np.abs(p - p_ref).max() <= tol_p
    assert np.abs(pt - pt_ref).max() <= tol_d
    # x,y channels of the patches are never written
    assert np.array_equal(pt[:, :2], s["patches"][:, :2])


def test_ba_at_the_benchmark_size_by_properties():
    """fastba.BA at BASELINE configs[1]'s graph size -- 23 keyframes x 96 patches, lifetime 13: ~42k factors, a 10-pose
    optimisation window, two Gauss-Newton steps -- through what does not depend on the size (the step itself is checked
    against the oracle at this size by test_full_size_update_step_against_cpu_oracle; here the solver's invariants):
      * a fixed point: with the targets on the solver's own reprojection (cuda_ba.reproject) and unit confidence the
        residuals are zero and poses / depths stay where they are;
      * poses outside [t0, t1) and the patches' pixel coordinates are never written, the run is bit-reproducible;
      * the factor list's order is bookkeeping: a permuted list gives the same step to fp32 summation accuracy;
      * a second call continues from the first one's state: 2 + 2 steps = 4 steps bit for bit."""
    from rampvo_amd import ops
    s = ba_scene(seed=31, n_frames=23, M=96, lifetime=13, n_total_frames=36)
    E, nf = len(s["ii"]), s["n_frames"]
    assert E > 40000
    t0, t1 = nf - 10, nf
    dev = lambda: (cu(s["poses"]), cu(s["patches"]))
    args = lambda tg, w, perm=None: (cu(s["intr"]), tg if perm is None else tg[perm], w if perm is None else w[perm], cu(s["lmbda"]),
                                     *(cu(s[k]) if perm is None else cu(s[k])[perm] for k in ("ii", "jj", "kk")))
    target, weight = cu(s["target"]), cu(s["weight"])
    # --- fixed point
    poses, patches = dev()
    proj = ops.reproject(poses, patches, cu(s["intr"]), cu(s["ii"]), cu(s["jj"]), cu(s["kk"]))[0, :, :, 1, 1].contiguous()
    ops.ba(poses, patches, *args(proj, torch.ones_like(weight)), t0, t1, 2)
    dp = float((poses - cu(s["poses"])).abs().max()); dd = float((patches - cu(s["patches"])).abs().max())
    print("zero-residual problem: poses move %.2e, depths %.2e" % (dp, dd))
    assert dp <= 1e-6 and dd <= 1e-6
    # --- a real step: untouched state, reproducibility
    runs = []
    for _ in range(2):
        poses, patches = dev()
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        ops.ba(poses, patches, *args(target, weight), t0, t1, 2, info)
        assert int(info.item()) == 0
        runs.append((poses.clone(), patches.clone()))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    p, pt = runs[0]
    assert torch.equal(p[:t0], cu(s["poses"])[:t0]) and torch.equal(p[t1:], cu(s["poses"])[t1:])
    assert torch.equal(pt[:, :2], cu(s["patches"])[:, :2])
    step = float((p - cu(s["poses"])).abs().max())
    assert step > 1e-4                                        # the problem is not degenerate
    # --- the order of the factor list
    perm = torch.from_numpy(np.random.default_rng(5).permutation(E)).cuda()
    poses, patches = dev()
    ops.ba(poses, patches, *args(target, weight, perm), t0, t1, 2)
    ep = float((poses - p).abs().max()) / max(1.0, float(p.abs().max())); ed = float((patches[:, 2] - pt[:, 2]).abs().max())
    print("permuted factor list: poses %.2e, depths %.2e from the listed order (GN step %.2e)" % (ep, ed, step))
    assert ep <= 1e-5 and ed <= 1e-4 * max(1.0, float(pt[:, 2].abs().max()))
    # --- 2 + 2 iterations = 4 iterations
    a_p, a_pt = dev()
    ops.ba(a_p, a_pt, *args(target, weight), t0, t1, 4)
    b_p, b_pt = dev()
    ops.ba(b_p, b_pt, *args(target, weight), t0, t1, 2)
    ops.ba(b_p, b_pt, *args(target, weight), t0, t1, 2)
    assert torch.equal(a_p, b_p) and torch.equal(a_pt, b_pt)


def test_ba_is_deterministic():
    from rampvo_amd import ops
    s = ba_scene(seed=12, n_frames=9, M=14, lifetime=4, n_total_frames=16, far=True)
    outs = []
    for _ in range(3):
        poses, patches = cu(s["poses"]), cu(s["patches"])
        ops.ba(poses, patches, cu(s["intr"]), cu(s["target"]), cu(s["weight"]), cu(s["lmbda"]), cu(s["ii"]),
               cu(s["jj"]), cu(s["kk"]), 2, 9, 2)
        outs.append((poses.cpu().numpy(), patches.cpu().numpy()))
    for p, pt in outs[1:]:
        assert np.array_equal(p, outs[0][0]) and np.array_equal(pt, outs[0][1])


def test_ops_refuse_cpu_tensors():
    from rampvo_amd import ops
    with pytest.raises(RuntimeError):
        ops.se3_unary("ramp_se3_inv", torch.zeros(1, 7), 7, 7)


@pytest.mark.parametrize("shape,k", [((5, 96, 128), 6), ((5, 480, 640), 96), ((5, 260, 348), 40)])
def test_event_topk_matches_aten_pipeline(shape, k):
    """ramp_event_topk against the reference's ATen pipeline (ramp/utils.py:186-226): identical cell
    indices in identical order, and x = index / h as a true division"""
    import torch.nn.functional as F
    from rampvo_amd import ops
    g = torch.Generator().manual_seed(17)
    ev = (torch.randn(*shape, generator=g) * 20).cuda()
    ev[:, :8] = 0                                                   # a dead band: NMS zeros / ties at 0 stay below the top-k
    coords, idx = ops.event_topk(ev, k, 11, want_indices=True)
    s = F.avg_pool2d(ev.abs()[None], 4, 4).transpose(3, 2).mean(dim=1)          # [1, w, h]
    mx = F.max_pool2d(s.unsqueeze(0), 11, stride=1, padding=5).squeeze(0)
    s = s * (mx == s).float()
    hh = s.shape[-1]
    val, ref = torch.topk(s.flatten(1), k=k, dim=-1)
    assert float(val.min()) > 0                                     # tie-free fixture
    assert torch.equal(idx, ref[0])
    assert torch.equal(coords[:, 0], (ref[0] / hh).float()) and torch.equal(coords[:, 1], (ref[0] % hh).float())


def test_event_topk_ties_take_lowest_index():
    from rampvo_amd import ops
    ev = torch.zeros(1, 64, 64, device="cuda")
    ev[0, 8:12, 8:12] = 3.0           # one cell with score 3
    ev[0, 40:44, 20:24] = 5.0         # one cell with score 5
    coords, idx = ops.event_topk(ev, 5, 0, want_indices=True)
    h = 16
    assert idx[:2].tolist() == [5 * h + 10, 2 * h + 2]               # (X=5,Y=10) then (X=2,Y=2)
    assert idx[2:].tolist() == [0, 1, 2]                              # zeros: lowest flat indices


def test_event_topk_dense_map_without_nms():
    """no NMS: every cell is a candidate (more than the LDS list holds) -> the streaming passes"""
    import torch.nn.functional as F
    from rampvo_amd import ops
    g = torch.Generator().manual_seed(23)
    ev = (torch.randn(5, 480, 640, generator=g) * 20).cuda()
    coords, idx = ops.event_topk(ev, 200, 0, want_indices=True)
    s = F.avg_pool2d(ev.abs()[None], 4, 4).transpose(3, 2).mean(dim=1)
    val, ref = torch.topk(s.flatten(1), k=200, dim=-1)
    assert torch.equal(idx, ref[0])


def test_fused_gru_chain_matches_gemm_path():
    """csrc/update_mlp.hip::upd_gru_kernel (6 Linear layers + gates + LayerNorm in one launch) against
    the same operator stitched from library GEMMs and the row kernels; E not a multiple of the 64-row tile"""
    from rampvo_amd.synthetic import make_network
    from rampvo_amd.net import GraphPlan
    net = make_network("SingleScale")
    fu = net.update.fused(torch.float16)
    g = torch.Generator().manual_seed(3)
    E, M = 1000, 40
    kk = torch.sort(torch.randint(0, M * 6, (E,), generator=g)).values.cuda()
    ii = kk // M
    jj = torch.randint(0, 8, (E,), generator=g).cuda()
    plan = GraphPlan.build(ii, jj, kk)
    netst = (torch.randn(E, 384, generator=g) * 0.5).cuda()
    inp = (torch.randn(E, 384, generator=g) * 0.5).half().cuda()
    corr = (torch.randn(E, 882, generator=g) * 0.5).half().cuda()
    outs = {}
    with torch.no_grad():
        for mlp in (False, True):
            fu.use_mlp = mlp
            o32, rt = fu.hidden(netst.clone(), inp, None, 0, corr, plan)
            outs[mlp] = (o32.clone(), rt.float().clone())
    fu.use_mlp = True
    scale = float(outs[False][0].abs().max())
    assert float((outs[False][0] - outs[True][0]).abs().max()) <= 4e-3 * scale      # fp16 GEMM inputs on both sides
    assert float((outs[False][1] - outs[True][1]).abs().max()) <= 4e-3 * scale
    assert torch.equal(outs[True][1], torch.relu(outs[True][0]).half().float())
    # the tracker's form: state rows through a row map (-1 = new factor), context rows through a ring index
    net_map = torch.randint(-1, 700, (E,), generator=g).cuda()
    table = (torch.randn(300, 384, generator=g) * 0.5).half().cuda()
    inp_idx = torch.randint(0, 5000, (E,), generator=g).cuda()
    with torch.no_grad():
        for mlp in (False, True):
            fu.use_mlp = mlp
            o32, rt = fu.hidden(netst[:700].contiguous(), table, inp_idx, 300, corr, plan, net_map=net_map)
            outs[mlp] = (o32.clone(), rt.float().clone())
    fu.use_mlp = True
    scale = float(outs[False][0].abs().max())
    assert float((outs[False][0] - outs[True][0]).abs().max()) <= 4e-3 * scale
    assert float((outs[False][1] - outs[True][1]).abs().max()) <= 4e-3 * scale
    # padded correlation rows (the tracker's layout): the default path against the library path on the same padded rows
    corr_pad = torch.nn.functional.pad(corr, (0, 896 - 882)).contiguous()
    res = {}
    with torch.no_grad():
        for mlp in (False, True):
            fu.use_mlp = mlp
            o32, rt = fu.hidden(netst[:700].contiguous(), table, inp_idx, 300, corr_pad, plan, net_map=net_map)
            res[mlp] = (o32.clone(), rt.float().clone())
    fu.use_mlp = True
    # heads: row-wise dot-product kernel (+ target / weight epilogue) vs the [E,384]x[384,4] GEMM + upd_heads
    coords = (torch.rand(E, 2, 3, 3, generator=g) * 60).cuda()
    relu_t = res[True][1].half()
    with torch.no_grad():
        t_ref, w_ref, _ = fu.target_weight(fu.heads(relu_t), coords, 40.0, 30.0)
        t_new, w_new = fu.heads_linear(relu_t, coords, 40.0, 30.0)
    assert float((t_ref - t_new).abs().max()) <= 2e-3 * max(1.0, float(t_ref.abs().max()))
    near_edge = ((t_ref - torch.tensor([40.0, 30.0], device="cuda")).abs().min(-1).values < 0.1) | (t_ref.abs().min(-1).values < 0.1)
    assert float(((w_ref - w_new).abs().max(-1).values * (~near_edge)).max()) <= 2e-3
    assert float((res[False][0] - res[True][0]).abs().max()) <= 4e-3 * scale
    assert float((res[False][0] - outs[True][0]).abs().max()) <= 4e-3 * scale          # padding changes nothing


FUSED_CHAIN_TOL = 3e-3      # x the output scale; measured worst case is recorded by the test's print


@pytest.mark.parametrize("E,mode", [(1003, "small"), (20011, "small"), (41003, "small"), (41003, "pairs"), (5000, "ones")])
@torch.no_grad()
def test_softagg_fused_against_fp32_torch(E, mode):
    """SoftAgg without the [f | g] rows (csrc/update_mlp.hip::upd_softagg_kernel + upd_softagg_finish_kernel) against a
    plain fp32 PyTorch evaluation of ramp/blocks.py:42-47 on the fp16-rounded operands (f, g, y and h(y) are half tensors
    under the reference's autocast), and against the three-launch path it replaces.  Groupings: `small` = patch-like groups
    of 1..40 factors scattered over the list (runs cross lane blocks and tiles), `pairs` = 96 factors per group (a group =
    one and a fifth tiles), `ones` = every factor its own group."""
    import torch.nn.functional as F
    from rampvo_amd import ops
    from rampvo_amd.synthetic import make_network
    net = make_network("SingleScale")
    fu = net.update.fused(torch.float16)
    w = fu.weights()
    agg = make_network("SingleScale").update.float().agg_kk
    for lin in (agg.f, agg.g, agg.h):
        lin.weight.copy_(lin.weight.half().float()); lin.bias.copy_(lin.bias.half().float())
    g = torch.Generator().manual_seed(E)
    if mode == "small":
        sizes = torch.randint(1, 41, (E,), generator=g)
        keys = torch.repeat_interleave(torch.arange(E), sizes)[:E]
    elif mode == "pairs":
        keys = torch.arange(E) // 96
    else:
        keys = torch.arange(E)
    keys = keys[torch.randperm(E, generator=g)].cuda()
    x32 = (torch.randn(E, 384, generator=g) * 0.7).cuda()
    if mode == "small":
        # a few groups whose g lies ~100 below their neighbours' in every column: the block-wide shift of the fast sweep
        # underflows there and the exact sweep takes over (rows scaled so that g = W x + b moves by O(100))
        x32[keys < 3] *= 60.0
    G0 = 57
    hy0 = (torch.randn(G0, 384, generator=g) * 0.5).half().cuda()
    gid0 = torch.randint(0, G0, (E,), generator=g).int().cuda()
    grp = ops.group_by(keys)
    G = int(grp.ngroups.item())
    for add in (False, True):
        xe = x32 + hy0.float()[gid0.long()] if add else x32
        xh = xe.half().float()
        fh, gh = agg.f(xh).half().float(), agg.g(xh).half().float()
        inv = grp.gid[:E].long()
        m = torch.full((G, 384), -float("inf"), device="cuda").scatter_reduce(0, inv[:, None].expand(-1, 384), gh, "amax")
        e = torch.exp(gh - m[inv])
        z = torch.zeros(G, 384, device="cuda").index_add_(0, inv, e)
        y = (torch.zeros(G, 384, device="cuda").index_add_(0, inv, fh * e) / z).half().float()
        exp = agg.h(y).half().float()
        got = fu.softagg(x32, hy0 if add else None, gid0 if add else None, w["kk_fg_pack"], w["kk_h_pack"], grp, G + 5, E)
        assert got.shape == (G + 5, 384) and float(got[G:].abs().max()) == 0.0
        scale = float(exp.abs().max())
        err = float((got[:G].float() - exp).abs().max()) / scale
        old = fu.h_lin(fu.seg(fu.fg(x32.clone(), hy0 if add else None, gid0 if add else None, w["kk_fg_pack"], E), grp, G + 5),
                       w["kk_h_pack"], grp)
        err_old = float((old[:G].float() - exp).abs().max()) / scale
        print(E, mode, add, "softagg vs fp32 torch %.2e (three-launch path: %.2e)" % (err, err_old))
        assert err <= FUSED_CHAIN_TOL, (E, mode, add, err)


@pytest.mark.parametrize("E", [1003, 5408, 20011, 41003])
@torch.no_grad()
def test_fused_update_chains_against_fp32_torch(E):
    """every fused fp16 MFMA chain of the update operator (csrc/update_mlp.hip, update.hip) on its own against a
    PLAIN fp32 PyTorch evaluation of the same reference expressions (ramp/net.py:69-90, ramp/blocks.py:15-50) on the
    fp16-rounded operands the kernels consume (fp16 weights / biases / inputs, fp32 everywhere else): what separates
    the two is the kernels' fp16 rounding of the activations they park in LDS between layers.  No comparison with
    this repo's own GEMM path.  E = 1003: the 64-row kernels; 20011 / 41003: the big-tile kernels (96 / 176 rows per
    workgroup); none a multiple of its tile."""
    import torch.nn.functional as F
    from rampvo_amd.synthetic import make_network
    net = make_network("SingleScale")
    fu = net.update.fused(torch.float16)
    w = fu.weights()
    ref = make_network("SingleScale").update.float()          # same seeded weights, a second module
    # the operands the fp16 path consumes: Linear weights / biases rounded to fp16; LayerNorm parameters stay fp32
    for mod in ref.modules():
        if isinstance(mod, torch.nn.Linear):
            mod.weight.copy_(mod.weight.half().float())
            mod.bias.copy_(mod.bias.half().float())
    g = torch.Generator().manual_seed(17)
    G = 57
    rnd = lambda *s, sc=0.5: (torch.randn(*s, generator=g) * sc).cuda()
    worst = {}

    def cmp(name, got, exp, tol=FUSED_CHAIN_TOL):
        scale = float(exp.abs().max())
        err = float((got.float() - exp).abs().max()) / scale
        worst[name] = err
        assert err <= tol, (name, err, worst)

    # --- upd_gru: LN(x + hy[gid]) -> GatedResidual -> LN -> GatedResidual (+ relu copy)
    x32, hy = rnd(E, 384), rnd(G, 384).half()
    gid = torch.randint(0, G, (E,), generator=g).int().cuda()
    out32, relu_t = fu.gru(x32, add=(hy, gid))
    exp = ref.gru(x32 + hy.float()[gid.long()])
    cmp("gru", out32, exp)
    cmp("gru_relu", relu_t, torch.relu(exp))
    # the same launch with the heads in its epilogue (ramp_upd_gru_heads): out32 bit-equal, target / weight against fp32
    # torch on the launch's own relu copy (the heads' half input)
    hcoords = (torch.rand(E, 2, 3, 3, generator=g) * 60).cuda()
    out32_h, htarget, hweight = fu.gru(x32, add=(hy, gid), heads_at=(hcoords, 40.0, 30.0))
    assert torch.equal(out32_h, out32)
    t_exp = hcoords[:, :, 1, 1] + ref.d[1](relu_t.float())
    w_exp = torch.sigmoid(ref.w[1](relu_t.float()))
    inside = (t_exp[:, 0] >= 0) & (t_exp[:, 1] >= 0) & (t_exp[:, 0] <= 40.0) & (t_exp[:, 1] <= 30.0)
    cmp("gru_heads_target", htarget[0], t_exp, tol=2e-3)
    far = ((t_exp - torch.tensor([40.0, 30.0], device="cuda")).abs().min(-1).values > 0.2) & (t_exp.abs().min(-1).values > 0.2)
    assert float(((hweight[0] - w_exp * inside[:, None].float()).abs().max(-1).values * far.float()).max()) <= 2e-3
    # without the prologue: x32 is already gru[0]'s output
    xin = ref.gru[0](x32)
    cmp("gru_noprologue", fu.gru(xin)[0], ref.gru[3](ref.gru[2](ref.gru[1](xin))))

    # --- upd_nbr: net + Lb(relu(La(mask * net[idx])))
    net_in = rnd(E, 384)
    idx = torch.randint(-1, E, (E,), generator=g).cuda()
    idx[::5] = -1
    for name, seq in (("c1_pack", ref.c1), ("c2_pack", ref.c2)):
        o, ot = fu.nbr(net_in, idx, name[:2], want_t=True)
        gathered = net_in[idx.clamp(min=0)] * (idx >= 0).float()[:, None]
        exp = net_in + seq(gathered)
        cmp("nbr_" + name, o, exp)
        cmp("nbr_t_" + name, ot, exp)

    # --- upd_corr_mlp: LN_norm(net[map] + inp[idx % mod] + corr-MLP(corr))
    corr = F.pad(rnd(E, 882, sc=2.0).half(), (0, 14)).contiguous()
    state = rnd(700, 384)
    net_map = torch.randint(-1, 700, (E,), generator=g).cuda()
    net_map[-3:] = 699
    table = rnd(300, 384).half()
    inp_idx = torch.randint(0, 5000, (E,), generator=g).cuda()
    o = fu.corr_mlp(corr, state, net_map, table, inp_idx, 300)
    st = state[net_map.clamp(min=0)] * (net_map >= 0).float()[:, None]
    exp = ref.norm(st + table.float()[inp_idx % 300] + ref.corr(corr[:, :882].float()))
    cmp("corr_mlp", o, exp)
    # zero state / identity context (the motion probe's form)
    o = fu.corr_mlp(corr, None, None, rnd(E, 384).half(), None, 0)
    assert torch.isfinite(o).all()

    # --- upd_fg: x = x32 (+ add[gid], written back); fg = [f(x) | g(x)]; then the segment softmax + h: SoftAgg
    for name, agg in (("kk_fg_pack", ref.agg_kk), ("ij_fg_pack", ref.agg_ij)):
        xs = x32.clone()
        fg = fu.fg(xs, hy, gid, w[name], E)
        xe = x32 + hy.float()[gid.long()]
        cmp("fg_x_" + name, xs, xe, tol=1e-6)
        cmp("fg_" + name, fg, torch.cat([agg.f(xe), agg.g(xe)], 1))

    # --- heads: Linear(384 -> 2) x 2 on relu(net), target = centre + delta, weight = sigmoid(.) inside the image
    relu_in = torch.relu(rnd(E, 384)).half()
    coords = (torch.rand(E, 2, 3, 3, generator=g) * 60).cuda()
    target, weight = fu.heads_linear(relu_in, coords, 40.0, 30.0)
    delta = ref.d[1](relu_in.float())
    t_exp = coords[:, :, 1, 1] + delta
    w_exp = torch.sigmoid(ref.w[1](relu_in.float()))
    inside = (t_exp[:, 0] >= 0) & (t_exp[:, 1] >= 0) & (t_exp[:, 0] <= 40.0) & (t_exp[:, 1] <= 30.0)   # utils.py:557-570
    cmp("heads_target", target[0], t_exp, tol=2e-3)
    far = ((t_exp - torch.tensor([40.0, 30.0], device="cuda")).abs().min(-1).values > 0.2) & (t_exp.abs().min(-1).values > 0.2)
    assert float(((weight[0] - w_exp * inside[:, None].float()).abs().max(-1).values * far.float()).max()) <= 2e-3
    print("fused update chains vs fp32 torch, max err / output scale:", {k: round(v, 6) for k, v in worst.items()})


def test_event_stack_matches_reference_golden_and_oracle():
    """ramp_event_stack against the reference's EventToStack_Numpy output (tests/golden/event_stack.npz,
    incl. an int8 overflow) and against the oracle on a larger random list"""
    import os
    from rampvo_amd import ops
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "event_stack.npz"))
    H, W, B = int(g["height"]), int(g["width"]), int(g["bins"])
    out = ops.event_stack(cu(g["x"].astype(np.int32)), cu(g["y"].astype(np.int32)), cu(g["p"]), H, W, B, as_float=False)
    assert np.array_equal(out.cpu().numpy(), g["out"])
    rng = np.random.default_rng(5)
    N, H, W = 300001, 480, 640
    x, y = rng.integers(-2, W + 2, N).astype(np.int32), rng.integers(-2, H + 2, N).astype(np.int32)   # some outside
    p = rng.integers(0, 2, N).astype(np.int8) * 2 - 1
    ref = orc.event_stack(x, y, p, H, W, 5)
    outf = ops.event_stack(cu(x), cu(y), cu(p), H, W, 5)
    assert outf.dtype == torch.float32 and np.array_equal(outf.cpu().numpy(), ref.astype(np.float32))
    assert float(ops.event_stack(cu(x[:1]), cu(y[:1]), cu(p[:1]), H, W, 5).abs().sum()) == 0.0     # < 2 events


def test_depth_median_fill_matches_torch_median():
    from rampvo_amd import ops
    g = torch.Generator().manual_seed(2)
    N, M, P = 12, 96, 3
    state = (torch.rand(N, M, 3, P, P, generator=g) * 19 + 1e-3).cuda()
    state[5, :7, 2] = -0.25                                     # sign handling of the key map
    for n in (3, 8, 12):
        new = torch.rand(M, 3, P, P, generator=g).cuda()
        keep = new.clone()
        ops.depth_median_fill(state, n, 3, new)
        med = torch.median(state[n - 3:n, :, 2])
        assert torch.equal(new[:, 2], med.expand(M, P, P)) and torch.equal(new[:, :2], keep[:, :2])


def test_ba_flags_pair_list_overflow_instead_of_truncating():
    """> 1024 pose-pair records on one pose (a frame connected to 1100 others): ramp_ba_forward must raise bit 1 of
    *info rather than drop terms silently (csrc/ba.hip::ba_assemble_kernel's LDS list)"""
    from rampvo_amd import ops
    NF, M = 1102, 1
    rng = np.random.default_rng(0)
    poses = np.zeros((NF, 7), np.float32); poses[:, 6] = 1.0
    poses[:, :3] = rng.normal(0, 0.01, (NF, 3))
    patches = np.zeros((NF * M, 3, 3, 3), np.float32)
    gy, gx = np.meshgrid(np.arange(-1, 2), np.arange(-1, 2), indexing="ij")
    patches[:, 0] = 40 + gx; patches[:, 1] = 30 + gy; patches[:, 2] = 0.5
    intr = np.tile(np.array([80, 80, 80, 60], np.float32), (NF, 1))
    ii = np.arange(1, NF, dtype=np.int64); jj = np.zeros(NF - 1, np.int64); kk = ii.copy()      # every frame -> frame 0 ... and back
    ii = np.concatenate([ii, np.zeros(NF - 1, np.int64)]); jj = np.concatenate([jj, np.arange(1, NF)]); kk = np.concatenate([kk, np.zeros(NF - 1, np.int64)])
    E = len(ii)
    target = np.full((E, 2), 40.0, np.float32); weight = np.full((E, 2), 0.5, np.float32)
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    p, pt = cu(poses), cu(patches)
    ops.ba(p, pt, cu(intr), cu(target), cu(weight), cu(np.array([1e-4], np.float32)), cu(ii), cu(jj), cu(kk), 0, 4, 1, info)
    assert int(info.item()) & 2, int(info.item())
    # the same call on a graph within the limit leaves the bit clear
    sel = (ii < 300) & (jj < 300)
    info.zero_()
    ops.ba(cu(poses), cu(patches), cu(intr), cu(target[sel]), cu(weight[sel]), cu(np.array([1e-4], np.float32)), cu(ii[sel]),
           cu(jj[sel]), cu(kk[sel]), 0, 4, 1, info)
    assert int(info.item()) & 2 == 0


def test_ba_eff_impl_at_config5_size():
    """BASELINE configs[4]'s bundle adjustment (32 free keyframes: a 192 x 192 Schur system, 256 patches per frame,
    lifetime 33, ~10k patch depths, ~0.6M edges) with ``eff_impl=True``: against the oracle's restatement of the
    reference's block-sparse E lookup (fastba/block_e.cu:43-283, ``orc.ba(eff_ppf=...)``), which itself agrees with the
    dense restatement; the flag does not change this implementation's result (one storage serves both)."""
    import time
    from rampvo_amd import fastba, _lib
    M, NF, N = 256, 50, 32
    s = ba_scene(seed=31, n_frames=NF, M=M, lifetime=33, H=180, W=320, noise=0.4, n_total_frames=NF + 2)
    E = len(s["ii"])
    assert E > 500000
    t0, t1 = NF - N, NF
    w = (s["weight"] * 1e-2).astype(np.float32)      # small confidences keep this random problem well conditioned
    rp, rpt = s["poses"].copy(), s["patches"].copy()
    tic = time.perf_counter()
    st = orc.ba(rp, rpt, s["intr"], s["target"], w, s["lmbda"], s["ii"], s["jj"], s["kk"], t0, t1, 2, eff_ppf=M)
    t_cpu = time.perf_counter() - tic
    dp, dpt = s["poses"].copy(), s["patches"].copy()
    orc.ba(dp, dpt, s["intr"], s["target"], w, s["lmbda"], s["ii"], s["jj"], s["kk"], t0, t1, 2)
    step = float(np.abs(rp - s["poses"]).max())
    assert st == 0 and step > 1e-4
    assert np.abs(rp - dp).max() <= 1e-5 * max(1.0, step) and np.abs(rpt - dpt).max() <= 1e-4        # lookup == dense
    out = {}
    for eff in (True, False):
        poses, patches = cu(s["poses"]), cu(s["patches"])
        info = torch.zeros(1, dtype=torch.int32, device="cuda")
        args = (cu(s["intr"]), cu(s["target"]), cu(w), cu(s["lmbda"]), cu(s["ii"]), cu(s["jj"]), cu(s["kk"]), t0, t1)
        fastba.BA(poses, patches, *args, M=M, iterations=2, eff_impl=eff, info=info)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        p2, pt2 = cu(s["poses"]), cu(s["patches"])
        a.record()
        fastba.BA(p2, pt2, *args, M=M, iterations=2, eff_impl=eff, info=info)
        b.record(); torch.cuda.synchronize()
        assert int(info.item()) == 0
        out[eff] = (poses.cpu().numpy(), patches.cpu().numpy(), a.elapsed_time(b))
    assert np.array_equal(out[True][0], out[False][0]) and np.array_equal(out[True][1], out[False][1])
    scale = max(1.0, step)
    assert np.abs(out[True][0] - rp).max() <= 1e-4 * scale, np.abs(out[True][0] - rp).max()
    d_ref = rpt[:, 2, 1, 1]
    assert (np.abs(out[True][1][:, 2, 1, 1] - d_ref) / np.maximum(np.abs(d_ref), 1.0)).max() <= 1e-4 * scale
    Mu = len(np.unique(s["kk"]))
    ws = _lib.lib().ramp_ba_workspace_bytes(E, NF + 2, (NF + 2) * M, t0, t1)
    print("configs[4]-size BA: E=%d Mu=%d 6N=%d | per-patch E rows %.1f MB of a %.1f MB workspace | HIP %.2f ms (incl. its own "
          "group-by) vs oracle lookup path %.1f s | |GN step| %.3g, pose err %.2e"
          % (E, Mu, 6 * N, Mu * 6 * N * 4 / 1e6, ws / 1e6, out[True][2], t_cpu, step, np.abs(out[True][0] - rp).max()))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_frame_gather_equals_the_separate_patchify_launches(dtype):
    """ramp_frame_gather = the four patchify calls of ramp/net.py:167-203 + the colour conversion of
    Ramp_vo.py:353-354 in one launch: bit-identical, including centres on the border and fractional centres"""
    from rampvo_amd import altcorr, ops
    from rampvo_amd._lib import RAMP_NHWC
    from rampvo_amd.utils import coords_grid_with_index
    torch.manual_seed(8)
    h, w, M = 30, 40, 24
    f = torch.randn(h, w, 128, device="cuda").to(dtype)
    i = torch.randn(h, w, 384, device="cuda").to(dtype)
    img = torch.rand(3, 4 * h, 4 * w, device="cuda") - 0.5
    coords = torch.stack([torch.randint(0, w, (M,)), torch.randint(0, h, (M,))], -1).float().cuda()
    coords[0] = torch.tensor([0.0, 0.0]); coords[1] = torch.tensor([w - 1.0, h - 1.0])
    coords[2] = torch.tensor([3.25, 7.75]); coords[3] = torch.tensor([w - 1.5, 0.5])
    g, ip, pt, cl, col = ops.frame_gather(f, i, img, coords)
    cn = coords[None]
    g_ref = ops.patchify(f[None], cn, 1, True, RAMP_NHWC, RAMP_NHWC)[0]
    i_ref = ops.patchify(i[None], cn, 0, True, RAMP_NHWC, RAMP_NHWC)[0].view(M, 384)
    grid, _ = coords_grid_with_index(torch.ones(1, 1, h, w, device="cuda"), device="cuda")
    p_ref = altcorr.patchify(grid[0].contiguous(), cn, 1)[0]
    c_ref = altcorr.patchify(img[None], 4 * (cn + 0.5), 0)[0].view(M, 3)
    col_ref = ((c_ref.flip(-1) + 0.5) * (255.0 / 2)).to(torch.uint8)
    assert torch.equal(g, g_ref) and torch.equal(ip, i_ref)
    assert torch.equal(pt, p_ref) and torch.equal(cl, c_ref) and torch.equal(col, col_ref)


# ------------------------------------------------------- device-resident tracking step (csrc/track.hip)
@torch.no_grad()
@pytest.mark.parametrize("remove", [False, True])
def test_device_graph_edit_matches_host_edit(remove):
    """Ramp_vo.keyframe() + the next frame's append_factors as kernels (trk_flag / trk_decide / trk_apply, then the
    graph plan with device-side sizes) against the host-side restatements the host-driven path uses: the kept factors
    and their hidden-state rows (ramp_graph_edit_host), the new factors (Ramp_vo._new_edges, the reference's meshgrid),
    the rows of the per-frame buffers after the shift, the (t0, dP) log entry, and the plan (GraphPlan.build with
    host-side sizes).  Integer outputs exact; dP bit-equal to the lietorch ops."""
    from rampvo_amd import _lib, ops, track_dev as td
    from rampvo_amd.config import make_cfg
    from rampvo_amd.lietorch import SE3
    from rampvo_amd.net import GraphPlan
    from rampvo_amd.Ramp_vo import Ramp_vo
    from rampvo_amd.synthetic import make_network
    cfg = make_cfg("default", PATCHES_PER_FRAME=48, MIXED_PRECISION=True)
    slam = Ramp_vo(cfg, make_network("SingleScale"), {"event_bias": True}, ht=128, wd=192)
    dv = td.DeviceTrack(slam)
    M, r, R, KI = slam.M, cfg.PATCH_LIFETIME, cfg.REMOVAL_WINDOW, cfg.KEYFRAME_INDEX
    rng = np.random.default_rng(11 + remove)
    n = 31                                       # keyframes when keyframe() runs
    # a plausible graph: patches of the frames in the removal window (a few older ones that the edit must cull), each
    # connected to some frames within its lifetime; in append order of nothing in particular
    E = 9000
    kk = rng.integers((n - R - 3) * M, n * M, E).astype(np.int64)
    ii = kk // M
    jj = np.clip(ii + rng.integers(-r + 1, r, E), 0, n - 1).astype(np.int64)
    g = np.zeros((4, dv.E_cap), np.int64)
    g[0, :E], g[1, :E], g[2, :E], g[3, :E] = ii, jj, kk, np.arange(E)
    dv.graph[0].copy_(torch.from_numpy(g).cuda())
    dv.cur = 0
    flo = int(min(ii.min(), jj.min()))
    d = np.zeros(td.DYN_WORDS, np.int32)
    d[td.DYN_N], d[td.DYN_NROW], d[td.DYN_E] = n, n - 1, E
    d[td.DYN_KLO], d[td.DYN_FLO], d[td.DYN_W] = int(kk.min()) // M * M, flo, n - flo
    dv.dyn.copy_(torch.from_numpy(d).cuda())
    # recognisable per-frame state
    slam.tstamps_[:n] = torch.arange(100, 100 + n, device="cuda")
    xi = torch.from_numpy((0.2 * rng.normal(size=(n, 6))).astype(np.float32)).cuda()
    slam.poses_[:n] = ops.se3_unary("ramp_se3_exp", xi, 6, 7)
    for buf in (slam.patches_, slam.intrinsics_, slam.imap_, slam.gmap_, slam.fmap1_, slam.fmap2_):
        buf.copy_(torch.randn(buf.shape, device="cuda").to(buf.dtype))
    slam.colors_.copy_(torch.randint(0, 255, slam.colors_.shape, device="cuda", dtype=torch.uint8))
    before = {k: getattr(slam, k).clone() for k in ("tstamps_", "colors_", "poses_", "patches_", "intrinsics_", "imap_",
                                                     "gmap_", "fmap1_", "fmap2_")}
    thresh = cfg.KEYFRAME_THRESH
    dv.mm.copy_(torch.tensor([thresh - 1.0, thresh - 3.0] if remove else [thresh + 1.0, thresh - 0.5], device="cuda"))
    dv.active = True
    dv._frames = 0
    dv.step(counter=77, flags=td.KEYFRAME | td.MM_GIVEN)
    torch.cuda.synchronize()
    dd = dv.dyn.cpu().numpy()
    # ---- host restatement
    k = n - KI
    n_after = n - 1 if remove else n
    buf = np.empty((4, E), np.int64)
    Ek = _lib.lib().ramp_graph_edit_host(ii.ctypes.data, jj.ctypes.data, kk.ctypes.data, None, E, M, k if remove else -1,
                                         n_after, R, buf.ctypes.data, E, None)
    e_ii, e_jj, e_kk = slam._new_edges(n_after + 1)
    ne = len(e_kk)
    assert (dd[td.DYN_REMOVED], dd[td.DYN_K], dd[td.DYN_NPREV], dd[td.DYN_EPREV]) == (int(remove), k, n, E)
    assert (dd[td.DYN_EKEPT], dd[td.DYN_E], dd[td.DYN_NROW], dd[td.DYN_N]) == (Ek, Ek + ne, n_after, n_after + 1)
    assert dd[td.DYN_STATUS] == 0 and dd[td.DYN_FRAME] == 77
    got = dv.graph[1][:, :Ek + ne].cpu().numpy()
    assert np.array_equal(got[:, :Ek], buf[:, :Ek])
    assert np.array_equal(got[0, Ek:], e_ii) and np.array_equal(got[1, Ek:], e_jj) and np.array_equal(got[2, Ek:], e_kk)
    assert (got[3, Ek:] == -1).all()
    # ---- per-frame rows
    for name, ring in (("tstamps_", 0), ("colors_", 0), ("poses_", 0), ("patches_", 0), ("intrinsics_", 0),
                       ("imap_", slam.mem), ("gmap_", slam.mem), ("fmap1_", slam.mem), ("fmap2_", slam.mem)):
        exp = before[name].clone()
        if remove:
            for row in range(k, n - 1):
                exp[row % ring if ring else row] = exp[(row + 1) % ring if ring else row + 1]
        rows_now = getattr(slam, name)
        if name == "fmap1_" and dv.fmap1_slot is not None:
            # level-0 planes by slot table (ramp_track.fmap1_slot): ring row r lives in slot tab[r]; a dropped keyframe
            # rotates entries k .. n - 1 (the freed slot goes to row n - 1, the next new frame's: its content is unspecified)
            tab = dv.fmap1_slot.long()
            assert sorted(tab.tolist()) == list(range(ring))
            rows_now = rows_now[tab]
            if remove:
                keep = torch.ones(ring, dtype=torch.bool, device=rows_now.device)
                keep[(n - 1) % ring] = False
                rows_now, exp = rows_now[keep], exp[keep]
        assert torch.equal(rows_now, exp), name
    # ---- delta log
    assert dd[td.DYN_NLOG] == int(remove)
    if remove:
        ent = dv.dlog[0].cpu()
        t1, t0 = ent[:2].view(torch.int32).tolist()
        assert (t1, t0) == (100 + k, 100 + k - 1)
        dP = (SE3(before["poses_"][k]) * SE3(before["poses_"][k - 1]).inv()).data
        assert torch.equal(ent[2:9].cuda(), dP)
    # ---- plan of the new graph
    cu_ = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    a_ii, a_jj, a_kk = cu_(got[0]), cu_(got[1]), cu_(got[2])
    f_lo, f_hi = int(min(got[0].min(), got[1].min())), n_after + 1
    assert dd[td.DYN_FLO] == f_lo and dd[td.DYN_W] == f_hi - f_lo
    k_lo = int(dd[td.DYN_KLO])
    assert k_lo <= got[2].min()
    ref = GraphPlan.build(a_ii, a_jj, a_kk, max_kk=dv.kk_cap, max_ij=dv.ij_cap, kk_range=(k_lo, f_hi * M),
                          frame_range=(f_lo, f_hi))
    Et = Ek + ne
    for mine, theirs in ((dv.kk, ref.g_kk), (dv.ij, ref.g_ij)):
        ng = int(theirs.ngroups.item())
        assert int(mine["ngroups"].item()) == ng
        assert torch.equal(mine["order"][:Et], theirs.order[:Et]) and torch.equal(mine["gid"][:Et], theirs.gid[:Et])
        assert torch.equal(mine["seg"][:ng + 1], theirs.seg_start[:ng + 1])
        assert torch.equal(mine["ukeys"][:ng], theirs.ukeys[:ng])
    assert torch.equal(dv.ix[:Et], ref.ix) and torch.equal(dv.jx[:Et], ref.jx)


@torch.no_grad()
def test_upd_linear_matches_fp32_torch():
    """SoftAgg's `h` Linear on the group table (csrc/update_mlp.hip::upd_linear_kernel) against plain fp32 torch on the
    fp16-rounded operands; rows at and past the device-side row count are left alone"""
    from rampvo_amd import _lib
    from rampvo_amd.update_fused import pack_linear_f16
    torch.manual_seed(3)
    rows, live = 1000, 933
    x = torch.randn(rows, 384, device="cuda").half()
    lin = torch.nn.Linear(384, 384).cuda()
    y = torch.full((rows, 384), 7.0, device="cuda").half()
    nd = torch.tensor([live], dtype=torch.int32, device="cuda")
    # (a direct call: a freshly packed Linear and a poisoned output, not the module's operands)
    _lib.check(_lib.lib().ramp_upd_linear(_lib.ptr(x), _lib.ptr(pack_linear_f16(lin.weight)),
                                          _lib.ptr(lin.bias.detach().half().float().contiguous()), _lib.ptr(y), rows,
                                          _lib.ptr(nd), _lib.stream()), "ramp_upd_linear")
    ref = x.float() @ lin.weight.detach().half().float().t() + lin.bias.detach().half().float()
    err = (y[:live].float() - ref[:live]).abs().max().item()
    assert err <= 2e-3 * ref.abs().max().item(), err
    assert bool((y[live:] == 7.0).all())


@torch.no_grad()
def test_geometry_kernels_are_bit_stable_next_to_the_conv_towers():
    """The hazard behind -fno-slp-vectorize (tools/mb/pk_hazard.hip): per-lane fp32 kernels whose
    arithmetic the SLP vectoriser had packed (v_pk_*_f32) returned rounding-level-wrong values in 1-20 % of their launches
    while conv_tile_f16_kernel ran on another stream.  The library is built without packed fp32; this is the
    driver-visible guard: pops.transform and fastba.BA on static inputs, 200 launches each, bit-equal to their first
    run while the 1x1 / 3x3 tower layers replay from a hipGraph on a side stream."""
    from rampvo_amd import conv_hip, fastba, ops
    from rampvo_amd.synthetic import make_network
    rng = np.random.default_rng(5)
    s = ba_scene(seed=11, n_frames=16, M=96, lifetime=8, n_total_frames=20)
    poses0, patches0 = cu(s["poses"]), cu(s["patches"])
    intr, target, weight, lmbda = cu(s["intr"]), cu(s["target"]), cu(s["weight"]), cu(s["lmbda"])
    ii, jj, kk = cu(s["ii"]), cu(s["jj"]), cu(s["kk"])
    enc = make_network("SingleScale").patchify.encoder.imap_encoder
    x32 = torch.randn(240, 320, 32, device="cuda").half()
    x64 = torch.randn(120, 160, 64, device="cuda").half()
    load = lambda: [conv_hip.conv2d(x64, enc.conv2, half=True), conv_hip.conv2d(x32, enc.layer1[0].conv1, relu=True, half=True)]
    load(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        keep = [load() for _ in range(4)]
    side = torch.cuda.Stream()

    def transform():
        return ops.transform(poses0, patches0, intr, ii, jj, kk)

    def ba():
        p, pt = poses0.clone(), patches0.clone()
        ops.ba(p, pt, intr, target, weight, lmbda, ii, jj, kk, 3, 16, 2)
        return torch.cat([p.reshape(-1), pt.reshape(-1)])

    for fn in (transform, ba):
        ref = fn().clone()
        torch.cuda.synchronize()
        bad = 0
        for _ in range(200):
            with torch.cuda.stream(side):
                g.replay()
            bad += not torch.equal(fn(), ref)
        torch.cuda.synchronize()
        assert bad == 0, (fn.__name__, bad)


def test_signal_word_releases_or_times_out_the_waiting_stream():
    """the frame pipeline's gate (include/ramp_hip.h: ramp_signal_alloc / ramp_stream_wait_flag): a stream behind a
    wait for a word that is already >= the value goes on at once; a wait for a value nobody stores ends by its
    time-out instead of hanging the stream"""
    import ctypes
    import time
    from rampvo_amd import _lib, track_dev
    sig = track_dev.Signal()
    assert sig.ptr is not None                                  # MI355X supports signal memory
    side = torch.cuda.Stream()
    x = torch.zeros(1, device="cuda")
    sig.wait(side, 0)                                           # (untimed: loads the kernel, creates the stream's queue)
    with torch.cuda.stream(side):
        x += 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sig.wait(side, 0)                                           # the word is 0: satisfied
    with torch.cuda.stream(side):
        x += 1
    side.synchronize()
    quick = time.perf_counter() - t0
    t0 = time.perf_counter()
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    sig.wait(side, 7, timeout_us=20000, status=status.data_ptr())   # nobody stores 7: 20 ms, then on -- and it says so
    with torch.cuda.stream(side):
        x += 1
    side.synchronize()
    slow = time.perf_counter() - t0
    assert float(x.item()) == 2.0
    assert quick < 0.015 and 0.018 <= slow < 0.2, (quick, slow)
    assert int(status.item()) == 128                            # the time-out is recorded: whoever relied on the order raises
    assert _lib.lib().ramp_stream_wait_flag(None, None, 1, 10, 0, None) != 0        # no word: refused
