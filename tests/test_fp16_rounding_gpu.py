"""The fp16 and fp8 kernels against their own rounding, per element (tests/roundref.py).

A once-rounded output (a Linear layer, a conv layer, the correlation) must equal fp16(exact) of the float64 value on the
same rounded operands, or be the neighbour that an fp32 accumulation error of GAMMA(K) m can explain: `check_rounded`
leaves no mismatch unexplained.  The fused chains of the update operator round many times; they are held to
`roundref.Chains`, a float64 emulator with the kernels' rounding points, by the bounds below.

Chain bounds (measured on MI355X against the float64 emulator at E = 1003 / 20011 / 41003, then about doubled; the
teeth tests in test_roundref_cpu.py show every mutation outside them; roundref.py states the measured worst):
  * fp32 outputs (the residual stream, LayerNorm outputs): error / the element's local magnitude m (roundref.Chains:
    |x| + |gate * res| of the last residual step, |n||w| + |b| + |w| after a LayerNorm) <= CHAIN_FP32_MAX anywhere, and
    above 2^-14 m on at most CHAIN_FP32_FRAC of the elements.
  * SoftAgg's fp16 output (exp2 / rcp approximations inside, many rounding points): the same two measures relative to
    the magnitude of its `h` Linear's sum, with bounds of its own (SOFTAGG_MAX, SOFTAGG_FRAC).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

import roundref as rr
from scenes import corr_case

pytestmark = pytest.mark.gpu

CHAIN_FP32_MAX, CHAIN_FP32_FRAC = rr.CHAIN_FP32_MAX, rr.CHAIN_FP32_FRAC
SOFTAGG_MAX, SOFTAGG_FRAC = rr.SOFTAGG_MAX, rr.SOFTAGG_FRAC


def _ptr():
    from rampvo_amd._lib import check, lib, ptr, stream
    return check, lib, ptr, stream


# ---------------------------------------------------------------------------------------------------- upd_linear
@torch.no_grad()
def test_upd_linear_is_fp16_of_the_exact_sum():
    """csrc/update_mlp.hip::upd_linear_kernel: every live element fp16(x W^T + b) up to an explained flip; rows at and
    past the device-side row count untouched.  K = 384."""
    from rampvo_amd.update_fused import pack_linear_f16
    check, lib, ptr, stream = _ptr()
    torch.manual_seed(3)
    for rows, live in ((1000, 933), (40, 16), (37, 37)):
        x = torch.randn(rows, 384, device="cuda").half()
        x[: rows // 3] *= 1e-3                                          # small-magnitude rows
        lin = nn.Linear(384, 384).cuda()
        lin.bias[:8] *= 1e-3                                            # small biases
        w, b = lin.weight.half().float(), lin.bias.half().float()
        y = torch.full((rows, 384), 7.0, device="cuda").half()
        nd = torch.tensor([live], dtype=torch.int32, device="cuda")
        # (a direct call: a freshly packed Linear and a poisoned output, not the module's operands)
        check(lib().ramp_upd_linear(ptr(x), ptr(pack_linear_f16(lin.weight)), ptr(b.contiguous()), ptr(y), rows, ptr(nd),
                                    stream()), "ramp_upd_linear")
        ex, m = rr.linear_ref(x[:live], w, b)
        rr.check_rounded(y[:live], ex, m, "fp16", 384, "upd_linear rows=%d live=%d" % (rows, live))
        assert bool((y[live:] == 7.0).all())


# ---------------------------------------------------------------------------------------------------- the chains
def _setup():
    from rampvo_amd.synthetic import make_network
    net = make_network("SingleScale")
    fu = net.update.fused(torch.float16)
    return fu, fu.weights(), rr.Chains(net.update), net.update


@pytest.mark.parametrize("E", [1003, 20011, 41003])
@torch.no_grad()
def test_fused_chains_against_the_rounding_emulator(E):
    """every fp16 chain of the update operator against roundref.Chains: single-rounding outputs (fg, the heads' Linear)
    by check_rounded, fp32 outputs and SoftAgg by the elementwise bounds, fp16 copies of fp32 state bit for bit.
    The instantiations each E reaches on a 256-CU MI355X (update_mlp.hip: ramp_i_upd_gru's row choice, use_big):
    E = 1003: upd_gru_kernel<4> (64 rows), the 64-row upd_nbr / upd_fg kernels; E = 20011: upd_gru_kernel<5> (80 rows),
    upd_nbr_big_kernel with NMT = 5 (80 rows), upd_fg_big_kernel with NMT = 6 (96 rows); E = 41003: upd_gru_kernel<4> again and the same
    big kernels, with other partial last tiles.  upd_corr_mlp (64 rows), SoftAgg (80 sorted positions per workgroup)
    and the heads have one instantiation each; none of the E is a multiple of a tile."""
    fu, w, emu, upd = _setup()
    g = torch.Generator().manual_seed(17)
    rnd = lambda *s, sc=0.5: (torch.randn(*s, generator=g) * sc).cuda()
    G = 57
    measured = {}

    def fp32(name, got, val_mag):
        measured[name] = rr.check_fp32(got, val_mag[0], val_mag[1], CHAIN_FP32_MAX, CHAIN_FP32_FRAC, "%s E=%d" % (name, E))

    # --- upd_gru (with the prologue, then without), relu copy, heads in the epilogue
    x32, hy = rnd(E, 384), rnd(G, 384).half()
    gid = torch.randint(0, G, (E,), generator=g).int().cuda()
    out32, relu_t = fu.gru(x32, add=(hy, gid))
    o, mag, _ = emu.gru(x32, hy.float()[gid.long()])
    fp32("gru", out32, (o, mag))
    assert torch.equal(relu_t, torch.relu(out32).half())
    if E == 1003:
        strict = rr.Chains(upd, strict_autocast=True).gru(x32, hy.float()[gid.long()])
        print("  (gru against autocast's rounded gate * res product, for the record: worst %.2e, frac %.4f)"
              % rr.fp32_report(out32, strict[0], strict[1]))
    coords0 = torch.zeros(E, 2, 3, 3, device="cuda")
    out32_h, htarget, hweight = fu.gru(x32, add=(hy, gid), heads_at=(coords0, 1e9, 1e9))
    assert torch.equal(out32_h, out32)
    _heads_check("gru_heads E=%d" % E, relu_t, htarget[0], hweight[0], upd)

    ln1 = w["ln1"]
    xin = torch.nn.functional.layer_norm(x32 + hy.float()[gid.long()], (384,), ln1[0], ln1[1], float(ln1[2]))
    out32, relu_t = fu.gru(xin)
    o, mag, _ = emu.gru(xin, prologue=False)
    fp32("gru_noprologue", out32, (o, mag))
    assert torch.equal(relu_t, torch.relu(out32).half())

    # --- upd_nbr c1 / c2
    net_in = rnd(E, 384)
    idx = torch.randint(-1, E, (E,), generator=g).cuda()
    idx[::5] = -1
    for name, seq in (("c1_pack", upd.c1), ("c2_pack", upd.c2)):
        on, ot = fu.nbr(net_in, idx, name[:2], want_t=True)
        fp32("nbr_" + name[:2], on, emu.nbr(net_in, idx, seq))
        assert torch.equal(ot, on.half())

    # --- upd_corr_mlp, with a state and with a zero state
    corr = torch.nn.functional.pad(rnd(E, 882, sc=2.0).half(), (0, 14)).contiguous()
    state = rnd(700, 384)
    net_map = torch.randint(-1, 700, (E,), generator=g).cuda()
    net_map[-3:] = 699
    table = rnd(300, 384).half()
    inp_idx = torch.randint(0, 5000, (E,), generator=g).cuda()
    oc = fu.corr_mlp(corr, state, net_map, table, inp_idx, 300)
    fp32("corr_mlp", oc, emu.corr_mlp(corr[:, :882].float(), state, net_map, table.float(), inp_idx, 300))
    ctx = rnd(E, 384).half()
    oc = fu.corr_mlp(corr, None, None, ctx, None, 0)
    fp32("corr_mlp_zero_state", oc, emu.corr_mlp(corr[:, :882].float(), None, None, ctx.float(), None, 0))

    # --- upd_fg: x written back bit for bit, [f | g] = one Linear each, rounded once (K = 384)
    for name, agg in (("kk_fg_pack", upd.agg_kk), ("ij_fg_pack", upd.agg_ij)):
        xs = x32.clone()
        fg = fu.fg(xs, hy, gid, w[name], E)
        xe = x32 + hy.float()[gid.long()]
        assert torch.equal(xs, xe)
        for part, lin in ((0, agg.f), (1, agg.g)):
            ex, m = rr.linear_ref(xe.half(), lin.weight.half(), lin.bias.half())
            rr.check_rounded(fg[:, 384 * part:384 * (part + 1)], ex, m, "fp16", 384, "fg_%s[%d] E=%d" % (name[:2], part, E))

    # --- SoftAgg (upd_softagg + upd_softagg_finish), with and without the expand-and-add
    from rampvo_amd import ops
    keys = torch.repeat_interleave(torch.arange(E), torch.randint(1, 41, (E,), generator=g))[:E]
    keys = keys[torch.randperm(E, generator=g)].cuda()
    grp = ops.group_by(keys)
    NG = int(grp.ngroups.item())
    inv = grp.gid[:E].long()
    for add in (False, True):
        got = fu.softagg(x32, hy if add else None, gid if add else None, w["kk_fg_pack"], w["kk_h_pack"], grp, NG + 5, E)
        assert float(got[NG:].abs().max()) == 0.0
        xe = x32 + hy.float()[gid.long()] if add else x32
        val, mag = emu.softagg(xe, upd.agg_kk, inv, NG)
        measured["softagg_add%d" % add] = rr.check_fp32(got[:NG], val, mag, SOFTAGG_MAX, SOFTAGG_FRAC,
                                                        "softagg_add%d E=%d" % (add, E))

    # --- ramp_upd_heads_linear on a relu'd fp16 input
    relu_in = torch.relu(rnd(E, 384)).half()
    target, weight = fu.heads_linear(relu_in, coords0, 1e9, 1e9)
    _heads_check("heads_linear E=%d" % E, relu_in, target[0], weight[0], upd)
    print("E=%d measured:" % E, measured)


def _heads_check(name, relu_t, target, weight, upd):
    """coords = 0, image 1e9 x 1e9: target = the d head's fp16 output itself (one rounding of a K = 384 sum), weight =
    fp16(sigmoid(fp16 w head)) where the target is inside (x, y >= 0).  The weight's one-ulp slack is derived: the
    kernel's sigmoid is 1 / (1 + expf(-o)) in fp32, a few fp32 ulps from the exact value, so its fp16 rounding can land
    on the neighbour of fp16(exact sigmoid) and no further (a few fp32 ulps are far below one fp16 ulp)."""
    ex, m = rr.linear_ref(relu_t, upd.d[1].weight.half(), upd.d[1].bias.half())
    rr.check_rounded(target, ex, m, "fp16", 384, name + " d")
    exw, mw = rr.linear_ref(relu_t, upd.w[1].weight.half(), upd.w[1].bias.half())
    inside = (target >= 0).all(-1, keepdim=True)
    # the w head's own rounding is checked through the sigmoid: the weight must be fp16(sigmoid(o)) for an o that is
    # fp16(exact) or an explained neighbour -- i.e. between the sigmoids of the two extreme candidates
    lo = rr.round_to(exw - rr.GAMMA(384) * mw)
    hi = rr.round_to(exw + rr.GAMMA(384) * mw)
    wlo, whi = rr.round_to(torch.sigmoid(lo)), rr.round_to(torch.sigmoid(hi))
    one = rr.ulp_of(whi)
    wv = weight.double()
    ok = torch.where(inside, (wv >= wlo - one) & (wv <= whi + one), wv == 0)
    print("%-34s weight: %d of %d inside, all within [sigmoid(lo), sigmoid(hi)] +- 1 ulp" % (name, int(inside.sum()),
                                                                                          inside.numel()))
    assert bool(ok.all()), (name, int((~ok).sum()))


# ---------------------------------------------------------------------------------------------------- conv layers
F16_CONV_CASES = [(16, 32, 7, 2, (48, 64), True), (32, 32, 3, 1, (37, 53), False), (32, 64, 3, 2, (40, 56), False),
                  (64, 64, 3, 1, (20, 28), False), (32, 64, 1, 2, (40, 56), False), (64, 384, 1, 1, (21, 29), False)]
IN_STATS_TOL = 6e-7          # |mean - mean64| / rms and |var - var64| / mean square; measured on MI355X over these six
                             # layers: mean <= 5.5e-8, var <= 3.0e-7 (bound about 2x the larger)


@pytest.mark.parametrize("cin,cout,k,stride,hw,first", F16_CONV_CASES)
@torch.no_grad()
def test_conv_f16_is_fp16_of_the_exact_sum(cin, cout, k, stride, hw, first):
    """test_conv_mfma_f16_matches_torch's layers: the plain output, the normalise-and-ReLU prologue (the kernel rounds
    the normalised input to half; the first layer its fp32 input) and the residual + ReLU + scale epilogue, each
    fp16(exact) up to explained flips; the InstanceNorm statistics against fp64 relative to the sum of squares; the
    materialised map bit for bit against its fp32 expression on the kernel's own raw output and statistics"""
    from rampvo_amd import conv_hip
    torch.manual_seed(2)
    real_cin = 15 if cin == 16 else cin
    conv = nn.Conv2d(real_cin, cout, k, stride=stride, padding=k // 2).cuda()
    conv.weight.copy_(conv.weight.half().float())
    conv.bias.copy_(conv.bias.half().float())
    conv.bias[:4] *= 1e-3                                   # small biases: a dropped one must show
    K = real_cin * k * k
    x = torch.randn(hw[0], hw[1], cin, device="cuda")
    x[::4] *= 1e-2                                          # small-magnitude outputs
    if not first:
        x = x.half().float()
    if cin == 16:
        x[..., 15] = 0
    xin = x if first else x.half()
    xr = x.half().float()                                   # the operand the kernel multiplies
    name = "conv f16 %dx%d %d->%d s%d" % (k, k, cin, cout, stride)
    ex, m = rr.conv_ref(xr, conv.weight, conv.bias, stride, k // 2)
    y = conv_hip.conv2d(xin, conv, half=True)
    rr.check_rounded(y, ex, m, "fp16", K, name)
    # prologue: relu(x * sc + sh) in fp32 (no contraction: -ffp-contract=off), rounded to half
    sc, sh = torch.rand(cin, device="cuda") + 0.5, torch.randn(cin, device="cuda") * 0.1
    xq = torch.relu(xin.float() * sc + sh).half().float()
    if cin == 16:
        xq[..., 15] = 0
    res = torch.randn(ex.shape, device="cuda").half()
    ex2, m2 = rr.conv_ref(xq, conv.weight, conv.bias, stride, k // 2)
    y2 = conv_hip.conv2d(xin, conv, pre=(sc, sh), half=True)
    rr.check_rounded(y2, ex2, m2, "fp16", K, name + " prologue")
    # epilogue: fp16(relu(relu(conv) + res) * 0.25)
    y3 = conv_hip.conv2d(xin, conv, pre=(sc, sh), res=res, relu=True, out_scale=0.25, half=True)
    ex3 = torch.relu(torch.relu(ex2) + res.double()) * 0.25
    rr.check_rounded(y3, ex3, (m2 + res.double().abs()) * 0.25, "fp16", K + 2, name + " epilogue")
    # InstanceNorm statistics of the raw fp32 output
    p = conv_hip.conv2d(xin, conv, want_stats=True, half=True)
    mean, ms = ex.mean((0, 1)), (ex * ex).mean((0, 1))
    var = ex.var((0, 1), unbiased=False)
    mk = -p.shift.double() / p.scale.double()
    vk = 1.0 / p.scale.double() ** 2 - 1e-5
    em = float(((mk - mean).abs() / ms.sqrt()).max())
    ev = float(((vk - var).abs() / (ms + 1e-5)).max())
    print("%-34s IN stats: mean %.2e, var %.2e of the sum of squares (bound %.0e)" % (name, em, ev, IN_STATS_TOL))
    assert em <= IN_STATS_TOL and ev <= IN_STATS_TOL, (em, ev)
    mat = conv_hip.materialize(p)
    assert torch.equal(mat, torch.relu(p.raw.float() * p.scale + p.shift).half())
    assert float((mat.float() - torch.relu(torch.nn.functional.instance_norm(
        ex.float().permute(2, 0, 1)[None], eps=1e-5))[0].permute(1, 2, 0)).abs().max()) <= 1e-2


def _fp16_edge_values(device):
    """fp32 values: fp16 ties (the midpoints of consecutive fp16 numbers), both sides of the normal / subnormal boundary,
    subnormals, and the top of the range up to 65519 (which still rounds to 65504)"""
    allh = torch.arange(0, 0x7BFF, dtype=torch.int32).to(torch.int16).view(torch.half).double()
    mids = 0.5 * (allh[:-1] + allh[1:])
    pick = torch.cat([mids[:1100], mids[0x0380:0x0480], mids[-600:], mids[torch.randperm(mids.numel())[:3000]]])
    near = torch.tensor([6.103515625e-05, 6.1e-05, 6.11e-05, 6.0975552e-05, 5.9604645e-08, 2.98e-08, 2.99e-08,
                         65504.0, 65519.0, 65519.99, 65488.0, 65500.0, 1e-9, 0.0], dtype=torch.float64)
    pf = pick.float()
    v = torch.cat([pf, near.float(), pf.nextafter(torch.zeros_like(pf))])
    v = torch.cat([v, -v])
    return v.to(device)


@torch.no_grad()
def test_conv_f16_first_layer_converts_fp32_input_like_torch_half():
    """the fp32-input first layer (conv.hip IN_F32 path) with one-hot power-of-two weights at the centre tap: output
    channel o = x[channel o % 15] * 2^s(o), s in {-1, 0, 1} -- the operand the kernel multiplied.  Every fp16 tie, the
    normal / subnormal boundary and 65504 / 65519 must convert as torch's .half() does"""
    from rampvo_amd import conv_hip
    v = _fp16_edge_values("cuda")
    H, W, cout = 48, 64, 32
    npix = (H // 2) * (W // 2) * 15
    vals = v.repeat((npix + v.numel() - 1) // v.numel())[:npix]
    x = torch.zeros(H, W, 16, device="cuda")
    x[::2, ::2, :15] = vals.reshape(H // 2, W // 2, 15)
    conv = nn.Conv2d(15, cout, 7, stride=2, padding=3).cuda()
    conv.weight.zero_()
    conv.bias.zero_()
    s = torch.tensor([2.0 ** ((o % 3) - 1) for o in range(cout)], device="cuda")
    for o in range(cout):
        conv.weight[o, o % 15, 3, 3] = s[o]
    y = conv_hip.conv2d(x, conv, half=True)
    src = x[::2, ::2, [o % 15 for o in range(cout)]]
    exp = rr.round_to(src.half().double() * s.double())
    same = (y.double() == exp) | (torch.isnan(exp) & torch.isnan(y.double()))
    print("f16 first-layer conversion: %d edge values x 3 scales, %d mismatches" % (vals.numel(), int((~same).sum())))
    assert bool(same.all()), (src[~same][:8].tolist(), y[~same][:8].tolist(), exp[~same][:8].tolist())


def _e4m3_edge_values(device):
    """fp16 activations whose x * FP8_ACT_SCALE hits every e4m3 value, every tie between neighbours (subnormal ties
    included), and the +-448 saturation edge (448 / 8 = 56 and above)"""
    e = torch.arange(0, 0x7F, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).double()   # 0 .. 448
    mids = 0.5 * (e[:-1] + e[1:])
    sat = torch.tensor([448.0, 456.0, 464.0, 465.0, 480.0, 500.0, 4000.0, 65504.0 * 8], dtype=torch.float64)
    v = torch.cat([e, mids, sat]) / rr.FP8_ACT_SCALE
    v = torch.cat([v, -v])
    assert torch.equal(v.half().double(), v)                 # all representable in fp16
    return v.to(device)


@torch.no_grad()
def test_conv_fp8_conversion_matches_torch_e4m3fn_bit_for_bit():
    """the fp8 path (RAMP_CONV_FP8, __builtin_amdgcn_cvt_pk_fp8_f32, conv.hip:627) through a 1x1 conv with one-hot unit
    weights: output channel o = e4m3(clamp(x * 8, +-448)) / 8 of input channel o % 32, which must equal torch's
    float8_e4m3fn conversion of the clamped value for every e4m3 value, tie, subnormal and the saturation edge"""
    from rampvo_amd import conv_hip
    v = _e4m3_edge_values("cuda")
    H, W, cin = 40, 56, 32
    npix = (H // 2) * (W // 2) * cin
    vals = v.repeat((npix + v.numel() - 1) // v.numel())[:npix]
    x = torch.zeros(H, W, cin, device="cuda").half()
    x[::2, ::2] = vals.reshape(H // 2, W // 2, cin).half()
    convs = [nn.Conv2d(cin, 64, 1, stride=2).cuda() for _ in range(2)]
    for c in convs:
        c.weight.zero_()
        c.bias.zero_()
        for o in range(64):
            c.weight[o, o % 32, 0, 0] = 1.0
    out = conv_hip.conv2d_towers([dict(x=x, conv=convs[0]), dict(x=x, conv=convs[1])], half=True, fp8=True)
    src = x[::2, ::2][..., [o % 32 for o in range(64)]].float()
    t = (src * rr.FP8_ACT_SCALE).clamp(-448, 448)
    exp = t.to(torch.float8_e4m3fn).float() / rr.FP8_ACT_SCALE
    assert torch.equal(rr.e4m3(src, rr.FP8_ACT_SCALE).float() / rr.FP8_ACT_SCALE, exp)      # roundref's e4m3 = torch's
    for y in out:
        same = y.float() == exp
        print("fp8 conversion: %d edge values, %d mismatches" % (vals.numel(), int((~same).sum())))
        assert bool(same.all()), (src[~same][:8].tolist(), y[~same][:8].tolist(), exp[~same][:8].tolist())


FP8_CASES = [(32, (32, 32), 3, 1, (37, 53)), (32, (64, 64), 3, 2, (40, 56)), (64, (64, 64), 3, 1, (30, 44)),
             (32, (64, 64), 1, 2, (40, 56)), (64, (128, 384), 1, 1, (21, 29)), (128, (128, 384), 1, 1, (19, 35))]


@pytest.mark.parametrize("cin,couts,k,stride,hw", FP8_CASES)
@torch.no_grad()
def test_conv_fp8_layer_is_fp16_of_the_exact_sum(cin, couts, k, stride, hw):
    """test_conv_fp8_mfma_layer_against_fp32_on_rounded_operands's layers: e4m3 products are exact in fp32, so the
    output (prologue + bias for tower 0, ReLU + residual + scale for tower 1) is fp16(exact) of the same e4m3 operands
    up to explained flips (the 1x1 layers with K < roundref.FP8_K_SMALL take their bound at FP8_K_MIN: measured)"""
    from rampvo_amd import conv_hip
    torch.manual_seed(7)
    convs = [nn.Conv2d(cin, c, k, stride=stride, padding=k // 2).cuda() for c in couts]
    for c in convs:
        c.bias.copy_(c.bias.half().float())
    x = (torch.randn(hw[0], hw[1], cin, device="cuda") * 1.5).half()
    sc, sh = torch.rand(cin, device="cuda") + 0.5, torch.randn(cin, device="cuda") * 0.1
    oh, ow = (hw[0] + 2 * (k // 2) - k) // stride + 1, (hw[1] + 2 * (k // 2) - k) // stride + 1
    res = torch.randn(oh, ow, couts[1], device="cuda").half()
    jobs = [dict(x=conv_hip.Pending(x, sc, sh), conv=convs[0], want_stats=True),
            dict(x=x, conv=convs[1], relu=True, res=res, out_scale=0.25)]
    out = conv_hip.conv2d_towers(jobs, half=True, fp8=True)
    K = rr.fp8_K(cin * k * k)

    def ref(xin, conv):
        a = rr.FP8_ACT_SCALE
        xq = rr.e4m3(xin, a)                                  # scaled e4m3 values
        ws = float(np.float32(448.0 / float(conv.weight.abs().max())))
        wq = (conv.weight.float() * ws).clamp(-448, 448).to(torch.float8_e4m3fn).double()   # conv_hip.pack_conv_weight
        ex, m = rr.conv_ref(xq, wq, None, conv.stride, conv.padding)
        d = 1.0 / (a * ws)
        b = conv.bias.double()
        return ex * d + b, m * d + b.abs()
    e0, m0 = ref(torch.relu(x.float() * sc + sh), convs[0])
    e1, m1 = ref(x.float(), convs[1])
    name = "conv fp8 %dx%d %d->%s s%d" % (k, k, cin, couts, stride)
    rr.check_rounded(out[0].raw, e0, m0, "fp16", K, name + " t0")
    rr.check_rounded(out[1], torch.relu(torch.relu(e1) + res.double()) * 0.25, (m1 + res.double().abs()) * 0.25,
                     "fp16", K + 2, name + " t1")


# ---------------------------------------------------------------------------------------------------- correlation
@pytest.mark.parametrize("case", ["narrow", "wide", "ring_padded"])
@torch.no_grad()
def test_corr_half_is_fp16_of_the_fp32_accumulated_sum(case):
    """corr_mfma_kernel<half>: both pyramid levels, every output fp16(exact) of the float64 correlation (dot products over
    C = 128, bilinear blend) on the fp16 features up to explained flips (K = C + 8: the blend's weights and adds);
    zero (off-image) positions exactly zero.  ring_padded: edge indices past the buffers wrapped inside the kernel
    (mod_ii / mod_jj), target-frame-major schedule, 896-wide padded rows"""
    from rampvo_amd import ops
    from rampvo_amd._lib import RAMP_NHWC
    N1, N2 = 40, 6
    E = {"narrow": 64, "wide": 64, "ring_padded": 93}[case]
    fmap1, fmap2, coords, ii, jj = corr_case(seed={"narrow": 8, "wide": 8, "ring_padded": 21}[case], E=E, N1=N1, N2=N2,
                                             wide=case == "wide")
    fmap2b = np.ascontiguousarray(fmap2[:, :, :, ::2, ::2])
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    f1h = cu(fmap1[0]).half()
    f2h = [cu(fmap2[0]).half(), cu(fmap2b[0]).half()]
    kw = {}
    ii_k, jj_k = ii, jj
    if case == "ring_padded":
        rng = np.random.default_rng(5)
        ii_k = (ii + N1 * rng.integers(0, 3, E)).astype(np.int64)
        jj_k = (jj + N2 * rng.integers(0, 3, E)).astype(np.int64)
        kw = dict(order=torch.argsort(cu(jj_k), stable=True).int(), row_elems=896, mod_ii=N1, mod_jj=N2)
    out = ops.corr(f1h.permute(0, 2, 3, 1).contiguous(), [f.permute(0, 2, 3, 1).contiguous() for f in f2h],
                   cu(coords[0]), cu(ii_k), cu(jj_k), 3, (1.0, 4.0), RAMP_NHWC, **kw)
    assert out.dtype == torch.float16
    if case == "ring_padded":
        assert float(out[:, 882:].abs().max()) == 0.0
        out = out[:, :882]
    out = out.reshape(E, 7, 7, 3, 3, 2)
    for lvl, div in ((0, 1.0), (1, 4.0)):
        ex, m = rr.corr_ref(f1h, f2h[lvl], cu(coords[0]).double() / div, cu(ii).long(), cu(jj).long(), 3)
        y = out[..., lvl]
        dead = m == 0
        assert bool((y[dead] == 0).all()), "off-image positions must be exactly zero"
        rr.check_rounded(y, ex, m, "fp16", 128 + 8, "corr half %s level %d" % (case, lvl))
