"""CPU tests of tests/roundref.py: its rounding functions against torch's conversions, and that its checks have teeth --
correct results computed another way are accepted, every mutation a fp16 kernel could plausibly carry is rejected, and
(for the record) the old max-scaled tolerances accept the mutations they cannot see."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import roundref as rr

OLD_TOL = 2e-3               # test_conv_mfma_f16_matches_torch / test_upd_linear_matches_fp32_torch: x the output's max


def _old_ok(y, exact):
    return float((y.double() - exact).abs().max()) <= OLD_TOL * float(exact.abs().max())


def _bad(y, exact, m, K):
    return rr.rounding_report(y, exact, m, "fp16", K)["bad"]


def test_rounding_functions_match_torch():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 18, generator=g) * torch.exp(torch.randn(1 << 18, generator=g) * 4)
    assert torch.equal(rr.fp16(x), x.half().float())
    allh = torch.arange(0, 0x7C00, dtype=torch.int32).to(torch.int16).view(torch.half).float()
    mids = 0.5 * (allh[:-1] + allh[1:])                     # every positive fp16 tie
    for v in (mids, -mids, mids.nextafter(torch.zeros_like(mids)), torch.tensor([65519.99, 65520.0, 7e4])):
        assert torch.equal(rr.fp16(v), v.half().float())
    e = torch.arange(0, 0x7F, dtype=torch.int32).to(torch.uint8).view(torch.float8_e4m3fn).double()
    t = torch.cat([e, 0.5 * (e[:-1] + e[1:]), torch.tensor([449.0, 464.0, 465.0, 1e4])])
    t = torch.cat([t, -t]).float()
    assert torch.equal(rr.e4m3(t).float(), t.clamp(-448, 448).to(torch.float8_e4m3fn).float())


def _linear_case():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(256, 384, generator=g).half().float()
    x[:64] *= 1e-3
    lin = nn.Linear(384, 384)
    with torch.no_grad():
        lin.bias[:4] = torch.tensor([3e-3, -2e-3, 1e-3, -3.5e-3])
    w, b = lin.weight.detach().half().float(), lin.bias.detach().half().float()
    return x, w, b


def test_check_rounded_accepts_correct_linears_and_rejects_mutations():
    x, w, b = _linear_case()
    ex, m = rr.linear_ref(x, w, b)
    K = 384
    correct = {
        "fp32 GEMM": (x @ w.t() + b).half(),
        "fp32, K reversed, bias first": (b + x.flip(1) @ w.flip(1).t()).half(),
        "torch CPU half F.linear": F.linear(x.half(), w.half(), b.half()),
    }
    for name, y in correct.items():
        assert _bad(y, ex, m, K) == 0, name
    acc = x @ w.t()
    drop = acc.clone()
    drop[16:32] -= x[16:32, 32:64] @ w[:, 32:64].t()        # one 32-wide K step of one 16-row tile
    bsmall = torch.where(b.abs() < 4e-3, torch.zeros_like(b), b)
    mutants = {
        "rounded toward zero": rr.round_to(acc + b, "fp16", "rtz").half(),
        "small biases dropped": (acc + bsmall).half(),
        "extra rounding before the bias": ((acc.half().float()) + b).half(),
        "one K step dropped in one tile": (drop + b).half(),
    }
    for name, y in mutants.items():
        rep = rr.rounding_report(y, ex, m, "fp16", K)
        assert rep["bad"] > 0, name
        print("linear mutant %-32s unexplained %6d of %d; old tolerance %s" % (name, rep["bad"], rep["n"],
                                                                            "accepts" if _old_ok(y, ex) else "rejects"))
    # the record: the old max-scaled bound cannot see these
    for name in ("rounded toward zero", "small biases dropped", "extra rounding before the bias"):
        assert _old_ok(mutants[name], ex), name


def test_check_rounded_accepts_a_correct_conv_and_rejects_mutations():
    g = torch.Generator().manual_seed(2)
    conv = nn.Conv2d(64, 64, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(conv.weight.half().float())
        conv.bias.copy_(conv.bias.half().float())
        conv.bias[:4] = torch.tensor([2e-3, -1e-3, 3e-3, -2.5e-3])
    x = torch.randn(20, 28, 64, generator=g).half().float()
    ex, m = rr.conv_ref(x, conv.weight.detach(), conv.bias.detach(), 1, 1)
    K = 64 * 9
    with torch.no_grad():
        nchw = x.permute(2, 0, 1)[None]
        raw = F.conv2d(nchw, conv.weight, None, 1, 1)[0].permute(1, 2, 0)
        y = (raw + conv.bias).half()
        wt = conv.weight.clone()
        wt[:, 5, 1, 2] = 0                                   # one (input channel, tap) dropped
        tap = (F.conv2d(nchw, wt, conv.bias, 1, 1)[0].permute(1, 2, 0)).half()
        bsmall = torch.where(conv.bias.abs() < 4e-3, torch.zeros_like(conv.bias), conv.bias)
    assert _bad(y, ex, m, K) == 0
    mutants = {"rounded toward zero": rr.round_to(raw + conv.bias, "fp16", "rtz").half(),
               "small biases dropped": (raw + bsmall).half(), "one (channel, tap) dropped": tap}
    for name, yy in mutants.items():
        rep = rr.rounding_report(yy, ex, m, "fp16", K)
        assert rep["bad"] > 0, name
        print("conv mutant %-28s unexplained %6d of %d; old tolerance %s" % (name, rep["bad"], rep["n"],
                                                                          "accepts" if _old_ok(yy, ex) else "rejects"))
    assert _old_ok(mutants["rounded toward zero"], ex) and _old_ok(mutants["small biases dropped"], ex)


# ------------------------------------------------------------------- the conv towers' tiled kernel (test_conv_instances_gpu.py)
def _acc_of(x, tile_rows=8, tile_cols=16, R=8):
    """the accumulators a layer leaves for its raw output x [H, W, C] (csrc/conv.hip::conv_tile_epilogue): per 8 x 16 tile
    the fp32 sums of x and x^2, as 2^-20 fixed-point integers, added to replica (tile index % R) -> [R][C][2] int64"""
    H, W, C = x.shape
    acc = torch.zeros(R, C, 2, dtype=torch.int64)
    t = 0
    for y0 in range(0, H, tile_rows):
        for x0 in range(0, W, tile_cols):
            v = x[y0:y0 + tile_rows, x0:x0 + tile_cols].float().reshape(-1, C)
            s = torch.stack([v.sum(0), (v * v).sum(0)], dim=1)
            acc[t % R] += torch.round(s.double() * rr.IN_ACC_ONE).to(torch.int64)
            t += 1
    return acc


def _tail_case():
    g = torch.Generator().manual_seed(5)
    H, W, C = 11, 19, 32                                     # two tile rows, two tile columns, both ragged
    y = (torch.randn(H, W, C, generator=g) * 0.6 + 0.2).half()
    skip = (torch.randn(H, W, C, generator=g) * 0.8 - 0.1).half()
    return y, skip, _acc_of(y), _acc_of(skip), float(H * W)


def test_accumulator_statistics_and_tail_pixel_match_a_plain_torch_evaluation():
    """roundref.acc_stats / tail_ref on a tiny map against F.instance_norm and the written-out expression in float64: the
    statistics agree to the accumulators' resolution (2^-21 per tile and sum, 4 tiles over 209 pixels), the tail pixel
    formed with torch's own statistics to that resolution times the scale"""
    y, skip, acc_y, acc_s, n = _tail_case()
    C = y.shape[-1]
    mean, var, sc, sh = rr.acc_stats(acc_y, C, n, 1e-5)
    yd = y.double()
    res = 4 * 2.0 ** -21 / n
    assert float((mean - yd.mean((0, 1))).abs().max()) <= res + 1e-7 * float(yd.abs().max())     # (+ the tiles' fp32 sums)
    assert float((var - yd.var((0, 1), unbiased=False)).abs().max()) <= 4 * res + 1e-6
    assert torch.equal(sh, -mean * sc) and float((sc - 1.0 / torch.sqrt(var + float(torch.tensor(1e-5)))).abs().max()) == 0.0
    norm = lambda t: F.instance_norm(t.double().permute(2, 0, 1)[None], eps=1e-5)[0].permute(1, 2, 0)
    _, _, s2, h2 = rr.acc_stats(acc_s, C, n, 1e-5)
    forms = {
        "tensor": (rr.tail_ref(y, sc, sh, skip), torch.relu(torch.relu(norm(y)) + skip.double())),
        "norm": (rr.tail_ref(y, sc, sh, skip, s2, h2), torch.relu(torch.relu(norm(y)) + norm(skip))),
        "norm_relu": (rr.tail_ref(y, sc, sh, skip, s2, h2, skip_relu=True),
                      torch.relu(torch.relu(norm(y)) + torch.relu(norm(skip)))),
    }
    for name, ((e, m), plain) in forms.items():
        tol = 2e-5 if name != "norm_relu" else 2e-5 + 2.0 ** -11 * float(plain.max())     # (the inner fp16 rounding)
        assert float((e - plain).abs().max()) <= tol, name
        assert bool((m >= e.abs() - 1e-12).all()), name
    # the prologue's operand
    e, m = rr.norm_relu_ref(y, sc, sh)
    assert float((e - torch.relu(norm(y))).abs().max()) <= 2e-5 and bool((m >= e).all())


def test_tail_reference_accepts_the_fp32_evaluation_and_rejects_its_defects():
    """the tail pixel as the kernels form it (fp32 scale and shift from the accumulators, fp32 arithmetic, one rounding to
    fp16; the normalised-and-ReLU'd skip rounded once more) is accepted with zero unexplained elements by the float64
    reference alone; without the inner ReLU, or with the skip's normalisation dropped, it is rejected -- by check_rounded
    and by the bit equality with the unfused kernel's output that the GPU test also asserts"""
    y, skip, acc_y, acc_s, n = _tail_case()
    C = y.shape[-1]
    _, _, sc, sh = rr.acc_stats(acc_y, C, n, 1e-5)
    _, _, s2, h2 = rr.acc_stats(acc_s, C, n, 1e-5)
    f = lambda t: t.float()

    def kernel(inner_relu=True, skip_norm=True, skip_relu=False):
        a = f(y) * f(sc) + f(sh)
        if inner_relu:
            a = torch.relu(a)
        b = f(skip) * f(s2) + f(h2) if skip_norm else f(skip)
        if skip_relu:
            b = torch.relu(b).half().float()
        return torch.relu(a + b).half()
    for relu in (False, True):
        e, m = rr.tail_ref(y, sc, sh, skip, s2, h2, skip_relu=relu)
        good = kernel(skip_relu=relu)
        assert _bad(good, e, m, rr.TAIL_K) == 0
        for name, kw in (("inner ReLU skipped", dict(inner_relu=False)), ("skip's normalisation dropped", dict(skip_norm=False))):
            bad = kernel(skip_relu=relu, **kw)
            rep = rr.rounding_report(bad, e, m, "fp16", rr.TAIL_K)
            print("tail mutant %-30s (skip relu %d) unexplained %5d of %d" % (name, relu, rep["bad"], rep["n"]))
            assert rep["bad"] > 0 and not torch.equal(bad, good), name
    e, m = rr.tail_ref(y, sc, sh, skip)
    assert _bad(kernel(skip_norm=False), e, m, rr.TAIL_K) == 0          # a plain tensor skip: that IS the expression
    e, m = rr.norm_relu_ref(y, sc, sh)
    assert _bad(torch.relu(f(y) * f(sc) + f(sh)).half(), e, m, rr.NORM_K) == 0
    assert _bad((f(y) * f(sc) + f(sh)).half(), e, m, rr.NORM_K) > 0


@pytest.mark.parametrize("k,stride,hw", [(3, 1, (11, 19)), (3, 2, (21, 37)), (1, 2, (21, 37)), (7, 2, (21, 37))])
def test_conv_reference_rejects_the_tiled_kernels_defects(k, stride, hw):
    """a tiled layer emulated in fp32 on a ragged map (two tile rows, two tile columns of 8 x 16 output pixels), one defect
    at a time: the last live row of the ragged bottom tile zeroed; the halo column left of the image taken from the
    neighbouring pixel where it should be padding; one of the tiny biases (roundref.TINY_BIASES,
    the smallest) dropped.  check_rounded rejects
    each and accepts the undamaged emulation with zero unexplained elements"""
    g = torch.Generator().manual_seed(8)
    cin, cout = (15, 32) if k == 7 else (32, 32)
    conv = nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2)
    with torch.no_grad():
        conv.weight.copy_(conv.weight.half().float())
        conv.bias.copy_(conv.bias.half().float())
        conv.bias[:4] = torch.tensor(rr.TINY_BIASES).half().float()      # test_conv_instances_gpu.py::make_conv's
    w, b = conv.weight.detach(), conv.bias.detach()
    x = torch.randn(hw[0], hw[1], cin, generator=g)
    x[::4] *= 1e-2
    x = x.half().float()
    ex, m = rr.conv_ref(x, w, b, stride, k // 2)
    K = cin * k * k
    nchw = x.permute(2, 0, 1)[None]
    run = lambda inp, pad, bias: F.conv2d(inp, w, bias, stride, pad)[0].permute(1, 2, 0)
    good = run(nchw, k // 2, b).half()
    assert 8 < good.shape[0] < 16 and 16 < good.shape[1] < 32 and good.shape[0] % 8 and good.shape[1] % 16
    assert _bad(good, ex, m, K) == 0
    mutants = {}
    row = good.clone()
    row[-1] = 0
    mutants["last live row of the ragged tile zeroed"] = row
    bdrop = b.clone()
    bdrop[1] = 0                                             # the smallest of the tiny biases
    mutants["smallest tiny bias dropped"] = run(nchw, k // 2, bdrop).half()
    if k > 1:
        p = k // 2
        halo = F.pad(F.pad(nchw, (p, 0, 0, 0), mode="replicate"), (0, p, p, p))
        mutants["halo column from the neighbouring pixel"] = run(halo, 0, b).half()
    for name, y in mutants.items():
        rep = rr.rounding_report(y, ex, m, "fp16", K)
        print("conv %dx%d s%d mutant %-42s unexplained %5d of %d" % (k, k, stride, name, rep["bad"], rep["n"]))
        assert y.shape == good.shape and rep["bad"] > 0, name


@pytest.fixture(scope="module")
def gru_case():
    from rampvo_amd.synthetic import make_network
    upd = make_network("SingleScale", device="cpu").update
    g = torch.Generator().manual_seed(3)
    E = 1500
    x32 = torch.randn(E, 384, generator=g) * 0.5
    add = (torch.randn(E, 384, generator=g) * 0.5).half().float()
    return upd, x32, add, rr.Chains(upd).gru(x32, add)


def test_chain_bounds_accept_fp32_evaluation_and_reject_mutations(gru_case):
    """the gru chain: the emulator evaluated in fp32 (fp32 accumulation, the same rounding points -- what a correct
    kernel does) passes the GPU test's fp32-output bound; a skipped rounding point (res Linear output), an added one
    (autocast's rounded gate * res product), round-toward-zero everywhere and LayerNorm eps 1e-4 instead of the module's
    1e-3 all fail it -- and pass the old 3e-3 x max bound (FUSED_CHAIN_TOL)"""
    upd, x32, add, ref = gru_case
    tol, frac = rr.CHAIN_FP32_MAX, rr.CHAIN_FP32_FRAC
    o = rr.Chains(upd, torch.float32).gru(x32, add)
    worst, f = rr.fp32_report(o[0], ref[0], ref[1])
    print("gru fp32 evaluation: worst %.2e, frac %.4f (bounds %.1e, %.3f)" % (worst, f, tol, frac))
    assert worst <= tol and f <= frac
    old = lambda y: float((y.double() - ref[0]).abs().max()) <= 3e-3 * float(ref[0].abs().max())
    for name, kw in (("res output not rounded", dict(skip_r=True)), ("gate * res rounded", dict(strict_autocast=True)),
                     ("round toward zero", dict(rtz=True)), ("LayerNorm eps 1e-4", dict(eps=1e-4))):
        y = rr.Chains(upd, **kw).gru(x32, add)[0]
        worst, f = rr.fp32_report(y, ref[0], ref[1])
        print("gru mutant %-24s worst %.2e, frac %.4f; old tolerance %s" % (name, worst, f, "accepts" if old(y) else "rejects"))
        assert worst > tol or f > frac, name
        if name != "round toward zero":
            assert old(y), name


def test_softagg_bounds_accept_fp32_evaluation_and_reject_mutations(gru_case):
    """SoftAgg (upd_softagg + upd_softagg_finish) at the GPU test's grouping (E = 1003, groups of 1..40 factors): the
    emulator evaluated in fp32 passes roundref.SOFTAGG_MAX / SOFTAGG_FRAC; one factor of the last group reading another
    factor's row, and autocast's form with half softmax weights and sums (row 11 of the rounding table: it pins that
    deliberate departure) fail it; the old 3e-3 x max bound sees the first but accepts the second"""
    upd = gru_case[0]
    agg = upd.agg_kk
    g = torch.Generator().manual_seed(1003)
    E = 1003
    keys = torch.repeat_interleave(torch.arange(E), torch.randint(1, 41, (E,), generator=g))[:E]
    keys = keys[torch.randperm(E, generator=g)]
    _, inv = torch.unique(keys, return_inverse=True)
    G = int(inv.max()) + 1
    x = torch.randn(E, 384, generator=g) * 0.5
    ref, m = rr.Chains(upd).softagg(x, agg, inv, G)
    tol, frac = rr.SOFTAGG_MAX, rr.SOFTAGG_FRAC
    worst, f = rr.fp32_report(rr.Chains(upd, torch.float32).softagg(x, agg, inv, G)[0], ref, m)
    print("softagg fp32 evaluation: worst %.2e, frac %.4f (bounds %.1e, %.4f)" % (worst, f, tol, frac))
    assert worst <= tol and f <= frac
    last = (inv == G - 1).nonzero()[:, 0]
    xw = x.clone()
    xw[last[0]] = x[(inv != G - 1).nonzero()[0, 0]]          # one factor of the last group reads a wrong row
    old = lambda y: float((y.double() - ref).abs().max()) <= 3e-3 * float(ref.abs().max())
    for name, y in (("wrong row in the last group", rr.Chains(upd).softagg(xw, agg, inv, G)[0]),
                    ("half softmax weights and sums", rr.Chains(upd, strict_autocast=True).softagg(x, agg, inv, G)[0])):
        worst, f = rr.fp32_report(y, ref, m)
        print("softagg mutant %-30s worst %.2e, frac %.4f; old tolerance %s" % (name, worst, f,
                                                                             "accepts" if old(y) else "rejects"))
        assert worst > tol or f > frac, name
        assert old(y) == (name != "wrong row in the last group"), name
