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
