"""Rounding-matched references for the fp16 and fp8 kernels, and the checks that hold them to their rounding.

A kernel that multiplies fp16 (or e4m3) operands, accumulates in fp32 and rounds its output once to fp16 has a
contract that can be checked per element: the output is fp16(exact), where `exact` is the float64 value of the same
expression on the same (already rounded) operands -- or, where the fp32 accumulation lands on the other side of a
rounding boundary, the neighbouring fp16 number.  That second case is only possible where `exact` lies within the fp32
accumulation error of the boundary.  `check_rounded` demands exactly that: every mismatch must be explained.

gamma_K (the accumulation bound).  Summing n = K + 1 terms (K products, exact in fp32 for fp16 and e4m3 operands, plus
the bias) in fp32 in any order errs by at most gamma_n * sum|terms| with gamma_n = n u / (1 - n u), u = 2^-24
(Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., eq. 4.4 / lemma 3.1).  The matrix cores' internal
adder is not documented as round-to-nearest, so the unit is taken as 2^-23 (a truncating adder) and one more term is
allowed for epilogue steps (bias, scale): GAMMA(K) = (K + 2) 2^-23.  With m = sum |x||w| + |b| (the same expression on
absolute values) the fp32 result lies within GAMMA(K) m of `exact`.

The fp16 chains of the update operator are checked against `Chains`, an emulator that evaluates the same torch
modules (rampvo_amd.synthetic.make_network's seeded weights) in float64 and rounds to fp16 at every point where the
kernels round.  Its rounding points, against what the reference's autocast does (ramp/Ramp_vo.py:23 runs the network
under torch.amp.autocast('cuda'): F.linear casts its operands to half and returns half; elementwise ops on half tensors
return half; half + fp32 promotes to fp32; layer_norm runs in fp32):

| # | rounding point | autocast (reference) | kernel | verdict |
|---|---|---|---|---|
| 1 | Linear operands x, W, b -> fp16 | F.linear casts to half | fp16 LDS tiles (to_lds, update_mlp.hip:436-442) / fp16 packed weights / fp16-valued biases | agrees |
| 2 | Linear output -> fp16 | half tensor | h_round / (_Float16) of acc + b (update_mlp.hip:463, 498, 650, 790, 836, 956, 1139, 1220, 1329, 1388, 1506, 1562) | agrees |
| 3 | gate = sigmoid(half) -> fp16 | sigmoid of a half tensor is half (ramp/blocks.py:15) | to_lds(Gs, sigm(h_round(.))) (update_mlp.hip:463-466) | agrees |
| 4 | relu(half) -> fp16 | half (ramp/blocks.py:16) | fmaxf(acc + b, 0) -> fp16 (update_mlp.hip:483 + to_lds, 636, 766) | agrees (relu commutes with rounding) |
| 5 | GatedResidual gate * res | half * half -> fp16, then fp32 x + half (ramp/blocks.py:30) | res += (float)g * h_round(r), product NOT rounded (update_mlp.hip:498) | deliberate departure: the kernel keeps the fp32 product (more accurate); the emulator follows the kernel, `strict_autocast=True` gives autocast's form |
| 6 | residual adds (x + half, net + inp + c) | fp32 | fp32 in the reference's order (update_mlp.hip:498, 668, 858-873) | agrees |
| 7 | LayerNorm (gru[0], gru[2], corr LN, norm) | fp32 | fp32 two-pass (update_mlp.hip:195-215, 261-300) | agrees (emulator: float64) |
| 8 | corr LN -> relu -> Linear3 input | fp32 relu, cast to half by F.linear | (_Float16)fmaxf(LN, 0) (update_mlp.hip:812) | agrees |
| 9 | gathered / state rows entering a Linear | cast to half by F.linear | (_Float16) on staging (update_mlp.hip:620, 1114, 1198, 1313) | agrees |
| 10 | SoftAgg f, g | half tensors | f = h_round(acc + bf), g = (_Float16)(acc + bg) (update_mlp.hip:1329-1330, 1388) | agrees |
| 11 | SoftAgg softmax weights exp(g - max) and the weighted sums | scatter_softmax / scatter_sum on half tensors: weights and sums rounded to half | fp32 online softmax (exp2 in log2 units), fp32 sums (update_mlp.hip:1384-1391, 1476) | deliberate departure: fp32 weights and sums (more accurate); the emulator follows the kernel |
| 12 | SoftAgg y = sum / z -> fp16, h(y) -> fp16 | half | (_Float16)(a / z), (_Float16)(acc + b) (update_mlp.hip:1481, 1506) | agrees |
| 13 | heads: relu(net) -> fp16, Linear -> fp16, sigmoid -> fp16 | half tensors (ramp/net.py:87-90) | h_round at update_mlp.hip:538, 567-569; update.hip:249-253 | agrees |
| 14 | fp16 copies of fp32 state (relu_t, nbr out_t) | .half() of the fp32 value | (_Float16) of the fp32 result (update_mlp.hip:518, 670) | agrees (checked bit for bit) |

Deliberate departures outside the update operator: the correlation accumulates in fp32 where the reference's kernel
accumulates in half (altcorr.hip, reference correlation_kernel.cu:121, 130); `corr_ref` is fp32 accumulation followed
by one rounding, which is what the kernel claims.
"""
import math

import torch
import torch.nn.functional as F

# (mantissa bits, smallest normal exponent, largest finite value)
FORMATS = {"fp16": (10, -14, 65504.0), "e4m3": (3, -6, 448.0)}
FP8_ACT_SCALE = 8.0          # rampvo_amd/conv_hip.py: activations are multiplied by this before the e4m3 conversion
# fp8 layers (measured on MI355X; the cause is not established): the 1x1 layers with K = 32 and 64 went past GAMMA(K) m
# (flips at 0.99 of it, and unexplained mismatches), so for K < FP8_K_SMALL the bound is taken at K = FP8_K_MIN, where
# their worst flips are 0.64 (K = 32) and 0.23 (K = 64) of it.  K = 128 (0.51) and the 3x3 layers (K = 288 / 576:
# <= 0.19) keep their own GAMMA(K).
FP8_K_SMALL = 128
FP8_K_MIN = 512


def fp8_K(K):
    """the K at which an fp8 layer's accumulation bound is taken (see FP8_K_MIN)"""
    return FP8_K_MIN if K < FP8_K_SMALL else K
# the fused chains' fp32 outputs against the emulator, relative to the local magnitude m of `Chains` (measured on
# MI355X at E = 1003 / 20011 / 41003: worst 0.083 (gru, E = 20011), at most 2.2 % of the elements above 2^-14 m;
# bounds about 2x that).  m is not a propagated error bound: near-cancelling elements get a small m, which is why the
# per-element maximum is loose; the fraction above 2^-14 m is the criterion that separates correct from mutated.
CHAIN_FP32_MAX = 0.15
CHAIN_FP32_FRAC = 0.05
# SoftAgg's fp16 output against the emulator, relative to the magnitude of its `h` Linear's sum (measured on MI355X at
# the same sizes: worst 2.5e-4 of m, at most 0.22 % of the elements above 2^-14 m; the emulator's own fp32 evaluation,
# test_roundref_cpu.py: 2.5e-4 and 0.55 %; bounds about 2x the larger)
SOFTAGG_MAX = 5e-4
SOFTAGG_FRAC = 0.01


def GAMMA(K):
    """fp32 accumulation bound for K products + bias (module docstring)"""
    return (K + 2) * 2.0 ** -23


def _pow2(e):
    """2^e as float64 for an int64 tensor e (built from the exponent bits: exact on every device, unlike pow / ldexp,
    whose device implementations need not be)"""
    return ((e + 1023) << 52).view(torch.float64)


def round_to(x, fmt="fp16", mode="rne"):
    """x (any float tensor) rounded to `fmt` in float64: round to nearest even ("rne") or toward zero ("rtz", the
    mutation of the teeth test).  A single rounding from float64 (torch's float64 -> half goes through float: a double
    rounding).  fp16 overflows to +-inf; e4m3fn values must be clamped to +-448 first (it has no inf)."""
    mant, emin, vmax = FORMATS[fmt]
    x = x.detach().double()
    _, e = torch.frexp(x)
    e = torch.clamp(e.to(torch.int64) - 1, min=emin)
    ulp = _pow2(e - mant)
    q = x / ulp                                           # exact: a power-of-two scale
    r = (torch.round(q) if mode == "rne" else torch.trunc(q)) * ulp
    if fmt == "fp16":
        r = torch.where(r.abs() > vmax, torch.copysign(torch.full_like(r, math.inf), x), r)
    r = torch.where(torch.isfinite(x), r, x)
    return r


def fp16(x):
    """round to nearest even fp16, returned in x's float dtype (fp32 input: the same as .half())"""
    return round_to(x, "fp16").to(x.dtype)


def e4m3(x, scale=1.0):
    """the fp8 conversion of the kernels: clamp (x * scale) to +-448 (conv.hip:624, the weights' 448 / max|w| scale),
    round to e4m3fn (nearest even); returned as the scaled e4m3 value in float64"""
    return round_to((x.double() * scale).clamp(-448.0, 448.0), "e4m3")


def ulp_of(r, fmt="fp16"):
    mant, emin, _ = FORMATS[fmt]
    _, e = torch.frexp(r.double())
    return _pow2(torch.clamp(e.to(torch.int64) - 1, min=emin) - mant)


# ------------------------------------------------------------------------------------------------- float64 references
def linear_ref(x, w, b=None):
    """y = x w^T + b in float64 and its magnitude |x| |w|^T + |b|"""
    x, w = x.double(), w.double()
    y, m = x @ w.t(), x.abs() @ w.abs().t()
    if b is not None:
        y, m = y + b.double(), m + b.double().abs()
    return y, m


def conv_ref(x_nhwc, w, b, stride, pad):
    """NHWC conv (x [H, W, Cin], w [Cout, Cin, k, k]) in float64 and its magnitude; [OH, OW, Cout]"""
    x = x_nhwc.double().permute(2, 0, 1)[None]
    w = w.double()
    if x.shape[1] != w.shape[1]:
        x = x[:, :w.shape[1]]
    bd = None if b is None else b.double()
    y = F.conv2d(x, w, bd, stride, pad)[0].permute(1, 2, 0)
    m = F.conv2d(x.abs(), w.abs(), None if b is None else bd.abs(), stride, pad)[0].permute(1, 2, 0)
    return y, m


# the small biases of the conv-layer cases (test_conv_instances_gpu.py::make_conv): a dropped one must show
TINY_BIASES = (2e-3, -1e-3, 3e-3, -2.5e-3)
IN_ACC_ONE = 2.0 ** 20       # csrc/conv.hip::IN_ACC_ONE: the accumulators' fixed point
# the fp32 steps between the float64 tail pixel and the kernels' (scale, shift as floats, product, sum: four for y, four
# for a normalised skip, one for the last sum), each within 2^-24 of a partial magnitude <= m: 9 2^-24 m < GAMMA(TAIL_K) m
TAIL_K = 8
NORM_K = 2                   # fp16(relu(x scale + shift)): scale, shift, product, sum -- 4 2^-24 m <= GAMMA(2) m


def acc_stats(acc, C, count, eps):
    """InstanceNorm statistics from the accumulator integers (csrc/conv.hip::in_acc_finalize; acc [R][C][2] int64:
    replicated 2^-20 fixed-point sums of x and x^2): (mean, biased variance, scale = rsqrt(var + eps), shift =
    -mean scale) in float64.  The integer sum is exact; eps is the float the kernel is handed."""
    s = acc.view(-1, C, 2).sum(0)
    eps = float(torch.tensor(eps, dtype=torch.float32))
    mean = s[:, 0].double() / IN_ACC_ONE / float(count)
    var = (s[:, 1].double() / IN_ACC_ONE / float(count) - mean * mean).clamp(min=0.0)
    scale = 1.0 / torch.sqrt(var + eps)
    return mean, var, scale, -mean * scale


def norm_relu_ref(x, scale, shift):
    """relu(x scale + shift) in float64 and its magnitude |x scale| + |shift| (the prologue's operand before rounding)"""
    a = x.double() * scale.double()
    return torch.relu(a + shift.double()), a.abs() + shift.double().abs()


def tail_ref(y, scale, shift, skip, skip_scale=None, skip_shift=None, skip_relu=False):
    """the residual block's tail pixel relu(relu(y scale + shift) + skip') in float64 and its magnitude; skip' = skip,
    or skip skip_scale + skip_shift (the downsample path's norm), or fp16(relu(that)) (`skip_relu`: a normalised map
    that was never materialised, rounded as the materialised one would be); y, skip [H, W, C]"""
    a, ma = norm_relu_ref(y, scale, shift)
    b = skip.double()
    mb = b.abs()
    if skip_scale is not None:
        t = b * skip_scale.double()
        b, mb = t + skip_shift.double(), t.abs() + skip_shift.double().abs()
    if skip_relu:
        b = round_to(torch.relu(b), "fp16")
    return torch.relu(a + b), ma + mb


def corr_ref(fmap1, fmap2, coords, ii, jj, R):
    """the correlation (oracle/ramp_oracle.c orc_corr: dot products over C at the integer window, then the bilinear
    blend) in float64, with its magnitude; fmap1 [N1, C, P, P], fmap2 [N2, C, H, W], coords [E, 2, P, P] ->
    [E, d (x offset), d (y offset), P, P]"""
    f1, f2, c = fmap1.double(), fmap2.double(), coords.double()
    E, _, P, _ = c.shape
    N2, C, H, W = f2.shape
    D, d = 2 * R + 2, 2 * R + 1
    x, y = c[:, 0], c[:, 1]
    fx, fy = torch.floor(x).clamp(-1e6, 1e6), torch.floor(y).clamp(-1e6, 1e6)
    off = torch.arange(D, device=c.device, dtype=torch.float64) - R
    yi = fy[..., None, None] + off[:, None]                 # [E, P, P, D(y), 1]
    xi = fx[..., None, None] + off[None, :]                 # [E, P, P, 1, D(x)]
    ok = (yi >= 0) & (yi < H) & (xi >= 0) & (xi < W)
    yc, xc = yi.clamp(0, H - 1).long(), xi.clamp(0, W - 1).long()
    a = f1[ii].permute(0, 2, 3, 1)                          # [E, P, P, C]
    g = f2.permute(0, 2, 3, 1)[jj[:, None, None, None, None], yc, xc]    # [E, P, P, D, D, C]
    raw = (a[:, :, :, None, None, :] * g).sum(-1) * ok
    mag = (a.abs()[:, :, :, None, None, :] * g.abs()).sum(-1) * ok
    dx, dy = (x - torch.floor(x))[..., None, None], (y - torch.floor(y))[..., None, None]

    def blend(t):
        return ((1 - dx) * (1 - dy) * t[..., :-1, :-1] + dx * (1 - dy) * t[..., :-1, 1:]
                + (1 - dx) * dy * t[..., 1:, :-1] + dx * dy * t[..., 1:, 1:])
    out, m = blend(raw), blend(mag)                          # [E, P, P, d(y), d(x)]
    return out.permute(0, 4, 3, 1, 2), m.permute(0, 4, 3, 1, 2)


# ----------------------------------------------------------------------------------------------------------- checks
def rounding_report(y, exact, m, fmt, K):
    """per-element comparison of a once-rounded kernel output with fmt(exact) (module docstring): counts of exact
    matches, explained flips (a neighbour, with `exact` within GAMMA(K) m of the rounding boundary) and unexplained
    mismatches; the worst flip as |exact - boundary| / (GAMMA(K) m) (<= 1) and the largest distance in ulps"""
    y, exact, m = y.detach().double(), exact.detach().double(), m.detach().double()
    nan = torch.isnan(exact)
    r = round_to(exact, fmt)
    g = GAMMA(K) * m
    eq = (y == r) | (nan & torch.isnan(y))
    lo, hi = round_to(exact - g, fmt), round_to(exact + g, fmt)
    flip = ~eq & ~nan & (y >= lo) & (y <= hi)
    bad = ~eq & ~flip
    worst = 0.0
    if bool(flip.any()):
        bnd = 0.5 * (y[flip] + r[flip])
        worst = float(((exact[flip] - bnd).abs() / g[flip]).max())
    fin = torch.isfinite(r) & torch.isfinite(y)
    ulps = float(((y - r).abs()[fin] / ulp_of(r[fin], fmt)).max()) if bool(fin.any()) else 0.0
    return dict(n=y.numel(), flips=int(flip.sum()), bad=int(bad.sum()), worst=worst, max_ulp=ulps,
                bad_idx=bad.nonzero()[:5].tolist())


def check_rounded(y, exact, m, fmt, K, name=""):
    """assert that every element of y is fmt(exact) or an explained neighbour; returns (explained flips, worst)"""
    rep = rounding_report(y, exact, m, fmt, K)
    print("%-34s n=%-8d flips=%-6d (%.4f %%) worst flip %.2f of gamma_K m, max %.0f ulp, bound: 0 unexplained"
          % (name, rep["n"], rep["flips"], 100.0 * rep["flips"] / max(rep["n"], 1), rep["worst"], rep["max_ulp"]))
    assert rep["bad"] == 0, (name, rep)
    return rep["flips"], rep["worst"]


def fp32_report(y, exact, m):
    """fp32 outputs: the error relative to each element's own magnitude m (not the tensor's max):
    (max |y - exact| / m, the fraction of elements with |y - exact| / m > 2^-14)"""
    r = (y.double() - exact.double()).abs() / m.double()
    return float(r.max()), float((r > 2.0 ** -14).double().mean())


def check_fp32(y, exact, m, tol, frac_tol, name=""):
    worst, frac = fp32_report(y, exact, m)
    print("%-34s fp32: worst %.2e of m (bound %.1e), above 2^-14 m: %.4f %% (bound %.3f %%)" % (name, worst, tol,
                                                                                             100 * frac, 100 * frac_tol))
    assert worst <= tol and frac <= frac_tol, (name, worst, frac)
    return worst, frac


# ------------------------------------------------------------------------------------------- the fp16 chain emulator
class Chains:
    """the fused fp16 chains of the update operator (csrc/update_mlp.hip, update.hip) restated on the torch modules of
    rampvo_amd.net.Update (ramp/net.py:34-90, ramp/blocks.py:15-50) with the kernels' rounding points (table in the
    module docstring).  dtype: float64 (the reference) or float32 (a correct evaluation done another way, for the
    teeth test).  The knobs are the teeth test's mutations: strict_autocast takes autocast's form of the two deliberate
    departures (rounds GatedResidual's product, row 5; SoftAgg's softmax weights and sums in half, row 11), skip_r skips
    the rounding of GatedResidual's `res` Linear output, eps overrides the LayerNorm epsilon, rtz rounds every fp16
    point toward zero."""

    def __init__(self, update, dtype=torch.float64, strict_autocast=False, skip_r=False, eps=None, rtz=False):
        self.u, self.dt = update, dtype
        self.strict, self.skip_r, self.eps, self.rtz = strict_autocast, skip_r, eps, rtz

    def h(self, t):
        return round_to(t, "fp16", "rtz" if self.rtz else "rne").to(self.dt)

    def lin(self, x, mod, out_round=True):
        w, b = self.h(mod.weight.detach()), self.h(mod.bias.detach())
        y = self.h(x) @ w.t() + b
        return self.h(y) if out_round else y

    def ln(self, v, mod):
        eps = mod.eps if self.eps is None else self.eps
        v = v.to(self.dt)
        mean = v.mean(-1, keepdim=True)
        var = ((v - mean) ** 2).mean(-1, keepdim=True)
        n = (v - mean) / torch.sqrt(var + eps)
        w, b = mod.weight.detach().to(self.dt), mod.bias.detach().to(self.dt)
        # value and its local magnitude: |n||w| + |b|, plus |w| for the row statistics' share (a local scale, not a
        # propagated error bound)
        return n * w + b, n.abs() * w.abs() + b.abs() + w.abs()

    def gated(self, x, gr):
        """GatedResidual (ramp/blocks.py:30) on the fp32 residual x: the new residual and its magnitude"""
        xh = self.h(x)
        gate = self.h(torch.sigmoid(self.lin(xh, gr.gate[0])))
        hid = self.h(torch.relu(self.lin(xh, gr.res[0])))
        r = self.lin(hid, gr.res[2], out_round=not self.skip_r)
        p = gate * r
        if self.strict:
            p = self.h(p)
        return x + p, x.abs() + p.abs()

    def gru(self, x32, add=None, prologue=True):
        """upd_gru: [LN_pre(x32 + add)] -> GatedResidual -> LN -> GatedResidual; (out32, its magnitude, relu_t)"""
        g = self.u.gru
        x = x32.to(self.dt)
        if prologue:
            x = self.ln(x + add.to(self.dt), g[0])[0]
        x, _ = self.gated(x, g[1])
        x = self.ln(x, g[2])[0]
        out, mag = self.gated(x, g[3])
        return out, mag, self.h(torch.relu(out))

    def nbr(self, net_in, idx, seq):
        """upd_nbr: net + Lb(relu(La(mask * net[idx]))); (out, magnitude)"""
        net = net_in.to(self.dt)
        gathered = net[idx.clamp(min=0)] * (idx >= 0).to(self.dt)[:, None]
        c = self.lin(self.h(torch.relu(self.lin(gathered, seq[0]))), seq[2])
        return net + c, net.abs() + c.abs()

    def corr_mlp(self, corr, state, net_map, table, inp_idx, mod):
        """upd_corr_mlp: norm(net[map] + inp[idx % mod] + corr-MLP(corr)); (out, magnitude)"""
        cm = self.u.corr
        c1 = self.h(torch.relu(self.lin(corr, cm[0])))
        ln, _ = self.ln(self.lin(c1, cm[2]), cm[3])
        c = self.lin(self.h(torch.relu(ln)), cm[5])
        if state is None:
            v = table.to(self.dt) + c
        else:
            st = state.to(self.dt)[net_map.clamp(min=0)] * (net_map >= 0).to(self.dt)[:, None]
            v = st + table.to(self.dt)[inp_idx % mod] + c
        return self.ln(v, self.u.norm)

    def softagg(self, x, agg, inv, G):
        """SoftAgg (ramp/blocks.py:42-47) on x = the fp32 rows (the add already applied), factor -> group `inv`:
        hy = fp16(h(fp16(sum_e softmax(g) f / ...))) with fp32-class softmax weights and sums (row 11); (hy, the
        magnitude of h's sum)"""
        xh = self.h(x.to(self.dt))
        fh, gh = self.lin(xh, agg.f), self.lin(xh, agg.g)
        C = fh.shape[1]
        idx = inv[:, None].expand(-1, C)
        mx = torch.full((G, C), -math.inf, dtype=self.dt, device=x.device).scatter_reduce(0, idx, gh, "amax")
        zeros = lambda: torch.zeros(G, C, dtype=self.dt, device=x.device)
        if self.strict:
            # autocast's form: torch_scatter's softmax and sum on half tensors, every intermediate a half tensor
            e = self.h(torch.exp(self.h(gh - mx[inv])))
            wgt = self.h(e / self.h(zeros().index_add_(0, inv, e))[inv])
            y = self.h(zeros().index_add_(0, inv, self.h(fh * wgt)))
        else:
            e = torch.exp(gh - mx[inv])
            z = zeros().index_add_(0, inv, e)
            a = zeros().index_add_(0, inv, fh * e)
            y = self.h(a / z)
        return self.lin(y, agg.h), y.abs() @ self.h(agg.h.weight.detach()).abs().t() + self.h(agg.h.bias.detach()).abs()
