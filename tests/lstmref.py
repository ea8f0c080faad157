"""float64 restatements of the front end's recurrent steps -- TEST INFRASTRUCTURE ONLY.

What ``csrc/conv.hip`` computes before the conv towers, stated once more in plain torch on the CPU without any of the
kernels' structure (no tiles, no fragments, no LDS staging, no permuted gate rows):

  * ``singlescale_step``: one time step of ``MergerLSTMsceneEncoder`` (reference ramp/extractor.py:233-259) -- two per-pixel
    LSTM cells with carried (h, c), the presence rule and the shared 1x1 super-state convolution;
  * ``multiscale_step``: one scale of ``MultiScaleMergerDoubleNet`` for one time step (:540-566) -- ``conv_1`` with zero
    padding, one LSTM step from the zero state, the events mix and, when the frame is present, the image mix;
  * ``any_nonzero``: the presence test, ``torch.any(x != 0)``.

The weights are read from the modules' parameters (``singlescale_weights``, ``multiscale_weights``) and every function
returns float64.  The ``*_f32`` twins evaluate the same statements in torch float32 on the CPU: the distance between a twin
and the float64 result is the envelope of ``georef.bound`` (the reference formulas' own rounding), never the kernel's.

The keyword arguments ``present``, ``pad`` and ``edge`` exist for tests/test_lstmref_cpu.py, which shows that the cases of
the GPU test tell the true statement from plausible wrong ones; the GPU tests never pass them.
"""
import contextlib

import numpy as np
import torch

F64 = torch.float64


def _t(a, dtype):
    if isinstance(a, np.ndarray):
        a = torch.from_numpy(np.ascontiguousarray(a))
    return a.detach().to("cpu").to(dtype)


# ---------------------------------------------------------------------------------------------------------------- weights
def _lstm_weights(lstm):
    return dict(w_ih=_t(lstm.weight_ih_l0, F64), w_hh=_t(lstm.weight_hh_l0, F64), b_ih=_t(lstm.bias_ih_l0, F64),
                b_hh=_t(lstm.bias_hh_l0, F64))


def _mix_weights(conv):
    return dict(w=_t(conv.weight, F64).reshape(conv.out_channels, -1), b=_t(conv.bias, F64))


def singlescale_weights(enc):
    """the parameters of a MergerLSTMsceneEncoder's front end, float64"""
    return dict(ev=_lstm_weights(enc.events_convlstm), im=_lstm_weights(enc.image_convlstm),
                ss=_mix_weights(enc.superstate_encoder))


def multiscale_weights(enc):
    """per scale index k: the parameters conv_hip._ms_modules lists, float64"""
    out = []
    for k, S in enumerate(enc.scales):
        ev, im = enc.ev_encoders[k], enc.im_encoders[k]
        out.append(dict(S=int(S),
                        conv_ev=dict(w=_t(ev.conv_1.weight, F64), b=_t(ev.conv_1.bias, F64)),
                        conv_im=dict(w=_t(im.conv_1.weight, F64), b=_t(im.conv_1.bias, F64)),
                        lstm_ev=_lstm_weights(ev.convlstm), lstm_im=_lstm_weights(im.convlstm),
                        mix_ev=_mix_weights(enc.super_state_ev_encoder[k].encoder),
                        mix_im=_mix_weights(enc.super_state_im_encoders[k].encoder)))
    return out


def _cast(w, dtype):
    if isinstance(w, dict):
        return {k: _cast(v, dtype) for k, v in w.items()}
    if isinstance(w, list):
        return [_cast(v, dtype) for v in w]
    return w.to(dtype) if torch.is_tensor(w) else w


# ------------------------------------------------------------------------------------------------------------ the LSTM cell
def _lstm_cell(w, x, h, c):
    """torch's nn.LSTM cell, gate rows (i, f, g, o): x [N, Cin], h, c [N, hid] -> (h', c')"""
    gates = x @ w["w_ih"].t() + w["b_ih"] + h @ w["w_hh"].t() + w["b_hh"]
    i, f, g, o = gates.chunk(4, dim=1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def _mix(w, s, h):
    """1x1 convolution on the channel concatenation [s ; h], per pixel row"""
    return torch.cat((s, h), dim=1) @ w["w"].t() + w["b"]


def _rows(x, dtype):
    """[C, H, W] (or [C, HW]) -> pixel rows [HW, C]"""
    x = _t(x, dtype)
    return x.reshape(x.shape[0], -1).t().contiguous()


# ------------------------------------------------------------------------------------------------------------- SingleScale
STATE_NAMES = ("ss", "h_ev", "c_ev", "h_im", "c_im")


def _singlescale(weights, ev, im, state, dtype, present):
    w = _cast(weights, dtype)
    xe, xi = _rows(ev, dtype), _rows(im, dtype)
    n, hid = xe.shape[0], w["ss"]["b"].shape[0]
    if state is None:
        state = {k: torch.zeros(n, hid, dtype=dtype) for k in STATE_NAMES}
    st = {k: _t(state[k], dtype) for k in STATE_NAMES}
    if present is None:
        present = any_nonzero(ev, im)
    # the cells advance whether or not their modality is present
    h_ev, c_ev = _lstm_cell(w["ev"], xe, st["h_ev"], st["c_ev"])
    h_im, c_im = _lstm_cell(w["im"], xi, st["h_im"], st["c_im"])
    s = st["ss"]
    if present[0]:
        s = _mix(w["ss"], s, h_ev)
    if present[1]:
        s = _mix(w["ss"], s, h_im)
    return dict(ss=s, h_ev=h_ev, c_ev=c_ev, h_im=h_im, c_im=c_im)


def singlescale_step(weights, ev, im, state, present=None):
    """one time step: ev [5,H,W], im [3,H,W], state None (zeros) or the dict a previous call returned ->
    dict(ss, h_ev, c_ev, h_im, c_im), each [HW, 15] float64"""
    return _singlescale(weights, ev, im, state, F64, present)


def singlescale_step_f32(weights, ev, im, state, present=None):
    return _singlescale(weights, ev, im, state, torch.float32, present)


# -------------------------------------------------------------------------------------------------------------- MultiScale
def scale_shape(H, W, S):
    """output plane of conv_1 (k = S + 1, stride S, pad 1; 1x1 for S = 1)"""
    if S <= 1:
        return H, W
    return (H + 2 - (S + 1)) // S + 1, (W + 2 - (S + 1)) // S + 1


def clips(H, W, S):
    """(right, bottom): does a tap of conv_1 fall at ix == W / at iy == H"""
    Hs, Ws = scale_shape(H, W, S)
    if S <= 1:
        return False, False
    return (Ws - 1) * S - 1 + S >= W, (Hs - 1) * S - 1 + S >= H


def _conv_1(w, x, S, pad, edge):
    """x [C, H, W] -> [Co, Hs, Ws]: output (oy, ox) sums the taps at (oy S - pad + ky, ox S - pad + kx); a tap outside the
    image counts as zero (``edge`` = "replicate": a tap past the right or bottom edge counts as the nearest pixel -- a
    deliberate mistake, confined to the two edges the top / left border cannot stand in for).  The output plane is always
    that of pad 1"""
    C, H, W = x.shape
    if S <= 1:
        return torch.einsum("oc,chw->ohw", w["w"][:, :, 0, 0], x) + w["b"][:, None, None]
    K = S + 1
    Hs, Ws = scale_shape(H, W, S)
    y = w["b"][:, None, None].expand(-1, Hs, Ws).clone()
    for ky in range(K):
        iy = torch.arange(Hs) * S - pad + ky
        for kx in range(K):
            ix = torch.arange(Ws) * S - pad + kx
            tap = x[:, iy.clamp(0, H - 1)][:, :, ix.clamp(0, W - 1)]
            inside = (iy >= 0)[:, None] & (ix >= 0)[None, :]
            if edge == "zero":
                inside = inside & (iy < H)[:, None] & (ix < W)[None, :]
            tap = tap * inside.to(x.dtype)
            y = y + torch.einsum("oc,chw->ohw", w["w"][:, :, ky, kx], tap)
    return y


def _multiscale(weights, k, ev, im, s, has_state, use_im, dtype, pad, edge):
    w = _cast(weights[k], dtype)
    S, D = w["S"], w["mix_ev"]["b"].shape[0]
    hs = []
    for x, conv, lstm in ((ev, w["conv_ev"], w["lstm_ev"]), (im, w["conv_im"], w["lstm_im"])):
        y = _rows(_conv_1(conv, _t(x, dtype), S, pad, edge), dtype)
        zero = torch.zeros(y.shape[0], D, dtype=dtype)
        hs.append(_lstm_cell(lstm, y, zero, zero)[0])         # h = sigma(o) tanh(sigma(i) tanh(g)): no state carry
    s = _t(s, dtype) if has_state else torch.zeros(hs[0].shape[0], D, dtype=dtype)
    s = _mix(w["mix_ev"], s, hs[0])
    if use_im:
        s = _mix(w["mix_im"], s, hs[1])
    return s


def multiscale_step(weights, k, ev, im, s, has_state, use_im, pad=1, edge="zero"):
    """one time step of scale index k: ev [5,H,W], im [3,H,W], s [Hs*Ws, D] (ignored without has_state) -> [Hs*Ws, D]"""
    return _multiscale(weights, k, ev, im, s, has_state, use_im, F64, pad, edge)


def multiscale_step_f32(weights, k, ev, im, s, has_state, use_im, pad=1, edge="zero"):
    return _multiscale(weights, k, ev, im, s, has_state, use_im, torch.float32, pad, edge)


# ------------------------------------------------------------------------------------------------------------ presence test
def any_nonzero(a, b):
    """(any(a != 0), any(b != 0)) as torch.any has it: NaN counts as nonzero, +-0.0 does not"""
    f = lambda x: bool((np.asarray(x.detach().cpu() if torch.is_tensor(x) else x) != 0).any())
    return f(a), f(b)


# ----------------------------------------------------------------------------------------------- the cases of the GPU test
FLOOR = 2e-5                 # test_lstm_superstate_kernel_matches_torch's, x max(1, max |ref|)

# (scale, H, W) per kernel; tests/test_frontend_recurrent_gpu.py runs them, tests/test_lstmref_cpu.py shows they can tell
MS_MFMA_CASES = [(1, 1, 5), (1, 3, 7), (1, 23, 41), (1, 1, 131205),
                 (2, 7, 63), (2, 8, 64), (2, 7, 64), (2, 8, 63),
                 (4, 7, 63), (4, 8, 64), (4, 11, 127)]
MS_VALU_CASES = [(2, 9, 50), (2, 7, 63), (4, 9, 50), (4, 11, 127), (4, 7, 63), (1, 3, 7), (1, 23, 41)]
SS_HW = [1, 15, 16, 17, 943, 131205]
SS_PRESENCE = [(1, 1), (0, 1), (1, 0), (0, 0)]
MS_STEPS = [(0, 1), (1, 1), (1, 0)]          # (has_state, use_im) of the three steps of a MultiScale case


def floor_of(ref):
    return FLOOR * max(1.0, float(ref.abs().max()))


def make_encoders(gain=1.0, seed=1):
    """(SingleScale, MultiScale) encoders on the CPU with torch's default init under the seed; ``gain`` scales every LSTM
    weight_ih (8: the gates leave the linear range)"""
    from rampvo_amd.extractor import MergerLSTMsceneEncoder, MultiScaleMergerDoubleNet
    torch.manual_seed(seed)
    ss = MergerLSTMsceneEncoder().eval()
    ms = MultiScaleMergerDoubleNet(5, 3).eval()
    if gain != 1.0:
        with torch.no_grad():
            for lstm in [ss.events_convlstm, ss.image_convlstm] + [e.convlstm for e in ms.ev_encoders] + \
                    [e.convlstm for e in ms.im_encoders]:
                lstm.weight_ih_l0.mul_(gain)
    return ss, ms


def ms_inputs(S, H, W, amp=1.0, seed=0):
    """three steps of float32 (events [5,H,W], image [3,H,W]) for a MultiScale case: unit normal, so that the last column
    and row carry as much as any other"""
    g = torch.Generator().manual_seed(1000 * S + 37 * H + W + seed)
    return [(torch.randn(5, H, W, generator=g) * amp, torch.randn(3, H, W, generator=g)) for _ in MS_STEPS]


def ss_inputs(HW, seed=0):
    """four steps of float32 (events [5,1,HW], image [3,1,HW]) with the presence patterns SS_PRESENCE"""
    g = torch.Generator().manual_seed(77 + HW + seed)
    return [(torch.randn(5, 1, HW, generator=g) * pe, torch.randn(3, 1, HW, generator=g) * pi) for pe, pi in SS_PRESENCE]


def ms_reference(weights, k, steps, **kw):
    """[(float64 state, envelope)] per step of a MultiScale case; each precision carries its own state"""
    out, s64, s32 = [], None, None
    for (ev, im), (has, use) in zip(steps, MS_STEPS):
        s64 = multiscale_step(weights, k, ev, im, s64, has, use, **kw)
        s32 = multiscale_step_f32(weights, k, ev, im, s32, has, use, **kw)
        out.append((s64, float((s32.double() - s64).abs().max())))
    return out


def ss_reference(weights, steps):
    """[(float64 state dict, envelope dict)] per step of a SingleScale case"""
    out, s64, s32 = [], None, None
    for ev, im in steps:
        s64 = singlescale_step(weights, ev, im, s64)
        s32 = singlescale_step_f32(weights, ev, im, s32)
        out.append((s64, {n: float((s32[n].double() - s64[n]).abs().max()) for n in STATE_NAMES}))
    return out


# fp32 HIP encoder against the ATen forward of the same modules, x the map's largest entry (measured 4.9e-6 / 9.4e-6)
ENC_HIP_VS_ATEN_TOL = 4e-5


@contextlib.contextmanager
def torch_towers():
    """bind the torch forwards of the tower modules (ResidualBlock ...) for the duration of the reference run"""
    from oracle import host_cpu
    saved = [(c, a, c.__dict__.get(a)) for c, a, _ in host_cpu.module_patches()]
    for c, a, f in host_cpu.module_patches():
        setattr(c, a, f)
    try:
        yield
    finally:
        for c, a, f in saved:
            setattr(c, a, f)
