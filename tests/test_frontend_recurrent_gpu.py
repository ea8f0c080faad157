"""GPU tests of the front end's recurrent kernels (csrc/conv.hip): any_nonzero_kernel, lstm_superstate_mfma_kernel and the
three MultiScale kernels -- ms_lstm_superstate_kernel (fp32 VALU), ms_lstm_superstate_mfma_kernel (scale 1) and
ms_lstm_superstate_split_kernel (scales 2, 4) -- each against the float64 restatement tests/lstmref.py, at the shapes where
they take another path: fewer pixels than a tile, tails, more than one tile per wave, planes whose last conv_1 tap falls on
the zero padding right of and below the image, widths the MFMA kernels refuse.

One tolerance rule (georef.bound): max(2e-5 max(1, max |ref|), 4 x the envelope), the envelope being the distance of the
float32 restatement from the float64 one on the CPU.  Every element of every output is compared; every buffer the test owns
lies between 64 canary rows.  tests/test_lstmref_cpu.py shows what the cases below can tell apart.
"""
import ctypes

import pytest
import torch

import georef
import lstmref as lr
from guarded import DIRTY, Guarded

pytestmark = pytest.mark.gpu

_nets, _refs = {}, {}


def nets(gain):
    """CPU encoders (the reference's weights) and their copies on the device (the kernels'), per weight set"""
    if gain not in _nets:
        import copy
        ss, ms = lr.make_encoders(gain)
        _nets[gain] = dict(ss=ss, ms=ms, wss=lr.singlescale_weights(ss), wms=lr.multiscale_weights(ms),
                           ss_gpu=copy.deepcopy(ss).cuda(), ms_gpu=copy.deepcopy(ms).cuda())
    return _nets[gain]


def ms_case(gain, S, H, W, amp=1.0):
    """(steps, [(float64 state, envelope)]) of a MultiScale case, computed once"""
    key = ("ms", gain, S, H, W, amp)
    if key not in _refs:
        n = nets(gain)
        steps = lr.ms_inputs(S, H, W, amp)
        _refs[key] = (steps, lr.ms_reference(n["wms"], n["ms"].scales.index(S), steps))
    return _refs[key]


def ss_case(gain, HW):
    key = ("ss", gain, HW)
    if key not in _refs:
        steps = lr.ss_inputs(HW)
        _refs[key] = (steps, lr.ss_reference(nets(gain)["wss"], steps))
    return _refs[key]


def _lib():
    from rampvo_amd._lib import lib
    return lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    from rampvo_amd._lib import stream
    return stream()


# ---------------------------------------------------------------------------------------------------------------- MultiScale
def ms_run(enc, S, H, W, steps, kernel, with16=False):
    """the three steps of a case through one entry point, over a dirty guarded state -> [(state, fp16 copy or None)]"""
    from rampvo_amd import conv_hip
    k = enc.scales.index(S)
    Hs, Ws = lr.scale_shape(H, W, S)
    st = Guarded(Hs * Ws, 16 * S)
    s16 = Guarded(Hs * Ws, 16 * S, torch.float16, fill=7.0, canary=-3.0) if with16 else None
    out = []
    for (ev, im), (has, use) in zip(steps, lr.MS_STEPS):
        ev, im = ev.cuda().contiguous(), im.cuda().contiguous()
        if kernel == "mfma":
            wfrag, wsmall = conv_hip.pack_ms_scale_mfma(enc, k)
            rc = _lib().ramp_ms_lstm_superstate_mfma(_ptr(ev), _ptr(im), _ptr(wfrag), _ptr(wsmall), _ptr(st.t),
                                                    _ptr(s16.t) if with16 else None, H, W, S, has, use, _stream())
        else:
            _, ptrs = conv_hip.pack_ms_scale(enc, k)
            rc = _lib().ramp_ms_lstm_superstate(_ptr(ev), _ptr(im), ptrs, _ptr(st.t), H, W, S, has, use, _stream())
        assert rc == 0, rc
        out.append((st.t.clone(), s16.t.clone() if with16 else None))
    torch.cuda.synchronize()
    assert st.intact() and (s16 is None or s16.intact()), "canary rows written"
    return out


def ms_check(table, name, outs, refs):
    for t, ((s, _), (ref, env)) in enumerate(zip(outs, refs)):
        assert s.shape == ref.shape
        s = s.cpu().double()
        err = float((s - ref).abs().max()) if bool(torch.isfinite(s).all()) else float("inf")
        table.add("%s step %d" % (name, t), err, env, lr.floor_of(ref))


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for (x, _), (y, _) in zip(a, b))


def _finish(table):
    table.show()
    worst = max(table.rows, key=lambda r: r[1] / r[3])
    print("  worst measured / bound: %.3f  (%s: measured %.2e, envelope %.2e, bound %.2e)" % (worst[1] / worst[3], *worst[:4]))
    assert not table.failed(), table.failed()


@pytest.mark.parametrize("gain", [1.0, 8.0])
def test_multiscale_mfma_kernels_against_float64(gain):
    """ms_lstm_superstate_mfma_kernel<16,1,4> and ms_lstm_superstate_split_kernel<32,2> / <64,4>: every step of every case,
    the fp16 copy, the run without it, repeated bits"""
    enc = nets(gain)["ms_gpu"]
    table = georef.Table("MultiScale MFMA kernels against float64, weight_ih x %g" % gain)
    with torch.no_grad():
        for S, H, W in lr.MS_MFMA_CASES:
            steps, refs = ms_case(gain, S, H, W)
            a = ms_run(enc, S, H, W, steps, "mfma", with16=True)
            ms_check(table, "mfma s%d %dx%d" % (S, H, W), a, refs)
            for s, s16 in a:
                assert torch.equal(s16, s.half()), "state16 is not the rounded fp32 state"
            assert same_bits(a, ms_run(enc, S, H, W, steps, "mfma", with16=True)), "two runs differ"
            assert same_bits(a, ms_run(enc, S, H, W, steps, "mfma", with16=False)), "the fp16 copy changes the fp32 state"
    _finish(table)


@pytest.mark.parametrize("gain", [1.0, 8.0])
def test_multiscale_valu_kernel_against_float64(gain):
    """ms_lstm_superstate_kernel<16,1> / <32,2> / <64,4> through ramp_ms_lstm_superstate, which no shipped plane reaches"""
    enc = nets(gain)["ms_gpu"]
    table = georef.Table("MultiScale fp32 VALU kernel against float64, weight_ih x %g" % gain)
    with torch.no_grad():
        for S, H, W in lr.MS_VALU_CASES:
            steps, refs = ms_case(gain, S, H, W)
            a = ms_run(enc, S, H, W, steps, "valu")
            ms_check(table, "valu s%d %dx%d" % (S, H, W), a, refs)
            assert same_bits(a, ms_run(enc, S, H, W, steps, "valu")), "two runs differ"
    _finish(table)


@pytest.mark.parametrize("kernel", ["mfma", "valu"])
def test_multiscale_saturated_gates_stay_finite_and_within_the_bound(kernel):
    """weight_ih x 8 and events of +-1000: e^-a overflows and underflows in every gate"""
    enc = nets(8.0)["ms_gpu"]
    table = georef.Table("MultiScale %s, saturated gates" % kernel)
    with torch.no_grad():
        for S, H, W in (lr.MS_MFMA_CASES if kernel == "mfma" else lr.MS_VALU_CASES):
            if H * W > 10000:
                continue                                  # (the large plane adds no gate value the small ones lack)
            steps, refs = ms_case(8.0, S, H, W, amp=1000.0)
            a = ms_run(enc, S, H, W, steps, kernel)
            assert all(bool(torch.isfinite(s).all()) for s, _ in a)
            ms_check(table, "%s s%d %dx%d" % (kernel, S, H, W), a, refs)
    _finish(table)


def test_multiscale_mfma_entry_refuses_what_it_cannot_tile():
    from rampvo_amd import conv_hip
    from rampvo_amd._lib import RAMP_EUNSUPPORTED
    enc = nets(1.0)["ms_gpu"]
    for S, H, W in [(2, 9, 50), (4, 9, 50), (4, 11, 123), (3, 8, 64)]:
        k = enc.scales.index(S) if S in enc.scales else 1
        wfrag, wsmall = conv_hip.pack_ms_scale_mfma(enc, k)
        _, ptrs = conv_hip.pack_ms_scale(enc, k)
        Hs, Ws = lr.scale_shape(H, W, S)
        st, s16 = Guarded(Hs * Ws, 16 * S), Guarded(Hs * Ws, 16 * S, torch.float16, fill=7.0, canary=-3.0)
        ev, im = torch.randn(5, H, W, device="cuda"), torch.randn(3, H, W, device="cuda")
        rc = _lib().ramp_ms_lstm_superstate_mfma(_ptr(ev), _ptr(im), _ptr(wfrag), _ptr(wsmall), _ptr(st.t), _ptr(s16.t), H, W, S,
                                                1, 1, _stream())
        assert rc == RAMP_EUNSUPPORTED, (S, H, W, rc)
        if S == 3:
            assert _lib().ramp_ms_lstm_superstate(_ptr(ev), _ptr(im), ptrs, _ptr(st.t), H, W, S, 1, 1, _stream()) == RAMP_EUNSUPPORTED
        torch.cuda.synchronize()
        assert st.intact() and s16.intact()
        assert bool((st.t == DIRTY).all()) and bool((s16.t == 7.0).all()), "a refused call wrote"


def test_ms_lstm_superstate_step_dispatches_by_width(monkeypatch):
    """scale 1 and widths that are multiples of 16 go to the MFMA entry, every other width to the fp32 VALU entry -- counted
    at the two library symbols"""
    from rampvo_amd import conv_hip
    enc = nets(1.0)["ms_gpu"]
    calls = {"mfma": 0, "valu": 0}
    l = _lib()
    real = dict(mfma=l.ramp_ms_lstm_superstate_mfma, valu=l.ramp_ms_lstm_superstate)

    def counted(which):
        def f(*a):
            calls[which] += 1
            return real[which](*a)
        return f
    monkeypatch.setattr(l, "ramp_ms_lstm_superstate_mfma", counted("mfma"), raising=False)
    monkeypatch.setattr(l, "ramp_ms_lstm_superstate", counted("valu"), raising=False)
    expect = [(c, "mfma") for c in lr.MS_MFMA_CASES if c[1] * c[2] < 10000] + \
             [(c, "valu" if c[0] > 1 and lr.scale_shape(c[1], c[2], c[0])[1] % 16 else "mfma") for c in lr.MS_VALU_CASES]
    assert sum(w == "valu" for _, w in expect) == 2
    with torch.no_grad():
        for (S, H, W), which in expect:
            k = enc.scales.index(S)
            steps, refs = ms_case(1.0, S, H, W)
            ev, im = steps[0][0].cuda(), steps[0][1].cuda()
            for want_half in (False, True):
                before = dict(calls)
                st = conv_hip.MsState(H, W, S, "cuda")
                out = conv_hip.ms_lstm_superstate_step(enc, k, ev, im, st, True, want_half=want_half)
                other = "valu" if which == "mfma" else "mfma"
                assert calls[which] == before[which] + 1 and calls[other] == before[other], (S, H, W, which)
                assert out.shape == (st.Hs, st.Ws, st.D)
                assert out.dtype == (torch.float16 if want_half and which == "mfma" else torch.float32)
                err = float((st.s.cpu().double() - refs[0][0]).abs().max())
                assert err <= georef.bound(lr.floor_of(refs[0][0]), refs[0][1]) and not st.fresh


# --------------------------------------------------------------------------------------------------------------- SingleScale
def ss_run(enc, HW, steps, mode):
    """the four steps of a case over dirty guarded buffers; mode "step": conv_hip.lstm_superstate_step (per-workgroup flags,
    nblk > 0), "direct": ramp_any_nonzero's two flags and ramp_lstm_superstate_blocks with nblk = 0"""
    from rampvo_amd import conv_hip
    st = conv_hip.LstmState(HW, "cuda")
    nt = (HW + 15) // 16
    g = {n: Guarded(nt * 16, 16) for n in ("h_ev", "c_ev", "h_im", "c_im")}
    g["ss"] = Guarded(HW, 16)
    for n, b in g.items():
        setattr(st, n, b.t.view(nt, 16, 16) if n != "ss" else b.t)
    flags = Guarded(1, 2, torch.int32, fill=-1, canary=0x5A5A5A5A)
    w = conv_hip.pack_lstm_mfma(enc)
    out = []
    for t, (ev, im) in enumerate(steps):
        ev, im = ev.cuda().contiguous(), im.cuda().contiguous()
        if mode == "step":
            ret = conv_hip.lstm_superstate_step(enc, ev, im, st)
            assert ret.data_ptr() == st.ss.data_ptr()
        else:
            assert _lib().ramp_any_nonzero(_ptr(ev), ev.numel(), _ptr(im), im.numel(), _ptr(flags.t), _stream()) == 0
            has = int(t > 0)
            assert _lib().ramp_lstm_superstate_blocks(_ptr(ev), _ptr(im), _ptr(st.h_ev), _ptr(st.c_ev), _ptr(st.h_im),
                                                     _ptr(st.c_im), _ptr(st.ss), _ptr(w), _ptr(flags.t), 0, HW, has, has,
                                                     _stream()) == 0
        got = {n: st.rows(n).clone() for n in ("h_ev", "c_ev", "h_im", "c_im")}
        got["ss"] = st.ss[:, :15].clone()
        # unit 15 of h and c, and channel 15 of the super-state, are padding: exactly zero
        for n in ("h_ev", "c_ev", "h_im", "c_im"):
            pad = getattr(st, n).view(-1, 16, 4, 4).permute(0, 1, 3, 2).reshape(-1, 16)[:HW, 15]
            assert bool((pad == 0).all()), (n, "unit 15")
        assert bool((st.ss[:, 15] == 0).all())
        out.append(got)
    torch.cuda.synchronize()
    assert all(b.intact() for b in g.values()) and flags.intact(), "canary rows written"
    return out


@pytest.mark.parametrize("mode", ["step", "direct"])
@pytest.mark.parametrize("gain", [1.0, 8.0])
def test_singlescale_kernel_against_float64(gain, mode):
    """lstm_superstate_mfma_kernel: ss, h and c of both cells after each of four steps with (events, image) present as
    (1,1), (0,1), (1,0), (0,0), from HW = 1 to 131,205 (four tiles per wave, a partly filled last workgroup)"""
    enc = nets(gain)["ss_gpu"]
    table = georef.Table("SingleScale kernel against float64, weight_ih x %g, %s" % (gain, mode))
    with torch.no_grad():
        for HW in lr.SS_HW:
            steps, refs = ss_case(gain, HW)
            a = ss_run(enc, HW, steps, mode)
            for t, (got, (ref, env)) in enumerate(zip(a, refs)):
                for n in lr.STATE_NAMES:
                    v = got[n].cpu().double()
                    assert v.shape == ref[n].shape
                    err = float((v - ref[n]).abs().max()) if bool(torch.isfinite(v).all()) else float("inf")
                    table.add("HW %d step %d %s" % (HW, t, n), err, env[n], lr.floor_of(ref[n]))
            b = ss_run(enc, HW, steps, mode)
            assert all(torch.equal(x[n].view(torch.int32), y[n].view(torch.int32)) for x, y in zip(a, b) for n in lr.STATE_NAMES)
    _finish(table)


# ------------------------------------------------------------------------------------------------------------- presence test
LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 1048576, 1048581, 1536000]
PAIRS = [(1, 3), (3, 1), (4, 5), (5, 4), (1023, 1025), (1025, 1024), (1024, 1023), (1048576, 5), (5, 1048581),
         (1048581, 1536000), (1536000, 1048576), (1048576, 1048581), (1536000, 1)]
ANY_MAXB = 1024
FLAG_CANARY = 0x5A5A5A5A


def _first_pass(na, nb):
    """elements one pass of the grid covers: 4 per thread, 256 threads, ceil(max(na, nb) / 4 / 256) <= 1024 workgroups"""
    n = max(na, nb)
    return min(max((n // 4 + 255) // 256, 1), ANY_MAXB) * 1024


def _presence_cases(na, nb):
    """(name, [(array, index, value)]) -- the edits of two all-zero arrays"""
    nan, fp = float("nan"), _first_pass(na, nb)
    cases = [("all zero", []), ("a[0]", [(0, 0, 1.0)]), ("b[0]", [(1, 0, 2.0)]), ("a[last]", [(0, na - 1, 1e-45)]),
             ("b[last]", [(1, nb - 1, -3.0)]), ("a[last] and b[last]", [(0, na - 1, 1.0), (1, nb - 1, 1.0)]),
             ("NaN in a only", [(0, na // 2, nan)]), ("NaN in b only", [(1, nb - 1, nan)])]
    if na > fp:
        cases += [("a[last of first pass]", [(0, fp - 1, 1.0)]), ("a[first of second pass]", [(0, fp, 1.0)])]
    if nb > fp:
        cases += [("b[last of first pass]", [(1, fp - 1, 1.0)])]
    return cases


@pytest.mark.parametrize("entry", ["ramp_any_nonzero", "ramp_any_nonzero_blocks", "ramp_any_nonzero_blocks_clear"])
def test_presence_test_is_torch_any(entry):
    assert sorted(set(sum(PAIRS, ()))) == LENGTHS and all(a != b for a, b in PAIRS)
    l = _lib()
    bufs = [torch.zeros(max(LENGTHS) + 4, device="cuda"), torch.zeros(max(LENGTHS) + 4, device="cuda")]
    clear = Guarded(4, 64, torch.int32, fill=FLAG_CANARY, canary=FLAG_CANARY)

    def call(na, nb):
        a, b = bufs[0][:na], bufs[1][:nb]
        if entry == "ramp_any_nonzero":
            flags = Guarded(1, 2, torch.int32, fill=FLAG_CANARY, canary=FLAG_CANARY)
            assert l.ramp_any_nonzero(_ptr(a), na, _ptr(b), nb, _ptr(flags.t), _stream()) == 0
            got = tuple(bool(v) for v in flags.t[0].tolist())
            assert set(flags.t[0].tolist()) <= {0, 1} and flags.intact()
            return got
        flags = Guarded(2, ANY_MAXB, torch.int32, fill=FLAG_CANARY, canary=FLAG_CANARY)
        if entry == "ramp_any_nonzero_blocks":
            nblk = l.ramp_any_nonzero_blocks(_ptr(a), na, _ptr(b), nb, _ptr(flags.t), _stream())
        else:
            nblk = l.ramp_any_nonzero_blocks_clear(_ptr(a), na, _ptr(b), nb, _ptr(flags.t), _ptr(clear.t), 4 * 64 * 4, _stream())
        assert nblk == _first_pass(na, nb) // 1024
        f = flags.t.cpu()
        assert bool(((f[:, :nblk] == 0) | (f[:, :nblk] == 1)).all()), "a workgroup did not report"
        assert bool((f[:, nblk:] == FLAG_CANARY).all()) and flags.intact(), "flags past nblk written"
        return bool(f[0, :nblk].any()), bool(f[1, :nblk].any())

    for na, nb in PAIRS:
        for name, edits in _presence_cases(na, nb):
            for which, idx, val in edits:
                bufs[which][idx] = val
            want = lr.any_nonzero(bufs[0][:na], bufs[1][:nb])
            assert want == (bool(torch.any(bufs[0][:na] != 0)), bool(torch.any(bufs[1][:nb] != 0)))
            assert call(na, nb) == want, (na, nb, name)
            for which, idx, _ in edits:
                bufs[which][idx] = 0.0
        # a nonzero just past the end of either array is not the array's
        bufs[0][na], bufs[1][nb] = 1.0, 1.0
        assert call(na, nb) == (False, False), (na, nb, "past the end")
        bufs[0][na], bufs[1][nb] = 0.0, 0.0
        # -0.0 everywhere
        bufs[0][:na] = -0.0
        bufs[1][:nb] = -0.0
        assert call(na, nb) == (False, False) == lr.any_nonzero(bufs[0][:na], bufs[1][:nb]), (na, nb, "-0.0")
        bufs[0][:na] = 0.0
        bufs[1][:nb] = 0.0
    if entry == "ramp_any_nonzero_blocks_clear":
        torch.cuda.synchronize()
        assert bool((clear.t == 0).all()) and clear.intact()


@pytest.mark.parametrize("n,clear_bytes", [(1, 16), (1, 4096), (1, 3 * 4096 + 16), (5, 1024 * 1024), (1536000, 16),
                                           (1536000, 4 * 1024 * 1024 + 16), (1536000, 9 * 1024 * 1024 + 48)])
def test_fused_clear_zeroes_exactly_clear_bytes(n, clear_bytes):
    """one pass of the grid clears 16 bytes per thread: 4,096 bytes with one workgroup, 4 MiB with 1,024"""
    a, b = torch.zeros(n, device="cuda"), torch.zeros(max(n // 2, 1), device="cuda")
    a[n - 1] = 1.0
    flags = torch.zeros(2, ANY_MAXB, dtype=torch.int32, device="cuda")
    buf = Guarded(clear_bytes // 16, 4, torch.int32, fill=FLAG_CANARY, canary=FLAG_CANARY)
    nblk = _lib().ramp_any_nonzero_blocks_clear(_ptr(a), n, _ptr(b), b.numel(), _ptr(flags), _ptr(buf.t), clear_bytes, _stream())
    assert nblk == _first_pass(n, b.numel()) // 1024
    torch.cuda.synchronize()
    assert bool((buf.t == 0).all()) and buf.intact()
    assert bool(flags[0, :nblk].any()) and not bool(flags[1, :nblk].any())


def test_fused_clear_refusals_write_nothing():
    from rampvo_amd._lib import lib
    a = torch.ones(64, device="cuda")
    flags = Guarded(2, ANY_MAXB, torch.int32, fill=FLAG_CANARY, canary=FLAG_CANARY)
    buf = Guarded(16, 4, torch.int32, fill=FLAG_CANARY, canary=FLAG_CANARY)
    p = buf.t.data_ptr()
    EINVAL = -1
    f = lib().ramp_any_nonzero_blocks_clear
    assert f(_ptr(a), 64, _ptr(a), 64, _ptr(flags.t), ctypes.c_void_p(p + 4), 64, _stream()) == EINVAL      # misaligned
    assert f(_ptr(a), 64, _ptr(a), 64, _ptr(flags.t), ctypes.c_void_p(p), 24, _stream()) == EINVAL         # not 16 n
    assert f(_ptr(a), 64, _ptr(a), 64, _ptr(flags.t), ctypes.c_void_p(p), -16, _stream()) == EINVAL
    assert f(_ptr(a), 64, _ptr(a), 64, _ptr(flags.t), None, 64, _stream()) == EINVAL
    assert f(_ptr(a), 0, _ptr(a), 0, _ptr(flags.t), ctypes.c_void_p(p), 64, _stream()) == EINVAL           # n = 0
    assert f(_ptr(a), 64, _ptr(a), 64, None, ctypes.c_void_p(p), 64, _stream()) == EINVAL
    torch.cuda.synchronize()
    assert bool((buf.t == FLAG_CANARY).all()) and buf.intact()
    assert bool((flags.t == FLAG_CANARY).all()) and flags.intact()


# ---------------------------------------------------------------------------------------- the whole encoder, fallback plane
def test_multiscale_encoder_at_a_plane_the_mfma_kernels_refuse():
    """96 x 136: the scale widths are 136, 68 and 34, so scales 2 and 4 run the fp32 VALU kernel and -- mixed precision --
    hand the fp16 towers an fp32 state.  fp32 against the ATen forward of the same modules, mixed precision against fp32"""
    from oracle import host_cpu
    from rampvo_amd.synthetic import SyntheticStream, make_network
    H, W = 96, 136
    stream = SyntheticStream(H, W, 3, seed=6)
    masks = [True, False, True]
    outs = {}
    with torch.no_grad():
        for backend in ("torch", "hip", "half"):
            enc = make_network("MultiScale").patchify.encoder
            enc.mixed_precision = backend == "half"
            res = []
            for t in range(3):
                im, ev, _, _ = stream.frame(t)
                kw = dict(events=ev.cuda(), images=im.cuda(), mask=torch.tensor([masks[t]]), reinit_hidden=(t == 0), out_scale=0.25)
                if backend == "torch":
                    with lr.torch_towers():
                        f, i = host_cpu.multiscale_forward(enc, **kw)
                else:
                    f, i = enc(**kw)
                    assert masks[t] or (f is None and i is None)
                if masks[t]:
                    res.append((f.float().clone(), i.float().clone()))
            outs[backend] = res
            if backend == "torch":
                ref_states = [s.clone() for s in enc.super_states]
            elif backend == "hip":
                assert [(s.Hs, s.Ws) for s in enc._hip_state] == [(96, 136), (48, 68), (24, 34)]
                for a, b in zip(ref_states, enc._hip_state):
                    assert a.shape == b.s.shape and float((a - b.s).abs().max()) <= 2e-5 * max(1.0, float(a.abs().max()))
            else:
                assert enc._hip_state[1].s16 is None and enc._hip_state[2].s16 is None        # (the VALU kernel writes no copy)
    rel = lambda x, y: float((x - y).abs().max()) / float(x.abs().max())
    assert len(outs["hip"]) == 2
    for (f0, i0), (f1, i1), (f2, i2) in zip(outs["torch"], outs["hip"], outs["half"]):
        assert f0.shape == f1.shape == f2.shape == (1, 1, 128, H // 4, W // 4) and i0.shape == i1.shape == i2.shape
        print("96x136 fp32 vs ATen: fmap %.2e imap %.2e; mixed vs fp32: fmap %.2e imap %.2e"
              % (rel(f0, f1), rel(i0, i1), rel(f1, f2), rel(i1, i2)))
        assert rel(f0, f1) <= lr.ENC_HIP_VS_ATEN_TOL and rel(i0, i1) <= lr.ENC_HIP_VS_ATEN_TOL
        assert rel(f1, f2) <= 3e-2 and rel(i1, i2) <= 3e-2
