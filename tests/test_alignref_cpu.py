"""The state machine of the event alignment (tests/alignref.py, include/ramp_hip.h ``ramp_event_align``) has to earn its place
as the GPU test's reference: it is the two existing host loops bit for bit, closed forms, budgets, the mistakes the definition
invites, and the new entry points' export and argument checks.  No GPU."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import alignref
import contrastref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def scene_evaluate(theta32):
    """contrastref's float64 evaluation of the dot scene, computed once per distinct float32 correction"""
    if "ev" not in _CACHE:
        _CACHE["ev"] = contrastref.evaluator(**contrastref.align_scene())
    key = np.asarray(theta32, np.float32).tobytes()
    if key not in _CACHE:
        _CACHE[key] = _CACHE["ev"](np.frombuffer(key, np.float32))
    return _CACHE[key]


def host_arguments(kw):
    """the keyword arguments of a call as the host loops take them: the start rounded to float32 first, as ops.event_align
    rounds it (torch.as_tensor of a list)"""
    kw = dict(dict(correction=None, free=(0, 0, 0, 1, 1, 1, 0), step=0.05, iters=20), **kw)
    kw["correction"] = [0.0] * 7 if kw["correction"] is None else alignref.f32(kw["correction"]).astype(np.float64).tolist()
    return kw


EXPECTED = {"default": (46, 20, "iters"), "iters3": (5, 3, "iters"), "step4": (13, 4, "iters"), "start": (15, 5, "iters"),
            "none_free": (1, 0, "flat"), "all_free": (11, 6, "iters"), "huge_step": (10, 0, "stalled")}


@pytest.mark.parametrize("call", list(alignref.CALLS))
def test_the_machine_is_the_two_host_loops(call):
    from rampvo_amd import ops
    kw = host_arguments(alignref.CALLS[call])
    count = [0]

    def counted(theta):
        count[0] += 1
        return scene_evaluate(theta)

    r = alignref.align(scene_evaluate, **kw)
    a = contrastref.align(counted, kw["correction"], kw["free"], kw["step"], kw["iters"])
    n_a, count[0] = count[0], 0
    q = ops.align_loop(lambda th: tuple(counted(th)), kw["correction"], kw["free"], kw["step"], kw["iters"])
    n_q = count[0]
    print(call, "evals", r["n_evals"], "accepted", r["n_accepted"], alignref.REASONS[r["reason"]], "variance", r["variance0"], "->",
          r["variance"])
    for x in r["norm_args"]:                         # a condition on these inputs: the two square roots agree
        assert x ** 0.5 == math.sqrt(x) and float(np.sqrt(np.float64(x))) == math.sqrt(x), x
    assert r["n_evals"] == n_a == n_q
    assert (r["n_evals"], r["n_accepted"], alignref.REASONS[r["reason"]]) == EXPECTED[call]
    for other in (a, q):
        assert np.array_equal(alignref.bits(np.asarray(other["correction"], np.float64)), alignref.bits(r["correction"]))
        assert np.array_equal(alignref.bits(np.asarray(other["history"], np.float64)), alignref.bits(np.asarray(r["history"], np.float64)))
        assert np.float64(other["variance"]).tobytes() == np.float64(r["variance"]).tobytes()
        assert np.float64(other["variance0"]).tobytes() == np.float64(r["variance0"]).tobytes()
    assert np.isnan(r["history_full"][r["n_accepted"]:]).all() and len(r["history_full"]) == kw["iters"]
    assert np.array_equal(r["correction_f32"], alignref.f32(r["correction"]))


def test_the_budget_on_the_dot_scene():
    """max_evals = 10 of the default call's 46: BUDGET at the full run's iterate after its 10th evaluation"""
    full = alignref.align(scene_evaluate)
    r = alignref.align(scene_evaluate, max_evals=10)
    assert r["reason"] == alignref.BUDGET and r["n_evals"] == 10 and 0 < r["n_accepted"] < full["n_accepted"]
    assert r["correction"].tolist() == full["thetas"][9] and r["history"] == full["history"][:r["n_accepted"]]
    exact = alignref.align(scene_evaluate, max_evals=full["n_evals"])
    more = alignref.align(scene_evaluate, max_evals=10 ** 6)           # (clamped to 1 + 9 * iters)
    for k in ("correction", "variance", "history", "reason", "n_evals", "length"):
        assert np.array_equal(exact[k], full[k]) and np.array_equal(more[k], full[k]), k
    short = alignref.align(scene_evaluate, max_evals=full["n_evals"] - 1)
    assert short["reason"] == alignref.BUDGET and short["n_accepted"] == full["n_accepted"] - 1


A = [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]


def quadratic(a=A, nan=False):
    """f = -|theta - a|^2 with its gradient -2 (theta - a): every number below is a dyadic fraction, so exact"""
    def evaluate(theta):
        th = [float(v) for v in theta]
        g = [-2.0 * (t - c) for t, c in zip(th, a)]
        return -sum((t - c) ** 2 for t, c in zip(th, a)), [float("nan")] * 7 if nan else g
    return evaluate


def test_closed_forms_on_a_quadratic():
    # 0 -> .25 (accepted) -> .75 (accepted) -> 1.75 (worse) -> 1.25 (equal: not accepted) -> 1 (accepted; the gradient is 0)
    r = alignref.align(quadratic(), step=0.25)
    assert (r["reason"], r["n_evals"], r["n_accepted"], r["halvings"]) == (alignref.FLAT, 6, 3, 0)
    assert r["correction"].tolist() == A and r["history"] == [-0.5625, -0.0625, 0.0] and r["variance0"] == -1.0
    assert r["length"] == 0.5 and not r["grad"].any() and r["thetas"][3][3] == r["thetas"][4][3] == 0.75
    assert alignref.align(quadratic(), step=0.25, max_evals=10)["info"].tolist() == r["info"].tolist()
    # budgets
    r1 = alignref.align(quadratic(), step=0.25, max_evals=1)
    assert (r1["reason"], r1["n_evals"], r1["n_accepted"]) == (alignref.BUDGET, 1, 0) and not r1["correction"].any()
    assert r1["variance"] == r1["variance0"] == -1.0 and r1["length"] == 0.25 and r1["grad"][3] == 2.0
    r2 = alignref.align(quadratic(), step=0.25, max_evals=2)
    assert (r2["reason"], r2["n_evals"], r2["n_accepted"]) == (alignref.BUDGET, 2, 1) and r2["correction"][3] == 0.25
    assert r2["history"] == [-0.5625] and r2["length"] == 0.5
    # iters = 0: one evaluation, ITERS, whatever the budget
    for budget in (1, 2, 10, None):
        r0 = alignref.align(quadratic(), step=0.25, iters=0, max_evals=budget)
        assert (r0["reason"], r0["n_evals"], r0["n_accepted"]) == (alignref.ITERS, 1, 0) and len(r0["history_full"]) == 0
    # a gradient that the mask zeroes, and one that is NaN: FLAT after one evaluation
    for ev in (quadratic([1.0, 0, 0, 0, 0, 0, 0.5]), quadratic(nan=True)):
        for budget in (1, 2, 10):
            rf = alignref.align(ev, step=0.25, max_evals=budget)
            assert (rf["reason"], rf["n_evals"], rf["n_accepted"]) == (alignref.FLAT, 1, 0) and not rf["correction"].any()
    # nine failed trials: STALLED, the length halved nine times, theta where it was
    rs = alignref.align(quadratic(), step=1024.0, iters=2, correction=[0, 0, 0, 0.999, 0, 0, 0])
    assert (rs["reason"], rs["n_evals"], rs["halvings"]) == (alignref.STALLED, 10, 9) and rs["length"] == 2.0
    # a NaN trial value is rejected like a worse one
    calls = [0]

    def nan_second(theta):
        calls[0] += 1
        f, g = quadratic()(theta)
        return (float("nan") if calls[0] == 2 else f), g
    rn = alignref.align(nan_second, step=0.25, max_evals=3)
    assert rn["n_accepted"] == 1 and rn["correction"][3] == 0.125 and rn["halvings"] == 0
    # a step that overflows float32: the evaluation reads infinity, theta stays a double
    seen = []
    alignref.align(lambda th: (seen.append(th.copy()), quadratic()(np.zeros(7)))[1], step=1e39, iters=1, max_evals=2)
    assert np.isinf(seen[1][3]) and not seen[1][[0, 1, 2, 4, 5, 6]].any()


def _inputs():
    yield "quadratic", quadratic(), dict(step=0.25)
    yield "quadratic, start off the axis", quadratic([0.5, 0, 0, 1.0, 0, 0, 0]), dict(step=0.25, correction=[0.25, 0, 0, 0, 0, 0, 0])
    for call in ("default", "step4", "huge_step"):
        yield call, scene_evaluate, alignref.CALLS[call]


@pytest.mark.parametrize("mistake", alignref.MISTAKES)
def test_every_mistake_is_told_apart(mistake):
    """each deliberate mistake changes the correction, the history or the evaluation count on at least one of these inputs"""
    told = []
    for name, ev, kw in _inputs():
        good, bad = alignref.align(ev, **kw), alignref.align(ev, mistake=mistake, **kw)
        same = (np.array_equal(alignref.bits(good["correction"]), alignref.bits(bad["correction"])) and good["history"] == bad["history"]
                and good["n_evals"] == bad["n_evals"] and good["reason"] == bad["reason"])
        if not same:
            told.append(name)
    print(mistake, "told apart on:", told)
    assert told


def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_event_align", "ramp_event_align_workspace_bytes"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    for macro, val in (("RAMP_ALIGN_ITERS", _lib.RAMP_ALIGN_ITERS), ("RAMP_ALIGN_STALLED", _lib.RAMP_ALIGN_STALLED),
                       ("RAMP_ALIGN_FLAT", _lib.RAMP_ALIGN_FLAT), ("RAMP_ALIGN_BUDGET", _lib.RAMP_ALIGN_BUDGET),
                       ("RAMP_ALIGN_MAX_ITERS", _lib.RAMP_ALIGN_MAX_ITERS), ("RAMP_ALIGN_TRIALS", _lib.RAMP_ALIGN_TRIALS)):
        assert re.search(r"#define %s %d\b" % (macro, val), header), macro
    assert (_lib.RAMP_ALIGN_ITERS, _lib.RAMP_ALIGN_STALLED, _lib.RAMP_ALIGN_FLAT, _lib.RAMP_ALIGN_BUDGET) == (
        alignref.ITERS, alignref.STALLED, alignref.FLAT, alignref.BUDGET) and _lib.RAMP_ALIGN_TRIALS == alignref.TRIALS
    assert {ops.ALIGN_REASONS[k] for k in (1, 2, 3, 4)} == {alignref.REASONS[k] for k in (1, 2, 3, 4)}
    n = lib.ramp_event_align_workspace_bytes(5, 24, 32)
    assert n % 8 == 0 and n > lib.ramp_event_contrast_workspace_bytes(5, 24, 32)
    assert lib.ramp_event_align_workspace_bytes(5, 0, 32) == 0
    for name in ("event_align", "event_align_info"):
        assert callable(getattr(ops, name))
    assert callable(TrackerQueries.align_events)
    import inspect
    for fn, names in ((ops.event_align, ("resident", "max_evals")), (TrackerQueries.align_events, ("resident", "max_evals", "as_tensor"))):
        assert all(k in inspect.signature(fn).parameters for k in names)


def test_argument_checks_that_need_no_gpu():
    """RAMP_EINVAL before anything touches the device (the pointers are never read)"""
    from rampvo_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    off = lambda n: ctypes.c_void_p(q.value + n)

    def call(N=10, T=2, t_ref=0.0, flags=0, H=24, W=32, free_mask=0x38, step=0.05, iters=3, max_evals=28, x=q, cor=None, out=q,
             f32_out=q, result=q, grad=q, history=q, status=q, info=q, ws=q):
        return lib.ramp_event_align(x, q, q, q, N, q, q, T, t_ref, q, q, cor, flags, H, W, free_mask, step, iters, max_evals, out,
                                    f32_out, result, grad, history, status, info, ws, 0, None)

    for kw in (dict(N=-1), dict(T=0), dict(H=0), dict(W=0), dict(t_ref=float("nan")), dict(t_ref=float("inf")),
               dict(step=float("nan")), dict(step=float("-inf")), dict(flags=_lib.RAMP_WARP_IDENTITY), dict(flags=32),
               dict(iters=-1), dict(iters=_lib.RAMP_ALIGN_MAX_ITERS + 1), dict(max_evals=0), dict(max_evals=-3),
               dict(free_mask=128), dict(free_mask=-1), dict(x=None), dict(out=None), dict(f32_out=None), dict(result=None),
               dict(grad=None), dict(history=None), dict(status=None), dict(info=None), dict(ws=None), dict(ws=off(8)),
               dict(out=off(4)), dict(result=off(4)), dict(grad=off(4)), dict(history=off(4)), dict(f32_out=off(2)),
               dict(status=off(2)), dict(info=off(1)), dict(cor=off(2))):
        assert call(**kw) == -1, kw
    assert call() == -3 and call(N=0) == -3                           # a workspace of 0 bytes: RAMP_EWORKSPACE
    assert call(history=None, iters=0) == -3                          # (no history to write: NULL is accepted)
    assert call(iters=_lib.RAMP_ALIGN_MAX_ITERS, max_evals=2 ** 31 - 1) == -3
