"""The line search of the event alignment (include/ramp_hip.h ``ramp_event_align``) restated as the state machine the header
defines, one ``step`` per evaluation -- TEST INFRASTRUCTURE ONLY.  Plain Python floats (float64) and ``math.sqrt``, no numpy in
the arithmetic: every operation is one IEEE double operation in the order the definition writes it, which is what makes the
device's answer derivable bit for bit.

``align(evaluate, ...)`` drives the machine over ``evaluate(theta32) -> (variance, grad[7])`` or ``(variance, grad[7],
status[8])``; ``theta32`` is the numpy float32 [7] the device's evaluation would read.  With ``max_evals = 1 + 9 * iters`` it is
``ops.align_loop`` and ``contrastref.align`` statement for statement; the one deliberate difference is the correctly rounded
``sqrt`` where ``align_loop`` writes ``** 0.5`` (``norm_args`` keeps every argument so a test can assert that the two agree).
The ``mistake`` keyword breaks the machine on purpose: every one of them has to be told apart by the tests.
"""
import math

import numpy as np

ITERS, STALLED, FLAT, BUDGET = 1, 2, 3, 4
REASONS = {0: "running", ITERS: "iters", STALLED: "stalled", FLAT: "flat", BUDGET: "budget"}
TRIALS = 9
MISTAKES = ("ge", "eight", "nodouble", "halvefirst", "unmasked", "stale", "noreset", "round32")


def f32(values):
    """float32 of a sequence of doubles, round to nearest even, overflow to infinity: what the device stores"""
    with np.errstate(over="ignore"):
        return np.asarray(values, np.float64).astype(np.float32)


class Machine:
    """the state of the definition, by its names"""

    def __init__(self, correction, free, step, iters, mistake=None):
        assert mistake is None or mistake in MISTAKES
        self.theta = [float(c) for c in (np.zeros(7) if correction is None else np.asarray(correction, np.float64).reshape(7))]
        self.mask = [1.0 if f else 0.0 for f in free]
        self.length, self.iters, self.mistake = float(step), int(iters), mistake
        self.f = self.f0 = self.norm = 0.0
        self.g, self.gm, self.trial = [0.0] * 7, [0.0] * 7, [0.0] * 7
        self.n_accepted = self.n_evals = self.halvings = self.reason = self.seen = 0
        self.history = [float("nan")] * self.iters
        self.status = [0] * 8
        self.cor = f32(self.theta)                  # what the next evaluation reads
        self.cor_theta = self.cor.copy()            # what the evaluation at theta read
        self.norm_args = []
        if mistake == "halvefirst":
            self.length *= 0.5

    def propose(self, new_direction):
        if new_direction:
            mask = [1.0] * 7 if self.mistake == "unmasked" else self.mask
            self.gm = [gi * mi for gi, mi in zip(self.g, mask)]
            total = 0.0
            for v in self.gm:
                total = total + v * v
            self.norm_args.append(total)
            self.norm = math.sqrt(total) if total >= 0.0 else float("nan")
            if not (self.norm > 0.0 and self.norm < float("inf")):
                self.reason = FLAT
                return
        self.trial = [ti + (self.length * gi) / self.norm for ti, gi in zip(self.theta, self.gm)]
        self.cor = f32(self.trial)

    def step(self, e, variance, grad, status):
        if self.reason != 0:
            return
        self.n_evals += 1
        self.seen |= int(status[0])
        if e == 0:
            self.f = self.f0 = float(variance)
            self.g, self.status = [float(v) for v in grad], [int(w) for w in status]
            if self.iters == 0:
                self.reason = ITERS
            else:
                self.propose(True)
            return
        ft = float(variance)
        if (ft >= self.f) if self.mistake == "ge" else (ft > self.f):
            self.theta = [float(v) for v in self.cor] if self.mistake == "round32" else list(self.trial)
            self.f, self.status, self.cor_theta = ft, [int(w) for w in status], self.cor.copy()
            if self.mistake != "stale" or self.n_accepted == 0:
                self.g = [float(v) for v in grad]
            self.history[self.n_accepted] = self.f
            self.n_accepted += 1
            if self.mistake != "nodouble":
                self.length *= 2.0
            if self.mistake != "noreset":
                self.halvings = 0
            if self.n_accepted == self.iters:
                self.reason = ITERS
            else:
                self.propose(True)
        else:
            self.length *= 0.5
            self.halvings += 1
            if self.halvings >= (TRIALS - 1 if self.mistake == "eight" else TRIALS):
                self.reason = STALLED
            else:
                self.propose(False)


def align(evaluate, correction=None, free=(0, 0, 0, 1, 1, 1, 0), step=0.05, iters=20, max_evals=None, mistake=None):
    """-> dict: correction float64 [7], correction_f32 float32 [7], variance, variance0, length, grad [7], history (the
    accepted variances), history_full (float64 [iters], NaN behind them), status [8], reason, n_accepted, n_evals, halvings,
    seen, info (int32 [8] as the entry writes it), norm_args (the arguments of every sqrt), thetas (theta after every
    evaluation that ran)"""
    need = 1 + TRIALS * int(iters)
    budget = need if max_evals is None else min(int(max_evals), need)
    assert budget >= 1
    m = Machine(correction, free, step, iters, mistake)
    thetas = []
    for e in range(budget):
        if m.reason != 0:
            break                                    # (the device enqueues the rest as empty launches)
        out = evaluate(m.cor.copy())
        m.step(e, out[0], out[1], out[2] if len(out) > 2 else [0] * 8)
        thetas.append(list(m.theta))
    if m.reason == 0:
        m.reason = BUDGET
    return dict(correction=np.asarray(m.theta, np.float64), correction_f32=m.cor_theta, variance=m.f, variance0=m.f0,
                length=m.length, grad=np.asarray(m.g, np.float64), history=m.history[:m.n_accepted],
                history_full=np.asarray(m.history, np.float64), status=np.asarray(m.status, np.int32), reason=m.reason,
                n_accepted=m.n_accepted, n_evals=m.n_evals, halvings=m.halvings, seen=m.seen,
                info=np.asarray([m.reason, m.n_accepted, m.n_evals, m.halvings, m.seen, 0, 0, 0], np.int32),
                norm_args=m.norm_args, thetas=thetas)


def bits(a):
    """the bit patterns of a float array, for comparisons that tell -0.0 from 0.0 and one NaN from another"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# the seven calls of the issue, over contrastref.align_scene(): keyword arguments of align / ops.event_align
CALLS = {
    "default": dict(),
    "iters3": dict(iters=3),
    "step4": dict(step=4.0, iters=4),
    "start": dict(correction=[0.0, 0.0, 0.0, 0.15, -0.10, 0.30, 0.0], iters=5),
    "none_free": dict(free=(0, 0, 0, 0, 0, 0, 0)),
    "all_free": dict(free=(1, 1, 1, 1, 1, 1, 1), iters=6),
    "huge_step": dict(step=1e6, iters=2),
}
