"""Float64 restatement of the window's uncertainty (include/ramp_hip.h ``ramp_ba_covariance``), numpy only.

The per-factor Jacobians come from ``oracle.ba_edge_terms`` (pinned to the reference's own Python at 1e-10 by
tests/golden/ba_f64_pin.npz); everything behind them -- the gate, B, E, C, the Schur complement, the solver's diagonal
damping, the inverse -- is restated here from the definition:

    Q = 1 / (C + lambda),  S = B - E Q E',  S_dd += 1e-4 S_dd + 1,  cov = S^-1,  depth_var_k = Q_k + Q_k^2 e_k' S^-1 e_k

``dtype=np.float32`` runs the same function with float32 Jacobians, float32 algebra and a float32 Cholesky: its distance
from the float64 result is the rounding envelope the GPU tests scale their bounds by (tests/test_ba_covariance_gpu.py).

The gate is restated from the projected centres, the targets and the bounds; the depth gate (Z > 0.2) is not -- the oracle's
per-factor terms do not return Z -- so the scenes this is used on keep every point in front of every camera
(scenes.ba_pin_scene).  The keyword switches of ``system`` break the restatement on purpose (tests/test_covref_cpu.py).
"""
import numpy as np

import oracle as orc

FLOOR = 1e-5          # see ``compare``


def system(s, t0, t1, dtype=np.float64, ji_sign=-1.0, ungated_edge=None):
    """B [6N,6N], E [6N,Mu], C [Mu], the sorted unique patches, chi2, the gate -- of the scene dict ``s`` (scenes.ba_pin_scene's
    keys), poses t0 .. t1-1 free.  ji_sign: the sign of the source pose's Jacobian (the kernel's -Ji); ungated_edge: a factor
    whose gate is ignored."""
    T = dtype
    f64 = T == np.float64
    t = orc.ba_edge_terms(s["poses"], s["patches"], s["intr"], s["ii"], s["jj"], s["kk"], f64=f64)
    Ji, Jj, Jz, xy = (np.asarray(t[k], T) for k in ("Ji", "Jj", "Jz", "xy"))
    intr = np.asarray(s["intr"], T).reshape(-1, 4)[0]
    r = np.asarray(s["target"], T).reshape(-1, 2) - xy
    valid = ((np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) < 128) & (xy[:, 0] > -64) & (xy[:, 1] > -64)
             & (xy[:, 0] < 2 * intr[2] + 64) & (xy[:, 1] < 2 * intr[3] + 64))
    gate = valid.copy()
    if ungated_edge is not None:
        gate[ungated_edge] = True
    w = np.asarray(s["weight"], T).reshape(-1, 2) * gate[:, None].astype(T)
    ii, jj, kk = (np.asarray(s[k], np.int64) for k in ("ii", "jj", "kk"))
    N, E = t1 - t0, len(ii)
    n6 = 6 * N
    uk, col = np.unique(kk, return_inverse=True)
    Jp = np.zeros((E, 2, n6 + 6), T)                      # (the last block collects the fixed poses and is cut off)
    ia = np.where((ii >= t0) & (ii < t1), ii - t0, N)
    ja = np.where((jj >= t0) & (jj < t1), jj - t0, N)
    e = np.arange(E)
    for c in range(6):
        np.add.at(Jp, (e, slice(None), 6 * ia + c), T(ji_sign) * Ji[:, :, c])
        np.add.at(Jp, (e, slice(None), 6 * ja + c), Jj[:, :, c])
    Jp = Jp[:, :, :n6]
    B = np.einsum("eda,ed,edb->ab", Jp, w, Jp).astype(T)
    Em = np.zeros((n6, len(uk)), T)
    np.add.at(Em.T, col, np.einsum("eda,ed,ed->ea", Jp, w, Jz).astype(T))
    C = np.zeros(len(uk), T)
    np.add.at(C, col, np.einsum("ed,ed,ed->e", Jz, w, Jz).astype(T))
    chi2 = float(np.sum((w * r * r).astype(np.float64))) if f64 else float(np.sum(w * r * r, dtype=T))
    return dict(B=B, E=Em, C=C, uk=uk, chi2=chi2, n_valid=int(gate.sum()), valid=valid)


def covariance(s, t0, t1, dtype=np.float64, damping=True, q_term=True, n_patches=None, **kw):
    """dict(cov [6N,6N], depth_var [n_patches] (inf where a patch has no factor), chi2, n_valid, Mu, Q, S, D) by the
    definition, in ``dtype``"""
    T = dtype
    y = system(s, t0, t1, dtype=T, **kw)
    B, Em, C, uk = y["B"], y["E"], y["C"], y["uk"]
    lm = T(np.asarray(s["lmbda"]).reshape(-1)[0])
    Q = (T(1) / (C + lm)).astype(T)
    S = (B - (Em * Q[None]) @ Em.T).astype(T)
    D = (T(1e-4) * np.diag(S) + T(1)).astype(T) if damping else np.zeros(S.shape[0], T)
    S = S + np.diag(D)
    n_patches = n_patches or np.asarray(s["patches"]).shape[0]
    dv = np.full(n_patches, np.inf, T)
    if S.shape[0]:
        L = np.linalg.cholesky(S)
        Li = np.linalg.inv(L).astype(T)
        cov = (Li.T @ Li).astype(T)
        v = (Li @ Em).astype(T)
        quad = np.sum(v * v, axis=0, dtype=T)
    else:
        cov, quad = np.zeros((0, 0), T), np.zeros(len(uk), T)
    dv[uk] = (Q if q_term else 0) + Q * Q * quad
    return dict(cov=cov, depth_var=dv, chi2=y["chi2"], n_valid=y["n_valid"], Mu=len(uk), Q=Q, S=S, D=D, uk=uk,
                B=B, E=Em, C=C, valid=y["valid"])


def errors(out_cov, out_dv, ref):
    """the three error figures of an output against the float64 result ``ref``: cov relative to the largest diagonal entry,
    the cov diagonal and depth_var per entry (relative), each as the maximum over the entries"""
    c64, d64 = ref["cov"], ref["depth_var"]
    fin = np.isfinite(d64)
    oc, od = np.asarray(out_cov, np.float64), np.asarray(out_dv, np.float64)
    if c64.size:
        e_cov = float(np.abs(oc - c64).max() / np.diag(c64).max())
        e_diag = float((np.abs(np.diag(oc) - np.diag(c64)) / np.diag(c64)).max())
    else:
        e_cov = e_diag = 0.0
    e_dv = float((np.abs(od[fin] - d64[fin]) / d64[fin]).max())
    return dict(cov=e_cov, diag=e_diag, depth_var=e_dv)


def compare(out_cov, out_dv, ref64, ref32, floor=FLOOR, cap=5e-3):
    """The comparison of the GPU tests: per output, the error against float64 must not exceed max(floor, 4 x the float32
    restatement's own error) -- the rule of tests/test_geometry_f64_gpu.py; the 4 x covers a different summation order -- and
    that envelope itself must stay below ``cap``, so that the bound cannot grow to hide a failure.

    floor: the envelope is ONE float32 evaluation's error and can come out small by luck where the system is tiny (6 x 6);
    an implementation that sums a few hundred terms in another order may then differ from it by more than 4 x without
    being wrong.  1e-5 is 170 ulp of float32 (2^-24): ordered sums of the few hundred terms per entry these scenes have stay
    below n 2^-24 of their positive terms, and nothing the definition could get wrong is that small.

    Returns (ok, report): report[name] = (error, bound, envelope)."""
    e, env = errors(out_cov, out_dv, ref64), errors(ref32["cov"], ref32["depth_var"], ref64)
    rep, ok = {}, True
    for k in ("cov", "diag", "depth_var"):
        bound = max(floor, 4 * env[k])
        rep[k] = (e[k], bound, env[k])
        ok = ok and e[k] <= bound and env[k] <= cap and np.isfinite(e[k])
    fin = np.isfinite(ref64["depth_var"])
    ok = ok and bool(np.all(np.isinf(np.asarray(out_dv)[~fin])))
    return ok, rep
