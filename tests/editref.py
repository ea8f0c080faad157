"""Numpy restatement of the tracker's keyframe edit and graph plan (csrc/track.hip trk_flag / trk_decide / trk_apply,
csrc/graph.hip plan_hist / plan_scan / plan_scatter / plan_segsort) -- TEST INFRASTRUCTURE ONLY.

int64 numpy throughout; nothing here calls libramp_hip.so or torch.  The operation is the reference's
``Ramp_vo.keyframe()`` (ramp/Ramp_vo.py:237-274) followed by the next frame's ``append_factors`` of ``__edges_forw`` /
``__edges_back`` (:312-325, :394-395), with the sizes the device keeps in ``dyn`` (include/ramp_hip.h RAMP_DYN_*):

    decide(mm, thresh)      the motion test: the two float32 magnitudes summed and compared in float64, strictly below.
    edit(...)               the factors kept (in their order, renumbered behind the dropped keyframe k = n - KI, culled below
                            kcut = max(n_after - R, 0) M) with row = their old index, then the factors of frame n_after + 1 in
                            the reference's meshgrid(indexing='ij') order with row = -1, and the dyn words.
    plan(ii, jj, kk, W)     both groupings (kk; pair key jj W + ii): order (stable by key), gid, seg_start, ukeys, ngroups;
                            the temporal neighbours ix / jx (previous / next factor of the same patch in (jj, factor) order)
                            and kj, the (kk, jj, factor)-sorted factor list.
    shift_rows(buf, k, n, ring)   the per-frame rows after keyframe k was dropped (:258-268).
    make_graph(...)         a valid random graph of an exact size.

The second half is the table of cases tests/test_graph_edit_gpu.py runs the kernels on; tests/test_editref_cpu.py checks that
every case that expects status 0 stays inside the device's capacities, so that expectation is justified."""
import collections
import zlib

import numpy as np

DYN = ("N", "NROW", "E", "KLO", "FLO", "W", "REMOVED", "K", "NPREV", "EPREV", "EKEPT")
ST_CAP, ST_GROUP, ST_LOG, ST_BOUND, ST_ROWS = 4, 8, 16, 32, 64          # RAMP_DYN_STATUS bits
EDIT_BLOCK = 1024                # factors per edit workgroup (csrc/track.hip TRK_EB)
PATCH_FACTORS_MAX = 1024         # more factors on one patch: no temporal neighbours from the plan (status bit 8)
THRESH = 15.0                    # KEYFRAME_THRESH of the default and the precise preset
MEM = 32                         # rows of the feature rings (Ramp_vo.mem)


# ------------------------------------------------------------------------------------------------ the operation
def decide(mm, thresh):
    """Ramp_vo.keyframe(): m = motionmag(i, j) + motionmag(j, i); m / 2 < KEYFRAME_THRESH, on python floats (doubles)"""
    a, b = np.float64(np.float32(mm[0])), np.float64(np.float32(mm[1]))
    with np.errstate(invalid="ignore"):
        return bool((a + b) / np.float64(2) < np.float64(thresh))


def new_factors(n1, M, r):
    """(ii, jj, kk) a frame adds when it becomes frame n1 - 1 (reference :312-325 with self.n = n1): forward, every live patch
    of the last r - 1 frames to the new frame; backward, the new frame's patches to the last r frames, itself included"""
    lo = max(n1 - r, 0)
    kf, jf = np.meshgrid(np.arange(M * lo, M * max(n1 - 1, 0)), np.arange(n1 - 1, n1), indexing="ij")
    kb, jb = np.meshgrid(np.arange(M * max(n1 - 1, 0), M * n1), np.arange(lo, n1), indexing="ij")
    kk = np.concatenate([kf.reshape(-1), kb.reshape(-1)]).astype(np.int64)
    jj = np.concatenate([jf.reshape(-1), jb.reshape(-1)]).astype(np.int64)
    return kk // M, jj, kk


def edit(ii, jj, kk, n, M, r, R, KI, remove, n_rows=None, E_cap=None):
    """n: keyframes when keyframe() runs.  n_rows / E_cap (optional): the frame-buffer and factor capacities the device
    clamps to (status bits 64 / 4): the next frame's row is at most n_rows - 2, the new factors are cut at E_cap.
    Returns dict(graph [4, E_new] = (ii, jj, kk, row), idx, Ek, ne, dyn {name: value}, status)"""
    ii, jj, kk = (np.array(a, np.int64) for a in (ii, jj, kk))
    E = len(ii)
    k = n - KI
    keep = np.ones(E, bool)
    n_after = n
    if remove:
        keep &= ~((ii == k) | (jj == k))
        behind_i, behind_j = ii > k, jj > k
        kk[behind_i] -= M
        ii[behind_i] -= 1
        jj[behind_j] -= 1
        n_after = n - 1
    kcut = max(n_after - R, 0) * M
    keep &= kk >= kcut
    idx = np.nonzero(keep)[0]
    status, nrow = 0, n_after
    if n_rows is not None and nrow > n_rows - 2:
        status, nrow = status | ST_ROWS, n_rows - 2
    n1 = nrow + 1
    lo = max(n1 - r, 0)
    e_ii, e_jj, e_kk = new_factors(n1, M, r)
    Ek, ne = len(idx), len(e_kk)
    if E_cap is not None and Ek + ne > E_cap:
        status, ne = status | ST_CAP, max(E_cap - Ek, 0)
    flo = min(int(min(ii[idx].min(), jj[idx].min())), lo) if Ek else lo
    graph = np.stack([np.concatenate([ii[idx], e_ii[:ne]]), np.concatenate([jj[idx], e_jj[:ne]]),
                      np.concatenate([kk[idx], e_kk[:ne]]), np.concatenate([idx, np.full(ne, -1, np.int64)])])
    dyn = dict(N=n1, NROW=nrow, E=Ek + ne, KLO=min(kcut, M * lo), FLO=flo, W=n1 - flo, REMOVED=int(bool(remove)), K=k,
               NPREV=n, EPREV=E, EKEPT=Ek)
    return dict(graph=graph, idx=idx, Ek=Ek, ne=ne, dyn=dyn, status=status)


def _groups(key):
    ukeys, gid, counts = np.unique(key, return_inverse=True, return_counts=True)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return dict(order=np.argsort(key, kind="stable").astype(np.int64), gid=gid.reshape(-1).astype(np.int64), seg_start=seg,
                ukeys=ukeys.astype(np.int64), ngroups=len(ukeys))


def plan(ii, jj, kk, W):
    """W: dyn's W (pair keys are jj W + ii).  Returns dict(kk=groups, ij=groups, ix, jx, kj)"""
    ii, jj, kk = (np.asarray(a, np.int64) for a in (ii, jj, kk))
    E = len(kk)
    kj = np.lexsort((np.arange(E), jj, kk)).astype(np.int64)            # by (kk, jj, factor)
    ix, jx = np.full(E, -1, np.int64), np.full(E, -1, np.int64)
    if E > 1:
        same = kk[kj[1:]] == kk[kj[:-1]]
        ix[kj[1:][same]] = kj[:-1][same]
        jx[kj[:-1][same]] = kj[1:][same]
    return dict(kk=_groups(kk), ij=_groups(jj * np.int64(W) + ii), ix=ix, jx=jx, kj=kj)


def shift_source(k, n, nrows, ring=0):
    """for each of a buffer's nrows rows, the row whose content it holds after keyframe k of n was dropped: rows k + 1 ..
    n - 1 move down by one (ring rows modulo ring); every other row keeps its content"""
    src = np.arange(nrows, dtype=np.int64)
    for row in range(k, n - 1):
        src[row % ring if ring else row] = (row + 1) % ring if ring else row + 1
    return src


def shift_rows(buf, k, n, ring=0):
    """the per-frame buffer (first axis: rows) after the drop"""
    buf = np.asarray(buf)
    return buf[shift_source(k, n, buf.shape[0], ring)]


def make_graph(rng, n, M, r, R, E, KI=4, remove=False, mode="mixed"):
    """exactly E factors with kk // M == ii, |ii - jj| <= r - 1 and frames in [max(n - R - 3, 0), n), in no particular order.
    mode "mixed": some factors older than the removal window, some on keyframe k = n - KI; "kept": every factor survives the
    edit with this `remove`; "touch_k": every factor has ii == k or jj == k"""
    k = n - KI
    f0 = max(n - R - 3, 0)
    if mode == "kept":
        n_after = n - 1 if remove else n
        frames = np.array([f for f in range(f0, n)
                           if not (remove and f == k) and (f - (1 if remove and f > k else 0)) >= n_after - R], np.int64)
        ii = frames[rng.integers(0, len(frames), E)]
    elif mode == "touch_k":
        ii = np.clip(k + rng.integers(-r + 1, r, E), f0, n - 1).astype(np.int64)
        ii[rng.random(E) < 0.5] = k
    else:
        assert mode == "mixed"
        ii = rng.integers(f0, n, E).astype(np.int64)
    kk = ii * M + rng.integers(0, M, E)
    jj = np.clip(ii + rng.integers(-r + 1, r, E), 0, n - 1).astype(np.int64)
    if mode == "kept" and remove:
        jj[jj == k] = ii[jj == k]
    if mode == "touch_k":
        jj[ii != k] = k
    return ii.astype(np.int64), jj, kk.astype(np.int64)


# ------------------------------------------------------------------------------------------------ geometries and cases
class Geometry(collections.namedtuple("Geometry", "name preset M r R")):
    """the capacities DeviceTrack derives from a configuration (rampvo_amd/track_dev.py)"""
    E_cap = property(lambda s: (s.R + 2) * (2 * s.r - 1) * s.M)
    kk_cap = property(lambda s: (s.R + 2) * s.M)
    ij_cap = property(lambda s: min((s.R + 2) * 2 * s.r, (s.R + s.r + 1) ** 2))
    kkey_cap = property(lambda s: (s.R + 2) * s.M)
    pkey_cap = property(lambda s: (s.R + s.r + 1) ** 2)
    new_cap = property(lambda s: (2 * s.r - 1) * s.M)            # factors one frame adds
    pad = property(lambda s: 4 * (2 * s.r - 1) * s.M)            # defined rows behind the live factors

    def ne(self, n1):
        return self.M * (max(n1 - 1, 0) - max(n1 - self.r, 0)) + self.M * (n1 - max(n1 - self.r, 0))

    def fill_bound(self, E_bound):
        """rows up to which the plan leaves defined gid / ix / jx entries: the next step's launch bound"""
        Eb = E_bound if 0 < E_bound < self.E_cap else self.E_cap
        return min(Eb + self.new_cap, self.E_cap)


GEOMS = {g.name: g for g in (Geometry("A", "default", 48, 13, 22), Geometry("B", "default", 37, 13, 22),
                             Geometry("C", "precise", 96, 33, 42), Geometry("D", "precise", 300, 33, 42))}

Case = collections.namedtuple("Case", "id geom n E KI mode mm flag nlog log_cap n_rows E_bound")
Case.__doc__ = """one edit: geometry name, keyframes n, factors E, KEYFRAME_INDEX, make_graph's mode ("oversize": mixed + one patch with
1025 factors), the motion magnitudes, the status bit the case raises (0: none), the delta-log fill and capacity, the frame
buffers' rows (None: the allocation's) and the step's launch bound (None: max(E, 1))"""

MM_DROP, MM_KEEP = (THRESH - 1.0, THRESH - 3.0), (THRESH + 1.0, THRESH - 0.5)
_BELOW_15 = float(np.nextafter(np.float32(15), np.float32(0)))
# (mm, dropped?): the comparison is strict; the exact sum 30 - 2^-20 rounds to 30.0 in float32; NaN and inf - inf compare false
DECISIONS = (("equal", (15.0, 15.0), False), ("below_by_one_ulp", (15.0, _BELOW_15), True),
             ("nan", (float("nan"), 1.0), False), ("inf_minus_inf", (float("inf"), float("-inf")), False))
CHAIN_PATTERN = (False, True, True, False, True, False)           # (keep, drop, drop, keep, drop, keep)
# (A starts below the removal window: the kk key range N M - KLO and the pair range W^2 change from step to step)
CHAINS = {"A": dict(n=21, E=9000), "D": dict(n=47, E=500000)}


def _case(id, geom, n, E, KI=4, mode="mixed", mm=MM_KEEP, flag=0, nlog=0, log_cap=4096, n_rows=None, E_bound=None):
    return Case(id, geom, n, E, KI, mode, mm, flag, nlog, log_cap, n_rows, E_bound)


def _both(id, geom, n, E, **kw):
    return [_case("%s-%s" % (id, tag), geom, n, E, mm=mm, **kw) for tag, mm in (("keep", MM_KEEP), ("drop", MM_DROP))]


def _build_cases():
    A = GEOMS["A"]
    out = []
    # 1. sizes
    for E in (0, 1, 1023, 1024, 1025, 4096, 9000):
        out += _both("A-size-%d" % E, "A", 31, E)
    # (everything kept and the new graph fills E_cap exactly: n1 is 32 without the drop, 31 with it; both add (2r - 1) M)
    out += _both("A-size-fills-cap", "A", 31, A.E_cap - A.ne(31), mode="kept")
    out += _both("A-all-touch-k", "A", 31, 3000, mode="touch_k")
    out += _both("A-all-kept", "A", 31, 9000, mode="kept")
    # C: more than 256 edit workgroups (E > 262144) fold two per thread of trk_decide; 264000 -> 258 workgroups, 266300 -> 261
    # (odd: a ragged last thread); D: 820000 -> 801 workgroups, four per thread, ragged; 400000 -> 391, two per thread
    for g, sizes in (("C", (140000, 264000, 266300)), ("D", (400000, 820000))):
        for E in sizes:
            out += _both("%s-size-%d" % (g, E), g, 47, E)
    # 2. window boundaries: kcut and lo leave zero
    for n in (5, A.r - 1, A.r, A.r + 1, A.R, A.R + 1, A.R + 2, A.R + 3, 31):
        out += _both("A-window-n%d" % n, "A", n, 3000)
    # 3. row shift: nmove = KI - 1 rows; n = mem + KI - 1 puts keyframe k in the ring's last row (the first move wraps)
    for g in ("A", "B"):
        for KI, n in ((2, MEM + 1), (3, MEM + 2), (4, MEM + 3), (5, MEM + 4), (6, MEM + 5), (8, MEM + 7), (8, MEM + 3)):
            out.append(_case("%s-shift-KI%d-n%d-drop" % (g, KI, n), g, n, 3000, KI=KI, mm=MM_DROP))
        out.append(_case("%s-shift-KI4-n%d-keep" % (g, MEM + 3), g, MEM + 3, 3000))
    # 4. decision
    for tag, mm, _ in DECISIONS:
        out.append(_case("A-decide-%s" % tag, "A", 31, 3000, mm=mm))
    # 5. status bits
    out.append(_case("A-flag-cap", "A", 31, A.E_cap - A.ne(31) + 1, mode="kept", flag=ST_CAP))
    out.append(_case("A-flag-log-full", "A", 31, 3000, mm=MM_DROP, flag=ST_LOG, nlog=2, log_cap=2))
    out.append(_case("A-log-last-row", "A", 31, 3000, mm=MM_DROP, nlog=1, log_cap=2))
    out.append(_case("A-flag-rows", "A", 31, 3000, flag=ST_ROWS, n_rows=32))
    out += [_case("A-flag-bound-%s" % tag, "A", 31, 3000, mm=mm, flag=ST_BOUND, E_bound=2999)
            for tag, mm in (("keep", MM_KEEP), ("drop", MM_DROP))]
    out += [_case("A-flag-group-%s" % tag, "A", 31, 9000, mode="oversize", mm=mm, flag=ST_GROUP)
            for tag, mm in (("keep", MM_KEEP), ("drop", MM_DROP))]
    return out


CASES = _build_cases()
CASE_IDS = [c.id for c in CASES]
assert len(set(CASE_IDS)) == len(CASE_IDS)


def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def case_graph(c):
    """the case's input graph (deterministic in its id)"""
    g = GEOMS[c.geom]
    rng = _rng(c.id)
    remove = decide(c.mm, THRESH)
    if c.mode != "oversize":
        return make_graph(rng, c.n, g.M, g.r, g.R, c.E, KI=c.KI, remove=remove, mode=c.mode)
    ii, jj, kk = make_graph(rng, c.n, g.M, g.r, g.R, c.E, KI=c.KI, remove=remove)
    # one patch of the newest frame carries 1025 factors: its (ii, jj, kk) repeated at scattered places
    at = rng.permutation(c.E)[:PATCH_FACTORS_MAX + 1]
    ii[at], jj[at], kk[at] = c.n - 1, c.n - 2, (c.n - 1) * g.M + 5
    return ii, jj, kk


def case_expected(c, graph=None):
    """editref's result for the case: edit() (with the capacities the case runs under) and remove"""
    g = GEOMS[c.geom]
    ii, jj, kk = case_graph(c) if graph is None else graph
    remove = decide(c.mm, THRESH)
    out = edit(ii, jj, kk, c.n, g.M, g.r, g.R, c.KI, remove, n_rows=c.n_rows, E_cap=g.E_cap)
    out["remove"] = remove
    return out


def capacity_violations(g, graph, dyn, pl=None):
    """what of the device's capacities the graph (after an edit) exceeds; empty: the step has to leave status 0"""
    ii, jj, kk = graph[0], graph[1], graph[2]
    pl = plan(ii, jj, kk, dyn["W"]) if pl is None else pl
    bad = []
    if len(kk) > g.E_cap:
        bad.append("E %d > E_cap %d" % (len(kk), g.E_cap))
    if pl["kk"]["ngroups"] > g.kk_cap or pl["ij"]["ngroups"] > g.ij_cap:
        bad.append("groups %d / %d > %d / %d" % (pl["kk"]["ngroups"], pl["ij"]["ngroups"], g.kk_cap, g.ij_cap))
    K_kk, K_ij = dyn["N"] * g.M - dyn["KLO"], dyn["W"] ** 2
    if K_kk > g.kkey_cap or K_ij > g.pkey_cap:
        bad.append("key ranges %d / %d > %d / %d" % (K_kk, K_ij, g.kkey_cap, g.pkey_cap))
    if len(kk):
        key_kk, key_ij = kk - dyn["KLO"], (jj - dyn["FLO"]) * dyn["W"] + (ii - dyn["FLO"])
        if key_kk.min() < 0 or key_kk.max() >= K_kk or key_ij.min() < 0 or key_ij.max() >= K_ij:
            bad.append("a key outside its range")
        if min(ii.min(), jj.min()) < dyn["FLO"] or max(ii.max(), jj.max()) >= dyn["N"]:
            bad.append("a frame index outside [FLO, N)")
        if np.diff(pl["kk"]["seg_start"]).max() > PATCH_FACTORS_MAX:
            bad.append("a patch with more than %d factors" % PATCH_FACTORS_MAX)
    return bad


def chain_steps(geom):
    """six consecutive edits on one graph, decisions CHAIN_PATTERN: yields dict(step, n, graph (ii, jj, kk) before the edit,
    remove, mm, out = edit(...)); each step's output graph and N are the next step's input"""
    g = GEOMS[geom]
    rng = _rng("chain-" + geom)
    n, E = CHAINS[geom]["n"], CHAINS[geom]["E"]
    graph = make_graph(rng, n, g.M, g.r, g.R, E)
    for step, remove in enumerate(CHAIN_PATTERN):
        mag = THRESH + (-1.0 if remove else 1.0) * rng.uniform(0.5, 5.0, 2)
        mm = (float(np.float32(mag[0])), float(np.float32(mag[1])))
        assert decide(mm, THRESH) == remove
        out = edit(graph[0], graph[1], graph[2], n, g.M, g.r, g.R, 4, remove, E_cap=g.E_cap)
        yield dict(step=step, n=n, graph=graph, remove=remove, mm=mm, out=out)
        graph, n = (out["graph"][0], out["graph"][1], out["graph"][2]), out["dyn"]["N"]
