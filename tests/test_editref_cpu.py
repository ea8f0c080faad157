"""The numpy restatement of the keyframe edit and the graph plan (tests/editref.py) against the project's host-side code
(ramp_graph_edit_host, the oracle-side tracker's _graph_edit, Ramp_vo._new_edges) and against brute force, and the
capacity check of every case tests/test_graph_edit_gpu.py expects status 0 from: what the kernels are compared with has to
be right, and a clean status has to be what the capacities promise.  Everything is exact."""
import numpy as np
import pytest

import editref as er


def _host_edit(ii, jj, kk, M, k, n_after, R):
    from rampvo_amd import _lib
    E = len(ii)
    out = np.empty((4, max(E, 1)), np.int64)
    ii, jj, kk = (np.ascontiguousarray(a, np.int64) for a in (ii, jj, kk))
    m = _lib.lib().ramp_graph_edit_host(ii.ctypes.data, jj.ctypes.data, kk.ctypes.data, None, E, M, k, n_after, R,
                                        out.ctypes.data, max(E, 1), None)
    return out[:, :m]


def _oracle_edit(ii, jj, kk, M, n, R, KI, remove):
    from oracle.host_cpu import RampVoCPU
    fake = type("T", (), {})()
    fake.cfg = type("C", (), dict(KEYFRAME_INDEX=KI, REMOVAL_WINDOW=R))()
    fake.M, fake.n, fake._ii, fake._jj, fake._kk = M, n, ii, jj, kk
    return RampVoCPU._graph_edit(fake, remove)


@pytest.mark.parametrize("remove", [False, True])
@pytest.mark.parametrize("mode", ["mixed", "kept", "touch_k"])
@pytest.mark.parametrize("n", [5, 13, 23, 31])
def test_edit_matches_host_edit_and_oracle_tracker(n, mode, remove):
    M, r, R, KI, E = 8, 13, 22, 4, 5000
    rng = np.random.default_rng(3 + n)
    ii, jj, kk = er.make_graph(rng, n, M, r, R, E, KI=KI, remove=remove, mode=mode)
    assert np.array_equal(kk // M, ii) and np.abs(ii - jj).max() <= r - 1
    assert min(ii.min(), jj.min()) >= 0 and max(ii.max(), jj.max()) < n and ii.min() >= max(n - R - 3, 0)
    out = er.edit(ii, jj, kk, n, M, r, R, KI, remove)
    Ek, d = out["Ek"], out["dyn"]
    n_after = n - 1 if remove else n
    host = _host_edit(ii, jj, kk, M, n - KI if remove else -1, n_after, R)
    assert host.shape[1] == Ek and np.array_equal(host, out["graph"][:, :Ek])
    ref = _oracle_edit(ii, jj, kk, M, n, R, KI, remove)
    assert ref["n"] == n_after == d["NROW"] and len(ref["ii"]) == Ek
    for row, name in enumerate(("ii", "jj", "kk")):
        assert np.array_equal(out["graph"][row, :Ek], ref[name])
    assert np.array_equal(out["idx"], ref["idx"] if ref["idx"] is not None else np.arange(E))
    if mode == "kept":
        assert Ek == E
    if mode == "touch_k" and remove:
        assert Ek == 0 and d["FLO"] == max(n_after + 1 - r, 0)
    assert (d["N"], d["EPREV"], d["EKEPT"], d["E"], d["K"], d["NPREV"]) == (n_after + 1, E, Ek, Ek + out["ne"], n - KI, n)
    assert d["W"] == d["N"] - d["FLO"] and d["KLO"] <= out["graph"][2].min() and d["KLO"] % M == 0


@pytest.mark.parametrize("M", [37, 48])
def test_new_factors_match_the_tracker_new_edges(M):
    from rampvo_amd.Ramp_vo import Ramp_vo
    r = 13
    fake = type("T", (), {})()
    fake.cfg = type("C", (), dict(PATCH_LIFETIME=r))()
    fake.M, fake._edge_tmpl = M, None
    fake._new_edges_at = lambda n1: Ramp_vo._new_edges_at(fake, n1)
    g = er.Geometry("t", "default", M, r, 22)
    for n1 in (1, 2, r - 1, r, r + 1, 31, 40):
        mine, theirs = er.new_factors(n1, M, r), Ramp_vo._new_edges(fake, n1)
        assert all(np.array_equal(a, b) for a, b in zip(mine, theirs)), n1
        assert len(mine[2]) == g.ne(n1) <= g.new_cap


def test_decide_is_strict_and_in_double():
    for tag, mm, dropped in er.DECISIONS:
        assert er.decide(mm, er.THRESH) == dropped, tag
    a, b = np.float32(15.0), np.float32(er.DECISIONS[1][1][1])
    assert b < a and float(a + b) == 30.0                    # the float32 sum rounds up to the threshold: kept
    assert float(a) + float(b) == 30.0 - 2.0 ** -20
    assert er.decide(er.MM_DROP, er.THRESH) and not er.decide(er.MM_KEEP, er.THRESH)


def test_plan_against_brute_force():
    rng = np.random.default_rng(5)
    M, n, E = 6, 9, 700
    ii, jj, kk = er.make_graph(rng, n, M, 4, 7, E)
    W = n - int(min(ii.min(), jj.min()))
    pl = er.plan(ii, jj, kk, W)
    for name, key in (("kk", kk), ("ij", jj * W + ii)):
        g = pl[name]
        uk = sorted(set(key.tolist()))
        assert g["ukeys"].tolist() == uk and g["ngroups"] == len(uk)
        members = [[e for e in range(E) if key[e] == u] for u in uk]                 # ascending factor index
        assert g["order"].tolist() == [e for m in members for e in m]
        assert g["seg_start"].tolist() == np.cumsum([0] + [len(m) for m in members]).tolist()
        assert g["gid"].tolist() == [uk.index(v) for v in key.tolist()]
    order = sorted(range(E), key=lambda e: (kk[e], jj[e], e))
    assert pl["kj"].tolist() == order
    for pos, e in enumerate(order):
        prev = order[pos - 1] if pos > 0 and kk[order[pos - 1]] == kk[e] else -1
        nxt = order[pos + 1] if pos + 1 < E and kk[order[pos + 1]] == kk[e] else -1
        assert (pl["ix"][e], pl["jx"][e]) == (prev, nxt)
    empty = er.plan(ii[:0], jj[:0], kk[:0], 3)
    assert empty["kk"]["ngroups"] == 0 and empty["kk"]["seg_start"].tolist() == [0] and len(empty["kj"]) == 0


def test_shift_rows_restates_the_reference_loop():
    rng = np.random.default_rng(6)
    for ring, nrows in ((0, 48), (er.MEM, er.MEM)):
        buf = rng.integers(0, 1 << 30, (nrows, 3))
        for n, KI in ((35, 4), (33, 2), (39, 8), (35, 8), (20, 4)):
            k = n - KI
            ref = buf.copy()
            for i in range(k, n - 1):                        # ramp/Ramp_vo.py:258-268
                ref[i % ring if ring else i] = ref[(i + 1) % ring if ring else i + 1]
            assert np.array_equal(er.shift_rows(buf, k, n, ring), ref)
            untouched = np.setdiff1d(np.arange(nrows), [(i % ring if ring else i) for i in range(k, n - 1)])
            assert np.array_equal(ref[untouched], buf[untouched])


def test_case_table_reaches_what_it_is_for():
    cases = {c.id: c for c in er.CASES}
    blocks = lambda c: -(-c.E // er.EDIT_BLOCK)
    per = lambda c: -(-blocks(c) // 256)
    assert per(cases["C-size-264000-drop"]) == 2 and per(cases["D-size-820000-drop"]) == 4
    assert blocks(cases["C-size-266300-drop"]) % 2 == 1 and blocks(cases["D-size-820000-drop"]) % 4 != 0
    A, D = er.GEOMS["A"], er.GEOMS["D"]
    assert (A.E_cap, er.GEOMS["B"].E_cap, er.GEOMS["C"].E_cap, D.E_cap) == (28800, 22200, 274560, 858000)
    assert A.kkey_cap <= 12288 and A.pkey_cap <= 12288 and D.kkey_cap == 13200 > 12288
    assert sorted({c.KI - 1 for c in er.CASES if "shift" in c.id}) == [1, 2, 3, 4, 5, 7]
    assert {c.flag for c in er.CASES} == {0, er.ST_CAP, er.ST_GROUP, er.ST_LOG, er.ST_BOUND, er.ST_ROWS}


@pytest.mark.parametrize("cid", [c.id for c in er.CASES if not c.flag])
def test_unflagged_case_stays_inside_the_capacities(cid):
    c = next(c for c in er.CASES if c.id == cid)
    g = er.GEOMS[c.geom]
    assert c.n >= c.KI + 1 and c.log_cap > c.nlog
    ii, jj, kk = er.case_graph(c)
    assert len(ii) == c.E and np.array_equal(kk // g.M, ii) and np.abs(ii - jj).max(initial=0) <= g.r - 1
    out = er.case_expected(c, (ii, jj, kk))
    assert out["status"] == 0 and out["dyn"]["NROW"] + 2 <= 2048
    assert er.capacity_violations(g, out["graph"], out["dyn"]) == []
    if c.mode == "kept":
        assert out["Ek"] == c.E
    if "fills-cap" in c.id:
        assert out["dyn"]["E"] == g.E_cap
    if c.mode == "touch_k" and out["remove"]:
        assert out["Ek"] == 0


def test_flagged_cases_raise_exactly_their_bit():
    for c in er.CASES:
        if not c.flag:
            continue
        g = er.GEOMS[c.geom]
        out = er.case_expected(c)
        bad = er.capacity_violations(g, out["graph"], out["dyn"])
        if c.flag == er.ST_CAP:
            assert out["status"] == er.ST_CAP and out["dyn"]["E"] == g.E_cap and out["Ek"] == c.E and bad == []
        elif c.flag == er.ST_ROWS:
            assert out["status"] == er.ST_ROWS and (out["dyn"]["NROW"], out["dyn"]["N"]) == (c.n_rows - 2, c.n_rows - 1)
            assert bad == []
        elif c.flag == er.ST_GROUP:
            assert out["status"] == 0 and len(bad) == 1 and "more than 1024" in bad[0]
            sizes = np.diff(er.plan(*out["graph"][:3], out["dyn"]["W"])["kk"]["seg_start"])
            assert (sizes > er.PATCH_FACTORS_MAX).sum() == 1
        elif c.flag == er.ST_LOG:
            assert out["status"] == 0 and bad == [] and out["remove"] and c.nlog == c.log_cap
        else:
            assert c.flag == er.ST_BOUND and out["status"] == 0 and bad == [] and c.E_bound == c.E - 1


@pytest.mark.parametrize("geom", sorted(er.CHAINS))
def test_chain_stays_inside_the_capacities(geom):
    g = er.GEOMS[geom]
    steps = list(er.chain_steps(geom))
    assert [s["remove"] for s in steps] == list(er.CHAIN_PATTERN)
    ranges = []
    for s in steps:
        out = s["out"]
        assert out["status"] == 0 and er.capacity_violations(g, out["graph"], out["dyn"]) == [], s["step"]
        ranges.append((out["dyn"]["N"] * g.M - out["dyn"]["KLO"], out["dyn"]["W"] ** 2))
    # the histograms a plan leaves behind are not the next plan's: the factor count moves both ways along the chain and the
    # key ranges change (in a valid sequence of frames they can only grow until the removal window is full)
    sizes = [s["out"]["dyn"]["E"] for s in steps]
    assert any(b < a for a, b in zip(sizes, sizes[1:])) and any(b > a for a, b in zip(sizes, sizes[1:]))
    assert len(set(ranges)) > 1
    # the factors a step adds (row -1) are kept by the next one under their own index
    for a, b in zip(steps[:-1], steps[1:]):
        new = np.nonzero(a["out"]["graph"][3] == -1)[0]
        assert len(new) and np.isin(new, b["out"]["graph"][3]).any()
