"""The stand-alone graph primitives of csrc/graph.hip -- ramp_group_by, ramp_neighbors, ramp_group_by_small,
ramp_neighbors_from_groups, ramp_segment_softmax_sum -- and GraphPlan.build on top of them, against the numpy restatements of
tests/graphref.py, at the sizes where the kernels change path (graphref.E_EDGES, SMALL_K, NB_GROUP_SIZES, SOFTMAX_C).

Every integer output is compared exactly, over its whole documented extent: the entries a call has to write against the
reference, the rest (ukeys past G, seg_start past G + 1) against the fill they started with.  Every buffer a kernel writes,
the workspace included, lies between canaries (tests/guarded.py), and every launch runs twice on fresh buffers and has to
give the same bits.  The softmax is held, element by element, to graphref.softmax_tolerance around the float64 reference."""
import ctypes

import numpy as np
import pytest
import torch

import georef
import graphref as gr
from guarded import Flat
from trackerkit import cu

pytestmark = pytest.mark.gpu

I32, I64 = torch.int32, torch.int64


def _L():
    from rampvo_amd import _lib
    return _lib.lib(), _lib.stream()


def P(f):
    if f is None:
        return None
    return ctypes.c_void_p(f.address() if isinstance(f, Flat) else f.data_ptr())


def _twice(launch):
    """the launch on fresh buffers, two times over: the same bits (atomics decide no output), returned once"""
    a, b = launch(), launch()
    assert sorted(a) == sorted(b)
    for k in a:
        assert georef.same_bits(a[k], b[k]) if a[k].dtype.kind == "f" else np.array_equal(a[k], b[k]), k
    return a


def _finish(rc, bufs):
    torch.cuda.synchronize()
    assert rc == 0, rc
    for name, f in bufs.items():
        assert f.intact(), name
    return {k: f.t.cpu().numpy() for k, f in bufs.items() if k != "ws"}


def _group_outputs(E, gid=True, ukeys=True):
    b = dict(order=Flat(E, I32), seg_start=Flat(E + 1, I32), ngroups=Flat(1, I32))
    if gid:
        b["gid"] = Flat(E, I32)
    if ukeys:
        b["ukeys"] = Flat(E, I64)
    return b


def _group_by(keys, bound, gid=True, ukeys=True):
    L, st = _L()
    E = len(keys)
    d_keys = cu(keys)

    def launch():
        b = _group_outputs(E, gid, ukeys)
        nbytes = L.ramp_group_by_workspace_bytes(E)
        b["ws"] = Flat(nbytes, torch.uint8, rows=4)
        rc = L.ramp_group_by(P(d_keys), E, int(bound), P(b["order"]), P(b.get("gid")), P(b["seg_start"]), P(b.get("ukeys")),
                             P(b["ngroups"]), P(b["ws"]), nbytes, st)
        return _finish(rc, b)
    return _twice(launch)


def _group_by_small(a, b_, mul, sub, K, max_groups, gid=True, ukeys=True):
    L, st = _L()
    E = len(a)
    d_a, d_b = cu(a), None if b_ is None else cu(b_)

    def launch():
        b = _group_outputs(E, gid, ukeys)
        nbytes = L.ramp_group_by_small_workspace_bytes(E, K)
        b["ws"] = Flat(nbytes, torch.uint8, rows=4)
        rc = L.ramp_group_by_small(P(d_a), P(d_b), int(mul), int(sub), K, E, P(b["order"]), P(b.get("gid")), P(b["seg_start"]),
                                   P(b.get("ukeys")), P(b["ngroups"]), max_groups, P(b["ws"]), nbytes, st)
        return _finish(rc, b)
    return _twice(launch)


def _expected_groups(keys, ukeys_offset=0):
    """the whole extent of every output: the reference, then the fill"""
    r = gr.group_by(keys)
    E, G = len(keys), r["G"]
    seg = np.full(E + 1, -77, np.int32)
    seg[:G + 1] = r["seg_start"]
    uk = np.full(E, -77, np.int64)
    uk[:G] = r["ukeys"] + ukeys_offset
    return dict(order=r["order"], gid=r["gid"], seg_start=seg, ukeys=uk, ngroups=np.array([G], np.int32))


def _same_groups(got, exp, what):
    for k in got:
        assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k)


# ------------------------------------------------------------------------------------------------ ramp_group_by
@pytest.mark.parametrize("kind", gr.GROUP_BY_KINDS)
def test_group_by(kind):
    for E in gr.E_EDGES:
        keys, bounds = gr.keys_for_group_by(kind, E)
        exp = _expected_groups(keys)
        for bound in bounds:
            _same_groups(_group_by(keys, bound), exp, (kind, E, bound))
        if E in (0, 257, 4099):                         # the optional outputs left out, one at a time and both
            for gid, ukeys in ((False, True), (True, False), (False, False)):
                _same_groups(_group_by(keys, bounds[-1], gid, ukeys), exp, (kind, E, gid, ukeys))


# ------------------------------------------------------------------------------------------------ ramp_neighbors
def _neighbors(kk, jj, kb, jb):
    L, st = _L()
    E = len(kk)
    d_kk, d_jj = cu(kk), cu(jj)

    def launch():
        nbytes = L.ramp_neighbors_workspace_bytes(E)
        b = dict(ix=Flat(E, I64), jx=Flat(E, I64), ws=Flat(nbytes, torch.uint8, rows=4))
        rc = L.ramp_neighbors(P(d_kk), P(d_jj), P(b["ix"]), P(b["jx"]), E, int(kb), int(jb), P(b["ws"]), nbytes, st)
        return _finish(rc, b)
    return _twice(launch)


@pytest.mark.parametrize("kind", gr.NEIGHBOR_KINDS)
def test_neighbors(kind):
    for E in gr.E_EDGES:
        kk, jj, settings = gr.neighbor_graph(kind, E)
        ix, jx, _ = gr.neighbors(kk, jj)
        for kb, jb in settings:
            got = _neighbors(kk, jj, kb, jb)
            assert np.array_equal(got["ix"], ix) and np.array_equal(got["jx"], jx), (kind, E, kb, jb)


# ------------------------------------------------------------------------------------------------ ramp_group_by_small
def _small_against_both(a, b, mul, sub, K, what):
    """every max_groups setting against graphref and against ramp_group_by on the same keys, field by field"""
    keys = gr.small_keys(a, b, mul, sub)
    exp = _expected_groups(keys, sub)
    radix = _group_by(keys + sub, K + sub)
    _same_groups(radix, exp, (what, "ramp_group_by"))
    G = int(exp["ngroups"][0])
    for mg in (0, G, G + 1):
        got = _group_by_small(a, b, mul, sub, K, mg)
        _same_groups(got, exp, (what, mg))
        _same_groups(got, radix, (what, mg, "ramp_group_by"))


@pytest.mark.parametrize("K", gr.SMALL_K)
def test_group_by_small(K):
    for E in gr.E_EDGES:
        for kind in gr.SMALL_KINDS:
            _small_against_both(gr.small_case(kind, K, E), None, 1, 0, K, (K, E, kind))


@pytest.mark.parametrize("K", [255, 4096, 4097])
def test_group_by_small_long_segment(K):
    keys = gr.long_segment_case(K)
    _small_against_both(keys + 1000, None, 1, 1000, K, ("long", K))
    exp = _expected_groups(keys)
    for gid, ukeys in ((False, True), (True, False)):
        _same_groups(_group_by_small(keys, None, 1, 0, K, 0, gid, ukeys), exp, ("long", K, gid, ukeys))


@pytest.mark.parametrize("W", [9, 64, 65])               # K = 81, 4096 (the last LDS histogram), 4225
def test_group_by_small_pair_form(W):
    for E in (257, 4099):
        a, b, mul, sub, K = gr.pair_case(W, E, 70)
        _small_against_both(a, b, mul, sub, K, ("pair", W, E))


@pytest.mark.parametrize("K0", [4096, 10000])            # the LDS histogram and the global one
def test_group_by_small_key_out_of_range_gives_the_empty_grouping(K0):
    from rampvo_amd import _lib
    L, st = _L()
    for name, a, b, mul, sub, K in gr.bad_key_cases(K0):
        E = len(a)
        for mg in (0, E):
            got = _group_by_small(a, b, mul, sub, K, mg)
            assert got["ngroups"][0] == 0 and got["seg_start"][0] == 0, (name, K, mg, got["ngroups"], got["seg_start"][:2])
        # what the consumers then do: nothing
        d = {k: cu(got[k]) for k in ("order", "seg_start", "ngroups")}
        ix, jx, kj, y = Flat(E, I64), Flat(E, I64), Flat(E, I32), Flat((E, 4), torch.float32)
        before = [f.snapshot() for f in (ix, jx, kj, y)]
        x, d_jj = torch.ones((E, 4), device="cuda"), cu(a)
        assert L.ramp_neighbors_from_groups(P(d["order"]), P(d["seg_start"]), P(d["ngroups"]), P(d_jj), P(ix), P(jx), P(kj), E,
                                            E, st) == 0
        assert L.ramp_segment_softmax_sum(P(x), P(x), P(d["order"]), P(d["seg_start"]), P(d["ngroups"]), P(y), E, 4, E,
                                          _lib.dtype_code(x), st) == 0
        torch.cuda.synchronize()
        assert all(f.unchanged(s) for f, s in zip((ix, jx, kj, y), before)), name


# ------------------------------------------------------------------------------------------------ ramp_neighbors_from_groups
def _neighbors_from_groups(groups, jj, max_groups, want_kj):
    L, st = _L()
    E = len(jj)
    d = {k: cu(groups[k]) for k in ("order", "seg_start")}
    d_ng, d_jj = cu(np.array([groups["G"]], np.int32)), cu(jj)

    def launch():
        b = dict(ix=Flat(E, I64), jx=Flat(E, I64))
        if want_kj:
            b["kj"] = Flat(E, I32)
        rc = L.ramp_neighbors_from_groups(P(d["order"]), P(d["seg_start"]), P(d_ng), P(d_jj), P(b["ix"]), P(b["jx"]),
                                          P(b.get("kj")), E, max_groups, st)
        return _finish(rc, b)
    return _twice(launch)


def test_neighbors_from_groups_every_group_length():
    """groups of 1 .. 3000 edges in one graph: below, at and above the 64-lane stride and the 1024-entry staging"""
    kk, jj = gr.sized_groups(gr.NB_GROUP_SIZES)
    ix, jx, kj = gr.neighbors(kk, jj)
    groups = gr.group_by(kk)
    G = groups["G"]
    sort = _neighbors(kk, jj, int(kk.max()) + 1, int(jj.max()) + 1)
    assert np.array_equal(sort["ix"], ix) and np.array_equal(sort["jx"], jx)
    for mg in (G, G + 7):
        for want_kj in (True, False):
            got = _neighbors_from_groups(groups, jj, mg, want_kj)
            sizes = dict(zip(*np.unique(kk, return_counts=True)))
            wrong = sorted({int(sizes[k]) for k in kk[(got["ix"] != ix) | (got["jx"] != jx)]})
            assert not wrong, ("groups of these lengths have wrong links", wrong, mg, want_kj)
            assert np.array_equal(got["ix"], sort["ix"]) and np.array_equal(got["jx"], sort["jx"])
            if want_kj:
                assert np.array_equal(got["kj"], kj), (mg, sorted({int(sizes[k]) for k in kk[kj[got["kj"] != kj]]}))


def test_neighbors_from_groups_of_the_device_grouping():
    """the two kernels chained as GraphPlan.build chains them: ramp_group_by_small's outputs straight into the links"""
    from rampvo_amd import ops
    kk, jj = gr.sized_groups((1025, 5, 64, 1, 2000), seed=1, n_jj=3)
    ix, jx, kj = gr.neighbors(kk, jj)
    for _ in range(2):
        g = ops.group_by_small(cu(kk), None, 1, 2, int(kk.max()) - 1, 5)
        got = ops.neighbors_from_groups(g, cu(jj), 5, want_kj=True)
        for out, ref in zip(got, (ix, jx, kj)):
            assert np.array_equal(out.cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------------ GraphPlan.build
def _plan_fields(p, E):
    G_kk, G_ij = int(p.g_kk.ngroups.item()), int(p.g_ij.ngroups.item())
    uk = p.g_ij.ukeys[:G_ij].cpu().numpy()
    return dict(ix=p.ix.cpu().numpy(), jx=p.jx.cpu().numpy(), kk_order=p.g_kk.order[:E].cpu().numpy(),
                kk_gid=p.g_kk.gid[:E].cpu().numpy(), kk_seg=p.g_kk.seg_start[:G_kk + 1].cpu().numpy(), kk_G=np.array(G_kk),
                kk_ukeys=p.g_kk.ukeys[:G_kk].cpu().numpy(), ij_order=p.g_ij.order[:E].cpu().numpy(),
                ij_gid=p.g_ij.gid[:E].cpu().numpy(), ij_seg=p.g_ij.seg_start[:G_ij + 1].cpu().numpy(), ij_G=np.array(G_ij),
                ij_pairs=np.stack([uk // p.pair_mul, uk % p.pair_mul]))          # (jj, ii): the multiplier differs by path


@pytest.mark.parametrize("heavy", [None, (60, 1100)], ids=["tracker", "patch_with_1100_factors"])
def test_graph_plan_counting_path_equals_sort_path(heavy):
    from rampvo_amd.net import GraphPlan
    from scenes import ba_scene
    N, M = 9, 14
    s = ba_scene(seed=5, n_frames=N, M=M, lifetime=4, n_total_frames=16)
    ii, jj, kk = gr.tracker_graph(s, heavy)
    E = len(kk)
    d = [cu(x) for x in (ii, jj, kk)]
    ix, jx, kj = gr.neighbors(kk, jj)
    g_kk, g_ij = gr.group_by(kk), gr.group_by(jj * N + ii)
    ref = dict(ix=ix, jx=jx, kk_order=g_kk["order"], kk_gid=g_kk["gid"], kk_seg=g_kk["seg_start"], kk_G=np.array(g_kk["G"]),
               kk_ukeys=g_kk["ukeys"], ij_order=g_ij["order"], ij_gid=g_ij["gid"], ij_seg=g_ij["seg_start"],
               ij_G=np.array(g_ij["G"]), ij_pairs=np.stack([g_ij["ukeys"] // N, g_ij["ukeys"] % N]))
    builds = dict(sort=lambda: GraphPlan.build(*d), sort_bounded=lambda: GraphPlan.build(*d, kk_bound=N * M, jj_bound=N),
                  count=lambda: GraphPlan.build(*d, max_kk=N * M, max_ij=N * N, kk_range=(0, N * M), frame_range=(0, N)))
    for name, build in builds.items():
        for _ in range(2):
            p = build()
            got = _plan_fields(p, E)
            assert (p.kj is not None) == (name == "count")
            for k in ref:
                assert np.array_equal(got[k], ref[k]), (name, k)
            if p.kj is not None:
                assert np.array_equal(p.kj.cpu().numpy(), kj), name


# ------------------------------------------------------------------------------------------------ ramp_segment_softmax_sum
PREFILL = 3.5


def _softmax(fx, gx, groups, max_groups, dtype):
    L, st = _L()
    from rampvo_amd import _lib
    E, C = fx.shape
    d_fx, d_gx = cu(fx).to(dtype), cu(gx).to(dtype)
    d = {k: cu(groups[k]) for k in ("order", "seg_start")}
    d_ng = cu(np.array([groups["G"]], np.int32))

    def launch():
        b = dict(y=Flat((max_groups, C), dtype, canary=1024.0, fill=PREFILL))
        rc = L.ramp_segment_softmax_sum(P(d_fx), P(d_gx), P(d["order"]), P(d["seg_start"]), P(d_ng), P(b["y"]), E, C, max_groups,
                                        _lib.dtype_code(d_fx), st)
        torch.cuda.synchronize()
        assert rc == 0 and b["y"].intact()
        return dict(y=b["y"].t.float().cpu().numpy())
    return _twice(launch)["y"]


@pytest.mark.parametrize("C", gr.SOFTMAX_C)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_segment_softmax_sum(dtype, C):
    half = dtype == torch.float16
    for kind in gr.SOFTMAX_KINDS:
        fx, gx, keys = gr.softmax_case(C, kind, half)
        groups = gr.group_by(keys)
        G = groups["G"]
        ref, bound = gr.segment_softmax_sum(fx, gx, groups["gid"], G)
        n = gr.group_sizes(keys)[:, None]
        for mg in (G, G + 5):
            y = _softmax(fx, gx, groups, mg, dtype).astype(np.float64)
            assert (y[G:] == PREFILL).all(), "rows >= G are untouched"
            y = y[:G]
            assert np.array_equal(np.isnan(y), np.isnan(ref)), (kind, "NaN exactly where every gx of the column is -inf")
            assert np.isnan(ref).any() == (kind == "all_inf")
            ok = ~np.isnan(ref)
            tol = gr.softmax_tolerance(n, bound, ref, half)
            err = np.abs(y - ref)
            worst = float((err[ok] / np.maximum(tol[ok], 1e-300)).max())
            print("softmax %s C=%d %s G+%d: worst error / bound = %.3f" % ("fp16" if half else "fp32", C, kind, mg - G, worst))
            assert np.isfinite(y[ok]).all() and (err[ok] <= tol[ok]).all(), (kind, mg, worst)
