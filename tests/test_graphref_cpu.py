"""tests/graphref.py against brute-force definitions (O(E^2) loops), against the existing oracle (oracle.neighbors,
oracle.backend_cpu.group_by, oracle.segment_softmax_sum), and its case generators against what they claim to produce.
No GPU."""
import math

import numpy as np
import pytest

import graphref as gr


# ----------------------------------------------------------------------------------------------- brute force
def _brute_group_by(keys):
    E = len(keys)
    rank = [sum(1 for f in range(E) if keys[f] < keys[e] or (keys[f] == keys[e] and f < e)) for e in range(E)]
    order = np.empty(E, np.int32)
    for e in range(E):
        order[rank[e]] = e
    ukeys = sorted(set(int(k) for k in keys))
    gid = np.array([sum(1 for u in ukeys if u < keys[e]) for e in range(E)], np.int32)
    seg = [sum(1 for f in range(E) if keys[f] < u) for u in ukeys] + [E]
    return order, gid, np.array(seg, np.int32), np.array(ukeys, np.int64)


def _brute_neighbors(kk, jj):
    E = len(kk)
    ix, jx = np.full(E, -1, np.int64), np.full(E, -1, np.int64)
    for e in range(E):
        before = [(jj[f], f) for f in range(E) if kk[f] == kk[e] and (jj[f], f) < (jj[e], e)]
        after = [(jj[f], f) for f in range(E) if kk[f] == kk[e] and (jj[f], f) > (jj[e], e)]
        if before:
            ix[e] = max(before)[1]
        if after:
            jx[e] = min(after)[1]
    kj = sorted(range(E), key=lambda e: (kk[e], jj[e], e))
    return ix, jx, np.array(kj, np.int32)


def _small_graphs():
    rng = np.random.default_rng(0)
    yield np.zeros(0, np.int64), np.zeros(0, np.int64)
    yield np.array([4], np.int64), np.array([1], np.int64)
    for E, nk, nj in ((2, 1, 1), (17, 3, 2), (100, 9, 4), (200, 200, 3), (200, 1, 2), (150, 40, 40)):
        yield rng.integers(0, nk, E).astype(np.int64) * 5, rng.integers(0, nj, E).astype(np.int64)


def test_group_by_against_brute_force():
    for keys, _ in _small_graphs():
        g = gr.group_by(keys)
        order, gid, seg, uk = _brute_group_by(keys)
        assert g["G"] == len(uk) and g["order"].dtype == np.int32 and g["ukeys"].dtype == np.int64
        assert np.array_equal(g["order"], order) and np.array_equal(g["gid"], gid)
        assert np.array_equal(g["seg_start"], seg) and np.array_equal(g["ukeys"], uk)
        # the properties the header states
        assert np.array_equal(g["ukeys"][g["gid"]], keys)
        for q in range(g["G"]):
            run = g["order"][g["seg_start"][q]:g["seg_start"][q + 1]]
            assert (keys[run] == uk[q]).all() and (np.diff(run) > 0).all()


def test_neighbors_against_brute_force():
    for kk, jj in _small_graphs():
        ix, jx, kj = gr.neighbors(kk, jj)
        bix, bjx, bkj = _brute_neighbors(kk, jj)
        assert ix.dtype == np.int64 and np.array_equal(ix, bix) and np.array_equal(jx, bjx) and np.array_equal(kj, bkj)
        linked = np.flatnonzero(jx >= 0)
        assert np.array_equal(ix[jx[linked]], linked)          # the two links are each other's inverse


def test_small_keys():
    a, b = np.array([5, 6, 9], np.int64), np.array([9, 5, 7], np.int64)
    assert gr.small_keys(a, b, 5, 30).tolist() == [4, 5, 22]
    assert gr.small_keys(a, None, 1, 5).tolist() == [0, 1, 4]
    big = gr.small_keys(np.array([3_000_000_000], np.int64), None, 1_000_000, 7)
    assert big.dtype == np.int64 and int(big[0]) == 3_000_000_000 * 1_000_000 - 7     # no 32-bit step anywhere


def test_segment_softmax_sum_against_brute_force():
    rng = np.random.default_rng(1)
    E, C, G = 60, 3, 4
    gid = rng.integers(0, G, E)
    gid[:G] = np.arange(G)
    fx, gx = rng.normal(size=(E, C)), 3 * rng.normal(size=(E, C))
    gx[gid == 1, 0] = -np.inf                                   # a whole column of one group
    gx[np.flatnonzero(gid == 2)[0], 1] = -np.inf                # one row of another
    y, bound = gr.segment_softmax_sum(fx, gx, gid, G)
    for g in range(G):
        rows = [e for e in range(E) if gid[e] == g]
        for c in range(C):
            m = max(gx[e, c] for e in rows)
            if m == -math.inf:
                assert np.isnan(y[g, c]) and np.isnan(bound[g, c])
                continue
            s = sum(math.exp(gx[e, c] - m) for e in rows)
            ref = sum(math.exp(gx[e, c] - m) / s * fx[e, c] for e in rows)
            refb = sum(math.exp(gx[e, c] - m) / s * abs(fx[e, c]) for e in rows)
            assert abs(y[g, c] - ref) <= 1e-14 * refb and abs(bound[g, c] - refb) <= 1e-14 * refb
    assert np.isnan(y[1, 0]) and np.isnan(y).sum() == 1


# ----------------------------------------------------------------------------------------------- the oracle
def _all_integer_cases():
    for E in gr.E_EDGES:
        for kind in gr.NEIGHBOR_KINDS:
            yield gr.neighbor_graph(kind, E)[:2]
    yield gr.sized_groups(gr.NB_GROUP_SIZES)


def test_neighbors_equal_oracle():
    import oracle as orc
    for kk, jj in _all_integer_cases():
        ix, jx, _ = gr.neighbors(kk, jj)
        rix, rjx = orc.neighbors(kk, jj)
        assert np.array_equal(ix, rix) and np.array_equal(jx, rjx)


def test_group_by_equals_oracle_backend():
    import torch
    from oracle import backend_cpu
    for E in gr.E_EDGES:
        for kind in gr.GROUP_BY_KINDS:
            keys, _ = gr.keys_for_group_by(kind, E)
            g, o = gr.group_by(keys), backend_cpu.group_by(torch.from_numpy(keys))
            assert g["G"] == int(o.ngroups)
            for name in ("order", "gid", "seg_start", "ukeys"):
                assert np.array_equal(g[name], getattr(o, name).numpy()), (kind, E, name)


@pytest.mark.parametrize("kind", ["normal", "equal", "peak", "some_inf"])
def test_segment_softmax_sum_near_oracle(kind):
    """the fp32 oracle lies within the bound the GPU kernel is held to (it rounds in the same places)"""
    import oracle as orc
    fx, gx, keys = gr.softmax_case(129, kind)
    g = gr.group_by(keys)
    y, bound = gr.segment_softmax_sum(fx, gx, g["gid"], g["G"])
    out = orc.segment_softmax_sum(fx, gx, g["gid"].astype(np.int64), g["G"])
    n = gr.group_sizes(keys)[:, None]
    assert np.isfinite(y).all() and (np.abs(out - y) <= gr.softmax_tolerance(n, bound)).all()


# ----------------------------------------------------------------------------------------------- the generators
def test_group_by_key_sets():
    for E in gr.E_EDGES:
        for kind in gr.GROUP_BY_KINDS:
            keys, bounds = gr.keys_for_group_by(kind, E)
            assert keys.dtype == np.int64 and len(keys) == E and 0 in bounds
            assert (keys >= 0).all() and all(b == 0 or (keys < b).all() for b in bounds)
    E = 4099
    assert len(set(gr.keys_for_group_by("equal", E)[0])) == 1
    d = gr.keys_for_group_by("descending", E)[0]
    assert (np.diff(d) < 0).all()
    z, zb = gr.keys_for_group_by("zeros", E)
    assert not z.any() and zb == (0, 1)
    p, pb = gr.keys_for_group_by("pow2", E)
    assert pb[1] == 256 == int(p.max()) + 1
    h, hb = gr.keys_for_group_by("huge", E)
    assert hb == (0,) and (h >= (1 << 62) - 3).all() and (h < (1 << 62)).any() and (h >= (1 << 62)).any()


def _bits(bound):
    return 63 if bound <= 0 else max(1, int(bound - 1).bit_length())


def test_neighbor_graphs():
    for E in gr.E_EDGES:
        for kind in gr.NEIGHBOR_KINDS:
            kk, jj, settings = gr.neighbor_graph(kind, E)
            assert len(kk) == len(jj) == E and (kk >= 0).all() and (jj >= 0).all()
            for kb, jb in settings:
                assert (kb == 0 or (kk < kb).all()) and (jb == 0 or (jj < jb).all())
            one_pass = [s for s in settings if s[0] > 0 and s[1] > 0 and _bits(s[0]) + _bits(s[1]) <= 62]
            two_bounded = [s for s in settings if s[0] > 0 and s[1] > 0 and _bits(s[0]) + _bits(s[1]) > 62]
            assert (0, 0) in settings and one_pass and two_bounded
            assert any(s[0] > 0 and s[1] == 0 for s in settings) and any(s[0] == 0 and s[1] > 0 for s in settings)
    kk, jj, _ = gr.neighbor_graph("ties", 4099)
    assert gr.group_sizes(kk * 8 + jj).max() >= 8                 # many edges share (kk, jj)
    assert len(set(gr.neighbor_graph("single", 4099)[0])) == 1
    kk, jj, _ = gr.neighbor_graph("distinct", 4099)
    assert len(set(kk)) == 4099
    ix, jx, _ = gr.neighbors(kk, jj)
    assert (ix == -1).all() and (jx == -1).all()


def test_small_cases():
    assert 4096 in gr.SMALL_K and 4097 in gr.SMALL_K and 1024 in gr.SMALL_K and 1025 in gr.SMALL_K
    for K in gr.SMALL_K:
        for E in gr.E_EDGES:
            for kind in gr.SMALL_KINDS:
                keys = gr.small_case(kind, K, E)
                assert len(keys) == E and (keys >= 0).all() and (keys < K).all()
        assert len(set(gr.small_case("three", K, 4099))) == min(3, len({K // 3, K // 2, K - 1}))
        assert set(gr.small_case("ends", K, 4099)) == {0, K - 1}
        if K <= 1025:
            assert len(set(gr.small_case("dense", K, 4099))) > 0.9 * K
        keys = gr.long_segment_case(K)
        assert (keys >= 0).all() and (keys < K).all()
        assert gr.group_sizes(keys).max() == gr.LONG_SEGMENT if K > 1 else len(keys) == gr.LONG_SEGMENT + 300
    a, b, mul, sub, K = gr.pair_case(9, 4099, 70)
    k = gr.small_keys(a, b, mul, sub)
    assert sub != 0 and K == 81 and k.min() == 0 and k.max() == 80 and len(set(k)) == 81


def test_bad_key_cases():
    for K0, lds in ((4096, True), (10000, False)):
        names = []
        for name, a, b, mul, sub, K in gr.bad_key_cases(K0):
            k = gr.small_keys(a, b, mul, sub)
            out = (k < 0) | (k >= K)
            assert out.sum() == 1 and (K <= 4096) == lds, (name, K)
            names.append((name, int(k[out][0]) - K))
            if name == "wrong_sub":                                     # in range under the right sub, every edge
                right = gr.small_keys(a, b, mul, sub + 5)
                assert b is not None and right.min() >= 0 and right.max() < K
        assert [n for n, _ in names] == ["minus_one", "at_K", "wrong_sub"]
        assert names[0][1] == -1 - K0 and names[1][1] == 0 and names[2][1] == 3


def test_sized_groups():
    kk, jj = gr.sized_groups(gr.NB_GROUP_SIZES)
    assert sorted(gr.group_sizes(kk)) == sorted(gr.NB_GROUP_SIZES)          # "a group of exactly 1024 and one of 1025"
    assert {1023, 1024, 1025, 63, 64, 65, 3000} <= set(gr.NB_GROUP_SIZES)
    assert len(set(jj)) == 7 and (np.diff(kk) != 0).any()
    big = kk == np.unique(kk)[gr.NB_GROUP_SIZES.index(3000)]
    assert gr.group_sizes(jj[big]).min() > 300                              # ties inside the long group


def test_tracker_graphs():
    from scenes import ba_scene
    s = ba_scene(seed=5, n_frames=9, M=14, lifetime=4, n_total_frames=16)
    ii, jj, kk = gr.tracker_graph(s)
    assert len(set(kk)) == 9 * 14 and kk.max() < 9 * 14 and max(ii.max(), jj.max()) < 9 and gr.group_sizes(kk).max() <= 9
    hi, hj, hk = gr.tracker_graph(s, heavy=(60, 1100))
    sizes = gr.group_sizes(hk)
    assert len(hk) == len(kk) + 1100 - int((kk == 60).sum()) and sizes.max() == 1100 == int((hk == 60).sum())
    assert np.sort(sizes)[-2] <= 9 and (hi[hk == 60] == 60 // 14).all() and hj.max() < 9 and hj.min() >= 0


def test_softmax_cases():
    for half in (False, True):
        big = 65504.0 if half else 80.0
        for C in gr.SOFTMAX_C:
            for kind in gr.SOFTMAX_KINDS:
                fx, gx, keys = gr.softmax_case(C, kind, half)
                assert fx.shape == gx.shape == (len(keys), C) and fx.dtype == gx.dtype == np.float32
                assert sorted(gr.group_sizes(keys)) == sorted(gr.SOFTMAX_GROUP_SIZES)
                if half:
                    assert np.array_equal(fx, fx.astype(np.float16).astype(np.float32))
                    assert np.array_equal(gx, gx.astype(np.float16).astype(np.float32))
                g = gr.group_by(keys)
                y, _ = gr.segment_softmax_sum(fx, gx, g["gid"], g["G"])
                colmax = np.stack([gx[keys == k].max(0) for k in np.unique(keys)])
                if kind == "equal":
                    assert all((gx[keys == k] == gx[keys == k][0, 0]).all() for k in np.unique(keys))
                if kind == "peak":
                    assert set(np.unique(gx)) == {-big, big} and (colmax == big).all()
                if kind == "some_inf":
                    assert np.isneginf(gx).any() and np.isfinite(colmax).all()
                if kind == "all_inf":
                    dead = np.zeros_like(colmax, bool)
                    dead[2, 0::2] = True                                 # the group of 17, even channels
                    assert gr.group_sizes(keys)[2] == 17 and np.array_equal(np.isneginf(colmax), dead)
                    assert np.array_equal(np.isnan(y), dead)
                else:
                    assert np.isfinite(y).all()


def test_softmax_tolerance_is_the_stated_bound():
    b = np.array([[2.0, 0.5]])
    assert np.array_equal(gr.softmax_tolerance(1000, b), 1016 * 2.0 ** -23 * b)
    ref = np.array([[-3.0, 1.0]])
    assert np.array_equal(gr.softmax_tolerance(1, b, ref, half=True), 17 * 2.0 ** -23 * b + 2.0 ** -11 * np.abs(ref))
