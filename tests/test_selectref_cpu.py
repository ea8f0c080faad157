"""The numpy restatement of the patch selection (tests/selectref.py) against the torch CPU pipeline of
rampvo_amd/utils.py::get_coords_from_topk_events and against closed forms, and its checks against deliberate mistakes: what
tests/test_patch_selection_gpu.py compares the kernels with has to be right, and has to have teeth.  Everything is exact."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import selectref as sr

_cache = {}


def _stacks():
    """the integer stacks of the GPU test by name, and a Poisson stack at the workload's size"""
    if not _cache:
        _cache.update({name: sr.stack(name) for name in sr.STACKS})
        rng = np.random.default_rng(114)
        _cache["poisson_5x480x640"] = rng.poisson(0.3, (5, 480, 640)).astype(np.float32) * rng.choice([-1, 1], (5, 480, 640))
    return _cache


def _torch_score(ev):
    return F.avg_pool2d(torch.tensor(ev).abs()[None], 4, 4).transpose(3, 2).mean(dim=1)          # [1, w, h]


def _torch_nms(s, ks):
    if ks == 0:
        return s
    mx = F.max_pool2d(s.unsqueeze(0), ks, stride=1, padding=(ks - 1) // 2).squeeze(0)
    return s * (mx == s).float()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rejected(name, mistake, ks, k):
    """does the fixture tell the mistaken restatement from the right one (in the selected indices or coordinates)?"""
    ev = _stacks()[name]
    idx, xy, _ = sr.select(ev, k, ks)
    bad_idx, bad_xy, _ = sr.select(ev, k, ks, mistake=mistake)
    return not (np.array_equal(idx, bad_idx) and _same_bits(xy, bad_xy))


# ------------------------------------------------------------------------------------------------- the torch CPU pipeline
def test_score_and_nms_equal_the_torch_pipeline_bit_for_bit():
    for name, ev in _stacks().items():
        s = sr.score(ev)
        t = _torch_score(ev)
        assert s.shape == (ev.shape[2] // 4, ev.shape[1] // 4), name
        assert _same_bits(s, t[0].numpy()), name
        for ks in sr.NMS_SIZES:
            assert _same_bits(sr.nms(s, ks), _torch_nms(t, ks)[0].numpy()), (name, ks)


def test_score_does_not_depend_on_the_summation_order_for_integer_events():
    ev = _stacks()["poisson_5x480x640"]
    a = np.abs(ev).reshape(5, 120, 4, 160, 4)
    pooled = a.astype(np.float64).sum((2, 4)) / 16
    assert np.array_equal(sr.score(ev), (pooled.sum(0).astype(np.float32) / np.float32(5)).T)


def test_topk_equals_torch_topk_on_a_tie_free_stack():
    g = torch.Generator().manual_seed(17)
    for shape, k, ks in (((5, 96, 128), 64, 0), ((3, 50, 68), 12, 3), ((2, 132, 100), 5, 11)):
        ev = (torch.randn(*shape, generator=g) * 20).numpy()
        s = sr.score(ev)
        t = _torch_score(ev)
        assert np.abs(s - t[0].numpy()).max() <= 2 ** -22 * s.max()      # (float stack: the bins' sum may round differently)
        kept = sr.nms(t[0].numpy(), ks)
        val, ref = torch.topk(torch.from_numpy(kept).flatten(), k)
        assert float(val.min()) > 0 and len(np.unique(val.numpy())) == k     # tie-free
        assert np.array_equal(sr.topk(kept, k), ref.numpy())


@pytest.mark.parametrize("name,k,ks", [("overflow_lds", 96, 0), ("overflow_lds", 96, 11), ("overflow_stream", 512, 0),
                                       ("cap_6144", 96, 0), ("ties_below_capacity", 64, 0), ("sparse_128", 512, 11),
                                       ("plateau_2x132x100_nms3", 200, 3), ("subnormal_tied", 48, 0)])
def test_topk_on_tied_stacks(name, k, ks):
    """the selected values are torch.topk's, element for element; every selected tie has a lower index than every unselected
    cell of the same value"""
    idx, _, s = sr.select(_stacks()[name], k, ks)
    flat = s.reshape(-1)
    val, _ = torch.topk(torch.from_numpy(flat), k)
    assert np.array_equal(_bits(flat[idx]), _bits(val.numpy()))
    assert len(np.unique(idx)) == k
    chosen = np.zeros(flat.size, bool)
    chosen[idx] = True
    assert len(np.unique(flat[idx])) < k                                    # the fixture has ties among the selected
    for v in np.unique(flat[idx]):
        same = flat == v
        if (same & ~chosen).any():
            assert np.flatnonzero(same & chosen).max() < np.flatnonzero(same & ~chosen).min()
    # equal values come out in index order
    for a, b in zip(idx[:-1], idx[1:]):
        assert flat[a] > flat[b] or (flat[a] == flat[b] and a < b)


# ------------------------------------------------------------------------------------------------------------ closed forms
@pytest.mark.parametrize("ks", [1, 3, 11, 17])
def test_a_hot_cell_in_each_corner_survives_any_radius(ks):
    w, h = 25, 33
    c = np.zeros((w, h), np.int64)
    corners = [(0, 0), (0, h - 1), (w - 1, 0), (w - 1, h - 1)]
    for x, y in corners:
        c[x, y] = 5
    kept = sr.nms(sr.score(sr.by_cells(c, 2, 132, 100)), ks)
    assert all(kept[x, y] == np.float32(5) / 16 / 2 for x, y in corners) and np.count_nonzero(kept) == 4
    assert sr.topk(kept, 4).tolist() == [x * h + y for x, y in corners]
    assert np.array_equal(sr.coords([0, h - 1, (w - 1) * h], h)[:, 1], np.float32([0, h - 1, 0]))


@pytest.mark.parametrize("ks", [0, 1, 3, 11, 17])
def test_a_constant_map_survives_whole(ks):
    s = sr.score(sr.by_cells(np.full((17, 12), 3), 3, 50, 68))
    assert (s == s[0, 0]).all() and s[0, 0] > 0
    assert np.array_equal(sr.nms(s, ks), s)
    assert sr.topk(sr.nms(s, ks), 50).tolist() == list(range(50))


def test_coords_carry_the_fraction():
    xy = sr.coords([0, 7, 33, 40], 33)
    assert np.array_equal(xy[:, 1], np.float32([0, 7, 0, 7]))
    assert xy[0, 0] == 0 and xy[2, 0] == np.float32(33) * (np.float32(1) / np.float32(33))
    assert abs(xy[3, 0] - (1 + 7 / 33)) < 1e-6 and xy[1, 0] > 0


def test_by_cells_gives_the_stated_score():
    rng = np.random.default_rng(5)
    c = rng.integers(0, 9, (17, 12))
    for bins in (1, 3):
        s = sr.score(sr.by_cells(c, bins, 50, 68))
        assert np.array_equal(s, c.astype(np.float32) / np.float32(16) / np.float32(bins))
    s = sr.score(sr.by_cells(c[:16, :], 1, 50, 64, scale=2.0 ** -140))
    assert np.array_equal(s.astype(np.float64), c[:16] * 2.0 ** -144) and s[s > 0].max() < 2.0 ** -126


def test_the_fixtures_are_what_their_cases_need():
    st = _stacks()
    def above_tied(name, k):
        flat = sr.score(st[name]).reshape(-1)
        T = np.sort(flat)[::-1][k - 1]
        return int((flat > T).sum()), int((flat == T).sum()), int(np.count_nonzero(flat)), flat, T
    a, t, nnz, flat, T = above_tied("overflow_lds", 96)
    assert (a, t, nnz) == (40, 1300, 1340) and a + t > sr.SEL_SLOTS and nnz <= sr.TOPK_CAP
    assert np.flatnonzero(flat > T).min() == 1560                         # the larger cells at the highest indices
    tied = np.flatnonzero(flat == T)
    assert tied.min() < 20 and tied.max() > 1540 and np.diff(tied).max() < 12       # ties spread over the whole range
    for k in (96, 512):
        a, t, nnz, flat, T = above_tied("overflow_stream", k)
        assert (a, t, nnz) == (40, 6440, 6480) and nnz > sr.TOPK_CAP and np.flatnonzero(flat > T).min() == 6440
    for name, n in (("cap_6144", 6144), ("cap_6145", 6145)):
        a, t, nnz, _, _ = above_tied(name, 96)
        assert (a, t, nnz) == (50, 800, n) and a + t < 900
    assert above_tied("ties_below_capacity", 64)[:2] == (30, 200)
    for name, ks in (("sparse_128", 11), ("sparse_132", 11)):
        kept = sr.nms(sr.score(st[name]), ks)
        assert 0 < np.count_nonzero(kept) < 512 <= kept.size
        # the zero fill takes zeros from several threads' chunks (chunk = ceil(N / 1024) cells per thread)
        chunk = -(-kept.size // 1024)
        fill = sr.topk(kept, 512)[np.count_nonzero(kept):]
        assert len(np.unique(fill // chunk)) > 100
    a, t, nnz, flat, T = above_tied("subnormal_tied", 48)
    assert (a, t) == (20, 100) and 0 < T < 2.0 ** -125
    assert above_tied("subnormal_few", 48)[2] == 30 and sr.score(st["subnormal_few"]).max() < 2.0 ** -125
    for shape in sr.NMS_SHAPES:
        assert np.abs(st["plateau_%dx%dx%d_nms3" % shape][:, 4 * (shape[1] // 4):]).sum() == (shape[1] % 4) * shape[2] * 7 * shape[0]


# ------------------------------------------------------------------------------------------------------ deliberate mistakes
MISTAKE_FIXTURES = {
    "ge": [("plateau_2x132x100_nms3", 3, 200), ("plateau_3x50x68_nms11", 11, 48)],
    "radius": [("plateau_2x132x100_nms3", 3, 200), ("plateau_2x132x100_nms11", 11, 48), ("plateau_2x132x100_nms17", 17, 48)],
    "wrap": [("plateau_2x132x100_nms3", 3, 200), ("plateau_3x50x68_nms11", 11, 48)],
    "highest": [("overflow_lds", 0, 96), ("overflow_stream", 0, 512), ("ties_below_capacity", 0, 64), ("subnormal_tied", 0, 48)],
    "hw": [("overflow_lds", 0, 96), ("plateau_2x132x100_nms11", 11, 48), ("plateau_3x50x68_nms3", 3, 48)],
    "floordiv": [("overflow_lds", 0, 96), ("plateau_3x50x68_nms0", 0, 48)],
    "rows": [("plateau_3x50x68_nms0", 0, 48), ("plateau_3x50x68_nms11", 11, 48)],
}


def test_every_mistake_is_listed():
    assert set(MISTAKE_FIXTURES) == set(sr.SCORE_MISTAKES + sr.NMS_MISTAKES + sr.TOPK_MISTAKES + sr.COORD_MISTAKES)


@pytest.mark.parametrize("mistake", sorted(MISTAKE_FIXTURES))
def test_each_mistake_is_rejected(mistake):
    for name, ks, k in MISTAKE_FIXTURES[mistake]:
        assert _rejected(name, mistake, ks, k), (mistake, name)


def test_each_mistake_breaks_the_torch_comparison_too():
    """the mistakes of score and nms are told apart by the bit-for-bit comparison with torch, not only by the selection"""
    st = _stacks()
    ev = st["plateau_3x50x68_nms3"]
    t = _torch_score(ev)
    for m in sr.SCORE_MISTAKES:
        assert not _same_bits(sr.score(ev, mistake=m), t[0].numpy()), m
    for m in sr.NMS_MISTAKES:
        assert not _same_bits(sr.nms(sr.score(ev), 3, mistake=m), _torch_nms(t, 3)[0].numpy()), m
