"""Patch selection on the GPU: ``ramp_event_topk`` (csrc/select.hip: score, NMS, one-workgroup radix select) through
``ops.event_topk`` and ``utils.get_coords_from_topk_events``, on integer-valued event stacks -- many exact ties and zeros,
what real event stacks produce -- against the numpy restatement tests/selectref.py (itself held to the torch CPU pipeline and
to deliberate mistakes in tests/test_selectref_cpu.py).

Every comparison is exact, there is no tolerance in this file: indices with array_equal, coordinates bit for bit against
``selectref.coords`` and against ``idx / h``, ``idx % h`` evaluated by torch on the device.  Every call writes into rows
1 .. k of a [k + 2, 2] buffer whose first and last rows are canaries, and runs twice: same bits."""
import numpy as np
import pytest
import torch

import selectref as sr
from rampvo_amd._lib import RAMP_EUNSUPPORTED, RAMP_EWORKSPACE

pytestmark = pytest.mark.gpu

CANARY = -777.25
_ref = {}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _reference(name, k, ks):
    key = (name, k, ks)
    if key not in _ref:
        _ref[key] = sr.select(sr.stack(name), k, ks)[:2]
    return _ref[key]


def _call(fn, ev, k, h):
    """``fn(ev_dev, out)`` -> coords written into ``out`` [k,2] (and the indices, or None), twice, each into the middle of a
    canaried buffer -> (indices or None, coords) as numpy after the checks every test shares"""
    dev = torch.tensor(ev, dtype=torch.float32).cuda()
    runs = []
    for _ in range(2):
        buf = torch.full((k + 2, 2), CANARY, dtype=torch.float32, device="cuda")
        idx = fn(dev, buf[1:k + 1])
        torch.cuda.synchronize()
        assert torch.equal(buf[0], torch.full_like(buf[0], CANARY)) and torch.equal(buf[-1], torch.full_like(buf[-1], CANARY))
        if idx is not None:
            assert idx.dtype == torch.int64
            assert torch.equal(buf[1:k + 1, 0], (idx / h).float()) and torch.equal(buf[1:k + 1, 1], (idx % h).float())
        runs.append((None if idx is None else idx.cpu().numpy(), buf[1:k + 1].cpu().numpy()))
    assert np.array_equal(_bits(runs[0][1]), _bits(runs[1][1])), "two calls, two results"
    assert runs[0][0] is None or np.array_equal(runs[0][0], runs[1][0]), "two calls, two results"
    return runs[0]


def _topk(ev, k, ks):
    from rampvo_amd import ops
    return _call(lambda dev, out: ops.event_topk(dev, k, ks, want_indices=True, out=out)[1], ev, k, ev.shape[1] // 4)


def _describe(idx, ref, s):
    """what differs, for the assertion message"""
    flat = s.reshape(-1)
    bad = np.flatnonzero(idx != ref)
    lost, extra = np.setdiff1d(ref, idx), np.setdiff1d(idx, ref)
    return ("%d of %d positions differ (first at %d: got cell %d, expected %d); %d expected cells missing (values %s), "
            "%d unexpected cells (values %s)" % (len(bad), len(ref), bad[0], idx[bad[0]], ref[bad[0]], len(lost),
                                                 np.unique(flat[lost])[::-1][:6], len(extra), np.unique(flat[extra])[::-1][:6]))


def _check(name, k, ks):
    ev = sr.stack(name)
    ref_idx, ref_xy = _reference(name, k, ks)
    idx, xy = _topk(ev, k, ks)
    assert np.array_equal(idx, ref_idx), "%s k=%d nms=%d: %s" % (name, k, ks, _describe(idx, ref_idx, sr.select(ev, k, ks)[2]))
    assert np.array_equal(_bits(xy), _bits(ref_xy))


# ------------------------------------------------------------------------------------------------------------------- ties
def test_ties_overflow_the_gather_lds_path():
    """1 x 160 x 160, k = 96: 40 cells above the threshold at the highest flat indices, 1300 cells tied with it spread over all
    the others -- 1340 cells >= the threshold.  Expected: the 40, then the 56 tied cells of lowest index"""
    idx, _ = _reference("overflow_lds", 96, 0)
    assert idx[:40].min() >= 1560 and np.array_equal(idx[40:], np.sort(idx[40:])) and idx[40:].max() < 100
    _check("overflow_lds", 96, 0)


@pytest.mark.parametrize("k", [96, 512])
def test_ties_overflow_the_gather_streaming_path(k):
    """1 x 320 x 324: all 6480 cells non-zero (more than the LDS candidate list holds), 40 above the threshold at the highest
    indices, every other cell tied"""
    idx, _ = _reference("overflow_stream", k, 0)
    assert idx[:40].min() >= 6440 and idx[40:].tolist() == list(range(k - 40))
    _check("overflow_stream", k, 0)


@pytest.mark.parametrize("nnz", [sr.TOPK_CAP, sr.TOPK_CAP + 1])
def test_candidate_list_boundary(nnz):
    """exactly as many non-zero cells as the LDS list holds, and one more (the streaming passes); 50 + 800 cells >= the
    threshold, so nothing overflows: the switch alone"""
    _check("cap_%d" % nnz, 96, 0)


def test_ties_below_the_gather_capacity():
    """5 x 96 x 128, k = 64: 30 above the threshold, 200 tied with it -- the tie order alone"""
    _check("ties_below_capacity", 64, 0)


# -------------------------------------------------------------------------------------------------------------------- NMS
@pytest.mark.parametrize("ks", sr.NMS_SIZES)
@pytest.mark.parametrize("shape", sr.NMS_SHAPES)
def test_nms_plateaus_and_borders(shape, ks):
    """h = 33, w = 25 and h = 12, w = 17 (H % 4 == 2: two rows of events that no cell owns): no multiple of the 16 x 16 NMS
    tile.  Plateaus (one across a tile boundary), a maximum in each corner, equal maxima r and r + 1 cells apart"""
    name = "plateau_%dx%dx%d_nms%d" % (shape + (ks,))
    N = (shape[1] // 4) * (shape[2] // 4)
    for k in (48, min(N, 300)):
        _check(name, k, ks)


# ---------------------------------------------------------------------------------------------------------- k at its limits
@pytest.mark.parametrize("name", ["sparse_128", "sparse_132"])
def test_k_512_with_a_zero_fill_from_many_chunks(name):
    """fewer than 512 positive cells after NMS 11: the rest are the zero cells of lowest index, counted by all 1024 threads
    (N = 1024: one cell per thread; N = 825: not even that)"""
    _check(name, 512, 11)


@pytest.mark.parametrize("ks", [0, 3])
def test_k_equals_the_cell_count(ks):
    _check("sparse_16", 16, ks)


@pytest.mark.parametrize("name,ks", [("sparse_16", 0), ("overflow_lds", 0), ("plateau_3x50x68_nms11", 11)])
def test_k_1(name, ks):
    _check(name, 1, ks)


# ------------------------------------------------------------------------------------------------------- tiny thresholds
@pytest.mark.parametrize("name", ["subnormal_tied", "subnormal_few"])
def test_threshold_below_2_to_minus_125(name):
    """scores count x 2^-144: the top key byte of every cell is 0, so the zero cells share radix bin 0 with the candidates in
    every pass.  Ties at the threshold; fewer than k positive cells"""
    s = sr.score(sr.stack(name))
    assert 0 < s.max() < 2.0 ** -125 and np.count_nonzero(s) >= 30
    _check(name, 48, 0)


@pytest.mark.parametrize("ks", [0, 11])
def test_all_zero(ks):
    idx, xy = _topk(np.zeros((1, 160, 160), np.float32), 96, ks)
    assert idx.tolist() == list(range(96))
    assert np.array_equal(_bits(xy), _bits(sr.coords(np.arange(96), 40)))


# ----------------------------------------------------------------------------------------------------- the product path
def test_get_coords_from_topk_events():
    """rampvo_amd.utils.get_coords_from_topk_events on [1, 1, bins, H, W], the first overflow map, non_max_supp_rad = 11:
    selectref's coordinates, with and without out="""
    from rampvo_amd.utils import get_coords_from_topk_events
    ev = sr.stack("overflow_lds")
    k = 96
    ref_idx, ref_xy = _reference("overflow_lds", k, 11)
    kept = sr.select(ev, k, 11)[2].reshape(-1)
    T = kept[ref_idx[-1]]
    assert (kept >= T).sum() > sr.SEL_SLOTS and (kept > T).sum() < k              # still an overflow after the NMS

    def with_out(dev, out):
        r = get_coords_from_topk_events(dev[None, None], k, non_max_supp_rad=11, out=out)
        assert r.shape == (1, k, 2) and r.data_ptr() == out.data_ptr()

    def without_out(dev, out):
        r = get_coords_from_topk_events(dev[None, None], k, non_max_supp_rad=11)
        assert r.shape == (1, k, 2) and r.dtype == torch.float32 and r.is_cuda
        out.copy_(r[0])

    for fn in (with_out, without_out):
        _, xy = _call(fn, ev, k, 40)
        assert np.array_equal(_bits(xy), _bits(ref_xy)), fn.__name__


# --------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("shape,k,ks,short,code", [
    ((1, 64, 62), 16, 0, 0, RAMP_EUNSUPPORTED),            # W % 4 != 0
    ((1, 160, 160), 513, 0, 0, RAMP_EUNSUPPORTED),         # k > 512
    ((1, 16, 16), 17, 0, 0, RAMP_EUNSUPPORTED),            # k > N
    ((1, 64, 64), 16, 4, 0, RAMP_EUNSUPPORTED),            # an even NMS size
    ((1, 64, 64), 16, 19, 0, RAMP_EUNSUPPORTED),           # an NMS window beyond the staged halo
    ((1, 64, 64), 16, 11, 1, RAMP_EWORKSPACE),             # a workspace one byte short
])
def test_refusals_write_nothing(shape, k, ks, short, code):
    from rampvo_amd._lib import lib, ptr, stream
    bins, H, W = shape
    ev = torch.ones(shape, dtype=torch.float32, device="cuda")
    buf = torch.full((k + 2, 2), CANARY, dtype=torch.float32, device="cuda")
    idx = torch.full((k,), -1, dtype=torch.int64, device="cuda")
    nbytes = lib().ramp_event_topk_workspace_bytes(H, W)
    assert nbytes == 2 * (H // 4) * (W // 4) * 4
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib().ramp_event_topk(ptr(ev), bins, H, W, k, ks, ptr(buf[1:]), ptr(idx), ptr(ws), nbytes - short, stream())
    torch.cuda.synchronize()
    assert rc == code
    assert bool((buf == CANARY).all()) and bool((idx == -1).all()) and not bool(ws.any())
