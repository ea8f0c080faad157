"""The numpy restatement of the event voxel grid (tests/voxelref.py) against the REFERENCE'S OWN CLASS, recorded in
tests/golden/event_voxel.npz by tools/make_voxel_golden.py, against closed forms, and against deliberate mistakes: what
tests/test_event_voxel_gpu.py compares the kernel with has to be right, and has to have teeth.

The tolerance is the project's envelope rule, per cell (voxelref.compare): four times the reference's own recorded error
against float64, or what the fixed point may add -- 2^-25 per contribution -- plus one fp32 ulp, whichever is larger."""
import ctypes
import os
import re

import numpy as np
import pytest

import voxelref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = voxelref.load_case(name)
    return _cases[name]


def run(c, normalize, mistake=None, subpixel=False):
    e = c["events"]
    bins, H, W = (int(v) for v in c["shape"])
    return voxelref.voxel_grid(e[:, 1], e[:, 2], e[:, 0], e[:, 3], H, W, bins, normalize=normalize, subpixel=subpixel,
                               mistake=mistake)


# ------------------------------------------------------------------------------------------------ 1. the reference fixture
def test_the_fixture_holds_the_cases_the_tests_need():
    with np.load(voxelref.GOLDEN) as z:
        names = sorted({k.split("/")[0] for k in z.files if "/" in k})
    assert names == sorted(voxelref.CASES)
    assert os.path.getsize(voxelref.GOLDEN) < 512 * 1024
    c = case("random")
    assert len(c["events"]) == 4099 and c["shape"].tolist() == [5, 13, 17]
    t = c["events"][:, 0]
    assert t.min() < t[0] < t[-1] < t.max()                   # unsorted: first / last by position are not min / max
    assert case("three")["shape"].tolist() == [2, 4, 5] and len(case("three")["events"]) == 3
    assert case("onebin")["shape"][0] == 1
    assert np.ptp(case("equal_times")["events"][:, 0]) == 0
    e = case("cancel")["events"]
    assert e[1, 0] == e[2, 0] and (np.trunc(e[1, 1:3]) == np.trunc(e[2, 1:3])).all() and e[1, 3] == 1 and e[2, 3] == 0
    assert case("cancel")["ref_raw"][:, 1, 2].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("name", voxelref.CASES)
def test_masks_agree(name):
    """the condition on the fixture: the reference's non-zero cells, the float64 restatement's and the emulator's are one
    set; no non-empty cell of the random case within 1e-4 of zero"""
    c = case(name)
    assert voxelref.masks_agree(c)
    if name == "random":
        raw = c["ref_raw"]
        assert np.abs(raw[raw != 0]).min() >= 1e-4


@pytest.mark.parametrize("name", voxelref.CASES)
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_against_the_reference(name, normalize):
    c = case(name)
    r = run(c, normalize)
    q = voxelref.compare(r["grid"][0], c, normalize)
    print("%s normalize=%d: err %.3e, largest bound %.3e, worst err / bound %.3f" % (name, normalize, q["err"], q["bound"], q["worst"]))
    assert q["ok"], q
    n, mean, std, _ = r["stats"][0]
    assert n == (c["ref_raw"] != 0).sum()
    E = c["count"].max() * 2.0 ** -25                          # (the largest fixed-point error of a cell)
    assert abs(mean - float(c["mean"])) <= E and abs(std - float(c["std"])) <= 3 * E
    assert r["status"].tolist() == [0, len(c["events"]), 0, 0, r["status"][4], r["status"][5], 0, 0]
    assert r["status"][4] + r["status"][5] == len(c["events"])
    # the sub-pixel mode on the truncated coordinates: the same bits
    e = c["events"].copy()
    e[:, 1:3] = np.trunc(e[:, 1:3])
    s = run(dict(c, events=e), normalize, subpixel=True)
    assert np.array_equal(s["acc"], r["acc"]) and np.array_equal(s["status"], r["status"])
    assert np.array_equal(s["grid"], r["grid"])


@pytest.mark.parametrize("mistake", voxelref.MISTAKES)
def test_mistakes_are_rejected(mistake):
    """each deliberate mistake fails the comparison with the reference on the random case (raw or normalised)"""
    c = case("random")
    bad = [voxelref.compare(run(c, normalize, mistake=mistake)["grid"][0], c, normalize) for normalize in (False, True)]
    print(mistake, "worst err / bound: raw %.3g, normalised %.3g" % (bad[0]["worst"], bad[1]["worst"]))
    assert not (bad[0]["ok"] and bad[1]["ok"])
    if mistake in ("biased", "allcells"):                      # (mistakes of the normalisation alone)
        assert bad[0]["ok"] and not bad[1]["ok"]


# ------------------------------------------------------------------------------------------------ 2. closed forms
def _one(x, y, t, p, H=4, W=5, bins=5, **kw):
    return voxelref.voxel_grid(np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(t, np.float64), np.asarray(p), H, W,
                               bins, **kw)


def test_one_event_between_two_bins():
    # t = (0, 1.25, 4) with 5 bins: tn = 1.25 puts 0.75 / 0.25 into bins 1 / 2 of its pixel
    r = _one([0, 2, 4], [0, 1, 3], [0.0, 1.25, 4.0], [1, 1, 1], normalize=False)
    g = r["grid"][0]
    assert g[1, 1, 2] == 0.75 and g[2, 1, 2] == 0.25 and r["acc"][0, 1, 1, 2] == 3 << 22
    assert g[0, 0, 0] == 1.0                                  # the first event: all of it in bin 0
    assert g[4, 3, 4] == 1.0 and g.sum() == 3.0               # the last event lands wholly in the last bin
    assert r["stats"][0].tolist()[0] == 4 and r["stats"][0][3] == 3.0 and r["stats"][0][1] == 0.75
    assert r["status"].tolist() == [0, 3, 0, 0, 0, 3, 0, 0]


def test_one_bin_and_equal_times():
    r = _one([1, 1, 3], [2, 2, 0], [0.0, 0.5, 2.0], [1, 0, -1], bins=1, normalize=False)
    assert r["grid"][0, 0, 2, 1] == 0.0 and r["grid"][0, 0, 0, 3] == -1.0 and r["stats"][0][0] == 1
    r = _one([1, 1, 3], [2, 2, 0], [7.0, 7.0, 7.0], [1, 1, -1], bins=3, normalize=False)    # deltaT = 0 -> 1: tn = 0
    assert r["grid"][0, 0, 2, 1] == 2.0 and r["grid"][0, 0, 0, 3] == -1.0 and not r["grid"][0, 1:].any()


def test_normalisation_conventions():
    # n = 1: the unbiased std is NaN, the mean is subtracted and the cell becomes 0
    r = _one([1], [2], [0.0], [1], bins=2)
    assert not r["grid"].any() and r["stats"][0][0] == 1 and r["stats"][0][1] == 1.0 and np.isnan(r["stats"][0][2])
    # std = 0: two cells of the same value
    r = _one([1, 3], [2, 0], [0.0, 0.0], [1, 1], bins=2)
    assert not r["grid"].any() and r["stats"][0].tolist() == [2.0, 1.0, 0.0, 2.0]
    # n = 0: untouched, stats 0
    r = _one([], [], [], [], bins=2)
    assert not r["grid"].any() and not r["stats"].any() and not r["status"].any()
    # +1 and -1 in two cells: mean 0, unbiased std sqrt(2)
    r = _one([1, 3], [2, 0], [0.0, 0.0], [1, -1], bins=2)
    assert r["grid"][0, 0, 2, 1] == np.float32(1 / np.sqrt(2.0)) and r["grid"][0, 0, 0, 3] == -np.float32(1 / np.sqrt(2.0))


def test_status_words_and_failures():
    x = [1, np.nan, 9, 2, 2, 2.5, -0.5]
    y = [1, 1, 1, 1, 1, 1, 3.9]
    t = [0.0, 0.1, 0.2, -1.0, np.inf, 0.5, 1.0]
    r = _one(x, y, t, [1] * 7, normalize=False)
    # the NaN x and the infinite t: word 2; x = 9: word 3; t = -1 (ti < 0): word 4; x = -0.5 truncates to pixel 0: inside
    assert r["status"].tolist() == [0, 7, 2, 1, 1, 3, 0, 0]
    assert r["grid"][0, 4, 3, 0] == 1.0
    # sub-pixel: x = -0.5 has one neighbour inside, of weight 0.5; y = 3.9 loses its lower neighbour
    s = _one(x, y, t, [1] * 7, normalize=False, subpixel=True)
    assert s["status"].tolist() == [0, 7, 2, 1, 1, 3, 0, 0]
    assert abs(s["grid"][0, 4, 3, 0] - 0.5 * np.float32(1 - np.float32(3.9 - 3))) < 1e-7 and s["grid"][0, 4].sum() == s["grid"][0, 4, 3, 0]
    # a first time stamp that is not finite: the slice is NaN, its events are counted without a vote
    r = _one([1, 2], [1, 1], [np.nan, 1.0], [1, 1], normalize=False)
    assert r["status"].tolist() == [voxelref.BAD_TIMES, 2, 1, 0, 1, 0, 0, 0] and np.isnan(r["grid"]).all() and np.isnan(r["stats"]).all()
    # slices: an empty one in the middle; bad offsets
    r = _one([1, 2, 3], [1, 1, 1], [0.0, 1.0, 2.0], [1, 1, 1], offsets=[0, 2, 2, 3], normalize=False)
    assert r["grid"].shape[0] == 3 and not r["grid"][1].any() and r["grid"][2, 0, 1, 3] == 1.0 and r["status"][1] == 3
    for off in ([0, 2, 1, 3], [-1, 3], [0, 4]):
        r = _one([1, 2, 3], [1, 1, 1], [0.0, 1.0, 2.0], [1, 1, 1], offsets=off)
        assert r["status"].tolist() == [voxelref.BAD_OFFSETS, 0, 0, 0, 0, 0, 0, 0] and np.isnan(r["grid"]).all()


# ------------------------------------------------------------------------------------------------ 3. the C entries
def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib, ops
    from rampvo_amd.queries import TrackerQueries
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_event_voxel", "ramp_event_voxel_workspace_bytes", "ramp_event_voxel_grid_events",
                 "ramp_event_voxel_lds_offsets"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    for macro, val in (("RAMP_VOXEL_NORMALIZE", _lib.RAMP_VOXEL_NORMALIZE), ("RAMP_VOXEL_SUBPIXEL", _lib.RAMP_VOXEL_SUBPIXEL),
                       ("RAMP_VOXEL_BAD_OFFSETS", _lib.RAMP_VOXEL_BAD_OFFSETS), ("RAMP_VOXEL_BAD_TIMES", _lib.RAMP_VOXEL_BAD_TIMES)):
        assert re.search(r"#define %s %d\b" % (macro, val), header), macro
    assert (voxelref.BAD_OFFSETS, voxelref.BAD_TIMES) == (_lib.RAMP_VOXEL_BAD_OFFSETS, _lib.RAMP_VOXEL_BAD_TIMES)
    one, three = (lib.ramp_event_voxel_workspace_bytes(s, 5, 13, 17) for s in (1, 3))
    assert one % 8 == 0 and one >= 64 + 5 * 13 * 17 * 8 and three - one == 2 * (one - 64)
    assert lib.ramp_event_voxel_workspace_bytes(1, 0, 13, 17) == 0 and lib.ramp_event_voxel_workspace_bytes(0, 5, 13, 17) == 0
    assert lib.ramp_event_voxel_grid_events() == lib.ramp_event_warp_grid_events() and lib.ramp_event_voxel_lds_offsets() >= 2
    for name in ("event_voxel_grid", "event_voxel_status", "event_slices"):
        assert callable(getattr(ops, name))
    assert callable(TrackerQueries.event_voxel_grid)
    assert "voxel.hip" in open(os.path.join(ROOT, "rampvo_amd", "csrc", "Makefile")).read()


def test_argument_checks_that_need_no_gpu():
    """RAMP_EINVAL / RAMP_EWORKSPACE before anything touches the device (the pointers are never read)"""
    from rampvo_amd import _lib
    lib = _lib.lib()
    buf = (ctypes.c_double * 64)()
    q = ctypes.cast(buf, ctypes.c_void_p)
    off8 = ctypes.c_void_p(q.value + 8)
    assert q.value % 16 == 0 or off8.value % 16 == 0
    if q.value % 16:
        q, off8 = off8, ctypes.c_void_p(q.value + 16)
    odd = ctypes.c_void_p(q.value + 4)

    def call(N=10, S=1, bins=5, H=13, W=17, flags=0, offsets=None, grid=q, stats=q, status=q, ws=q, x=q, ws_bytes=0):
        return lib.ramp_event_voxel(x, q, q, q, N, offsets, S, bins, H, W, flags, grid, stats, status, ws, ws_bytes, None)

    for kw in (dict(N=-1), dict(S=0), dict(bins=0), dict(H=0), dict(W=0), dict(flags=4), dict(S=2), dict(grid=None),
               dict(stats=None), dict(status=None), dict(ws=None), dict(x=None), dict(ws=off8), dict(stats=odd),
               dict(offsets=odd, S=2)):
        assert call(**kw) == -1, kw
    assert call() == -3                                               # a workspace of 0 bytes: RAMP_EWORKSPACE
    assert call(ws_bytes=lib.ramp_event_voxel_workspace_bytes(1, 5, 13, 17) - 8) == -3
    assert call(offsets=q, S=3, ws_bytes=lib.ramp_event_voxel_workspace_bytes(1, 5, 13, 17) - 8) == -3
    assert call(bins=1 << 20, H=1 << 10, W=1 << 10) == -4             # bins * H * W >= 2^31: RAMP_EUNSUPPORTED


def test_event_slices_rejects_a_count_of_zero():
    from rampvo_amd import ops
    with pytest.raises(RuntimeError):
        ops.event_slices(10, 0)


def test_the_status_check_of_the_query_reads_both_bits():
    import torch
    from rampvo_amd import queries
    ok = torch.zeros(8, dtype=torch.int32)
    queries._check_status("q", voxel=ok)
    for word, text in ((1, "slice offsets"), (2, "first or last time stamp"), (3, "slice offsets")):
        with pytest.raises(RuntimeError, match=text):
            queries._check_status("q", voxel=torch.tensor([word, 5, 0, 0, 0, 5, 0, 0], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="time stamps decrease"):       # (the warp's word comes first)
        queries._check_status("q", interp=torch.tensor([1], dtype=torch.int32), voxel=torch.tensor([1], dtype=torch.int32))
