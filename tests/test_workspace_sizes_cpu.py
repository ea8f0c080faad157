"""The workspace sizes are ABI: every ``ramp_*_workspace_bytes`` returns what it returned before the layouts moved to the one
carver of csrc/workspace.h.  tests/golden/workspace_bytes.json holds, per query, argument tuples and the values recorded from
the library of the commit before (tools/record_workspace_bytes.py); the library as built has to return them, value for value.

Four families contain hipcub's temporary storage, which may differ between rocPRIM builds and is therefore in no fixture:
ramp_group_by, ramp_neighbors, ramp_event_filter and the unplanned bundle adjustment.  For those the differences in which
that term cancels are held to the layout's own arithmetic.  No GPU: the queries are host code."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")) as _f:
    RECORDED = json.load(_f)

E_EDGES = (-1, 0, 1, 255, 256, 257, 4099)


def up256(n):
    return (n + 255) // 256 * 256


def lib():
    from rampvo_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_size_is_what_the_commit_before_returned(name):
    fn = getattr(lib(), name)
    rows = RECORDED[name]
    assert len(rows) >= 4
    for args, value in rows:
        assert fn(*args) == value, (name, args)


def test_fixture_names_every_query_without_a_hipcub_term():
    from rampvo_amd import _lib
    queries = {n for n in _lib.SIGNATURES if n.endswith("_workspace_bytes")}
    hipcub = {"ramp_group_by_workspace_bytes", "ramp_neighbors_workspace_bytes", "ramp_event_filter_workspace_bytes",
              "ramp_ba_workspace_bytes", "ramp_ba_covariance_workspace_bytes", "ramp_ba_map_covariance_workspace_bytes"}
    by_descriptor = {"ramp_track_uncertainty_workspace_bytes", "ramp_track_map_workspace_bytes"}     # (the GPU tests' to cover)
    assert queries - hipcub - by_descriptor == set(RECORDED)


def test_neighbors_is_group_by_and_two_orders():
    l = lib()
    for E in E_EDGES:
        assert l.ramp_neighbors_workspace_bytes(E) - l.ramp_group_by_workspace_bytes(E) == 2 * up256(4 * max(E, 1)), E
        assert l.ramp_group_by_workspace_bytes(E) % 256 == 0


def test_filter_moves_with_the_image_by_start_and_hot():
    l = lib()
    image = lambda hw: up256(4 * (hw + 2)) + up256(hw)
    for N in (0, 1, 257, 4099):
        base = l.ramp_event_filter_workspace_bytes(N, 1, 1)
        assert base > 0 and base % 256 == 0
        for H, W in ((13, 17), (1, 255), (16, 16), (260, 346)):
            assert l.ramp_event_filter_workspace_bytes(N, H, W) - base == image(H * W) - image(1), (N, H, W)
    for N, H, W in ((-1, 13, 17), (1 << 31, 13, 17), (5, 0, 17), (5, 13, 0)):
        assert l.ramp_event_filter_workspace_bytes(N, H, W) == 0


def test_unplanned_ba_is_planned_and_its_own_grouping():
    l = lib()
    for E in E_EDGES:
        for t1 in (1, 2, 11):
            a = (E, 11, 88, 1, t1)
            e = max(E, 1)
            own = l.ramp_group_by_workspace_bytes(E) + 3 * up256(8 * e) + 2 * up256(4 * e) + 2 * up256(4 * (e + 1))
            planned = l.ramp_ba_planned_workspace_bytes(*a, 0, 0)
            assert l.ramp_ba_workspace_bytes(*a) - planned == own, a
            cov = l.ramp_ba_covariance_planned_workspace_bytes(*a, 0, 0) - planned
            assert l.ramp_ba_covariance_workspace_bytes(*a) - l.ramp_ba_workspace_bytes(*a) == cov, a
            assert l.ramp_ba_map_covariance_workspace_bytes(*a) == l.ramp_ba_covariance_workspace_bytes(*a), a
