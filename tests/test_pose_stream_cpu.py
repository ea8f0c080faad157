"""Live poses, host side (no GPU): the reader of the pose ring on hand-made buffers, the record layout against the C header,
the new entry points' export."""
import os
import re
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _record(ring, slot, frame, frame2=None, tstamp=None, pose=None, dropped=0, t1=-1, t0=-1, n=10, E=500, status=0):
    """what csrc/publish.hip writes for frame `frame` into ring[slot] (frame2: the tag of the second half, to tear it)"""
    from rampvo_amd import track_dev as td
    r = ring[slot]
    r[:] = 0
    r[td.POSE_FRAME] = frame
    r[td.POSE_FRAME2] = frame if frame2 is None else frame2
    r[td.POSE_N], r[td.POSE_E], r[td.POSE_STATUS], r[td.POSE_DROPPED] = n, E, status, dropped
    r[td.POSE_T1], r[td.POSE_T0], r[td.POSE_KF_TSTAMP] = t1, t0, frame
    r[td.POSE_TSTAMP:td.POSE_TSTAMP + 2] = np.array([0.25 * frame if tstamp is None else tstamp], np.float64).view(np.int32)
    p = np.arange(7, dtype=np.float32) + frame if pose is None else np.asarray(pose, np.float32)
    r[td.POSE_POSE:td.POSE_POSE + 7] = p.view(np.int32)
    r[td.POSE_INV:td.POSE_INV + 7] = (-p).view(np.int32)


def _empty(cap):
    from rampvo_amd import track_dev as td
    return np.full((cap, td.POSE_WORDS), -1, np.int32)


def test_an_empty_ring_has_no_latest_record_and_nothing_since():
    from rampvo_amd import track_dev as td
    ring = _empty(4)
    assert td.pose_latest(ring) is None and td.pose_latest(ring, hint=3) is None and td.pose_latest(ring, hint=-1) is None
    assert td.pose_since(ring, -1) == ([], 0)
    assert td.pose_records(ring) == []


def test_a_record_decodes_to_the_values_written():
    from rampvo_amd import track_dev as td
    ring = _empty(4)
    _record(ring, 2, 6, tstamp=1234.5678901234, pose=[1, 2, 3, 0.1, 0.2, 0.3, 0.9], dropped=1, t1=3, t0=2, n=11, E=777, status=1)
    r = td.pose_latest(ring, hint=6)
    assert (r.frame, r.n, r.factors, r.status, r.dropped, r.delta, r.kf_frame) == (6, 11, 777, 1, True, (3, 2), 6)
    assert r.tstamp == 1234.5678901234                                   # (a double: bit for bit)
    assert np.array_equal(r.pose, np.array([1, 2, 3, 0.1, 0.2, 0.3, 0.9], np.float32))
    assert np.array_equal(r.pose_inv, -r.pose)
    _record(ring, 3, 7)
    assert td.pose_latest(ring, hint=7).delta is None


def test_a_torn_record_is_never_returned_and_the_older_complete_one_is():
    from rampvo_amd import track_dev as td
    ring = _empty(4)
    for f in range(5):                                  # frames 0 .. 4: slot 0 holds frame 4
        _record(ring, f % 4, f)
    _record(ring, 5 % 4, 5, frame2=1)                   # frame 5 half written over frame 1: the second tag is still the old one
    assert td.pose_read_slot(ring, 1) is None
    for hint in (5, None, 9):
        r = td.pose_latest(ring, hint=hint)
        assert r is not None and r.frame == 4, (hint, r)
    recs, lost = td.pose_since(ring, -1)
    assert [r.frame for r in recs] == [2, 3, 4]         # never the torn one, under either of its tags
    assert lost == 2                                    # frames 0 and 1 are gone
    assert all(r.frame != 5 and r.frame != 1 for r in td.pose_records(ring))
    # the other way round (the second half landed, the first did not): torn all the same
    _record(ring, 1, 1, frame2=5)
    assert td.pose_read_slot(ring, 1) is None and td.pose_latest(ring, hint=5).frame == 4


def test_slots_with_out_of_order_tags_come_back_ordered_by_tag():
    from rampvo_amd import track_dev as td
    ring = _empty(8)
    for slot, f in ((0, 16), (1, 9), (2, 18), (3, 11), (5, 13), (6, 22), (7, 15)):      # slot 4 still empty
        _record(ring, slot, f)
    assert [r.frame for r in td.pose_records(ring)] == [9, 11, 13, 15, 16, 18, 22]
    recs, lost = td.pose_since(ring, 12)
    assert [r.frame for r in recs] == [13, 15, 16, 18, 22]
    assert lost == (22 - 13 + 1) - 5
    assert td.pose_latest(ring).frame == 22
    assert td.pose_latest(ring, hint=22).frame == 22
    assert td.pose_since(ring, 22) == ([], 0)
    # tags are consecutive from the first frame published: nothing below it counts as lost
    ring = _empty(4)
    for f in (20, 21, 22):
        _record(ring, f % 4, f)
    assert td.pose_since(ring, -1, first=20)[1] == 0 and td.pose_since(ring, -1, first=0)[1] == 20


def test_pose_record_mirror_matches_the_header(tmp_path):
    """track_dev's POSE_* / TRAJ_UNRESOLVED equal include/ramp_hip.h's RAMP_POSE_* / RAMP_TRAJ_UNRESOLVED, and the record is two
    64-byte halves with a tag in each: printed by a C program built with the system compiler"""
    from rampvo_amd import track_dev as td
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler on PATH"
    names = ["WORDS", "FRAME", "N", "E", "STATUS", "DROPPED", "T1", "T0", "KF_TSTAMP", "TSTAMP", "POSE", "INV", "FRAME2"]
    src, exe = tmp_path / "pose.c", tmp_path / "pose"
    src.write_text('#include "ramp_hip.h"\n#include <stdio.h>\nint main(void) {\n  printf("'
                   + " ".join(["%d"] * (len(names) + 2)) + '\\n", ' + ", ".join("RAMP_POSE_" + n for n in names)
                   + ", RAMP_TRAJ_UNRESOLVED, RAMP_TRACK_LOG);\n  return 0;\n}\n")
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    want = [getattr(td, "POSE_" + n) for n in names] + [td.TRAJ_UNRESOLVED, td.LOG_WORDS]
    assert got == want, (got, want)
    assert td.POSE_WORDS * 4 == 128 and td.POSE_FRAME < 16 <= td.POSE_FRAME2 < 32
    words = set()                                       # no two fields share a word
    for n, width in (("FRAME", 1), ("N", 1), ("E", 1), ("STATUS", 1), ("DROPPED", 1), ("T1", 1), ("T0", 1), ("KF_TSTAMP", 1),
                     ("TSTAMP", 2), ("POSE", 7), ("INV", 7), ("FRAME2", 1)):
        w = set(range(getattr(td, "POSE_" + n), getattr(td, "POSE_" + n) + width))
        assert not (w & words) and max(w) < td.POSE_WORDS, n
        words |= w


def test_the_new_entry_points_are_declared_exported_and_bound():
    from rampvo_amd import _lib
    header = open(os.path.join(ROOT, "include", "ramp_hip.h")).read()
    declared = set(re.findall(r"\b(ramp_[a-z0-9_]+)\s*\(", header))
    lib = _lib.lib()
    for name in ("ramp_track_publish", "ramp_trajectory_resolve"):
        assert name in declared and hasattr(lib, name) and name in _lib.SIGNATURES, name
    # argument checks that need no GPU: no ring, an empty ring, a row outside the pose buffer
    assert lib.ramp_track_publish(None, 0, 0.0, None, 4, None, None, 8, 0, 0, 0, 0, 0, -1, -1, None) == -1
    assert lib.ramp_trajectory_resolve(None, None, 0, None, None, 0, None, 0, -1, None, None, None, None) == -1
    assert lib.ramp_trajectory_resolve(None, None, 0, None, None, 0, None, 0, 0, None, None, None, None) == 0
