"""CPU test of rampvo_amd.queries._check_status, the closing check of every query's numpy form: which word of which status
tensor it reads, for any length of any of them, and which message wins.  (CPU tensors: the check needs no GPU or library.)"""
import itertools

import pytest
import torch

from rampvo_amd import _lib, ops, track_dev
from rampvo_amd.queries import _check_status

MESSAGES = {"traj": "a frame is neither a keyframe nor reachable through the delta chain",
            "interp": "the frames' time stamps decrease or are not finite",
            "cam": "the camera pose at t_ref is not finite"}
PRECEDENCE = ("traj", "interp", "cam")
BIT = {"traj": track_dev.TRAJ_UNRESOLVED, "interp": 1, "cam": 1}
LENGTHS = (1, 4, 8)


def _status(key, length, bad):
    """a status tensor whose word 0 carries the condition's bit or not -- with every bit and every word the check must not
    read set: the other bits of word 0 and all of the later words"""
    w = torch.full((length,), -1, dtype=torch.int32)
    w[0] = (BIT[key] if bad else 0) | (~BIT[key] & 0x7FFFFFFF)
    return w


@pytest.mark.parametrize("lengths", list(itertools.product(LENGTHS, repeat=3)))
def test_every_combination_of_conditions_for_every_length_in_every_position(lengths):
    for present in itertools.product((False, True), repeat=3):
        for bad in itertools.product((False, True), repeat=3):
            if any(b and not p for b, p in zip(bad, present)):
                continue                                          # (an absent tensor cannot carry a condition)
            kw = {k: (_status(k, n, b) if p else None) for k, n, b, p in zip(PRECEDENCE, lengths, bad, present)}
            first = next((k for k, b in zip(PRECEDENCE, bad) if b), None)
            if first is None:
                assert _check_status("q()", **kw) is None         # clean words (and absent ones) raise nothing
                continue
            with pytest.raises(RuntimeError) as e:
                _check_status("q()", **kw)
            assert str(e.value) == "q(): " + MESSAGES[first], (present, bad, str(e.value))


def test_later_words_are_not_read():
    """counts in the words behind word 0 (odd ones included) are no condition"""
    assert _check_status("q()", traj=torch.zeros(1, dtype=torch.int32), interp=torch.tensor([0, 3, 5, 7], dtype=torch.int32),
                         cam=torch.tensor([0, 1, 1, 1, 1, 1, 1, 1], dtype=torch.int32)) is None
    assert _check_status("q()") is None


# ------------------------------------------------------------------------------------------------ the status table
# The cases below are generated from the table (ops._STATUS, ops.STATUS_ROLES) and the raise order (ops.STATUS_ORDER).  The
# texts are written out once, as the ladder the table replaced raised them (``depth_points``: as event_map_insert() did by
# hand), so a changed string fails; the text of ``scale_failed`` is the one of a word with every refining bit set.
SCALE = "the scale and gravity solve failed: "
TEXTS = {("filter", "bad_order"): "a pixel's events decrease in time, or lie before the filter's state",
         ("rectify", "bad_camera"): "the camera record is not finite or a focal length is not positive",
         ("traj", "unresolved"): "a frame is neither a keyframe nor reachable through the delta chain",
         ("interp", "bad_times"): "the frames' time stamps decrease or are not finite",
         ("cam", "bad_cam"): "the camera pose at t_ref is not finite",
         ("voxel", "bad_offsets"): "the slice offsets decrease or leave the event list",
         ("voxel", "bad_times"): "the first or last time stamp of a slice is not finite",
         ("imu", "bad_order"): "the IMU samples' or the frames' time stamps decrease or are not finite",
         ("imu", "gyro_failed"): "the gyro bias step failed (no interval between two frames is covered by the samples, or its system is not finite)",
         ("imu", "scale_failed"): SCALE + "fewer than two triples of frames are covered by the samples",
         ("propagate", "bad_order"): "the IMU samples' time stamps decrease or are not finite",
         ("propagate", "bad_anchor"): "the anchor is not finite or its scale is not positive (a failed alignment leaves NaN)",
         ("propagate", "no_start"): "no IMU sample lies at or before the anchor's time stamp",
         ("dsi", "bad_times"): "the frames' time stamps decrease or are not finite",
         ("dsi", "bad_range"): "the range of inverse depths is not finite, negative or empty (no depth median yet?)",
         ("depth_points", "bad_camera"): "the camera pose at t_ref is not finite"}
ORDER = tuple(ops.STATUS_ORDER)
PAIRS = [(ORDER[i], ORDER[j]) for i in range(len(ORDER)) for j in range(i + 1, len(ORDER))]


def _mask(role, bit):
    return ops._STATUS[ops.STATUS_ROLES[role]][0][bit][0]


def _word(role, bits=(), length=8):
    """a status tensor of ``role`` whose word 0 carries, of the bits that raise, exactly ``bits`` -- and every bit that raises
    nothing; every later word is set"""
    raising = sum(_mask(r, b) for r, b in ORDER if r == role)
    w = torch.full((length,), -1, dtype=torch.int32)
    w[0] = (~raising & 0x7FFFFFFF) | sum(_mask(role, b) for b in bits)
    return w


def _raises(text, **roles):
    with pytest.raises(RuntimeError) as e:
        _check_status("q()", **roles)
    assert str(e.value) == "q(): " + text, (sorted(roles), str(e.value))


def test_the_table_imports_without_a_gpu_and_holds_single_bits_of_the_header():
    assert set(ops.STATUS_ROLES) == {"traj", "interp", "cam", "voxel", "rectify", "filter", "imu", "propagate", "dsi", "depth_points"}
    assert ORDER[-1] == ("depth_points", "bad_camera") and len(set(ORDER)) == len(ORDER) and set(TEXTS) == set(ORDER)
    constants = set(_lib.CONSTANTS.values())
    for entry, (bits, counters) in ops._STATUS.items():
        masks = [m for m, _ in bits.values()]
        assert all(m > 0 and m & (m - 1) == 0 and m in constants for m in masks), entry
        assert len(set(masks)) == len(masks) and len(set(counters)) == len(counters) and len(counters) <= 7, entry
        for message in (msg for _, msg in bits.values() if msg is not None and not isinstance(msg, str)):
            head, refined, default = message                      # (a bit whose text the word's other bits refine)
            assert isinstance(head, str) and isinstance(default, str) and {m for m, _ in refined} <= set(masks), entry
    for role, entry in ops.STATUS_ROLES.items():                  # the order names every bit of a role that has a text, and no other
        assert {b for b, (_, msg) in ops._STATUS[entry][0].items() if msg is not None} == {b for r, b in ORDER if r == role}, role
    assert _mask("interp", "bad_times") == _lib.RAMP_INTERP_BAD_TIMES and _mask("cam", "bad_cam") == _lib.RAMP_DEPTHMAP_BAD_CAM
    assert _mask("traj", "unresolved") == track_dev.TRAJ_UNRESOLVED
    assert _mask("depth_points", "bad_camera") == _lib.RAMP_DEPTH_POINTS_BAD_CAMERA


@pytest.mark.parametrize("length", (1, 8))
@pytest.mark.parametrize("role,bit", ORDER, ids=["%s.%s" % rb for rb in ORDER])
def test_each_bit_alone_raises_its_text(role, bit, length):
    _raises(TEXTS[role, bit], **{role: _word(role, (bit,), length)})
    clean = {r: _word(r, (), length) for r in ops.STATUS_ROLES if r != role}     # among every other role, clean
    _raises(TEXTS[role, bit], **clean, **{role: _word(role, (bit,), length)})


@pytest.mark.parametrize("first,second", PAIRS, ids=["%s.%s-%s.%s" % (a + b) for a, b in PAIRS])
def test_of_two_bits_the_earlier_in_the_order_wins(first, second):
    (r1, b1), (r2, b2) = first, second
    words = {r1: _word(r1, (b1, b2))} if r1 == r2 else {r1: _word(r1, (b1,)), r2: _word(r2, (b2,))}
    _raises(TEXTS[first], **words)
    _raises(TEXTS[first], **dict(reversed(list(words.items()))))                 # (the order of the keywords is not the order)


def test_every_role_present_and_clean_returns_none():
    for length in (1, 4, 8):
        assert _check_status("q()", **{r: _word(r, (), length) for r in ops.STATUS_ROLES}) is None
    assert _check_status("q()", **{r: None for r in ops.STATUS_ROLES}) is None


def test_the_three_refinements_of_a_failed_scale_solve():
    F, few, bad, sing = (_lib.RAMP_IMU_SCALE_FAILED, _lib.RAMP_IMU_FEW_TRIPLES, _lib.RAMP_IMU_BAD_SCALE, _lib.RAMP_IMU_SINGULAR)
    word = lambda w: torch.tensor([w, 7, 7, 7, 7, 7, 7, 7], dtype=torch.int32)
    for w, why in ((F | few, "fewer than two triples of frames are covered by the samples"), (F | bad, "the scale is not positive"),
                   (F | sing, "the system is singular"), (F, "the system is singular"),
                   (F | few | bad | sing, "fewer than two triples of frames are covered by the samples"),
                   (F | bad | sing, "the scale is not positive")):
        _raises(SCALE + why, imu=word(w))
    assert _check_status("q()", imu=word(few | bad | sing)) is None              # the refining bits alone raise nothing


def test_an_unknown_role_is_a_type_error():
    with pytest.raises(TypeError):
        _check_status("q()", interp=torch.zeros(4, dtype=torch.int32), warp=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(TypeError):
        _check_status("q()", nothing=None)


def test_five_roles_go_to_the_host_in_one_copy(monkeypatch):
    count, cpu = [0], torch.Tensor.cpu

    def counting(self, *a, **kw):
        count[0] += 1
        return cpu(self, *a, **kw)

    monkeypatch.setattr(torch.Tensor, "cpu", counting)
    five = ("traj", "interp", "rectify", "filter", "dsi")
    assert _check_status("q()", **{r: _word(r) for r in five}) is None
    assert count[0] == 1
    _raises(TEXTS["dsi", "bad_range"], **{**{r: _word(r) for r in five}, "dsi": _word("dsi", ("bad_range",))})
    assert count[0] == 2
