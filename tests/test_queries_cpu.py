"""CPU test of rampvo_amd.queries._check_status, the closing check of every query's numpy form: which word of which status
tensor it reads, for any length of any of them, and which message wins.  (CPU tensors: the check needs no GPU or library.)"""
import itertools

import pytest
import torch

from rampvo_amd import track_dev
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
