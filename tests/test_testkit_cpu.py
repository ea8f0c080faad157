"""The shared test kit on the CPU: the one guard check (tests/guarded.py ``Flat``) catches a single element written on either
side of the inside, next to it and at the ends of the allocation, for every dtype and layout the suite uses; the one
bit-for-bit comparison (tests/trackerkit.py ``same``) names the first leaf that differs and compares floats as words."""
import numpy as np
import pytest
import torch

from guarded import GUARD, Flat
from trackerkit import same

DTYPES = (torch.uint8, torch.int8, torch.int32, torch.int64, torch.float32, torch.float64)
LAYOUTS = {"flat": dict(shape=37), "shift": dict(shape=37, shift=2), "shaped": dict(shape=(5, 7), rows=7),
           "shaped+shift": dict(shape=(5, 7), rows=7, shift=2)}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: str(d).split(".")[1])
def test_a_write_on_either_side_is_caught(dtype, layout):
    kw = dict(LAYOUTS[layout])
    shape, rows, shift = kw.pop("shape"), kw.get("rows", 1), kw.get("shift", 0)
    n = int(np.prod(shape))

    def fresh():
        return Flat(shape, dtype, device="cpu", **kw)

    g = fresh()
    assert g.t.shape == (shape if isinstance(shape, tuple) else (shape,)) and g.t.dtype == dtype
    assert g.buf.numel() == n + 2 * GUARD * rows + shift and g.address() == g.t.data_ptr()
    assert (g.address() - g.buf.data_ptr()) == (GUARD * rows + shift) * g.buf.element_size()
    assert g.intact() and bool((g.t == g.canary).all())
    before = g.snapshot()
    assert g.unchanged(before)
    g.t.fill_(3)                                                   # every inner element, through the shaped view
    assert g.intact() and not g.unchanged(before) and bool((g.buf[g.lo:g.lo + n] == 3).all())
    for at in (g.lo - 1, g.lo + n, 0, g.buf.numel() - 1):          # inner index -1, inner index n, the allocation's ends
        g = fresh()
        g.buf[at] = 3
        assert not g.intact(), at
    g = Flat(shape, dtype, canary=5, fill=9, device="cpu", **kw)   # a dirty inside that is not the canary
    assert g.intact() and bool((g.t == 9).all()) and g.buf[0] == 5 and g.buf[-1] == 5


def test_same_names_the_first_leaf_that_differs():
    a = dict(x=np.arange(3, dtype=np.float32), y=dict(u=np.arange(4), v=1.5, w="s"))
    b = dict(x=a["x"].copy(), y=dict(u=a["y"]["u"].copy(), v=1.5, w="s"))
    same(a, b, "root")
    b["y"]["u"][2] = 9
    b["y"]["v"] = 2.5                                              # (behind u in the walk: not reported)
    with pytest.raises(AssertionError, match=r"^root\.y\.u$"):
        same(a, b, "root")
    with pytest.raises(AssertionError, match=r"^root\.y$"):
        same(a, dict(x=a["x"], y=dict(u=a["y"]["u"])), "root")     # other keys
    with pytest.raises(AssertionError, match=r"^root\.x$"):
        same(a, dict(b, x=a["x"].astype(np.float64)), "root")      # another dtype
    with pytest.raises(AssertionError, match=r"^root$"):
        same(1, 1.0, "root")                                       # another type


def test_same_compares_floats_as_words():
    for dtype, word, quiet, other in ((np.float32, np.uint32, 0x7FC00000, 0x7FC00001),
                                      (np.float64, np.uint64, 0x7FF8000000000000, 0x7FF8000000000001)):
        nan_a, nan_b = (np.array([p], word).view(dtype) for p in (quiet, other))
        assert np.isnan(nan_a).all() and np.isnan(nan_b).all()
        same(dict(x=nan_a), dict(x=nan_a.copy()), "nan")
        with pytest.raises(AssertionError, match=r"^nan\.x$"):
            same(dict(x=nan_a), dict(x=nan_b), "nan")
        with pytest.raises(AssertionError, match=r"^zero\.x$"):
            same(dict(x=np.array([0.0], dtype)), dict(x=np.array([-0.0], dtype)), "zero")
    same(float("nan"), float("nan"), "number")
    with pytest.raises(AssertionError, match=r"^number$"):
        same(0.0, -0.0, "number")
    with pytest.raises(AssertionError, match=r"^number$"):
        same(float(nan_a[0]), float(nan_b[0]), "number")
