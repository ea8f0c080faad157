"""tests/filterref.py -- the numpy restatement the GPU tests of ramp_event_filter compare against, bit for bit -- held to closed
forms of the definition (include/ramp_hip.h, "event denoising"), and shown to tell the definition from ten plausible wrong
rules on the very streams the GPU tests use.  No GPU, seconds in total."""
import numpy as np
import pytest

import filterref as fr

H, W = 13, 17
NAN = float("nan")


def run(ev, **kw):
    """ev: rows (x, y, t)"""
    ev = np.asarray(ev, np.float64).reshape(-1, 3)
    return fr.event_filter(ev[:, 0], ev[:, 1], ev[:, 2], kw.pop("H", H), kw.pop("W", W), **kw)


# ------------------------------------------------------------------------------------------------ closed forms
def test_a_lone_event_is_dropped():
    r = run([(5, 5, 1.0)], support_dt=1.0)
    assert r["cls"].tolist() == [6] and r["keep"].tolist() == [0] and r["status"].tolist() == [0, 1, 0, 0, 0, 0, 1, 0]
    assert np.isnan(r["xy"]).all() and r["index"].tolist() == [-1] and r["count"] == 0
    assert r["last_t"][5, 5] == 1.0 and np.isnan(r["last_t"]).sum() == H * W - 1


def test_of_two_neighbours_the_second_is_kept():
    r = run([(5, 5, 1.0), (6, 6, 1.5)], support_dt=0.5)
    assert r["cls"].tolist() == [6, 7] and r["index"].tolist() == [1, -1] and r["count"] == 1
    assert r["xy"][1].tolist() == [6.0, 6.0] and np.isnan(r["xy"][0]).all()
    assert run([(5, 5, 1.0), (6, 6, 1.5)], support_dt=0.49)["cls"].tolist() == [6, 6]
    assert run([(5, 5, 1.0), (7, 5, 1.5)], support_dt=0.5)["cls"].tolist() == [6, 6]            # two pixels apart


def test_the_own_pixel_gives_no_support():
    assert run([(5.2, 5.9, 1.0), (5.7, 5.1, 1.5)], support_dt=0.5)["cls"].tolist() == [6, 6]


def test_the_corner_pixel_has_three_neighbours():
    for nb, want in (((1, 0), 7), ((0, 1), 7), ((1, 1), 7), ((2, 0), 6), ((W - 1, 0), 6), ((0, H - 1), 6), ((W - 1, H - 1), 6)):
        r = run([(nb[0], nb[1], 1.0), (0, 0, 1.1)], support_dt=0.5)
        assert r["cls"].tolist() == [6, want], nb


def test_equal_time_stamps_are_ordered_by_index():
    assert run([(5, 5, 1.0), (6, 5, 1.0)], support_dt=0.0)["cls"].tolist() == [6, 7]
    assert run([(6, 5, 1.0), (5, 5, 1.0)], support_dt=0.0)["cls"].tolist() == [6, 7]


def test_support_dt_zero_admits_only_equal_time_neighbours():
    r = run([(5, 5, 1.0), (6, 5, 1.0), (7, 5, np.nextafter(1.0, 2.0)), (8, 5, np.nextafter(1.0, 2.0))], support_dt=0.0)
    assert r["cls"].tolist() == [6, 7, 6, 7]


def test_refractory_boundary_is_kept():
    r = run([(5, 5, 1.0), (5, 5, 1.25), (5, 5, 1.25 + 0.2499999)], refractory=0.25)
    assert r["cls"].tolist() == [7, 7, 5]
    # history-free: the predecessor is the previous candidate, kept or not
    assert run([(5, 5, 1.0), (5, 5, 1.2), (5, 5, 1.4)], refractory=0.25)["cls"].tolist() == [7, 5, 5]
    # an event dropped by the refractory test still supports its neighbours
    assert run([(5, 5, 1.0), (5, 5, 1.1), (6, 5, 1.15)], refractory=0.25, support_dt=0.05)["cls"].tolist() == [6, 5, 7]


def test_classes_and_precedence():
    ev = [(NAN, 1, 1.0), (1, np.inf, 1.0), (1, 1, NAN), (-1.0, 1, 1.0), (W, 1, 1.0), (1, H, 1.0), (-0.5, 0.5, 1.0), (3, 3, 1.0),
          (3, 3, 1.0)]
    r = run(ev, refractory=0.5, hot_count=1)
    assert r["cls"].tolist() == [2, 2, 2, 3, 3, 3, 7, 4, 4]                  # (-0.5 truncates to pixel 0; hot before refractory)
    assert r["status"][1] == 9 and r["status"][2:].sum() == 9 and r["hot"].sum() == 1 and r["hot"][3, 3] == 1
    assert np.isnan(r["last_t"][3, 3])                                       # a hot pixel does not touch the state


def test_hot_rule_is_the_formula():
    c = np.zeros((H, W), int)
    c[0, :4] = (1, 1, 1, 5)
    hot, stats = fr.hot_rule(c, hot_sigma=1.5)
    assert stats.tolist() == [4.0, 2.0, np.sqrt(3.0), 2.0 + 1.5 * np.sqrt(3.0)] and hot.sum() == 1 and hot[0, 3]
    assert fr.hot_rule(c, hot_sigma=1.5, mistake="sample_variance")[0].sum() == 0          # thr = 5: 5 > 5 is false
    hot, stats = fr.hot_rule(c, hot_count=0, hot_sigma=0.0, hot_mask=np.eye(H, W))
    assert np.isnan(stats[3]) and hot.sum() == min(H, W)
    hot, stats = fr.hot_rule(np.zeros((H, W), int), hot_sigma=1.0)
    assert stats[0] == 0 and np.isnan(stats[1:]).all() and hot.sum() == 0


def test_hot_pixels_give_no_support():
    ev = [(5, 5, 1.0), (5, 5, 1.1), (5, 5, 1.2), (6, 5, 1.25)]
    assert run(ev, support_dt=0.5, hot_count=2)["cls"].tolist() == [4, 4, 4, 6]
    assert run(ev, support_dt=0.5)["cls"].tolist() == [6, 6, 6, 7]


def test_state_one_call_equals_two():
    x, y, t = fr.stream(600)
    kw = dict(support_dt=2e-3, refractory=4e-4)
    whole = fr.event_filter(x, y, t, H, W, **kw)
    for cut in (1, 300, 599):
        a = fr.event_filter(x[:cut], y[:cut], t[:cut], H, W, **kw)
        b = fr.event_filter(x[cut:], y[cut:], t[cut:], H, W, last_t=a["last_t"], **kw)
        assert np.array_equal(np.concatenate([a["cls"], b["cls"]]), whole["cls"]), cut
        assert np.array_equal(b["last_t"], whole["last_t"], equal_nan=True), cut


def test_bad_order():
    r = run([(5, 5, 2.0), (6, 5, 2.1), (5, 5, 1.9)], support_dt=1.0)
    assert r["status"].tolist() == [fr.BAD_ORDER, 3, 0, 0, 0, 0, 0, 0] and not r["keep"].any() and r["count"] == 0
    assert np.isnan(r["last_t"]).all() and np.isnan(r["stats"]).all() and np.isnan(r["xy"]).all() and (r["index"] == -1).all()
    state = np.full((H, W), NAN)
    state[5, 5] = 2.5
    assert run([(5, 5, 2.0)], last_t=state)["status"][0] == fr.BAD_ORDER
    assert run([(5, 5, 2.5)], last_t=state)["status"][0] == 0
    # per-pixel sorted, globally shuffled: allowed
    assert run([(5, 5, 2.0), (9, 9, 1.0), (5, 5, 2.0)])["status"][0] == 0


def test_a_shuffled_stream_gives_the_sorted_streams_classes():
    x, y, t = fr.stream(1500, seed=9)
    want = fr.event_filter(x, y, t, H, W, **fr.STREAM_PARAMS)
    perm = fr.shuffle_keeping_pixels(x, y, np.random.default_rng(2))
    got = fr.event_filter(x[perm], y[perm], t[perm], H, W, **fr.STREAM_PARAMS)
    assert got["status"][0] == 0
    # ties across pixels are ordered by index, which the shuffle changes: compare away from them
    clear = ~np.isin(t, t[1:][np.diff(t) == 0])
    assert clear.sum() > 1000 and np.array_equal(got["cls"][np.argsort(perm)][clear], want["cls"][clear])


# ------------------------------------------------------------------------------------------------ the streams
def test_the_stream_exercises_every_class():
    x, y, t = fr.stream(4099)
    assert len(t) == 4099 and (np.diff(t) >= 0).all() and (np.diff(t) == 0).sum() > 100
    r = fr.event_filter(x, y, t, H, W, **fr.STREAM_PARAMS)
    share = r["status"][2:] / 4099.0
    print("\nclass shares [2] .. [7]:", share.round(3), " stats:", r["stats"])
    assert r["status"][0] == 0 and r["status"][2:].sum() == 4099
    assert (share[2:] >= 0.05).all(), share
    thr = r["stats"][3]
    assert abs(thr - round(thr)) > 1e-6                           # a last-bit difference in sqrt cannot flip a pixel


def _mistake_case(mistake):
    """the stream and the parameters that tell ``mistake`` from the definition"""
    x, y, t = fr.stream(4099)
    kw = dict(fr.STREAM_PARAMS)
    if mistake == "hot_in_ignored":
        kw["hot_mask"] = (np.arange(H * W).reshape(H, W) % 7 == 0)
    if mistake == "sample_variance":                              # four active pixels with 1, 1, 1 and 5 events: thr = 4.6 against 5
        x, y, t = np.array([0, 1, 2, 3, 3, 3, 3, 3], np.float32), np.zeros(8, np.float32), np.arange(8.0)
        kw = dict(hot_sigma=1.5)
    return x, y, t, kw


@pytest.mark.parametrize("mistake", fr.MISTAKES)
def test_the_streams_reject_the_mistake(mistake):
    x, y, t, kw = _mistake_case(mistake)
    want = fr.event_filter(x, y, t, H, W, **kw)
    got = fr.event_filter(x, y, t, H, W, mistake=mistake, **kw)
    differ = int((want["cls"] != got["cls"]).sum())
    print("\n%-32s %d of %d events differ" % (mistake, differ, len(t)))
    assert differ > 0, "%s: %d events differ" % (mistake, differ)
