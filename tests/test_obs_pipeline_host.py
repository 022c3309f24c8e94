"""The observation pipeline's semantics on the host (no library, no GPU): the two
restatements of tests/obs_pipeline_ref.py agree exactly over a grid of options, hand-written
known answers pin them, and dexterity_amd.manipulation.obs_pipeline_options maps composer's
units to the C ABI's and refuses what the device cannot express."""

import collections

import numpy as np
import pytest

from dexterity_amd import _lib
from dexterity_amd.manipulation import obs_pipeline_options
from tests import obs_pipeline_ref as ref

FIRST, MID, LAST = 0, 1, 2
W = 5


def _episodes(lengths=(1, 7, 13)):
    """Step types of episodes of the given numbers of control steps, back to back, and one
    more FIRST behind them."""
    st = []
    for n in lengths:
        st += [FIRST] + [MID] * (n - 1) + [LAST]
    return st + [FIRST]


@pytest.mark.parametrize("aggregator", ref.AGGREGATORS)
@pytest.mark.parametrize("padding", ref.PADDINGS)
@pytest.mark.parametrize("nsub", [1, 5])
def test_event_simulation_equals_closed_form(nsub, padding, aggregator):
    st = _episodes()
    rows = np.random.RandomState(3).standard_normal((len(st), W)).astype(np.float32)
    for m in (1, 2, 3):
        for d in (0, 1, 2, 5):
            for K in (1, 2, 4):
                a = ref.simulate_events(rows, st, nsub, m * nsub, d * nsub, K, padding, aggregator)
                b = ref.closed_form(rows, st, m, d, K, padding, aggregator)
                assert a.dtype == b.dtype == np.float32 and a.shape == b.shape
                assert a.shape == ((len(st), W) if aggregator else (len(st), K, W))
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (m, d, K)


@pytest.mark.parametrize("nsub", [2, 5])
def test_default_interval_one_reads_like_one_control_step(nsub):
    """Composer's default, update_interval 1 with a buffer of 1: the boundary read returns the
    boundary's own sample, as update_interval = n_sub_steps does -- with a delay too."""
    st = _episodes()
    rows = np.random.RandomState(4).standard_normal((len(st), W)).astype(np.float32)
    for d in (0, 1, 3):
        a = ref.simulate_events(rows, st, nsub, 1, d * nsub, 1)
        b = ref.closed_form(rows, st, 1, d, 1)
        assert np.array_equal(a, b)


def test_corruptor_runs_once_per_sample_in_both():
    st = _episodes()
    rows = np.random.RandomState(5).standard_normal((len(st), W)).astype(np.float32)
    sigma = np.array([0.0, 0.1, 0.0, 2.0, 0.5])
    for m, d, K in ((1, 0, 1), (2, 3, 4), (3, 1, 2)):
        ra, rb = np.random.RandomState(9), np.random.RandomState(9)
        a = ref.simulate_events(rows, st, 5, 5 * m, 5 * d, K, "initial_value", None, ref.gaussian_corruptor(ra, sigma))
        b = ref.closed_form(rows, st, m, d, K, "initial_value", None, ref.gaussian_corruptor(rb, sigma))
        assert np.array_equal(a, b)
        # W draws per sample, none on a step that takes no sample: an episode of L control
        # steps is observed at n = 0 .. L and sampled at the multiples of m among them
        samples = sum(L // m + 1 for L in (1, 7, 13)) + 1
        rc = np.random.RandomState(9)
        for _ in range(samples):
            rc.normal(scale=sigma, size=W)
        nxt = rc.standard_normal()
        assert ra.standard_normal() == nxt and rb.standard_normal() == nxt


def _both(rows, st, m, d, K, padding):
    a = ref.simulate_events(rows, st, 1, m, d, K, padding)
    b = ref.closed_form(rows, st, m, d, K, padding)
    assert np.array_equal(a, b)
    return a


def test_known_answers():
    o = np.arange(1, 7, dtype=np.float32)[:, None] * np.ones((1, 2), np.float32)  # o[i] = [i+1, i+1]
    st = [FIRST, MID, MID, MID, MID, MID]
    z = np.zeros(2, np.float32)
    # m = 1, d = 0, K = 3, ZERO: FIRST gives [0, 0, o0], then [0, o0, o1]
    r = _both(o, st, 1, 0, 3, "zero")
    assert np.array_equal(r[0], [z, z, o[0]]) and np.array_equal(r[1], [z, o[0], o[1]])
    assert np.array_equal(r[2], [o[0], o[1], o[2]]) and np.array_equal(r[3], [o[1], o[2], o[3]])
    # d = 2: FIRST and n = 1 are all zeros, n = 2 ends in o0
    r = _both(o, st, 1, 2, 3, "zero")
    assert not r[0].any() and not r[1].any()
    assert np.array_equal(r[2], [z, z, o[0]]) and np.array_equal(r[3], [z, o[0], o[1]])
    # INITIAL: FIRST gives [o0, o0, o0], including with d = 2
    for d in (0, 2):
        r = _both(o, st, 1, d, 3, "initial_value")
        assert np.array_equal(r[0], [o[0], o[0], o[0]])
    assert np.array_equal(r[1], [o[0], o[0], o[0]]) and np.array_equal(r[3], [o[0], o[0], o[1]])
    # m = 2: n = 1 repeats n = 0's read; n = 2 brings o2
    r = _both(o, st, 2, 0, 3, "zero")
    assert np.array_equal(r[1], r[0]) and np.array_equal(r[2], [z, o[0], o[2]]) and np.array_equal(r[3], r[2])
    # a FIRST in the middle starts afresh; LAST is an ordinary step
    r = _both(o, [FIRST, MID, LAST, FIRST, MID, MID], 1, 0, 3, "zero")
    assert np.array_equal(r[2], [o[0], o[1], o[2]]) and np.array_equal(r[3], [z, z, o[3]])


def test_aggregates_known_answers():
    o = np.array([[1.0, -2.0], [4.0, 0.5], [2.0, 8.0], [3.0, 1.0]], np.float32)
    st = [FIRST, MID, MID, MID]
    want = {"min": [1, -2], "max": [4, 8], "sum": [10, 7.5], "mean": [2.5, 1.875], "median": [2.5, 0.75]}
    for agg, w in want.items():
        a = ref.simulate_events(o, st, 1, 1, 0, 4, "zero", agg)
        b = ref.closed_form(o, st, 1, 0, 4, "zero", agg)
        assert np.array_equal(a, b) and np.array_equal(a[3], np.array(w, np.float32)), agg
    # the padding takes part: K = 4 at n = 1 is [0, 0, o0, o1]
    assert np.array_equal(ref.closed_form(o, st, 1, 0, 4, "zero", "median")[1], np.array([0.5, 0.0], np.float32))
    assert np.array_equal(ref.closed_form(o, st, 1, 0, 3, "zero", "median")[2], np.array([2.0, 0.5], np.float32))


# ---------------------------------------------------------------- the pure validation function
LAYOUT = collections.OrderedDict((("hand/joint_positions", slice(0, 3)), ("prop/position", 3), ("goal_state", 1)))


def test_options_accepted_forms():
    # composer's default: interval 1 with a buffer of 1
    assert obs_pipeline_options(5, 1, 1, 0)[:5] == (1, 0, 1, 0, 0)
    assert obs_pipeline_options(5)[:5] == (1, 0, 1, 0, 0) and obs_pipeline_options(5)[5] is None
    # physics steps -> control steps
    assert obs_pipeline_options(5, 10, 4, 15, "median", "initial_value")[:5] == (
        2, 3, 4, _lib.OBS_AGG["median"], _lib.OBS_PAD["initial_value"])
    assert obs_pipeline_options(1, 3, 2, 2, "sum", "ZERO")[:5] == (3, 2, 2, _lib.OBS_AGG["sum"], 0)
    assert obs_pipeline_options(5, np.int64(5), np.int32(2), 0)[:3] == (1, 0, 2)
    # noise_std: a float, an array, a dict by name (absent names get 0)
    s = obs_pipeline_options(5, noise_std=0.25, widths=LAYOUT)[5]
    assert s.dtype == np.float64 and np.array_equal(s, np.full(7, 0.25))
    s = obs_pipeline_options(5, noise_std=np.arange(7), widths=LAYOUT)[5]
    assert np.array_equal(s, np.arange(7.0))
    s = obs_pipeline_options(5, noise_std={"prop/position": [1, 2, 3], "goal_state": 0.5}, widths=LAYOUT)[5]
    assert np.array_equal(s, [0, 0, 0, 1, 2, 3, 0.5])
    assert np.array_equal(obs_pipeline_options(5, noise_std=0.0, widths=LAYOUT)[5], np.zeros(7))


@pytest.mark.parametrize("kw, reason", [
    (dict(update_interval=7), "not a multiple"),
    (dict(update_interval=1, buffer_size=2), "not a multiple"),
    (dict(delay=3), "not a multiple"),
    (dict(delay=-5), "negative"),
    (dict(update_interval=lambda: 5), "callables"),
    (dict(delay=lambda: 5), "callables"),
    (dict(buffer_size=lambda: 1), "callables"),
    (dict(aggregator=np.mean), "callables"),
    (dict(noise_std=lambda v, random_state: v), "callables"),
    (dict(update_interval=5.0), "integer"),
    (dict(update_interval=0), "at least 1"),
    (dict(aggregator="mode"), "unknown aggregator"),
    (dict(padding="edge"), "unknown padding"),
    (dict(buffer_size=0), "at least 1"),
    (dict(buffer_size=17), "device limit"),
    (dict(update_interval=5 * 65), "device limits"),
    (dict(delay=5 * 65), "device limits"),
    (dict(noise_std=-0.1), "not negative"),
    (dict(noise_std={"goal_state": -1.0}), "not negative"),
    (dict(noise_std=float("nan")), "finite"),
    (dict(noise_std=np.ones(6)), "entries"),
    (dict(noise_std={"prop/position": [1.0, 2.0]}), "entries"),
    (dict(noise_std={"prop/velocity": 1.0}), "unknown observables"),
])
def test_options_rejected(kw, reason):
    with pytest.raises(ValueError, match=reason):
        obs_pipeline_options(5, widths=LAYOUT, **kw)
