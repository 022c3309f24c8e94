"""Two independent fp64 / numpy restatements of the observation pipeline (include/dx.h
dx_env_set_obs_pipeline) for one env, over a recorded sequence of raw rows and step types:

  simulate_events  composer's observation updater as an event simulation at PHYSICS-step
                   granularity ([3P] dm_control composer observation updater / buffer, written
                   from its description): a pending queue with arrival times, a K-deep buffer,
                   an insertion at time 0 on reset, a read at each control-step boundary;
  closed_form      the index rule the kernel uses: n, J = floor((n - d) / m), slot k = s_{J-(K-1-k)}.

rows is [T, W] float32 (the env's DX_OUT_OBS || hand row after each call), step_types [T]
(0 FIRST, 1 MID, 2 LAST); the first entry starts an episode whatever its step type (the
pipeline was switched on there).  corrupt(row) -> row is called once per sample taken, in
the order the samples are taken (None: no corruptor).  Both return float32 [T, K, W], or
[T, W] with an aggregator.
"""

import collections

import numpy as np

FIRST = 0
AGGREGATORS = (None, "min", "max", "mean", "median", "sum")
PADDINGS = ("zero", "initial_value")


def _aggregate_numpy(slots, aggregator):
    """numpy's own reductions over axis 0 of the float64 [K, W] stack."""
    x = np.asarray(slots, dtype=np.float64)
    if aggregator is None:
        return x.astype(np.float32)
    return getattr(np, aggregator)(x, axis=0).astype(np.float32)


def _aggregate_definition(slots, aggregator):
    """The stated fp64 definitions, spelled out: the sum in slot order (oldest first), mean =
    sum / K, the median of an even K as (a + b) * 0.5, every result rounded to fp32 once."""
    x = np.asarray(slots, dtype=np.float64)
    K = x.shape[0]
    if aggregator is None:
        return x.astype(np.float32)
    if aggregator in ("sum", "mean"):
        s = x[0].copy()
        for k in range(1, K):
            s = s + x[k]
        return (s / K if aggregator == "mean" else s).astype(np.float32)
    if aggregator == "min":
        return x.min(axis=0).astype(np.float32)
    if aggregator == "max":
        return x.max(axis=0).astype(np.float32)
    assert aggregator == "median"
    srt = np.sort(x, axis=0)
    return ((srt[(K - 1) // 2] + srt[K // 2]) * 0.5).astype(np.float32)


def simulate_events(rows, step_types, nsub, update_interval, delay, buffer_size, padding="zero",
                    aggregator=None, corrupt=None):
    """update_interval and delay in PHYSICS steps, as composer counts them."""
    rows = np.asarray(rows, dtype=np.float32)
    W = rows.shape[1]
    corrupt = corrupt or (lambda r: r)
    out = []
    t = 0                          # physics steps since the episode's reset
    pending = collections.deque()  # (arrival time, value) in sampling order
    buf = collections.deque(maxlen=buffer_size)
    for i, (row, st) in enumerate(zip(rows, step_types)):
        if i == 0 or st == FIRST:
            # the updater's reset: an empty history, the first sample inserted at time 0
            t = 0
            pending.clear()
            buf.clear()
            initial = np.asarray(corrupt(row), dtype=np.float32)
            pad = initial if padding == "initial_value" else np.zeros(W, np.float32)
            for _ in range(buffer_size):
                buf.append(pad)
            pending.append((delay, initial))
        else:
            # one control step: update() after every physics step
            for _ in range(nsub):
                t += 1
                if t % update_interval == 0:
                    # the device has a row only at the boundary; a sample inside the control
                    # step (interval 1 with a buffer of 1) is a value no boundary read returns
                    value = np.asarray(corrupt(row), dtype=np.float32) if t % nsub == 0 else None
                    pending.append((t + delay, value))
        while pending and pending[0][0] <= t:
            buf.append(pending.popleft()[1])
        slots = list(buf)
        assert all(s is not None for s in slots), "a boundary read returned a sample taken inside a control step"
        out.append(_aggregate_numpy(slots, aggregator))
    return np.stack(out)


def closed_form(rows, step_types, m, d, K, padding="zero", aggregator=None, corrupt=None):
    """m and d in CONTROL steps."""
    rows = np.asarray(rows, dtype=np.float32)
    W = rows.shape[1]
    corrupt = corrupt or (lambda r: r)
    out = []
    n, samples = 0, []
    for i, (row, st) in enumerate(zip(rows, step_types)):
        if i == 0 or st == FIRST:
            n, samples = 0, []
        else:
            n += 1
        if n % m == 0:
            samples.append(np.asarray(corrupt(row), dtype=np.float32))
            assert len(samples) == n // m + 1
        J = (n - d) // m if n >= d else -1
        slots = []
        for k in range(K):
            j = J - (K - 1 - k)
            if j >= 0:
                slots.append(samples[j])
            else:
                slots.append(samples[0] if padding == "initial_value" else np.zeros(W, np.float32))
        out.append(_aggregate_definition(slots, aggregator))
    return np.stack(out)


def gaussian_corruptor(random_state, sigma):
    """The one corruptor built: v + random_state.normal(scale=sigma, size=v.shape) in fp64,
    rounded to fp32 once; a zero sigma still consumes its draw."""
    sigma = np.asarray(sigma, dtype=np.float64)

    def corrupt(row):
        v = np.asarray(row, dtype=np.float64)
        return (v + random_state.normal(scale=sigma, size=v.shape)).astype(np.float32)

    return corrupt
