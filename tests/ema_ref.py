"""fp64 NumPy restatements of what DESIGN.md §23 adds to the optimiser: the exponential moving average of the parameters
(tf.train.ExponentialMovingAverage(decay, num_updates)) and the learning-rate schedule (tf.train.exponential_decay behind a
linear warm-up).  Written from the TF documentation's formulas, not from the library's code."""
import math

import numpy as np


def ema_decay_at(decay, n, constant=False):
    """d_n of the update that follows n applied ones: min(decay, (1 + n) / (10 + n)), or decay itself with `constant`"""
    decay = float(decay)
    return decay if constant else min(decay, (1.0 + n) / (10.0 + n))


def ema_run(e0, params, decay, n0=0, constant=False):
    """The average after the updates P_1..P_N (`params`, each the parameters an applied step produced), from the shadow
    value e0 with n0 updates behind it: E <- E + (1 - d_n)(P - E) = E - (1 - d_n)(E - P) in float64.  Returns (E_N, n0 + N)."""
    e = np.asarray(e0, dtype=np.float64).copy()
    n = int(n0)
    for p in params:
        d = ema_decay_at(decay, n, constant)
        e = e - (1.0 - d) * (e - np.asarray(p, dtype=np.float64))
        n += 1
    return e, n


def lr_schedule(base, s, warmup, decay_steps, rate, staircase):
    """the step size of the 1-based global step s, float64:
    base * min(1, s / warmup) * rate ** (max(0, s - warmup) / decay_steps), the exponent floored with `staircase`;
    warmup = 0: no warm-up, decay_steps = 0: no decay"""
    lr = float(base)
    if warmup > 0:
        lr *= min(1.0, s / float(warmup))
    if decay_steps > 0:
        e = max(0, s - warmup) / float(decay_steps)
        lr *= float(rate) ** (math.floor(e) if staircase else e)
    return lr
