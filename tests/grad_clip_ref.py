"""fp64 restatement of the optimiser step with global-norm clipping (include/nasr.h, nasr_set_grad_clip):
the decision the device takes from the gradient's norm, then TF's Adam on the scaled gradient."""
import numpy as np


def global_norm(g, grad_scale=1.0):
    """|grad_scale| * sqrt(sum g_i^2) over the flat gradient, in fp64"""
    g = np.asarray(g, np.float64).ravel()
    with np.errstate(over='ignore', invalid='ignore'):
        return abs(float(grad_scale)) * float(np.sqrt(np.dot(g, g)))


def decide(g, max_norm, grad_scale=1.0):
    """(skip, norm, coef): tf.clip_by_global_norm's rule, coef = max_norm / norm where the norm exceeds max_norm and 1
    otherwise; a norm that is not finite skips the step (coef is None then).  max_norm may be inf."""
    norm = global_norm(g, grad_scale)
    if not np.isfinite(norm):
        return True, norm, None
    return False, norm, (float(max_norm) / norm if norm > float(max_norm) else 1.0)


def adam_tf(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer on flat fp64 arrays: lr_t = lr*sqrt(1-b2^t)/(1-b1^t), eps added to sqrt(v) uncorrected;
    step = t of this update (1 for the first).  Returns the new (p, m, v)."""
    lr_t = lr * np.sqrt(1 - beta2 ** step) / (1 - beta1 ** step)
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def clipped_step(p, g, m, v, step, lr, max_norm, grad_scale=1.0, **adam):
    """One optimiser step: (p, m, v, step, info).  A skipped step returns its inputs; step counts the applied updates."""
    skip, norm, coef = decide(g, max_norm, grad_scale)
    info = {'skip': skip, 'norm': norm, 'coef': coef}
    if skip:
        return p, m, v, step, info
    g = np.asarray(g, np.float64) * (float(grad_scale) * coef)
    p, m, v = adam_tf(np.asarray(p, np.float64), g, np.asarray(m, np.float64), np.asarray(v, np.float64), step + 1, lr, **adam)
    return p, m, v, step + 1, info
