"""The distillation term of DESIGN.md §22 restated in fp64 NumPy, for the tests of the GPU kernels and of the step.  Not
collected (no test_ prefix).

With student logits z and teacher logits y [T',B,C], weight a, temperature tau, p = softmax(y / tau), q = softmax(z / tau)
and len_b the logit frames of utterance b:

    kd_b = sum_{t < len_b, c} p_c (log p_c - log q_c)        KD = tau^2 mean_b kd_b
    loss = (1 - a) CTC + a KD                                 dloss/dz = (1 - a) dCTC/dz + a tau (q - p) / B

term() is the rule; with_term() puts it into oracle.nasr_oracle.ctc_loss_and_grad for as long as a `with` block lasts, so
that the oracle's own backward code (network_loss_and_grads, and tests/lc_train_ref.py over it) turns the combined logit
gradient into parameter gradients; wavenet_loss_and_grads() does the same for tests/wavenet_ref.py through autograd.
rows_f32() is the row formula in float32 NumPy, in the order the kernel uses: the measure of what fp32 can give."""
import contextlib

import numpy as np

from oracle import nasr_oracle as O


def log_softmax(x):
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def term(z, y, seq_len, a, tau):
    """(kd_b [B], a tau (q - p) / B as [T',B,C]) in fp64; frames t >= seq_len[b] contribute nothing and get zero rows"""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    Tp, B, C = z.shape
    lq, lp = log_softmax(z / tau), log_softmax(y / tau)
    p = np.exp(lp)
    live = (np.arange(Tp)[:, None] < np.asarray(seq_len)[None, :])[:, :, None]
    kd = np.where(live, p * (lp - lq), 0.0).sum(axis=(0, 2))
    grad = np.where(live, a * tau * (np.exp(lq) - p) / B, 0.0)
    return kd, grad


def conditioning(z, y, seq_len, tau):
    """[B]: sum p (1 + |log p| + |log q|) / kd_b, the factor by which kd_b amplifies the rounding of the log-softmaxes it is
    made of: a float32 log-softmax value v carries an absolute error of about eps (1 + |v|), whatever the arithmetic.  Two
    rows peaked on the same class have a KL of almost nothing, the difference of two such values: no fp32 evaluation of
    the rule gives that kd_b to full relative precision, and a test that measures relative error keeps its inputs clear of
    it."""
    z, y = np.asarray(z, np.float64), np.asarray(y, np.float64)
    lq, lp = log_softmax(z / tau), log_softmax(y / tau)
    p = np.exp(lp)
    live = (np.arange(z.shape[0])[:, None] < np.asarray(seq_len)[None, :])[:, :, None]
    kd = np.where(live, p * (lp - lq), 0.0).sum(axis=(0, 2))
    return np.where(live, p * (1.0 + np.abs(lp) + np.abs(lq)), 0.0).sum(axis=(0, 2)) / kd


def combined(ctc, kd, a, tau):
    """the loss from the batch-mean CTC loss and kd_b"""
    return (1.0 - a) * ctc + a * tau * tau * float(np.mean(kd))


def rows_f32(z, y, seq_len, a, tau):
    """term() in float32 arithmetic with the kernel's expressions: max-subtracted exponents scaled by 1 / tau, a float32 sum
    of exponentials, p and q by division, the row's KL summed in float32; kd_b sums the rows in fp64, as the kernel does."""
    f = np.float32
    z, y = np.asarray(z, f), np.asarray(y, f)
    Tp, B, C = z.shape
    it, gs = f(1) / f(tau), f(a) * f(tau) / f(B)
    uz = (z - z.max(axis=-1, keepdims=True)) * it
    uy = (y - y.max(axis=-1, keepdims=True)) * it
    ez, ey = np.exp(uz), np.exp(uy)
    sz, sy = ez.sum(axis=-1, keepdims=True, dtype=f), ey.sum(axis=-1, keepdims=True, dtype=f)
    q, p = ez / sz, ey / sy
    kl = (p * ((uy - np.log(sy)) - (uz - np.log(sz)))).sum(axis=-1, dtype=f)
    live = np.arange(Tp)[:, None] < np.asarray(seq_len)[None, :]
    kd = np.where(live, kl.astype(np.float64), 0.0).sum(axis=0)
    grad = np.where(live[:, :, None], gs * (q - p), f(0))
    assert grad.dtype == f
    return kd, grad


@contextlib.contextmanager
def with_term(teacher_logits, a, tau):
    """Inside the block oracle.nasr_oracle.ctc_loss_and_grad returns, for logits z, per-utterance losses
    (1 - a) nll_b + a tau^2 kd_b and the gradient (1 - a) dnll/dz + a tau (q - p): every caller takes the batch mean of the
    first and divides the second by B, which makes them the combined loss and its logit gradient."""
    plain = O.ctc_loss_and_grad

    def both(logits_tm, labels, label_len, seq_len, blank=None):
        nll, g = plain(logits_tm, labels, label_len, seq_len, blank)
        B = np.asarray(logits_tm).shape[1]
        kd, gk = term(logits_tm, teacher_logits, seq_len, a, tau)
        return (1.0 - a) * nll + a * tau * tau * kd, (1.0 - a) * g + gk * B
    O.ctc_loss_and_grad = both
    try:
        yield
    finally:
        O.ctc_loss_and_grad = plain


def network_loss_and_grads(spec, params, feats, seq_len, labels, label_len, teacher_logits, a, tau, chunking=None):
    """(loss, grads list in TF order, student logits) of the distilled step; chunking = (C, R): the student of
    tests/lc_train_ref.py"""
    with with_term(teacher_logits, a, tau):
        if chunking:
            from tests import lc_train_ref as LC
            loss, _, grads, logits = LC.loss_and_grads(spec, params, feats, seq_len, labels, label_len, *chunking)
        else:
            loss, _, grads, logits = O.network_loss_and_grads(spec, params, feats, seq_len, labels, label_len)
    return loss, grads, logits


def wavenet_loss_and_grads(spec, flat, feats, seq_len, labels, label_len, teacher_logits, a, tau):
    """(loss, flat grads in TF order) of a distilled training-mode pass of tests/wavenet_ref.py's network"""
    import torch
    from tests import wavenet_ref as W
    P = W.unflatten(spec, flat)
    for t in P.values():
        t.requires_grad_(True)
    logits, _ = W.forward(spec, P, feats, True)
    ctc, _ = W.ctc_mean(logits, seq_len, labels, label_len)
    lq = torch.log_softmax(logits / tau, dim=2)
    lp = torch.log_softmax(torch.as_tensor(np.asarray(teacher_logits, np.float64)) / tau, dim=2)
    live = torch.as_tensor(np.arange(logits.shape[0])[:, None] < np.asarray(seq_len)[None, :])[:, :, None]
    kd = torch.where(live, lp.exp() * (lp - lq), torch.zeros((), dtype=torch.float64)).sum(dim=(0, 2))
    loss = (1.0 - a) * ctc + a * tau * tau * kd.mean()
    loss.backward()
    return float(loss.detach()), W.flatten_grads(spec, P)
