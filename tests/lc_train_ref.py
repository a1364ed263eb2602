"""float64 model of latency-controlled training of a bidirectional (concat) LSTM CTC network: what
tests/test_lc_train_host.py pins to tests/lookahead_ref.py and oracle.nasr_oracle, and what tests/test_gpu_lc_train.py holds
nasr_set_chunking to.

The rule, for one utterance of T_b frames, a chunk length C >= 1 and a look-ahead R >= 1: window k = 0, 1, ... holds rows
[kC, min(kC + C + R, T_b)), its P pending rows.  The first window with kC + C + R >= T_b is the last and emits all its rows
(E = P); every earlier one emits E = C rows.  Every layer runs window by window as lookahead_ref.run_window does: the
forward direction from the state after row E-1 of the window before (zero for window 0) over all P rows, the backward
direction from zero at row P-1 down to row 0, all P rows [fw | bw] handed up.  The utterance's logits are the emitted rows
in order.  Loss = mean over the batch of the CTC loss; its logit gradient comes from oracle.nasr_oracle.ctc_loss_and_grad
and autograd pushes it back, through the carried forward state too.

Parameter order: oracle.nasr_oracle.ModelSpec.param_shapes; cell arithmetic: lookahead_ref._cell, on torch float64."""
import numpy as np
import torch

from oracle import nasr_oracle as O


def windows(T_b, C, R):
    """[(start, P, E)] of an utterance of T_b frames"""
    assert T_b >= 1 and C >= 1 and R >= 1
    out, k = [], 0
    while True:
        s = k * C
        P = min(s + C + R, T_b) - s
        if s + C + R >= T_b:
            out.append((s, P, P))
            return out
        out.append((s, P, C))
        k += 1


def session_feeds(T_b, C, R):
    """the feeds of a look-ahead session that runs these windows: C + R rows, then C per feed, then the remainder with `last`
    (the remainder may be 0 rows: the session then flushes its R held rows)"""
    if T_b <= C + R:
        return [T_b]
    feeds, left = [C + R], T_b - C - R
    while left > C:
        feeds.append(C)
        left -= C
    feeds.append(left)
    if left == C:            # T_b = jC + R: every row has been fed, `last` comes with an empty feed
        feeds.append(0)
    return feeds


def _cell(x, h, c, kernel, bias, H, fb):
    g = torch.cat([x, h]) @ kernel + bias
    c = c * torch.sigmoid(g[2 * H:3 * H] + fb) + torch.sigmoid(g[0:H]) * torch.tanh(g[H:2 * H])
    return torch.tanh(c) * torch.sigmoid(g[3 * H:4 * H]), c


def _utterance(spec, p, x, C, R):
    """x [T_b, F] (tensor) -> logits [T_b, classes]"""
    H, L = spec.hidden, spec.num_layers
    zero = torch.zeros(H, dtype=torch.float64)
    state = [(zero, zero) for _ in range(L)]          # per layer the forward direction's (c, h)
    rows = []
    for s, P, E in windows(x.shape[0], C, R):
        a = x[s:s + P]
        for l in range(L):
            kf, bf, kb, bb = p[4 * l:4 * l + 4]
            c, h = state[l]
            fw = []
            for t in range(P):
                h, c = _cell(a[t], h, c, kf, bf, H, spec.forget_bias)
                fw.append(h)
                if t == E - 1:
                    state[l] = (c, h)
            c, h = zero, zero
            bw = [None] * P
            for t in range(P - 1, -1, -1):
                h, c = _cell(a[t], h, c, kb, bb, H, spec.forget_bias)
                bw[t] = h
            a = torch.stack([torch.cat([fw[t], bw[t]]) for t in range(P)])
        rows.append(a[:E] @ p[-2] + p[-1])
    return torch.cat(rows)


def _check(spec):
    assert spec.bidirectional and spec.merge == 'concat' and not spec.deepspeech and not any(spec.dropout)


def forward(spec, params, feats, seq_len, C, R, _tensors=None):
    """feats [B, T, F], seq_len [B] -> logits [T, B, classes] time-major (numpy float64); from seq_len[b] on the layers'
    outputs are zero and a row is the projection's bias, as in oracle.nasr_oracle.network_forward"""
    _check(spec)
    p = _tensors if _tensors is not None else [torch.tensor(np.asarray(q, np.float64)) for q in params]
    feats = np.asarray(feats, np.float64)
    B, T = feats.shape[0], feats.shape[1]
    out = p[-1].detach().repeat(T, B, 1)
    per = []
    for b in range(B):
        lg = _utterance(spec, p, torch.tensor(feats[b, :int(seq_len[b])]), C, R)
        per.append(lg)
    if _tensors is not None:
        return per
    for b, lg in enumerate(per):
        out[:lg.shape[0], b] = lg
    return out.detach().numpy()


def loss_and_grads(spec, params, feats, seq_len, labels, label_len, C, R):
    """(loss, nll [B], grads in parameter order, logits [T, B, classes]) as oracle.nasr_oracle.network_loss_and_grads"""
    _check(spec)
    p = [torch.tensor(np.asarray(q, np.float64), requires_grad=True) for q in params]
    per = forward(spec, params, feats, seq_len, C, R, _tensors=p)
    feats = np.asarray(feats)
    B, T = feats.shape[0], feats.shape[1]
    logits = np.tile(np.asarray(params[-1], np.float64), (T, B, 1))
    for b, lg in enumerate(per):
        logits[:lg.shape[0], b] = lg.detach().numpy()
    nll, dlog = O.ctc_loss_and_grad(logits, labels, label_len, seq_len)
    dlog = dlog / B
    # d loss / d params = sum over the utterances of (their logit gradient pushed back through their windows)
    surrogate = sum((per[b] * torch.tensor(dlog[:per[b].shape[0], b])).sum() for b in range(B))
    surrogate.backward()
    grads = [q.grad.numpy() if q.grad is not None else np.zeros(q.shape) for q in p]
    return float(nll.mean()), nll, grads, logits
