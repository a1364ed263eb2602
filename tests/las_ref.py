"""An independent fp64 torch-CPU model of the reference's LAS (networks/las.py) for the tests: the pyramidal BiLSTM encoder,
the attention decoder with the per-step input ids given (so that a GPU pass's scheduled samples can be replayed),
sequence_loss, and the sampling hash of neuralasr_amd/csrc/las.hip."""
import numpy as np
import torch

from neuralasr_amd.networks.las import tensor_specs

H = 250


def unflatten(flat, F, C):
    out, off = {}, 0
    for name, r, c in tensor_specs(F, C):
        n = r * c
        t = torch.tensor(np.asarray(flat[off:off + n], np.float64).reshape(r, c) if c > 1 else
                         np.asarray(flat[off:off + n], np.float64), requires_grad=True)
        out[name] = t
        off += n
    return out


def _cell(x, h, c, W, b):
    g = torch.cat([x, h], 1) @ W + b
    i, j, f, o = g.split(g.shape[1] // 4, 1)
    c = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    return torch.tanh(c) * torch.sigmoid(o), c


def forward(P, feats, labels, ids):
    """feats [B,T,F], labels [B,U], ids [B,U] (the inputs fed to every step) -> logits [B,U,C]"""
    x = torch.tensor(np.asarray(feats, np.float64))
    B = x.shape[0]
    for i in range(4):
        if x.shape[1] % 2:
            x = torch.cat([x, torch.zeros(B, 1, x.shape[2], dtype=x.dtype)], 1)
        L = x.shape[1]
        outs = []
        finals = []
        for d in ('fw', 'bw'):
            W, b = P['bidirectional_rnn/%s/%s_%d/kernel' % (d, d, i)], P['bidirectional_rnn/%s/%s_%d/bias' % (d, d, i)]
            h = torch.zeros(B, H, dtype=x.dtype)
            c = torch.zeros(B, H, dtype=x.dtype)
            seq = [None] * L
            order = range(L) if d == 'fw' else range(L - 1, -1, -1)
            for t in order:
                h, c = _cell(x[:, t], h, c, W, b)
                seq[t] = h
            outs.append(torch.stack(seq, 1))
            finals.append((h, c))
        mem = torch.cat(outs, 2)
        x = torch.cat([mem[:, 0::2], mem[:, 1::2]], 2)
    hd = torch.cat([finals[0][0], finals[1][0]], 1)
    cd = torch.cat([finals[0][1], finals[1][1]], 1)
    keys = mem @ P['memory_layer/kernel']
    C = P['projection_layer/bias'].shape[0]
    a = torch.zeros(B, H, dtype=x.dtype)
    ids = torch.tensor(np.asarray(ids, np.int64))
    logits = []
    for t in range(ids.shape[1]):
        inp = torch.cat([torch.nn.functional.one_hot(ids[:, t], C).to(x.dtype), a], 1)
        hd, cd = _cell(inp, hd, cd, P['decoder_lstm/kernel'], P['decoder_lstm/bias'])
        q = hd @ P['query_layer/kernel']
        score = (torch.tanh(keys + q[:, None, :]) * P['attention_v']).sum(2)
        alpha = torch.softmax(score, 1)
        ctx = (alpha[:, :, None] * mem).sum(1)
        a = torch.cat([hd, ctx], 1) @ P['attention_layer/kernel']
        logits.append(a @ P['projection_layer/kernel'] + P['projection_layer/bias'])
    return torch.stack(logits, 1)


def sequence_loss(logits, labels, labels_len):
    U = logits.shape[1]
    w = torch.tensor((np.arange(U)[None, :] < np.asarray(labels_len)[:, None]).astype(np.float64))
    ce = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[2]),
                                           torch.tensor(np.asarray(labels, np.int64)).reshape(-1), reduction='none')
    return (ce * w.reshape(-1)).sum() / (w.sum() + 1e-12)


def loss_and_grads(flat, F, C, feats, labels, labels_len, ids=None):
    """(loss, logits [B,U,C], flat gradient in TF order) in fp64"""
    P = unflatten(flat, F, C)
    ids = labels if ids is None else ids
    logits = forward(P, feats, labels, ids)
    loss = sequence_loss(logits, labels, labels_len)
    loss.backward()
    g = np.concatenate([P[n].grad.detach().numpy().ravel() for n, _, _ in tensor_specs(F, C)])
    return float(loss), logits.detach().numpy(), g


def lowbias32(x):
    x = np.uint32(x)
    with np.errstate(over='ignore'):
        x ^= x >> np.uint32(16); x = np.uint32(x * np.uint32(0x7FEB352D))
        x ^= x >> np.uint32(15); x = np.uint32(x * np.uint32(0x846CA68B))
        x ^= x >> np.uint32(16)
    return np.uint32(x)


def sample_uniforms(seed, counter, tower, t, b):
    """(u0, u1): the 24-bit Bernoulli and inverse-CDF draws of utterance b's input at step t"""
    with np.errstate(over='ignore'):
        key = np.uint32((seed + 0x9E3779B9 * (tower + 1) + 0x85EBCA6B * counter) & 0xFFFFFFFF)
    base = np.uint32(((t * 64 + b) * 2) & 0xFFFFFFFF)
    return int(lowbias32(base ^ key) >> np.uint32(8)), int(lowbias32(np.uint32(base + 1) ^ key) >> np.uint32(8))
