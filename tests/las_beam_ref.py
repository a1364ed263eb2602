"""A NumPy restatement of the LAS inference graph's beam search (tf.contrib.seq2seq.BeamSearchDecoder and gather_tree of
TF 1.15, as DESIGN.md §10 writes the rules out) in float32 and TF's operation order, driven by a callback that gives the
logits of the current beam rows; and an fp64 replay of tests/las_ref.py's model along a given parent / word trace."""
import ctypes
import ctypes.util

import numpy as np
import torch

from tests import las_ref

F32 = np.float32
FLT_LOWEST = F32(-3.4028235e38)


_libm = ctypes.CDLL(ctypes.util.find_library('m'))
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def penalty(n, weight):
    """((5 + n)^w / 6^w) in float32 with the C library's powf (the pow of TF's CPU kernel); exactly 1 when w is 0 (TF's
    static shortcut)"""
    n = np.asarray(n)
    if weight == 0:
        return np.ones(n.shape, F32)
    top = int(n.max()) if n.size else 0
    table = np.array([F32(_libm.powf(5.0 + k, weight)) / F32(_libm.powf(6.0, weight)) for k in range(top + 1)], F32)
    return table[n]


def log_softmax(logits):
    logits = np.asarray(logits, F32)
    sh = logits - logits.max(axis=-1, keepdims=True)
    return sh - np.log(np.exp(sh).sum(axis=-1, keepdims=True, dtype=F32))


def step(logits, log_probs, finished, lengths, end_id, weight):
    """one step: (scores [B,W] top-W, word [B,W], parent [B,W], new log_probs, finished, lengths, sorted flat scores)"""
    B, W, C = logits.shape
    with np.errstate(over='ignore', invalid='ignore'):
        lp = log_softmax(logits)
        is_end = np.arange(C) == end_id
        lp = np.where(finished[..., None], np.where(is_end, F32(0), FLT_LOWEST)[None, None, :], lp).astype(F32)
        total = (log_probs[..., None] + lp).astype(F32)
        len_s = lengths[..., None] + ((~finished)[..., None] & ~is_end[None, None, :]).astype(np.int64)
        score = (total / penalty(len_s, weight)).astype(F32)
    flat = score.reshape(B, W * C)
    idx = np.arange(W * C)
    order = np.stack([np.lexsort((idx, -flat[b].astype(np.float64))) for b in range(B)])
    sel = order[:, :W]
    scores = np.take_along_axis(flat, sel, 1)
    parent, word = sel // C, sel % C
    new_lp = np.take_along_axis(total.reshape(B, W * C), sel, 1)
    prev_fin = np.take_along_axis(finished, parent, 1)
    fin = prev_fin | (word == end_id)
    lens = np.take_along_axis(lengths, parent, 1) + (~prev_fin).astype(np.int64)
    return scores, word, parent, new_lp, fin, lens, np.take_along_axis(flat, order, 1)


def beam_search(logits_fn, B, W, C, start_id, end_id, max_steps, weight=0.5):
    """logits_fn(t, parent [B,W] or None at t = 0, ids [B,W]) -> logits [B,W,C] of the beam rows after feeding ids (the
    callback gathers its own state by parent first).  Returns a dict of the trace [T_dec,B,W] ('scores', 'word',
    'parent'), the final 'log_probs' / 'finished' / 'lengths' [B,W], 'steps' = T_dec, gather_tree's 'ids' [T_dec,B,W]
    and 'margin' [T_dec]: the least non-zero gap between consecutive scores among an utterance's best W+1 that are
    ordinary finite values (inf when there is none).  A margin well above float32 rounding means the order of the best
    W+1 (exact ties aside, which both sides break by index) does not hang on the last bits."""
    log_probs = np.full((B, W), -np.inf, F32)
    log_probs[:, 0] = 0
    finished = np.ones((B, W), bool)
    finished[:, 0] = False
    lengths = np.zeros((B, W), np.int64)
    ids = np.full((B, W), start_id, np.int64)
    parent = None
    tr = {'scores': [], 'word': [], 'parent': [], 'margin': []}
    for t in range(max_steps):
        logits = np.asarray(logits_fn(t, parent, ids), F32)
        sc, word, parent, log_probs, finished, lengths, srt = step(logits, log_probs, finished, lengths, end_id, weight)
        ids = word
        tr['scores'].append(sc)
        tr['word'].append(word)
        tr['parent'].append(parent)
        top = srt[:, :W + 1].astype(np.float64)
        with np.errstate(invalid='ignore'):
            d = top[:, :-1] - top[:, 1:]
        ok = np.isfinite(top[:, 1:]) & (top[:, 1:] > -1e30) & (d != 0)
        tr['margin'].append(float(d[ok].min()) if ok.any() else np.inf)
        if finished.all():
            break
    out = {k: np.stack(v) if k != 'margin' else np.asarray(v) for k, v in tr.items()}
    out.update(log_probs=log_probs, finished=finished, lengths=lengths, steps=len(tr['word']))
    out['ids'] = gather_tree(out['word'], out['parent'], lengths.max(axis=1), end_id)
    return out


def gather_tree(step_ids, parent_ids, max_len, end_id):
    """TF 1.15's gather_tree kernel: [T,B,W] ids from [T,B,W] step ids and parents, max_len [B]"""
    T, B, W = step_ids.shape
    out = np.full((T, B, W), end_id, np.int64)
    for b in range(B):
        ml = min(T, int(max_len[b]))
        if ml <= 0:
            continue
        out[ml - 1, b] = step_ids[ml - 1, b]
        p = np.asarray(parent_ids[ml - 1, b], np.int64)
        for lvl in range(ml - 2, -1, -1):
            out[lvl, b] = step_ids[lvl, b, p]
            p = np.asarray(parent_ids[lvl, b, p], np.int64)
        is_end = out[:ml, b] == end_id
        after = (np.cumsum(is_end, axis=0) - is_end) > 0
        out[:ml, b][after] = end_id
    return out


def encode(P, feats):
    """las_ref's encoder in fp64: (memory [B,L4,500], h0 [B,500], c0 [B,500])"""
    x = torch.tensor(np.asarray(feats, np.float64))
    B = x.shape[0]
    H = las_ref.H
    for i in range(4):
        if x.shape[1] % 2:
            x = torch.cat([x, torch.zeros(B, 1, x.shape[2], dtype=x.dtype)], 1)
        L = x.shape[1]
        outs, finals = [], []
        for d in ('fw', 'bw'):
            W, b = P['bidirectional_rnn/%s/%s_%d/kernel' % (d, d, i)], P['bidirectional_rnn/%s/%s_%d/bias' % (d, d, i)]
            h = torch.zeros(B, H, dtype=x.dtype)
            c = torch.zeros(B, H, dtype=x.dtype)
            seq = [None] * L
            for t in (range(L) if d == 'fw' else range(L - 1, -1, -1)):
                h, c = las_ref._cell(x[:, t], h, c, W, b)
                seq[t] = h
            outs.append(torch.stack(seq, 1))
            finals.append((h, c))
        mem = torch.cat(outs, 2)
        x = torch.cat([mem[:, 0::2], mem[:, 1::2]], 2)
    return mem, torch.cat([finals[0][0], finals[1][0]], 1), torch.cat([finals[0][1], finals[1][1]], 1)


class Replay:
    """The fp64 decoder of tests/las_ref.py over B*W beam rows (memory and initial state tiled), usable as the callback of
    beam_search or stepped along a recorded trace: logits(t, parent, ids) -> [B,W,C] float64."""

    def __init__(self, flat, F, C, feats, W):
        self.P = las_ref.unflatten(flat, F, C)
        with torch.no_grad():
            mem, h, c = encode(self.P, feats)
            self.keys = (mem @ self.P['memory_layer/kernel']).repeat_interleave(W, 0)
        self.mem = mem.repeat_interleave(W, 0)
        self.B, self.W, self.C = mem.shape[0], W, C
        self.h, self.c = h.repeat_interleave(W, 0), c.repeat_interleave(W, 0)
        self.a = torch.zeros(self.B * W, las_ref.H, dtype=torch.float64)

    @torch.no_grad()
    def __call__(self, t, parent, ids):
        B, W, C, P = self.B, self.W, self.C, self.P
        if parent is not None:
            rows = torch.tensor((np.arange(B)[:, None] * W + np.asarray(parent)).ravel())
            self.h, self.c, self.a = self.h[rows], self.c[rows], self.a[rows]
        x = torch.nn.functional.one_hot(torch.tensor(np.asarray(ids, np.int64).ravel()), C).to(torch.float64)
        self.h, self.c = las_ref._cell(torch.cat([x, self.a], 1), self.h, self.c, P['decoder_lstm/kernel'], P['decoder_lstm/bias'])
        q = self.h @ P['query_layer/kernel']
        score = (torch.tanh(self.keys + q[:, None, :]) * P['attention_v']).sum(2)
        alpha = torch.softmax(score, 1)
        ctx = (alpha[:, :, None] * self.mem).sum(1)
        self.a = torch.cat([self.h, ctx], 1) @ P['attention_layer/kernel']
        logits = self.a @ P['projection_layer/kernel'] + P['projection_layer/bias']
        return logits.numpy().reshape(B, W, C)
