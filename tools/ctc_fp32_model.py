#!/usr/bin/env python3
"""The error the CTC lattice's fp32 arithmetic alone makes at the long and sharp cases of tests/test_gpu_ctc_lattice.py, on the
CPU: recursion (2) of csrc/ctc.hip (log domain, columns rescaled by their maximum every 4 frames, fp64 offsets) in numpy
float32 with correctly rounded exp and log, against the fp64 oracle on the same logits.  Prints the relative error of the
projection bias gradient b (the frame sum of the logit gradient) and of the whole logit gradient, b of the fp64 lattice on
logits with noise of 5e-6, and, for the WaveNet case, the worst network gradient when only the lattice is fp32.  The test's
tolerances quote these numbers.
    python tools/ctc_fp32_model.py [--group G]       (G frames between rescalings, 4 as in the kernels)"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle import nasr_oracle as O  # noqa: E402

F32 = np.float32
NEG = F32(-1e30)


def lse3(a, b, c):
    m = np.maximum(a, np.maximum(b, c))
    return (m + np.log(np.exp(a - m) + np.exp(b - m) + np.exp(c - m))).astype(F32)


def ctc_fp32(logits, label, blank, G=4):
    """(nll, d nll / d logits) of one utterance, logits [T, C], as recursion (2) computes them in fp32"""
    x = np.asarray(logits, F32)
    T, C = x.shape
    mx = x.max(1, keepdims=True)
    z = (mx[:, 0] + np.log(np.exp(x - mx).sum(1))).astype(F32)
    L = len(label)
    S = 2 * L + 1
    ext = np.full(S, blank)
    ext[1::2] = label
    e = (x[:, ext] - z[:, None]).astype(F32)
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    skip_f = np.zeros(S, bool)
    skip_f[:-2] = skip[2:]

    def rescale(v, off):
        m = v.max()
        return np.where(v > NEG / 2, v - m, NEG).astype(F32), off + float(m)
    al, ao = np.full((T, S), NEG, F32), np.zeros(T)
    a, A = np.full(S, NEG, F32), 0.0
    a[:2] = e[0, :2]
    al[0] = a
    for t in range(1, T):
        if (t - 1) % G == 0:
            a, A = rescale(a, A)
        a1 = np.concatenate([[NEG], a[:-1]]).astype(F32)
        a2 = np.where(skip, np.concatenate([[NEG, NEG], a])[:S], NEG).astype(F32)
        a = (e[t] + lse3(a, a1, a2)).astype(F32)
        al[t], ao[t] = a, A
    be, bo = np.full((T, S), NEG, F32), np.zeros(T)
    b, Bo = np.full(S, NEG, F32), 0.0
    b[max(S - 2, 0):] = 0
    be[T - 1] = b
    for t in range(T - 2, -1, -1):
        if (T - 2 - t) % G == 0:
            b, Bo = rescale(b, Bo)
        bb = (b + e[t + 1]).astype(F32)
        b1 = np.concatenate([bb[1:], [NEG]]).astype(F32)
        b2 = np.where(skip_f, np.concatenate([bb, [NEG, NEG]])[2:], NEG).astype(F32)
        b = lse3(bb, b1, b2)
        be[t], bo[t] = b, Bo
    logp = A + float(lse3(a[S - 1], a[S - 2] if S > 1 else NEG, NEG))
    w = np.exp(al.astype(np.float64) + be + (ao + bo - logp)[:, None])
    post = np.zeros((T, C))
    for s in range(S):
        post[:, ext[s]] += w[:, s]
    return -logp, np.exp(x.astype(np.float64) - z[:, None]) - post


def logit_grads(logits, seq_len, labels, label_len, G):
    """d nll / d logits [T, B, C] of the fp64 oracle and of the fp32 model"""
    C = logits.shape[2]
    g64, g32 = np.zeros_like(logits), np.zeros_like(logits)
    for b in range(logits.shape[1]):
        Tb, lab = int(seq_len[b]), labels[b, :int(label_len[b])]
        g64[:Tb, b] = O.ctc_single(logits[:Tb, b], lab, C - 1)[1]
        g32[:Tb, b] = ctc_fp32(logits[:Tb, b], lab, C - 1, G)[1]
    return g64, g32


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--group', type=int, default=4)
    G = ap.parse_args().group
    import test_gpu_ctc_lattice as TL
    for scale, Lmax, T in ((60.0, 255, 1000), (60.0, 511, 1000), (1.0, 511, 1100)):
        spec = O.ModelSpec(5, 16, 1, True, 'concat', 29)
        sharp = scale > 1
        params = TL.net_params(spec, Lmax + 1 if sharp else Lmax, scale=scale)
        batch = TL.lattice_batch(29, Lmax, seed=Lmax + 29 if sharp else Lmax * 7 + 29, T=T)
        logits, _ = O.network_forward(spec, params, batch[0], batch[1])
        g64, g32 = logit_grads(logits, *batch[1:], G)
        # what the engine's own logit error (3e-7; 1.5e-5 scaled by 60) can do: the fp64 lattice on logits + 5e-6 noise
        noisy = logits + np.random.RandomState(0).randn(*logits.shape) * 5e-6
        g64n = logit_grads(noisy, *batch[1:], G)[0]
        print('%s Lmax %d T %d: b %.2g, logit gradient %.2g; fp64 on logits + 5e-6 noise: b %.2g' % (
              'sharp' if sharp else 'flat', Lmax, T, rel(g32.sum((0, 1)), g64.sum((0, 1))), rel(g32, g64),
              rel(g64n.sum((0, 1)), g64.sum((0, 1)))), flush=True)
    # the WaveNet case: the network in fp64 torch, only the lattice's logit gradient from the fp32 model
    import torch
    import test_gpu_wavenet as TW
    import wavenet_ref as W
    spec = W.Spec(13, 29, num_blocks=1)
    _, seq_len, labels, label_len = TL.lattice_batch(29, 450, seed=450, T=600)
    rs = np.random.RandomState(451)
    feats = rs.randn(4, 600, spec.F).astype(np.float32)
    for b in range(4):
        feats[b, seq_len[b]:] = 0
    flat = TW.start_params(spec, 12)
    out = []
    for k in range(2):
        P = W.unflatten(spec, flat)
        for t in P.values():
            t.requires_grad_(True)
        logits, _ = W.forward(spec, P, feats, True)
        g = logit_grads(logits.detach().numpy(), seq_len, labels, label_len, G)[k] / len(seq_len)
        logits.backward(torch.tensor(g))
        out.append(W.flatten_grads(spec, P))
    floor, o, errs = 1e-3 * np.linalg.norm(out[0]), 0, {}
    for name, r, c in W.tensor_specs(spec):
        a, b = out[1][o:o + r * c], out[0][o:o + r * c]
        errs[name] = np.linalg.norm(a - b) / max(np.linalg.norm(b), floor)
        o += r * c
    worst = max(errs, key=errs.get)
    print('wavenet Lmax 450 T 600: worst gradient tensor %s %.2g' % (worst, errs[worst]))


if __name__ == '__main__':
    main()
