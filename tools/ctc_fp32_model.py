#!/usr/bin/env python3
"""The error the CTC lattice's fp32 arithmetic alone makes at the long and sharp cases of tests/test_gpu_ctc_lattice.py, on the
CPU: recursion (2) of csrc/ctc.hip (log domain, columns rescaled by their maximum every 4 frames, fp64 offsets) in numpy
float32 with correctly rounded exp and log (ctc_fp32 of tests/ctc_ref.py), against the fp64 oracle on the same logits.  Prints the relative error of the
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

from ctc_ref import ctc_fp32  # noqa: E402


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
