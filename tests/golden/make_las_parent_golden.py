"""Generates tests/golden/las_parent.json: SHA-256 digests of what LasEngine's training pass and beam search give for the
cases below (tests/test_gpu_las_parent_bits.py runs the same cases and compares).  Run it on an MI355X with the commit
BEFORE a change to the LAS decoder step, its attention kernel or its initial-state gather built
(`python tests/golden/make_las_parent_golden.py`); a change that claims to keep every bit is then measured against what
that commit computed.  A mismatch is fixed in the code, never by running this again.

Only data is written: digests (floats as float32(x + 0.0) bytes, so the sign of an exact zero does not count; int arrays
as they are), and a few plain numbers (loss, gradient norm, T_dec) that tell a reader of a failing test how far apart the
two results are in value.  Only LasEngine's public calls are used; every input comes from a fixed numpy seed."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'las_parent.json')

F = 13
NOISE = 0.05

# T, B, U, C, sampling probability                 L4   what it reaches
TRAIN = [
    (1, 1, 1, 5, 0.0),       # 2    fewer frames than the attention kernel's four waves
    (17, 5, 7, 5, 0.0),      # 4    Bp = 16, one padded block of rows
    (17, 5, 7, 5, 1.0),      # 4    every step fed a sample: fed_ids() depends on the logits' bits
    (100, 17, 3, 33, 0.1),   # 14   L4 no multiple of 4; Bp = 32; Cp = 64
]

# B, T, W, C, length penalty, max_steps, n-gram (order, weight) or None, bias added at the end id
# chosen on the host with tests/las_beam_ref.py's fp64 replay: at 0.5 the last case's search finishes after 3 of 20 steps with
# a least score margin of 0.035 (at 0.4 and below it runs into the cut at 20); main asserts the step count
END_BIAS = 0.5
SEARCH = [
    (1, 1, 4, 3, 0.5, 10, None, 0.0),        # nrows 4 of R 16
    (5, 17, 1, 7, 0.0, 10, None, 0.0),       # W = 1: the search's rows are the training pass's rows
    (3, 17, 5, 32, 0.5, 10, None, 0.0),      # nrows 15 of R 16: exactly one padding row
    (2, 100, 8, 5, 0.5, 10, None, 0.0),      # nrows = R = 16: no padding row; L4 = 14
    (3, 17, 6, 5, 0.5, 10, (2, 0.3), 0.0),   # nrows 18 of R 32; an order-2 table at weight 0.3
    (2, 17, 3, 5, 0.5, 20, None, END_BIAS),  # ends early, in the middle of a chunk of eight steps
]
BEAM_KEYS = ('predicted_ids', 'scores', 'word_ids', 'parent_ids', 'log_probs', 'lengths', 'finished')


def train_id(c):
    T, B, U, C, p = c
    return f'train-T{T}B{B}U{U}C{C}p{p:g}'


def search_id(c):
    B, T, W, C, lp, steps, lm, bias = c
    return f'search-B{B}T{T}W{W}C{C}lp{lp:g}' + (f'-lm{lm[0]}' if lm else '') + ('-early' if bias else '')


def digest(x):
    """SHA-256 over the bytes of x: floats as float32(x + 0.0), everything else as int32"""
    a = np.asarray(x)
    if a.dtype.kind == 'f':
        a = a.astype(np.float32) + np.float32(0.0)
    else:
        a = a.astype(np.int32)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def noisy_params(tensors, seed):
    """LAS.initial_params plus seeded noise of 0.05 on every entry (tensors: (name, offset, rows, cols))"""
    from neuralasr_amd.networks.las import LAS
    flat = LAS.__new__(LAS).initial_params(tensors, seed=seed)
    return (flat + NOISE * np.random.RandomState(seed + 1).randn(flat.size)).astype(np.float32)


def _engine(C, p, seed):
    from neuralasr_amd.engine import LasEngine
    e = LasEngine(F, C, sampling_probability=p, seed=5, learning_rate=1e-3)
    e.set_params(noisy_params(e.tensors(), seed))
    return e


def run_train(case):
    """One loss_and_grads: (engine, record).  The caller closes the engine."""
    T, B, U, C, p = case
    rs = np.random.RandomState(1000 * T + 10 * B + U)
    feats = rs.randn(B, T, F).astype(np.float32)
    labels = rs.randint(0, C, size=(B, U)).astype(np.int32)
    label_len = rs.randint(0, U + 1, size=B).astype(np.int32)
    label_len[0] = U
    e = _engine(C, p, seed=T + B)
    loss, nll, grads = e.loss_and_grads(feats, np.full(B, T, np.int32), labels, label_len)
    rec = {'loss': digest(np.float32(loss)), 'nll': digest(nll), 'grads': digest(grads), 'logits': digest(e.logits()),
           'fed_ids': digest(e.fed_ids()), 'sampled': digest(e.sampled()),
           'loss_value': float(np.float32(loss)), 'grad_norm': float(np.linalg.norm(grads.astype(np.float64))),
           'samples': int(e.sampled().sum())}
    return e, rec


def search_inputs(case):
    """(features [B, T, F], table [K, C] or None) of a search case"""
    B, T, W, C, lp, steps, lm, bias = case
    rs = np.random.RandomState(1000 * B + 10 * T + W + C)
    feats = rs.randn(B, T, F).astype(np.float32)
    table = None
    if lm:
        x = rs.randn(C ** (lm[0] - 1), C) * 1.5
        table = (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)
    return feats, table


def add_end_bias(flat, tensors, end_id, bias):
    off = {n: o for n, o, _, _ in tensors}['projection_layer/bias']
    flat = flat.copy()
    flat[off + end_id] += np.float32(bias)
    return flat


def run_search(case):
    """One beam_search(..., trace=True) with start id 1 and end id C - 1: (engine, record).  The caller closes the engine."""
    B, T, W, C, lp, steps, lm, bias = case
    feats, table = search_inputs(case)
    e = _engine(C, 0.1, seed=B + T + W)
    if bias:
        e.set_params(add_end_bias(e.get_params(), e.tensors(), C - 1, bias))
    if lm:
        e.set_lm((table, lm[0]), lm[1])
    g = e.beam_search(feats, np.full(B, T, np.int32), W, steps, 1, C - 1, lp, trace=True)
    rec = {k: digest(g[k]) for k in BEAM_KEYS}
    rec['steps'] = int(g['steps'])
    rec['max_steps'] = steps
    rec['best'] = g['predicted_ids'][0, :, 0].tolist()
    rec['best_score'] = float(g['scores'][0, -1, 0])
    if lm:
        rec['lm_context'] = digest(e.lm_context(B, W))
    return e, rec


def main():
    sys.path.insert(0, ROOT)
    doc = {'_note': 'SHA-256 of LasEngine.loss_and_grads / logits / fed_ids / sampled and of beam_search(trace=True), taken on '
                    'an MI355X from the commit before the shared decoder step and attention kernel.  '
                    'tests/golden/make_las_parent_golden.py'}
    for c in TRAIN:
        e, rec = run_train(c)
        e.close()
        doc[train_id(c)] = rec
        print(train_id(c), rec['loss_value'], rec['grad_norm'], rec['samples'], rec['grads'][:16], flush=True)
    for c in SEARCH:
        e, rec = run_search(c)
        e.close()
        doc[search_id(c)] = rec
        print(search_id(c), rec['steps'], rec['best'], rec['best_score'], rec['scores'][:16], flush=True)
        if c[7]:   # the done word is raised inside a chunk: the chunk's remaining launches return at once
            assert rec['steps'] < c[5] and rec['steps'] % 8 != 0, rec['steps']
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
