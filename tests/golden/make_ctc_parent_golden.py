"""Generates tests/golden/ctc_parent.json: SHA-256 digests of what every instantiation of the CTC kernels of csrc/ctc.hip
computes - the alpha / beta walks of the engineered and of the plain lattice with the gradient kernel behind them, and the
forced alignment on both back-pointer routes (tests/test_gpu_ctc_parent_bits.py runs the same cases and compares).  Run it
on an MI355X with the commit BEFORE a change to csrc/ctc.hip is built (`python tests/golden/make_ctc_parent_golden.py`); a
change that claims to keep every bit is then measured against what that commit computed.  A mismatch is fixed in the code,
never by running this again.

Only digests are written.  Loss cases: the batch, the parameters and the engine of tests/test_gpu_ctc_lattice.py (B 4: a
label that fills the width, a short one, an empty one and a pinned one; an H 16 one-layer network), one label-array width per
instantiation, C 29 (engineered lattice) and C 40 (plain), and the projection scaled by 60 at the widths 224 and 511, where
paths die and the column rescale meets NEG; the loss, the per-utterance nll, the flat gradient (floats as float32(x + 0.0)
bytes, so the sign of an exact zero does not count) and the greedy ids.  Alignment cases: Engine.align_logits on seeded
logits, integer-valued and float, every instantiation with its back-pointers in LDS and in the global workspace
(Engine.align_in_lds says which, and the case asserts it; KS 12 and 16 reach LDS only with a label array wider than its
labels and F <= 225); the paths (int32) and the fp64 scores (float64 bytes).  Every case is run twice, each on a fresh
engine, and one whose two records differ is not recorded.
`python make_ctc_parent_golden.py OUT ID...` runs only the cases named and merges them into OUT."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'ctc_parent.json')

WIDTHS = {31: 2, 64: 3, 96: 4, 128: 5, 160: 6, 192: 7, 224: 8, 256: 12, 511: 16}     # label-array width -> KS
KERNEL_C = {'fast': 29, 'plain': 40}
# the longest utterance whose back-pointers stay in LDS: 56 KB of 1 / 2 / 4 words per lane and group of 4 frames
ALIGN_LDS_FRAMES = {2: 897, 3: 897, 4: 897, 5: 449, 6: 449, 7: 449, 8: 449, 12: 225, 16: 225}

LOSS_CASES = [dict(id='loss-Lmax%d-%s%s' % (Lmax, kind, '-sharp' if scale != 1.0 else ''), Lmax=Lmax, kernel=kind, scale=scale)
              for Lmax in WIDTHS for kind in KERNEL_C for scale in ((1.0, 60.0) if Lmax in (224, 511) else (1.0,))]
ALIGN_CASES = [dict(id='align-Lmax%d-%s-%s' % (Lmax, route, kind), Lmax=Lmax, route=route, kind=kind)
               for Lmax in WIDTHS for route in ('lds', 'global') for kind in ('int', 'float')]
CASES = LOSS_CASES + ALIGN_CASES


def case_id(c):
    return c['id']


def digest(x, dtype=np.float32):
    """SHA-256 over the bytes of x as dtype(x + 0.0) (float32 unless said otherwise)"""
    a = np.asarray(x).astype(dtype) + dtype(0)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_loss_case(case):
    import test_gpu_ctc_lattice as L
    from oracle import nasr_oracle as O
    Lmax, C = case['Lmax'], KERNEL_C[case['kernel']]
    assert L.ks_of(Lmax) == WIDTHS[Lmax]
    spec = O.ModelSpec(5, 16, 1, True, 'concat', C)
    sharp = case['scale'] != 1.0
    batch = L.lattice_batch(C, Lmax, seed=Lmax * 7 + C + (1 if sharp else 0))
    e = L.engine_for(spec)
    e.set_params(O.flatten(L.net_params(spec, Lmax, scale=case['scale'])))
    loss, nll, grads = e.loss_and_grads(*batch)
    ids = e.greedy_decode(batch[0], batch[1])
    e.close()
    assert np.isfinite(loss) and np.isfinite(grads).all()
    return dict(loss=digest(loss), nll=digest(nll), grads=digest(grads), greedy_lens=digest([len(h) for h in ids], np.int32),
                greedy_ids=digest([i for h in ids for i in h], np.int32))


def align_label(rs, L, C, runs):
    lab = rs.randint(0, C - 1, size=L)
    for i in rs.permutation(max(L - 1, 0))[:runs]:
        lab[i + 1] = lab[i]
    return lab.astype(np.int32)


def needed(lab):
    return len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def align_batch(case):
    """B 3 on a label array of width Lmax: the longest label the frames allow with runs of repeats, a short one on fewer
    frames, an empty one on a handful of frames.  -> logits [T',B,C], seq_len, labels (padding = class ids), label_len"""
    Lmax, KS, C = case['Lmax'], WIDTHS[case['Lmax']], 29
    lds = case['route'] == 'lds'
    rs = np.random.RandomState(1000 + 2 * Lmax + (1 if lds else 0) + (7 if case['kind'] == 'float' else 0))
    if lds:
        F = ALIGN_LDS_FRAMES[KS] if KS >= 12 else min(ALIGN_LDS_FRAMES[KS], 2 * Lmax + 90)
    else:
        F = max(ALIGN_LDS_FRAMES[KS] + 3, min(1100, 2 * Lmax + 78))
    Lfull = min(Lmax, (F * 4) // 9) if lds else Lmax  # the KS 12 / 16 LDS cases: labels far narrower than their array
    full = align_label(rs, Lfull, C, Lfull // 8)
    short = align_label(rs, max(1, Lfull // 5), C, 2)
    utts = [(F, full), (F - 37, short), (6, np.zeros(0, np.int32))]
    assert all(needed(l) <= f for f, l in utts)
    Tp = F + 3
    if case['kind'] == 'int':
        logits = rs.randint(-8, 9, size=(Tp, 3, C)).astype(np.float32)
    else:
        logits = (3.0 * rs.randn(Tp, 3, C)).astype(np.float32)
    labels = rs.randint(0, C - 1, size=(3, Lmax)).astype(np.int32)
    for b, (_, l) in enumerate(utts):
        labels[b, :len(l)] = l
    return logits, [f for f, _ in utts], labels, [len(l) for _, l in utts]


def run_align_case(case):
    from neuralasr_amd.engine import Engine
    logits, seq, labels, ll = align_batch(case)
    e = Engine(8, 16, 1, False, 'none', 5)
    assert e.align_in_lds(max(seq), labels.shape[1]) == (case['route'] == 'lds')
    path, score = e.align_logits(logits, seq, labels, ll)
    e.close()
    assert np.isfinite(score).all() and all(path[b, seq[b] - 1] >= 2 * ll[b] - 1 for b in range(3))
    return dict(path=digest(path, np.int32), score=digest(score, np.float64))


def run_case(case):
    """Runs the case on a fresh engine: the record that goes into the JSON"""
    return run_align_case(case) if 'route' in case else run_loss_case(case)


def main():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    only = sys.argv[2:]
    doc = {}
    if only and os.path.exists(out):
        with open(out) as f:
            doc = json.load(f)
    doc['_note'] = ('SHA-256 of loss, nll, gradient and greedy ids of every CTC lattice instantiation (engineered and plain), and of '
                    'the paths and fp64 scores of every alignment instantiation on both back-pointer routes, taken on an MI355X from '
                    'the commit before ctc.hip\'s four walks came to share one lattice set-up, step and rescale.  '
                    'tests/golden/make_ctc_parent_golden.py')
    refused = []
    for c in CASES:
        if only and case_id(c) not in only:
            continue
        rec, again = run_case(c), run_case(c)
        if rec != again:
            print(case_id(c), 'NOT RECORDED: two runs differ in', sorted(k for k in rec if rec[k] != again[k]), flush=True)
            refused.append(case_id(c))
            doc.pop(case_id(c), None)
            continue
        doc[case_id(c)] = rec
        print(case_id(c), {k: v[:12] for k, v in rec.items()}, flush=True)
        with open(out, 'w') as f:                     # after every case: what ran is kept whatever the next one does
            json.dump(doc, f, indent=1)
            f.write('\n')
    print('wrote', out, 'refused', refused)
    return 1 if refused else 0


if __name__ == '__main__':
    sys.exit(main())
