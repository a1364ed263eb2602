"""Generates tests/golden/step_parent.json: SHA-256 digests of what the per-timestep recurrence kernels give when a whole
batch, or the windows of a chunked batch, are driven over them (tests/test_gpu_step_parent_bits.py runs the same cases and
compares).  Run it on an MI355X with the commit BEFORE a change to how the per-step launches are chained
(csrc/nasr_pass.hip: run_steps, lc_run_steps), to the step kernels' launchers or the carry kernels (csrc/lstm.hip) or to who
rebuilds the per-step operand images (csrc/nasr_rec.hip) is built (`python tests/golden/make_step_parent_golden.py`); a
change that claims to keep every bit is then measured against what that commit computed.  A mismatch is fixed in the code,
never by running this again.

Only data is written.  Per case, one engine: digests of the logits, the loss, the flat gradient, the loss of every
train_step and the parameters and Adam state after them (floats as float32(x + 0.0) bytes, so the sign of an exact zero
does not count), and in plain the recurrence mode and the recurrence launches of the last forward and backward pass.  Only
Engine's public calls are used; every input comes from a fixed numpy seed.  `python make_step_parent_golden.py OUT ID...`
runs only the cases named and merges them into OUT."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'step_parent.json')

F, C = 13, 5


def lc_lengths(T, Cf, R, B):
    """the pattern of tests/test_gpu_lc_train.py::lengths at T frames: T_b = T, <= C + R, = jC + R, = jC + R + 1 (none beyond
    T) and 2 frames; then random ones"""
    j = max(1, (T - R - 1) // Cf)
    lens = [T, min(Cf + R, T - 1), min(j * Cf + R, T), min(j * Cf + R + 1, T), 2]
    rs = np.random.RandomState(B)
    return (lens + [int(rs.randint(1, T + 1)) for _ in range(B - len(lens))])[:B]


# kind 'step': set_recurrence_mode(False), graph mode as given.  kind 'chunk': the handle's mode stays what create chose
# (the persistent kind where the device has it), chunking (C, R); two steps with set_params between them, then chunking
# off and one more step.
CASES = [
    dict(id='step-bi-H20x2-B5-T7', kind='step', H=20, L=2, B=5, T=7, bi=True, graph=False, lens=[7, 1, 4, 6, 3]),
    dict(id='step-bi-H20x2-B5-T7-graph', kind='step', H=20, L=2, B=5, T=7, bi=True, graph=True, lens=[7, 1, 4, 6, 3]),
    dict(id='step-uni-H70x2-B17-T7', kind='step', H=70, L=2, B=17, T=7, bi=False, graph=False,
         lens=[7, 1, 4, 6, 3, 2, 7, 5, 1, 3, 6, 4, 2, 7, 5, 3, 1]),
    dict(id='step-uni-H70x2-B17-T7-graph', kind='step', H=70, L=2, B=17, T=7, bi=False, graph=True,
         lens=[7, 1, 4, 6, 3, 2, 7, 5, 1, 3, 6, 4, 2, 7, 5, 3, 1]),
    dict(id='step-bi-H576-B2-T3', kind='step', H=576, L=1, B=2, T=3, bi=True, graph=False, lens=[3, 2]),   # NQ = 0, KSP = 0
    dict(id='chunk-c4r3-T23', kind='chunk', H=20, L=2, B=5, T=23, bi=True, C=4, R=3),
    dict(id='chunk-c1r2-T23', kind='chunk', H=20, L=2, B=5, T=23, bi=True, C=1, R=2),      # every window carries
    dict(id='chunk-c3r7-T23', kind='chunk', H=20, L=2, B=5, T=23, bi=True, C=3, R=7),      # R > C
    dict(id='chunk-c8r3-T6', kind='chunk', H=20, L=2, B=5, T=6, bi=True, C=8, R=3),        # W = T <= C: one window
    dict(id='chunk-c2r1-H640-T5', kind='chunk', H=640, L=1, B=2, T=5, bi=True, C=2, R=1),  # the two-launch wide BPTT, carried c0
]


def case_id(c):
    return c['id']


def digest(x):
    """SHA-256 over the bytes of x as float32(x + 0.0)"""
    a = np.asarray(x).astype(np.float32) + np.float32(0.0)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def params(e, seed):
    return (0.2 * np.random.RandomState(seed).randn(e.param_count)).astype(np.float32)


def batch(case):
    B, T = case['B'], case['T']
    rs = np.random.RandomState(7 + B + 10 * T)
    seq_len = np.asarray(case['lens'] if 'lens' in case else lc_lengths(T, case['C'], case['R'], B), np.int32)
    assert len(seq_len) == B and seq_len.max() == T and seq_len.min() >= 1
    feats = rs.randn(B, T, F).astype(np.float32)
    for b in range(B):
        feats[b, seq_len[b]:] = 0
    Lmax = 3
    labels = np.zeros((B, Lmax), np.int32)
    label_len = np.zeros(B, np.int32)
    for b in range(B):
        n = min(Lmax, max(1, int(seq_len[b]) // 3))
        labels[b, :n], label_len[b] = rs.permutation(C - 1)[:n], n     # distinct labels: feasible with n frames
    return feats, seq_len, labels, label_len


def launches(e):
    pt = e.phase_times()
    return [int(pt['rec_fwd_launches']), int(pt['rec_bwd_launches'])]


def run_case(case):
    """Runs the case on a fresh engine: the record that goes into the JSON"""
    from neuralasr_amd.engine import Engine
    e = Engine(F, case['H'], case['L'], case['bi'], 'concat' if case['bi'] else 'none', C, learning_rate=1e-3)
    chunk = case['kind'] == 'chunk'
    if not chunk:
        e.set_recurrence_mode(False)
        e.set_graph_mode(case['graph'])
    e.set_params(params(e, 11))
    n = e.param_count
    e.set_adam_state(np.zeros(n, np.float32), np.zeros(n, np.float32), 0)
    bt = batch(case)
    if chunk:
        e.set_chunking(case['C'], case['R'])
    rec = {'mode': e.recurrence_mode}
    logits = e.forward(bt[0], bt[1])
    loss, nll, grads = e.loss_and_grads(*bt)
    rec.update(logits=digest(logits), loss=digest(loss), nll=digest(nll), grads=digest(grads), launches_grads=launches(e),
               logits_abs_sum=float(np.abs(logits.astype(np.float64)).sum()), grads_abs_sum=float(np.abs(grads.astype(np.float64)).sum()))
    steps = [e.train_step(*bt)]
    if chunk:
        e.set_params(params(e, 12))                   # a resident kind in use: the per-step operand images are rebuilt
    steps.append(e.train_step(*bt))                   # (graph mode: replays the graphs the passes above captured)
    rec['launches_step'] = launches(e)
    if chunk:
        e.set_chunking(0)
        steps.append(e.train_step(*bt))
        rec['launches_whole'] = launches(e)
    m, v, t = e.get_adam_state()
    rec.update(steps=[digest(s) for s in steps], step_losses=[float(s) for s in steps], params=digest(e.get_params()),
               adam_m=digest(m), adam_v=digest(v), adam_step=int(t), mode_after=e.recurrence_mode)
    e.close()
    return rec


def main():
    sys.path.insert(0, ROOT)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    only = sys.argv[2:]
    doc = {}
    if only and os.path.exists(out):
        with open(out) as f:
            doc = json.load(f)
    doc['_note'] = ('SHA-256 of logits, loss, gradient, step losses, parameters and Adam state of per-step and chunked training '
                    'steps, taken on an MI355X from the commit before the per-step launch loops became one window runner.  '
                    'tests/golden/make_step_parent_golden.py')
    for c in CASES:
        if only and case_id(c) not in only:
            continue
        rec = run_case(c)
        doc[case_id(c)] = rec
        print(case_id(c), rec['mode'], 'launches', rec['launches_grads'], rec['launches_step'], rec.get('launches_whole'),
              'sum|logits|', rec['logits_abs_sum'], 'sum|grads|', rec['grads_abs_sum'], 'losses', rec['step_losses'],
              rec['logits'][:16], rec['grads'][:16], rec['params'][:16], flush=True)
        with open(out, 'w') as f:                     # after every case: what ran is kept whatever the next one does
            json.dump(doc, f, indent=1)
            f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
