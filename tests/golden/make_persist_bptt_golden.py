"""Generates tests/golden/persist_bptt_parent.json: SHA-256 digests of loss, nll and the flat gradient that
Engine.loss_and_grads gives in persistent mode for the cases below (tests/test_gpu_persist_bptt_exchange.py runs the same
cases and compares).  Run it on an MI355X with the commit BEFORE a change to lstm_persist_bwd_kernel built
(`python tests/golden/make_persist_bptt_golden.py`); a change that claims to keep every bit is then measured against
what that commit computed.  A mismatch is fixed in the kernel, never by running this again.

Only data is written: digests, and a few plain numbers (loss, gradient norm) that tell a reader of a failing test how far
apart the two results are in value."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'persist_bptt_parent.json')

# (feature_size, hidden, layers, bidirectional, merge, classes), B, T        Hp   NU  what it adds
CASES = [
    ((14, 50, 1, True, 'stack_reshape', 8), 5, 13),     # 64   2   utterance slots partly filled (ub 2, one slice 1 of 2)
    ((13, 128, 1, False, 'none', 6), 1, 9),             # 128  4   one utterance: seven of eight groups idle
    ((11, 180, 2, False, 'none', 6), 16, 17),           # 192  6   two layers; a partly filled 16-byte row set (H 180 of 192)
    ((20, 250, 1, True, 'concat', 11), 19, 12),         # 256  8   19 bidirectional: two rounds, the second partly filled
    ((15, 300, 1, True, 'concat', 8), 16, 24),          # 320  10  full slots (4 per group); H 300 of 320
    ((12, 380, 1, False, 'none', 7), 40, 11),           # 384  12  40 unidirectional: two rounds of 8 x 4 (the flag barrier)
    ((16, 440, 1, True, 'stack_reshape', 9), 5, 15),    # 448  14
    ((18, 500, 1, True, 'stack_reshape', 10), 16, 21),  # 512  16  the flagship width, full slots
    ((12, 500, 1, False, 'none', 7), 40, 10),           # 512  16  two rounds at the flagship width
]


def case_id(c):
    s, B, T = c
    return f"H{s[1]}L{s[2]}{'bi' if s[3] else 'uni'}-B{B}T{T}"


def make_inputs(case):
    """(spec, params, feats, seq_len, labels, label_len): ragged lengths, one utterance of about T/3 (many masked
    timesteps, and the first valid BPTT timestep of that utterance far into the launch)."""
    from oracle import nasr_oracle as O
    s, B, T = case
    spec = O.ModelSpec(*s)
    feats, seq_len, labels, label_len = O.synth_batch(spec, B, T, seed=7 * B + T, var_len=True, Lmin=1, Lmax=max(1, T // 5))
    seq_len[0] = max(int(label_len[0]) * 2 + 1, T // 3)
    feats[0, seq_len[0]:] = 0.0
    rs = np.random.RandomState(5)
    params = [p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=5)]
    return spec, params, feats, seq_len, labels, label_len


def digest(x):
    """SHA-256 over the float32 bytes of x + 0.0: the sign of an exact zero does not count."""
    a = np.ascontiguousarray(np.asarray(x, np.float32) + np.float32(0.0))
    return hashlib.sha256(a.tobytes()).hexdigest()


def run_case(case):
    """One persistent-mode loss_and_grads: (engine, loss, nll, grads).  The caller closes the engine."""
    from oracle import nasr_oracle as O
    from neuralasr_amd.engine import Engine
    spec, params, feats, seq_len, labels, label_len = make_inputs(case)
    e = Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes,
               forget_bias=spec.forget_bias, learning_rate=1e-3)
    assert e.recurrence_mode == 'persistent'
    e.set_params(O.flatten(params))
    loss, nll, grads = e.loss_and_grads(feats, seq_len, labels, label_len)
    return e, (feats, seq_len, labels, label_len), loss, nll, grads


def record(loss, nll, grads):
    return {'loss': digest(np.float32(loss)), 'nll': digest(nll), 'grads': digest(grads),
            'loss_value': float(np.float32(loss)), 'grad_norm': float(np.linalg.norm(grads.astype(np.float64)))}


def main():
    sys.path.insert(0, ROOT)
    doc = {'_note': 'SHA-256 of float32(x + 0.0) bytes of Engine.loss_and_grads in persistent mode, taken on an MI355X from the '
                    'commit before the 16-byte exchange loads of lstm_persist_bwd_kernel.  tests/golden/make_persist_bptt_golden.py'}
    for c in CASES:
        e, _, loss, nll, grads = run_case(c)
        assert e.persist_stats()[0] == 0
        e.close()
        doc[case_id(c)] = record(loss, nll, grads)
        print(case_id(c), doc[case_id(c)]['loss_value'], doc[case_id(c)]['grads'][:16], flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out)


if __name__ == '__main__':
    main()
