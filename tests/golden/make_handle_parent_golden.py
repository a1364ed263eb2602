"""Generates tests/golden/handle_parent.json: SHA-256 digests of what the handle computes on the paths that the other parent
fixtures (step, stream, LAS, front end, plane GEMM, persistent BPTT) do not reach (tests/test_gpu_handle_parent_bits.py runs
the same cases and compares).  Run it on an MI355X with the commit BEFORE a change to where the handle keeps its state or to
how the host side orders its work (csrc/nasr_ctx.h, nasr_lstm.h and the nasr_*.hip files) is built
(`python tests/golden/make_handle_parent_golden.py`); a change that claims to keep every bit is then measured against what
that commit computed.  A mismatch is fixed in the code, never by running this again.

Only data is written.  Per case, one engine: digests of the logits, the loss, the per-utterance nll and the flat gradient,
of the parameters and Adam state after two train_steps (floats as float32(x + 0.0) bytes, so the sign of an exact zero does
not count), and in plain the recurrence mode and the recurrence launches of a forward and backward pass; per case what it
is about (below).  Only Engine's public calls are used; every input comes from a fixed numpy seed.  Every case is run twice,
each on a fresh engine, and one whose two records differ is not recorded.
`python make_handle_parent_golden.py OUT ID...` runs only the cases named and merges them into OUT."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, 'handle_parent.json')

C = 5
LENS17 = [7, 1, 4, 6, 3, 2, 7, 5, 1, 3, 6, 4, 2, 7, 5, 3, 1]

# net 'lstm' (Engine) or 'wavenet' (WaveNetEngine); `do`: what the case runs beyond the common record (run_case)
CASES = [
    # the persistent kind at Hp = 512 with more than one layer: the weight-gradient side stream and the deferred buckets
    dict(id='persist-bi-H500x2-B3-T6-sidestream', H=500, L=2, bi=True, B=3, T=6, lens=[6, 2, 5], do='sidestream'),
    dict(id='persist-uni-H70x2-B17-T7', H=70, L=2, bi=False, B=17, T=7, lens=LENS17),
    dict(id='compact-bi-H20x2-B5-T20', H=20, L=2, bi=True, B=5, T=20, lens=[20, 3, 2, 1, 5], do='compaction'),
    dict(id='literal-bi-H20-B5-T7', H=20, L=1, bi=True, merge='stack_reshape', B=5, T=7, lens=[7, 1, 4, 6, 3]),
    dict(id='deepspeech-H20-B4-T6', H=20, L=1, bi=True, B=4, T=6, lens=[6, 1, 4, 3], pre=(24, 24, 24), post=24,
         dropout=(0.1, 0.1, 0.1, 0.1), do='dropout'),
    dict(id='wide-bi-H2048-F10-B2-T3', H=2048, L=1, bi=True, F=10, B=2, T=3, lens=[3, 2]),
    dict(id='wavenet-1x(1,2)-B3-T9', net='wavenet', B=3, T=9, lens=[9, 4, 7], do='bn'),
    dict(id='staged-bi-H20x2-B5-T7', H=20, L=2, bi=True, B=5, T=7, lens=[7, 1, 4, 6, 3], do='staged'),
    dict(id='clip-bi-H20x2-B5-T7', H=20, L=2, bi=True, B=5, T=7, lens=[7, 1, 4, 6, 3], do='clip'),
    dict(id='align-bi-H20x2-B5-T7', H=20, L=2, bi=True, B=5, T=7, lens=[7, 1, 4, 6, 3], do='align'),
]


def case_id(c):
    return c['id']


def digest(x, dtype=np.float32):
    """SHA-256 over the bytes of x as dtype(x + 0.0) (float32 unless said otherwise)"""
    a = np.asarray(x).astype(dtype) + dtype(0)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def params(e, seed):
    return (0.2 * np.random.RandomState(seed).randn(e.param_count)).astype(np.float32)


def batch(case):
    B, T, F = case['B'], case['T'], case.get('F', 13)
    rs = np.random.RandomState(7 + B + 10 * T)
    seq_len = np.asarray(case['lens'], np.int32)
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


def make_engine(case):
    from neuralasr_amd.engine import Engine, WaveNetEngine
    if case.get('net') == 'wavenet':
        return WaveNetEngine(13, C, num_blocks=1, rates=(1, 2), learning_rate=1e-3)
    merge = case.get('merge', 'concat' if case['bi'] else 'none')
    return Engine(case.get('F', 13), case['H'], case['L'], case['bi'], merge, C, learning_rate=1e-3,
                  pre=case.get('pre', ()), post=case.get('post', 0), dropout=case.get('dropout', ()))


def grads_record(e, bt):
    """One gradient pass over a fresh upload: its digests, its recurrence launches and the rows it covered"""
    loss, nll, grads = e.loss_and_grads(*bt)
    return dict(loss=digest(loss), nll=digest(nll), grads=digest(grads), launches=launches(e), rows=int(e.resident_rows()),
                grads_abs_sum=float(np.abs(grads.astype(np.float64)).sum()))


def call(fn, *a):
    """What a setter answers: 'ok', or the library's message"""
    from neuralasr_amd import _lib
    try:
        fn(*a)
        return 'ok'
    except _lib.NasrError as err:
        return str(err)


def run_case(case):
    """Runs the case on a fresh engine: the record that goes into the JSON"""
    e = make_engine(case)
    do = case.get('do')
    wavenet = case.get('net') == 'wavenet'
    e.set_params(params(e, 11))
    n = e.param_count
    e.set_adam_state(np.zeros(n, np.float32), np.zeros(n, np.float32), 0)
    bt = batch(case)
    B, T = case['B'], case['T']
    rec = {'mode': 'none' if wavenet else e.recurrence_mode}
    if do == 'dropout':
        e.set_dropout_state(4567, 0)
    logits = e.forward(bt[0], bt[1])
    rec.update(logits=digest(logits), logits_abs_sum=float(np.abs(logits.astype(np.float64)).sum()))
    rec.update(grads_record(e, bt))

    if do == 'sidestream':
        # the weight gradients beside the BPTT of the layer below, on and off; the deferred bucket events, on and off
        rec['overlap_at_create'] = bool(e.wgrad_overlap)
        var = {}
        for name, fn, on in (('overlap-on', e.set_wgrad_overlap, True), ('overlap-off', e.set_wgrad_overlap, False),
                             ('defer-on', e.set_bucket_defer, True), ('defer-off', e.set_bucket_defer, False)):
            var[name] = dict(answer=call(fn, on), overlap=bool(e.wgrad_overlap), **grads_record(e, bt))
        rec['variants'] = var
        rec['overlap_back_on'] = call(e.set_wgrad_overlap, True)     # the two steps below: overlap on, events not deferred
        rec['persist_stats'] = list(e.persist_stats())
    elif do == 'compaction':
        var = {}
        for own in (True, False):
            if not own:
                e.set_recurrence_mode(False)
            for on in (True, False):
                e.set_row_compaction(on)
                var['%s-compaction-%s' % ('own' if own else 'step', 'on' if on else 'off')] = dict(
                    mode=e.recurrence_mode, **grads_record(e, bt))
        rec['variants'] = var
        e.set_row_compaction(True)                                   # the two steps below: per-step kernels, compacted rows
    elif do == 'staged':
        e.set_step_decode(True, logits=True)
        ticket = e.stage_batch(*bt)
        assert ticket is not None
        e.commit_batch(ticket)
        e.compute_grads()
        loss, fault, hyps = e.step_results(B, T)
        rec['staged'] = dict(loss=digest(loss), fault=bool(fault), hyps=[[int(i) for i in hy] for hy in hyps],
                             step_logits=digest(e.step_logits(B, T)), grads=digest(e.get_grads()),
                             decoded=[[int(i) for i in hy] for hy in e.get_decoded(B, T)])
        e.apply_adam()
        rec['staged']['void'] = bool(e.settle_step())
    elif do == 'clip':
        e.set_grad_clip(0.5)
    elif do == 'align':
        path, score = e.align(*bt)
        rec['align'] = dict(path=digest(path, np.int32), score=digest(score, np.float64), path_rows=[[int(i) for i in r] for r in path])

    steps = [e.train_step(*bt), e.train_step(*bt)]
    rec['launches_step'] = launches(e)
    m, v, t = e.get_adam_state()
    rec.update(steps=[digest(s) for s in steps], step_losses=[float(s) for s in steps], params=digest(e.get_params()),
               adam_m=digest(m), adam_v=digest(v), adam_step=int(t), mode_after='none' if wavenet else e.recurrence_mode)
    if do == 'dropout':
        rec['dropout_state'] = list(e.dropout_state())
    elif do == 'bn':
        mm, mv, bs, cnt = e.bn_state()
        rec['bn'] = dict(moving_mean=digest(mm), moving_var=digest(mv), biased=digest(bs), updates=int(cnt))
    elif do == 'clip':
        st = e.grad_clip_stats()
        rec['clip'] = dict(threshold=e.grad_clip, last_norm=digest(st['last_norm'], np.float64), last_coef=digest(st['last_coef']),
                           steps=int(st['steps']), clipped=int(st['clipped']), skipped=int(st['skipped']))
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
    doc['_note'] = ('SHA-256 of logits, loss, nll, gradient, step losses, parameters and Adam state on the handle\'s paths that the '
                    'other parent fixtures do not reach, taken on an MI355X from the commit before the LSTM family\'s state moved out '
                    'of nasr_ctx into LstmState.  tests/golden/make_handle_parent_golden.py')
    refused = []
    for c in CASES:
        if only and case_id(c) not in only:
            continue
        rec, again = run_case(c), run_case(c)
        if rec != again:
            diff = sorted(k for k in set(rec) | set(again) if rec.get(k) != again.get(k))
            print(case_id(c), 'NOT RECORDED: two runs differ in', diff, flush=True)
            for k in diff:
                print('  ', k, rec.get(k), '|', again.get(k), flush=True)
            refused.append(case_id(c))
            doc.pop(case_id(c), None)
            continue
        doc[case_id(c)] = rec
        print(case_id(c), rec['mode'], 'launches', rec['launches'], rec['launches_step'], 'rows', rec['rows'], 'sum|logits|',
              rec['logits_abs_sum'], 'sum|grads|', rec['grads_abs_sum'], 'losses', rec['step_losses'],
              {k: (v.get('answer'), v['launches'], v['rows'], v['grads'][:12]) for k, v in rec.get('variants', {}).items()},
              rec['logits'][:16], rec['grads'][:16], rec['params'][:16], flush=True)
        with open(out, 'w') as f:                     # after every case: what ran is kept whatever the next one does
            json.dump(doc, f, indent=1)
            f.write('\n')
    print('wrote', out, 'refused', refused)
    return 1 if refused else 0


if __name__ == '__main__':
    sys.exit(main())
