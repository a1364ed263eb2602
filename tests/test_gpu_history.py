"""GPU: a handle's results do not depend on what it ran before ("What a handle carries between calls").

Every handle family - the (Bi)LSTM CTC Engine in its three merge forms, at widths with and without a resident recurrence,
a DeepSpeech-shaped Engine, WaveNetEngine, LasEngine and the featurizer - runs each history of tests/history_ref.py that
its features allow, in two variants (other seeds, features x1 and x8) on two handles.  Then every piece of carried state
is reset through the public API and one fixed small batch goes through every output the family has.  The two variants and
a fresh handle must give those outputs bit for bit: a result that reads a workspace byte it did not write in this call
cannot equal both.  No resident recurrence may have aborted along the way.

Bitwise agreement alone would pass if all three were wrong alike: once per family the fresh handle's probe outputs are
held to the family's fp64 reference, with the tolerances its own test file applies at its small shapes."""
import types

import numpy as np
import pytest

import history_ref as H
import test_gpu_deepspeech as TD
import test_gpu_edges as TE
import test_gpu_wavenet as TW
from oracle import nasr_oracle as O

pytestmark = pytest.mark.gpu

_fresh = {}


def fresh_probe(name):
    """the probe outputs of a handle that has run nothing else: once per family, never changed afterwards"""
    if name not in _fresh:
        f = H.family(name)
        e = f.make()
        out = f.probe(e)
        assert e.persist_stats()[0] == 0
        e.close()
        for v in out.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _fresh[name] = out
    return _fresh[name]


@pytest.mark.parametrize('name,history', H.CASES, ids=['%s-%s' % c for c in H.CASES])
def test_probe_after_history_equals_fresh(name, history):
    f = H.family(name)
    want = fresh_probe(name)
    teacher = f.make() if history == 'distill' else None
    try:
        for variant in H.VARIANTS:
            e = f.make()
            try:
                H.run_history(f, e, history, variant, teacher)
                assert e.persist_stats()[0] == 0, 'a resident recurrence aborted during the history'
                got = f.probe(e)
                assert e.persist_stats()[0] == 0, 'a resident recurrence aborted during the probe'
                H.assert_same(got, want, '%s after %s, variant %d' % (name, history, variant))
            finally:
                e.close()
    finally:
        if teacher is not None:
            teacher.close()


# ------------------------------------------------------------------------------------------------ the anchors
def rel(a, b):
    return np.linalg.norm(np.asarray(a, np.float64) - b) / max(np.linalg.norm(b), 1e-30)


@pytest.mark.parametrize('name', [n for n in H.TABLE if H.TABLE[n] and n not in ('wavenet', 'las')])
def test_fresh_lstm_probe_against_the_oracle(name):
    """loss, nll, every gradient tensor and the logits against oracle.nasr_oracle: the tolerances of
    tests/test_gpu_edges.py's check (its TOL_ constants) and, tensor by tensor, the rule of tests/test_gpu_deepspeech.py
    (TOL_TENSOR of the tensor's norm + TOL_TENSOR_FLOOR of the whole gradient's).  The logits are those of the parameters
    the probe's two steps left, which the oracle is given."""
    f = H.family(name)
    out = fresh_probe(name)
    spec = f.spec
    feats, seq, labels, ll = f.probe_batch()
    lo, nllo, go, _ = O.network_loss_and_grads(spec, O.unflatten(spec, f.p0.astype(np.float64)), feats, seq, labels, ll,
                                               drop=f.drop)
    print(name, 'loss rel', abs(out['loss'] - lo) / abs(lo), 'grad rel', rel(out['grads'], O.flatten(go)))
    assert out['loss'] == pytest.approx(lo, rel=TE.TOL_LOSS)
    if not f.drop:
        assert out['train'][0] == pytest.approx(lo, rel=TE.TOL_LOSS)                # the first step sees the same parameters
    np.testing.assert_allclose(out['nll'], nllo, rtol=TE.TOL_LOSS, atol=TE.TOL_NLL_ABS)
    assert rel(out['grads'], O.flatten(go)) < TE.TOL_GRAD
    scale, off = np.linalg.norm(O.flatten(go)), 0
    for (tname, shp), g_o in zip(spec.param_shapes(), go):
        g = out['grads'][off:off + g_o.size].reshape(g_o.shape)
        off += g_o.size
        err = np.linalg.norm(g - g_o)
        print('   ', tname, err / max(np.linalg.norm(g_o), 1e-30))
        assert err <= TD.TOL_TENSOR * np.linalg.norm(g_o) + TD.TOL_TENSOR_FLOOR * scale, tname
    drop = (out['drop_state'][0], out['drop_state'][1]) if f.drop else None
    logits_o, _ = O.network_forward(spec, O.unflatten(spec, out['params'].astype(np.float64)), feats, seq, drop=drop)
    np.testing.assert_allclose(out['logits'], logits_o, atol=TE.TOL_LOGITS)
    if f.drop:      # the decoder's own forward pass drew the next masks
        lg, _ = O.network_forward(spec, O.unflatten(spec, out['params'].astype(np.float64)), feats, seq, drop=(drop[0], drop[1] + 1))
        assert out['greedy'] == O.greedy_decode(lg, seq)
    else:
        assert out['greedy'] == O.greedy_decode(out['logits'].astype(np.float64), seq)
    assert out['adam_step'] == 2 and out['mode'] == ('persistent' if f.persistent else 'per-step')


def test_fresh_wavenet_probe_against_torch():
    """tests/test_gpu_wavenet.py's check_pass on the probe's outputs, with its small-shape tolerances"""
    f = H.family('wavenet')
    out = fresh_probe('wavenet')
    W, spec = f.W, f.spec
    feats, seq, labels, ll = f.probe_batch()
    loss_r, g_r, stats = W.loss_and_grads(spec, f.p0, feats, seq, labels, ll)
    assert abs(out['loss'] - loss_r) <= TW.TOL_LOSS * abs(loss_r), (out['loss'], loss_r)
    layout, off = [], 0
    for tname, r, c in W.tensor_specs(spec):
        layout.append((tname, off, r, c))
        off += r * c
    errs = TW.grad_errors(spec, types.SimpleNamespace(tensors=lambda: layout), out['grads'], g_r)
    worst = max(errs, key=errs.get)
    assert errs[worst] <= TW.TOL_GRAD, (worst, errs[worst])
    m_r, v_r = W.update_variance(spec, stats)
    assert TW.rel(out['batch_var'], v_r) <= TW.TOL_GRAD
    assert np.abs(out['batch_mean'] - m_r).max() <= TW.TOL_GRAD * (np.abs(m_r).max() + 1)
    # inference with the moving statistics and the parameters that the probe's two steps left
    mm, mv, _, n = out['bn']
    assert n == out['bn_after_grads'][3] + 2 and out['adam_step'] == 2      # one update per training step
    _, _, lg_r = W.eval_loss(spec, out['params'], feats, seq, labels, ll, (mm, mv))
    for b in range(len(seq)):
        assert TW.rel(out['logits'][:seq[b], b], lg_r[:seq[b], b]) < TW.TOL_GRAD
    assert out['greedy'] == W.greedy(lg_r, seq)


def test_fresh_las_probe_against_torch():
    """tests/test_gpu_las.py's _pass and _assert_per_tensor with the GPU's fed ids replayed, as its trained-like regime
    cases run them: loss, logits and every gradient tensor within what the same model costs in torch fp32
    (las_ref.tolerances)"""
    import torch
    f = H.family('las')
    out = fresh_probe('las')
    R = f.R
    feats, seq, labels, ll = f.probe_batch()
    ref = R.loss_and_grads(f.p0, f.F, f.C, feats, labels, ll, out['fed'])
    ref32 = R.loss_and_grads(f.p0, f.F, f.C, feats, labels, ll, out['fed'], dtype=torch.float32)
    tol, e32 = R.tolerances(ref, ref32, f.F, f.C)
    el = abs(out['loss'] - ref[0]) / max(abs(ref[0]), 1e-30)
    eg = np.max(np.abs(out['grads'] - ref[2])) / max(np.max(np.abs(ref[2])), 1e-30)
    elog = np.max(np.abs(out['logits'] - ref[1]))
    errs = R.per_tensor_errors(out['grads'], ref[2], f.F, f.C)
    worst = max(errs, key=errs.get)
    print('LAS probe: loss rel %.2e, grad rel-to-max %.2e, logits abs %.2e, worst tensor %.2e %s (tol %.1e)'
          % (el, eg, elog, errs[worst], worst, tol['grad']))
    assert (out['fed'][:, 0] == labels[:, 0]).all()
    assert errs[worst] <= tol['grad'], (worst, errs[worst], tol['grad'])
    assert el <= tol['loss'] and R.rel_norm(out['logits'], ref[1]) <= tol['logits']
    assert np.isfinite(out['grads']).all() and np.isfinite(out['logits']).all()
    p, seed, counter, tower = out['sampling']
    assert (p, seed, tower) == (pytest.approx(f.SAMPLING[0]), f.SAMPLING[1], 0) and counter > f.SAMPLING[2]


# ------------------------------------------------------------------------------------------------ the featurizer
def test_featurizer_after_history_equals_fresh():
    """noise and RIR banks set and cleared, an augmentation and a resampling call, longer and shorter utterances: the
    features of a fixed clip are then what a fresh featurizer gives, bit for bit"""
    from neuralasr_amd.features import Featurizer

    def make():
        return Featurizer(H.FZ_RATE, H.FZ_CEP, H.FZ_CTX)
    fz = make()
    want = H.featurizer_probe(fz)
    fz.close()
    assert np.isfinite(want['feats']).all() and want['feats'].shape[1] == (2 * H.FZ_CTX + 1) * H.FZ_CEP
    for variant in H.VARIANTS:
        fz = make()
        try:
            H.featurizer_history(fz, variant)
            H.assert_same(H.featurizer_probe(fz), want, 'featurizer, variant %d' % variant)
        finally:
            fz.close()
