"""The LAS network on the GPU against the fp64 torch model of tests/las_ref.py: logits, sequence loss and every gradient
(scheduled sampling off, then with the GPU's fed ids replayed), the sampling draws against the hash, Adam and determinism.
Every gradient tensor is also measured against its own norm (las_ref.per_tensor_errors), from initial_params and in two
trained-like regimes with peaked attention, at the batch sizes and class counts where the kernels change path; the
tolerance of that metric is what the same model costs in torch fp32 on the same batch (las_ref.tolerances).
Measured errors are printed (pytest -s) and recorded in DESIGN.md §10."""
import numpy as np
import pytest

from tests import las_ref

pytestmark = pytest.mark.gpu

C = 12


def _engine(F, p=0.0, lr=1e-3, classes=None, flat=None):
    """classes: C unless given; flat: the parameters, initial_params(seed=3) unless given"""
    from neuralasr_amd.engine import LasEngine
    from neuralasr_amd.networks.las import LAS
    e = LasEngine(F, classes or C, sampling_probability=p, seed=5, learning_rate=lr)
    net = LAS.__new__(LAS)
    e.set_params(net.initial_params(e.tensors(), seed=3) if flat is None else flat)
    return e


def _batch(B, T, F, U, rs, empty=False):
    return las_ref.make_batch(B, T, F, U, C, rs, empty)


def _pass(e, F, feats, seq, labels, ll, classes=None, p32=True):
    """One loss_and_grads call against the fp64 model with the GPU's fed ids replayed.  el / eg / elog: loss relative,
    gradient relative to the largest entry of the whole gradient, logits absolute.  p32: the same batch through the fp32
    model too, for the tolerances (las_ref.tolerances) of the loss, the logits (rel_norm) and the per-tensor metric."""
    import torch
    Cn = classes or C
    loss, nll, g = e.loss_and_grads(feats, seq, labels, ll)
    r = {'loss': loss, 'g': g, 'logits': e.logits(), 'fed': e.fed_ids()}
    ref = las_ref.loss_and_grads(e.get_params(), F, Cn, feats, labels, ll, r['fed'])
    r['el'] = abs(loss - ref[0]) / max(abs(ref[0]), 1e-30)
    r['eg'] = np.max(np.abs(g - ref[2])) / max(np.max(np.abs(ref[2])), 1e-30)
    r['elog'] = np.max(np.abs(r['logits'] - ref[1]))
    if p32:
        ref32 = las_ref.loss_and_grads(e.get_params(), F, Cn, feats, labels, ll, r['fed'], dtype=torch.float32)
        r['tol'], r['e32'] = las_ref.tolerances(ref, ref32, F, Cn)
        r['errs'] = las_ref.per_tensor_errors(g, ref[2], F, Cn)
        r['elogn'] = las_ref.rel_norm(r['logits'], ref[1])
    return r


def _assert_per_tensor(r, tag):
    """every gradient tensor against its own norm, the loss and the logits, within what the fp32 model allows"""
    worst = max(r['errs'], key=r['errs'].get)
    print('LAS %s: loss rel %.2e (fp32 model %.1e, tol %.1e), logits rel %.2e (%.1e, %.1e), '
          'worst tensor %.2e %s (%.1e, %.1e)'
          % (tag, r['el'], r['e32']['loss'], r['tol']['loss'], r['elogn'], r['e32']['logits'], r['tol']['logits'],
             r['errs'][worst], worst, r['e32']['grad'], r['tol']['grad']))
    assert r['errs'][worst] <= r['tol']['grad'], (worst, r['errs'][worst], r['tol']['grad'])
    assert r['el'] <= r['tol']['loss'] and r['elogn'] <= r['tol']['logits']
    assert np.isfinite(r['g']).all() and np.isfinite(r['logits']).all()


def _errs(e, F, feats, seq, labels, ll):
    r = _pass(e, F, feats, seq, labels, ll, p32=False)
    return r['el'], r['eg'], r['elog'], r['fed']


def _replay_draws(fed, labels, logits, seed, counter, tower, p, utterances, classes):
    """every draw of `utterances` against the hash: Bernoulli by u0, the sample by inverse CDF over the GPU's own logits;
    returns (sampled inputs, those whose class could be checked)"""
    logits = logits.astype(np.float64)
    thr = (1 << 24) if p >= 1 else int(np.floor(p * 2 ** 24))
    n_s = checked = 0
    for b in utterances:
        for t in range(1, labels.shape[1]):
            u0, u1 = las_ref.sample_uniforms(seed, counter, tower, t, b)
            if u0 >= thr:
                assert fed[b, t] == labels[b, t]
                continue
            n_s += 1
            z = logits[b, t - 1] - logits[b, t - 1].max()
            cdf = np.cumsum(np.exp(z) / np.exp(z).sum())
            u = u1 / 2.0 ** 24
            if np.min(np.abs(cdf - u)) < 1e-6:
                continue
            assert fed[b, t] == min(int(np.searchsorted(cdf, u, side='right')), classes - 1)
            checked += 1
    return n_s, checked


@pytest.mark.parametrize('T,B,U', [(1, 1, 1), (2, 5, 7), (3, 17, 7), (15, 5, 30), (16, 1, 7), (17, 5, 1), (60, 5, 7)])
def test_loss_grads_p0(T, B, U):
    F = 20
    rs = np.random.RandomState(T * 100 + B + U)
    e = _engine(F)
    feats, seq, labels, ll = _batch(B, T, F, U, rs, empty=True)
    r = _pass(e, F, feats, seq, labels, ll)
    el, eg, elog, fed = r['el'], r['eg'], r['elog'], r['fed']
    print('LAS p=0 T=%d B=%d U=%d: loss rel %.2e, grad rel-to-max %.2e, logits abs %.2e' % (T, B, U, el, eg, elog))
    assert (fed == labels).all()
    # MI355X: loss rel <= 1.2e-7, gradients rel-to-max <= 1.5e-7, logits abs <= 3.1e-8
    assert el < 5e-7 and eg < 5e-7 and elog < 1e-7
    _assert_per_tensor(r, 'p=0 T=%d B=%d U=%d' % (T, B, U))


@pytest.mark.parametrize('p', [0.1, 1.0])
def test_sampling_replayed(p):
    F, B, T, U = 16, 5, 17, 12
    rs = np.random.RandomState(11)
    e = _engine(F, p=p)
    feats, seq, labels, ll = _batch(B, T, F, U, rs)
    _, seed, counter, tower = e.sampling_state()
    r = _pass(e, F, feats, seq, labels, ll)
    el, eg, elog, fed = r['el'], r['eg'], r['elog'], r['fed']
    print('LAS p=%g: loss rel %.2e, grad rel-to-max %.2e, logits abs %.2e' % (p, el, eg, elog))
    # MI355X: loss rel <= 3.6e-8, gradients rel-to-max <= 1.0e-7, logits abs <= 2.6e-8
    assert el < 2e-7 and eg < 3e-7 and elog < 1e-7
    _assert_per_tensor(r, 'p=%g' % p)
    assert (fed[:, 0] == labels[:, 0]).all()
    assert e.sampling_state()[2] == counter + 1
    n_s, checked = _replay_draws(fed, labels, r['logits'], seed, counter, tower, p, range(B), C)
    if p >= 1:
        assert n_s == B * (U - 1)
    assert checked >= n_s - 2


# ---- Trained-like weights (las_ref.trained_like): at initial_params the attention is uniform and the gradients of
# query_layer, memory_layer and attention_v are 1e-8 .. 1e-4 of the whole, so the cases above cannot see the attention's
# backward pass.  tests/test_las_host.py asserts, on the fp64 model alone, what these cases rest on: how peaked each
# regime's attention is, that every tensor's share of the gradient is above the metric's floor, and that a backward pass
# with the q or the alpha path cut misses the tolerance by more than 100x.
# MI355X, worst tensor of per_tensor_errors / logits rel / loss rel (the fp32 torch model's in brackets): DESIGN.md §10.
@pytest.mark.parametrize('T,B,U', las_ref.REGIME_SHAPES)
@pytest.mark.parametrize('regime', list(las_ref.REGIMES))
def test_regime_every_tensor(regime, T, B, U):
    F = 16
    flat, feats, seq, labels, ll = las_ref.regime_case(regime, T, B, U, F, C)
    e = _engine(F, flat=flat)
    r = _pass(e, F, feats, seq, labels, ll)
    assert ll[0] == 0 and (r['fed'] == labels).all()
    _assert_per_tensor(r, '%s T=%d B=%d U=%d' % (regime, T, B, U))


@pytest.mark.parametrize('B,p', [(16, 0.0), (33, 0.0), (64, 0.0), (64, 1.0)])
def test_batch_edges(B, p):
    """Bp = B (no padded row), Bp = 48, and the widest batch the handle takes: the last lane of las_loss_kernel's sum
    and, with every input sampled, the draws of b = 63 (the hash packs t * 64 + b)."""
    F, T, U = 16, 9, 5
    flat, feats, seq, labels, ll = las_ref.regime_case('moderate', T, B, U, F, C)
    ll[B - 1] = U                                       # the last utterance counts in the loss at every step
    e = _engine(F, p=p, flat=flat)
    _, seed, counter, tower = e.sampling_state()
    r = _pass(e, F, feats, seq, labels, ll)
    _assert_per_tensor(r, 'B=%d p=%g' % (B, p))
    if p == 0:
        assert (r['fed'] == labels).all()
    else:
        assert (r['fed'][:, 0] == labels[:, 0]).all() and (r['fed'] != labels).any()
        n_s, checked = _replay_draws(r['fed'], labels, r['logits'], seed, counter, tower, p, [B - 1], C)
        assert n_s == U - 1 and checked >= n_s - 1


@pytest.mark.parametrize('classes', [31, 33, 65, 2300])
def test_class_edges(classes):
    """Cp = 32 / 64 / 96 (C = 65: the second trip of las_ce_kernel's lane loops) and Cp = 2304, where the projection
    bias's column sum needs more workspace than the encoder's and the decoder's gate sums.  Utterance 1's labels hold
    class C - 1 (las_embed_grad's last row) and, from C = 65, classes >= 64 (k == y in the second trip)."""
    F, B, T, U = 16, 5, 17, 7
    must = (classes - 1,) if classes <= 64 else (classes - 1, 64, classes // 2)
    flat, feats, seq, labels, ll = las_ref.regime_case('moderate', T, B, U, F, classes, must_use=must)
    assert set(must) <= set(labels[1, :ll[1]].tolist())
    e = _engine(F, classes=classes, flat=flat)
    r = _pass(e, F, feats, seq, labels, ll, classes=classes)
    assert (r['fed'] == labels).all()
    _assert_per_tensor(r, 'C=%d' % classes)
    if classes > 2000:
        # the same pass again: a neighbour of the column-sum workspace that the first pass overwrote would show here
        loss2, _, g2 = e.loss_and_grads(feats, seq, labels, ll)
        assert loss2 == r['loss'] and np.array_equal(g2, r['g']) and np.array_equal(e.logits(), r['logits'])


def test_sampled_fraction_within_binomial_bounds():
    F, B, T, U = 8, 17, 6, 30
    rs = np.random.RandomState(2)
    e = _engine(F, p=0.1)
    feats, seq, labels, ll = _batch(B, T, F, U, rs)
    _, seed, counter, tower = e.sampling_state()
    e.upload_batch(feats, seq, labels, ll)
    e.compute_grads()
    sampled = e.sampled()                                   # what the GPU's sampler did, step by step
    assert (sampled[:, 0] == 0).all()
    n = B * (U - 1)
    k = int(sampled[:, 1:].sum())
    assert abs(k - 0.1 * n) < 4 * np.sqrt(n * 0.1 * 0.9)
    want = np.array([[las_ref.sample_uniforms(seed, counter, tower, t, b)[0] < int(0.1 * 2 ** 24) for t in range(1, U)]
                     for b in range(B)])
    np.testing.assert_array_equal(sampled[:, 1:], want.astype(np.int32))
    fed = e.fed_ids()
    assert (fed[sampled == 0] == labels[sampled == 0]).all()


def test_two_runs_bitwise_and_adam():
    F, B, T, U = 24, 5, 15, 9
    rs = np.random.RandomState(4)
    feats, seq, labels, ll = _batch(B, T, F, U, rs)
    out = []
    for _ in range(2):
        e = _engine(F, p=0.1)
        losses = [e.train_step(feats, seq, labels, ll) for _ in range(3)]
        m, v, step = e.get_adam_state()
        out.append((losses, e.get_params(), m, v, step))
    assert out[0][0] == out[1][0] and out[0][4] == out[1][4] == 3
    for a, b in zip(out[0][1:4], out[1][1:4]):
        assert np.array_equal(a, b)
    assert np.isfinite(out[0][0]).all()


def test_adam_against_fp64():
    F, B, T, U = 16, 3, 9, 6
    rs = np.random.RandomState(8)
    feats, seq, labels, ll = _batch(B, T, F, U, rs)
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    e = _engine(F, lr=lr)
    p = e.get_params().astype(np.float64)
    m = np.zeros_like(p)
    v = np.zeros_like(p)
    for k in range(1, 4):
        loss = e.train_step(feats, seq, labels, ll)
        rl, _, g = las_ref.loss_and_grads(p.astype(np.float32), F, C, feats, labels, ll)
        assert abs(loss - rl) / rl < 1e-5
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        lr_t = lr * np.sqrt(1 - b2 ** k) / (1 - b1 ** k)
        p = p - lr_t * m / (np.sqrt(v) + eps)
    got = e.get_params().astype(np.float64)
    err = np.max(np.abs(got - p))
    print('LAS Adam x3: params abs %.2e' % err)
    assert err < 1e-6                                    # MI355X: 2.9e-7


def test_full_size():
    F, B, T, U, Cf = 840, 8, 400, 80, 32
    global C
    saved, C = C, Cf
    try:
        rs = np.random.RandomState(1)
        e = _engine(F)
        feats, seq, labels, ll = _batch(B, T, F, U, rs)
        el, eg, elog, _ = _errs(e, F, feats, seq, labels, ll)
    finally:
        C = saved
    print('LAS full size: loss rel %.2e, grad rel-to-max %.2e, logits abs %.2e' % (el, eg, elog))
    # MI355X: loss rel 1.7e-7, gradients rel-to-max 1.2e-7, logits abs 9.8e-8
    assert el < 5e-7 and eg < 4e-7 and elog < 3e-7


def test_ctc_only_calls_refused():
    from neuralasr_amd._lib import NasrError
    e = _engine(8)
    assert e.logit_frames(4) == -4                       # NASR_ERR_STATE
    assert e.lib.nasr_set_step_decode(e.h, 1) == -4
    with pytest.raises(NasrError):
        e._ck(e.lib.nasr_set_step_decode(e.h, 1))
