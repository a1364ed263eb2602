"""The LAS network on the GPU against the fp64 torch model of tests/las_ref.py: logits, sequence loss and every gradient
(scheduled sampling off, then with the GPU's fed ids replayed), the sampling draws against the hash, Adam and determinism.
Measured errors are printed (pytest -s) and recorded in DESIGN.md §10."""
import numpy as np
import pytest

from tests import las_ref

pytestmark = pytest.mark.gpu

C = 12


def _engine(F, p=0.0, lr=1e-3):
    from neuralasr_amd.engine import LasEngine
    from neuralasr_amd.networks.las import LAS
    e = LasEngine(F, C, sampling_probability=p, seed=5, learning_rate=lr)
    net = LAS.__new__(LAS)
    e.set_params(net.initial_params(e.tensors(), seed=3))
    return e


def _batch(B, T, F, U, rs, empty=False):
    feats = rs.randn(B, T, F).astype(np.float32)
    seq = rs.randint(1, T + 1, size=B)
    for b in range(B):
        feats[b, seq[b]:] = 0
    labels = rs.randint(0, C, size=(B, U)).astype(np.int32)
    ll = rs.randint(0, U + 1, size=B).astype(np.int32)
    if empty:
        ll[0] = 0
    return feats, seq, labels, ll


def _errs(e, F, feats, seq, labels, ll, ids=None):
    loss, nll, g = e.loss_and_grads(feats, seq, labels, ll)
    logits = e.logits()
    fed = e.fed_ids()
    rl, rlogits, rg = las_ref.loss_and_grads(e.get_params(), F, C, feats, labels, ll, fed if ids is None else ids)
    el = abs(loss - rl) / max(abs(rl), 1e-30)
    eg = np.max(np.abs(g - rg)) / max(np.max(np.abs(rg)), 1e-30)
    elog = np.max(np.abs(logits - rlogits))
    return el, eg, elog, fed


@pytest.mark.parametrize('T,B,U', [(1, 1, 1), (2, 5, 7), (3, 17, 7), (15, 5, 30), (16, 1, 7), (17, 5, 1), (60, 5, 7)])
def test_loss_grads_p0(T, B, U):
    F = 20
    rs = np.random.RandomState(T * 100 + B + U)
    e = _engine(F)
    feats, seq, labels, ll = _batch(B, T, F, U, rs, empty=True)
    el, eg, elog, fed = _errs(e, F, feats, seq, labels, ll)
    print('LAS p=0 T=%d B=%d U=%d: loss rel %.2e, grad rel-to-max %.2e, logits abs %.2e' % (T, B, U, el, eg, elog))
    assert (fed == labels).all()
    # MI355X: loss rel <= 1.2e-7, gradients rel-to-max <= 1.5e-7, logits abs <= 3.1e-8
    assert el < 5e-7 and eg < 5e-7 and elog < 1e-7


@pytest.mark.parametrize('p', [0.1, 1.0])
def test_sampling_replayed(p):
    F, B, T, U = 16, 5, 17, 12
    rs = np.random.RandomState(11)
    e = _engine(F, p=p)
    feats, seq, labels, ll = _batch(B, T, F, U, rs)
    _, seed, counter, tower = e.sampling_state()
    el, eg, elog, fed = _errs(e, F, feats, seq, labels, ll)
    print('LAS p=%g: loss rel %.2e, grad rel-to-max %.2e, logits abs %.2e' % (p, el, eg, elog))
    # MI355X: loss rel <= 3.6e-8, gradients rel-to-max <= 1.0e-7, logits abs <= 2.6e-8
    assert el < 2e-7 and eg < 3e-7 and elog < 1e-7
    assert (fed[:, 0] == labels[:, 0]).all()
    assert e.sampling_state()[2] == counter + 1
    # every draw against the hash: Bernoulli by u0, the sample by inverse CDF over the GPU's own logits
    logits = e.logits().astype(np.float64)
    thr = (1 << 24) if p >= 1 else int(np.floor(p * 2 ** 24))
    n_s = checked = 0
    for b in range(B):
        for t in range(1, U):
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
            assert fed[b, t] == min(int(np.searchsorted(cdf, u, side='right')), C - 1)
            checked += 1
    if p >= 1:
        assert n_s == B * (U - 1)
    assert checked >= n_s - 2


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
