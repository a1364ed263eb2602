"""Host-side parts of the LAS network (no GPU): network resolution, variable specs, the pyramid's lengths, the LER and the
scheduled-sampling hash; and the conditions that the regime tests of tests/test_gpu_las.py rest on, checked on the fp64
model alone: how peaked the attention of each regime is, that no tensor's gradient hides below the metric's floor, and
that the per-tensor metric would catch a backward pass with the attention's q or alpha path cut."""
import functools
import types

import numpy as np
import pytest

from neuralasr_amd.config import Config
from neuralasr_amd.networks import las
from tests import las_ref


def test_load_network_resolves_las(monkeypatch):
    made = []
    monkeypatch.setattr(las.LAS, '__init__', lambda self, config, fortraining=False: made.append((config, fortraining)))
    cfg = types.SimpleNamespace(network='networks.las.LAS')
    net = Config.load_network(cfg, fortraining=True)
    assert isinstance(net, las.LAS) and made == [(cfg, True)]


def test_tensor_specs_order_and_shapes():
    specs = las.tensor_specs(840, 32)
    names = [n for n, _, _ in specs]
    assert names[:4] == ['bidirectional_rnn/fw/fw_0/kernel', 'bidirectional_rnn/fw/fw_0/bias',
                         'bidirectional_rnn/bw/bw_0/kernel', 'bidirectional_rnn/bw/bw_0/bias']
    assert names[16:] == ['memory_layer/kernel', 'decoder_lstm/kernel', 'decoder_lstm/bias', 'query_layer/kernel',
                          'attention_v', 'attention_layer/kernel', 'projection_layer/kernel', 'projection_layer/bias']
    shapes = {n: (r, c) for n, r, c in specs}
    assert shapes['bidirectional_rnn/fw/fw_0/kernel'] == (840 + 250, 1000)
    assert shapes['bidirectional_rnn/bw/bw_3/kernel'] == (1000 + 250, 1000)
    assert shapes['decoder_lstm/kernel'] == (32 + 250 + 500, 2000)
    assert shapes['attention_layer/kernel'] == (1000, 250)
    assert shapes['projection_layer/kernel'] == (250, 32)


@pytest.mark.parametrize('T', range(1, 41))
def test_pyramid_lengths(T):
    L = las.pyramid_lengths(T)
    # the reference: pad an odd length with one frame, run, halve by pairs
    n = T
    for i in range(4):
        n += n % 2
        assert L[i] == n
        n //= 2


def test_label_error_rate_drops_zero_and_empty_reference():
    assert las.label_error_rate([[3, 0, 4, 5]], [[3, 4, 5, 0]]) == 0.0
    assert las.label_error_rate([[3, 4, 0]], [[3, 5, 6]]) == pytest.approx(2 / 3)
    assert las.label_error_rate([[0, 0]], [[0, 0]]) == 0.0
    assert np.isinf(las.label_error_rate([[2, 0]], [[0, 0]]))
    logits = np.zeros((1, 3, 4))
    logits[0, :, 2] = 1
    assert las.model_ids(logits, [2]).tolist() == [[2, 2, 0]]


def test_sampling_hash_matches_definition():
    # lowbias32 of a few fixed words (the function of las.hip / dense.hip), recomputed in pure Python
    def lb(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16; x = (x * 0x7FEB352D) & 0xFFFFFFFF
        x ^= x >> 15; x = (x * 0x846CA68B) & 0xFFFFFFFF
        x ^= x >> 16
        return x
    for x in (0, 1, 12345, 0xFFFFFFFF, 0x9E3779B9):
        assert int(las_ref.lowbias32(x)) == lb(x)
    seed, counter, tower, t, b = 7, 3, 1, 5, 2
    key = (seed + 0x9E3779B9 * (tower + 1) + 0x85EBCA6B * counter) & 0xFFFFFFFF
    base = (t * 64 + b) * 2
    assert las_ref.sample_uniforms(seed, counter, tower, t, b) == (lb(base ^ key) >> 8, lb((base + 1) ^ key) >> 8)
    # the Bernoulli draws are uniform enough for p = 0.1
    u = [las_ref.sample_uniforms(1, c, 0, t, b)[0] for c in range(20) for t in range(1, 20) for b in range(8)]
    frac = np.mean(np.asarray(u) < int(0.1 * 2 ** 24))
    assert 0.07 < frac < 0.13


def test_fp64_reference_sequence_loss_masks():
    import torch
    logits = torch.zeros(2, 3, 4, dtype=torch.float64)
    loss = las_ref.sequence_loss(logits, [[1, 2, 3], [1, 0, 0]], [3, 0])
    assert float(loss) == pytest.approx(np.log(4))


# ---------------------------------------------------------------- the regimes of tests/test_gpu_las.py
# Measured with this file (F 16, C 12, initial_params(seed=3), las_ref.regime_case):
#   (T, B, U)     regime    (k_att, k_rec)  median / min of max_l alpha   smallest tensor share   worst tensor, fp32 vs fp64
#   (40, 5, 9)    init      (1, 1)          0.167 / 0.167 (uniform 1/6)   5e-8   query_layer      5.5e-7
#   (40, 5, 9)    moderate  (8, 2)          0.58  / 0.28                  1.6e-2 query_layer      2.0e-6
#   (40, 5, 9)    peaked    (16, 3)         0.995 / 0.42                  5.4e-3 attention_v      1.1e-5
#   (17, 17, 12)  moderate  (8, 2)          0.58  / 0.34                  1.3e-2 query_layer      1.9e-6
#   (17, 17, 12)  peaked    (16, 3)         0.99  / 0.40                  1.2e-2 attention_v      1.3e-5
# (the last column depends on how torch's CPU kernels split their sums, so on the thread count: 1.3e-6 .. 3.3e-5 seen)
# Either mutant's worst tensor is wrong by 1.0 (its gradient is gone) in all four regime cases: 2e4 .. 1e5 tolerances.
F_R, C_R = 16, 12
CASES = [(r, s) for r in las_ref.REGIMES for s in las_ref.REGIME_SHAPES]


@functools.lru_cache(maxsize=None)
def _regime(regime, T, B, U):
    """the fp64 model of a regime case, once: (batch, reference, per-step max alpha, tolerances)"""
    import torch
    flat, feats, seq, labels, ll = las_ref.regime_case(regime, T, B, U, F_R, C_R)
    alphas = []
    ref = las_ref.loss_and_grads(flat, F_R, C_R, feats, labels, ll, alphas=alphas)
    ref32 = las_ref.loss_and_grads(flat, F_R, C_R, feats, labels, ll, dtype=torch.float32)
    tol, e32 = las_ref.tolerances(ref, ref32, F_R, C_R)
    return (flat, feats, labels, ll), ref, np.stack(alphas).max(2), tol, e32


@pytest.mark.parametrize('regime,shape', CASES)
def test_regime_attention_is_as_peaked_as_its_name(regime, shape):
    _, _, amax, _, _ = _regime(regime, *shape)
    med = float(np.median(amax))                      # over (step, utterance)
    print('LAS %s %s: max_l alpha median %.3f, min %.3f' % (regime, shape, med, amax.min()))
    if regime == 'moderate':
        assert 0.3 <= med <= 0.7
    else:
        assert med >= 0.9


@pytest.mark.parametrize('regime,shape', CASES)
def test_regime_no_tensor_below_the_metric_floor(regime, shape):
    _, ref, _, _, e32 = _regime(regime, *shape)
    shares = las_ref.tensor_shares(ref[2], F_R, C_R)
    low = min(shares, key=shares.get)
    print('LAS %s %s: smallest share %.1e (%s); fp32 model: loss %.1e, logits %.1e, worst tensor %.1e'
          % (regime, shape, shares[low], low, e32['loss'], e32['logits'], e32['grad']))
    assert shares[low] >= 1e-3, (low, shares[low])


@pytest.mark.parametrize('mutant', las_ref.MUTANTS)
@pytest.mark.parametrize('regime,shape', CASES)
def test_regime_metric_catches_a_cut_attention_path(regime, shape, mutant):
    (flat, feats, labels, ll), ref, _, tol, _ = _regime(regime, *shape)
    lm, logm, gm = las_ref.loss_and_grads(flat, F_R, C_R, feats, labels, ll, mutant=mutant)
    assert lm == ref[0] and np.array_equal(logm, ref[1])          # only the backward pass is wrong
    errs = las_ref.per_tensor_errors(gm, ref[2], F_R, C_R)
    worst = max(errs, key=errs.get)
    print('LAS %s %s %s: worst tensor %.2e (%s), tolerance %.1e' % (regime, shape, mutant, errs[worst], worst, tol['grad']))
    assert errs[worst] >= 100 * tol['grad']


def test_old_metric_at_initialisation_lets_a_cut_q_path_through():
    """Why the gradient metric changed: at initial_params the attention is uniform, query_layer's gradient is ~1e-7 of
    the whole, and max|g - ref| / max|ref| <= 5e-7 (the only gradient check there was) passes a model whose q path is cut."""
    T, B, U = las_ref.REGIME_SHAPES[0]
    flat = las_ref.initial_params(F_R, C_R, seed=3)
    _, feats, seq, labels, ll = las_ref.regime_case('moderate', T, B, U, F_R, C_R)
    alphas = []
    _, _, g = las_ref.loss_and_grads(flat, F_R, C_R, feats, labels, ll, alphas=alphas)
    _, _, gm = las_ref.loss_and_grads(flat, F_R, C_R, feats, labels, ll, mutant='q_detached')
    L4 = alphas[0].shape[1]
    assert abs(np.median(np.stack(alphas).max(2)) - 1.0 / L4) < 0.01   # uniform attention
    old = np.max(np.abs(gm - g)) / np.max(np.abs(g))
    print('LAS init, q detached: old metric %.2e' % old)
    assert old < 5e-7
    sl = las_ref.tensor_slices(F_R, C_R)['query_layer/kernel']
    assert not gm[sl].any() and g[sl].any()


def test_fp32_model_and_trained_like():
    import torch
    flat = las_ref.initial_params(F_R, C_R, seed=3)
    P64, P32 = las_ref.unflatten(flat, F_R, C_R), las_ref.unflatten(flat, F_R, C_R, torch.float32)
    assert all(t.dtype == torch.float64 for t in P64.values()) and all(t.dtype == torch.float32 for t in P32.values())
    scaled = las_ref.trained_like(flat, F_R, C_R, 8, 2)
    assert scaled.dtype == np.float32
    for name, sl in las_ref.tensor_slices(F_R, C_R).items():
        k = 8 if name in ('attention_v', 'memory_layer/kernel', 'query_layer/kernel') else \
            2 if name.endswith('/kernel') and (name.startswith('bidirectional_rnn/') or name == 'decoder_lstm/kernel') else 1
        np.testing.assert_array_equal(scaled[sl], (flat[sl].astype(np.float64) * k).astype(np.float32), err_msg=name)
    # the metric: a tensor's error against its own norm, the floor for a tensor that is (nearly) zero
    g = np.zeros(flat.size)
    sl = las_ref.tensor_slices(F_R, C_R)
    g[sl['attention_v']] = 1.0
    bad = g.copy()
    bad[sl['attention_v']] *= 1.01
    bad[sl['projection_layer/bias']] = 1e-3 * np.linalg.norm(g) / np.sqrt(C_R)
    errs = las_ref.per_tensor_errors(bad, g, F_R, C_R)
    assert errs['attention_v'] == pytest.approx(0.01) and errs['projection_layer/bias'] == pytest.approx(1.0)
    assert errs['query_layer/kernel'] == 0.0
    # a batch without a label: the gradient is zero, and only zeros match it
    zero = np.zeros(flat.size)
    assert set(las_ref.per_tensor_errors(zero, zero, F_R, C_R).values()) == {0.0}
    assert las_ref.per_tensor_errors(g * 1e-20, zero, F_R, C_R)['attention_v'] > 1.0
