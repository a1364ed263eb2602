"""Host-side parts of the LAS network (no GPU): network resolution, variable specs, the pyramid's lengths, the LER and the
scheduled-sampling hash."""
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
