"""CPU: pins the fp64 torch model of the WaveNet (tests/wavenet_ref.py) that the GPU tests check the HIP network against,
and the WaveNet's C ABI surface (header, ctypes binding, exports, no CPU fallback)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wavenet_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ['nasr_create_wavenet', 'nasr_wavenet_bn_count', 'nasr_wavenet_get_bn_state', 'nasr_wavenet_set_bn_state',
               'nasr_wavenet_set_bn_hold', 'nasr_wavenet_get_batch_stats', 'nasr_wavenet_apply_bn_stats']


def test_dilated_convolution_is_same_padded_cross_correlation():
    """atrous_conv2d 'SAME' at rate r: y[t] = sum_k x[t + (k-3) r] W[k], frames outside [0, T) read zero."""
    rs = np.random.RandomState(0)
    T, Ci, Co, r = 9, 3, 2, 2
    x = rs.randn(1, T, Ci)
    w = rs.randn(W.KS, Ci, Co)
    want = np.zeros((T, Co))
    for t in range(T):
        for k in range(W.KS):
            s = t + (k - 3) * r
            if 0 <= s < T:
                want[t] += x[0, s] @ w[k]
    got = F.conv1d(torch.tensor(x).permute(0, 2, 1), torch.tensor(w).permute(2, 1, 0), dilation=r, padding=3 * r)
    assert np.allclose(got.permute(0, 2, 1).numpy()[0], want, atol=1e-12)


def test_whole_model_gradcheck_at_a_tiny_size():
    spec = W.Spec(5, 4, num_blocks=1, rates=(1, 2), dim=4)
    feats, seq, labels, ll = W.synth_batch(spec, 3, 6, seed=1, Lmax=2)
    flat = W.init_params(spec, 2).astype(np.float64) + 0.1 * np.random.RandomState(3).randn(
        sum(r * c for _, r, c in W.tensor_specs(spec)))
    names = [n for n, _, _ in W.tensor_specs(spec)]
    P0 = W.unflatten(spec, flat)

    def fn(*ts):
        P = dict(zip(names, ts))
        logits, _ = W.forward(spec, P, feats, True)
        return W.ctc_mean(logits, seq, labels, ll)[0]
    inputs = tuple(P0[n].clone().requires_grad_(True) for n in names)
    assert torch.autograd.gradcheck(fn, inputs, eps=1e-6, atol=1e-6, rtol=1e-4)


def test_moving_statistics_recurrence_by_hand():
    """Three updates of a 1x1 site (Bessel-corrected variance) and a dilated site (population variance), by hand:
    biased <- biased - (biased - mu)(1-d); moving_mean = biased / (1 - d^n); moving_var <- moving_var - (moving_var - v)(1-d)."""
    spec = W.Spec(5, 4, num_blocks=1, rates=(1,), dim=2)
    assert W.bessel_sites(spec) == [True, False, False, True, True]
    st = W.bn_initial(spec)
    rs = np.random.RandomState(4)
    d = 0.99
    bm, mv = np.zeros(2), np.ones(2)
    for n in range(1, 4):
        mean = rs.randn(spec.sites, 2).astype(np.float32)
        var = rs.rand(spec.sites, 2).astype(np.float32)
        N = 6
        stats = [(mean[s], var[s], N) for s in range(spec.sites)]
        m, v = W.update_variance(spec, stats)
        assert np.allclose(v[0], var[0] * 6 / 5, rtol=1e-6) and np.allclose(v[1], var[1], rtol=0)
        st = W.bn_update(spec, st, m, v)
        # site 1 (dilated filter) by hand in fp64
        bm = bm - (bm - mean[1]) * (1 - d)
        mv = mv - (mv - var[1]) * (1 - d)
        assert st['n'] == n
        assert np.allclose(st['mm'][1], bm / (1 - d ** n), rtol=1e-5)
        assert np.allclose(st['mv'][1], mv, rtol=1e-5)
        assert np.allclose(st['biased'][1], bm, rtol=1e-5, atol=1e-7)
    # after the first update the zero-debiased mean is the batch mean itself
    st1 = W.bn_update(spec, W.bn_initial(spec), mean, var)
    assert np.allclose(st1['mm'], mean, rtol=1e-5)
    # N = 1: TF's fused batch norm takes N-1 as 1
    assert np.allclose(W.update_variance(spec, [(mean[s], var[s], 1) for s in range(spec.sites)])[1], var)


def test_parameter_names_order_and_count_at_the_reference_size():
    spec = W.Spec(546, 29)
    ts = W.tensor_specs(spec)
    assert sum(r * c for _, r, c in ts) == 3788416
    assert len(ts) == 3 + 15 * 9 + 3 + 1
    assert [n for n, _, _ in ts[:6]] == ['front/conv_in/W', 'front/conv_in/BatchNorm/beta', 'front/conv_in/BatchNorm/gamma',
                                         'block_0_1/conv_filterblock_0_1/W', 'block_0_1/conv_filterblock_0_1/BatchNorm/beta',
                                         'block_0_1/conv_filterblock_0_1/BatchNorm/gamma']
    assert ts[6][0] == 'block_0_1/conv_gateblock_0_1/W' and ts[9][0] == 'block_0_1/conv_outblock_0_1/W'
    assert ts[12][0] == 'block_0_2/conv_filterblock_0_2/W' and (ts[12][1], ts[12][2]) == (7 * 128, 128)
    assert [n for n, _, _ in ts[-4:]] == ['logit/conv_1/W', 'logit/conv_1/BatchNorm/beta', 'logit/conv_1/BatchNorm/gamma',
                                          'logit/conv_2/W']
    assert (ts[-1][1], ts[-1][2]) == (128, 29) and (ts[0][1], ts[0][2]) == (546, 128)
    assert spec.sites == 47


def test_initializer_bounds_keep_the_fan_quirk():
    from neuralasr_amd.networks.wavenet import WaveNet
    spec = W.Spec(546, 29)
    tensors, o = [], 0
    for n, r, c in W.tensor_specs(spec):
        tensors.append((n, o, r, c))
        o += r * c
    net = WaveNet.__new__(WaveNet)
    flat = net.initial_params(tensors, seed=1)
    assert np.array_equal(flat, W.init_params(spec, 1))
    for n, off, r, c in tensors:
        x = flat[off:off + r * c]
        if n.endswith('/W'):
            bound = np.sqrt(1 / (7 * 128)) if ('conv_filter' in n or 'conv_gate' in n) else np.sqrt(1 / np.sqrt(r * c))
            assert np.abs(x).max() <= bound and np.abs(x).max() > 0.95 * bound, n
        elif n.endswith('gamma'):
            assert np.all(x == 1)
        else:
            assert np.all(x == 0)
    # conv_in at F = 546: fan_in = sqrt(546*128) ~ 264.4, bound ~ 0.0615; a dilated kernel: 1/sqrt(896) ~ 0.0334
    assert abs(np.sqrt(1 / np.sqrt(546 * 128)) - 0.0615) < 1e-3


def test_new_symbols_are_declared_bound_and_exported():
    from neuralasr_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nasr.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r'\b%s\s*\(' % n, text), n
        assert n in _lib.SYMBOLS
        assert hasattr(lib, n)
    assert ctypes.sizeof(_lib.WaveNetCfg) == 6 * 4 + 8 * 4 + 6 * 4


def test_wavenet_create_fails_without_a_gpu():
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import WaveNetEngine
    with pytest.raises(_lib.NasrError, match='no HIP device|no CPU fallback'):
        WaveNetEngine(39, 29)


def test_wavenet_rejects_other_widths_before_looking_for_a_device():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import WaveNetEngine
    with pytest.raises(_lib.NasrError, match='dim = 128'):
        WaveNetEngine(39, 29, dim=64)
    with pytest.raises(_lib.NasrError, match='kernel_size = 7'):
        WaveNetEngine(39, 29, kernel_size=5)


def test_network_module_resolves_by_reference_name():
    import importlib
    mod = importlib.import_module('neuralasr_amd.networks.wavenet')
    assert mod.WaveNet.num_blocks == 3 and mod.WaveNet.rates == (1, 2, 4, 8, 16) and mod.WaveNet.num_dim == 128
