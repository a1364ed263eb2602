"""Distillation without a GPU: the fp64 restatement of the rule (tests/distill_ref.py) against central
differences and at its edges, its float32 restatement against it, the three config keys with every refusal of config.py,
and the argument checks of the ABI that need no device."""
import ctypes
import os

import numpy as np
import pytest

from oracle import nasr_oracle as O
from tests import distill_ref as D

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')


def logits_pair(Tp, B, C, seed, scale=1.0):
    rs = np.random.RandomState(seed)
    return scale * rs.randn(Tp, B, C), scale * rs.randn(Tp, B, C)


# ------------------------------------------------------------------------------------------- the rule
@pytest.mark.parametrize('a,tau', [(0.5, 2.0), (0.9, 1.0), (0.3, 0.25)])
def test_gradient_of_the_term_against_central_differences(a, tau):
    Tp, B, C = 5, 3, 4
    z, y = logits_pair(Tp, B, C, 3)
    seq_len = [5, 1, 3]
    _, grad = D.term(z, y, seq_len, a, tau)

    def value(zz):
        return a * tau * tau * float(np.mean(D.term(zz, y, seq_len, a, tau)[0]))
    h = 1e-6
    fd = np.zeros_like(z)
    for i in np.ndindex(*z.shape):
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        fd[i] = (value(zp) - value(zm)) / (2 * h)
    # central differences of a smooth fp64 function: h^2 f''' / 6 + eps f / h, both below 1e-9 here
    assert np.abs(fd - grad).max() <= 1e-8


def test_combined_loss_and_logit_gradient_through_the_oracle():
    """with_term(): the mean of what ctc_loss_and_grad returns is the combined loss, its gradient / B the combined one"""
    Tp, B, C, a, tau = 6, 2, 5, 0.4, 2.0
    z, y = logits_pair(Tp, B, C, 5)
    seq_len, labels, label_len = [6, 4], np.asarray([[1, 2], [3, 0]]), [2, 1]
    nll, _ = O.ctc_loss_and_grad(z, labels, label_len, seq_len)
    kd, _ = D.term(z, y, seq_len, a, tau)

    def loss_of(zz):
        with D.with_term(y, a, tau):
            return float(O.ctc_loss_and_grad(zz, labels, label_len, seq_len)[0].mean())
    assert abs(loss_of(z) - D.combined(nll.mean(), kd, a, tau)) <= 1e-12
    with D.with_term(y, a, tau):
        g = O.ctc_loss_and_grad(z, labels, label_len, seq_len)[1] / B
    assert O.ctc_loss_and_grad(z, labels, label_len, seq_len)[0].tobytes() == nll.tobytes()     # the oracle is itself again
    h = 1e-6
    for i in [(0, 0, 0), (3, 1, 4), (5, 0, 2), (4, 1, 1), (2, 0, 3)]:
        zp, zm = z.copy(), z.copy()
        zp[i] += h
        zm[i] -= h
        fd = (loss_of(zp) - loss_of(zm)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-8, i
    assert not g[4:, 1].any()


def test_teacher_equal_to_student_gives_nothing():
    z, _ = logits_pair(7, 3, 29, 1, 6.0)
    for fn in (D.term, D.rows_f32):
        kd, grad = fn(z, z, [7, 2, 5], 0.5, 1.0)
        assert not kd.any() and not grad.any()


def test_masked_rows():
    z, y = logits_pair(7, 3, 6, 2)
    seq_len = [7, 1, 4]
    for fn in (D.term, D.rows_f32):
        kd, grad = fn(z, y, seq_len, 0.5, 2.0)
        for b, n in enumerate(seq_len):
            assert not grad[n:, b].any() and grad[:n, b].any()
        z2, y2 = z.copy(), y.copy()
        z2[1:, 1], y2[4:, 2] = 99.0, -99.0                     # what lies behind an utterance's end is never read
        kd2, grad2 = fn(z2, y2, seq_len, 0.5, 2.0)
        assert kd2.tobytes() == kd.tobytes() and grad2.tobytes() == grad.tobytes()
    assert (kd > 0).all()                                       # a KL divergence of different rows


def test_large_logits_stay_finite():
    """magnitude 80 at tau = 0.25: exponents down to -640 - p underflows to 0 and contributes 0, nothing is inf or NaN"""
    z, y = logits_pair(4, 2, 33, 9, 80.0 / 3)
    z, y = np.clip(z, -80, 80), np.clip(y, -80, 80)
    z[0, 0, 0], y[0, 0, 1] = 80.0, 80.0
    z[0, 0, 1], y[0, 0, 0] = -80.0, -80.0
    for fn in (D.term, D.rows_f32):
        kd, grad = fn(z, y, [4, 3], 0.5, 0.25)
        assert np.isfinite(kd).all() and np.isfinite(grad).all() and (kd > 0).all()


def test_float32_restatement_is_close_to_fp64():
    """what fp32 arithmetic gives for the rule: the GPU tests allow the kernel 8 times this error, inside 1e-4"""
    for scale, tau in ((1, 1.0), (6, 4.0), (20, 0.25), (80 / 3.0, 0.25)):
        z, y = logits_pair(23, 5, 29, 4, scale)
        z, y = np.clip(z, -80, 80).astype(np.float32), np.clip(y, -80, 80).astype(np.float32)
        seq_len = [23, 1, 17, 9, 23]
        kd, g = D.term(z, y, seq_len, 0.5, tau)
        kd32, g32 = D.rows_f32(z, y, seq_len, 0.5, tau)
        eg = np.abs(g32 - g).max() / (0.5 * tau / 5)
        ek = (np.abs(kd32 - kd) / kd).max()
        print(scale, tau, 'grad', eg, 'kd', ek)
        assert 8 * eg <= 1e-4 and 8 * ek <= 1e-4


# ------------------------------------------------------------------------------------------- the config keys
def config_with(tmp_path, **extra):
    out = []
    for ln in open(os.path.join(SAMPLES, 'toy.config')).read().splitlines():
        if ln.startswith('output='):
            ln = 'output=' + SAMPLES
        out.append(ln)
        if ln.strip() == '[Parameters]':
            out += ['%s=%s' % kv for kv in extra.items()]
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_config_keys(tmp_path):
    from neuralasr_amd.config import Config
    c = Config(config_with(tmp_path), True)
    assert c.teacher_config is None and c.distill_weight == 0.5 and c.distill_temperature == 1.0
    c = Config(config_with(tmp_path, teacher_config='/some/teacher.config'), True)
    assert c.teacher_config == '/some/teacher.config' and c.distill_weight == 0.5 and c.distill_temperature == 1.0
    c = Config(config_with(tmp_path, teacher_config='t.config', distill_weight='0.25', distill_temperature=' 4 '), True)
    assert (c.teacher_config, c.distill_weight, c.distill_temperature) == ('t.config', 0.25, 4.0)
    for tau in ('0.25', '16'):
        assert Config(config_with(tmp_path, teacher_config='t', distill_temperature=tau), True).distill_temperature == float(tau)


@pytest.mark.parametrize('extra,words', [
    (dict(distill_weight='0.5'), ("'distill_weight' needs 'teacher_config'",)),
    (dict(distill_temperature='2'), ("'distill_temperature' needs 'teacher_config'",)),
    (dict(teacher_config=''), ("'teacher_config' must name",)),
    (dict(teacher_config='t', distill_weight='0'), ("'distill_weight' must be a number in (0,1)", "'0'")),
    (dict(teacher_config='t', distill_weight='1'), ("'distill_weight' must be a number in (0,1)",)),
    (dict(teacher_config='t', distill_weight='-0.1'), ("'distill_weight' must be a number in (0,1)",)),
    (dict(teacher_config='t', distill_weight='nan'), ("'distill_weight' must be a number in (0,1)",)),
    (dict(teacher_config='t', distill_weight='half'), ("'distill_weight' must be a number in (0,1)", "'half'")),
    (dict(teacher_config='t', distill_temperature='0.2'), ("'distill_temperature' must be a number in [0.25,16]",)),
    (dict(teacher_config='t', distill_temperature='16.5'), ("'distill_temperature' must be a number in [0.25,16]",)),
    (dict(teacher_config='t', distill_temperature='inf'), ("'distill_temperature' must be a number in [0.25,16]",)),
    (dict(teacher_config='t', distill_temperature='warm'), ("'distill_temperature' must be a number in [0.25,16]",)),
])
def test_config_refusals(tmp_path, extra, words):
    from neuralasr_amd.config import Config
    path = config_with(tmp_path, **extra)
    with pytest.raises(ValueError) as err:
        Config(path, True)
    for w in words + (path,):
        assert w in str(err.value), str(err.value)


# ------------------------------------------------------------------------------------------- the ABI without a device
def test_abi_refuses_a_null_handle():
    from neuralasr_amd import _lib
    lib = _lib.load()
    f, d = ctypes.c_float(7), ctypes.c_double(7)
    buf = (ctypes.c_float * 8)()
    seq = (ctypes.c_int32 * 1)(1)
    assert lib.nasr_set_distill(None, 0.5, 1.0) == _lib.NASR_ERR_ARG
    assert lib.nasr_get_distill(None, ctypes.byref(f), ctypes.byref(f)) == _lib.NASR_ERR_ARG
    assert lib.nasr_set_teacher_logits(None, buf) == _lib.NASR_ERR_ARG
    assert lib.nasr_take_teacher_logits(None, None) == _lib.NASR_ERR_ARG
    assert lib.nasr_get_distill_loss(None, ctypes.byref(f), ctypes.byref(f)) == _lib.NASR_ERR_ARG
    assert lib.nasr_distill_logits(None, buf, buf, seq, 1, 1, 0.5, 1.0, buf, ctypes.byref(d)) == _lib.NASR_ERR_ARG
    assert f.value == 7 and d.value == 7


def test_binding_declares_the_six_calls():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine, WaveNetEngine
    names = ['nasr_set_distill', 'nasr_get_distill', 'nasr_set_teacher_logits', 'nasr_take_teacher_logits',
             'nasr_get_distill_loss', 'nasr_distill_logits']
    assert all(n in _lib.SYMBOLS for n in names)
    for cls in (Engine, WaveNetEngine):
        for m in ('set_distill', 'distill', 'set_teacher_logits', 'take_teacher_logits', 'distill_loss', 'distill_logits'):
            assert hasattr(cls, m), (cls.__name__, m)
