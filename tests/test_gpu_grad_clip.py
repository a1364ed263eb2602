"""GPU: global-norm gradient clipping with the non-finite guard in the optimiser step (include/nasr.h, nasr_set_grad_clip;
DESIGN.md §14).  Gradients are planted with set_grads, so every case is exact: the measured norm and the coefficient against
fp64, the step bit for bit against a twin handle without clipping, the skipped and the void step, on all three model
families and on buffers below one workgroup's share and above one sweep of the reduction's grid."""
import ctypes
import math
import os

import numpy as np
import pytest

import grad_clip_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')
EPS22 = 2.0 ** -22


def _tiny():
    from neuralasr_amd.engine import Engine
    return Engine(10, 8, 1, True, 'stack_reshape', 4, learning_rate=2e-3)


def _big():
    # 2 x (39 + 256) x 1024 + 2 x (512 + 256) x 1024 weights and more: above the 1024 x 256 x 4 floats of one sweep of the
    # norm's grid, so every loop of both of its stages runs more than once
    from neuralasr_amd.engine import Engine
    return Engine(39, 256, 2, True, 'concat', 29, learning_rate=2e-3)


def _wavenet():
    from neuralasr_amd.engine import WaveNetEngine
    return WaveNetEngine(11, 7, num_blocks=1, rates=(1, 2, 4), learning_rate=2e-3)


def _las():
    from neuralasr_amd.engine import LasEngine
    return LasEngine(8, 12, sampling_probability=0.0, seed=5, learning_rate=2e-3)


MAKERS = {'tiny': _tiny, 'big': _big, 'wavenet': _wavenet, 'las': _las}
ALL = sorted(MAKERS)
_cache = {}


@pytest.fixture(scope='module', autouse=True)
def _close_engines():
    yield
    for e in _cache.values():
        e.close()
    _cache.clear()


def fresh(model, twin=0, clip=0.0, seed=1):
    """the module's handle (model, twin) with seeded parameters, zero Adam state, an empty stats window and `clip` set"""
    e = _cache.get((model, twin))
    if e is None:
        e = _cache[(model, twin)] = MAKERS[model]()
    n = e.param_count
    e.set_params((0.1 * np.random.RandomState(seed).randn(n)).astype(np.float32))
    e.set_adam_state(np.zeros(n, np.float32), np.zeros(n, np.float32), 0)
    e.set_grad_clip(clip)
    e.grad_clip_stats(reset=True)
    return e


def planted(n, seed):
    """random gradients with one large element at index 0 and one at the last index: a dropped head or tail shows"""
    g = (0.01 * np.random.RandomState(seed).randn(n)).astype(np.float32)
    g[0], g[-1] = 3.0, -4.0
    return g


def state(e):
    m, v, step = e.get_adam_state()
    return e.get_params(), m, v, step


def assert_same_state(a, b):
    for x, y, name in zip(a, b, ('P', 'M', 'V')):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=name)
    assert a[3] == b[3]


def f32(x):
    return float(np.float32(x))


def test_sizes_cover_both_ends_of_the_reduction():
    # the norm's first stage runs min(1024, ceil(n / 1024)) workgroups of 256 lanes x 4 floats.  tiny: the smallest layout a
    # handle has (padded to the kernels' tiles) - a handful of workgroups with one load per lane and a ragged last share,
    # fewer partial sums than the second stage has lanes; big: more than one sweep of the capped grid
    assert fresh('tiny').grad_device_ptr()[1] < 64 * 1024
    assert fresh('big').param_count > 1024 * 256 * 4


@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
@pytest.mark.parametrize('model', ALL)
def test_norm_and_coefficient_against_fp64(model, grad_scale):
    e = fresh(model)
    g = planted(e.param_count, 3)
    e.set_grads(g)
    back = e.get_grads()
    np.testing.assert_array_equal(back, g)
    norm = R.global_norm(back, grad_scale)
    max_norm = f32(norm / 3)
    e.set_grad_clip(max_norm)
    assert e.grad_clip == max_norm
    e.apply_adam(grad_scale)
    st = e.grad_clip_stats()
    print(model, grad_scale, 'norm', st['last_norm'], 'ref', norm, 'rel', abs(st['last_norm'] - norm) / norm,
          'coef', st['last_coef'], 'ref', max_norm / norm)
    assert abs(st['last_norm'] - norm) <= EPS22 * norm
    assert abs(st['last_coef'] - max_norm / norm) <= EPS22 * (max_norm / norm)
    assert st['window_max_norm'] == st['last_norm']
    assert (st['steps'], st['clipped'], st['skipped']) == (1, 1, 0)
    assert not e.step_void()


def test_two_runs_give_the_same_norm_bits():
    e = fresh('big', clip=1.0)
    g = planted(e.param_count, 3)
    norms = []
    for _ in range(2):
        e.set_grads(g)
        e.apply_adam(0.5)
        norms.append(np.float64(e.grad_clip_stats()['last_norm']).view(np.uint64))
    assert norms[0] == norms[1]


@pytest.mark.parametrize('above', ['2x', 'inf'])
@pytest.mark.parametrize('model', ALL)
def test_bitwise_twin_when_clipping_does_not_trigger(model, above):
    a, b = fresh(model, 0), fresh(model, 1)
    n = a.param_count
    top = max(R.global_norm(planted(n, 10 + k), 0.5) for k in range(3))
    a.set_grad_clip(math.inf if above == 'inf' else f32(2 * top))
    for k in range(3):
        for e in (a, b):
            e.set_grads(planted(n, 10 + k))
            e.apply_adam(0.5)
    assert_same_state(state(a), state(b))
    st = a.grad_clip_stats()
    assert (st['steps'], st['clipped'], st['skipped']) == (3, 0, 0) and st['last_coef'] == 1.0
    assert abs(st['window_max_norm'] - top) <= EPS22 * top
    assert b.grad_clip == 0.0 and b.grad_clip_stats()['steps'] == 0


@pytest.mark.parametrize('warm', [False, True], ids=['from_zero_moments', 'after_one_step'])
@pytest.mark.parametrize('model', ALL)
def test_bitwise_twin_when_clipping_triggers(model, warm):
    """g * (grad_scale * coef) is ONE fp32 product: a twin without clipping that is handed fl32(g * coef) lands on the same
    bits.  `warm`: from a non-zero Adam state - from zero moments the first step moves every weight by about lr whatever
    the gradient's scale, and a wrong coefficient would not show in P."""
    a, b = fresh(model, 0), fresh(model, 1)
    n = a.param_count
    if warm:
        for e in (a, b):
            e.set_grads(planted(n, 20))
            e.apply_adam(1.0)
    g = planted(n, 21)
    a.set_grad_clip(f32(R.global_norm(g) / 3))
    a.set_grads(g)
    a.apply_adam(1.0)
    st = a.grad_clip_stats()
    assert st['clipped'] == 1 and 0.3 < st['last_coef'] < 0.36
    b.set_grads(np.float32(g) * np.float32(st['last_coef']))
    b.apply_adam(1.0)
    sa, sb = state(a), state(b)
    assert sa[3] == (2 if warm else 1)
    assert_same_state(sa, sb)


@pytest.mark.parametrize('model', ['tiny', 'big'])
def test_clipped_steps_against_fp64_adam(model):
    """tolerances and the update-relative comparison of tests/test_gpu_parity.py::test_train_steps_match_tf_adam"""
    lr = 2e-3
    e = fresh(model)
    n = e.param_count
    p0 = e.get_params()
    p, m, v, step = p0.astype(np.float64), np.zeros(n), np.zeros(n), 0
    for k in range(3):
        g = planted(n, 30 + k) * np.float32(1 + k)
        max_norm = f32(R.global_norm(g) / 3)
        e.set_grad_clip(max_norm)
        e.set_grads(g)
        e.apply_adam(1.0)
        p, m, v, step, info = R.clipped_step(p, g, m, v, step, lr, max_norm)
        assert not info['skip'] and info['coef'] < 1
    got, gm, gv, gstep = state(e)

    def rel(x, y):
        return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-30)
    print(model, 'update', rel(got - p0, p - p0), 'abs', np.abs(got - p).max(), 'm', rel(gm, m), 'v', rel(gv, v))
    assert gstep == step == 3
    assert rel(got - p0, p - p0) < 2e-3
    assert np.abs(got - p).max() < 2e-4
    assert rel(gm, m) < 1e-4
    assert rel(gv, v) < 2e-4
    assert e.grad_clip_stats()['clipped'] == 3


@pytest.mark.parametrize('bad', [np.inf, np.nan], ids=['inf', 'nan'])
@pytest.mark.parametrize('model', ['tiny', 'big'])
def test_a_non_finite_gradient_skips_the_step(model, bad):
    a, b = fresh(model, 0, clip=math.inf), fresh(model, 1)
    n = a.param_count
    for e in (a, b):                       # a non-zero Adam state to lose
        e.set_grads(planted(n, 40))
        e.apply_adam(1.0)
    before = state(a)
    assert_same_state(before, state(b))
    g = planted(n, 41)
    g[n // 2] = bad
    a.set_grads(g)
    a.apply_adam(1.0)
    assert not a.step_void()               # skipped, not void: nothing to repeat
    assert not a.settle_step()
    assert_same_state(state(a), before)
    st = a.grad_clip_stats()
    assert (st['steps'], st['clipped'], st['skipped']) == (1, 0, 1)
    assert not math.isfinite(st['last_norm']) and math.isfinite(st['window_max_norm'])
    for e in (a, b):                       # the next step applies as if the skipped one had never been
        e.set_grads(planted(n, 42))
        e.apply_adam(1.0)
    assert_same_state(state(a), state(b))
    assert state(a)[3] == 2 and a.grad_clip_stats()['steps'] == 2
    # what the guard is for: without it the same gradient poisons the parameters for good
    b.set_grads(g)
    b.apply_adam(1.0)
    assert not np.isfinite(b.get_params()).all()
    assert np.isfinite(a.get_params()).all()


@pytest.mark.parametrize('model', ['tiny', 'big'])
def test_all_zero_gradient(model):
    e = fresh(model, clip=1.0)
    p0 = e.get_params()
    e.set_grads(np.zeros(e.param_count, np.float32))
    e.apply_adam(1.0)
    st = e.grad_clip_stats()
    assert st['last_norm'] == 0.0 and st['last_coef'] == 1.0
    assert (st['steps'], st['clipped'], st['skipped']) == (1, 0, 0)
    p, m, v, step = state(e)
    assert step == 1 and np.isfinite(p).all() and not m.any() and not v.any()
    np.testing.assert_array_equal(p, p0)


def test_a_void_step_touches_neither_parameters_nor_stats():
    import torch
    e = MAKERS['tiny']()
    n = e.param_count
    e.set_params((0.1 * np.random.RandomState(1).randn(n)).astype(np.float32))
    e.set_grad_clip(1.0)
    e.set_grads(planted(n, 50))
    e.apply_adam(1.0)
    before, stats = state(e), e.grad_clip_stats()
    assert stats['steps'] == 1 and stats['clipped'] == 1
    e.set_grads(planted(n, 51) * np.float32(2))
    e.synchronize()
    e.grad_tensor()[0] = 1.0               # the fault word of the step, as an aborted recurrence would leave it
    torch.cuda.synchronize()
    e.apply_adam(1.0)
    assert e.step_void()
    assert_same_state(state(e), before)
    assert e.grad_clip_stats() == stats
    e.close()


def test_window_reset_and_argument_checks():
    from neuralasr_amd._lib import NasrError
    e = fresh('tiny', clip=1.0)
    e.set_grads(planted(e.param_count, 60))
    e.apply_adam(1.0)
    st = e.grad_clip_stats(reset=True)
    assert st['steps'] == 1 and st['window_max_norm'] > 0
    again = e.grad_clip_stats()
    assert (again['steps'], again['clipped'], again['skipped'], again['window_max_norm']) == (0, 0, 0, 0.0)
    assert again['last_norm'] == st['last_norm'] and again['last_coef'] == st['last_coef']
    for bad in (-1.0, math.nan, -math.inf):
        with pytest.raises(NasrError, match='max_norm'):
            e.set_grad_clip(bad)
    assert e.grad_clip == 1.0
    e.set_grad_clip(0)
    assert e.grad_clip == 0.0


def config_with(tmp_path, **extra):
    lines = open(os.path.join(SAMPLES, 'toy.config')).read().splitlines()
    out = []
    for ln in lines:
        if ln.startswith('output='):
            ln = 'output=' + SAMPLES
        elif ln.startswith('model_dir='):
            ln = 'model_dir=' + str(tmp_path / 'model')
        out.append(ln)
        if ln.strip() == '[Parameters]':
            out += ['%s=%s' % kv for kv in extra.items()]
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_network_from_config_trains_with_clipping(tmp_path):
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    cfg = Config(config_with(tmp_path, max_grad_norm='0.5'), True)
    net = cfg.load_network(fortraining=True)
    assert net.engine.grad_clip == 0.5
    ds = DataSet(cfg.train_input, cfg)
    for _ in range(3):
        if not ds.has_more_batches():
            ds.reset_epoch()
        loss, _ = net.train(*ds.get_next_batch())
        assert np.isfinite(loss)
    net.save_checkpoint()                  # settles the last step
    st = net.engine.grad_clip_stats()
    assert st['steps'] == 3 and st['skipped'] == 0 and st['last_norm'] > 0
    assert np.isfinite(net.engine.get_params()).all()
    off = Config(config_with(tmp_path), True).load_network(fortraining=True)
    assert off.engine.grad_clip == 0.0


def test_the_three_calls_are_model_calls(tmp_path):
    from neuralasr_amd import _lib
    from neuralasr_amd.features import Featurizer
    f = Featurizer(8000, 13, 0)
    lib, h = f.lib, f.h
    v, st = ctypes.c_float(), _lib.ClipStats()
    calls = {'nasr_set_grad_clip': lambda: lib.nasr_set_grad_clip(h, 1.0),
             'nasr_get_grad_clip': lambda: lib.nasr_get_grad_clip(h, ctypes.byref(v)),
             'nasr_get_grad_clip_stats': lambda: lib.nasr_get_grad_clip_stats(h, ctypes.byref(st), 0)}
    for name, call in calls.items():
        assert call() == _lib.NASR_ERR_STATE, name
        msg = lib.nasr_last_error(h)
        assert name.encode() in msg and b'featurizer handle has no model' in msg
