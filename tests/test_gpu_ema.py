"""GPU: the exponential moving average of the parameters inside the Adam sweep, the swap that puts it in the parameters'
place, and the learning-rate schedule (include/nasr.h, nasr_set_ema).  Engines, planted gradients and the
bitwise helpers follow tests/test_gpu_grad_clip.py; the average is compared with the fp64 restatement of tests/ema_ref.py
under a bound derived from the arithmetic, everything else bit for bit against a twin handle."""
import ctypes
import math
import os

import numpy as np
import pytest

import ema_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')


def _tiny():
    from neuralasr_amd.engine import Engine
    return Engine(10, 8, 1, True, 'stack_reshape', 4, learning_rate=2e-3)


def _big():
    # above 2048 x 256 x 4 parameters: the stride loop of the Adam grid (and of the swap's) takes a second trip
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


def fresh(model, twin=0, ema=0.0, clip=0.0, seed=1):
    """the module's handle (model, twin) with seeded parameters, zero Adam state, `clip` set and averaging switched on
    anew with `ema` (0: off), so that the average starts at the seeded parameters with no update behind it"""
    e = _cache.get((model, twin))
    if e is None:
        e = _cache[(model, twin)] = MAKERS[model]()
    if e.ema()[2]:
        e.ema_swap()
    e.set_ema(0)
    n = e.param_count
    e.set_params((0.1 * np.random.RandomState(seed).randn(n)).astype(np.float32))
    e.set_adam_state(np.zeros(n, np.float32), np.zeros(n, np.float32), 0)
    e.set_grad_clip(clip)
    e.grad_clip_stats(reset=True)
    if ema:
        e.set_ema(ema)
    return e


def planted(n, seed):
    """random gradients with one large element at index 0 and one at the last index: a dropped head or tail shows"""
    g = (0.01 * np.random.RandomState(seed).randn(n)).astype(np.float32)
    g[0], g[-1] = 3.0, -4.0
    return g


def step(e, seed, scale=1.0):
    e.set_grads(planted(e.param_count, seed))
    e.apply_adam(scale)


def state(e):
    m, v, t = e.get_adam_state()
    return e.get_params(), m, v, t


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def assert_same_bits(x, y, name=''):
    np.testing.assert_array_equal(bits(x), bits(y), err_msg=name)


def assert_same_state(a, b):
    for x, y, name in zip(a, b, ('P', 'M', 'V')):
        assert_same_bits(x, y, name)
    assert a[3] == b[3]


def f32(x):
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------------------------- 1
def test_off_is_the_default_and_switch_on_copies_the_parameters():
    from neuralasr_amd._lib import NASR_ERR_ARG, NASR_ERR_STATE, NasrError
    e = fresh('tiny')
    big = fresh('big')
    assert big.param_count > 2048 * 256 * 4            # the Adam grid's stride loop goes round again on `big`
    assert (e.grad_device_ptr()[1] - 32) // 4 % 256 != 0      # and the last workgroup of `tiny` is ragged
    assert e.ema() == (0.0, 0, False)
    for call in (e.get_ema, e.ema_swap, lambda: e.set_ema_state(np.zeros(e.param_count, np.float32), 0)):
        with pytest.raises(NasrError) as exc:
            call()
        assert exc.value.code == NASR_ERR_STATE and 'averaging is off' in str(exc.value)
    for bad in (-1.0, 1.0, math.nan, 2.0, math.inf):
        with pytest.raises(NasrError, match='decay') as exc:
            e.set_ema(bad)
        assert exc.value.code == NASR_ERR_ARG
    assert e.ema() == (0.0, 0, False)
    for h in (e, big):
        h.set_ema(0.5)
        assert h.ema() == (0.5, 0, False)
        assert_same_bits(h.get_ema(), h.get_params())
    # a later call only changes the decay: the average and its count stay
    step(e, 3)
    before = e.get_ema()
    e.set_ema(0.25)
    assert e.ema() == (0.25, 1, False)
    assert_same_bits(e.get_ema(), before)
    # set_params does not touch the average
    e.set_params(np.zeros(e.param_count, np.float32))
    assert_same_bits(e.get_ema(), before)
    e.set_ema(0)
    assert e.ema() == (0.0, 0, False)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize('decay,N', [(0.05, 6), (0.999, 6), (0.4, 12)], ids=['constant', 'ramp', 'hand_over'])
@pytest.mark.parametrize('model', ALL)
def test_average_against_fp64(model, decay, N):
    """|E_gpu - E_ref| <= N * 2^-22 * max(|P|, |E|) per element: an update rounds twice (p - e, then the fma), each error
    is at most 2^-24 of the larger magnitude, errors do not grow because d <= 1, and the margin is a factor 2.  The
    magnitude is the largest the element took in the run (the average is a convex combination of those values)."""
    e = fresh(model, ema=decay)
    e0 = e.get_params()
    ps = []
    for k in range(N):
        step(e, 100 + k)
        ps.append(e.get_params())
    got = e.get_ema()
    want, n = R.ema_run(e0, ps, f32(decay))
    mag = np.max(np.abs(np.stack([e0] + ps).astype(np.float64)), axis=0)
    err = np.abs(got.astype(np.float64) - want)
    print(model, decay, 'max err / bound', (err / np.maximum(N * 2.0 ** -22 * mag, 1e-300)).max(),
          'moved', np.abs(want - e0).max())
    assert (err <= N * 2.0 ** -22 * mag).all()
    assert np.abs(want - e0).max() > 1e-4              # the average did move
    assert e.ema() == (f32(decay), N, False) and n == N


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize('clip', [0.0, 0.5], ids=['plain', 'clipped'])
@pytest.mark.parametrize('model', ALL)
def test_the_average_disturbs_nothing(model, clip):
    a, b = fresh(model, 0, ema=0.9, clip=clip), fresh(model, 1, clip=clip)
    for k in range(4):
        for e in (a, b):
            step(e, 200 + k, 0.5)
    assert_same_state(state(a), state(b))
    assert a.ema()[1] == 4 and b.ema() == (0.0, 0, False)
    if clip:
        assert a.grad_clip_stats()['clipped'] == 4     # the threshold did bite


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.mark.parametrize('model', ALL)
def test_one_arithmetic_on_both_paths(model):
    a, b = fresh(model, 0, ema=0.9, clip=math.inf), fresh(model, 1, ema=0.9)
    for k in range(3):
        for e in (a, b):
            step(e, 300 + k)
    assert_same_bits(a.get_ema(), b.get_ema())
    assert a.ema() == b.ema() == (f32(0.9), 3, False)
    assert a.grad_clip_stats()['steps'] == 3


# ---------------------------------------------------------------------------------------------------------------- 5
@pytest.mark.parametrize('model', ['tiny', 'big'])
def test_a_skipped_step_does_not_count(model):
    a, b = fresh(model, 0, ema=0.8, clip=math.inf), fresh(model, 1, ema=0.8, clip=math.inf)
    for e in (a, b):
        step(e, 400)
    n = a.param_count
    for bad in (np.inf, np.nan):
        before, avg, count = state(a), a.get_ema(), a.ema()
        g = planted(n, 401)
        g[n // 2] = bad
        a.set_grads(g)
        a.apply_adam(1.0)
        assert not a.step_void()
        assert_same_state(state(a), before)
        assert_same_bits(a.get_ema(), avg)
        assert a.ema() == count == (f32(0.8), 1, False)
    assert a.grad_clip_stats()['skipped'] == 2
    for e in (a, b):                                   # the next good step: as if the bad ones had never been
        step(e, 402)
    assert_same_state(state(a), state(b))
    assert_same_bits(a.get_ema(), b.get_ema())
    assert a.ema() == b.ema() == (f32(0.8), 2, False)


@pytest.mark.parametrize('clip', [0.0, 1.0], ids=['plain', 'clipped'])
def test_a_void_step_does_not_count(clip):
    import torch
    a, b = MAKERS['tiny'](), MAKERS['tiny']()
    n = a.param_count
    for e in (a, b):
        e.set_params((0.1 * np.random.RandomState(1).randn(n)).astype(np.float32))
        e.set_grad_clip(clip)
        e.set_ema(0.8)
        step(e, 500)
    before, avg, count = state(a), a.get_ema(), a.ema()
    a.set_grads(planted(n, 501) * np.float32(2))
    a.synchronize()
    a.grad_tensor()[0] = 1.0               # the fault word of the step, as an aborted recurrence would leave it
    torch.cuda.synchronize()
    a.apply_adam(1.0)
    assert a.step_void()
    assert_same_state(state(a), before)
    assert_same_bits(a.get_ema(), avg)
    assert a.ema() == count == (f32(0.8), 1, False)
    for e in (a, b):
        step(e, 502)
    assert not a.step_void()
    assert_same_state(state(a), state(b))
    assert_same_bits(a.get_ema(), b.get_ema())
    assert a.ema() == b.ema() == (f32(0.8), 2, False)
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------------------------- 6
def test_two_runs_give_the_same_average_bits():
    runs = []
    for _ in range(2):
        e = fresh('big', ema=0.4, clip=0.5)
        for k in range(3):
            step(e, 600 + k, 0.5)
        runs.append(e.get_ema())
    assert_same_bits(runs[0], runs[1])


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.mark.parametrize('model', ALL)
def test_swap_exchanges_the_contents_and_refuses_training(model):
    from neuralasr_amd._lib import NASR_ERR_STATE, NasrError
    a, b = fresh(model, 0, ema=0.7), fresh(model, 1, ema=0.7)
    for k in range(3):
        for e in (a, b):
            step(e, 700 + k)
    p, avg = a.get_params(), a.get_ema()
    assert (bits(p) != bits(avg)).any()
    a.ema_swap()
    assert a.ema() == (f32(0.7), 3, True)
    assert_same_bits(a.get_params(), avg)
    assert_same_bits(a.get_ema(), p)
    a.set_grads(planted(a.param_count, 703))           # (planting gradients is not training)
    B, T = 2, 6
    feats = np.zeros((B, T, a.cfg.feature_size), np.float32)
    refused = {'nasr_compute_grads': a.compute_grads, 'nasr_apply_adam': lambda: a.apply_adam(1.0),
               'nasr_set_ema_state': lambda: a.set_ema_state(p, 3), 'nasr_set_ema': lambda: a.set_ema(0)}
    if model in ('tiny', 'big'):                        # (the one-call step over host buffers, on the CTC LSTM handles)
        refused['nasr_train_step'] = lambda: a.train_step(feats, [T, T], np.ones((B, 1), np.int32), [1, 1])
    for name, call in refused.items():
        with pytest.raises(NasrError, match=name + ':') as exc:
            call()
        assert exc.value.code == NASR_ERR_STATE, name
    a.set_ema(0.6)                                      # changing the decay is not refused
    a.set_ema(0.7)
    a.ema_swap()
    assert a.ema() == (f32(0.7), 3, False)
    assert_same_bits(a.get_params(), p)
    assert_same_bits(a.get_ema(), avg)
    for k in range(2):                                  # the next two steps: those of the run that never swapped
        for e in (a, b):
            step(e, 710 + k)
    assert_same_state(state(a), state(b))
    assert_same_bits(a.get_ema(), b.get_ema())


def sample_batch():
    """the first batch of tests/golden/sample_set (features 9 wide), a zero column added: the width `tiny` reads"""
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        cfg = Config(config_with(__import__('pathlib').Path(d)), True)
        mfccs, labels, seq_len, labels_len = DataSet(cfg.train_input, cfg).get_next_batch()
    mfccs = np.asarray(mfccs, np.float32)
    feats = np.concatenate([mfccs, np.zeros(mfccs.shape[:2] + (1,), np.float32)], axis=2)
    labels = np.asarray(labels, np.int32).reshape(len(seq_len), -1) % 3      # (tiny has 4 classes: labels 0..2)
    return feats, labels, list(seq_len), list(labels_len)


@pytest.mark.parametrize('persistent', [None, False], ids=['default_recurrence', 'per_step'])
def test_swap_on_a_real_batch(persistent):
    """The operand images follow the swap: the logits of the swapped handle are those of a handle that was GIVEN the
    average as its parameters; and after the swap back, two real training steps are those of a run that never swapped."""
    a, b, c = _tiny(), _tiny(), _tiny()
    feats, labels, seq_len, labels_len = sample_batch()
    n = a.param_count
    p0 = (0.3 * np.random.RandomState(7).randn(n)).astype(np.float32)
    for e in (a, b, c):
        if persistent is not None:
            e.set_recurrence_mode(persistent)
        e.set_params(p0)
    for e in (a, b):
        e.set_ema(0.5)
        for _ in range(3):
            e.train_step(feats, seq_len, labels, labels_len)
    avg = a.get_ema()
    plain = a.forward(feats, seq_len)
    a.ema_swap()
    c.set_params(avg)
    got, want = a.forward(feats, seq_len), c.forward(feats, seq_len)
    assert_same_bits(got, want)
    assert (bits(got) != bits(plain)).any()            # and they are not the logits of the training parameters
    a.ema_swap()
    assert_same_bits(a.forward(feats, seq_len), plain)  # every derived image is back
    losses = {}
    for e in (a, b):
        losses[e] = [e.train_step(feats, seq_len, labels, labels_len) for _ in range(2)]
    assert_same_bits(losses[a], losses[b])
    assert_same_state(state(a), state(b))
    assert_same_bits(a.get_ema(), b.get_ema())
    assert a.ema() == b.ema() == (0.5, 5, False)
    for e in (a, b, c):
        e.close()


# ---------------------------------------------------------------------------------------------------------------- 8
@pytest.mark.parametrize('model', ALL)
def test_state_round_trip(model):
    k, N = 3, 7
    a = fresh(model, 0, ema=0.4, clip=0.5)
    for i in range(k):
        step(a, 800 + i)
    p, (m, v, t), avg, (decay, updates, _) = a.get_params(), a.get_adam_state(), a.get_ema(), a.ema()
    assert updates == k
    for i in range(k, N):
        step(a, 800 + i)
    b = fresh(model, 1, ema=decay, clip=0.5, seed=2)
    b.set_params(p)
    b.set_adam_state(m, v, t)
    b.set_ema_state(avg, updates)
    assert b.ema() == (decay, k, False)
    assert_same_bits(b.get_ema(), avg)
    for i in range(k, N):
        step(b, 800 + i)
    assert_same_state(state(a), state(b))
    assert_same_bits(a.get_ema(), b.get_ema())
    assert a.ema() == b.ema() == (decay, N, False)


# ---------------------------------------------------------------------------------------------------------------- 9
def config_with(tmp_path, name='toy.config', **keys):
    """tests/golden/sample_set/toy.config re-rooted, with [Parameters] keys set or replaced"""
    keys.setdefault('model_dir', str(tmp_path / 'model'))
    out, seen = [], False
    for ln in open(os.path.join(SAMPLES, 'toy.config')).read().splitlines():
        if ln.startswith('output='):
            ln = 'output=' + SAMPLES
        if ln.strip().startswith('['):
            seen = ln.strip() == '[Parameters]'
        if seen and ln.split('=')[0] in keys:
            continue
        out.append(ln)
        if ln.strip() == '[Parameters]':
            out += ['%s=%s' % kv for kv in keys.items()]
    p = tmp_path / name
    p.write_text('\n'.join(out) + '\n')
    return str(p)


SCHEDULE = dict(lr_warmup_steps='2', lr_decay_steps='2', lr_decay_rate='0.5')


def want_lr(s):
    return f32(R.lr_schedule(0.005, s, 2, 2, 0.5, False))


def train_steps(net, ds, steps, validate_after=None):
    for k in steps:
        if not ds.has_more_batches():
            ds.reset_epoch()
        batch = ds.get_next_batch()
        loss, _ = net.train(*batch)
        assert np.isfinite(loss)
        assert net.global_step == k
        assert net.engine.learning_rate() == want_lr(k), k      # the step size this step was enqueued with
        if k == validate_after:
            vloss, vler = net.validate(*batch)
            assert np.isfinite(vloss)
            assert net.engine.ema()[2] is False


@pytest.mark.parametrize('num_gpus', [1, 2], ids=['async_step', 'sliced_towers'])
def test_network_from_config(tmp_path, num_gpus):
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    runs = {}
    for name, validate_after in (('with_validate', 2), ('without', None)):
        d = tmp_path / name
        d.mkdir()
        cfg = Config(config_with(d, ema_decay='0.9', num_gpus=num_gpus, **SCHEDULE), True)
        net = cfg.load_network(fortraining=True)
        assert net.engine.ema() == (f32(0.9), 0, False)
        train_steps(net, DataSet(cfg.train_input, cfg), range(1, 5), validate_after)
        net.save_checkpoint()
        runs[name] = (net.engine.get_params(), net.engine.get_ema(), net.engine.ema())
        net.engine.close()
    # a validation in the middle ran on the average and left the training bits alone
    for x, y in zip(runs['with_validate'][:2], runs['without'][:2]):
        assert_same_bits(x, y)
    assert runs['with_validate'][2] == runs['without'][2] == (f32(0.9), 4, False)

    d = tmp_path / 'with_validate'
    with np.load(str(d / 'model' / 'model-4.npz')) as z:
        ck = {k: z[k] for k in z.files}
    assert int(ck['ema_updates']) == 4 and ck['ema_updates'].dtype == np.int64
    assert ck['ema_decay'].dtype == np.float32 and float(ck['ema_decay']) == f32(0.9)
    assert_same_bits(ck['ema'], runs['with_validate'][1])
    assert_same_bits(ck['params'], runs['with_validate'][0])
    assert (bits(ck['ema']) != bits(ck['params'])).any()

    # inference: the average with the key, the last iterate without it
    model_dir = str(d / 'model')
    inf = Config(config_with(d, 'inf.config', ema_decay='0.9', num_gpus=num_gpus, model_dir=model_dir), True).load_network(False)
    assert inf.engine.ema() == (0.0, 0, False)          # no second image on an inference handle
    assert_same_bits(inf.engine.get_params(), ck['ema'])
    inf.engine.close()
    last = Config(config_with(d, 'last.config', num_gpus=num_gpus, model_dir=model_dir), True).load_network(False)
    assert_same_bits(last.engine.get_params(), ck['params'])
    last.engine.close()

    # a resumed run continues the average and the schedule from the checkpoint's step
    cfg = Config(config_with(d, 'resume.config', ema_decay='0.9', num_gpus=num_gpus, model_dir=model_dir, start_step=1,
                             **SCHEDULE), True)
    net = cfg.load_network(fortraining=True)
    assert net.global_step == 4
    assert net.engine.ema() == (f32(0.9), 4, False)
    assert_same_bits(net.engine.get_ema(), ck['ema'])
    assert_same_bits(net.engine.get_params(), ck['params'])
    train_steps(net, DataSet(cfg.train_input, cfg), [5])
    assert net.engine.ema()[1] == 5
    net.engine.close()


def test_a_checkpoint_without_the_average_starts_it_at_the_restored_parameters(tmp_path):
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    cfg = Config(config_with(tmp_path, num_gpus=1), True)
    net = cfg.load_network(fortraining=True)
    ds = DataSet(cfg.train_input, cfg)
    net.train(*ds.get_next_batch())
    net.save_checkpoint()
    params = net.engine.get_params()
    net.engine.close()
    with np.load(str(tmp_path / 'model' / 'model-1.npz')) as z:
        assert not {'ema', 'ema_updates', 'ema_decay'} & set(z.files)       # the arrays of a run without the key: as ever
    cfg = Config(config_with(tmp_path, 'resume.config', ema_decay='0.9', num_gpus=1, start_step=1), True)
    net = cfg.load_network(fortraining=True)
    assert net.engine.ema() == (f32(0.9), 0, False)
    assert_same_bits(net.engine.get_ema(), params)
    net.engine.close()
    inf = Config(config_with(tmp_path, 'inf.config', ema_decay='0.9', num_gpus=1), True).load_network(False)
    assert_same_bits(inf.engine.get_params(), params)                         # (warns, and uses the parameters)
    inf.engine.close()


def test_a_stream_session_of_a_training_network_runs_on_the_average(tmp_path):
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    cfg = Config(config_with(tmp_path, ema_decay='0.5', num_gpus=1, network='networks.lstm_ctc_net.LstmCTCNet'), True)
    net = cfg.load_network(fortraining=True)
    ds = DataSet(cfg.train_input, cfg)
    for _ in range(2):
        net.train(*ds.get_next_batch())
    rec = net.stream(1)                                 # (settles the last step)
    p, avg = net.engine.get_params(), net.engine.get_ema()
    real_feed, seen = net.engine.stream_feed, []

    def spy(f, n):
        seen.append((net.engine.ema()[2], real_feed(f, n)))
        return seen[-1][1]
    net.engine.stream_feed = spy
    x = np.random.RandomState(9).randn(24, cfg.feature_size).astype(np.float32)
    for t in range(0, 24, 8):
        rec.feed([x[t:t + 8]])
        assert net.engine.ema()[2] is False             # between the feeds the training parameters are back
    del net.engine.stream_feed
    assert [live for live, _ in seen] == [True, True, True]
    got = np.concatenate([lg[:8, 0] for _, lg in seen])
    net.engine.ema_swap()
    want = net.engine.forward(x[None], [24])[:, 0]      # the whole utterance on the average
    net.engine.ema_swap()
    np.testing.assert_allclose(got, want, atol=1e-4, rtol=0)     # (a chunked utterance's logits: tests/test_gpu_stream.py's bound)
    rec.close()
    assert_same_bits(net.engine.get_params(), p)
    assert_same_bits(net.engine.get_ema(), avg)
    assert net.engine.ema() == (0.5, 2, False)
    net.engine.close()


# --------------------------------------------------------------------------------------------------------------- 10
def test_the_new_calls_are_model_calls():
    from neuralasr_amd import _lib
    from neuralasr_amd.features import Featurizer
    f = Featurizer(8000, 13, 0)
    lib, h = f.lib, f.h
    v, n, live = ctypes.c_float(), ctypes.c_int64(), ctypes.c_int()
    buf = np.zeros(4, np.float32)
    fp = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    calls = {'nasr_set_ema': lambda: lib.nasr_set_ema(h, 0.5),
             'nasr_get_ema': lambda: lib.nasr_get_ema(h, ctypes.byref(v), ctypes.byref(n), ctypes.byref(live)),
             'nasr_get_ema_state': lambda: lib.nasr_get_ema_state(h, fp, 4, ctypes.byref(n)),
             'nasr_set_ema_state': lambda: lib.nasr_set_ema_state(h, fp, 4, 0),
             'nasr_ema_swap': lambda: lib.nasr_ema_swap(h),
             'nasr_get_learning_rate': lambda: lib.nasr_get_learning_rate(h, ctypes.byref(v))}
    for name, call in calls.items():
        assert call() == _lib.NASR_ERR_STATE, name
        msg = lib.nasr_last_error(h)
        assert name.encode() in msg and b'featurizer handle has no model' in msg


def test_learning_rate_getter():
    e = fresh('tiny')
    assert e.learning_rate() == f32(2e-3)
    e.set_learning_rate(1e-3)
    assert e.learning_rate() == f32(1e-3)
    e.set_learning_rate(2e-3)
