"""GPU: the MFCC front end (kernels csrc/mfcc.hip, handle csrc/nasr_fz.hip) against the fp64 restatement of tests/mfcc_ref.py, for the feature shapes of
the reference configs and the edge cases, plus batch invariance, run-to-run equality and the featurizer handle's
refusal of model calls."""
import ctypes

import numpy as np
import pytest

import mfcc_ref as R

pytestmark = pytest.mark.gpu

TOL_MAX, TOL_MEAN = 1e-4, 1e-6


def speech_like(n, sr, seed, level=0.3):
    """Harmonics of a wandering pitch under a syllable-rate envelope, plus noise, quantised to int16 (float32 x/32768)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = 110 + 40 * np.sin(2 * np.pi * 0.7 * t + rng.uniform(0, 6)) + 15 * np.sin(2 * np.pi * 3.1 * t)
    phase = 2 * np.pi * np.cumsum(f0) / sr
    x = np.zeros(n)
    for h in range(1, 30):
        if h * 160 > sr / 2:
            break
        x += np.sin(h * phase + rng.uniform(0, 6)) / h ** 1.2
    env = 0.55 + 0.45 * np.sin(2 * np.pi * 4.0 * t + rng.uniform(0, 6))
    x = x * env / 3 + 0.05 * rng.standard_normal(n)
    q = np.clip(np.round(x * level * 32767), -32768, 32767).astype(np.int16)
    return q.astype(np.float32) / np.float32(32768)


def check(got, audio, sr, nc, numcep):
    want, _ = R.features(audio, sr, nc, numcep)
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want)
    return err.max(), err.mean()


@pytest.fixture(scope='module')
def fz():
    from neuralasr_amd.features import Featurizer
    made = {}

    def get(sr, numcep, nc, **kw):
        key = (sr, numcep, nc, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = Featurizer(sr, numcep, nc, **kw)
        return made[key]
    yield get
    for f in made.values():
        f.close()


@pytest.mark.parametrize('sr,numcep,nc', [(16000, 26, 10), (8000, 13, 0), (8000, 40, 10)])
def test_reference_config_shapes(fz, sr, numcep, nc):
    f = fz(sr, numcep, nc)
    audios = [speech_like(int(sr * s), sr, seed) for seed, s in enumerate((1.0, 2.37, 0.61, 3.2))]
    feats, stats = f.compute(audios, return_stats=True)
    for a, g, (mean, std) in zip(audios, feats, stats):
        assert g.shape[0] == f.frames(a.size) == R.num_frames(a.size, sr)
        mx, mn = check(g, a, sr, nc, numcep)
        assert mx <= TOL_MAX and mn <= TOL_MEAN, (mx, mn)
        _, (rm, rs) = R.features(a, sr, nc, numcep)
        assert abs(mean - rm) <= 1e-4 * abs(rs) and abs(std - rs) <= 1e-4 * rs


@pytest.mark.parametrize('case', ['short', 'one_frame', 'leading_silence', 'all_zero', 'quiet'])
def test_edge_cases(fz, case):
    sr, numcep, nc = 16000, 26, 10
    if case == 'short':
        a = speech_like(250, sr, 7)
    elif case == 'one_frame':
        a = speech_like(400, sr, 8)
    elif case == 'leading_silence':
        a = np.concatenate([np.zeros(8000, np.float32), speech_like(16000, sr, 9)])
    elif case == 'all_zero':
        a = np.zeros(3000, np.float32)
    else:
        a = speech_like(16000, sr, 10, level=0.001)        # about -60 dB
    g = fz(sr, numcep, nc).compute([a])[0]
    mx, _ = check(g, a, sr, nc, numcep)
    assert g.shape[0] == R.num_frames(a.size, sr)
    assert mx <= TOL_MAX, mx


def test_all_zero_filters_sit_at_eps(fz):
    """numcontext 0: every frame of digital silence is c0 = log(eps) and a DCT of a constant, the same for every frame."""
    g = fz(8000, 13, 0).compute([np.zeros(2000, np.float32)])[0]
    mx, _ = check(g, np.zeros(2000, np.float32), 8000, 0, 13)
    assert mx <= TOL_MAX
    assert np.all(g == g[0])


def test_22k_frames_truncated_to_nfft(fz):
    sr = 22050
    assert R.frame_params(sr)[0] > 512
    a = speech_like(int(1.3 * sr), sr, 11)
    g = fz(sr, 13, 0).compute([a])[0]
    mx, mn = check(g, a, sr, 0, 13)
    assert mx <= TOL_MAX and mn <= TOL_MEAN, (mx, mn)


def test_long_utterance_grows_buffers(fz):
    sr = 16000
    f = fz(sr, 26, 10)
    f.compute([speech_like(4000, sr, 1)])
    a = speech_like(35 * sr, sr, 12)
    g = f.compute([a])[0]
    mx, mn = check(g, a, sr, 10, 26)
    assert mx <= TOL_MAX and mn <= TOL_MEAN, (mx, mn)


def test_ragged_batch_is_bitwise_per_utterance_and_repeatable(fz):
    sr = 8000
    f = fz(sr, 40, 10)
    audios = [speech_like(n, sr, 20 + i) for i, n in enumerate((100, 200, 8000, 12345, 640, 30001, 201))]
    batch = f.compute(audios)
    again = f.compute(audios)
    for i, a in enumerate(audios):
        one = f.compute([a])[0]
        assert np.array_equal(batch[i], one), i
        assert np.array_equal(batch[i], again[i]), i
    small = fz(sr, 40, 10, max_samples=10000).compute(audios)      # split over several library calls
    for b, s in zip(batch, small):
        assert np.array_equal(b, s)


def test_bad_arguments(fz):
    from neuralasr_amd import _lib
    f = fz(8000, 13, 0)
    with pytest.raises(ValueError):
        f.compute([np.zeros(0, np.float32)])
    a = speech_like(4000, 8000, 3)
    out = np.empty((f.frames(a.size) + 1, 13), np.float32)
    off = np.array([0, a.size], np.int64)
    rc = f.lib.nasr_featurize(f.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                              off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1,
                              out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.shape[0], None)
    assert rc == _lib.NASR_ERR_ARG and b'frames' in f.lib.nasr_last_error(f.h)
    from neuralasr_amd.features import Featurizer
    with pytest.raises(_lib.NasrError, match='numcep'):
        Featurizer(8000, 129, 0)


def test_model_calls_on_a_featurizer_handle(fz):
    from neuralasr_amd import _lib
    f = fz(8000, 13, 0)
    lib, h = f.lib, f.h
    fp = ctypes.POINTER(ctypes.c_float)
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data_as(fp)
    i32 = np.ones(4, np.int32)
    ip = i32.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    i64 = ctypes.c_int64()
    calls = {
        'nasr_param_count': lambda: lib.nasr_param_count(h),
        'nasr_num_tensors': lambda: lib.nasr_num_tensors(h),
        'nasr_set_params': lambda: lib.nasr_set_params(h, p, 0),
        'nasr_get_params': lambda: lib.nasr_get_params(h, p, 0),
        'nasr_set_learning_rate': lambda: lib.nasr_set_learning_rate(h, 1e-3),
        'nasr_logit_frames': lambda: lib.nasr_logit_frames(h, 4),
        'nasr_train_step': lambda: lib.nasr_train_step(h, p, ip, ip, ip, 1, 2, 1, p),
        'nasr_forward': lambda: lib.nasr_forward(h, p, ip, 1, 2, p),
        'nasr_loss': lambda: lib.nasr_loss(h, p, ip, ip, ip, 1, 2, 1, p, p),
        'nasr_greedy_decode': lambda: lib.nasr_greedy_decode(h, p, ip, 1, 2, ip, ip),
        'nasr_upload_batch': lambda: lib.nasr_upload_batch(h, p, ip, ip, ip, 1, 2, 1),
        'nasr_compute_grads': lambda: lib.nasr_compute_grads(h),
        'nasr_apply_adam': lambda: lib.nasr_apply_adam(h, 1.0),
        'nasr_get_loss': lambda: lib.nasr_get_loss(h, p),
        'nasr_resident_frames': lambda: lib.nasr_resident_frames(h, ctypes.byref(i64)),
        'nasr_set_profiling': lambda: lib.nasr_set_profiling(h, 1),
        'nasr_set_graph_mode': lambda: lib.nasr_set_graph_mode(h, 0),
        'nasr_get_recurrence_mode': lambda: lib.nasr_get_recurrence_mode(h),
        'nasr_set_recurrence_mode': lambda: lib.nasr_set_recurrence_mode(h, 0),
        'nasr_comm_size': lambda: lib.nasr_comm_size(h),
        'nasr_comm_allreduce_grads': lambda: lib.nasr_comm_allreduce_grads(h),
        'nasr_wavenet_bn_count': lambda: lib.nasr_wavenet_bn_count(h),
    }
    for name, call in calls.items():
        assert call() == _lib.NASR_ERR_STATE, name
    assert not lib.nasr_grad_device_ptr(h)
    assert lib.nasr_synchronize(h) == _lib.NASR_OK
    g = f.compute([speech_like(2000, 8000, 4)])[0]          # the handle still works
    assert g.shape == (R.num_frames(2000, 8000), 13)
