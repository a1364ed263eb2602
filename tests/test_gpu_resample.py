"""GPU: resampling to the config rate (csrc/resample.hip), librosa.load(wav, sr=sr)'s step of the reference's
utils.py:25, against the fp64 restatement of tests/resample_ref.py fed the library's own filter table: the resampled
audio bit for bit, batch invariance across rates, and the features of resampled audio."""
import ctypes

import numpy as np
import pytest

import mfcc_ref as R
import resample_ref as RR
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu

PAIRS = [(16000, 8000), (48000, 16000), (44100, 16000), (22050, 16000), (11025, 8000), (22050, 8000), (96000, 8000),
         (8000, 16000)]


@pytest.fixture(scope='module')
def fz():
    from neuralasr_amd.features import Featurizer
    made = {}

    def get(sr, numcep=13, nc=0, **kw):
        key = (sr, numcep, nc, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = Featurizer(sr, numcep, nc, **kw)
        return made[key]
    yield get
    for f in made.values():
        f.close()


@pytest.fixture(scope='module')
def table():
    from neuralasr_amd.features import resample_filter
    return resample_filter()


def lengths_for(sr_orig, sr_new):
    """the shortest length with one filtered sample, lengths with and without fix_length's zero, and speech lengths."""
    n1 = next(n for n in range(1, 100) if RR.lengths(n, sr_orig, sr_new)[1] >= 1)
    tails = [n for n in range(n1, n1 + 400) if RR.lengths(n, sr_orig, sr_new)[0] > RR.lengths(n, sr_orig, sr_new)[1]]
    exact = [n for n in range(n1, n1 + 400) if RR.lengths(n, sr_orig, sr_new)[0] == RR.lengths(n, sr_orig, sr_new)[1]]
    return [n1] + tails[:2] + exact[:2] + [int(0.37 * sr_orig) + 1, int(1.3 * sr_orig)]


@pytest.mark.parametrize('sr_orig,sr_new', PAIRS)
def test_resampled_audio_is_bitwise_the_restatement(fz, table, sr_orig, sr_new):
    lens = lengths_for(sr_orig, sr_new)
    audios = [speech_like(n, sr_orig, 10 + i) for i, n in enumerate(lens)]
    got = fz(sr_new).resample(audios, [sr_orig] * len(audios))
    for n, a, g in zip(lens, audios, got):
        want = RR.resample(a, sr_orig, sr_new, win=table)
        assert g.dtype == np.float32 and g.shape == want.shape, n
        bad = np.nonzero(g.view(np.int32) != want.view(np.int32))[0]
        assert bad.size == 0, (n, bad[:8], g[bad[:8]], want[bad[:8]])
        n_samples, n_out = RR.lengths(n, sr_orig, sr_new)
        assert g.size == n_samples and np.all(g[n_out:] == 0)


def test_long_utterance_follows_the_drifting_register(fz, table):
    """31 s at 44.1 kHz: the sequential register drifts from exact positions, so outputs where a position crosses an
    integer differ from exact-rational interpolation; the kernel must follow the register."""
    a = speech_like(31 * 44100 + 17, 44100, 7)
    got = fz(16000).resample([a], [44100])[0]
    want = RR.resample(a, 44100, 16000, win=table)
    assert got.shape == want.shape
    bad = np.nonzero(got.view(np.int32) != want.view(np.int32))[0]
    assert bad.size == 0, (bad.size, bad[:8])


def test_mixed_rate_batch_is_bitwise_each_alone(fz):
    f = fz(16000, 26, 10)
    rates = [44100, 16000, 8000, 48000, 22050, 16000, 96000]
    audios = [speech_like(int(r * (0.6 + 0.17 * i)) + i, r, 40 + i) for i, r in enumerate(rates)]
    batch = f.resample(audios, rates)
    for a, r, b in zip(audios, rates, batch):
        alone = f.resample([a], [r])[0]
        assert b.tobytes() == alone.tobytes()
        if r == 16000:
            assert b.tobytes() == a.tobytes()
    feats, stats = f.compute(audios, return_stats=True, rates=rates)
    for a, r, x, s in zip(audios, rates, feats, stats):
        xa, sa = f.compute([a], return_stats=True, rates=[r])
        assert x.tobytes() == xa[0].tobytes() and s == sa[0]
    same = [a for a, r in zip(audios, rates) if r == 16000]
    assert all(x.tobytes() == y.tobytes() for x, y in
               zip(f.compute(same, rates=[16000] * len(same)), f.compute(same)))


def test_packing_counts_native_and_resampled_samples(fz):
    from neuralasr_amd.features import Featurizer
    rates = [48000, 44100, 8000, 16000]
    audios = [speech_like(int(0.5 * r) + 3, r, 60 + i) for i, r in enumerate(rates)]
    want = fz(16000, 13, 0).compute(audios, rates=rates)
    small = Featurizer(16000, 13, 0, max_samples=30000)
    try:
        got = small.compute(audios, rates=rates)
    finally:
        small.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want))


@pytest.mark.parametrize('sr,numcep,nc', [(16000, 26, 10), (8000, 13, 0)])
def test_features_of_resampled_audio(fz, table, sr, numcep, nc):
    f = fz(sr, numcep, nc)
    rates = [44100, 48000, 22050, sr, 11025]
    audios = [speech_like(int(r * (0.9 + 0.2 * i)), r, 80 + i) for i, r in enumerate(rates)]
    feats = f.compute(audios, rates=rates)
    restated = [RR.resample(a, r, sr, win=table) for a, r in zip(audios, rates)]
    again = f.compute(restated)
    for x, y, ra in zip(feats, again, restated):
        assert x.tobytes() == y.tobytes()
        want, _ = R.features(ra, sr, nc, numcep)
        assert x.shape == want.shape and np.abs(x.astype(np.float64) - want).max() <= 1e-4


def test_times_include_the_resampling_kernel(fz):
    f = fz(16000)
    a = speech_like(44100 * 2, 44100, 3)
    f.compute([a], rates=[44100])
    h2d, k, d2h = f.times()
    assert k > 0 and h2d > 0 and d2h > 0
    f.resample([a], [44100])
    assert f.times()[1] > 0


def test_errors(fz):
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine
    f = fz(8000)
    ok = speech_like(4000, 16000, 1)
    short = np.zeros(11, np.float32)          # int(11 * 8000 / 96000) = 0
    with pytest.raises(ValueError, match='utterance 1'):
        f.compute([ok, short], rates=[16000, 96000])
    with pytest.raises(ValueError, match='utterance 1'):
        f.resample([ok, ok], [16000, 0])
    with pytest.raises(ValueError, match='utterance 0'):
        f.compute([ok], rates=[-8000])

    fp, i64p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    flat = np.concatenate([ok, short])
    off = np.array([0, ok.size, flat.size], np.int64)
    out = np.zeros(8192, np.float32)
    ms = np.zeros(4, np.float64)

    def call(h, rates, featurize):
        r = np.array(rates, np.int32)
        args = (h, flat.ctypes.data_as(fp), off.ctypes.data_as(i64p), r.ctypes.data_as(i32p), 2, out.ctypes.data_as(fp))
        if featurize:
            return f.lib.nasr_featurize_rates(*args, 10, ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return f.lib.nasr_resample(*args, 2000 + 1)

    for featurize in (False, True):
        assert call(f.h, [16000, 96000], featurize) == _lib.NASR_ERR_ARG
        assert b'utterance 1' in f.lib.nasr_last_error(f.h)
        assert call(f.h, [0, 16000], featurize) == _lib.NASR_ERR_ARG
        msg = f.lib.nasr_last_error(f.h)
        assert b'utterance 0' in msg and b'must be > 0' in msg
    assert call(f.h, [16000, 16000], False) == _lib.NASR_ERR_ARG      # out_len is not the resampled total
    assert b'out_len' in f.lib.nasr_last_error(f.h)

    eng = Engine(8, 16, 1, True, 'stack_reshape', 5, device_id=0)
    try:
        for featurize in (False, True):
            assert call(eng.h, [16000, 16000], featurize) == _lib.NASR_ERR_STATE
            assert b'not a featurizer handle' in f.lib.nasr_last_error(eng.h)
    finally:
        eng.close()
