"""Resampling's host side, no GPU: the library's kaiser_best table and lengths against resampy 0.2's and librosa's
formulas, read_wav_native against read_wav, and the sanity of the fp64 restatement (tests/resample_ref.py) itself."""
import numpy as np
import pytest

import resample_ref as RR
from neuralasr_amd import features
from test_mfcc_host import riff

PAIRS = [(16000, 8000), (48000, 16000), (44100, 16000), (22050, 16000), (11025, 8000), (22050, 8000), (96000, 8000),
         (8000, 16000), (8000, 44100), (16000, 16000)]


def test_table_matches_the_scipy_construction():
    lib_t = features.resample_filter()
    ref = RR.table()
    assert lib_t.shape == ref.shape == (32769,)
    assert np.abs(lib_t - ref).max() <= 1e-12
    assert lib_t[0] == pytest.approx(RR.ROLLOFF, abs=1e-15)


@pytest.mark.parametrize('sr_orig,sr_new', PAIRS)
def test_lengths_are_librosas_and_resampys(sr_orig, sr_new):
    ns = list(range(1, 200)) + [441, 882, 1000, 4410, 44100, 160000, 441 * 1001, 10 ** 6 + 7, 30 * 44100 + 13]
    zero_tail = 0
    for n in ns:
        n_samples, n_out = RR.lengths(n, sr_orig, sr_new)
        if sr_orig == sr_new:
            n_samples = n_out = n
        if n_out < 1:
            with pytest.raises(ValueError, match='give no sample'):
                features.resample_length(n, sr_orig, sr_new)
            continue
        assert features.resample_length(n, sr_orig, sr_new) == (n_samples, n_out), n
        assert n_samples - n_out in (0, 1)
        zero_tail += n_samples - n_out
    if sr_orig != sr_new and sr_new % sr_orig:
        assert zero_tail > 0                        # the grid has lengths that fix_length pads


def test_too_short_and_bad_rates_are_errors():
    from neuralasr_amd import _lib
    lib = _lib.load()
    assert lib.nasr_resample_length(44100, 16000, 2, None) < 0      # int(2 * 0.3628) = 0: resampy raises
    assert lib.nasr_resample_length(44100, 16000, 3, None) == 2     # one filtered sample plus one zero
    assert lib.nasr_resample_length(0, 16000, 100, None) < 0
    assert lib.nasr_resample_length(16000, -1, 100, None) < 0
    assert lib.nasr_resample_length(16000, 8000, 0, None) < 0
    with pytest.raises(ValueError):
        features.resample_length(1, 96000, 8000)
    with pytest.raises(ValueError):
        RR.resample_f(np.zeros(11, np.float32), 96000, 8000)


def test_read_wav_native_is_read_wav(tmp_path):
    rng = np.random.default_rng(5)
    i16 = rng.integers(-32768, 32768, size=(50, 2)).astype('<i2')
    u8 = rng.integers(0, 256, size=40).astype(np.uint8)
    v24 = b''.join(int(v).to_bytes(4, 'little', signed=True)[:3] for v in rng.integers(-(1 << 23), 1 << 23, size=30))
    i32 = rng.integers(-2 ** 31, 2 ** 31, size=30).astype('<i4')
    f32 = rng.standard_normal(30).astype('<f4')
    f64 = rng.standard_normal(30).astype('<f8')
    files = [
        (riff(tmp_path / 'a.wav', 1, 2, 44100, 16, i16.tobytes()), 44100),
        (riff(tmp_path / 'b.wav', 0xFFFE, 2, 48000, 16, i16.tobytes(), extensible_sub=1), 48000),
        (riff(tmp_path / 'c.wav', 1, 1, 8000, 8, u8.tobytes()), 8000),
        (riff(tmp_path / 'd.wav', 1, 1, 22050, 24, v24), 22050),
        (riff(tmp_path / 'e.wav', 1, 1, 16000, 32, i32.tobytes()), 16000),
        (riff(tmp_path / 'f.wav', 3, 1, 96000, 32, f32.tobytes()), 96000),
        (riff(tmp_path / 'g.wav', 3, 1, 11025, 64, f64.tobytes()), 11025),
        (riff(tmp_path / 'h.wav', 0xFFFE, 1, 16000, 32, f32.tobytes(), extensible_sub=3), 16000),
    ]
    for path, rate in files:
        y, r = features.read_wav_native(path)
        want = features.read_wav(path, rate)
        assert r == rate and y.dtype == np.float32 and y.tobytes() == want.tobytes(), path
    with pytest.raises(ValueError, match='resampling is not supported'):
        features.read_wav(files[0][0], 8000)


def test_register_is_the_sequential_loop():
    for sr_orig, sr_new in [(44100, 16000), (22050, 16000), (8000, 44100)]:
        ratio = float(sr_new) / sr_orig
        tr = RR.register(600000, ratio)
        inc, t, loop = 1.0 / ratio, 0.0, np.empty(600000)
        for i in range(600000):
            loop[i] = t
            t += inc
        assert tr.tobytes() == loop.tobytes()


def test_restatement_pass_and_stop_band():
    sr, n = 16000, 16000
    t = np.arange(n) / sr
    for f, lo, hi in [(3500.0, 0.999, 1.001), (4200.0, 0.0, 1e-7)]:
        y = RR.resample_f(np.sin(2 * np.pi * f * t), sr, 8000, acc='f64')
        assert y.size == 8000
        amp = np.sqrt(2) * np.sqrt(np.mean(y[500:-500] ** 2))
        assert lo <= amp <= hi, (f, amp)


def test_restatement_accumulations_agree():
    rng = np.random.default_rng(2)
    x = (np.round(0.3 * rng.standard_normal(1500) * 32767) / 32768).astype(np.float32)
    a = RR.resample_f(x, 44100, 16000, acc='f32')
    b = RR.resample_f(x, 44100, 16000, acc='f64')
    assert a.dtype == np.float32 and a.size == 544
    assert np.abs(a - b).max() <= 2e-6
