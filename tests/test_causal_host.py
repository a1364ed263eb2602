"""Host: the causal normalisation.  The C ABI of the two new nasr_mfcc_cfg fields and what cfg_ok refuses,
the config keys, tests/causal_ref.py against values worked by hand, and its stream simulator - fed one sample at a time,
in 37-sample pieces, in step-aligned and in random pieces - against the offline rule, bit for bit.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import causal_ref as CR
import mfcc_ref as R
from test_gpu_mfcc import speech_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 8000
FLEN, FSTEP = R.frame_params(SR)          # 200, 80


# ------------------------------------------------------------------------------------------------------------ ABI
def _cfg(**kw):
    from neuralasr_amd import _lib
    base = dict(samplerate=SR, numcep=13, numcontext=0, nfilt=128, nfft=512, winlen=0.025, winstep=0.01, preemph=0.97,
                ceplifter=22, append_energy=1, kind=0, deltas=0)
    base.update(kw)
    return _lib.MfccCfg(**base)


def test_cfg_layout_matches_the_header(tmp_path):
    from neuralasr_amd import _lib
    gcc = shutil.which('gcc')
    if not gcc:
        pytest.skip('no gcc')
    src = tmp_path / 'abi.c'
    src.write_text(r'''
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "nasr.h"
int main(void) {
  nasr_mfcc_cfg cfg;
  memset(&cfg, 0, sizeof cfg);
  cfg.samplerate = 8000; cfg.numcep = 13; cfg.nfilt = 128; cfg.nfft = 512; cfg.winlen = 0.025; cfg.winstep = 0.01;
  cfg.preemph = 0.97f;
  int zeroed = nasr_mfcc_width(&cfg);
  cfg.norm = 1; cfg.norm_min_frames = 50;
  int causal = nasr_mfcc_width(&cfg);
  cfg.norm_min_frames = 0;
  printf("%zu %zu %zu %zu %d %d %d\n", sizeof(nasr_mfcc_cfg), offsetof(nasr_mfcc_cfg, deltas), offsetof(nasr_mfcc_cfg, norm),
         offsetof(nasr_mfcc_cfg, norm_min_frames), zeroed, causal, nasr_mfcc_width(&cfg));
  return 0;
}
''')
    exe = tmp_path / 'abi'
    libdir = os.path.dirname(_lib.LIB_PATH)
    cmd = [gcc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe),
           '-L', libdir, '-l:libnasr.so', '-Wl,-rpath,' + libdir, '-Wl,-rpath,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    size, off_deltas, off_norm, off_min, zeroed, causal, bad = (int(x) for x in out.stdout.split())
    assert size == ctypes.sizeof(_lib.MfccCfg)
    assert off_norm == _lib.MfccCfg.norm.offset and off_min == _lib.MfccCfg.norm_min_frames.offset
    assert off_deltas == _lib.MfccCfg.deltas.offset
    assert off_norm == off_deltas + 4 and off_min == off_norm + 4          # appended behind deltas, in this order
    assert zeroed == 13 and causal == 13 and bad < 0


def test_a_zeroed_cfg_means_what_it_meant():
    from neuralasr_amd import _lib
    lib = _lib.load()
    cfg = _cfg()
    assert (cfg.norm, cfg.norm_min_frames) == (0, 0)
    assert lib.nasr_mfcc_frames(ctypes.byref(cfg), 4000) == R.num_frames(4000, SR)
    assert lib.nasr_mfcc_width(ctypes.byref(cfg)) == 13
    # norm_min_frames is read only under the causal rule
    assert lib.nasr_mfcc_width(ctypes.byref(_cfg(norm=0, norm_min_frames=-7))) == 13
    assert lib.nasr_mfcc_width(ctypes.byref(_cfg(norm=0, deltas=2))) == 39


def test_width_and_frames_refuse_bad_norm_fields():
    from neuralasr_amd import _lib
    lib = _lib.load()

    def width(**kw):
        return lib.nasr_mfcc_width(ctypes.byref(_cfg(**kw)))

    def frames(**kw):
        return lib.nasr_mfcc_frames(ctypes.byref(_cfg(**kw)), 4000)
    for good in (dict(norm=1, norm_min_frames=1), dict(norm=1, norm_min_frames=1000),
                 dict(norm=1, norm_min_frames=50, kind=1, numcep=8, nfilt=8)):
        assert width(**good) == good.get('numcep', 13), good
        assert frames(**good) == R.num_frames(4000, SR), good
    for bad in (dict(norm=2, norm_min_frames=50), dict(norm=-1, norm_min_frames=50), dict(norm=1, norm_min_frames=0),
                dict(norm=1), dict(norm=1, norm_min_frames=1001), dict(norm=1, norm_min_frames=-1),
                dict(norm=1, norm_min_frames=50, deltas=1), dict(norm=1, norm_min_frames=50, deltas=2)):
        assert width(**bad) < 0 and width(**bad) == _lib.NASR_ERR_ARG, bad
        assert frames(**bad) == _lib.NASR_ERR_ARG, bad


def test_create_names_the_field():
    """the argument checks run before the device is opened: the messages do not need a GPU"""
    from neuralasr_amd import _lib
    lib = _lib.load()
    for kw, text in ((dict(norm=2, norm_min_frames=50), 'norm must be 0'),
                     (dict(norm=1, norm_min_frames=0), r'norm_min_frames must be in \[1,1000\]'),
                     (dict(norm=1, norm_min_frames=1001), 'norm_min_frames'),
                     (dict(norm=1, norm_min_frames=50, deltas=1), 'deltas = 0.*look')):
        h = ctypes.c_void_p()
        rc = lib.nasr_create_featurizer(ctypes.byref(_cfg(**kw)), 0, None, ctypes.byref(h))
        assert rc == _lib.NASR_ERR_ARG and not h
        with pytest.raises(_lib.NasrError, match=text):
            _lib.check(lib, None, rc)


def test_featurizer_python_arguments():
    from neuralasr_amd import features
    cfg = features._cfg(SR, 13, 2, 128, 512)
    assert (cfg.norm, cfg.norm_min_frames) == (0, 0)
    cfg = features._cfg(SR, 13, 2, 128, 512, normalization='causal')
    assert (cfg.norm, cfg.norm_min_frames) == (1, 50)
    cfg = features._cfg(SR, 8, 0, 128, 512, 'logfbank', 0, 'causal', 3)
    assert (cfg.kind, cfg.nfilt, cfg.norm, cfg.norm_min_frames) == (1, 8, 1, 3)
    with pytest.raises(ValueError, match='normalization'):
        features._cfg(SR, 13, 0, 128, 512, normalization='running')
    with pytest.raises(ValueError, match='norm_min_frames'):
        features._cfg(SR, 13, 0, 128, 512, norm_min_frames=50)


# --------------------------------------------------------------------------------------------------------- config
def _config(tmp_path, extra=''):
    from neuralasr_amd.config import Config
    p = tmp_path / 'c.config'
    p.write_text('[Parameters]\nsamplerate=8000\nnumcep=13\nnumcontext=2\nlabel_context=0\nbatch_size=2\nepochs=1\n'
                 'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
                 'network=networks.lstm_ctc_net.LstmCTCNet\n%s[Train]\n[Test]\ninput=%s\n[MFCC Featurizer]\n'
                 % (tmp_path / 'model', extra, tmp_path / 'test.scp'))
    return Config(str(p))


def test_config_keys(tmp_path):
    from neuralasr_amd.utils import normalization_of
    c = _config(tmp_path)
    assert (c.normalization, c.norm_min_frames, c.feature_size) == ('utterance', None, 65)
    assert normalization_of(c) == dict(normalization='utterance', norm_min_frames=None)
    c = _config(tmp_path, 'normalization=causal\n')
    assert (c.normalization, c.norm_min_frames, c.feature_size) == ('causal', 50, 65)
    c = _config(tmp_path, 'normalization=causal\nnorm_min_frames=3\n')
    assert normalization_of(c) == dict(normalization='causal', norm_min_frames=3)
    c = _config(tmp_path, 'normalization=utterance\n')
    assert (c.normalization, c.norm_min_frames) == ('utterance', None)
    assert normalization_of(object()) == dict(normalization='utterance', norm_min_frames=None)


def test_config_lists_the_keys(tmp_path, caplog):
    import logging
    from neuralasr_amd.config import log
    with caplog.at_level(logging.INFO, logger=log.name):
        _config(tmp_path, 'normalization=causal\nnorm_min_frames=7\n').print_config()
    assert 'normalization=causal' in caplog.text and 'norm_min_frames=7' in caplog.text


@pytest.mark.parametrize('extra,key', [('normalization=running\n', 'normalization'), ('normalization=Causal\n', 'normalization'),
                                       ('norm_min_frames=50\n', 'norm_min_frames'),
                                       ('normalization=utterance\nnorm_min_frames=50\n', 'norm_min_frames'),
                                       ('normalization=causal\nnorm_min_frames=0\n', 'norm_min_frames'),
                                       ('normalization=causal\nnorm_min_frames=1001\n', 'norm_min_frames'),
                                       ('normalization=causal\nnorm_min_frames=half\n', 'norm_min_frames'),
                                       ('normalization=causal\ndeltas=1\n', 'deltas')])
def test_config_bad_values_raise(tmp_path, extra, key):
    with pytest.raises(ValueError, match=key):
        _config(tmp_path, extra)


# ------------------------------------------------------------------------------------------------ the rule by hand
def test_rule_by_hand():
    x = np.array([[1.0, 3.0], [2.0, 6.0], [5.0, 5.0], [0.0, 2.0]])
    p1, p2 = CR.frame_sums(x)
    assert np.array_equal(p1, [4, 8, 10, 2]) and np.array_equal(p2, [10, 40, 50, 4])
    assert np.array_equal(CR.prefix(p1), [0, 4, 12, 22, 24])
    assert [CR.count(u, 4, 2) for u in range(4)] == [2, 2, 3, 4]
    assert [CR.count(u, 4, 9) for u in range(4)] == [4, 4, 4, 4]          # a short utterance: all of it, never more
    assert [CR.count(u, 4, 1) for u in range(4)] == [1, 2, 3, 4]
    y, (mean, sd) = CR.normalise_frames(x, 2)
    # frames 0 and 1 with the first two frames: mean 12/4 = 3, var 50/4 - 9 = 3.5; frame 2 with three: 22/6, 100/6 - (22/6)^2
    assert np.array_equal(y[0], ((x[0] - 3.0) / np.sqrt(3.5)).astype(np.float32))
    assert np.array_equal(y[1], ((x[1] - 3.0) / np.sqrt(3.5)).astype(np.float32))
    m2 = 22.0 / 6.0
    assert np.array_equal(y[2], ((x[2] - m2) / np.sqrt(100.0 / 6.0 - m2 * m2)).astype(np.float32))
    assert mean == 3.0 and sd == np.sqrt(104.0 / 8.0 - 9.0)
    # a variance that is not > 0: sd = 1, the output 0 (and no NaN)
    z, (zm, zs) = CR.normalise_frames(np.full((3, 2), -4.0), 1)
    assert (zm, zs) == (-4.0, 1.0) and np.array_equal(z, np.zeros((3, 2), np.float32))
    # context frames outside the utterance are exact zeros, not (0 - mean) / sd
    s = CR.stack(y, 1)
    assert s.shape == (4, 6) and np.array_equal(s[0, :2], [0, 0]) and np.array_equal(s[3, 4:], [0, 0])
    assert np.array_equal(s[1], np.concatenate([y[0], y[1], y[2]]))


def test_rows_total_by_hand():
    def rt(n, fin, nc=2, M=3):
        return CR.rows_total(n, fin, SR, nc, M)
    assert (CR.complete_frames(FLEN - 1, FLEN, FSTEP), CR.complete_frames(FLEN, FLEN, FSTEP)) == (0, 1)
    assert CR.complete_frames(FLEN + FSTEP - 1, FLEN, FSTEP) == 1 and CR.complete_frames(FLEN + FSTEP, FLEN, FSTEP) == 2
    assert rt(0, False) == 0 and rt(FLEN + FSTEP, False) == 0                   # 2 complete frames < M
    assert rt(FLEN + 2 * FSTEP, False) == 1                                      # 3 complete frames, nc 2 held back
    assert rt(FLEN + 2 * FSTEP, False, nc=5) == 0
    assert rt(FLEN + 9 * FSTEP, False) == 8 and rt(FLEN + 9 * FSTEP, False, nc=0, M=1) == 10
    assert rt(1, True) == 1 and rt(FLEN + 1, True) == 2 and rt(FLEN + 9 * FSTEP, True) == 10
    with pytest.raises(ValueError):
        rt(0, True)


# ----------------------------------------------------------------------------------- the simulator against the rule
def _pieces(n, how, seed=0):
    if how == 'one':
        return [1] * n
    if how == '37':
        return [37] * (n // 37) + ([n % 37] if n % 37 else [])
    if how == 'step':
        return [FSTEP] * (n // FSTEP) + ([n % FSTEP] if n % FSTEP else [])
    rng = np.random.default_rng(seed)
    out = []
    while sum(out) < n:
        out.append(int(min(n - sum(out), rng.choice([0, 1, 5, 79, 80, 81, 200, 433, 1200]))))
    return out


def _stream(a, nc, M, pieces, kind='mfcc', numcep=13, last_with_data=True):
    sim = CR.StreamSim(SR, nc, numcep, M, kind)
    rows, n, got, peak = [], 0, 0, (0, 0, 0)
    for i, k in enumerate(pieces):
        fin = last_with_data and i == len(pieces) - 1
        before = CR.rows_total(n, False, SR, nc, M)
        r = sim.feed(a[n:n + k], fin)
        n += k
        assert len(r) == CR.rows_total(n, fin, SR, nc, M) - before        # a feed emits rows_total(after) - rows_total(before)
        got += len(r)
        rows.append(r)
        if not fin:
            peak = tuple(max(p, q) for p, q in zip(peak, sim.max_state()))
    if not last_with_data:
        r = sim.feed(a[:0], True)                                          # finishing with an empty feed
        assert len(r) == CR.rows_total(n, True, SR, nc, M) - CR.rows_total(n, False, SR, nc, M)
        rows.append(r)
    return np.concatenate(rows), peak


@pytest.fixture(scope='module')
def utterance():
    a = speech_like(3000, SR, 5)
    return a, {(nc, M): CR.features(a, SR, nc, 13, M)[0] for nc in (0, 2) for M in (1, 3, 50)}


@pytest.mark.parametrize('how', ['one', '37', 'step', 'random'])
@pytest.mark.parametrize('nc,M', [(0, 1), (2, 3), (2, 50), (0, 50)])
def test_simulator_equals_the_offline_rule_bitwise(utterance, how, nc, M):
    a, want = utterance
    if how == 'one':
        a, ref = a[:700], CR.features(a[:700], SR, nc, 13, M)[0]            # (one sample per feed: a shorter utterance)
    else:
        ref = want[(nc, M)]
    got, peak = _stream(a, nc, M, _pieces(a.size, how), last_with_data=(how != 'random'))
    assert got.shape == ref.shape and got.tobytes() == ref.tobytes()
    # the state does not grow with the utterance
    biggest = max(_pieces(a.size, how))
    assert peak[0] <= FLEN + FSTEP + biggest and peak[1] <= M and peak[2] <= 2 * nc


def test_simulator_logfbank_and_silence():
    a = np.concatenate([np.zeros(1500, np.float32), speech_like(1700, SR, 6)])
    for kind, numcep in (('logfbank', 8), ('mfcc', 13)):
        ref, (mean, sd) = CR.features(a, SR, 2, numcep, 3, kind)
        assert np.all(np.isfinite(ref)) and np.isfinite(mean) and sd > 0
        got, _ = _stream(a, 2, 3, _pieces(a.size, 'random', 3), kind, numcep)
        assert got.tobytes() == ref.tobytes()
    z, (_, sd) = CR.features(np.zeros(2000, np.float32), SR, 2, 8, 3, 'logfbank')
    assert np.all(np.isfinite(z)) and np.abs(z).max() <= 1e-6              # every value is log(eps): (x - mean) is rounding noise


def _n_for_frames(T):
    """a sample count that makes T frames, not step-aligned"""
    n = FLEN if T == 1 else FLEN + (T - 1) * FSTEP - 7
    assert R.num_frames(n, SR) == T
    return n


@pytest.mark.parametrize('nc,M', [(0, 1), (2, 3), (2, 1), (0, 3), (5, 3)])
def test_emitted_rows_sum_to_T(nc, M):
    ns = [1, FLEN - 1, FLEN, FLEN + 1, FLEN + FSTEP] + [_n_for_frames(T) for T in (M - 1, M, M + 1) if T >= 1]
    ns += [_n_for_frames(T) for T in range(1, nc + 1)]                        # T <= nc
    for n in sorted(set(ns)):
        a = speech_like(n, SR, n)
        ref = CR.features(a, SR, nc, 13, M)[0]
        T = R.num_frames(n, SR)
        assert ref.shape[0] == T
        for how, fin in (('37', True), ('random', False), ('step', True)):
            got, _ = _stream(a, nc, M, _pieces(n, how, n), last_with_data=fin)
            assert got.shape[0] == T and got.tobytes() == ref.tobytes(), (n, how)


def test_forty_irregular_feeds_sum_to_T():
    a = speech_like(9000, SR, 11)
    rng = np.random.default_rng(2)
    cuts = np.sort(rng.choice(np.arange(1, a.size), 39, replace=False))
    pieces = np.diff(np.concatenate(([0], cuts, [a.size]))).tolist()
    assert len(pieces) == 40
    got, _ = _stream(a, 2, 50, pieces)
    assert got.shape[0] == R.num_frames(a.size, SR)
    assert got.tobytes() == CR.features(a, SR, 2, 13, 50)[0].tobytes()


def test_a_finished_slot_refuses_and_reset_starts_over():
    a = speech_like(1000, SR, 12)
    sim = CR.StreamSim(SR, 2, 13, 3)
    first = sim.feed(a, True)
    with pytest.raises(RuntimeError):
        sim.feed(a[:10])
    sim.reset()
    assert sim.feed(a, True).tobytes() == first.tobytes()
    with pytest.raises(ValueError):
        CR.StreamSim(SR, 2, 13, 3).feed(a[:0], True)                        # `last` on a slot that received nothing


def test_statistics_of_the_gpu_cases_keep_the_division_harmless():
    """the GPU test's tolerance is test_gpu_mfcc's: with sd >= 1 the division by sd does not widen the frames' error"""
    rng = np.random.default_rng(0)
    tone = (0.3 * np.sin(2 * np.pi * 440 * np.arange(4000) / SR)).astype(np.float32)
    cases = {'noise': (0.1 * rng.standard_normal(8000)).astype(np.float32), 'silence': np.zeros(4000, np.float32),
             'silence_tone': np.concatenate([np.zeros(4000, np.float32), tone]), 'sub_frame': speech_like(150, SR, 1)}
    for name, a in cases.items():
        x = CR.raw_frames(a, SR, 13)
        T = x.shape[0]
        p1, p2 = CR.frame_sums(x)
        S1, S2 = CR.prefix(p1), CR.prefix(p2)
        sds = [CR.mean_sd(S1[n], S2[n], n, 13)[1] for n in range(1, T + 1)]
        print('%s: sd in [%.2f, %.2f]' % (name, min(sds), max(sds)))
        assert min(sds) >= 1.0, name
        assert np.all(np.isfinite(CR.features(a, SR, 2, 13, 3)[0])), name
