"""Host: the restatement of tests/feat_ref.py (psf's logfbank and delta) against values worked by hand and against
mfcc_ref, that the GPU test's tolerance tells the right delta rule from three wrong ones, the config keys, and the C ABI
of the two new nasr_mfcc_cfg fields.  No GPU."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import feat_ref as FR
import mfcc_ref as R
from test_gpu_feat import TOL_MAX
from test_gpu_mfcc import speech_like

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 8000


# ------------------------------------------------------------------------------------------------- delta by hand
def test_delta_of_a_ramp_by_hand():
    ramp = np.arange(5, dtype=np.float64)[:, None] * np.ones((1, 3))
    d = FR.delta(ramp, 2)
    # t = 0: p = [0 0 |0| 1 2] -> ((1 - 0) + 2 (2 - 0)) / 10; t = 1: ((2 - 0) + 2 (3 - 0)) / 10; t = 2: ((3 - 1) + 2 (4 - 0)) / 10
    want = np.array([0.5, 0.8, 1.0, 0.8, 0.5])
    assert np.array_equal(d, want[:, None] * np.ones((1, 3)))
    # the delta-delta pads the DELTA array [.5 .8 1 .8 .5] by its own edges:
    # t = 0: ((.8 - .5) + 2 (1 - .5)) / 10 = .13; t = 1: ((1 - .5) + 2 (.8 - .5)) / 10 = .11; t = 2: ((.8 - .8) + 2 (.5 - .5)) / 10
    dd = FR.delta(d, 2)
    assert np.allclose(dd[:, 0], [0.13, 0.11, 0.0, -0.11, -0.13], rtol=0, atol=1e-15)
    full = FR.with_deltas(ramp, 2)
    assert full.shape == (5, 9)
    assert np.array_equal(full[:, :3], ramp) and np.array_equal(full[:, 3:6], d) and np.array_equal(full[:, 6:], dd)


def test_delta_of_one_frame_and_of_constants_is_exactly_zero():
    rng = np.random.default_rng(0)
    one = rng.standard_normal((1, 7))
    assert np.array_equal(FR.delta(one, 2), np.zeros((1, 7)))
    for T in range(1, 7):
        const = np.tile(rng.standard_normal((1, 4)), (T, 1))
        full = FR.with_deltas(const, 2)
        assert np.array_equal(full[:, 4:], np.zeros((T, 8))), T


def test_logfbank_is_mfcc_without_the_dct():
    a = speech_like(3000, SR, 1)
    lf = FR.logfbank(a, SR, 40)
    assert lf.shape == (R.num_frames(a.size, SR), 40) and np.all(np.isfinite(lf))
    # mfcc's columns 1.. are the lifted DCT of the same log energies
    m = R.mfcc(a, SR, 13, nfilt=40)
    assert np.allclose(m[:, 1:], R.lifter(lf @ R.dct_ortho(40, 13).T)[:, 1:], rtol=1e-12, atol=1e-12)
    silence = FR.logfbank(np.zeros(1000, np.float32), SR, 13)
    assert np.array_equal(silence, np.full(silence.shape, np.log(R.EPS)))


@pytest.mark.parametrize('nc,numcep', [(0, 13), (2, 13), (10, 40)])
def test_reduces_to_mfcc_ref_bitwise(nc, numcep):
    a = speech_like(5000, SR, 2)
    got, (gm, gs) = FR.features(a, SR, nc, numcep, kind='mfcc', deltas=0)
    want, (wm, ws) = R.features(a, SR, nc, numcep)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
    assert gm == wm and gs == ws


def test_widths():
    a = speech_like(2000, SR, 3)
    for kind, deltas, nc, numcep in [('logfbank', 0, 0, 40), ('logfbank', 2, 2, 13), ('mfcc', 1, 2, 13), ('mfcc', 2, 0, 40)]:
        x, _ = FR.features(a, SR, nc, numcep, kind, deltas)
        assert x.shape == (R.num_frames(a.size, SR), (2 * nc + 1) * numcep * (1 + deltas))
    with pytest.raises(ValueError):
        FR.features(a, SR, 0, 13, 'fbank', 0)
    with pytest.raises(ValueError):
        FR.features(a, SR, 0, 13, 'mfcc', 3)


# --------------------------------------------------------------------------------- the tolerance discriminates
def _delta_zero_pad(feat):
    T = feat.shape[0]
    p = np.pad(feat, ((2, 2), (0, 0)), mode='constant')
    return ((p[3:3 + T] - p[1:1 + T]) + 2 * (p[4:4 + T] - p[0:T])) / 10


def _wrong_zero_padding(statics, i):
    d = _delta_zero_pad(statics[i])
    return np.concatenate([statics[i], d, _delta_zero_pad(d)], axis=1)


def _wrong_clamped_across_utterances(statics, i):
    """the deltas of the packed frames of the whole batch, clamped only at the ends of the batch"""
    packed = FR.with_deltas(np.concatenate(statics), 2)
    f0 = sum(s.shape[0] for s in statics[:i])
    return packed[f0:f0 + statics[i].shape[0]]


def _wrong_delta_delta_beyond_the_edge(statics, i):
    """the delta-delta from deltas COMPUTED at t = -2, -1, T, T+1 (of the statics replicated further out)"""
    s = statics[i]
    T = s.shape[0]
    d_ext = FR.delta(np.pad(s, ((2, 2), (0, 0)), mode='edge'), 2)          # [T + 4]; d_ext[2:T+2] is the right delta
    dd = ((d_ext[3:3 + T] - d_ext[1:1 + T]) + 2 * (d_ext[4:4 + T] - d_ext[0:T])) / 10
    return np.concatenate([s, d_ext[2:T + 2], dd], axis=1)


@pytest.mark.parametrize('kind,numcep', [('logfbank', 40), ('mfcc', 13)])
def test_tolerance_tells_the_wrong_rules_apart(kind, numcep):
    audios = [speech_like(n, SR, 30 + k) for k, n in enumerate((4200, 6000, 3700))]
    statics = [FR.frames(a, SR, numcep, kind, 0) for a in audios]
    i = 1                                                 # the utterance in the middle: a neighbour on either side
    right, _ = FR.normalise(FR.with_deltas(statics[i], 2), 0)
    assert right.tobytes() == FR.features(audios[i], SR, 0, numcep, kind, 2)[0].tobytes()
    for wrong in (_wrong_zero_padding, _wrong_clamped_across_utterances, _wrong_delta_delta_beyond_the_edge):
        got, _ = FR.normalise(wrong(statics, i), 0)
        err = np.abs(got.astype(np.float64) - right).max()
        factor = err / TOL_MAX
        print('%s %s: max |wrong - right| = %.3e = %.0f x TOL_MAX' % (kind, wrong.__name__, err, factor))
        assert factor >= 10, (wrong.__name__, err)


# --------------------------------------------------------------------------------------------------------- config
def _config(tmp_path, extra='', numcep=13, numcontext=0):
    from neuralasr_amd.config import Config
    p = tmp_path / 'c.config'
    p.write_text('[Parameters]\nsamplerate=8000\nnumcep=%d\nnumcontext=%d\nlabel_context=0\nbatch_size=2\nepochs=1\n'
                 'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
                 'network=networks.bilstm_ctc_net.BiLstmCTCNet\n%s[Train]\n[Test]\ninput=%s\n[MFCC Featurizer]\n'
                 % (numcep, numcontext, tmp_path / 'model', extra, tmp_path / 'test.scp'))
    return Config(str(p))


def test_config_defaults_are_unchanged(tmp_path):
    c = _config(tmp_path, numcep=26, numcontext=10)
    assert (c.features, c.deltas, c.frame_width, c.feature_size) == ('mfcc', 0, 26, 21 * 26)


def test_config_logfbank_with_deltas(tmp_path):
    c = _config(tmp_path, 'features=logfbank\ndeltas=2\n', numcep=40, numcontext=2)
    assert (c.features, c.deltas, c.frame_width, c.feature_size) == ('logfbank', 2, 120, 600)
    c = _config(tmp_path, 'features=mfcc\ndeltas=1\n', numcep=13, numcontext=0)
    assert (c.frame_width, c.feature_size) == (26, 26)


@pytest.mark.parametrize('extra,key', [('features=fbank\n', 'features'), ('features=MFCC\n', 'features'),
                                       ('deltas=3\n', 'deltas'), ('deltas=-1\n', 'deltas'), ('deltas=two\n', 'deltas')])
def test_config_bad_values_raise(tmp_path, extra, key):
    with pytest.raises(ValueError, match=key):
        _config(tmp_path, extra)


# ------------------------------------------------------------------------------------------------------------ ABI
def _cfg(**kw):
    from neuralasr_amd import _lib
    base = dict(samplerate=8000, numcep=13, numcontext=0, nfilt=128, nfft=512, winlen=0.025, winstep=0.01, preemph=0.97,
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
  cfg.samplerate = 8000; cfg.numcep = 40; cfg.nfilt = 40; cfg.nfft = 512; cfg.winlen = 0.025; cfg.winstep = 0.01;
  cfg.preemph = 0.97f; cfg.kind = 1; cfg.deltas = 2;
  printf("%zu %zu %zu %d\n", sizeof(nasr_mfcc_cfg), offsetof(nasr_mfcc_cfg, kind), offsetof(nasr_mfcc_cfg, deltas),
         nasr_mfcc_width(&cfg));
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
    size, off_kind, off_deltas, width = (int(x) for x in out.stdout.split())
    assert size == ctypes.sizeof(_lib.MfccCfg)
    assert off_kind == _lib.MfccCfg.kind.offset and off_deltas == _lib.MfccCfg.deltas.offset
    assert off_deltas == off_kind + 4 and off_kind == _lib.MfccCfg.append_energy.offset + 4      # appended, in this order
    assert width == 120


def test_width_and_frames_are_host_only_and_refuse_bad_fields():
    from neuralasr_amd import _lib
    lib = _lib.load()

    def width(**kw):
        return lib.nasr_mfcc_width(ctypes.byref(_cfg(**kw)))

    def frames(**kw):
        return lib.nasr_mfcc_frames(ctypes.byref(_cfg(**kw)), 4000)
    T = R.num_frames(4000, 8000)
    assert width() == 13 and width(deltas=1) == 26 and width(deltas=2) == 39
    assert width(kind=1, numcep=40, nfilt=40, deltas=2) == 120 and width(kind=1, numcep=128, deltas=1) == 256
    assert frames() == frames(deltas=2) == frames(kind=1, numcep=40, nfilt=40, deltas=1) == T
    # ceplifter and append_energy are ignored for kind 1
    assert width(kind=1, numcep=13, nfilt=13, ceplifter=-5, append_energy=7) == 13
    for bad in (dict(kind=2), dict(kind=-1), dict(deltas=3), dict(deltas=-1), dict(kind=1, numcep=13, nfilt=128),
                dict(kind=1, numcep=13, nfilt=40, deltas=2)):
        assert width(**bad) == _lib.NASR_ERR_ARG, bad
        assert frames(**bad) == _lib.NASR_ERR_ARG, bad
    assert lib.nasr_mfcc_width(None) == _lib.NASR_ERR_ARG


def test_create_names_what_is_wrong_with_the_new_fields():
    """the argument checks run before the device is opened: the messages do not need a GPU"""
    from neuralasr_amd import _lib
    lib = _lib.load()
    for kw, text in ((dict(kind=2), 'kind must be 0'), (dict(deltas=3), 'deltas must be 0, 1 or 2'),
                     (dict(kind=1, numcep=13, nfilt=128), 'must equal nfilt')):
        h = ctypes.c_void_p()
        rc = lib.nasr_create_featurizer(ctypes.byref(_cfg(**kw)), 0, None, ctypes.byref(h))
        assert rc == _lib.NASR_ERR_ARG and not h
        with pytest.raises(_lib.NasrError, match=text):
            _lib.check(lib, None, rc)


def test_featurizer_python_arguments():
    from neuralasr_amd import features
    cfg = features._cfg(8000, 40, 2, 128, 512, 'logfbank', 2)
    assert (cfg.kind, cfg.deltas, cfg.nfilt, cfg.numcep) == (1, 2, 40, 40)
    cfg = features._cfg(8000, 13, 0, 128, 512)
    assert (cfg.kind, cfg.deltas, cfg.nfilt) == (0, 0, 128)
    with pytest.raises(ValueError, match='kind'):
        features._cfg(8000, 13, 0, 128, 512, 'fbank', 0)
