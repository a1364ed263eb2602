"""GPU: the causal normalisation of the front end (csrc/mfcc.hip: mfcc_norm_kernel<1, .>, cfg.norm = 1) against the fp64 restatement
of tests/causal_ref.py, at the smallest shapes that can still go wrong: 8 kHz, 13 cepstra (and 8 log-mel filters),
numcontext 0 and 2, norm_min_frames 1 and 3, utterances around every threshold of the rule, and one of 30 s (twelve
chunks of the sequential prefix).  Tolerance: test_gpu_mfcc's TOL_MAX, TOL_MEAN - the running std of the MFCC cases is
>= 9.6 (tests/test_causal_host.py) and of the log-mel ones >= 0.49 where there is signal, so the division widens the
frames' fp64 error (1e-12) by a small factor at most; measured: 0 on every case.  Then: the output does not depend on
how utterances are batched, the batch-slot form leaves the bits of the route through the host, norm = 0 is what it was."""
import ctypes

import numpy as np
import pytest

import causal_ref as CR
import mfcc_ref as R
from test_gpu_mfcc import TOL_MAX, TOL_MEAN, speech_like

pytestmark = pytest.mark.gpu

SR = 8000
FLEN, FSTEP = R.frame_params(SR)
CONFIGS = [('mfcc', 13, 0, 1), ('mfcc', 13, 2, 3), ('mfcc', 13, 0, 3), ('mfcc', 13, 2, 1), ('logfbank', 8, 2, 3),
           ('logfbank', 8, 0, 1)]


def n_for_frames(T):
    n = FLEN if T == 1 else FLEN + (T - 1) * FSTEP - 7
    assert R.num_frames(n, SR) == T
    return n


def utterances():
    rng = np.random.default_rng(0)
    tone = (0.3 * np.sin(2 * np.pi * 440 * np.arange(4000) / SR)).astype(np.float32)
    u = {'sub_frame': speech_like(150, SR, 1), 'one_frame': speech_like(FLEN, SR, 2)}
    for T in (2, 3, 4):                                     # T = M-1, M, M+1 for M = 3; T <= nc for nc = 2 (with one_frame)
        u['T%d' % T] = speech_like(n_for_frames(T), SR, 10 + T)
    u['noise'] = (0.1 * rng.standard_normal(SR)).astype(np.float32)
    u['silence_tone'] = np.concatenate([np.zeros(4000, np.float32), tone])
    u['all_zero'] = np.zeros(3000, np.float32)
    u['long'] = speech_like(30 * SR, SR, 3)
    return u


@pytest.fixture(scope='module')
def data():
    """the utterances, and per (kind, numcep) their un-normalised fp64 frames: computed once, read by every test"""
    u = utterances()
    raw = {(kind, numcep): {k: CR.raw_frames(a, SR, numcep, kind) for k, a in u.items()} for kind, numcep in (('mfcc', 13), ('logfbank', 8))}
    return u, raw


@pytest.fixture(scope='module')
def fz():
    from neuralasr_amd.features import Featurizer
    made = {}

    def get(kind, numcep, nc, M, **kw):
        key = (kind, numcep, nc, M, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = Featurizer(SR, numcep, nc, kind=kind, normalization='causal', norm_min_frames=M, **kw)
        return made[key]
    yield get
    for f in made.values():
        f.close()


@pytest.mark.parametrize('kind,numcep,nc,M', CONFIGS)
def test_against_the_rule(data, fz, kind, numcep, nc, M):
    u, raw = data
    names = list(u)
    f = fz(kind, numcep, nc, M)
    assert (f.cfg.norm, f.cfg.norm_min_frames, f.width) == (1, M, (2 * nc + 1) * numcep)
    feats, stats = f.compute([u[k] for k in names], return_stats=True)
    worst = 0.0
    for k, g, (mean, sd) in zip(names, feats, stats):
        y, (rm, rs) = CR.normalise_frames(raw[(kind, numcep)][k], M)
        want = CR.stack(y, nc)
        assert g.shape == want.shape == (R.num_frames(u[k].size, SR), f.width) and g.dtype == np.float32
        assert np.all(np.isfinite(g)), k
        err = np.abs(g.astype(np.float64) - want)
        print('%s %s nc %d M %d %s: max %.3e mean %.3e sd(T) %.4f' % (kind, numcep, nc, M, k, err.max(), err.mean(), sd))
        worst = max(worst, err.max())
        assert err.max() <= TOL_MAX and err.mean() <= TOL_MEAN, (k, err.max(), err.mean())
        if k != 'all_zero' or kind == 'mfcc':             # (log-mel silence: the variance is rounding noise around 0)
            assert abs(mean - rm) <= 1e-4 * abs(rs) and abs(sd - rs) <= 1e-4 * rs, (k, mean, rm, sd, rs)
        # context frames outside the utterance are exact zeros
        if nc:
            assert not g[0, :nc * numcep].any() and not g[-1, (nc + 1) * numcep:].any(), k
    print('worst max-abs error %.3e' % worst)


def test_a_variance_of_exactly_zero_gives_sd_one(fz):
    """two log-mel filters over digital silence, M = 1: S1 = 2v, 4v and S2 = 2 fl(v v), 4 fl(v v) are exact, so mean = v and
    the variance is exactly 0 for both frames: sd = 1 and every output 0, not NaN"""
    f = fz('logfbank', 2, 2, 1)
    (g,), ((mean, sd),) = f.compute([np.zeros(n_for_frames(2), np.float32)], return_stats=True)
    assert g.shape == (2, 10) and not g.any()
    assert sd == 1.0 and abs(mean - np.log(R.EPS)) <= 1e-12
    # ... and all-zero audio of any length stays finite under every config
    for kind, numcep, nc, M in CONFIGS:
        z = fz(kind, numcep, nc, M).compute([np.zeros(3000, np.float32)])[0]
        assert np.all(np.isfinite(z))


@pytest.mark.parametrize('kind,numcep,nc,M', [('mfcc', 13, 2, 3), ('logfbank', 8, 0, 1)])
def test_batching_does_not_change_a_bit(data, fz, kind, numcep, nc, M):
    u, _ = data
    names = [k for k in u if k != 'long'] + ['long']
    f = fz(kind, numcep, nc, M)
    batch = f.compute([u[k] for k in names])
    again = f.compute([u[k] for k in reversed(names)])[::-1]
    small = fz(kind, numcep, nc, M, max_samples=9000).compute([u[k] for k in names])      # split over several library calls
    for k, b, a, s in zip(names, batch, again, small):
        one = f.compute([u[k]])[0]
        assert b.tobytes() == one.tobytes() == a.tobytes() == s.tobytes(), k


def tiny_net(F, layers=1, C=5, seed=3):
    from neuralasr_amd.engine import Engine
    e = Engine(F, 16, layers, False, 'none', C, learning_rate=1e-3)
    rs = np.random.RandomState(seed)
    e.set_params((0.2 * rs.randn(e.param_count)).astype(np.float32))
    return e


@pytest.mark.parametrize('kind,numcep,nc,M', [('mfcc', 13, 2, 3), ('mfcc', 13, 0, 1), ('logfbank', 8, 2, 3)])
def test_batch_slot_form_equals_the_route_through_the_host(data, fz, kind, numcep, nc, M):
    """nasr_upload_batch_audio under the causal rule leaves the slot with the bits of nasr_featurize + zero-pad +
    nasr_upload_batch_context with pad 0: logits and loss of a tiny net, as bits"""
    u, _ = data
    names = ['noise', 'sub_frame', 'T2', 'T3', 'T4', 'silence_tone', 'all_zero']
    audios = [u[k] for k in names]
    f = fz(kind, numcep, nc, M)
    B, C = len(audios), 5
    labels = np.ones((B, 1), np.int32)
    ll = [1] * B
    e = tiny_net(f.width)
    seq, T = e.upload_batch_audio(f, audios, labels, ll)
    got = (e.forward_resident(B, T), e.loss_resident(B))
    feats = f.compute(audios)
    assert [int(t) for t in seq] == [x.shape[0] for x in feats] and T == max(x.shape[0] for x in feats)
    centre = np.zeros((B, T, numcep), np.float32)
    for b, x in enumerate(feats):
        centre[b, :x.shape[0]] = x[:, nc * numcep:(nc + 1) * numcep]
    pad = np.zeros(B, np.float32)
    fp, ip = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    seq32, ll32 = np.asarray(seq, np.int32), np.asarray(ll, np.int32)
    e._ck(e.lib.nasr_upload_batch_context(e.h, centre.ctypes.data_as(fp), pad.ctypes.data_as(fp), nc, numcep,
                                          seq32.ctypes.data_as(ip), labels.ctypes.data_as(ip), ll32.ctypes.data_as(ip), B, T, 1))
    want = (e.forward_resident(B, T), e.loss_resident(B))
    assert got[0].tobytes() == want[0].tobytes()
    assert np.float32(got[1][0]).tobytes() == np.float32(want[1][0]).tobytes()
    assert np.asarray(got[1][1], np.float32).tobytes() == np.asarray(want[1][1], np.float32).tobytes()
    # ... and of the stacked rows uploaded whole
    full = np.zeros((B, T, f.width), np.float32)
    for b, x in enumerate(feats):
        full[b, :x.shape[0]] = x
    assert e.forward(full, seq).tobytes() == want[0].tobytes()
    e.close()


def test_norm_zero_is_what_a_cfg_without_the_fields_gave(data):
    """Featurizer's defaults put zeros into the two new fields: the whole-utterance kernels run, bit for bit those of
    normalization='utterance' spelled out, within test_gpu_mfcc's bounds of the whole-utterance reference"""
    from neuralasr_amd.features import Featurizer
    u, _ = data
    audios = [u[k] for k in ('noise', 'sub_frame', 'T3', 'silence_tone')]
    a, b = Featurizer(SR, 13, 2), Featurizer(SR, 13, 2, normalization='utterance')
    assert (a.cfg.norm, a.cfg.norm_min_frames) == (b.cfg.norm, b.cfg.norm_min_frames) == (0, 0)
    for x, y, audio in zip(a.compute(audios), b.compute(audios), audios):
        assert x.tobytes() == y.tobytes()
        want, _ = R.features(audio, SR, 2, 13)
        err = np.abs(x.astype(np.float64) - want)
        assert err.max() <= TOL_MAX and err.mean() <= TOL_MEAN
    c = Featurizer(SR, 13, 2, normalization='causal', norm_min_frames=3)
    assert not np.array_equal(c.compute(audios[:1])[0], a.compute(audios[:1])[0])
    for f in (a, b, c):
        f.close()


def test_refusals_at_create():
    from neuralasr_amd import _lib, features
    from neuralasr_amd.features import Featurizer
    for kw, text in ((dict(norm_min_frames=0), 'norm_min_frames must be in'), (dict(norm_min_frames=1001), 'norm_min_frames'),
                     (dict(norm_min_frames=3, deltas=1), 'deltas = 0'), (dict(norm_min_frames=3, deltas=2), 'look')):
        with pytest.raises(_lib.NasrError, match=text) as err:
            Featurizer(SR, 13, 0, normalization='causal', **kw)
        assert err.value.code == _lib.NASR_ERR_ARG
    cfg = _lib.MfccCfg.from_buffer_copy(features._cfg(SR, 13, 0, 128, 512))
    cfg.norm = 2
    h = ctypes.c_void_p()
    lib = _lib.load()
    assert lib.nasr_create_featurizer(ctypes.byref(cfg), 0, None, ctypes.byref(h)) == _lib.NASR_ERR_ARG and not h
    with pytest.raises(_lib.NasrError, match='norm must be 0'):
        _lib.check(lib, None, _lib.NASR_ERR_ARG)
