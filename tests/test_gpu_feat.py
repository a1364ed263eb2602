"""GPU: the log-mel filterbank and the delta columns of the front end (csrc/mfcc.hip under csrc/nasr_fz.hip: cfg.kind, cfg.deltas) against the
fp64 restatement of tests/feat_ref.py on one ragged batch whose short utterances are shorter than the delta window
and than the delta-delta's reach; the exact properties of the edge replication; batch invariance; buffer growth; the
batch slot of a model handle; and preprocess_mfcc / train / train --from-audio / decode_wav on a config with the two
new keys.  Tolerances are the front end's own (tests/test_gpu_mfcc.py), on the normalised output.

Measured on one MI355X: in all 16 parity cases every float32 of the output equals the restatement's (max and mean
|error| 0); the table is in DESIGN.md §9."""
import functools
import logging
import os

import numpy as np
import pytest

import feat_ref as FR
import mfcc_ref as R
from test_gpu_mfcc import speech_like

TOL_MAX, TOL_MEAN = 1e-4, 1e-6          # as tests/test_gpu_mfcc.py
SR = 8000
FRAME_LEN, FRAME_STEP = 200, 80         # 25 ms, 10 ms at 8 kHz
RAGGED_FRAMES = (3, 1, 104, 2, 9, 5, 100, 4)

KINDS = [('logfbank', 0), ('logfbank', 2), ('mfcc', 1), ('mfcc', 2)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def samples_for(frames, k):
    """a sample count that psf frames into `frames` frames (not always a whole number of steps)"""
    if frames == 1:
        return 150
    return FRAME_LEN + FRAME_STEP * (frames - 1) - (17 * k) % FRAME_STEP


@functools.lru_cache(maxsize=None)
def ragged():
    audios = tuple(speech_like(samples_for(t, k), SR, 60 + k) for k, t in enumerate(RAGGED_FRAMES))
    assert tuple(R.num_frames(a.size, SR) for a in audios) == RAGGED_FRAMES
    return audios


@functools.lru_cache(maxsize=None)
def ragged_ref(kind, deltas, nc, numcep):
    """[(float32 features, (mean, std))] of the ragged batch, computed once per case"""
    return tuple(FR.features(a, SR, nc, numcep, kind, deltas) for a in ragged())


@pytest.fixture(scope='module')
def fz():
    from neuralasr_amd.features import Featurizer
    made = {}

    def get(numcep, nc, kind, deltas, **kw):
        key = (numcep, nc, kind, deltas, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = Featurizer(SR, numcep, nc, kind=kind, deltas=deltas, **kw)
        return made[key]
    yield get
    for f in made.values():
        f.close()


def parity(got, stats, want, note):
    """the checks of tests/test_gpu_mfcc.py on one utterance; TOL_MEAN only where there are frames to average over"""
    (feat, (rm, rs)), (mean, std) = want, stats
    assert got.shape == feat.shape and got.dtype == np.float32, note
    err = np.abs(got.astype(np.float64) - feat)
    mx, mn = err.max(), err.mean()
    assert mx <= TOL_MAX, (note, mx)
    if got.shape[0] >= 50:
        assert mn <= TOL_MEAN, (note, mn)
    assert abs(mean - rm) <= 1e-4 * abs(rs) and abs(std - rs) <= 1e-4 * rs, (note, mean, rm, std, rs)
    return mx, (mn if got.shape[0] >= 50 else 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize('numcep', [13, 40])
@pytest.mark.parametrize('nc', [0, 2])
@pytest.mark.parametrize('kind,deltas', KINDS)
def test_parity_with_the_fp64_restatement(fz, kind, deltas, nc, numcep):
    f = fz(numcep, nc, kind, deltas)
    assert f.frame_width == numcep * (1 + deltas) and f.width == (2 * nc + 1) * f.frame_width
    feats, stats = f.compute(list(ragged()), return_stats=True)
    want = ragged_ref(kind, deltas, nc, numcep)
    worst = [parity(g, s, w, 'utterance of %d frames' % t) for g, s, w, t in zip(feats, stats, want, RAGGED_FRAMES)]
    print('%s deltas %d numcontext %d numcep %d: max |error| %.3e, mean |error| (>= 50 frames) %.3e'
          % (kind, deltas, nc, numcep, max(w[0] for w in worst), max(w[1] for w in worst)))


@pytest.mark.gpu
@pytest.mark.parametrize('kind,deltas,numcep', [('logfbank', 2, 40), ('mfcc', 1, 13), ('mfcc', 2, 13)])
def test_one_frame_utterance_has_exactly_the_pad_value_in_its_delta_columns(fz, kind, deltas, numcep):
    """numcontext 0: the deltas of one frame are exact zeros, so every such column is float32((0 - mean) / std)"""
    f = fz(numcep, 0, kind, deltas)
    feats, stats = f.compute(list(ragged()), return_stats=True)
    k = RAGGED_FRAMES.index(1)
    mean, std = stats[k]
    want = np.float32((0.0 - mean) / std)
    got = feats[k]
    assert got.shape == (1, numcep * (1 + deltas))
    assert np.all(bits(got[:, numcep:]) == bits(want)), (got[:, numcep:], want)
    assert not np.all(got[:, :numcep] == want)


@pytest.mark.gpu
@pytest.mark.parametrize('kind,deltas,numcep', [('logfbank', 2, 40), ('mfcc', 1, 13)])
def test_digital_silence_gives_identical_rows(fz, kind, deltas, numcep):
    silence = np.zeros(2000, np.float32)
    g = fz(numcep, 0, kind, deltas).compute([silence])[0]
    assert g.shape == (R.num_frames(2000, SR), numcep * (1 + deltas)) and np.all(np.isfinite(g))
    assert np.all(bits(g) == bits(g[0]))
    want, _ = FR.features(silence, SR, 0, numcep, kind, deltas)
    assert np.abs(g.astype(np.float64) - want).max() <= TOL_MAX


@pytest.mark.gpu
@pytest.mark.parametrize('kind,deltas,nc,numcep', [('logfbank', 2, 2, 40), ('mfcc', 2, 0, 13), ('mfcc', 1, 2, 13)])
def test_ragged_batch_is_bitwise_per_utterance_and_repeatable(fz, kind, deltas, nc, numcep):
    f = fz(numcep, nc, kind, deltas)
    audios = list(ragged())
    batch = f.compute(audios)
    again = f.compute(audios)
    for i, a in enumerate(audios):
        assert same(batch[i], f.compute([a])[0]), i
        assert same(batch[i], again[i]), i
    small = fz(numcep, nc, kind, deltas, max_samples=9000)          # the batch split over several library calls
    for i, (b, s) in enumerate(zip(batch, small.compute(audios))):
        assert same(b, s), i


@pytest.mark.gpu
def test_long_utterance_grows_buffers():
    from neuralasr_amd.features import Featurizer
    f = Featurizer(SR, 40, 2, kind='logfbank', deltas=2)
    try:
        f.compute([speech_like(SR // 4, SR, 1)])
        a = speech_like(3 * SR, SR, 12)
        g, st = f.compute([a], return_stats=True)
        parity(g[0], st[0], FR.features(a, SR, 2, 40, 'logfbank', 2), '3 s after 0.25 s')
    finally:
        f.close()


@pytest.mark.gpu
@pytest.mark.parametrize('numcep,nc', [(13, 0), (26, 2)])
def test_defaults_are_the_mfcc_of_before(numcep, nc):
    from neuralasr_amd.features import Featurizer
    a, b = Featurizer(SR, numcep, nc), Featurizer(SR, numcep, nc, kind='mfcc', deltas=0)
    try:
        assert a.width == b.width == (2 * nc + 1) * numcep and (a.cfg.kind, a.cfg.deltas) == (0, 0)
        audios = list(ragged())
        for x, y, w in zip(a.compute(audios), b.compute(audios), audios):
            assert same(x, y)
            assert np.abs(x.astype(np.float64) - R.features(w, SR, nc, numcep)[0]).max() <= TOL_MAX
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_create_refuses_bad_fields():
    from neuralasr_amd import _lib
    from neuralasr_amd.features import Featurizer
    with pytest.raises(_lib.NasrError, match='deltas must be 0, 1 or 2'):
        Featurizer(SR, 13, 0, deltas=3)
    with pytest.raises(_lib.NasrError, match='nfilt'):
        Featurizer(SR, 129, 0, kind='logfbank')


@pytest.mark.gpu
def test_batch_slot_from_audio_equals_the_host_routes(fz):
    """(logfbank, 2), numcontext 2, numcep 13 into a one-layer BiLSTM of 16 cells: the audio route, the centre form of
    the host's features and the plain stacked upload give the same logits, on one handle (tests/test_gpu_audio_batch.py)"""
    from neuralasr_amd.engine import Engine
    numcep, nc, C = 13, 2, 12
    f = fz(numcep, nc, 'logfbank', 2)
    audios = [ragged()[k] for k in (4, 2, 1)]             # 9, 104 and 1 frames
    B = len(audios)
    labels, label_len = np.ones((B, 1), np.int32), [1] * B
    e = Engine(f.width, 16, 1, True, 'stack_reshape', C, learning_rate=1e-3)
    rs = np.random.RandomState(3)
    e.set_params((0.2 * rs.randn(e.param_count)).astype(np.float32))
    try:
        seq, T = e.upload_batch_audio(f, audios, labels, label_len, None)
        assert [int(t) for t in seq] == [9, 104, 1] and T == 104
        from_audio = e.forward_resident(B, T)
        feats = f.compute(audios)
        x = np.zeros((B, T, f.width), np.float32)
        for b, g in enumerate(feats):
            x[b, :g.shape[0]] = g
        assert e.upload_batch_context(x, seq, labels, label_len, nc, f.frame_width), 'the centre form was not taken'
        from_centre = e.forward_resident(B, T)
        e.upload_batch(x, seq, labels, label_len)
        from_stacked = e.forward_resident(B, T)
        assert np.all(np.isfinite(from_audio))
        assert same(from_audio, from_centre)
        assert same(from_audio, from_stacked)
    finally:
        e.close()


@pytest.mark.gpu
def test_preprocess_train_and_decode_wav_with_the_new_keys(tmp_path, caplog):
    """features=logfbank, deltas=1: pickles of the new width; two training steps from the pickles and two straight from
    audio give the same loss bits; decode_wav runs"""
    from neuralasr_amd import decode_wav, preprocess_mfcc, train
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    from neuralasr_amd.features import write_wav16
    texts = ['hello world', 'a cat a dog', 'speech to text', 'one two three', 'front end']
    rows, audios = [], {}
    for i, text in enumerate(texts):
        wav, txt = tmp_path / ('utt%d.wav' % i), tmp_path / ('utt%d.txt' % i)
        audios['utt%d' % i] = speech_like(int(SR * (0.5 + 0.1 * i)), SR, 400 + i)
        write_wav16(wav, audios['utt%d' % i], SR)
        txt.write_text(text + '\n')
        rows.append('%s,%s,%d' % (wav, txt, os.path.getsize(wav)))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'feat'
    cfg_path = tmp_path / 'e2e.config'
    cfg_path.write_text(
        '[Parameters]\nsamplerate=%d\nnumcep=13\nnumcontext=2\nfeatures=logfbank\ndeltas=1\nlabel_context=0\nbatch_size=2\n'
        'epochs=1\nlearningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
        'sym_file=${MFCC Featurizer:output}/symbols\nnetwork=networks.bilstm_ctc_net.BiLstmCTCNet\n'
        '[Train]\ninput=${MFCC Featurizer:output}/train.scp\n[Test]\ninput=${MFCC Featurizer:output}/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\n' % (SR, tmp_path / 'model', tmp_path / 'data.csv', out))
    preprocess_mfcc.main([str(cfg_path)])
    config = Config(str(cfg_path), True)
    assert config.feature_size == 5 * 26
    ds = DataSet(config.train_input, config)
    for name in (out / 'train.scp').read_text().split():
        x = ds.load_pkl(str(out / name))[0]
        want, _ = FR.features(audios[name[:-4]], SR, 2, 13, 'logfbank', 1)
        assert x.shape == want.shape and x.shape[1] == 130 and np.abs(x - want).max() <= TOL_MAX

    def two_steps(data):
        net = config.load_network(fortraining=True)
        losses = [net.train(*data.get_next_batch())[0] for _ in range(2)]
        net._settle()
        kernels = (net.engine.recurrence_mode, net.engine.persist_stats())
        return net, losses, kernels
    net_p, pickled, kernels_p = two_steps(ds)
    net_p.engine.close()
    net_a, from_audio, kernels_a = two_steps(train.audio_datasets(str(cfg_path), config)[0])
    note = 'recurrence %r (pickles), %r (from audio)' % (kernels_p, kernels_a)
    assert np.all(np.isfinite(pickled)), pickled
    assert same(pickled, from_audio), (pickled, from_audio, note)
    net_a.save_checkpoint()
    net_a.engine.close()
    with caplog.at_level(logging.INFO):
        decoded = decode_wav.main([str(cfg_path), str(tmp_path / 'utt4.wav')])
    assert isinstance(decoded, str)
    assert any(r.getMessage().startswith('Decoded: ') for r in caplog.records)
