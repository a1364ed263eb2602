"""GPU: a batch straight from audio (nasr_upload_batch_audio / nasr_stage_batch_audio) against the route through the host:
Featurizer.compute, zero-pad to T, upload_batch_context (or upload_batch).  Everything is compared as bits, and the
expected side is always the host route."""
import ctypes
import logging
import os

import numpy as np
import pytest

from test_audio_batch_host import SR as E2E_SR
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu

C = 12
FRONT = [(16000, 26, 10), (8000, 13, 0), (8000, 40, 10)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope='module')
def fz():
    from neuralasr_amd.features import Featurizer
    made = {}

    def get(sr, numcep, nc):
        if (sr, numcep, nc) not in made:
            made[(sr, numcep, nc)] = Featurizer(sr, numcep, nc)
        return made[(sr, numcep, nc)]
    yield get
    for f in made.values():
        f.close()


def make_batch(sr, B, mixed, seed=0, dense_classes=0):
    """ragged utterances: a one-frame one (B > 1), one at the batch maximum, the rest in between; labels that fit"""
    rng = np.random.default_rng(seed + 100 * B)
    secs = [0.62] + [float(s) for s in rng.uniform(0.08, 0.6, size=max(0, B - 2))] + ([0.0] if B > 1 else [])
    native = [16000, 44100, 8000]
    audios, rates = [], []
    for i, s in enumerate(secs):
        r = native[i % 3] if mixed else sr
        n = int(r * s) if s > 0 else int(0.012 * r)            # 12 ms: one frame
        audios.append(speech_like(n, r, seed * 1000 + i))
        rates.append(r)
    from neuralasr_amd.features import AudioBatch
    seq = [int(t) for t in AudioBatch(sr, audios, rates if mixed else None).seq_len]
    assert max(seq) == seq[0] and (B == 1 or seq[-1] == 1)
    Lmax = 6
    if dense_classes:
        label_len = [int(rng.integers(1, Lmax + 1)) for _ in seq]
        labels = rng.integers(0, dense_classes, size=(B, Lmax)).astype(np.int32)
    else:
        label_len = [int(min(Lmax, t // 2, rng.integers(1, Lmax + 1))) if t > 1 else 1 for t in seq]
        labels = np.zeros((B, Lmax), np.int32)
        for b, n in enumerate(label_len):
            labels[b, :n] = rng.integers(1, C - 1, size=n)
    return audios, (rates if mixed else None), labels, label_len, seq


def host_feats(f, audios, rates):
    feats = f.compute(audios, rates=rates)
    T = max(x.shape[0] for x in feats)
    out = np.zeros((len(feats), T, f.width), np.float32)
    for b, x in enumerate(feats):
        out[b, :x.shape[0]] = x
    return out, [x.shape[0] for x in feats], T


def init(e, seed=3):
    """seeded parameters and a fresh optimiser: also puts a handle that has taken a step back where it started"""
    rs = np.random.RandomState(seed)
    e.set_params((0.2 * rs.randn(e.param_count)).astype(np.float32))
    zero = np.zeros(e.param_count, np.float32)
    e.set_adam_state(zero, zero, 0)
    return e


def lstm(F):
    from neuralasr_amd.engine import Engine
    return init(Engine(F, 32, 1, True, 'stack_reshape', C, learning_rate=1e-3))


def observe(e, B, T, ctc=True):
    """what the two routes must agree on, from the resident batch"""
    out = {'frames': e.resident_frames()}
    if ctc:
        out['logits'] = e.forward_resident(B, T)
        out['loss_fwd'], out['nll'] = e.loss_resident(B)
        out['greedy'] = e.greedy_decode_resident(B, T)
    e.compute_grads()
    out['loss'] = e.get_loss()
    out['grads'] = e.get_grads()
    e.apply_adam(1.0)
    out['params'] = e.get_params()
    return out


def state(e):
    """what kernels served the handle: a recurrence that fell back to the per-step kernels computes other bits"""
    return (e.recurrence_mode, e.persist_stats()) if hasattr(e.cfg, 'hidden') else None


def assert_same(got, want, note=''):
    assert sorted(got) == sorted(want)
    for k in want:
        if k in ('frames', 'greedy'):
            assert got[k] == want[k], '%s differs %s' % (k, note)
        else:
            g, w = np.asarray(got[k], np.float32), np.asarray(want[k], np.float32)
            assert same(g, w), '%s differs: %d of %d elements, max |difference| %g %s' % (
                k, int(np.sum(bits(g) != bits(w))) if g.shape == w.shape else -1, w.size,
                float(np.abs(g.astype(np.float64) - w).max()) if g.shape == w.shape else float('nan'), note)


def route_host(e, f, batch, plain=False):
    audios, rates, labels, label_len, _ = batch
    feats, seq, T = host_feats(f, audios, rates)
    if plain or not e.upload_batch_context(feats, seq, labels, label_len, f.numcontext, f.numcep):
        e.upload_batch(feats, seq, labels, label_len)
    return seq, T


def route_audio(e, f, batch):
    audios, rates, labels, label_len, _ = batch
    seq, T = e.upload_batch_audio(f, audios, labels, label_len, rates)
    return [int(t) for t in seq], T


@pytest.mark.parametrize('mixed', [True, False], ids=['mixed-rates', 'rates-none'])
@pytest.mark.parametrize('B', [1, 5, 17])
@pytest.mark.parametrize('front', FRONT, ids=lambda c: '%dk-%d-nc%d' % (c[0] // 1000, c[1], c[2]))
def test_two_routes_give_the_same_bits(fz, front, B, mixed):
    """Both routes on ONE handle, put back to the same parameters and optimiser state in between: which kernels run the
    recurrence is settled per handle at create (a placement census), so two handles are not guaranteed the same bits."""
    sr, numcep, nc = front
    f = fz(sr, numcep, nc)
    batch = make_batch(sr, B, mixed, seed=numcep)
    e = lstm(f.width)
    before = state(e)
    seq_a, T_a = route_host(e, f, batch)
    want = observe(e, B, T_a)
    init(e)
    seq_b, T_b = route_audio(e, f, batch)
    assert seq_b == seq_a == batch[4] and T_b == T_a
    got = observe(e, B, T_b)
    note = '(recurrence %r at create, %r now)' % (before, state(e))
    assert_same(got, want, note)
    if B == 5:
        # the stacked array uploaded whole, through the calls that upload for themselves
        init(e)
        feats, seq, T = host_feats(f, batch[0], batch[1])
        assert same(e.forward(feats, seq), got['logits'])
        assert e.resident_frames() == got['frames']
        loss, nll, grads = e.loss_and_grads(feats, seq, batch[2], batch[3])
        assert same(loss, got['loss']) and same(nll, got['nll']) and same(grads, got['grads'])
        assert e.greedy_decode(feats, seq) == got['greedy']
        e.upload_batch(feats, seq, batch[2], batch[3])
        assert e.resident_frames() == got['frames']
        e.compute_grads()
        e.apply_adam(1.0)
        assert same(e.get_params(), got['params']), 'parameters after Adam, plain upload ' + note
    assert state(e) == before, 'the recurrence changed kernels during the test: ' + note
    e.close()


@pytest.mark.parametrize('family', ['deepspeech', 'wavenet', 'las'])
def test_other_families(fz, family):
    from neuralasr_amd.engine import Engine, LasEngine, WaveNetEngine
    sr, numcep, nc = 8000, 13, 1
    f = fz(sr, numcep, nc)

    def make():
        if family == 'deepspeech':
            return init(Engine(f.width, 32, 1, True, 'concat', C, learning_rate=1e-3, pre=(48, 32, 40), post=24))
        if family == 'wavenet':
            return init(WaveNetEngine(f.width, C, num_blocks=1, rates=(1, 2), learning_rate=1e-3), seed=4)
        return init(LasEngine(f.width, C, sampling_probability=0.1, seed=5, learning_rate=1e-3), seed=6)
    batch = make_batch(sr, 5, True, seed=7, dense_classes=C if family == 'las' else 0)
    # two handles: batch-norm and sampling state make a handle that has taken a step a different one.  The WaveNet and
    # LAS have one set of kernels; the DeepSpeech LSTM's are compared below.
    a, b = make(), make()
    assert state(a) == state(b)
    seq_a, T_a = route_host(a, f, batch)
    seq_b, T_b = route_audio(b, f, batch)
    assert seq_b == seq_a and T_b == T_a
    want, got = observe(a, 5, T_a, ctc=family != 'las'), observe(b, 5, T_b, ctc=family != 'las')
    assert_same(got, want, '(recurrence %r and %r)' % (state(a), state(b)))
    a.close()
    b.close()


def test_staging(fz):
    from neuralasr_amd import _lib
    sr, numcep, nc = 16000, 26, 10
    f = fz(sr, numcep, nc)
    batches = [make_batch(sr, B, True, seed=40 + B) for B in (5, 4, 3)]
    e = lstm(f.width)
    before = state(e)
    want = []                                            # the synchronous upload of each batch, on the same handle
    for bt in batches[1:]:
        seq, T = route_audio(e, f, bt)
        e.compute_grads()
        want.append((seq, T, e.get_loss(), e.get_grads()))
    probe = speech_like(5000, sr, 99)
    probe_feats = f.compute([probe])[0].copy()

    route_audio(e, f, batches[0])
    e.compute_grads()                                   # in flight while the next two batches are staged
    staged = [e.stage_batch_audio(f, bt[0], bt[2], bt[3], bt[1]) for bt in batches[1:]]
    assert all(t is not None for _, _, t in staged)
    assert e.stage_batch_audio(f, batches[0][0], batches[0][2], batches[0][3], batches[0][1])[2] is None
    rc, _, _ = e._audio_call(e.lib.nasr_stage_batch_audio, f, batches[0][0], batches[0][2], batches[0][3], batches[0][1],
                             ctypes.byref(ctypes.c_int(-1)))
    assert rc == _lib.NASR_ERR_STATE                    # two staged ahead: the third is refused
    # the featurizer handle itself, between stage and commit: ordered behind the staged kernels, and both results stand
    assert same(f.compute([probe])[0], probe_feats)
    e.get_loss()
    for (seq, T, ticket), (wseq, wT, wloss, wgrads) in zip(staged, want):
        assert [int(t) for t in seq] == wseq and T == wT
        e.commit_batch(ticket)
        e.compute_grads()
        assert same(e.get_loss(), wloss) and same(e.get_grads(), wgrads)
    # a discarded ticket frees its slot
    t1 = e.stage_batch_audio(f, batches[1][0], batches[1][2], batches[1][3], batches[1][1])[2]
    t2 = e.stage_batch_audio(f, batches[2][0], batches[2][2], batches[2][3], batches[2][1])[2]
    assert t1 is not None and t2 is not None
    assert e.stage_batch_audio(f, batches[0][0], batches[0][2], batches[0][3], batches[0][1])[2] is None
    e.discard_batch(t1)
    with pytest.raises(_lib.NasrError):
        e.commit_batch(t1)
    t3 = e.stage_batch_audio(f, batches[1][0], batches[1][2], batches[1][3], batches[1][1])[2]
    assert t3 is not None
    e.commit_batch(t3)
    e.compute_grads()
    assert same(e.get_loss(), want[0][2]) and same(e.get_grads(), want[0][3])
    e.discard_batch(t2)
    assert state(e) == before
    e.close()


def test_batch_independence(fz):
    """Utterance b alone, and inside a batch whose padded length a longer utterance sets: the same logits below
    seq_len[b] and the same loss contribution."""
    from neuralasr_amd.engine import Engine
    sr, numcep, nc = 8000, 40, 10
    f = fz(sr, numcep, nc)
    audios, rates, labels, label_len, seq = make_batch(sr, 5, True, seed=11)
    longer = speech_like(int(0.9 * 44100), 44100, 77)
    e = init(Engine(f.width, 32, 1, True, 'concat', C, learning_rate=1e-3))
    for b in (1, 2, 4):
        s1, T1 = e.upload_batch_audio(f, [audios[b]], labels[b:b + 1], [label_len[b]], [rates[b]])
        alone_logits = e.forward_resident(1, T1)
        _, alone_nll = e.loss_resident(1)
        s2, T2 = e.upload_batch_audio(f, [audios[b], longer], np.stack([labels[b], labels[0]]), [label_len[b], label_len[0]],
                                      [rates[b], 44100])
        both_logits = e.forward_resident(2, T2)
        _, both_nll = e.loss_resident(2)
        n = int(s1[0])
        assert int(s2[0]) == n == seq[b] and T2 > T1
        print('utterance %d: max |logit difference| %g, nll %r vs %r' % (
            b, np.abs(alone_logits[:n, 0] - both_logits[:n, 0]).max(), alone_nll[0], both_nll[0]))
        assert same(alone_logits[:n, 0], both_logits[:n, 0])
        assert same(alone_nll[0], both_nll[0])
    e.close()


def test_errors(fz):
    import torch
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine
    sr, numcep, nc = 8000, 13, 0
    f = fz(sr, numcep, nc)
    e = lstm(f.width)
    audios, rates, labels, label_len, seq = make_batch(sr, 3, True, seed=2)

    def refused(code, text, *args, model=None, **kw):
        with pytest.raises(_lib.NasrError) as err:
            (model or e).upload_batch_audio(*args, **kw)
        assert err.value.code == code and text in str(err.value), str(err.value)

    other = lstm(f.width)
    refused(_lib.NASR_ERR_STATE, 'not a featurizer handle', other, audios, labels, label_len, rates)
    other.close()
    # the model handle is a featurizer
    saved, e.h = e.h, f.h
    try:
        refused(_lib.NASR_ERR_STATE, 'a featurizer handle has no model', f, audios, labels, label_len, rates)
    finally:
        e.h = saved
    # The different-devices refusal needs two GPUs: on a one-GPU machine this branch does not run, and that refusal of
    # audio_batch() in nasr_api.hip is NOT covered by the suite.
    if torch.cuda.device_count() > 1:
        from neuralasr_amd.features import Featurizer
        far = Featurizer(sr, numcep, nc, device_id=1)
        refused(_lib.NASR_ERR_STATE, 'device', far, audios, labels, label_len, rates)
        far.close()
    wide = lstm(f.width + 1)
    refused(_lib.NASR_ERR_ARG, '(2*numcontext+1)*numcep', f, audios, labels, label_len, rates, model=wide)
    wide.close()
    refused(_lib.NASR_ERR_ARG, 'utterance 1', f, audios, labels, label_len, [rates[0], 0, rates[2]])
    short = [audios[0], audios[1], np.zeros(3, np.float32)]
    refused(_lib.NASR_ERR_ARG, 'utterance 2', f, short, labels, label_len, [rates[0], rates[1], 44100])
    refused(_lib.NASR_ERR_ARG, '[1,64]', f, [], np.zeros((0, 1), np.int32), [], None)
    many = [audios[2]] * 65
    refused(_lib.NASR_ERR_ARG, '[1,64]', f, many, np.ones((65, 1), np.int32), [1] * 65, None)
    # what validate_batch refuses, with the computed seq_len: the one-frame utterance cannot carry two labels
    assert seq[2] == 1
    two = labels.copy()
    two[2, :2] = (1, 2)
    with pytest.raises(_lib.InfeasibleLabelError) as err:
        e.upload_batch_audio(f, audios, two, [label_len[0], label_len[1], 2], rates)
    assert 'in sequence 2' in str(err.value) and 'available: 1' in str(err.value)
    refused(_lib.NASR_ERR_ARG, 'label_len[1]', f, audios, labels, [label_len[0], labels.shape[1] + 1, label_len[2]], rates)
    bad = labels.copy()
    bad[0, 0] = C - 1
    refused(_lib.NASR_ERR_ARG, 'label id', f, audios, bad, label_len, rates)
    # and the handle still works
    seq2, _ = e.upload_batch_audio(f, audios, labels, label_len, rates)
    assert [int(t) for t in seq2] == seq
    e.close()


def test_train_from_audio_equals_the_pickled_loop(tmp_path, caplog):
    """the same WAVs through preprocess_mfcc + train, and through train --from-audio: the same cost lines, the same
    parameters"""
    from neuralasr_amd import preprocess_mfcc, train
    from neuralasr_amd.features import write_wav16
    texts = ['hello world', 'a cat a dog', 'speech to text', 'one two three', 'front end', 'six seven', 'eight nine',
             'ten eleven', 'twelve', 'the last one']
    rows = []
    for i, text in enumerate(texts):
        rate = (E2E_SR, 16000, 44100)[i % 3]
        wav, txt = tmp_path / ('utt%d.wav' % i), tmp_path / ('utt%d.txt' % i)
        write_wav16(wav, speech_like(int(rate * (0.5 + 0.07 * i)), rate, 300 + i), rate)
        txt.write_text(text + '\n')
        rows.append('%s,%s,%d' % (wav, txt, os.path.getsize(wav) * E2E_SR // rate))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'mfcc'
    cfg_path = tmp_path / 'e2e.config'
    cfg_path.write_text(
        '[Parameters]\nsamplerate=%d\nnumcep=13\nnumcontext=2\nlabel_context=0\nbatch_size=3\nepochs=2\n'
        'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
        'sym_file=${MFCC Featurizer:output}/symbols\nnetwork=networks.bilstm_ctc_net.BiLstmCTCNet\n'
        '[Train]\ninput=${MFCC Featurizer:output}/train.scp\n[Test]\ninput=${MFCC Featurizer:output}/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\n' % (E2E_SR, tmp_path / 'model', tmp_path / 'data.csv', out))
    preprocess_mfcc.main([str(cfg_path)])

    def run(argv):
        caplog.clear()
        with caplog.at_level(logging.INFO):
            net = train.main(argv)
        lines = [r.getMessage() for r in caplog.records]
        steps = [m.split(', time')[0] for m in lines if m.startswith('Step: ')]
        valid = [m for m in lines if m.startswith('Valid: ')]
        net._settle()
        params = net.engine.get_params()
        kernels = state(net.engine)                        # an aborted recurrence repeats its step on other kernels
        net.engine.close()
        return steps, valid, params, kernels
    steps_p, valid_p, params_p, kernels_p = run([str(cfg_path)])
    steps_a, valid_a, params_a, kernels_a = run([str(cfg_path), '--from-audio'])
    print('\n'.join(steps_p + valid_p))
    note = 'recurrence %r (pickled loop), %r (from audio)' % (kernels_p, kernels_a)
    assert len(steps_p) == 6 and len(valid_p) == 6         # 8 training utterances in batches of 3, two epochs
    assert steps_a == steps_p and valid_a == valid_p, note
    assert same(params_a, params_p), note
