"""GPU: audio in the LAS network and in decode.py.  The resident entry points (nasr_las_forward_resident,
nasr_las_beam_search_resident) after LasEngine.upload_batch_audio, the LAS plugin's *_audio calls, train --from-audio with
LAS, decode --from-audio and decode_wav, each against the feature route: Featurizer.compute(audios, rates=...), zero-padded
to the batch's longest utterance and given to the existing feature calls.  Both routes put the same bits in the batch slot
and run the same kernels after it, so everything is compared as bits.

One corpus serves every test (test_audio_batch_host.make_corpus): 8 kHz, numcep 13, numcontext 2, utterances of 0.2 to
0.5 s (19 to 49 frames), utt03 at 16 kHz so that the resampler is on the path, start and end markers set."""
import ctypes
import logging
import os

import numpy as np
import pytest

from test_audio_batch_host import SR, make_corpus
from test_las_audio_host import las_config

pytestmark = pytest.mark.gpu

NUMCEP, NUMCONTEXT = 13, 2
W, STEPS, LP = 1000, 100, 0.5          # the reference's inference graph, as tests/test_gpu_las_decode_e2e.py runs it


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    """(directory, LAS config, {name: (float32 audio, rate)}, BiLstmCTCNet config): the WAVs, the CSV, and what
    preprocess_mfcc makes of them (pickles, lists, symbol table).  The tests only add model directories."""
    from neuralasr_amd import preprocess_mfcc
    from neuralasr_amd.features import read_wav_native
    d = tmp_path_factory.mktemp('las_audio')
    ctc_path, _ = make_corpus(d)
    text = ctc_path.read_text()
    cfg_path = d / 'las.config'
    cfg_path.write_text(text)
    las_config(cfg_path)
    ctc_path.write_text(text.replace('model_dir=%s\n' % (d / 'model'), 'model_dir=%s\n' % (d / 'model_ctc')))
    assert 'model_ctc' in ctc_path.read_text()
    preprocess_mfcc.main([str(cfg_path)])
    wavs = {p.name[:-4]: read_wav_native(str(p)) for p in sorted(d.glob('utt*.wav'))}
    assert wavs['utt03'][1] == 16000 and all(r == SR for n, (_, r) in wavs.items() if n != 'utt03')
    return d, cfg_path, wavs, ctc_path


@pytest.fixture(scope='module')
def fz():
    from neuralasr_amd.features import Featurizer
    f = Featurizer(SR, NUMCEP, NUMCONTEXT)
    yield f
    f.close()


def host_feats(f, audios, rates):
    """the feature route's array: the features through the host, zero-padded to the batch's longest utterance"""
    feats = f.compute(audios, rates=rates)
    T = max(x.shape[0] for x in feats)
    out = np.zeros((len(feats), T, f.width), np.float32)
    for b, x in enumerate(feats):
        out[b, :x.shape[0]] = x
    return out, [np.asarray(x.shape[0], dtype=np.int32) for x in feats]


def pick(wavs, names):
    return [wavs[n][0] for n in names], [wavs[n][1] for n in names]


# ---------------------------------------------------------------------------------------------- the engine
C = 12
RAGGED = ['utt05', 'utt03', 'utt00']    # 0.21 s, 0.42 s at 16 kHz, 0.50 s


def las_engine(F, p=0.5):
    from neuralasr_amd.engine import LasEngine
    from neuralasr_amd.networks.las import LAS
    e = LasEngine(F, C, sampling_probability=p, seed=5, learning_rate=1e-3)
    e.set_params(LAS.__new__(LAS).initial_params(e.tensors(), seed=3))
    return e


def dense_labels(B, U=6):
    rs = np.random.RandomState(9)
    return rs.randint(0, C, size=(B, U)).astype(np.int32), [U, 3, 1][:B]


BEAM_KEYS = ('predicted_ids', 'scores', 'word_ids', 'parent_ids', 'log_probs', 'lengths', 'finished')


def assert_same_search(got, want):
    assert got['steps'] == want['steps']
    for k in BEAM_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].tobytes() == want[k].tobytes(), k + ' differs'


def test_resident_calls_equal_the_feature_calls(corpus, fz):
    audios, rates = pick(corpus[2], RAGGED)
    labels, ll = dense_labels(3)
    feats, seq = host_feats(fz, audios, rates)
    assert len({int(t) for t in seq}) == 3 and feats.shape[1] == 49
    e = las_engine(fz.width)
    p, seed, _, tower = e.sampling_state()
    # audio route
    seq_a, T_a = e.upload_batch_audio(fz, audios, labels, ll, rates)
    assert [int(t) for t in seq_a] == [int(t) for t in seq] and T_a == feats.shape[1]
    got = e.beam_search_resident(W, STEPS, 1, 2, LP, trace=True)
    e.set_sampling_state(p, seed, 7, tower)
    got_logits = e.las_forward_resident(sample=True)
    got_fed, got_sampled, got_loss, got_state = e.fed_ids(), e.sampled(), e.get_loss(), e.sampling_state()
    # feature route
    want = e.beam_search(feats, seq, W, STEPS, 1, 2, LP, trace=True)
    e.set_sampling_state(p, seed, 7, tower)
    want_logits = e.las_forward(feats, seq, labels, ll, sample=True)
    assert_same_search(got, want)
    assert want_logits.shape == (3, 6, C) and same(got_logits, want_logits)
    assert np.array_equal(got_fed, e.fed_ids()) and np.array_equal(got_sampled, e.sampled())
    assert got_sampled.any(), 'no step was fed a sample: the comparison would not see the sampling state'
    assert same(got_loss, e.get_loss()) and got_state == e.sampling_state() == (p, seed, 8, tower)
    # sample off, and without an output buffer
    assert same(e.las_forward_resident(sample=False), e.las_forward(feats, seq, labels, ll, sample=False))
    assert e.lib.nasr_las_forward_resident(e.h, 0, None) == 0 and e.sampling_state()[2] == 8
    e.close()


def test_search_leaves_the_resident_batch_alone(corpus, fz):
    audios, rates = pick(corpus[2], RAGGED)
    labels, ll = dense_labels(3)
    e = las_engine(fz.width)
    state = e.sampling_state()

    def grads(search):
        e.set_sampling_state(*state)
        e.upload_batch_audio(fz, audios, labels, ll, rates)
        if search:
            e.beam_search_resident(W, STEPS, 1, 2, LP)
        e.compute_grads()
        return e.get_loss(), e.get_grads(), e.logits()
    a, b = grads(False), grads(True)
    assert np.abs(a[1]).max() > 0
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[2], b[2])
    e.close()


def test_state_and_argument_errors(corpus, fz):
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine
    steps = ctypes.c_int32()

    def search(e, width=4):
        return e.lib.nasr_las_beam_search_resident(e.h, width, 5, 1, 2, LP, ctypes.byref(steps))

    def forward(e):
        return e.lib.nasr_las_forward_resident(e.h, 1, None)

    def refused(e, rc, code, text):
        msg = e.lib.nasr_last_error(e.h).decode()
        assert rc == code and text in msg, (rc, msg)

    fresh = las_engine(fz.width)
    refused(fresh, search(fresh), _lib.NASR_ERR_STATE, 'nasr_las_beam_search_resident: no resident batch')
    refused(fresh, forward(fresh), _lib.NASR_ERR_STATE, 'nasr_las_forward_resident: no resident batch')
    ctc = Engine(fz.width, 16, 1, True, 'stack_reshape', C)
    refused(ctc, search(ctc), _lib.NASR_ERR_STATE, 'nasr_las_beam_search_resident: not a LAS handle')
    refused(ctc, forward(ctc), _lib.NASR_ERR_STATE, 'nasr_las_forward_resident: not a LAS handle')
    ctc.close()
    audios, rates = pick(corpus[2], RAGGED)
    labels, ll = dense_labels(3)
    fresh.upload_batch_audio(fz, audios, labels, ll, rates)
    refused(fresh, search(fresh, width=0), _lib.NASR_ERR_ARG, 'beam_width must be in [1,1024]')
    refused(fresh, search(fresh, width=1025), _lib.NASR_ERR_ARG, 'beam_width must be in [1,1024]')
    assert search(fresh) == _lib.NASR_OK and 1 <= steps.value <= 5
    # a batch without labels can be searched; the decoder pass needs them
    fresh.upload_batch_audio(fz, audios, None, None, rates)
    assert search(fresh) == _lib.NASR_OK
    refused(fresh, forward(fresh), _lib.NASR_ERR_ARG, 'needs labels')
    fresh.close()


# ---------------------------------------------------------------------------------------------- the plugin
def two_networks(corpus, tmp_path, num_gpus=1):
    """(network fed audio, network fed features, training AudioDataSet, test AudioDataSet): the same seed, a model
    directory each"""
    from neuralasr_amd.audio_dataset import AudioDataSet
    from neuralasr_amd.config import Config
    cfg_path = corpus[1]
    nets = []
    for tag in ('audio', 'feats'):
        config = Config(str(cfg_path), True)
        config.model_dir = str(tmp_path / ('model_' + tag))
        config.num_gpus = num_gpus
        train_set = AudioDataSet(config.mfcc_input, config, 'train')
        test_set = AudioDataSet(config.mfcc_input, config, 'test')
        nets.append(config.load_network(fortraining=True))
    assert nets[0].beam_width == W and nets[0].max_decode_steps == STEPS and nets[0].length_penalty_weight == LP
    return nets[0], nets[1], train_set, test_set


def compose(ads, names):
    """the utterances `names` as AudioDataSet.get_next_batch composes a batch"""
    by_name = dict(zip(ads.names(), ads.X))
    items = [ads.load(by_name[n]) for n in names]
    labels = np.full((len(items), max(n for _, _, _, n in items)), ads.padding_id, dtype=np.int32)
    for i, (_, _, l, n) in enumerate(items):
        labels[i, :n] = l
    return [a for a, _, _, _ in items], [r for _, r, _, _ in items], labels, [n for _, _, _, n in items]


def handle_state(net):
    m, v, step = net.engine.get_adam_state()
    return net.engine.get_params(), m, v, step, net.engine.sampling_state()


def assert_same_handles(a, b):
    sa, sb = handle_state(a), handle_state(b)
    assert same(sa[0], sb[0]), 'parameters differ'
    assert same(sa[1], sb[1]) and same(sa[2], sb[2]) and sa[3] == sb[3], 'Adam state differs'
    assert sa[4] == sb[4], 'sampling state differs'


def run_both_routes(net_a, net_f, fz, train_batches, eval_batch):
    """three steps, then validate, evaluate and decode: the audio calls of net_a against the feature calls of net_f"""
    for audios, rates, labels, ll in train_batches:
        feats, seq = host_feats(fz, audios, rates)
        got = net_a.train_audio(audios, rates, labels, ll)
        want = net_f.train(feats, labels, seq, ll)
        print('step %d: loss %r ler %r (audio), %r %r (features)' % (net_a.global_step, got[0], got[1], want[0], want[1]))
        assert np.isfinite(want[0]) and same(got[0], want[0]) and same(got[1], want[1])
    assert net_a.global_step == net_f.global_step == len(train_batches)
    assert_same_handles(net_a, net_f)
    assert net_a.engine.sampling_state()[2] == len(train_batches)
    audios, rates, labels, ll = eval_batch
    feats, seq = host_feats(fz, audios, rates)
    got, want = net_a.validate_audio(audios, rates, labels, ll), net_f.validate(feats, labels, seq, ll)
    assert np.isfinite(want[0]) and same(got[0], want[0]) and same(got[1], want[1])
    got, want = net_a.evaluate_audio(audios, rates, labels, ll), net_f.evaluate(feats, labels, seq, ll)
    assert want[0].shape[0] == len(audios) and got[0].dtype == want[0].dtype and np.array_equal(got[0], want[0])
    assert same(got[1], want[1]) and same(got[2], want[2])          # (NaN when T_dec != U: the same NaN bits)
    got, want = net_a.decode_audio(audios, rates), net_f.decode(feats, seq)
    assert want.ndim == 1 and got.dtype == want.dtype and np.array_equal(got, want)
    assert_same_handles(net_a, net_f)                                # validate drew once more; the searches drew nothing
    assert net_a.engine.sampling_state()[2] == len(train_batches) + 1


def test_plugin_audio_calls_equal_the_feature_calls(corpus, fz, tmp_path):
    net_a, net_f, train_set, test_set = two_networks(corpus, tmp_path)
    assert net_a.takes_audio and train_set.config.batch_size == 3
    batches = [train_set.get_next_batch(), train_set.get_next_batch()]
    assert 16000 in batches[0][1] and not train_set.has_more_batches()
    run_both_routes(net_a, net_f, fz, batches + batches[:1], test_set.get_next_batch())
    assert net_a.stage_batch(net_a.audio_batch(*batches[0][:2]), batches[0][2], None, batches[0][3]) is False


def test_plugin_two_towers(corpus, fz, tmp_path):
    """num_gpus = 2 towers time-sliced, B 4.  The feature route keeps the whole batch's padded length for every tower and
    the audio route pads each tower to its own longest utterance, so the batches are ordered short, long, long, short
    with both long ones at the batch's length (0.50 s, 49 frames): each tower's longest utterance is the batch's, and the
    two routes give every tower the same array."""
    net_a, net_f, train_set, _ = two_networks(corpus, tmp_path, num_gpus=2)
    orders = [['utt01', 'utt00', 'utt02', 'utt03'], ['utt00', 'utt01', 'utt03', 'utt06']]
    batches = [compose(train_set, names) for names in orders]
    for audios, rates, _, _ in batches:
        b = net_a.audio_batch(audios, rates)
        assert [b.shard(lo, lo + 2).shape[1] for lo in (0, 2)] == [b.shape[1]] * 2 == [49, 49]
        assert 16000 in rates
    assert net_a._towers() == (2, [0, 1])
    run_both_routes(net_a, net_f, fz, batches + batches[:1], batches[1])


# ---------------------------------------------------------------------------------------------- the scripts
def logged(caplog, fn):
    caplog.clear()
    with caplog.at_level(logging.INFO):
        result = fn()
    return result, [r.getMessage() for r in caplog.records]


def decode_lines(lines):
    """what decode() logs, without the wall time"""
    keep = [m for m in lines if m.startswith(('Valid: ', 'Decoded: ', 'Original: '))]
    done = [m[m.index('avg_loss'):] for m in lines if m.startswith('Decoded Time')]
    assert len(done) == 1
    return keep + done


def test_train_and_decode_from_audio_with_las(corpus, caplog, monkeypatch):
    from neuralasr_amd import decode, decode_wav, train
    from neuralasr_amd.config import Config
    from neuralasr_amd.features import Featurizer, read_wav_native
    from neuralasr_amd.networks.las import LAS
    tmp_path, cfg_path = corpus[0], corpus[1]

    def run(argv):
        net, lines = logged(caplog, lambda: train.main(argv))
        steps = [m.split(', time')[0] for m in lines if m.startswith('Step: ')]
        valid = [m for m in lines if m.startswith('Valid: ')]
        files = sorted(os.listdir(tmp_path / 'model'))
        with np.load(tmp_path / 'model' / ('model-%d.npz' % net.global_step)) as z:
            ckpt = {k: z[k].copy() for k in z.files}
        net.engine.close()
        return steps, valid, files, ckpt
    steps_p, valid_p, files_p, ckpt_p = run([str(cfg_path)])
    steps_a, valid_a, files_a, ckpt_a = run([str(cfg_path), '--from-audio'])
    print('\n'.join(steps_p + valid_p))
    assert len(steps_p) == 2 and len(valid_p) == 2                    # 5 training utterances in batches of 3, one epoch
    assert steps_a == steps_p and valid_a == valid_p
    assert files_a == files_p and sorted(ckpt_a) == sorted(ckpt_p) and 'las_sampling' in ckpt_p
    for k in ckpt_p:
        assert ckpt_a[k].dtype == ckpt_p[k].dtype and ckpt_a[k].tobytes() == ckpt_p[k].tobytes(), k + ' differs'

    # decode over the test list, from the checkpoint just written
    _, lines_p = logged(caplog, lambda: decode.main([str(cfg_path)]))
    _, lines_a = logged(caplog, lambda: decode.main([str(cfg_path), '--from-audio']))
    want = decode_lines(lines_p)
    print('\n'.join(want))
    assert len(want) == 3 * 3 + 1 and decode_lines(lines_a) == want

    # decode_wav: a LAS config goes through decode_audio, and logs what the feature route logs
    calls = []
    plain = LAS.decode_audio
    monkeypatch.setattr(LAS, 'decode_audio', lambda self, *a, **k: calls.append(1) or plain(self, *a, **k))
    wav = str(tmp_path / 'utt03.wav')
    text_a, lines_a = logged(caplog, lambda: decode_wav.main([str(cfg_path), wav]))
    assert calls == [1]
    config = Config(str(cfg_path), True)
    f = Featurizer(config.samplerate, config.numcep, config.numcontext)
    audio, rate = read_wav_native(wav)
    assert rate == 16000
    mfcc = f.compute([audio], rates=[rate])[0][None]
    f.close()
    text_f, lines_f = logged(caplog, lambda: decode_wav.decode(config, mfcc, [np.asarray(mfcc.shape[1], dtype=np.int32)]))
    one = [m for m in lines_f if m.startswith('Decoded: ')]
    assert len(one) == 1 and [m for m in lines_a if m.startswith('Decoded: ')] == one and text_a == text_f


def test_decode_from_audio_with_a_ctc_network(corpus, caplog):
    from neuralasr_amd import decode
    from neuralasr_amd.config import Config
    cfg_path = corpus[3]
    net = Config(str(cfg_path), True).load_network(fortraining=True)
    net.save_checkpoint()
    net.engine.close()
    _, lines_p = logged(caplog, lambda: decode.main([str(cfg_path)]))
    _, lines_a = logged(caplog, lambda: decode.main([str(cfg_path), '--from-audio']))
    want = decode_lines(lines_p)
    print('\n'.join(want))
    assert len(want) == 3 * 3 + 1 and decode_lines(lines_a) == want
