"""Host side of the augmentation of `train --from-audio`: the draws of augment.Augmenter, the masks an
AudioBatch carries through shard(), the counter of AudioFeed, the config keys, the refusals and the C ABI.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

SR = 8000
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg_ns(**kw):
    from types import SimpleNamespace
    base = dict(samplerate=SR, numcep=13, feature_size=65, spec_time_masks=2, spec_time_width=10, spec_time_ratio=1.0,
                spec_freq_masks=2, spec_freq_width=5, speed_perturb=(), augment_seed=0, start_step=0)
    base.update(kw)
    return SimpleNamespace(**base)


def make_corpus(tmp_path, batch_size=3, rand_shift=0, extra=''):
    """test_audio_batch_host.make_corpus: 11 utterances - sizes with ties, one missing WAV, one missing transcript, one
    transcription longer than its frames, one file at another rate; `extra` goes into [Parameters]"""
    from neuralasr_amd.features import write_wav16
    rs = np.random.RandomState(5)
    texts = ['Hello world.', 'A cat, a dog!', 'speech to text', 'one two three', 'GPU front end', 'six', 'seven of nine',
             'x' * 40, 'the last one', 'ten', 'eleven']
    secs = [0.50, 0.30, 0.50, 0.42, 0.30, 0.21, 0.50, 0.05, 0.33, 0.30, 0.26]
    rows = []
    for i, (text, sec) in enumerate(zip(texts, secs)):
        wav, txt = tmp_path / ('utt%02d.wav' % i), tmp_path / ('utt%02d.txt' % i)
        rate = 16000 if i == 3 else SR
        if i != 4:
            write_wav16(wav, 0.1 * rs.randn(int(rate * sec)), rate)
        if i != 5:
            txt.write_text(text + '\n')
        rows.append('%s,%s,%d' % (wav, txt, int(sec * 1000)))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'mfcc'
    cfg_path = tmp_path / 'a.config'
    cfg_path.write_text(
        '[Parameters]\nsamplerate=%d\nnumcep=13\nnumcontext=2\nlabel_context=1\nbatch_size=%d\nepochs=1\n'
        'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\nrand_shift=%d\n'
        '%snetwork=networks.bilstm_ctc_net.BiLstmCTCNet\n'
        '[Train]\ninput=${MFCC Featurizer:output}/train.scp\n[Test]\ninput=${MFCC Featurizer:output}/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\nstart_marker=^\nend_marker=$$\n'
        % (SR, batch_size, tmp_path / 'model', rand_shift, extra, tmp_path / 'data.csv', out))
    return cfg_path, out


# ---------------------------------------------------------------------------------------------------- draws
@pytest.mark.parametrize('width,ratio', [(10, 1.0), (100, 0.2), (3, 0.05), (0, 1.0)])
def test_masks_lie_inside_the_utterance_and_the_static_block(width, ratio):
    from neuralasr_amd.augment import Augmenter
    a = Augmenter(cfg_ns(spec_time_masks=8, spec_freq_masks=8, spec_time_width=width, spec_time_ratio=ratio, spec_freq_width=20))
    seq = [1, 2, 5, 19, 104, 500]          # len = 1, and ratio * len < 1 for the short ones
    widths = set()
    for counter in range(1, 40):
        tm, fm = a.masks(counter, seq)
        assert tm.shape == (len(seq), 8, 2) and fm.shape == (len(seq), 8, 2) and tm.dtype == fm.dtype == np.int32
        for i, n in enumerate(seq):
            t0, tw = tm[i, :, 0], tm[i, :, 1]
            assert (t0 >= 0).all() and (tw >= 0).all() and (t0 + tw <= n).all()
            assert (tw <= min(width, int(np.floor(ratio * n)))).all()
            f0, fw = fm[i, :, 0], fm[i, :, 1]
            assert (f0 >= 0).all() and (fw >= 0).all() and (f0 + fw <= 13).all()     # spec_freq_width 20 > numcep: capped
            if n == 500:
                widths.update(int(w) for w in tw)
    wmax = min(width, int(500 * ratio))
    if wmax <= 10:          # 312 draws over at most 11 values: every width of {0..wmax} turns up, the ends included
        assert widths == set(range(wmax + 1))
    else:                   # over 101 values: the whole range is in use
        assert min(widths) < 5 and max(widths) > wmax - 5 and len(widths) > wmax // 2
    if ratio * 2 < 1:
        assert not a.masks(3, [1, 2])[0][:, :, 1].any()


def test_draws_are_a_pure_function_of_their_key():
    from neuralasr_amd.augment import KIND_FREQ, KIND_SPEED, KIND_TIME, Augmenter
    a = Augmenter(cfg_ns(speed_perturb=(0.9, 1.0, 1.1)))
    seq = [50, 60, 70]
    first = a.masks(7, seq)
    np.random.seed(123)
    np.random.rand(10)                                   # the global state plays no part
    a.masks(9, seq[::-1])                                # nor do the draws made in between
    again = Augmenter(cfg_ns(speed_perturb=(0.9, 1.0, 1.1))).masks(7, seq)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    base = a.raw(7, 1, KIND_TIME, 0)
    others = [Augmenter(cfg_ns(augment_seed=1)).raw(7, 1, KIND_TIME, 0), a.raw(8, 1, KIND_TIME, 0),
              Augmenter(cfg_ns(), rank=1).raw(7, 1, KIND_TIME, 0), a.raw(7, 2, KIND_TIME, 0), a.raw(7, 1, KIND_FREQ, 0),
              a.raw(7, 1, KIND_SPEED, 0), a.raw(7, 1, KIND_TIME, 1)]
    assert len({base, *others}) == 8                     # seed, counter, rank, utterance, kind, mask index: each one matters
    # and in the arrays: utterance 1's masks are the same whatever stands beside it, and change with each of the four
    long = [200, 200, 200]
    t7 = a.masks(7, long)[0]
    assert np.array_equal(a.masks(7, [9, 200])[0][1], t7[1])
    assert not np.array_equal(a.masks(8, long)[0], t7)
    assert not np.array_equal(Augmenter(cfg_ns(augment_seed=5)).masks(7, long)[0], t7)
    assert not np.array_equal(Augmenter(cfg_ns(), rank=3).masks(7, long)[0], t7)
    assert not np.array_equal(t7[0], t7[1])


def test_shard_of_a_masked_batch_is_the_whole_batch_sliced():
    """the tower split plays no part: masks are drawn for the global batch and travel with their utterances"""
    from neuralasr_amd.augment import Augmenter
    from neuralasr_amd.networks.hipnetwork import take_shard
    rs = np.random.RandomState(0)
    audios = [0.1 * rs.randn(n).astype(np.float32) for n in (4000, 2400, 3000, 1700)]
    a = Augmenter(cfg_ns())
    b = a.batch(4, audios, None)
    tm, fm = a.masks(4, b.seq_len)
    assert np.array_equal(b.time_masks, tm) and np.array_equal(b.freq_masks, fm) and tm[:, :, 1].any()
    labels = np.zeros((4, 2), np.int32)
    for world in (2, 4):
        got_t, got_f = [], []
        for rank in range(world):
            s = take_shard(b, labels, b.seq_len, [2] * 4, world, rank)[0]
            assert len(s) == 4 // world and s.shape[1] == max(int(x) for x in s.seq_len)
            got_t.append(s.time_masks)
            got_f.append(s.freq_masks)
        assert np.array_equal(np.concatenate(got_t), tm) and np.array_equal(np.concatenate(got_f), fm)
    aug = b.shard(1, 3).aug(13)
    assert aug.static_width == 13 and np.array_equal(aug.time_masks, tm[1:3])
    from neuralasr_amd.features import AudioBatch
    assert AudioBatch(SR, audios).aug(13) is None and AudioBatch(SR, audios).shard(0, 2).time_masks is None
    with pytest.raises(ValueError, match='time_masks'):
        AudioBatch(SR, audios, time_masks=np.zeros((3, 1, 2), np.int32))


def test_resumed_feed_draws_what_the_uninterrupted_one_drew(tmp_path):
    """The counter is the global step the batch trains: start_step + the batches handed out, this one included.  A feed
    made with start_step = k draws for its first batch what a fresh feed draws for batch index k (its k+1-th: the batch
    that trains step k+1 in either run)."""
    from neuralasr_amd.audio_dataset import AudioDataSet, AudioFeed
    from neuralasr_amd.augment import Augmenter
    from neuralasr_amd.config import Config
    keys = 'spec_time_masks=2\nspec_time_width=8\nspec_freq_masks=1\nspec_freq_width=4\nspeed_perturb=0.9,1.0,1.1\naugment_seed=3\n'
    cfg_path, _ = make_corpus(tmp_path, batch_size=5, extra=keys)

    def feed(start_step):
        config = Config(str(cfg_path), True)
        config.start_step = start_step
        return AudioFeed(AudioDataSet(config.mfcc_input, config, 'train'), Augmenter(config))
    fresh, k = feed(0), 2
    batches = []
    for _ in range(k + 1):
        batches.append(fresh.get_next_batch()[0])
        fresh.reset_epoch()                              # one batch per epoch: every step sees the same five utterances
    assert not np.array_equal(batches[0].time_masks, batches[1].time_masks)
    first = feed(k).get_next_batch()[0]
    assert first.rates == batches[k].rates and [int(t) for t in first.seq_len] == [int(t) for t in batches[k].seq_len]
    assert np.array_equal(first.time_masks, batches[k].time_masks) and np.array_equal(first.freq_masks, batches[k].freq_masks)
    # a feed without an augmenter (validation, decode) hands out plain batches
    plain = AudioFeed(AudioDataSet(Config(str(cfg_path), True).mfcc_input, Config(str(cfg_path), True), 'train'))
    b = plain.get_next_batch()[0]
    assert b.time_masks is None and b.freq_masks is None and 16000 in b.rates and set(b.rates) <= {SR, 16000}


def test_speed_perturbation_declares_the_rate(tmp_path):
    from neuralasr_amd.audio_dataset import AudioDataSet
    from neuralasr_amd.augment import KIND_SPEED, Augmenter
    from neuralasr_amd.config import Config
    from neuralasr_amd.features import AudioBatch
    cfg_path, _ = make_corpus(tmp_path, batch_size=5, extra='speed_perturb=0.9,1.0,1.1\n')
    config = Config(str(cfg_path), True)
    ds = AudioDataSet(config.mfcc_input, config, 'train')
    audios, rates, _, _ = ds.get_next_batch()
    assert sorted(rates) == [SR] * 4 + [16000] and len(ds.last_chars) == 5
    a = Augmenter(config)
    plain = AudioBatch(SR, audios, rates)
    seen = set()
    for counter in range(1, 30):
        new, factors = a.speed(counter, [x.size for x in audios], rates, ds.last_chars)
        b = a.batch(counter, audios, rates, ds.last_chars)
        assert b.rates == new and b.time_masks is None and b.freq_masks is None
        for i, (r, f) in enumerate(zip(rates, factors)):
            assert f == (0.9, 1.0, 1.1)[a.raw(counter, i, KIND_SPEED)[0] % 3]       # nothing here is short enough to be refused
            assert new[i] == (r if f == 1.0 else int(round(r * f)))
            if f == 1.0:
                assert int(b.seq_len[i]) == int(plain.seq_len[i])
            else:                                        # 1/f of the length, to within the frame grid
                assert abs(int(b.seq_len[i]) - int(plain.seq_len[i]) / f) <= 1.5
            seen.add(f)
    assert seen == {0.9, 1.0, 1.1}
    # an utterance that the perturbation would leave with fewer frames than characters keeps factor 1.0 (kept_rows' rule)
    fast = Augmenter(cfg_ns(speed_perturb=(1.9,), spec_time_masks=0, spec_freq_masks=0))
    sizes = [x.size for x in audios]
    frames = [fast.frames(n, r) for n, r in zip(sizes, rates)]
    shrunk = [fast.frames(n, int(round(r * 1.9))) for n, r in zip(sizes, rates)]
    chars = [shrunk[0] + 1, shrunk[1], frames[2], 0, shrunk[4] + 1]       # 0 and 4 do not fit any more; 2 is on kept_rows' edge
    new, factors = fast.speed(1, sizes, rates, chars)
    assert factors == [1.0, 1.9, 1.0, 1.9, 1.0]
    assert new == [rates[0], int(round(rates[1] * 1.9)), rates[2], int(round(rates[3] * 1.9)), rates[4]]
    # without speed_perturb the rates pass through
    assert Augmenter(cfg_ns()).speed(1, sizes, rates, chars) == (list(rates), [1.0] * 5)


# ---------------------------------------------------------------------------------------------------- config
def test_config_defaults_are_off_and_bad_values_name_their_key(tmp_path):
    from neuralasr_amd.config import Config
    cfg_path, _ = make_corpus(tmp_path)
    c = Config(str(cfg_path), True)
    assert (c.spec_time_masks, c.spec_time_width, c.spec_time_ratio, c.spec_freq_masks, c.spec_freq_width, c.speed_perturb,
            c.augment_seed, c.augment_on) == (0, 0, 1.0, 0, 0, (), 0, False)
    assert c.feature_size == 65 and c.rand_shift == 0
    good = 'spec_time_masks=2\nspec_time_width=40\nspec_time_ratio=0.2\nspec_freq_masks=8\nspec_freq_width=7\n' \
           'speed_perturb=0.9, 1.0,1.1\naugment_seed=11\n'
    cfg_path, _ = make_corpus(tmp_path, extra=good)
    c = Config(str(cfg_path), True)
    assert (c.spec_time_masks, c.spec_time_width, c.spec_time_ratio, c.spec_freq_masks, c.spec_freq_width, c.speed_perturb,
            c.augment_seed, c.augment_on) == (2, 40, 0.2, 8, 7, (0.9, 1.0, 1.1), 11, True)
    for bad in ('spec_time_masks=9', 'spec_time_masks=-1', 'spec_time_masks=two', 'spec_time_width=-1', 'spec_time_width=1.5',
                'spec_time_ratio=1.5', 'spec_time_ratio=-0.1', 'spec_time_ratio=nan', 'spec_freq_masks=9', 'spec_freq_masks=x',
                'spec_freq_width=-2', 'speed_perturb=0.5', 'speed_perturb=0.9,2.0', 'speed_perturb=fast', 'speed_perturb=',
                'augment_seed=-1', 'augment_seed=1.0'):
        cfg_path, _ = make_corpus(tmp_path, extra=bad + '\n')
        with pytest.raises(ValueError) as e:
            Config(str(cfg_path), True)
        assert "'%s'" % bad.split('=')[0] in str(e.value) and str(cfg_path) in str(e.value), bad


def test_refusals(tmp_path):
    from neuralasr_amd import train
    cfg_path, _ = make_corpus(tmp_path, extra='spec_time_masks=1\n')
    with pytest.raises(ValueError, match='--from-audio'):
        train.main([str(cfg_path)])
    cfg_path, _ = make_corpus(tmp_path, extra='speed_perturb=0.9\n')
    with pytest.raises(ValueError, match='--from-audio'):
        train.main([str(cfg_path)])
    cfg_path, _ = make_corpus(tmp_path, rand_shift=3, extra='spec_time_masks=1\n')
    with pytest.raises(ValueError, match='rand_shift'):
        train.main([str(cfg_path), '--from-audio'])


def test_the_product_does_not_import_the_oracle_for_its_draws():
    src = open(os.path.join(ROOT, 'neuralasr_amd', 'augment.py')).read()
    assert 'import torch' not in src and 'oracle' not in src.replace('the oracle', '')


# ---------------------------------------------------------------------------------------------------- ABI
def test_aug_symbols_and_struct_layout(tmp_path):
    import shutil
    import subprocess
    from neuralasr_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    H, fp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    lp, cp, ap = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_lib.BatchAug)
    ci = ctypes.c_int
    audio = [H, H, fp, lp, ip, ip, ip, ci, ci, ip, cp]
    for name, args in (('nasr_upload_batch_context_aug', [H, fp, fp, ci, ci, ip, ip, ip, ci, ci, ci, ap]),
                       ('nasr_upload_batch_audio_aug', audio + [ap]), ('nasr_stage_batch_audio_aug', audio + [ap, cp])):
        assert name in _lib.SYMBOLS
        assert hasattr(raw, name), name + ' is not exported by libnasr.so'
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
    header = open(os.path.join(ROOT, 'include', 'nasr.h')).read()
    assert '#define NASR_AUG_MAX_MASKS 8' in header and _lib.AUG_MAX_MASKS == 8
    for name in ('nasr_upload_batch_context_aug', 'nasr_upload_batch_audio_aug'):
        decl = header[:header.index('int ' + name + '(')]
        assert 'No counterpart in the reference' in decl[decl.rindex('/*'):]
    B = _lib.BatchAug
    assert [n for n, _ in B._fields_] == ['static_width', 'n_time', 'n_freq', 'time_mask', 'freq_mask']
    assert (B.static_width.offset, B.n_time.offset, B.n_freq.offset, B.time_mask.offset, B.freq_mask.offset) == (0, 4, 8, 16, 24)
    assert ctypes.sizeof(B) == 32
    gcc = shutil.which('gcc')
    if gcc:                                              # the layout a C caller sees
        src = tmp_path / 'aug.c'
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nasr.h"\nint main(void) {\n'
                       '  printf("%zu %zu %zu %zu %zu %zu %d\\n", sizeof(nasr_batch_aug), offsetof(nasr_batch_aug, static_width),\n'
                       '         offsetof(nasr_batch_aug, n_time), offsetof(nasr_batch_aug, n_freq), offsetof(nasr_batch_aug, time_mask),\n'
                       '         offsetof(nasr_batch_aug, freq_mask), NASR_AUG_MAX_MASKS);\n  return 0;\n}\n')
        exe = tmp_path / 'aug'
        r = subprocess.run([gcc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
        assert [int(x) for x in out.stdout.split()] == [32, 0, 4, 8, 16, 24, 8]


def test_engine_aug_struct_checks_shapes():
    from neuralasr_amd.engine import BatchAug
    tm = np.array([[[0, 2], [3, 0]], [[1, 1], [0, 0]]], np.int64)
    st, keep = BatchAug(13, tm, None).struct(2)
    assert (st.static_width, st.n_time, st.n_freq) == (13, 2, 0)
    assert [st.time_mask[i] for i in range(8)] == [0, 2, 3, 0, 1, 1, 0, 0] and keep[0].dtype == np.int32
    with pytest.raises(ValueError, match=r'\[B=3, n, 2\]'):
        BatchAug(13, tm, None).struct(3)
