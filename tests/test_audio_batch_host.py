"""Host side of batches from audio: the two C entry points are exported and bound, and AudioDataSet composes the batches
that preprocess_mfcc + DataSet compose from the same CSV (names and labels; the features need a GPU)."""
import ctypes
import os

import numpy as np
import pytest

SR = 8000


def test_audio_batch_symbols_are_exported_and_bound():
    from neuralasr_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    H, fp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    lp, cp = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)
    common = [H, H, fp, lp, ip, ip, ip, ctypes.c_int, ctypes.c_int, ip, cp]
    for name, args in (('nasr_upload_batch_audio', common), ('nasr_stage_batch_audio', common + [cp])):
        assert name in _lib.SYMBOLS
        assert hasattr(raw, name), name + ' is not exported by libnasr.so'
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'nasr.h')).read()
    for name in ('nasr_upload_batch_audio', 'nasr_stage_batch_audio'):
        decl = header[:header.index('int ' + name + '(')]
        comment = decl[decl.rindex('/*'):]
        assert 'utils.py:24-31' in comment and 'dataset.py:33-40' in comment


def make_corpus(tmp_path, batch_size=3, rand_shift=0, sym_file=True):
    """11 utterances: sizes with ties, one missing WAV, one missing transcript, one transcription longer than its
    frames, one file at another rate"""
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
        rows.append('%s,%s,%d' % (wav, txt, int(sec * 1000)))       # ties: 0.50 x3, 0.30 x3
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'mfcc'
    cfg_path = tmp_path / 'a.config'
    cfg_path.write_text(
        '[Parameters]\nsamplerate=%d\nnumcep=13\nnumcontext=2\nlabel_context=1\nbatch_size=%d\nepochs=1\n'
        'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\nrand_shift=%d\n'
        '%snetwork=networks.bilstm_ctc_net.BiLstmCTCNet\n'
        '[Train]\ninput=${MFCC Featurizer:output}/train.scp\n[Test]\ninput=${MFCC Featurizer:output}/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\nstart_marker=^\nend_marker=$$\n'
        % (SR, batch_size, tmp_path / 'model', rand_shift, 'sym_file=${MFCC Featurizer:output}/symbols\n' if sym_file else '',
           tmp_path / 'data.csv', out))
    return cfg_path, out


def host_featurize(config):
    """frame counts without a GPU: zeros of the right shape (preprocess_mfcc only reads shape[0] for its filter)"""
    from neuralasr_amd.features import num_frames, read_wav_native, resample_length

    def run(paths):
        feats = []
        for p in paths:
            a, r = read_wav_native(p)
            n = a.size if r == config.samplerate else resample_length(a.size, r, config.samplerate)[0]
            feats.append(np.zeros((num_frames(n, config.samplerate), config.feature_size), np.float32))
        return feats
    return run


@pytest.mark.parametrize('existing_symbols', [True, False])
def test_audio_dataset_composes_the_batches_of_preprocess_and_dataset(tmp_path, existing_symbols):
    from neuralasr_amd import preprocess_mfcc
    from neuralasr_amd.audio_dataset import AudioDataSet
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    cfg_path, out = make_corpus(tmp_path)
    preprocess_mfcc.main([str(cfg_path)], featurize=host_featurize(Config(str(cfg_path))))
    want_symbols = (out / 'symbols').read_text()
    if not existing_symbols:
        os.rename(out / 'symbols', out / 'symbols.preprocess')      # AudioDataSet has to rebuild the same table
    for which, scp in (('train', 'train.scp'), ('test', 'test.scp')):
        config = Config(str(cfg_path), True)
        ads = AudioDataSet(config.mfcc_input, config, which)
        if not existing_symbols:
            assert (out / 'symbols').read_text() == want_symbols
        cfg2 = Config(str(cfg_path), True)
        ds = DataSet(str(out / scp), cfg2)
        names = [os.path.basename(p)[:-4] for p in ds.X]
        assert ads.names() == names and ads.get_num_of_sample() == ds.get_num_of_sample()
        if which == 'train':
            # 8 rows: utt04 (no WAV), utt05 (no transcript) and utt07 (40 characters, 4 frames) leave; ties in CSV order
            assert names == ['utt01', 'utt03', 'utt00', 'utt02', 'utt06']
        for item, path in zip(ads.X, ds.X):
            _, labels, _, n = ds.load_pkl(path)
            assert item[1].dtype == np.int32 and np.array_equal(item[1], labels) and n == len(labels)
        nb = 0
        while ds.has_more_batches():
            assert ads.has_more_batches()
            _, labels, seq_len, labels_len = ds.get_next_batch()
            audios, rates, alabels, alabels_len = ads.get_next_batch()
            assert np.array_equal(alabels, labels) and list(alabels_len) == list(labels_len)
            assert len(audios) == len(seq_len) == len(rates) == config.batch_size     # the duplicated tail included
            from neuralasr_amd.features import AudioBatch
            b = AudioBatch(config.samplerate, audios, rates, config.feature_size)
            assert [int(t) for t in b.seq_len] == [int(t) for t in seq_len]
            assert all(a.dtype == np.float32 for a in audios)
            nb += 1
        assert not ads.has_more_batches() and nb == -(-len(names) // config.batch_size)
        ads.reset_epoch()
        assert ads.has_more_batches()
        assert ads.get_feature_shape() == ds.get_feature_shape() and ads.get_label_shape() == ds.get_label_shape()


def test_mixed_rates_reach_the_batch(tmp_path):
    from neuralasr_amd.audio_dataset import AudioDataSet
    from neuralasr_amd.config import Config
    cfg_path, _ = make_corpus(tmp_path, batch_size=8, sym_file=False)
    config = Config(str(cfg_path), True)
    ads = AudioDataSet(config.mfcc_input, config, 'train')
    _, rates, _, _ = ads.get_next_batch()
    assert sorted(set(rates)) == [SR, 16000]


def test_from_audio_refuses_rand_shift(tmp_path):
    from neuralasr_amd import train
    from neuralasr_amd.audio_dataset import AudioDataSet
    from neuralasr_amd.config import Config
    cfg_path, _ = make_corpus(tmp_path, rand_shift=3, sym_file=False)
    with pytest.raises(ValueError, match='rand_shift'):
        train.main([str(cfg_path), '--from-audio'])
    with pytest.raises(ValueError, match='rand_shift'):
        AudioDataSet(str(tmp_path / 'data.csv'), Config(str(cfg_path), True))


def test_wav_info_agrees_with_the_decoder(tmp_path):
    """the header-only length and rate AudioDataSet filters by are those of the decoded file"""
    import struct
    from neuralasr_amd.features import read_wav_native, wav_info, write_wav16
    rs = np.random.RandomState(1)
    p = tmp_path / 'a.wav'
    write_wav16(p, 0.1 * rs.randn(1234), 22050)
    a, r = read_wav_native(str(p))
    assert wav_info(str(p)) == (a.size, r) == (1234, 22050)
    # stereo 24-bit with a chunk in front of fmt, an odd-sized chunk in front of data, and a data chunk cut short
    pcm = rs.randint(0, 256, size=3 * 2 * 100 + 4).astype(np.uint8).tobytes()
    fmt = struct.pack('<HHIIHH', 1, 2, 8000, 8000 * 6, 6, 24)
    body = (b'WAVE' + b'LIST' + struct.pack('<I', 4) + b'abcd' + b'fmt ' + struct.pack('<I', 16) + fmt +
            b'fact' + struct.pack('<I', 3) + b'xyz\0' + b'data' + struct.pack('<I', len(pcm) + 50) + pcm)
    q = tmp_path / 'b.wav'
    q.write_bytes(b'RIFF' + struct.pack('<I', len(body)) + body)
    a, r = read_wav_native(str(q))
    assert wav_info(str(q)) == (a.size, r) == (100, 8000)
