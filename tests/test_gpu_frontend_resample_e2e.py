"""GPU: WAV files at other rates than the config's through the project alone, as the reference's librosa.load(wav,
mono=True, sr=sr) takes them.  int16 WAVs at 8, 16 (stereo) and 44.1 kHz and a CSV -> preprocess_mfcc for an 8 kHz
config -> pickles checked against the restated load() and MFCC; one training step -> checkpoint -> decode_wav of a
48 kHz file."""
import logging
import os
import struct

import numpy as np
import pytest

import mfcc_ref as R
import resample_ref as RR
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu

SR = 8000


def write_wav16(path, channels, rate):
    """channels float32 [c, n] -> an int16 PCM WAV at `rate`."""
    pcm = np.round(np.asarray(channels).T * 32768).astype('<i2').tobytes()
    c = len(channels)
    fmt = struct.pack('<HHIIHH', 1, c, rate, rate * 2 * c, 2 * c, 16)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', 16) + fmt + b'data' + struct.pack('<I', len(pcm)) + pcm
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def test_wavs_at_other_rates_to_features_to_decode(tmp_path, caplog):
    from neuralasr_amd import decode_wav, preprocess_mfcc
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    from neuralasr_amd.features import read_wav_native, resample_filter
    from neuralasr_amd.utils import featurizer
    table = resample_filter()
    specs = [('Hello world.', 8000, 1), ('A cat, a dog!', 16000, 2), ('speech to text', 44100, 1),
             ('one two three', 16000, 1), ('GPU front end', 44100, 2)]
    channels, rows = {}, []
    for i, (text, rate, c) in enumerate(specs):
        ch = np.stack([speech_like(int(rate * (0.8 + 0.3 * i)), rate, 300 + 10 * i + k) for k in range(c)])
        wav, txt = tmp_path / ('utt%d.wav' % i), tmp_path / ('utt%d.txt' % i)
        write_wav16(wav, ch, rate)
        txt.write_text(text + '\n')
        channels['utt%d' % i] = (ch, rate, str(wav))
        rows.append('%s,%s,%d' % (wav, txt, i))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'mfcc'
    cfg_path = tmp_path / 'rs.config'
    cfg_path.write_text(
        '[Parameters]\nsamplerate=%d\nnumcep=13\nnumcontext=0\nlabel_context=0\nbatch_size=2\nepochs=1\n'
        'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
        'sym_file=${MFCC Featurizer:output}/symbols\nnetwork=networks.bilstm_ctc_net.BiLstmCTCNet\n'
        '[Train]\ninput=${MFCC Featurizer:output}/train.scp\n[Test]\ninput=${MFCC Featurizer:output}/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\nstart_marker=^\nend_marker=$$\n'
        % (SR, tmp_path / 'model', tmp_path / 'data.csv', out))
    preprocess_mfcc.main([str(cfg_path)])
    train = (out / 'train.scp').read_text().split()
    test = (out / 'test.scp').read_text().split()
    assert train == ['utt0.pkl', 'utt1.pkl', 'utt2.pkl', 'utt3.pkl'] and test == ['utt4.pkl']

    config = Config(str(cfg_path), True)
    ds = DataSet(config.train_input, config)
    for name in train + test:
        ch, rate, wav = channels[name[:-4]]
        mfcc, _, _, _ = ds.load_pkl(str(out / name))
        y = RR.load(np.round(ch * 32768) / 32768, rate, SR, win=table)
        want, _ = R.features(y, SR, 0, 13)
        assert mfcc.shape == want.shape and np.abs(mfcc - want).max() <= 1e-4, name
        if rate == SR:
            audio, r = read_wav_native(wav)
            assert r == SR and mfcc.tobytes() == featurizer(SR, 0, 13).compute([audio])[0].tobytes()

    mfccs, labels, seq_len, labels_len = ds.get_next_batch()
    net = config.load_network(fortraining=True)
    loss, _ = net.train(mfccs, labels, seq_len, labels_len)
    assert np.isfinite(loss)
    net.save_checkpoint()

    a48 = speech_like(int(48000 * 1.7), 48000, 77)
    write_wav16(tmp_path / 'x48.wav', a48[None], 48000)
    with caplog.at_level(logging.INFO):
        decoded = decode_wav.main([str(cfg_path), str(tmp_path / 'x48.wav')])
    assert any(r.getMessage().startswith('Decoded: ') for r in caplog.records)
    feat = featurizer(SR, 0, 13).compute([read_wav_native(str(tmp_path / 'x48.wav'))[0]], rates=[48000])[0]
    assert feat.shape[0] == R.num_frames(RR.lengths(a48.size, 48000, SR)[0], SR)
    network = config.load_network(fortraining=False)
    want = config.symbols.convert_to_str(network.decode(feat[None], [np.asarray(feat.shape[0], dtype=np.int32)]))
    assert decoded == want
    assert os.path.exists(str(tmp_path / 'model'))
