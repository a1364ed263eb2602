"""GPU: audio to text through the project alone.  WAV files, transcripts and a CSV -> preprocess_mfcc -> DataSet ->
one BiLstmCTCNet training step -> checkpoint -> decode_wav."""
import logging
import os
import struct

import numpy as np
import pytest

import mfcc_ref as R
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu

SR = 8000


def write_wav16(path, audio):
    pcm = np.round(audio * 32768).astype('<i2').tobytes()
    fmt = struct.pack('<HHIIHH', 1, 1, SR, SR * 2, 2, 16)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', 16) + fmt + b'data' + struct.pack('<I', len(pcm)) + pcm
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def test_wav_to_training_step_to_decode(tmp_path, caplog):
    from neuralasr_amd import decode_wav, preprocess_mfcc
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    texts = ['Hello world.', 'A cat, a dog!', 'speech to text', 'one two three', 'GPU front end']
    audios = {}
    rows = []
    for i, text in enumerate(texts):
        a = speech_like(int(SR * (0.8 + 0.3 * i)), SR, 100 + i)
        wav, txt = tmp_path / ('utt%d.wav' % i), tmp_path / ('utt%d.txt' % i)
        write_wav16(wav, a)
        txt.write_text(text + '\n')
        audios['utt%d' % i] = a
        rows.append('%s,%s,%d' % (wav, txt, os.path.getsize(wav)))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'mfcc'
    cfg_path = tmp_path / 'e2e.config'
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
    for name in train:
        mfcc, labels, T, L = ds.load_pkl(str(out / name))
        want, _ = R.features(audios[name[:-4]], SR, 0, 13)
        assert mfcc.shape == want.shape and np.abs(mfcc - want).max() <= 1e-4
        assert labels[0] == config.symbols.get_id('^') and labels[-1] == config.symbols.get_id('$')
    mfccs, labels, seq_len, labels_len = ds.get_next_batch()
    assert mfccs.shape[0] == 2 and mfccs.shape[2] == 13

    net = config.load_network(fortraining=True)
    loss, _ = net.train(mfccs, labels, seq_len, labels_len)
    assert np.isfinite(loss)
    net.save_checkpoint()

    with caplog.at_level(logging.INFO):
        decoded = decode_wav.main([str(cfg_path), str(tmp_path / 'utt4.wav')])
    assert isinstance(decoded, str)
    assert any(r.getMessage().startswith('Decoded: ') for r in caplog.records)
