"""GPU: LAS from audio to text through the project alone.  WAV files, transcripts and a CSV -> preprocess_mfcc (start and
end markers) -> one LAS training step -> checkpoint -> decode_wav and decode over the test list, both through the
beam-search decoder at the reference's width."""
import logging
import os

import numpy as np
import pytest

from test_gpu_frontend_e2e import SR, write_wav16
from test_gpu_mfcc import speech_like

pytestmark = pytest.mark.gpu


def test_wav_to_las_step_to_decode(tmp_path, caplog):
    from neuralasr_amd import decode, decode_wav, preprocess_mfcc
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    texts = ['Hello world.', 'A cat, a dog!', 'speech to text', 'one two three', 'GPU front end']
    rows = []
    for i, text in enumerate(texts):
        a = speech_like(int(SR * (0.8 + 0.3 * i)), SR, 200 + i)
        wav, txt = tmp_path / ('utt%d.wav' % i), tmp_path / ('utt%d.txt' % i)
        write_wav16(wav, a)
        txt.write_text(text + '\n')
        rows.append('%s,%s,%d' % (wav, txt, os.path.getsize(wav)))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    out = tmp_path / 'mfcc'
    cfg_path = tmp_path / 'las.config'
    cfg_path.write_text(
        '[Parameters]\nsamplerate=%d\nnumcep=13\nnumcontext=0\nlabel_context=0\nbatch_size=2\nepochs=1\n'
        'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
        'sym_file=${MFCC Featurizer:output}/symbols\nnetwork=networks.las.LAS\n'
        '[Train]\ninput=${MFCC Featurizer:output}/train.scp\n[Test]\ninput=${MFCC Featurizer:output}/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\nstart_marker=^\nend_marker=$$\n'
        % (SR, tmp_path / 'model', tmp_path / 'data.csv', out))
    preprocess_mfcc.main([str(cfg_path)])

    config = Config(str(cfg_path), True)
    ds = DataSet(config.train_input, config)
    mfccs, labels, seq_len, labels_len = ds.get_next_batch()
    net = config.load_network(fortraining=True)
    assert net.beam_width == 1000 and net.max_decode_steps == 100 and net.length_penalty_weight == 0.5
    loss, _ = net.train(mfccs, labels, seq_len, labels_len)
    assert np.isfinite(loss)
    net.save_checkpoint()

    with caplog.at_level(logging.INFO):
        decoded = decode_wav.main([str(cfg_path), str(tmp_path / 'utt4.wav')])
        assert isinstance(decoded, str)
        decode.main([str(cfg_path)])
    msgs = [r.getMessage() for r in caplog.records]
    assert any(m.startswith('Decoded: ') for m in msgs)
    done = [m for m in msgs if 'avg_ler' in m]
    assert len(done) == 1
    print(done[0])
