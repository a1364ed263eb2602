#!/usr/bin/env python3
"""Wall time per step of the training loop from audio (python -m neuralasr_amd.train CONFIG --from-audio: WAV files ->
AudioDataSet -> features made on the GPU per batch) against the pickled loop (preprocess_mfcc -> DataSet) on the same
utterances: synthetic WAVs at 16 kHz, numcep 26, numcontext 10, the 3x500 bidirectional net, one GPU.

    python tools/e2e_audio.py [utterances=64] [epochs=4] [seconds=5] [batch=16] [augment=0]

augment=1: the loop from audio without and with the augmentation keys (2 time masks up to 40 frames, 2 frequency masks up
to 7 columns, speed_perturb=0.9,1.0,1.1) in the place of the pickled loop.  augment=2: without and with
the waveform keys (three noise clips at 0 to 20 dB and three 4000-tap RIRs, every utterance gets both).
Every leg also prints the persistent recurrence's (aborts, re-arms) of its handle (nasr_get_persist_stats)."""
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from mfccbench import synth                            # noqa: E402
from neuralasr_amd import preprocess_mfcc              # noqa: E402
from neuralasr_amd import train as train_mod          # noqa: E402
from neuralasr_amd.config import Config               # noqa: E402
from neuralasr_amd.dataset import DataSet              # noqa: E402
from neuralasr_amd.features import write_wav16        # noqa: E402

CONFIG = """[Parameters]
samplerate=16000
numcep=26
numcontext=10
label_context=0
batch_size=%(batch)d
epochs=%(epochs)d
learningrate=0.0001
model_dir=%(out)s/model
start_step=0
report_step=1000000
num_gpus=1
%(keys)spunc_regex=[^a-z0-9 ]
sym_file=${MFCC Featurizer:output}/symbols
network=networks.bilstm_ctc_net.BiLstm3x500CTCNet

[Train]
input=${MFCC Featurizer:output}/train.scp

[Test]

[MFCC Featurizer]
input=%(out)s/data.csv
output=%(out)s/mfcc
"""
KEYS = ('spec_time_masks=2\nspec_time_width=40\nspec_freq_masks=2\nspec_freq_width=7\nspeed_perturb=0.9,1.0,1.1\n'
        'augment_seed=1\n')


def main():
    n_utt = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    epochs = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    seconds = float(sys.argv[3]) if len(sys.argv) > 3 else 5.0
    batch = int(sys.argv[4]) if len(sys.argv) > 4 else 16
    augment = int(sys.argv[5]) if len(sys.argv) > 5 else 0
    out = tempfile.mkdtemp(prefix='nasr_e2e_audio_')
    try:
        rs = np.random.RandomState(7)
        rows = []
        n_all = int(np.ceil(n_utt / 0.8))                       # the first 80 % of the rows are the training set
        for i in range(n_all):
            wav, txt = os.path.join(out, 'u%d.wav' % i), os.path.join(out, 'u%d.txt' % i)
            write_wav16(wav, synth(int(seconds * 16000), 16000, i), 16000)
            with open(txt, 'w') as fh:
                fh.write(''.join(rs.choice(list('abcdefghijklmnopqrstuvwxyz '), size=rs.randint(40, 81))) + '\n')
            rows.append('%s,%s,%d' % (wav, txt, os.path.getsize(wav)))
        with open(os.path.join(out, 'data.csv'), 'w') as fh:
            fh.write('\n'.join(rows) + '\n')
        cfgp, cfga = os.path.join(out, 'e2e.config'), os.path.join(out, 'e2e_aug.config')
        with open(cfgp, 'w') as fh:
            fh.write(CONFIG % dict(out=out, epochs=epochs, batch=batch, keys=''))
        with open(cfga, 'w') as fh:
            fh.write(CONFIG % dict(out=out, epochs=epochs, batch=batch, keys=KEYS))
        preprocess_mfcc.main([cfgp])
        legs = (('pickled features (DataSet)', False), ('from audio (AudioDataSet)', True),
                ('pickled features, again', False), ('from audio, again', True))
        if augment == 2:
            from neuralasr_amd.augment import prepare_rir
            for kind in ('noise', 'rir'):
                names = []
                for i in range(3):
                    a = 0.1 * rs.randn(3 * 16000 + 1000 * i)
                    if kind == 'rir':
                        a = 0.9 * prepare_rir(rs.randn(4000) * np.exp(-np.arange(4000) / 800.0))
                    names.append(os.path.join(out, '%s%d.wav' % (kind, i)))
                    write_wav16(names[-1], a, 16000)
                with open(os.path.join(out, kind + '.lst'), 'w') as fh:
                    fh.write('\n'.join(names) + '\n')
            with open(cfga, 'w') as fh:
                keys = 'noise_list=%s/noise.lst\nnoise_snr=0,20\nrir_list=%s/rir.lst\naugment_seed=1\n' % (out, out)
                fh.write(CONFIG % dict(out=out, epochs=epochs, batch=batch, keys=keys))
        if augment:
            legs = (('from audio (AudioDataSet)', True), ('from audio, augmented', cfga),
                    ('from audio, again', True), ('from audio, augmented, again', cfga))
        for label, audio in legs:
            path = audio if isinstance(audio, str) else cfgp
            cfg = Config(path, True)
            data = train_mod.audio_datasets(path, cfg)[0] if audio else DataSet(cfg.train_input, cfg)
            steps_per_epoch = (data.get_num_of_sample() + batch - 1) // batch
            stamps = []
            orig = cfg.load_network.__func__

            def load(self, fortraining=False, _orig=orig, _stamps=stamps):
                net = _orig(self, fortraining)
                inner = net.finish_step

                def timed(*a, **kw):
                    r = inner(*a, **kw)
                    _stamps.append(time.perf_counter())
                    return r
                net.finish_step = timed
                return net
            cfg.load_network = load.__get__(cfg)
            net = train_mod.train_model(data, None, cfg)
            persist = net.engine.persist_stats()
            net.engine.close()
            gaps = np.diff(np.asarray(stamps)) * 1e3
            print('%-34s median %.3f ms, mean %.3f ms per step over %d steps after the first epoch (%d x %.1f s per batch); '
                  'persistent recurrence (aborts, re-arms) %r'
                  % (label, float(np.median(gaps[steps_per_epoch:])), float(gaps[steps_per_epoch:].mean()),
                     len(gaps) - steps_per_epoch, batch, seconds, persist), flush=True)
    finally:
        shutil.rmtree(out, ignore_errors=True)


if __name__ == '__main__':
    main()
