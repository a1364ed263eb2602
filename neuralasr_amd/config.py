"""Run configuration (reference: config.py:11-113): the same INI files (ExtendedInterpolation,
sections Parameters / Train / Test / MFCC Featurizer), the same derived fields
(feature_size = (2*numcontext+1)*numcep, batch_size multiplied by num_gpus) and the same dotted-name
network loader.  Two optional [Parameters] keys choose the features the GPU front end makes: features=mfcc|logfbank
(default mfcc) and deltas=0|1|2 (default 0); a frame is frame_width = numcep*(1+deltas) wide and feature_size is
(2*numcontext+1)*frame_width.  `network=networks.bilstm_ctc_net.BiLstmCTCNet` resolves to the HIP implementation in
neuralasr_amd.networks when the reference's TensorFlow package of that name is not importable.  Three more optional
[Parameters] keys fuse an n-gram model into the beam searches of evaluate / decode (lm.py): lm_file, lm_weight (default 0)
and lm_bonus (per emitted symbol, CTC only, default 0); without lm_file nothing changes, and training never reads them.
Seven more optional [Parameters] keys switch on the augmentation of `train --from-audio` (augment.py; the
reference has none but rand_shift): spec_time_masks / spec_freq_masks (masks per utterance, 0..8, default 0),
spec_time_width / spec_freq_width (largest width in frames / static columns, default 0), spec_time_ratio (largest time
mask as a share of the utterance, default 1.0), speed_perturb (comma-separated factors, each in (0.5, 2.0), default none)
and augment_seed (default 0); without them nothing changes.  One more optional [Parameters] key, max_grad_norm, switches
on global-norm gradient clipping with a non-finite guard in the optimiser step (the reference clips
nothing): absent or 0 = off, a positive number = tf.clip_by_global_norm's threshold, inf = measure and guard only; only
training reads it.  Two more optional [Parameters] keys choose how the GPU front end normalises (the
reference has only the whole-utterance rule of utils.py:29): normalization=utterance|causal (default utterance) and, with
causal only, norm_min_frames (the frames the running statistics wait for, 1..1000, default 50 = 0.5 s); training,
preprocessing and decoding all read them, so that a model is decoded with the normalisation it was trained with.  Five
more optional [Parameters] keys switch on the waveform augmentation of `train --from-audio` (augment.py; the
reference has none): noise_list / rir_list (a file that lists WAV paths, one per line: noise clips, room impulse
responses), noise_prob / rir_prob (the share of utterances that get one, in [0,1], default 1 when the list is given) and
noise_snr=lo,hi (dB, lo <= hi, default 10,20); without them nothing changes, and only the training feed reads them.  One
more optional [Parameters] key, stream_lookahead (frames, 0..1024, default 0 = off), is the look-ahead with which a
bidirectional network streams (HipNetwork.stream, decode_wav --stream; the reference decodes whole
utterances); unidirectional networks ignore it.  One more optional [Parameters] key, chunk_frames (frames, 0..4096, default
0 = off), trains and evaluates a bidirectional network as a look-ahead session runs it: windows of
chunk_frames + stream_lookahead rows, the forward state carried from window to window, the backward direction restarted
in each; it needs stream_lookahead >= 1, and train, validate, evaluate, decode and align all read it.  Three more optional
[Parameters] keys distil a teacher network into the one that is trained (the reference has nothing like
it): teacher_config (the teacher's config file: its network and model_dir are used, its data sections are not),
distill_weight (the share of the distillation term in the loss, in (0,1), default 0.5) and distill_temperature (in
[0.25,16], default 1.0); the last two need teacher_config, only training reads them, and without them nothing changes.  Five more optional
[Parameters] keys shape the optimiser (the reference trains at a fixed learningrate and keeps the last
iterate): ema_decay (in (0,1); default off) keeps tf.train.ExponentialMovingAverage's average of the parameters, which
validate / evaluate / decode / align then run on and which a network built for inference loads from the checkpoint;
lr_warmup_steps (>= 0, default 0), lr_decay_steps (>= 0, 0 = no decay), lr_decay_rate (in (0,1], default 1) and lr_staircase
(0 or 1) make the step size of global step s learningrate * min(1, s / warmup) * rate ** (max(0, s - warmup) / decay_steps);
without them nothing changes.  One more optional [Parameters] key, frame_skip (an integer in 1..8, default 1), gives the LSTM
CTC networks low-frame-rate input (the reference has no such key, the rule is this project's own): the
network sees every frame_skip-th stacked frame of an utterance; train, validate, evaluate, decode, align and stream all
read it, a checkpoint remembers it, and without the key nothing changes."""
import importlib
import math
from configparser import ConfigParser, ExtendedInterpolation

import numpy as np

from .logger import get_logger
from .symbols import Symbols

log = get_logger()

_INT_KEYS = ('samplerate', 'numcep', 'batch_size', 'epochs', 'start_step', 'report_step', 'num_gpus', 'label_context')


def network_class(name):
    """the class a config's `network=` names, not yet constructed"""
    parts = name.split('.')
    modname, classname = '.'.join(parts[:-1]), parts[-1]
    module = None
    for candidate in (modname, 'neuralasr_amd.' + modname):
        try:
            module = importlib.import_module(candidate)
            getattr(module, classname)
            break
        except (ImportError, AttributeError):
            module = None
    if module is None:
        raise ImportError('cannot load network class ' + name)
    return getattr(module, classname)


class Config(object):
    def __init__(self, configfile, isTraining=False):
        self.isTraining = isTraining
        self.configfile = configfile
        log.info('Reading configuration from: ' + configfile)
        self.cfg = ConfigParser(interpolation=ExtendedInterpolation())
        self.cfg.read(configfile)
        par = self.cfg['Parameters']
        for key in _INT_KEYS:
            setattr(self, key, int(par[key]))
        self.numcontext = int(par['numcontext']) if 'numcontext' in par else 0
        self.rand_shift = int(par['rand_shift']) if 'rand_shift' in par else 0
        self.learningrate = float(par['learningrate'])
        self.model_dir = par['model_dir']
        self.punc_regex = par['punc_regex']
        self.network = par['network']
        self.sym_file = par['sym_file'] if 'sym_file' in par else None
        self.features = par['features'].strip() if 'features' in par else 'mfcc'
        if self.features not in ('mfcc', 'logfbank'):
            raise ValueError("'features' must be mfcc or logfbank, not %r, in %s" % (self.features, configfile))
        deltas = par['deltas'].strip() if 'deltas' in par else '0'
        if deltas not in ('0', '1', '2'):
            raise ValueError("'deltas' must be 0, 1 or 2, not %r, in %s" % (deltas, configfile))
        self.deltas = int(deltas)
        self._read_normalization(par, configfile)
        # frames of look-ahead with which a bidirectional network streams (the reference decodes whole
        # utterances): 0 = off, unidirectional networks ignore it
        try:
            self.stream_lookahead = int(par['stream_lookahead'].strip()) if 'stream_lookahead' in par else 0
        except ValueError:
            self.stream_lookahead = -1
        if not 0 <= self.stream_lookahead <= 1024:
            raise ValueError("'stream_lookahead' must be an integer in [0,1024], not %r, in %s"
                             % (par['stream_lookahead'], configfile))
        # rows a window of latency-controlled training emits: 0 = off, the whole-utterance graph
        try:
            self.chunk_frames = int(par['chunk_frames'].strip()) if 'chunk_frames' in par else 0
        except ValueError:
            self.chunk_frames = -1
        if not 0 <= self.chunk_frames <= 4096:
            raise ValueError("'chunk_frames' must be an integer in [0,4096], not %r, in %s" % (par['chunk_frames'], configfile))
        if self.chunk_frames > 0 and self.stream_lookahead < 1:
            raise ValueError("'chunk_frames' needs 'stream_lookahead' >= 1 (the window is chunk_frames + stream_lookahead rows), in %s"
                             % configfile)
        # low-frame-rate input: the network sees input frames 0, frame_skip, 2*frame_skip, ... ; 1 = every frame
        try:
            self.frame_skip = int(par['frame_skip'].strip()) if 'frame_skip' in par else 1
        except ValueError:
            self.frame_skip = 0
        if not 1 <= self.frame_skip <= 8:
            raise ValueError("'frame_skip' must be an integer in [1,8], not %r, in %s" % (par['frame_skip'], configfile))
        self.frame_width = self.numcep * (1 + self.deltas)
        self.feature_size = (2 * self.numcontext + 1) * self.frame_width
        self.lm_file = par['lm_file'].strip() if 'lm_file' in par else None
        self.lm_weight = float(par['lm_weight']) if 'lm_weight' in par else 0.0
        self.lm_bonus = float(par['lm_bonus']) if 'lm_bonus' in par else 0.0
        self._read_augment(par, configfile)
        self.max_grad_norm = self._read_max_grad_norm(par, configfile)
        self._read_distill(par, configfile)
        self._read_optimiser(par, configfile)
        # the configured batch is per GPU (reference: config.py:35-36)
        self.batch_size *= self.num_gpus if self.num_gpus > 0 else 1
        self.symbols = Symbols(self.label_context, self.sym_file) if isTraining else Symbols(self.label_context)

        train, test, feat = self.cfg['Train'], self.cfg['Test'], self.cfg['MFCC Featurizer']
        self.train_input = train['input'] if 'input' in train else None
        self.mfcc_input = feat['input'] if 'input' in feat else None
        self.mfcc_output = feat['output'] if 'output' in feat else None
        self.start_marker = feat['start_marker'] if 'start_marker' in feat else None
        self.end_marker = feat['end_marker'] if 'end_marker' in feat else None
        self.test_input = test['input'] if 'input' in test else None
        if self.test_input is None and not self.train_input:
            raise ValueError("Missing 'test_input' in configuration file: " + configfile)

    def _read_normalization(self, par, configfile):
        """normalization and norm_min_frames (None under the whole-utterance rule, which has no such number)"""
        self.normalization = par['normalization'].strip() if 'normalization' in par else 'utterance'
        if self.normalization not in ('utterance', 'causal'):
            raise ValueError("'normalization' must be utterance or causal, not %r, in %s" % (self.normalization, configfile))
        self.norm_min_frames = None
        if 'norm_min_frames' in par:
            if self.normalization != 'causal':
                raise ValueError("'norm_min_frames' needs normalization=causal, in %s" % configfile)
            try:
                self.norm_min_frames = int(par['norm_min_frames'].strip())
            except ValueError:
                self.norm_min_frames = 0
            if not 1 <= self.norm_min_frames <= 1000:
                raise ValueError("'norm_min_frames' must be an integer in [1,1000], not %r, in %s"
                                 % (par['norm_min_frames'], configfile))
        elif self.normalization == 'causal':
            self.norm_min_frames = 50
        if self.normalization == 'causal' and self.deltas:
            raise ValueError("'normalization=causal' needs deltas=0 (the delta columns look ahead; DESIGN.md §16), in %s"
                             % configfile)

    @staticmethod
    def _number(par, configfile, key, kind, default, lo, hi, what, open_lo=False, open_hi=False):
        """an optional numeric key of [Parameters] in [lo,hi] (open_lo / open_hi: that end excluded), or its default"""
        if key not in par:
            return default
        try:
            v = kind(par[key].strip())
        except ValueError:
            v = None
        if v is None or not lo <= v <= hi or (open_lo and v == lo) or (open_hi and v == hi):
            raise ValueError("'%s' must be %s, not %r, in %s" % (key, what, par[key], configfile))
        return v

    def _read_optimiser(self, par, configfile):
        """ema_decay (0.0: no parameter averaging) and the learning-rate schedule's keys; all optional"""
        def number(*a, **k):
            return self._number(par, configfile, *a, **k)
        big = 1 << 62
        self.ema_decay = number('ema_decay', float, 0.0, 0.0, 1.0, 'a number in (0,1)', open_lo=True, open_hi=True)
        self.lr_warmup_steps = number('lr_warmup_steps', int, 0, 0, big, 'an integer >= 0')
        self.lr_decay_steps = number('lr_decay_steps', int, 0, 0, big, 'an integer >= 0')
        self.lr_decay_rate = number('lr_decay_rate', float, 1.0, 0.0, 1.0, 'a number in (0,1]', open_lo=True)
        self.lr_staircase = number('lr_staircase', int, 0, 0, 1, '0 or 1')
        # some schedule key is in the file: train logs an "LR:" line behind each "Step:" line
        self.lr_schedule_on = any(k in par for k in ('lr_warmup_steps', 'lr_decay_steps', 'lr_decay_rate', 'lr_staircase'))

    def learning_rate_at(self, step):
        """The step size of optimiser step `step` (the 1-based global_step about to be applied): tf.train.exponential_decay
        behind a linear warm-up, in float64, rounded to fp32.
          lr(s) = learningrate * min(1, s / warmup) * rate ** (max(0, s - warmup) / decay_steps)   (staircase: floored)"""
        lr = float(self.learningrate)
        if self.lr_warmup_steps > 0:
            lr *= min(1.0, step / float(self.lr_warmup_steps))
        if self.lr_decay_steps > 0:
            e = max(0, step - self.lr_warmup_steps) / float(self.lr_decay_steps)
            lr *= float(self.lr_decay_rate) ** (math.floor(e) if self.lr_staircase else e)
        return float(np.float32(lr))

    def _read_augment(self, par, configfile):
        def number(*a):
            return self._number(par, configfile, *a)
        big = 1 << 62
        self.spec_time_masks = number('spec_time_masks', int, 0, 0, 8, 'an integer in [0,8]')
        self.spec_time_width = number('spec_time_width', int, 0, 0, big, 'an integer >= 0')
        self.spec_time_ratio = number('spec_time_ratio', float, 1.0, 0.0, 1.0, 'a number in [0,1]')
        self.spec_freq_masks = number('spec_freq_masks', int, 0, 0, 8, 'an integer in [0,8]')
        self.spec_freq_width = number('spec_freq_width', int, 0, 0, big, 'an integer >= 0')
        self.augment_seed = number('augment_seed', int, 0, 0, (1 << 64) - 1, 'an integer in [0, 2^64)')
        self.speed_perturb = ()
        if 'speed_perturb' in par:
            try:
                self.speed_perturb = tuple(float(x) for x in par['speed_perturb'].split(','))
            except ValueError:
                self.speed_perturb = ()
            if not self.speed_perturb or not all(0.5 < f < 2.0 for f in self.speed_perturb):
                raise ValueError("'speed_perturb' must be comma-separated factors, each in (0.5, 2.0), not %r, in %s"
                                 % (par['speed_perturb'], configfile))
        # waveform augmentation: list files of WAV paths, one per line
        self.noise_list = par['noise_list'].strip() if 'noise_list' in par else None
        self.rir_list = par['rir_list'].strip() if 'rir_list' in par else None
        for key, lst in (('noise_list', self.noise_list), ('rir_list', self.rir_list)):
            if lst is not None and not lst:
                raise ValueError("'%s' must name a file that lists WAV paths, in %s" % (key, configfile))
        for key, lst in (('noise_prob', 'noise_list'), ('noise_snr', 'noise_list'), ('rir_prob', 'rir_list')):
            if key in par and getattr(self, lst) is None:
                raise ValueError("'%s' needs '%s', in %s" % (key, lst, configfile))
        self.noise_prob = number('noise_prob', float, 1.0 if self.noise_list else 0.0, 0.0, 1.0, 'a number in [0,1]')
        self.rir_prob = number('rir_prob', float, 1.0 if self.rir_list else 0.0, 0.0, 1.0, 'a number in [0,1]')
        self.noise_snr = (10.0, 20.0)
        if 'noise_snr' in par:
            try:
                snr = tuple(float(x) for x in par['noise_snr'].split(','))
            except ValueError:
                snr = ()
            if len(snr) != 2 or not all(math.isfinite(v) for v in snr) or not snr[0] <= snr[1]:
                raise ValueError("'noise_snr' must be lo,hi in dB with lo <= hi, not %r, in %s" % (par['noise_snr'], configfile))
            self.noise_snr = snr

    def _read_distill(self, par, configfile):
        """teacher_config (None: no distillation), distill_weight and distill_temperature"""
        self.teacher_config = par['teacher_config'].strip() if 'teacher_config' in par else None
        if self.teacher_config is not None and not self.teacher_config:
            raise ValueError("'teacher_config' must name the teacher's config file, in %s" % configfile)
        for key in ('distill_weight', 'distill_temperature'):
            if key in par and self.teacher_config is None:
                raise ValueError("'%s' needs 'teacher_config', in %s" % (key, configfile))

        def number(key, default, ok, what):
            if key not in par:
                return default
            try:
                v = float(par[key].strip())
            except ValueError:
                v = float('nan')
            if not ok(v):       # out of range, NaN, or not a number at all
                raise ValueError("'%s' must be %s, not %r, in %s" % (key, what, par[key], configfile))
            return v
        self.distill_weight = number('distill_weight', 0.5, lambda v: 0.0 < v < 1.0, 'a number in (0,1)')
        self.distill_temperature = number('distill_temperature', 1.0, lambda v: 0.25 <= v <= 16.0, 'a number in [0.25,16]')

    @staticmethod
    def _read_max_grad_norm(par, configfile):
        if 'max_grad_norm' not in par:
            return 0.0
        try:
            v = float(par['max_grad_norm'].strip())
        except ValueError:
            v = -1.0
        if not v >= 0.0:        # negative, NaN, or not a number at all
            raise ValueError("'max_grad_norm' must be 0 (off), a positive number or inf, not %r, in %s"
                             % (par['max_grad_norm'], configfile))
        return v

    @property
    def augment_on(self):
        """some augmentation key is switched on"""
        return self.spec_time_masks > 0 or self.spec_freq_masks > 0 or len(self.speed_perturb) > 0 or self.wave_on

    @property
    def wave_on(self):
        """the waveform augmentation (noise, reverberation) is switched on"""
        return (self.noise_list is not None and self.noise_prob > 0) or (self.rir_list is not None and self.rir_prob > 0)

    def load_network(self, fortraining=False):
        return network_class(self.network)(self, fortraining=fortraining)

    def print_config(self):
        names = ['samplerate', 'numcep', 'numcontext', 'features', 'deltas', 'normalization', 'norm_min_frames', 'stream_lookahead', 'chunk_frames', 'frame_skip', 'rand_shift', 'batch_size', 'epochs', 'learningrate',
                 'model_dir', 'start_step', 'report_step', 'num_gpus', 'label_context', 'punc_regex', 'network',
                 'sym_file', 'train_input', 'test_input', 'mfcc_input', 'mfcc_output', 'start_marker', 'end_marker']
        lines = ['']
        for n in names:
            v = getattr(self, n)
            lines.append(('%s=%f' % (n, v)) if n == 'learningrate' else '%s=%s' % (n, v))
        log.info('\n'.join(lines) + '\n')

    def write_symbols(self):
        self.symbols.write(self.sym_file)

    def write(self, filename):
        log.info('Writing configuration to: ' + filename)
        with open(filename, 'w') as fh:
            self.cfg.write(fh)
