"""HipNetwork — the counterpart of TensorFlowNetwork (reference: networks/tfnetwork.py:13-190): numpy-in /
numpy-out train / validate / evaluate / decode, checkpoints, and data-parallel training, with every
arithmetic step in the HIP library behind include/nasr.h (no TensorFlow, no CPU fallback).

Differences from the reference that a caller can observe, all deliberate and documented in DESIGN.md:
  * train() / validate() / evaluate() / decode() all use the reference's decoder (ctc_beam_search_decoder, width 100,
    merge_repeated, host C++).  The `mean_ler` of a training step is decoded from the step's own logits, copied out
    behind the CTC kernels, while the device runs the backward pass; train_model does not even wait for it - it
    collects the steps' LERs when it logs (`train_ler_decoder = 'greedy'` switches to the greedy decoder the
    reference names in the comment at tfnetwork.py:62-63: no host work at all);
  * num_gpus > 1 means one process per GPU (torch.distributed.run); inside a single process the towers are
    time-sliced on one GPU with the same split / averaging arithmetic;
  * checkpoints are `model-<step>.npz` (flat fp32 params + Adam m, v + step; with ema_decay in the config also the
    averaged parameters) with TF Saver's cadence and keep-5 policy, not TF's format."""
import contextlib
import glob
import json
import os
import shutil
import threading
import weakref

import numpy as np

from ..engine import Engine
from ..features import AudioBatch
from ..parallel import Collective, shard_bounds
from ..parallel import take_shard as _take_feature_shard
from ..utils import normalization_of
from .network import Network


def _glorot_init(tensors, seed):
    """Default TF initialisers the reference relies on: glorot-uniform LSTM kernels, zero biases,
    xavier-normal W (networks/bilstm_ctc_net.py:35-36), zero b.  TF's own seeded stream
    (tf.set_random_seed(1), tfnetwork.py:19) is not reproducible outside TF."""
    rs = np.random.RandomState(seed)
    chunks = []
    for name, _, rows, cols in tensors:
        if name.endswith('kernel'):
            lim = np.sqrt(6.0 / (rows + cols))
            chunks.append(rs.uniform(-lim, lim, size=rows * cols))
        elif name == 'W':
            chunks.append(rs.randn(rows * cols) * np.sqrt(2.0 / (rows + cols)))
        else:
            chunks.append(np.zeros(rows * cols))
    return np.concatenate(chunks).astype(np.float32)


def take_shard(mfccs, labels, seq_len, labels_len, world, rank):
    """parallel.take_shard; a batch given as audio (features.AudioBatch) is split by utterance"""
    if not isinstance(mfccs, AudioBatch):
        return _take_feature_shard(mfccs, labels, seq_len, labels_len, world, rank)
    if world == 1:
        return mfccs, np.asarray(labels), list(seq_len), list(labels_len) if labels_len is not None else None
    lo, hi = shard_bounds(len(seq_len), world, rank)
    labels = np.asarray(labels)
    return (mfccs.shard(lo, hi), labels[lo:hi] if labels.ndim else labels, list(seq_len[lo:hi]),
            list(labels_len[lo:hi]) if labels_len is not None else None)


class HipNetwork(Network):
    # model shape; subclasses override (the reference hard-codes these as locals of create_network)
    num_hidden = 500
    num_layers = 1
    bidirectional = True
    merge = 'stack_reshape'
    keep_checkpoints = 5                     # tf.train.Saver() default max_to_keep
    decoder = 'beam'                         # validate / evaluate / decode: tf.nn.ctc_beam_search_decoder defaults
    train_ler_decoder = 'beam'               # mean_ler of train(): the reference's decoder on the step's own logits ('greedy': on the device)
    beam_width = 100
    device_context = True                    # rebuild include_context's stacking on the GPU (1/(2c+1) of the H2D bytes)
    bucketed_allreduce = True                # one process per GPU: exchange per-layer gradient buckets under the backward pass
    # train() returns as soon as the step's loss and decode exist (after the forward pass + CTC), while the device runs the
    # backward pass, the exchange and Adam: the next step is enqueued behind it and the device never waits for the host.
    # A void step (rare: a persistent-recurrence abort on some rank) is noticed one call later and repeated then.
    # False: train() additionally waits for the END of its step (and repeats it there if it was void) - same code path.
    async_step = True
    takes_audio = True                       # train_audio / validate_audio / evaluate_audio / decode_audio work on this network

    def __init__(self, config, fortraining=False):
        Network.__init__(self)
        self.fortraining = fortraining
        self.config = config
        self.num_classes = config.symbols.counter
        self.coll = Collective()
        device = int(os.environ.get('LOCAL_RANK', '0')) if self.coll.world > 1 else 0
        # (a teacher network, DESIGN.md §22, is given the stream of the network it teaches)
        stream = getattr(config, 'engine_stream', None)
        if stream is None and self.coll.world > 1:
            # a dedicated non-default torch stream, made current: the engine launches on it and the RCCL
            # all-reduce is ordered against it (the legacy default stream is neither capturable nor shared)
            import torch
            torch.cuda.set_device(device)
            self._torch_stream = torch.cuda.Stream(device=device)
            torch.cuda.set_stream(self._torch_stream)
            stream = self._torch_stream.cuda_stream
        elif stream is None and fortraining and getattr(config, 'teacher_config', None):
            # student and teacher share one stream (_load_teacher says why): one that has a name outside the library
            import torch
            self._torch_stream = torch.cuda.Stream(device=device)
            stream = self._torch_stream.cuda_stream
        self._stream = stream
        self.logger.info('Initializing network for %s.' % ('training' if fortraining else 'inference'))
        self._device = device
        self._featurizer = None                 # the front end of the *_audio calls, made at the first of them
        self.engine = self.make_engine(config, device, stream)
        if getattr(config, 'frame_skip', 1) != 1:
            # frame_skip: every upload and every stream feed of this network from here on; a network that
            # cannot (WaveNet, LAS: the library says why) fails here, on every rank alike
            self.engine.set_frame_skip(config.frame_skip)
        if fortraining and getattr(config, 'max_grad_norm', 0.0) > 0:
            self.engine.set_grad_clip(config.max_grad_norm)     # every apply_adam of every step path clips from here on
        if getattr(config, 'chunk_frames', 0) > 0:
            # chunk_frames: train, validate, evaluate, decode and align all run the graph a look-ahead session
            # serves; a network that cannot (the library says why) fails here, on every rank alike
            self.engine.set_chunking(config.chunk_frames, config.stream_lookahead)
        self.engine.set_step_decode(True)
        self.engine.set_params(self.initial_params(self.engine.tensors(), seed=1))
        # ema_decay: a training network keeps the average beside the parameters and validates, evaluates,
        # decodes and aligns on it; one built for inference loads the checkpoint's average as its parameters instead
        self._ema = fortraining and getattr(config, 'ema_decay', 0.0) > 0
        if self._ema:
            self.engine.set_ema(config.ema_decay)               # the average starts at the initial parameters
        self._grad_tensor = None
        self._reducer = None
        self._staged = {}                       # id(mfccs) -> (ticket, weakref to mfccs): batches stage_batch() sent ahead
        self._staged_lock = threading.Lock()
        self._banks_lock = threading.Lock()     # the featurizer's noise and RIR banks are set once (_wave)
        self._banks_set = False
        self._pending = None                    # the batch of the last fast-path step, until that step is known not to be void
        self._begun = None                      # begin_step() without its finish_step() yet
        self._pool = None                       # host threads that decode the steps' logits (train_ler_decoder = 'beam')
        self._lm = None                         # config.lm_file's model, loaded at the first evaluate / decode
        self.global_step = self.config.start_step
        self.load_checkpoint(self.global_step if fortraining else 1, self.config.model_dir)
        self._teacher = None                    # config.teacher_config's network: every training batch goes to it too
        if fortraining and getattr(config, 'teacher_config', None):
            self.engine.set_distill(config.distill_weight, config.distill_temperature)     # (the library refuses a student that cannot)
            self._teacher = self._load_teacher()
        if fortraining and self.coll.rank == 0:
            self.write_config()
            self.config.symbols.write(os.path.join(self.config.model_dir, os.path.basename(self.config.sym_file)))

    # ------------------------------------------------------------------ distillation
    TEACHER_MUST_MATCH = ('feature_size', 'samplerate', 'numcep', 'numcontext', 'features', 'deltas', 'normalization', 'frame_skip')

    def _load_teacher(self):
        """config.teacher_config's network, built for inference on this network's device from its latest checkpoint (none is
        an error: a random teacher is a mistake).  It must read what the student reads and write what the student writes:
        the same features and the same symbol table."""
        from ..config import Config, network_class
        from ..engine import LasEngine
        cfg = self.config
        tcfg = Config(cfg.teacher_config, isTraining=True)      # (isTraining: the symbol table is read from its sym_file)
        if tcfg.symbols.sym_to_id != cfg.symbols.sym_to_id:
            raise ValueError("teacher_config %s: 'symbols' differ from the student's: the teacher's posteriors are over another "
                             'table (%d symbols, the student has %d)' % (cfg.teacher_config, tcfg.symbols.counter, cfg.symbols.counter))
        for key in self.TEACHER_MUST_MATCH:
            if getattr(tcfg, key, 1) != getattr(cfg, key, 1):   # (the default only ever stands in for frame_skip)
                raise ValueError("teacher_config %s: '%s' is %r, the student's is %r: both must see the same features"
                                 % (cfg.teacher_config, key, getattr(tcfg, key, None), getattr(cfg, key, None)))
        # On the student's stream: the teacher's forward pass then runs between two of the student's steps, never beside
        # one.  On a stream of its own it would meet the step before, which train() leaves running on the device, and two
        # persistent recurrences that each want every compute unit can take each other's places: one that gives up is a
        # void step, and the per-step kernels for the next 200.
        tcfg.engine_stream = self._stream
        teacher = network_class(tcfg.network)(tcfg, fortraining=False)     # (inference: restores the latest checkpoint)
        why = None
        if isinstance(teacher.engine, LasEngine):
            why = 'a LAS network has no CTC posteriors to distil'
        elif teacher.engine.logit_frames(1) != 1:
            why = 'a stack_reshape network has no logit frames to compare'
        if why:
            teacher.engine.close()
            raise ValueError("teacher_config %s: 'network' %s cannot teach: %s" % (cfg.teacher_config, tcfg.network, why))
        teacher.featurizer = self.featurizer                    # one front end: the same audio gives both the same features
        return teacher

    def _feed_teacher(self, f, s):
        """The shard that has just become the student's resident batch, by the same route to the teacher (uploaded the
        synchronous way, also where the student committed a staged batch): the same features, or the same audio with the
        same augmentation draws; then the teacher's forward pass, and its logits device to device."""
        t = self._teacher
        if t is None:
            return

        def run():
            if isinstance(f, AudioBatch):
                t._upload_audio(f, None, None, f.aug(self.config.numcep), self._wave(f))
            else:
                t._upload(f, None, s, None)
            t.engine.forward_resident(len(s), np.shape(f)[1], fetch=False)
        self._retry_aborted(run)
        self.engine.take_teacher_logits(t.engine)

    # the two hooks a model family overrides (DeepSpeech does): how the engine is shaped, how variables start
    def make_engine(self, config, device, stream):
        return Engine(config.feature_size, self.num_hidden, self.num_layers, self.bidirectional, self.merge,
                      self.num_classes, learning_rate=config.learningrate, device_id=device, stream=stream)

    def initial_params(self, tensors, seed):
        return _glorot_init(tensors, seed)

    # model families with state beyond the trainable variables (WaveNet's batch norm) override these three
    def model_state(self):
        """Extra arrays a checkpoint carries (name -> array); none for the LSTM families."""
        return {}

    def restore_model_state(self, npz):
        pass

    def after_compute_grads(self):
        """Called on every rank of a multi-process step right after compute_grads has been enqueued."""
        pass

    # ------------------------------------------------------------------ per-model hook
    def create_network(self, features, labels, seq_len, labels_len, num_classes, is_training):
        """(logits [T',B,C], loss, decoded ids per utterance, None, mean LER) for a batch
        (reference: networks/bilstm_ctc_net.py:10-52 returns the same five graph nodes)."""
        logits = self.engine.forward(features, seq_len)
        loss, _ = self.engine.loss(features, seq_len, labels, labels_len)
        hyps = self.engine.get_decoded(len(seq_len), np.asarray(features).shape[1])
        ler = self.engine.label_error_rate(hyps, labels, labels_len)
        return logits, loss, hyps, None, ler

    # ------------------------------------------------------------------ checkpoints
    def _ckpt_files(self, model_dir):
        files = glob.glob(os.path.join(model_dir, 'model-*.npz'))
        return sorted(files, key=lambda f: int(os.path.basename(f)[6:-4]))

    def load_checkpoint(self, start_epoch, model_dir):
        if start_epoch > 0:
            self.logger.info('Restoring checkpoint: ' + model_dir)
            files = self._ckpt_files(model_dir)
            if not files:
                raise FileNotFoundError('no checkpoint (model-<step>.npz) in ' + model_dir)
            with np.load(files[-1]) as z:
                # frame_skip changes no tensor's shape: only this field tells a model trained on every
                # third frame from one trained on every frame.  A checkpoint without the field was trained on every frame.
                saved = int(json.loads(str(z['meta'])).get('frame_skip', 1)) if 'meta' in z else 1
                mine = int(getattr(self.config, 'frame_skip', 1))
                if saved != mine:
                    raise ValueError("checkpoint %s was trained with frame_skip = %d, the config says frame_skip = %d: the "
                                     "network would see other frames than it was trained on" % (files[-1], saved, mine))
                params = z['params']
                if not self.fortraining and getattr(self.config, 'ema_decay', 0.0) > 0:
                    if 'ema' in z:
                        params = z['ema']                       # the averaged model is the one that is decoded
                    else:
                        self.logger.warning("'ema_decay' is set but the checkpoint holds no average: using its parameters")
                self.engine.set_params(params)
                self.engine.set_adam_state(z['adam_m'], z['adam_v'], int(z['step']))
                if self._ema and 'ema' in z:
                    self.engine.set_ema_state(z['ema'], int(z['ema_updates']))
                elif self._ema:
                    self.logger.info('The checkpoint holds no average: it starts at the restored parameters.')
                    self.engine.set_ema_state(z['params'], 0)
                self.restore_model_state(z)
            if self.fortraining and getattr(self.config, 'lr_schedule_on', False):
                # the schedule is a function of the global step: the checkpoint's, whatever start_step says
                self.global_step = int(os.path.basename(files[-1])[6:-4])
            self.logger.info('Done Restoring checkpoint: ' + files[-1])
        elif self.coll.rank == 0:
            if os.path.exists(model_dir):
                shutil.rmtree(model_dir)
            os.makedirs(model_dir)

    def write_config(self):
        dst = os.path.join(self.config.model_dir, os.path.basename(self.config.configfile))
        if os.path.exists(dst):
            self.logger.warning('Not overwriting. Config file already exists: ' + dst)
        else:
            self.config.write(dst)

    def save_checkpoint(self):
        self._settle()
        if self.coll.rank != 0:
            return
        m, v, step = self.engine.get_adam_state()
        path = os.path.join(self.config.model_dir, 'model-%d.npz' % self.global_step)
        ema = {}
        if self._ema:
            decay, updates, _ = self.engine.ema()
            ema = {'ema': self.engine.get_ema(), 'ema_updates': np.int64(updates), 'ema_decay': np.float32(decay)}
        np.savez(path, params=self.engine.get_params(), adam_m=m, adam_v=v, step=np.int64(step),
                 meta=json.dumps({'hidden': self.num_hidden, 'layers': self.num_layers,
                                  'bidirectional': self.bidirectional, 'merge': self.merge,
                                  'classes': self.num_classes, 'feature_size': self.config.feature_size,
                                  'frame_skip': int(getattr(self.config, 'frame_skip', 1))}),
                 **ema, **self.model_state())
        for old in self._ckpt_files(self.config.model_dir)[:-self.keep_checkpoints]:
            os.remove(old)

    # ------------------------------------------------------------------ numpy-in / numpy-out API
    def _towers(self):
        """(n, owned tower indices): one tower per process under torch.distributed, otherwise all
        num_gpus towers time-sliced in this process."""
        n = max(1, int(self.config.num_gpus)) if self.fortraining else 1
        if self.coll.world > 1:
            if n != self.coll.world:
                raise ValueError('config num_gpus=%d but %d processes were launched' % (n, self.coll.world))
            return n, [self.coll.rank]
        return n, list(range(n))

    @staticmethod
    def _is_abort(exc):
        return 'persistent recurrence aborted' in str(exc) or 'training step is void' in str(exc)

    def _retry_aborted(self, fn):
        """Run fn(); if this rank's persistent recurrence gave up in it (the handle has then switched to the per-step
        kernels, nasr_rec.hip rec_check), run it once more.  Forward-only calls have no collective inside, so a
        local repeat keeps multi-rank runs in step."""
        from .._lib import NasrError
        try:
            return fn()
        except NasrError as exc:
            if not self._is_abort(exc):
                raise
            self.logger.warning('persistent recurrence aborted in a forward-only call: repeating it on the per-step kernels')
            return fn()

    def _frame_width(self):
        """the width of one un-stacked frame of the pickled features: numcep*(1+deltas); 0 without a numcep"""
        numcep = getattr(self.config, 'numcep', 0)
        return getattr(self.config, 'frame_width', numcep)

    # ------------------------------------------------------------------ batches given as audio
    def featurizer(self):
        """The feature front end of the *_audio calls: on this network's device, shaped by the config."""
        if self._featurizer is None:
            from ..features import Featurizer
            self._featurizer = Featurizer(self.config.samplerate, self.config.numcep, self.config.numcontext,
                                          device_id=self._device, kind=getattr(self.config, 'features', 'mfcc'),
                                          deltas=getattr(self.config, 'deltas', 0), **normalization_of(self.config))
        return self._featurizer

    def audio_batch(self, audios, rates=None):
        """The batch `audios` (float32 utterances at `rates` Hz, None: all at config.samplerate) as train / validate /
        evaluate / decode / stage_batch take it in the place of the padded features; its .seq_len is their seq_len."""
        n, _ = self._towers()
        if n > 1 and self.merge == 'stack_reshape' and self.bidirectional:
            raise ValueError('batches from audio are padded per tower; the stack_reshape merge is a function of the padded '
                             'length of the WHOLE batch: use features with num_gpus > 1 on this network')
        return AudioBatch(self.config.samplerate, audios, rates, self.config.feature_size)

    def _wave(self, b):
        """The waveform augmentation that a TRAINING batch carries (engine.WaveAug), or None; the
        featurizer gets the banks of config.noise_list / config.rir_list before the first such batch."""
        wave = b.wave()
        if wave is not None:
            with self._banks_lock:
                if not self._banks_set:
                    from ..augment import load_banks
                    fz = self.featurizer()
                    noise, rirs = load_banks(self.config, fz)
                    fz.set_noise(noise)
                    fz.set_rirs(rirs)
                    self._banks_set = True
        return wave

    def _upload_audio(self, b, labels=None, labels_len=None, aug=None, wave=None):
        self.engine.upload_batch_audio(self.featurizer(), b.audios, labels, labels_len, b.rates, aug, wave)

    def _upload(self, f, l, s, ll, training=True):
        """One tower's shard made the resident batch, the synchronous way; the only place that knows the kinds of batch.
        Audio goes through the GPU front end, features cross as they are.  training: a training step's upload - audio with
        the batch's SpecAugment masks and waveform augmentation when it carries any, features as their centre slice where _context() allows it
        (inference uploads the whole stacked array, as engine.forward / loss / greedy_decode / align do)."""
        ctx = self._context() if training else 0
        if isinstance(f, AudioBatch):
            self._upload_audio(f, l, ll, f.aug(self.config.numcep) if training else None, self._wave(f) if training else None)
        elif not (ctx and self.engine.upload_batch_context(f, s, l, ll, ctx, self._frame_width())):
            self.engine.upload_batch(f, s, l, ll)

    def _forward(self, mfccs, seq_len):
        self._upload(mfccs, None, seq_len, None, training=False)
        return self.engine.forward_resident(len(seq_len), np.shape(mfccs)[1])

    def language_model(self):
        """The n-gram model of config.lm_file (lm.py), or None without the key: evaluate() and decode() fuse it into
        their beam search with config.lm_weight and config.lm_bonus; train() and validate() never do."""
        if self._lm is None and getattr(self.config, 'lm_file', None):
            from ..lm import load_for
            self._lm = load_for(self.config)
        return self._lm

    def _logit_lens(self, seq_len):
        """the lengths that go with the logits: seq_len itself, or under frame_skip the network's frames"""
        if getattr(self.config, 'frame_skip', 1) == 1:
            return seq_len
        return self.engine.logit_lens(seq_len)

    def _decode(self, mfccs, seq_len, which, lm=None):
        if which == 'beam':
            logits = self._retry_aborted(lambda: self._forward(mfccs, seq_len))
            if lm is None:
                return self.engine.beam_search(logits, self._logit_lens(seq_len), self.beam_width, merge_repeated=True)[0]
            return self.engine.beam_search(logits, self._logit_lens(seq_len), self.beam_width, merge_repeated=True, lm=lm,
                                           lm_weight=self.config.lm_weight, lm_bonus=self.config.lm_bonus)[0]

        def run():
            self._upload(mfccs, None, seq_len, None, training=False)
            return self.engine.greedy_decode_resident(len(seq_len), np.shape(mfccs)[1])
        return self._retry_aborted(run)

    def _loss_ler_one(self, mfccs, labels, seq_len, labels_len, lm=None):
        def run():
            self._upload(mfccs, labels, seq_len, labels_len, training=False)
            loss, _ = self.engine.loss_resident(len(seq_len))
            hyps = None if self.decoder == 'beam' else self.engine.get_decoded(len(seq_len), np.shape(mfccs)[1])
            return loss, hyps
        loss, hyps = self._retry_aborted(run)
        if hyps is None:
            hyps = self._decode(mfccs, seq_len, 'beam', lm)
        return loss, self.engine.label_error_rate(hyps, labels, labels_len), hyps

    def _loss_ler(self, mfccs, labels, seq_len, labels_len, lm=None):
        """(loss, mean LER, hypotheses).  A training network evaluates the way its graph was built
        (setup_training_network, tfnetwork.py:115-140): per tower on the tf.split shards - the literal net's
        stack-reshape map is a function of the SHARD's batch size - and the mean of the shard means."""
        n, mine = self._towers()
        if n == 1:
            return self._loss_ler_one(mfccs, labels, seq_len, labels_len, lm)
        losses, lers, hyps = [], [], []
        for k in mine:
            f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, n, k)
            lo, le, hy = self._loss_ler_one(f, l, s, ll, lm)
            losses.append(lo)
            lers.append(le)
            hyps.extend(hy)
        loss, ler = float(np.mean(losses)), float(np.mean(lers))
        if self.coll.world > 1:
            loss, ler = self.coll.mean_scalars([loss, ler])
        return loss, ler, hyps

    def train(self, mfccs, labels, seq_len, labels_len):
        self.begin_step(mfccs, labels, seq_len, labels_len)
        return self.finish_step()

    def begin_step(self, mfccs, labels, seq_len, labels_len):
        """First half of train(): everything of the optimisation step is ENQUEUED (upload or commit of the staged batch,
        forward, CTC, backward, gradient exchange, Adam) and the call returns.  The host is free until finish_step() -
        train_model loads and stages the next batch there, under the step the device is running (the reference loads the
        next batch inside the timed step with the device idle, train.py:23-26)."""
        self.global_step += 1
        n, mine = self._towers()
        if len(mine) == 1:
            f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, n, mine[0])
            batch = (mfccs, f, l, s, ll, n)
            self._begun = ('one', (batch, self._enqueue_step(*batch)))
        else:
            self._begun = ('sliced', (mfccs, labels, seq_len, labels_len))

    def finish_step(self, lazy=False):
        """Second half of train(): (loss, mean_ler) of the step begun last - available after its forward pass + CTC; the
        device may still be in its backward pass when this returns (async_step = False: it has ended, and was repeated if it
        was void).  lazy=True: mean_ler may come back as a handle with a .result() (the beam search of the step's logits
        still runs on host threads) - for a caller like train_model, which only needs the LERs when it logs; multi-process
        runs average such a window with mean_over_ranks()."""
        kind, batch = self._begun
        self._begun = None
        if kind == 'sliced':
            return self._train_sliced(*batch)
        out = self._finish_async(*batch, lazy=lazy)
        if not self.async_step:
            self._settle()
        return out

    def mean_over_ranks(self, value):
        """Mean of a host float over the towers' processes (reduce_mean of tfnetwork.py:135-136); the value itself with one."""
        return self.coll.mean_scalars([value])[0] if self.coll.world > 1 else float(value)

    # ------------------------------------------------------------------ the fast path of train()
    def _enqueue_step(self, mfccs, f, l, s, ll, n):
        """Everything of one optimisation step, enqueued without waiting for any of it.  Returns the step's token
        (nasr_step_token): the name under which its end can be asked about later, however many steps follow."""
        ticket = self._take_staged(mfccs)
        if ticket is not None:
            self.engine.commit_batch(ticket)
        else:
            self._upload(f, l, s, ll)
        self._feed_teacher(f, s)
        beam = self.train_ler_decoder == 'beam'
        self.engine.set_step_decode(True, logits=beam, greedy=not beam)     # (the beam search reads the logits; no greedy pass then)
        self.engine.compute_grads()
        if self.coll.world > 1:
            self.after_compute_grads()
            if self._grad_tensor is None:
                self._grad_tensor = self.engine.grad_tensor()
                self._reducer = self.coll.bucketed(self.engine, self._grad_tensor) if self.bucketed_allreduce else None
            if self._reducer is not None:
                self._reducer.all_reduce()
            else:
                self.coll.all_reduce_sum_(self._grad_tensor)
        self._apply_adam(1.0 / n)
        return self.engine.step_token()

    def _apply_adam(self, grad_scale):
        """apply_adam of every step path.  With a learning-rate schedule in the config the step size of
        global step s is set right before it: a launch argument, so steps still in flight keep theirs."""
        if getattr(self.config, 'lr_schedule_on', False):
            self.engine.set_learning_rate(self.config.learning_rate_at(self.global_step))
        self.engine.apply_adam(grad_scale)

    @contextlib.contextmanager
    def _averaged(self):
        """What is not a training step runs inside: the last step settled, and with ema_decay the average in the
        parameters' place (swap, run, swap: the training bits come back as they were)."""
        self._settle()
        if not self._ema or self.engine.ema()[2]:           # (nested: the average is in place already)
            yield
            return
        self.engine.ema_swap()
        try:
            yield
        finally:
            self.engine.ema_swap()

    # ------------------------------------------------------------------ the step's LER (tfnetwork.py:61-70)
    def _beam_ler(self, logits, s, l, ll):
        hyps = self.engine.beam_search(logits, self._logit_lens(s), self.beam_width, merge_repeated=True)[0]
        return self.engine.label_error_rate(hyps, l, ll)

    def _step_ler(self, hyps, f, l, s, ll, lazy):
        """mean_ler of the step just enqueued: greedy from the device's decode, or the reference's beam search on the step's
        own logits - on a host thread (the C++ decoder runs one thread per utterance and holds no interpreter lock)."""
        if self.train_ler_decoder != 'beam':
            return self.engine.label_error_rate(hyps, l, ll)
        logits = self.engine.step_logits(len(s), f.shape[1])
        if not lazy:
            return self._beam_ler(logits, s, l, ll)
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=4, thread_name_prefix='nasr-beam')
        return self._pool.submit(self._beam_ler, logits, s, l, ll)

    def _redo_step(self, batch, why):
        """A void step's batch again, start to finish, until it counts; returns the (loss, mean_ler) of the attempt that
        did.  Every rank takes this path at the same point of its call sequence and runs the same number of attempts: the
        fault word is all-reduced with the gradients, so 'void' is the same answer everywhere."""
        mfccs, f, l, s, ll, n = batch
        for attempt in range(3):
            self.logger.warning('%s: repeating its batch' % why)
            token = self._enqueue_step(None, f, l, s, ll, n)
            loss, fault, hyps = self.engine.step_results(len(s), f.shape[1])
            ler = float('nan') if fault else self._step_ler(hyps, f, l, s, ll, lazy=False)
            if not self.engine.settle_token(token):
                return loss, ler
        raise RuntimeError('a training step stayed void after 3 attempts')

    def _settle(self):
        """Before anything that is not the next fast-path step (validation, checkpoint, decode, the slow path): wait for
        the last fast-path step and repeat it if it was void."""
        if self._pending is not None:
            (batch, token), self._pending = self._pending, None
            if self.engine.settle_token(token):
                self._redo_step(batch, 'the last training step was void (persistent recurrence aborted on some rank)')

    def _finish_async(self, batch, token, lazy=False):
        mfccs, f, l, s, ll, n = batch
        loss, fwd_fault, hyps = self.engine.step_results(len(s), f.shape[1])
        if fwd_fault:
            # THIS rank's forward recurrence aborted: its loss and decode mean nothing.  The step is void on every rank
            # (the fault word travels with the gradients); it is repeated where every rank notices it.
            loss, ler = float('nan'), float('nan')
        else:
            ler = self._step_ler(hyps, f, l, s, ll, lazy)
        # the step BEFORE this one has ended by now (stream order): was it void?
        prev, self._pending = self._pending, (batch, token)
        if prev is not None and self.engine.settle_token(prev[1]):
            # This step was enqueued before anybody knew: whatever voided the previous one (a co-tenant, a placement) may
            # have voided it too.  Learn its fate BEFORE anything else is enqueued, then repeat what was void, in order.
            self._pending = None
            cur_void = self.engine.settle_token(token)
            self._redo_step(prev[0], 'step %d was void (persistent recurrence aborted on some rank)' % (self.global_step - 1))
            if cur_void:
                loss, ler = self._redo_step(batch, 'step %d was void as well' % self.global_step)
        elif fwd_fault and self.coll.world == 1:
            # single process: nobody else to keep in step with - settle this one now and report the repeat's values
            self._pending = None
            self.engine.settle_token(token)
            loss, ler = self._redo_step(batch, 'step %d was void (persistent recurrence aborted)' % self.global_step)
        if hasattr(ler, 'result'):
            # lazy: the LER is still being decoded; the caller averages its window over the ranks (mean_over_ranks)
            if self.coll.world > 1:
                loss = self.coll.mean_scalars([loss])[0]
            return np.float32(loss), ler
        if self.coll.world > 1:
            # (a rank-local forward fault leaves NaN here on every rank: train_model keeps such a step out of its means;
            # the step itself is repeated one call later, where every rank sees the fault word)
            loss, ler = self.coll.mean_scalars([loss, ler])
        return np.float32(loss), np.float32(ler)

    def _context(self):
        """numcontext when training batches of features go to the GPU as their centre slice, else 0"""
        # rand_shift's roll-and-crop (dataset.py:23-31) leaves real neighbour frames where include_context put its pad
        # in the first / last numcontext frames: such batches are uploaded whole
        ctx = getattr(self.config, 'numcontext', 0)
        return ctx if self.device_context and ctx > 0 and not getattr(self.config, 'rand_shift', 0) > 0 else 0

    # ------------------------------------------------------------------ input pipeline
    def stage_batch(self, mfccs, labels, seq_len, labels_len):
        """Send a batch that train() will be given NEXT towards the GPU now: this process's shard goes through pinned
        memory and the engine's copy stream while the current step computes (the reference loads and feeds the next
        batch inside the timed step, dataset.py:33-40, train.py:23-26).  Safe to call from DataSet.prefetch's loader
        thread.  train() recognises the batch by identity; anything not staged is uploaded the synchronous way."""
        n, mine = self._towers()
        if len(mine) != 1:
            return False                        # towers time-sliced on one GPU: each upload replaces the resident batch
        f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, n, mine[0])
        if isinstance(f, AudioBatch):
            ticket = self.engine.stage_batch_audio(self.featurizer(), f.audios, l, ll, f.rates, f.aug(self.config.numcep),
                                                   self._wave(f))[2]
        else:
            ticket = self.engine.stage_batch(f, s, l, ll, self._context(), self._frame_width())
        if ticket is None:
            return False
        with self._staged_lock:
            self._staged[id(mfccs)] = (ticket, weakref.ref(mfccs))
        return True

    def _take_staged(self, mfccs):
        with self._staged_lock:
            ent = self._staged.pop(id(mfccs), None)
        if ent is None:
            return None
        if ent[1]() is not mfccs:               # the id was recycled by another array: the staged batch is an orphan
            self.engine.discard_batch(ent[0])
            return None
        return ent[0]

    def discard_staged(self):
        """Give back the slots of batches that were staged but never trained on (the loop ended or raised)."""
        self._settle()
        with self._staged_lock:
            ents, self._staged = list(self._staged.values()), {}
        for ticket, _ in ents:
            try:
                self.engine.discard_batch(ticket)
            except Exception:                   # noqa: BLE001 - already committed or discarded
                pass

    def _train_sliced(self, mfccs, labels, seq_len, labels_len):
        """num_gpus towers time-sliced on the one GPU of a single process: each tower's shard in turn through the engine, the
        gradients summed on the host (average_gradients, tfnetwork.py:72-86), one Adam step; a void tower (its persistent
        recurrence gave up: the handle runs the per-step kernels from then on) repeats the whole step."""
        from .._lib import NasrError
        self._settle()
        n, mine = self._towers()
        for attempt in range(3):
            losses, lers, gsum, void = [], [], None, False
            for k in mine:
                f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, n, k)
                self._upload(f, l, s, ll)
                self._feed_teacher(f, s)
                beam = self.train_ler_decoder == 'beam'
                self.engine.set_step_decode(True, logits=beam, greedy=not beam)
                self.engine.compute_grads()
                try:
                    losses.append(self.engine.get_loss())
                    hyps = None if self.train_ler_decoder == 'beam' else self.engine.get_decoded(len(s), f.shape[1])
                    lers.append(self._step_ler(hyps, f, l, s, ll, lazy=False))
                    g = self.engine.get_grads().astype(np.float64)
                except NasrError as exc:
                    if not self._is_abort(exc):
                        raise
                    void = True
                    break
                gsum = g if gsum is None else gsum + g
            if not void:
                self.engine.set_grads((gsum / n).astype(np.float32))
                self._apply_adam(1.0)
                if not self.engine.step_void():
                    return np.float32(np.mean(losses)), np.float32(np.mean(lers))
            self.logger.warning('step %d was void (persistent recurrence aborted): repeating it' % self.global_step)
        raise RuntimeError('training step %d stayed void after 3 attempts' % self.global_step)

    def validate(self, mfccs, labels, seq_len, labels_len):
        with self._averaged():
            loss, ler, _ = self._loss_ler(mfccs, labels, seq_len, labels_len)
        return [np.float32(loss), np.float32(ler)]

    def evaluate(self, mfccs, labels, seq_len, labels_len):
        with self._averaged():
            loss, ler, hyps = self._loss_ler(mfccs, labels, seq_len, labels_len, self.language_model())
        # SparseTensorValue.values: every utterance's ids concatenated (tfnetwork.py:176-177)
        flat = np.asarray([i for h in hyps for i in h], dtype=np.int64)
        return flat, np.float32(loss), np.float32(ler)

    def decode(self, mfccs, seq_len):
        with self._averaged():
            hyps = self._decode(mfccs, seq_len, self.decoder, self.language_model())
        return np.asarray([i for h in hyps for i in h], dtype=np.int64)

    def stream(self, slots=1, lookahead=None):
        """A stream.StreamingRecognizer on this network: `slots` concurrent streams fed chunk by chunk, the LSTM state
        carried on the GPU, the hypothesis available after every chunk.  On a training network with ema_decay
        every feed of the session runs on the averaged parameters.  A bidirectional network streams
        with `lookahead` frames of right context (None: the config's stream_lookahead), a unidirectional
        one ignores both.  Raises the library's message for a network that cannot stream (stack-reshape merge, dropout,
        WaveNet, LAS)."""
        from ..stream import StreamingRecognizer
        if not int(getattr(getattr(self.engine, 'cfg', None), 'bidirectional', 0)):
            return StreamingRecognizer(self, slots)
        if lookahead is None:
            lookahead = int(getattr(self.config, 'stream_lookahead', 0))
        if lookahead < 1:
            raise ValueError('a bidirectional network streams only with a look-ahead: set stream_lookahead (frames, >= 1) '
                             'under [Parameters] or pass lookahead=')
        return StreamingRecognizer(self, slots, lookahead=lookahead)

    def align(self, mfccs, labels, seq_len, labels_len):
        """Forced alignment: for every utterance (score, [(symbol id, first frame, last frame)] in label
        order) - the log-probability of its best CTC path and the logit frames that path spends on each label (blank
        frames belong to no symbol).  Walk and traceback run on the GPU."""
        from ..align import spans
        labels = np.asarray(labels, dtype=np.int32).reshape(len(seq_len), -1)

        def run():
            self._upload(mfccs, labels, seq_len, labels_len, training=False)
            return self.engine.align_resident(len(seq_len), np.shape(mfccs)[1])
        with self._averaged():
            path, score = self._retry_aborted(run)
        return [(float(score[b]), spans(path[b], labels[b, :int(labels_len[b])])) for b in range(len(seq_len))]

    def align_audio(self, audios, rates, labels, labels_len):
        b = self.audio_batch(audios, rates)
        return self.align(b, labels, b.seq_len, labels_len)

    # ------------------------------------------------------------------ the same four calls on audio
    # (utils.py:24-31 made on the device per batch instead of pickled ahead: the features never reach the host)
    def train_audio(self, audios, rates, labels, labels_len):
        b = self.audio_batch(audios, rates)
        return self.train(b, labels, b.seq_len, labels_len)

    def validate_audio(self, audios, rates, labels, labels_len):
        b = self.audio_batch(audios, rates)
        return self.validate(b, labels, b.seq_len, labels_len)

    def evaluate_audio(self, audios, rates, labels, labels_len):
        b = self.audio_batch(audios, rates)
        return self.evaluate(b, labels, b.seq_len, labels_len)

    def decode_audio(self, audios, rates=None):
        b = self.audio_batch(audios, rates)
        return self.decode(b, b.seq_len)
