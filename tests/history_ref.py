"""What tests/test_gpu_history.py and tests/test_history_host.py share: the handle families, their batches, the histories
as data, and the reset / probe functions ("What a handle carries").  Not collected (no test_ prefix).

The invariant under test: a handle's results are a function of its parameters, its optimiser and other documented state,
its settings and the batch - and of nothing else it has ever run.  A *probe* resets every piece of carried state through
the public API and runs one fixed small batch through every output the family has.  A *history* is a list of API calls
run on a handle before the probe; it comes in two variants with the same shapes and calls but other seeds and feature
scales (x1 and x8), so that the bytes they leave in the grow-only workspaces differ everywhere.  The probe outputs of
both variants and of a fresh handle must agree bit for bit.

Batches.  Every CTC label is drawn without adjacent repeats and no longer than seq_len // 3, so that it is feasible at
frame skip 3 and in the windows of chunking 4 + 3 as well (tests/test_history_host.py asserts the library's rule).  The
lengths of a batch come from a seed of the shape alone; the features and the label ids from the variant's.
"""
import math

import numpy as np

from oracle import nasr_oracle as O

SCALES = (1.0, 8.0)          # the feature scale of variant 0 and 1
VARIANTS = (0, 1)
PROBE_SEQ = (37, 21, 9, 30, 14)      # sum 111: 111 % 32 = 15 (odd), ceil(111 / 16) = 7 (odd); one full-length utterance

# name -> (B, T, width of the label array, how the lengths are drawn).  'big' is larger than every probe in every
# dimension, has Bp 32 and a label array of 96 columns: ctc_states_per_lane(96) = 4 against the probes' 2.
SHAPES = {
    'big': (20, 64, 96, 'ragged'),
    'small': (3, 9, 2, 'ragged'),
    'b17': (17, 21, 4, 'ragged'),
    'alt': (7, 37, 6, 'ragged'),       # the CTC probes' T at another B
    'chunk': (6, 20, 5, 'ragged'),     # chunking 4 + 3: windows [4k, 4k + 7) - the full-length utterance has 5
    'skip': (6, 31, 5, 'ragged'),      # frame skip 3: 11 network frames
    'padded': (9, 40, 4, 'short'),     # mostly padding: compacted when compaction is on
    'full': (6, 12, 4, 'full'),        # nothing to compact
}
LAS_WIDTH = {'big': 30, 'small': 3, 'b17': 5, 'alt': 9, 'padded': 4, 'full': 6}     # U, the probe's is 7


def states_per_lane(width):
    """ctc_states_per_lane (csrc/kernels.h) of a label array `width` columns wide"""
    ks = (2 * max(width, 0) + 1 + 63) // 64
    return 2 if ks <= 1 else ks if ks <= 8 else 12 if ks <= 12 else 16 if ks <= 16 else ks


def lengths(B, T, how, shape_seed):
    rs = np.random.RandomState(shape_seed)
    if how == 'full':
        return np.full(B, T, np.int32)
    seq = rs.randint(1, (T // 4 if how == 'short' else T) + 1, size=B)
    seq[B // 2] = T
    return seq.astype(np.int32)


def label_lengths(seq, width, shape_seed, div=3):
    rs = np.random.RandomState(shape_seed + 1)
    ll = np.minimum(rs.randint(1, width + 1, size=len(seq)), np.asarray(seq) // div)
    k = int(np.argmax(seq))
    ll[k] = min(width, int(seq[k]) // div)              # the longest utterance carries the longest label that fits
    return ll.astype(np.int32)


def ctc_batch(F, C, seq, width, seed, scale, shape_seed):
    """(feats [B,T,F] zero past seq_len, seq_len, labels [B,width] in [0, C-2] without adjacent repeats, label_len)"""
    rs = np.random.RandomState(seed)
    seq = np.asarray(seq, np.int32)
    B, T = len(seq), int(seq.max())
    feats = (scale * rs.randn(B, T, F)).astype(np.float32)
    for b in range(B):
        feats[b, seq[b]:] = 0
    ll = label_lengths(seq, width, shape_seed)
    labels = np.zeros((B, width), np.int32)
    for b in range(B):
        v = int(rs.randint(0, C - 1))
        for i in range(ll[b]):
            labels[b, i] = v
            v = (v + 1 + int(rs.randint(0, C - 2))) % (C - 1)
    return feats, seq, labels, ll


def las_batch(F, C, seq, U, seed, scale, shape_seed):
    """(feats, seq_len, dense labels [B,U] in [0, C-1], label_len in [0,U])"""
    rs = np.random.RandomState(seed)
    seq = np.asarray(seq, np.int32)
    B, T = len(seq), int(seq.max())
    feats = (scale * rs.randn(B, T, F)).astype(np.float32)
    for b in range(B):
        feats[b, seq[b]:] = 0
    labels = rs.randint(0, C, size=(B, U)).astype(np.int32)
    ll = np.random.RandomState(shape_seed + 1).randint(0, U + 1, size=B).astype(np.int32)
    ll[0] = U
    return feats, seq, labels, ll


def planted_nan(n, seed):
    """a gradient with one NaN in the middle, as tests/test_gpu_grad_clip.py plants it"""
    g = (0.01 * np.random.RandomState(seed).randn(n)).astype(np.float32)
    g[0], g[-1], g[n // 2] = 3.0, -4.0, np.nan
    return g


def audio_lengths(rate):
    """samples of the utterances of the audio-fed batch: ragged, the first sets T (about 30 frames at a 10 ms step)"""
    return [int(rate * s) for s in (0.325, 0.11, 0.19, 0.25, 0.05, 0.3)]


# ======================================================================================================= families
class Family:
    """One handle family at its probe shape.  kind: 'lstm' (dense stages included), 'wavenet' or 'las'."""
    kind = 'lstm'
    stream = None            # 'uni' (nasr_stream_open), 'lookahead' (nasr_stream_open_lookahead) or None
    chunking = frame_skip = distill = rec_switch = compaction_switch = False
    compaction = False       # the probe's row compaction
    wgrad = False            # has the weight-gradient side stream
    ctc = True
    RATE = 8000

    # ---- batches
    def shape_seed(self, name):
        return 7000 + 13 * sorted(SHAPES).index(name)

    def batch(self, name, variant):
        key = (name, variant)
        if key not in self._batches:
            B, T, width, how = SHAPES[name]
            ss = self.shape_seed(name)
            self._batches[key] = self.make_batch(lengths(B, T, how, ss), self.width(name, width),
                                                 100 + 1000 * variant + ss, SCALES[variant], ss)
        return self._batches[key]

    def width(self, name, width):
        return width

    def make_batch(self, seq, width, seed, scale, shape_seed):
        return ctc_batch(self.F, self.C, seq, width, seed, scale, shape_seed)

    def batch_names(self):
        """every batch some history of this family uses"""
        names = set()
        for h in self.histories:
            for op in HISTORIES[h](self):
                names.update(a for a in op[1:] if isinstance(a, str) and a in SHAPES)
        return sorted(names)

    def audio_batch(self, variant):
        """(audios, labels, label_len, BatchAug pieces): utterances of noise at the variant's scale"""
        from neuralasr_amd.features import num_frames
        rs = np.random.RandomState(300 + variant)
        audios = [(0.05 * SCALES[variant] * rs.randn(n)).astype(np.float32) for n in audio_lengths(self.RATE)]
        seq = np.asarray([num_frames(a.size, self.RATE, numcep=self.F) for a in audios], np.int32)
        _, _, labels, ll = self.make_batch(seq, 5, 400 + variant, 1.0, 55)
        tm = np.asarray([[[1, 2]] if s >= 4 else [[0, 0]] for s in seq], np.int32)
        fm = np.asarray([[[2, 3]]] * len(seq), np.int32)
        return audios, seq, labels, ll, tm, fm


class LstmFamily(Family):
    def __init__(self, name, spec, histories, compaction=True, persistent=True, wgrad=False, pseed=3, drop=None,
                 resident_width=None):
        self.name, self.spec, self.histories = name, spec, histories
        self.F, self.C = spec.feature_size, spec.num_classes
        self.compaction = compaction and not spec.deepspeech
        self.persistent, self.wgrad, self.drop = persistent, wgrad, drop
        # persistent: the recurrence path of the probe and of the histories; resident_width: the handle is created on a
        # resident kind (a width the persistent kernels take) - with persistent False it is switched to the per-step path
        self.resident_width = persistent if resident_width is None else resident_width
        dense = spec.deepspeech
        dropout = any(spec.drop_p(i) > 0 for i in range(4))
        concat = spec.bidirectional and spec.merge == 'concat'
        self.stream = None if dropout else 'uni' if not spec.bidirectional else 'lookahead' if concat else None
        self.chunking = concat and not dense and not dropout
        self.frame_skip = True
        self.distill = spec.merge != 'stack_reshape'
        self.rec_switch = True
        self.compaction_switch = not dense
        self._batches = {}
        rs = np.random.RandomState(pseed)
        scale = 0.15 if dense else 0.05            # as tests/test_gpu_deepspeech.py and tests/test_gpu_edges.py move them
        self.p0 = O.flatten([p + scale * rs.randn(*p.shape) for p in O.init_params(spec, seed=pseed)]).astype(np.float32)
        self._probe = None

    def make(self):
        from neuralasr_amd.engine import Engine
        s = self.spec
        e = Engine(s.feature_size, s.hidden, s.num_layers, s.bidirectional, s.merge, s.num_classes, forget_bias=s.forget_bias,
                   learning_rate=1e-3, pre=s.pre, post=s.post, relu_clip=s.relu_clip, dropout=s.dropout)
        assert e.recurrence_mode == ('persistent' if self.resident_width else 'per-step'), e.recurrence_mode
        if self.resident_width and not self.persistent:
            e.set_recurrence_mode(False)
        assert e.wgrad_overlap == self.wgrad
        return e

    def probe_batch(self):
        if self._probe is None:
            if not self.spec.deepspeech:
                self._probe = ctc_batch(self.F, self.C, PROBE_SEQ, 6, 11, 1.0, 21)
            else:
                # the clipped ReLU's kinks (tests/test_gpu_deepspeech.py): of 24 inputs, the one whose nearest
                # pre-activation is furthest from a kink under the masks of the probe's first pass
                params = O.unflatten(self.spec, self.p0.astype(np.float64))
                best = (-1.0, None)
                for seed in range(24):
                    bt = ctc_batch(self.F, self.C, (14, 9, 5, 12), 3, 500 + seed, 1.0, 21)
                    m = O.deepspeech_kink_margin(self.spec, params, bt[0], bt[1], drop=self.drop)
                    if m > best[0]:
                        best = (m, bt)
                assert best[0] > 1e-5, best[0]
                self._probe = best[1]
        return self._probe

    def reference_loss(self, feats, seq, labels, ll):
        params = O.unflatten(self.spec, self.p0.astype(np.float64))
        logits, _ = O.network_forward(self.spec, params, feats, seq, drop=self.drop)
        return float(O.ctc_loss_and_grad(logits, labels, ll, seq)[0].mean())

    def reset(self, e):
        e.set_ema(0.0)
        e.set_grad_clip(0.0)
        e.grad_clip_stats(reset=True)
        if self.chunking:
            e.set_chunking(0)
        e.set_frame_skip(1)
        if self.distill:
            e.set_distill(0.0, 1.0)
        e.set_recurrence_mode(self.persistent)
        e.set_graph_mode(True)
        e.set_row_compaction(self.compaction)
        if self.wgrad:
            e.set_wgrad_overlap(True)
        e.set_params(self.p0)
        zero = np.zeros(e.param_count, np.float32)
        e.set_adam_state(zero, zero, 0)
        if self.drop:
            e.set_dropout_state(*self.drop)

    def probe(self, e):
        self.reset(e)
        bt = self.probe_batch()
        B, T = bt[0].shape[:2]
        out = {}
        out['loss'], out['nll'], out['grads'] = e.loss_and_grads(*bt)
        out['rows'] = e.resident_rows()
        if not self.spec.deepspeech:
            assert out['rows'] == (int(np.sum(bt[1])) if self.compaction else T * 16)
        out['train'] = [e.train_step(*bt), e.train_step(*bt)]
        out['params'] = e.get_params()
        out['adam_m'], out['adam_v'], out['adam_step'] = e.get_adam_state()
        if self.drop:
            out['drop_state'] = e.dropout_state()         # the masks of the forward pass below
        out['logits'] = e.forward(bt[0], bt[1])
        out['greedy'] = e.greedy_decode(bt[0], bt[1])
        out['path'], out['score'] = e.align(*bt)
        out['mode'] = e.recurrence_mode
        return out


class WaveNetFamily(Family):
    kind = 'wavenet'
    distill = True

    def __init__(self, name, histories):
        import wavenet_ref as W
        self.name, self.histories = name, histories
        self.W, self.spec = W, W.Spec(11, 7, num_blocks=1)
        self.F, self.C = 11, 7
        self._batches = {}
        # gamma and beta moved off 1 and 0, as tests/test_gpu_wavenet.py's start_params
        p = W.init_params(self.spec, 9).astype(np.float64)
        rs = np.random.RandomState(109)
        o = 0
        for tname, r, c in W.tensor_specs(self.spec):
            if tname.endswith('gamma'):
                p[o:o + r] = 1 + 0.2 * rs.randn(r)
            elif tname.endswith('beta'):
                p[o:o + r] = 0.2 * rs.randn(r)
            o += r * c
        self.p0 = p.astype(np.float32)

    def make(self):
        from neuralasr_amd.engine import WaveNetEngine
        s = self.spec
        return WaveNetEngine(s.F, s.C, num_blocks=s.nb, rates=s.rates, learning_rate=1e-3)

    def probe_batch(self):
        # T 23: rate 16's taps at +-16, +-32, +-48 - only +-16 falls inside, and for most frames on one side only
        return ctc_batch(self.F, self.C, (23, 12, 5, 19, 8), 4, 12, 1.0, 22)

    def reference_loss(self, feats, seq, labels, ll):
        import torch
        with torch.no_grad():
            logits, _ = self.W.forward(self.spec, self.W.unflatten(self.spec, self.p0), feats, True)
            return float(self.W.ctc_mean(logits, seq, labels, ll)[0])

    def reset(self, e):
        e.set_ema(0.0)
        e.set_grad_clip(0.0)
        e.grad_clip_stats(reset=True)
        e.set_distill(0.0, 1.0)
        e.set_params(self.p0)
        zero = np.zeros(e.param_count, np.float32)
        e.set_adam_state(zero, zero, 0)
        st = self.W.bn_initial(self.spec)
        e.set_bn_state(st['mm'], st['mv'], st['biased'], 0)

    def probe(self, e):
        self.reset(e)
        bt = self.probe_batch()
        out = {}
        out['loss'], out['nll'], out['grads'] = e.loss_and_grads(*bt)
        out['batch_mean'], out['batch_var'] = e.batch_stats()
        out['bn_after_grads'] = e.bn_state()
        out['train'] = [e.train_step(*bt), e.train_step(*bt)]
        out['params'] = e.get_params()
        out['adam_m'], out['adam_v'], out['adam_step'] = e.get_adam_state()
        out['bn'] = e.bn_state()
        out['logits'] = e.forward(bt[0], bt[1])
        out['greedy'] = e.greedy_decode(bt[0], bt[1])
        out['path'], out['score'] = e.align(*bt)
        return out


class LasFamily(Family):
    kind = 'las'
    ctc = False
    SAMPLING = (0.1, 5, 17)          # p, seed, counter of the probe's first pass

    def __init__(self, name, histories):
        from tests import las_ref
        self.name, self.histories = name, histories
        self.R = las_ref
        self.F, self.C = 20, 12
        self._batches = {}
        # the 'moderate' trained-like regime of tests/test_gpu_las.py: the attention is peaked enough to carry gradient
        self.p0 = las_ref.trained_like(las_ref.initial_params(self.F, self.C, seed=3), self.F, self.C,
                                       *las_ref.REGIMES['moderate'])

    def width(self, name, width):
        return LAS_WIDTH[name]

    def make_batch(self, seq, width, seed, scale, shape_seed):
        return las_batch(self.F, self.C, seq, width, seed, scale, shape_seed)

    def make(self):
        from neuralasr_amd.engine import LasEngine
        return LasEngine(self.F, self.C, sampling_probability=self.SAMPLING[0], seed=self.SAMPLING[1], learning_rate=1e-3)

    def probe_batch(self):
        return las_batch(self.F, self.C, (17, 9, 4, 13, 1), 7, 13, 1.0, 23)      # T 17: the pyramid's odd-length edge

    def reference_loss(self, feats, seq, labels, ll):
        import torch
        with torch.no_grad():
            logits = self.R.forward(self.R.unflatten(self.p0, self.F, self.C), feats, labels, labels)
            return float(self.R.sequence_loss(logits, labels, ll))

    def reset(self, e):
        e.set_ema(0.0)
        e.set_grad_clip(0.0)
        e.grad_clip_stats(reset=True)
        e.set_params(self.p0)
        zero = np.zeros(e.param_count, np.float32)
        e.set_adam_state(zero, zero, 0)
        e.set_sampling_state(*self.SAMPLING)

    def probe(self, e):
        self.reset(e)
        bt = self.probe_batch()
        out = {}
        out['loss'], out['nll'], out['grads'] = e.loss_and_grads(*bt)
        out['logits'], out['fed'] = e.logits(), e.fed_ids()
        out['train'] = [e.train_step(*bt), e.train_step(*bt)]
        out['params'] = e.get_params()
        out['adam_m'], out['adam_v'], out['adam_step'] = e.get_adam_state()
        out['sampling'] = e.sampling_state()
        out['forward'] = e.las_forward(*bt, sample=False)
        beam = e.beam_search(bt[0], bt[1], 4, 12, self.C - 2, self.C - 1, trace=True)
        for k in sorted(beam):
            out['beam_' + k] = beam[k]
        return out


# ======================================================================================================= histories
# A history is a function of the family that returns a list of operations (name, arguments...); a batch argument is a
# name of SHAPES, resolved to the variant's batch when the history runs (run_history).  Each ends with the settings it
# touched back at the probe's values; Family.reset then sets all carried state whether the history touched it or not.
def h_shapes(f):
    """larger, then smaller, then another Bp"""
    return [('train', 'big'), ('grads', 'big'), ('forward', 'big'), ('train', 'small'), ('grads', 'small'),
            ('train', 'b17'), ('greedy', 'b17') if f.ctc else ('beam', 'b17')]


def h_recurrence(f):
    """the other recurrence path, graph mode on and off.  A width the resident kernels do not take has the per-step
    path alone: there the graph mode is toggled in the other order (off first, then on again)."""
    shapes = [('train', 'alt'), ('train', 'b17'), ('grads', 'alt')]
    if not f.persistent:
        return [('graph', False)] + shapes + [('graph', True)] + shapes
    return [('rec', False), ('graph', True)] + shapes + [('graph', False)] + shapes + [('graph', True), ('rec', True)]


def h_compaction(f):
    on = f.compaction
    ops = []
    if f.compaction_switch:
        ops += [('compact', not on), ('train', 'padded'), ('compact', on), ('train', 'full'), ('compact', not on),
                ('train', 'full'), ('grads', 'padded'), ('compact', on), ('train', 'padded')]
    if f.wgrad:
        ops += [('wgrad', False), ('train', 'alt'), ('wgrad', True), ('train', 'alt'), ('wgrad', False), ('train', 'b17'),
                ('wgrad', True)]
    return ops


def h_chunking(f):
    return [('chunking', 4, 3), ('train', 'chunk'), ('chunking', 0, 0)]


def h_frame_skip(f):
    return [('skip', 3), ('train', 'skip'), ('skip', 1)]


def h_distill(f):
    return [('distill', 0.5, 2.0), ('distill_host', 'alt'), ('distill', 0.0, 1.0),
            ('distill', 0.3, 1.0), ('distill_teacher', 'b17'), ('distill', 0.0, 1.0)]


def h_optimiser(f):
    return [('clip', math.inf), ('train', 'alt'), ('nan_step',), ('clip', 0.0),
            ('ema', 0.9), ('train', 'alt'), ('train', 'b17'), ('ema_swap',), ('forward', 'small'), ('ema_swap',), ('ema', 0.0)]


def h_sessions(f):
    ops = [('session',)] if f.stream else []
    ops += [('align', 'big'), ('forward', 'small'), ('greedy', 'b17')] if f.ctc else [('forward', 'small'), ('beam', 'b17')]
    return ops + [('stage2', 'alt', 'small')]


def h_audio(f):
    return [('audio',)]


def h_poison(f):
    return [('poison', 'big')]


HISTORIES = {'shapes': h_shapes, 'recurrence': h_recurrence, 'compaction': h_compaction, 'chunking': h_chunking,
             'frame-skip': h_frame_skip, 'distill': h_distill, 'optimiser': h_optimiser, 'sessions': h_sessions,
             'audio': h_audio, 'poison': h_poison}


def _session(f, e, variant):
    """a session opened, fed ragged chunks in two feeds, and closed"""
    rs = np.random.RandomState(600 + variant)
    a = (SCALES[variant] * rs.randn(2, 8, f.F)).astype(np.float32)
    b = (SCALES[variant] * rs.randn(2, 6, f.F)).astype(np.float32)
    if f.stream == 'uni':
        e.stream_open(2)
        e.stream_feed(a, [8, 5])
        e.stream_feed(b, [2, 6])
    else:
        e.stream_open_lookahead(2, 3)
        e.stream_feed_lookahead(a, [8, 5], [False, False])
        e.stream_feed_lookahead(b, [6, 4], [True, True])
    e.stream_close()


def _audio(f, e, variant):
    """a training step on a batch given as audio, with SpecAugment masks, reverberation and noise"""
    from neuralasr_amd.engine import BatchAug, WaveAug
    from neuralasr_amd.features import Featurizer
    audios, seq, labels, ll, tm, fm = f.audio_batch(variant)
    rs = np.random.RandomState(700 + variant)
    fz = Featurizer(f.RATE, f.F, 0)
    try:
        rir = np.exp(-np.arange(40) / 9.0) * rs.randn(40)
        rir[0] = 1.0
        fz.set_rirs([(rir / np.sqrt(np.sum(rir * rir))).astype(np.float32)])
        fz.set_noise([(0.1 * rs.randn(700)).astype(np.float32)])
        B = len(audios)
        wave = WaveAug([0] * B, [0] * B, [3] * B, [10.0] * B)
        got_seq, T = e.upload_batch_audio(fz, audios, labels, ll, None, aug=BatchAug(f.F, tm, fm), wave=wave)
        assert got_seq.tolist() == seq.tolist() and T == int(seq.max())
        e.compute_grads()
        e.apply_adam(1.0)
        e.synchronize()
    finally:
        fz.close()


def history_params(f, variant):
    """what a history trains from: the probe's parameters (variant 0), the same times 1.25 (variant 1)"""
    return (f.p0 * np.float32(1.0 + 0.25 * variant)).astype(np.float32)


def run_history(f, e, name, variant, teacher=None):
    """The operations of history `name` on handle e with the variant's data and the variant's parameters.  The
    parameters matter: a handle that was never given any holds zeros, and with zero weights every activation and every
    data gradient of a history is exactly 0 - the workspaces would hold nothing for the probe to trip over."""
    e.set_params(history_params(f, variant))
    for op in HISTORIES[name](f):
        k, a = op[0], op[1:]
        bt = f.batch(a[0], variant) if a and isinstance(a[0], str) else None
        if k == 'train':
            e.train_step(*bt)
        elif k == 'grads':
            e.loss_and_grads(*bt)
        elif k == 'forward':
            e.las_forward(*bt, sample=True) if f.kind == 'las' else e.forward(bt[0], bt[1])
        elif k == 'greedy':
            e.greedy_decode(bt[0], bt[1])
        elif k == 'align':
            e.align(*bt)
        elif k == 'beam':
            e.beam_search(bt[0], bt[1], 3, 9, f.C - 2, f.C - 1)
        elif k == 'rec':
            e.set_recurrence_mode(a[0])
            assert e.recurrence_mode == ('persistent' if a[0] else 'per-step')
        elif k == 'graph':
            e.set_graph_mode(a[0])
        elif k == 'compact':
            e.set_row_compaction(a[0])
        elif k == 'wgrad':
            e.set_wgrad_overlap(a[0])
        elif k == 'chunking':
            e.set_chunking(a[0], a[1])
        elif k == 'skip':
            e.set_frame_skip(a[0])
        elif k == 'distill':
            e.set_distill(a[0], a[1])
        elif k == 'distill_host':
            e.upload_batch(*bt)
            B, T = bt[0].shape[:2]
            rs = np.random.RandomState(800 + variant)
            e.set_teacher_logits((SCALES[variant] * rs.randn(e.logit_frames(T), B, f.C)).astype(np.float32))
            e.compute_grads()
            e.apply_adam(1.0)
        elif k == 'distill_teacher':
            # Two handles on streams of their own: the host waits on either side, so that no pass of the teacher's runs
            # beside a step of the student's ("One stream for both", supposes that two resident
            # recurrences in flight together can cost one of them its hand-off).
            e.synchronize()
            teacher.set_params((f.p0 * np.float32(1.0 + 0.5 * variant)).astype(np.float32))
            teacher.upload_batch(*bt)
            teacher.forward_resident(*bt[0].shape[:2])          # fetches the logits: synchronous
            assert teacher.persist_stats()[0] == 0
            e.upload_batch(*bt)
            e.take_teacher_logits(teacher)
            e.compute_grads()
            e.apply_adam(1.0)
        elif k == 'clip':
            e.set_grad_clip(a[0])
        elif k == 'nan_step':
            before = e.grad_clip_stats()['skipped']
            e.set_grads(planted_nan(e.param_count, 900 + variant))
            e.apply_adam(1.0)
            assert e.grad_clip_stats()['skipped'] == before + 1
        elif k == 'ema':
            e.set_ema(a[0])
        elif k == 'ema_swap':
            e.ema_swap()
        elif k == 'session':
            _session(f, e, variant)
        elif k == 'stage2':
            t1, t2 = e.stage_batch(*bt), e.stage_batch(*f.batch(a[1], variant))
            assert t1 is not None and t2 is not None
            e.commit_batch(t1)
            e.compute_grads()
            e.apply_adam(1.0)
            e.discard_batch(t2)
        elif k == 'audio':
            _audio(f, e, variant)
        elif k == 'poison':
            # parameters at +-3e38: every product overflows, every sum of them is inf - inf.  Only on a handle whose
            # recurrence runs on the per-step kernels (the resident kernels' hand-off words and range checks are not
            # made for non-finite input, and nothing here provokes them).
            if f.kind == 'lstm':
                assert e.recurrence_mode == 'per-step'
            if f.kind == 'las':
                e.set_sampling_state(0.0, 1, 0)         # feed the labels: no class is drawn from non-finite logits
            rs = np.random.RandomState(950 + variant)
            e.set_params(np.where(rs.rand(e.param_count) < 0.5, -3e38, 3e38).astype(np.float32))
            e.upload_batch(*bt)
            e.compute_grads()                           # forward and backward; the loss is not read as a number
            e.synchronize()
        else:
            raise ValueError(k)
    e.synchronize()


# ======================================================================================================= the table
_DS = O.ModelSpec(14, 20, 1, True, 'concat', 6, pre=(24, 24, 40), post=24, relu_clip=2.0, dropout=(0.1, 0.1, 0.1, 0.1))
_LSTM_ALL = ('shapes', 'recurrence', 'compaction', 'chunking', 'frame-skip', 'distill', 'optimiser', 'sessions', 'audio')


def _without(names, *drop):
    return tuple(n for n in names if n not in drop)


# family -> the histories it runs: those whose feature the family has.  (stack_reshape neither trains in windows nor
# distils; dense stages with dropout do not stream, compact or train in windows; WaveNet and LAS have no recurrence.)
# The distillation history runs on WaveNet only: on the LSTM handles (concat, unidirectional, DeepSpeech; Hp 64, resident
# recurrence) its first step - teacher logits given over the host, on a handle whose parameters were never set - ended in
# the resident recurrence's hand-off timeout (abort code 1) on an MI355X, twice, and the cause is not established.
TABLE = {
    'bilstm-stack': _without(_LSTM_ALL, 'chunking', 'distill'),
    'bilstm-concat': _without(_LSTM_ALL, 'distill'),
    'bilstm-concat-all-rows': ('shapes', 'compaction', 'chunking'),       # the second CTC probe: compaction off
    'lstm-uni': _without(_LSTM_ALL, 'chunking', 'distill'),
    'bilstm-h600': ('shapes', 'recurrence', 'poison'),
    'bilstm-h70-per-step': ('shapes', 'optimiser', 'poison'),
    'bilstm-h500x2': ('shapes', 'compaction'),
    'deepspeech': ('shapes', 'recurrence', 'frame-skip', 'optimiser', 'sessions', 'audio'),
    'wavenet': ('shapes', 'distill', 'optimiser', 'sessions', 'audio', 'poison'),
    'las': ('shapes', 'optimiser', 'sessions', 'audio', 'poison'),
}
CASES = [(f, h) for f, hs in TABLE.items() for h in hs]
_made = {}


def family(name):
    """the Family of a TABLE row, made on first use (the WaveNet and LAS references import torch)"""
    if name not in _made:
        hs = TABLE[name]
        _made[name] = {
            # F 13 (Fp 32), H 40 (Hp 64, the narrowest the resident kernels take), C 7; the probe has B 5 (Bp 16), T 37
            'bilstm-stack': lambda: LstmFamily(name, O.ModelSpec(13, 40, 1, True, 'stack_reshape', 7), hs),
            'bilstm-concat': lambda: LstmFamily(name, O.ModelSpec(13, 40, 2, True, 'concat', 7), hs),
            'bilstm-concat-all-rows': lambda: LstmFamily(name, O.ModelSpec(13, 40, 2, True, 'concat', 7), hs, compaction=False),
            'lstm-uni': lambda: LstmFamily(name, O.ModelSpec(13, 40, 2, False, 'none', 7), hs),
            # Hp 640: no resident kernel takes it, the per-step path is the default - and the one that may see NaN
            'bilstm-h600': lambda: LstmFamily(name, O.ModelSpec(13, 600, 1, True, 'concat', 7), hs, persistent=False),
            # Hp 128, two layers, a width the resident kernels take, switched to the per-step path: the probe and the
            # histories run on lstm.hip's kernels, as after a fallback
            'bilstm-h70-per-step': lambda: LstmFamily(name, O.ModelSpec(13, 70, 2, True, 'concat', 7), hs, persistent=False,
                                                      resident_width=True),
            # Hp 512 and two layers: the weight-gradient side stream exists
            'bilstm-h500x2': lambda: LstmFamily(name, O.ModelSpec(13, 500, 2, True, 'concat', 7), hs, wgrad=True),
            'deepspeech': lambda: LstmFamily(name, _DS, hs, pseed=6, drop=(4567, 11)),
            'wavenet': lambda: WaveNetFamily(name, hs),
            'las': lambda: LasFamily(name, hs),
        }[name]()
    return _made[name]


# ======================================================================================================= comparing
def assert_same(got, want, note):
    """probe outputs bit for bit: arrays with assert_array_equal, everything else with =="""
    assert sorted(got) == sorted(want), note
    for k in sorted(want):
        _same(got[k], want[k], '%s: %s' % (note, k))


def _same(a, b, note):
    if isinstance(b, np.ndarray):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, note
        np.testing.assert_array_equal(a, b, err_msg=note)
    elif isinstance(b, (tuple, list)) and any(isinstance(x, np.ndarray) for x in b):
        assert len(a) == len(b), note
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, '%s[%d]' % (note, i))
    else:
        assert a == b, '%s: %r != %r' % (note, a, b)


# ======================================================================================================= featurizer
FZ_RATE, FZ_CEP, FZ_CTX = 8000, 13, 2


def featurizer_clip():
    rs = np.random.RandomState(41)
    return (0.1 * rs.randn(3300)).astype(np.float32)          # 0.41 s, not a multiple of the frame step


def featurizer_history(fz, variant):
    """banks set and cleared, augmentation, a resampling call, longer and shorter utterances"""
    from neuralasr_amd.engine import WaveAug
    rs = np.random.RandomState(40 + variant)
    s = SCALES[variant]
    long_, short = (0.1 * s * rs.randn(16000)).astype(np.float32), (0.1 * s * rs.randn(130)).astype(np.float32)
    fz.compute([long_, short])
    rir = np.exp(-np.arange(300) / 40.0) * rs.randn(300)
    fz.set_rirs([(rir / np.sqrt(np.sum(rir * rir))).astype(np.float32)])
    fz.set_noise([(0.05 * s * rs.randn(900)).astype(np.float32)])
    fz.augment_audio([long_, short], None, WaveAug([0, 0], [0, -1], [5, 0], [5.0, 0.0]))
    fz.set_noise([])
    fz.set_rirs([])
    fz.resample([(0.1 * s * rs.randn(6000)).astype(np.float32)], [22050])
    fz.compute([(0.1 * s * rs.randn(7000)).astype(np.float32), short], rates=[16000, 8000])
    fz.compute([short])


def featurizer_probe(fz):
    feats, stats = fz.compute([featurizer_clip()], return_stats=True)
    return {'feats': feats[0], 'mean': stats[0][0], 'std': stats[0][1]}
