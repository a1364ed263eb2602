"""Engine: NumPy-in / NumPy-out wrapper over one libnasr handle (= one GPU).  This is the thin layer the
`Network` plugin classes (neuralasr_amd/networks) and bench.py sit on; all arithmetic happens in the HIP
library behind include/nasr.h."""
import collections
import ctypes
from ctypes import POINTER, byref, c_char, c_double, c_float, c_int, c_int32, c_int64, c_uint8, c_uint32, c_void_p

import numpy as np

from . import _lib


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _fp(a):
    return a.ctypes.data_as(POINTER(c_float))


def _ip(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_int32))


def skip_frames(n, frame_skip):
    """The frames the network sees of n input frames under a frame skip: frames 0, s, 2s, ... - ceil(n/s).
    n: an int or an integer array."""
    s = int(frame_skip)
    if not 1 <= s <= 8:
        raise ValueError('frame_skip = %d: must be in [1,8]' % s)
    if isinstance(n, (int, np.integer)):
        return (int(n) + s - 1) // s
    return (np.asarray(n).astype(np.int64) + s - 1) // s


def stream_keep(phase, n, frame_skip):
    """A stream slot's bookkeeping under a frame skip, as the library does it (nasr_stream.hip, keep_rows): the slot's
    utterance has had `phase` input rows so far, modulo the skip, and n new ones arrive.  Returns (first, kept, phase after):
    the new rows first, first + s, ... - `kept` of them - are those whose index in the utterance is a multiple of the skip."""
    s, phase, n = int(frame_skip), int(phase), int(n)
    first = (s - phase) % s
    kept = skip_frames(n - first, s) if n > first else 0
    return first, kept, (phase + n) % s


class BatchAug(collections.namedtuple('BatchAug', 'static_width time_masks freq_masks')):
    """SpecAugment masks of one batch (nasr_batch_aug, include/nasr.h): time_masks int32 [B, nt, 2] of (first frame, width),
    freq_masks int32 [B, nf, 2] of (first static column, width), either may be None; static_width is the width of the
    static block of a frame (the config's numcep).  The library checks them; a mask of width 0 is no mask."""
    __slots__ = ()

    def struct(self, B):
        """(_lib.BatchAug, the arrays it points into - to be kept alive over the call)"""
        arrs = []
        for m in (self.time_masks, self.freq_masks):
            m = np.zeros((B, 0, 2), np.int32) if m is None else _i32(m)
            if m.ndim != 3 or m.shape[0] != B or m.shape[2] != 2:
                raise ValueError('masks must be [B=%d, n, 2], not %s' % (B, m.shape))
            arrs.append(m)
        tm, fm = arrs
        return _lib.BatchAug(int(self.static_width), tm.shape[1], fm.shape[1], _ip(tm), _ip(fm)), arrs


class WaveAug(collections.namedtuple('WaveAug', 'rir noise noise_off snr_db')):
    """Waveform augmentation of one batch given as audio (nasr_wave_aug, include/nasr.h): rir int32 [B] (an
    index into the featurizer's RIR bank, -1: none), noise int32 [B] (into its noise bank, -1: none), noise_off int64 [B]
    (the clip's first sample) and snr_db float32 [B]; rir or noise may be None (none for the whole batch), noise_off and
    snr_db only without noise.  The library checks them against the banks."""
    __slots__ = ()

    def struct(self, B):
        """(_lib.WaveAug, the arrays it points into - to be kept alive over the call)"""
        def arr(a, dtype, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=dtype).ravel()
            if a.size != B:
                raise ValueError('%s must be [B=%d], not %d values' % (name, B, a.size))
            return a
        keep = [arr(self.rir, np.int32, 'rir'), arr(self.noise, np.int32, 'noise'), arr(self.noise_off, np.int64, 'noise_off'),
                arr(self.snr_db, np.float32, 'snr_db')]
        ptr = [None if a is None else a.ctypes.data_as(POINTER(t)) for a, t in zip(keep, (c_int32, c_int32, c_int64, c_float))]
        return _lib.WaveAug(*ptr), keep


class Engine:
    def __init__(self, feature_size, hidden, num_layers, bidirectional, merge, num_classes, forget_bias=1.0,
                 learning_rate=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, device_id=0, stream=None,
                 pre=(), post=0, relu_clip=20.0, dropout=()):
        """`pre` / `post` / `relu_clip` / `dropout`: the clipped-ReLU dense stages of the DeepSpeech family
        (networks/deepspeech.py): widths of the stages in front of the LSTM stack, width of the one behind it (0 = none),
        and the drop probability of each of them in that order."""
        self.lib = _lib.load()
        merge_id = _lib.MERGE_BY_NAME[merge] if isinstance(merge, str) else int(merge)
        pre, dropout = tuple(int(w) for w in pre), tuple(float(p) for p in dropout)
        if len(pre) > 3 or len(dropout) > 4:
            raise ValueError('at most 3 dense stages before the LSTM stack and one behind it')
        cfg = _lib.ModelCfg(int(feature_size), int(hidden), int(num_layers), int(bool(bidirectional)), merge_id,
                            int(num_classes), float(forget_bias), float(learning_rate), float(beta1),
                            float(beta2), float(epsilon), len(pre), (c_int32 * 3)(*(pre + (0,) * (3 - len(pre)))),
                            int(post), float(relu_clip),
                            (c_float * 4)(*[dropout[i] if i < len(dropout) else 0.0 for i in range(4)]))
        self._open(self.lib.nasr_create, cfg, device_id, stream)

    # ------------------------------------------------------------------ lifetime
    def _open(self, create_fn, cfg, device_id, stream):
        """What the three engine constructors share: the handle for `cfg` from the family's create call."""
        if stream is not None and int(stream) == 0:
            raise ValueError('stream 0 (the legacy default stream) cannot carry the engine: pass a created stream '
                             '(e.g. torch.cuda.Stream().cuda_stream) or None for an engine-owned one')
        self.cfg = cfg
        self.h = c_void_p()
        rc = create_fn(byref(cfg), int(device_id), c_void_p(stream) if stream else None, byref(self.h))
        if rc != 0:
            msg = self.lib.nasr_last_error(None)
            self.h = None
            raise _lib.NasrError(rc, msg.decode() if msg else create_fn.__name__ + ' failed')
        self.num_classes = int(cfg.num_classes)
        self.param_count = int(self.lib.nasr_param_count(self.h))

    def close(self):
        if getattr(self, 'h', None):
            self.lib.nasr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _lib.check(self.lib, self.h, rc)

    @property
    def backend(self):
        return self.lib.nasr_backend(self.h).decode()

    def synchronize(self):
        self._ck(self.lib.nasr_synchronize(self.h))

    # ------------------------------------------------------------------ parameters
    def tensors(self):
        out = []
        for i in range(self.lib.nasr_num_tensors(self.h)):
            name = (c_char * 64)()
            off, r, c = c_int64(), c_int64(), c_int64()
            self._ck(self.lib.nasr_tensor_info(self.h, i, byref(name), byref(off), byref(r), byref(c)))
            out.append((name.value.decode(), off.value, r.value, c.value))
        return out

    def set_params(self, flat):
        flat = _f32(flat).ravel()
        self._ck(self.lib.nasr_set_params(self.h, _fp(flat), flat.size))

    def get_params(self):
        flat = np.empty(self.param_count, np.float32)
        self._ck(self.lib.nasr_get_params(self.h, _fp(flat), flat.size))
        return flat

    def set_adam_state(self, m, v, step):
        m, v = _f32(m).ravel(), _f32(v).ravel()
        self._ck(self.lib.nasr_set_adam_state(self.h, _fp(m), _fp(v), m.size, int(step)))

    def get_adam_state(self):
        m = np.empty(self.param_count, np.float32)
        v = np.empty(self.param_count, np.float32)
        step = c_int64()
        self._ck(self.lib.nasr_get_adam_state(self.h, _fp(m), _fp(v), m.size, byref(step)))
        return m, v, step.value

    def set_learning_rate(self, lr):
        self._ck(self.lib.nasr_set_learning_rate(self.h, float(lr)))

    def learning_rate(self):
        """the step size the next apply_adam() is launched with"""
        v = c_float()
        self._ck(self.lib.nasr_get_learning_rate(self.h, byref(v)))
        return float(v.value)

    # ------------------------------------------------------------------ parameter averaging (include/nasr.h, nasr_set_ema)
    def set_ema(self, decay):
        """An exponential moving average of the parameters, updated inside every applied apply_adam() from here on
        (tf.train.ExponentialMovingAverage's rule with its num_updates ramp): 0 = off, a number in (0,1) = on.  The first
        switch-on starts the average at the parameters as they stand."""
        self._ck(self.lib.nasr_set_ema(self.h, float(decay)))

    def ema(self):
        """(decay, updates, live): 0.0 = averaging is off; the updates applied so far; whether ema_swap() has the average
        in the parameters' place.  Synchronises."""
        decay, updates, live = c_float(), c_int64(), c_int()
        self._ck(self.lib.nasr_get_ema(self.h, byref(decay), byref(updates), byref(live)))
        return float(decay.value), int(updates.value), bool(live.value)

    def get_ema(self):
        """the averaged parameters, flat, in get_params()' order (while the average is live: the training parameters)"""
        flat = np.empty(self.param_count, np.float32)
        self._ck(self.lib.nasr_get_ema_state(self.h, _fp(flat), flat.size, None))
        return flat

    def set_ema_state(self, flat, updates):
        flat = _f32(flat).ravel()
        self._ck(self.lib.nasr_set_ema_state(self.h, _fp(flat), flat.size, int(updates)))

    def ema_swap(self):
        """The parameters and their average change places (the data, on the device; the operand images follow): every
        forward-only call then runs on the average, and the calls that train are refused until the next ema_swap()."""
        self._ck(self.lib.nasr_ema_swap(self.h))

    # ------------------------------------------------------------------ host-buffer entry points
    def _batch(self, feats, seq_len, labels=None, label_len=None):
        """The arrays of a batch as the library takes them.  The library reads B*T*feature_size floats behind a bare
        pointer: features of any other width are refused here, before any call."""
        feats = _f32(feats)
        assert feats.ndim == 3, 'features must be [B,T,F]'
        B, T, F = feats.shape
        if F != self.cfg.feature_size:
            raise ValueError(f'feature size {F} != configured {self.cfg.feature_size}')
        seq = _i32(np.asarray([int(x) for x in seq_len])).ravel()
        assert seq.size == B
        if labels is None:
            return feats, seq, None, None, B, T, 0
        labels = _i32(labels)
        if labels.ndim == 1:
            labels = labels.reshape(B, -1)
        ll = _i32(np.asarray([int(x) for x in label_len])).ravel()
        assert labels.shape[0] == B and ll.size == B
        return feats, seq, labels, ll, B, T, labels.shape[1]

    def logit_frames(self, T):
        """the logit frames of a batch of T input frames (of ceil(T / frame_skip) network frames; 2x for stack_reshape)"""
        return int(self.lib.nasr_logit_frames(self.h, int(T)))

    # ------------------------------------------------------------------ frame skip (include/nasr.h, nasr_set_frame_skip)
    def set_frame_skip(self, frame_skip):
        """Low-frame-rate input: from the next upload on the network sees input frames 0, s, 2s, ... of
        every utterance.  Callers keep passing input frames and input lengths; logits, decoded ids and alignment paths
        come back in network frames (logit_frames, logit_lens).  The library's refusals (outside [1,8], a WaveNet or LAS
        handle, an open stream session) raise with its reason."""
        self._ck(self.lib.nasr_set_frame_skip(self.h, int(frame_skip)))

    @property
    def frame_skip(self):
        s = c_int(1)
        self._ck(self.lib.nasr_get_frame_skip(self.h, byref(s)))
        return int(s.value)

    def logit_lens(self, seq_len):
        """input lengths -> the lengths that go with the logits (int32 [B]): ceil(len / frame_skip) network frames, what
        the beam searches, align_logits and distill_logits take as seq_len.  (stack_reshape's 2T logit frames mix the
        utterances: its decoders take these lengths too, as they always took seq_len.)"""
        return skip_frames(np.asarray([int(x) for x in seq_len]), self.frame_skip).astype(np.int32)

    def forward(self, feats, seq_len):
        feats, seq, _, _, B, T, _ = self._batch(feats, seq_len)
        out = np.empty((self.logit_frames(T), B, self.num_classes), np.float32)
        self._ck(self.lib.nasr_forward(self.h, _fp(feats), _ip(seq), B, T, _fp(out)))
        return out

    def loss(self, feats, seq_len, labels, label_len):
        feats, seq, labels, ll, B, T, Lmax = self._batch(feats, seq_len, labels, label_len)
        loss = c_float()
        nll = np.empty(B, np.float32)
        self._ck(self.lib.nasr_loss(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, Lmax, byref(loss),
                                    _fp(nll)))
        return float(loss.value), nll

    def loss_and_grads(self, feats, seq_len, labels, label_len):
        feats, seq, labels, ll, B, T, Lmax = self._batch(feats, seq_len, labels, label_len)
        loss = c_float()
        nll = np.empty(B, np.float32)
        grads = np.empty(self.param_count, np.float32)
        self._ck(self.lib.nasr_loss_and_grads(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, Lmax,
                                              byref(loss), _fp(nll), _fp(grads)))
        return float(loss.value), nll, grads

    def train_step(self, feats, seq_len, labels, label_len):
        feats, seq, labels, ll, B, T, Lmax = self._batch(feats, seq_len, labels, label_len)
        loss = c_float()
        self._ck(self.lib.nasr_train_step(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, Lmax, byref(loss)))
        return float(loss.value)

    def greedy_decode(self, feats, seq_len):
        feats, seq, _, _, B, T, _ = self._batch(feats, seq_len)
        Tp = self.logit_frames(T)
        ids = np.zeros((B, Tp), np.int32)
        lens = np.zeros(B, np.int32)
        self._ck(self.lib.nasr_greedy_decode(self.h, _fp(feats), _ip(seq), B, T, _ip(ids), _ip(lens)))
        return [ids[b, :lens[b]].tolist() for b in range(B)]

    # ------------------------------------------------------------------ resident-batch / data-parallel pieces
    def upload_batch(self, feats, seq_len, labels, label_len):
        feats, seq, labels, ll, B, T, Lmax = self._batch(feats, seq_len, labels, label_len)
        self._ck(self.lib.nasr_upload_batch(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, Lmax))

    @staticmethod
    def context_structure_ok(feats, seq, numcontext, numcep):
        """True when feats [B,T,(2*numcontext+1)*numcep] is what include_context (utils.py:8-21) + one constant pad value
        per utterance produce, so that the centre slice + the pad value determine it.  The first / last numcontext frames
        of EVERY utterance are checked exactly: that is where an array that went through rand_shift's roll-and-crop
        (dataset.py:23-31) differs (real neighbours instead of the pad value, and a pad read from a real sample); the
        interior is spot-checked.  `numcep` is the width of one un-stacked frame: config.frame_width, the static columns
        and their deltas."""
        B = feats.shape[0]
        w = 2 * numcontext + 1
        if numcontext < 1 or feats.shape[2] != w * numcep:
            return False
        pad = feats[:, 0, 0]
        c0 = numcontext * numcep
        rs = np.random.RandomState(0)
        for b in range(B):
            n = int(seq[b])
            edge = sorted(set(range(min(numcontext, n))) | set(range(max(0, n - numcontext), n)))
            t = np.asarray(edge + [rs.randint(n) for _ in range(4)], dtype=np.int64)
            src = t[:, None] + np.arange(w) - numcontext                      # [E, w]: source frame of each slot
            inside = (src >= 0) & (src < n)
            want = np.where(inside[:, :, None], feats[b, np.clip(src, 0, n - 1), c0:c0 + numcep], pad[b])
            if not np.array_equal(feats[b, t].reshape(len(t), w, numcep), want):
                return False
        return True

    @classmethod
    def _centre_form(cls, feats, seq, numcontext, numcep, bare=False):
        """(centre frames [B,T,numcep], pad value [B]) that determine the stacked feats, or None when they do not have
        include_context's structure (context_structure_ok); bare: un-stacked frames, taken as they are"""
        if not bare and not cls.context_structure_ok(feats, seq, numcontext, numcep):
            return None
        return (np.ascontiguousarray(feats[:, :, numcontext * numcep:(numcontext + 1) * numcep]),
                np.ascontiguousarray(feats[:, 0, 0]))

    def _with_aug(self, name, aug, B, wave=None):
        """(entry point, its arguments behind the plain ones, what those point into - to be kept alive over the call):
        `name` itself without masks, its _aug sibling with the BatchAug's struct with them, its _wave sibling with a
        WaveAug (an audio call's waveform augmentation) as well"""
        if aug is None and wave is None:
            return getattr(self.lib, name), (), None
        st, keep = aug.struct(B) if aug is not None else (None, None)
        if wave is None:
            return getattr(self.lib, name + '_aug'), (byref(st),), (st, keep)
        wst, wkeep = wave.struct(B)
        return getattr(self.lib, name + '_wave'), (None if st is None else byref(st), byref(wst)), (st, keep, wst, wkeep)

    def _ticket(self, rc, ticket):
        """What a stage call returns: its ticket, or None when no staging slot was free; any other failure raises"""
        if rc == _lib.NASR_ERR_STATE and ticket.value < 0:
            msg = self.lib.nasr_last_error(self.h)
            if msg and b'no free batch slot' in msg:
                return None
        self._ck(rc)
        return int(ticket.value)

    def upload_batch_context(self, feats, seq_len, labels, label_len, numcontext, numcep, aug=None):
        """Upload context-stacked features [B,T,(2*numcontext+1)*numcep] as their centre slice and rebuild the
        stacking on the device (include_context, utils.py:8-21).  Returns False (nothing uploaded) when the
        array does not have that structure (e.g. rand_shift cropped it), so the caller can upload it whole.
        `aug` (BatchAug): the kernel that stacks masks the centre frames first (nasr_upload_batch_context_aug)."""
        feats, seq, labels, ll, B, T, Lmax = self._batch(feats, seq_len, labels, label_len)
        bare = aug is not None and numcontext == 0 and feats.shape[2] == numcep      # un-stacked frames: masked as they are
        form = self._centre_form(feats, seq, numcontext, numcep, bare)
        if form is None:
            return False
        fn, tail, keep = self._with_aug('nasr_upload_batch_context', aug, B)
        self._ck(fn(self.h, _fp(form[0]), _fp(form[1]), int(numcontext), int(numcep), _ip(seq), _ip(labels), _ip(ll), B, T,
                    Lmax, *tail))
        return True

    def stage_batch(self, feats, seq_len, labels, label_len, numcontext=0, numcep=0):
        """Copy the NEXT batch towards the GPU while the current step runs (pinned staging + the handle's copy stream,
        include/nasr.h nasr_stage_batch); may be called from a loader thread.  With numcontext > 0 and features that have
        include_context's structure only the centre slice crosses PCIe.  Returns a ticket for commit_batch(), or None
        when no staging slot is free (upload the batch the synchronous way then)."""
        feats, seq, labels, ll, B, T, Lmax = self._batch(feats, seq_len, labels, label_len)
        ticket = c_int(-1)
        form = self._centre_form(feats, seq, numcontext, numcep)
        if form is not None:
            rc = self.lib.nasr_stage_batch_context(self.h, _fp(form[0]), _fp(form[1]), int(numcontext), int(numcep),
                                                   _ip(seq), _ip(labels), _ip(ll), B, T, Lmax, byref(ticket))
        else:
            rc = self.lib.nasr_stage_batch(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, Lmax, byref(ticket))
        return self._ticket(rc, ticket)

    # ------------------------------------------------------------------ batches straight from audio (nasr_upload_batch_audio)
    @staticmethod
    def _audio(audios, labels, label_len, rates):
        audios = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in audios]
        B = len(audios)
        offsets = np.zeros(B + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([a.size for a in audios])
        flat = np.concatenate(audios) if B > 1 else (audios[0] if B else np.zeros(1, np.float32))
        r = None if rates is None else _i32(np.asarray([int(x) for x in rates])).ravel()
        if r is not None and r.size != B:
            raise ValueError('%d rates for %d utterances' % (r.size, B))
        Lmax = 0
        if labels is not None:
            labels = _i32(labels)
            labels = labels.reshape(B, -1) if B else labels
            label_len = _i32(np.asarray([int(x) for x in label_len])).ravel()
            assert label_len.size == B
            Lmax = labels.shape[1] if B else 0
        else:
            label_len = None
        return flat, offsets, r, labels, label_len, B, Lmax

    def _audio_call(self, fn, featurizer, audios, labels, label_len, rates, *tail):
        flat, offsets, r, labels, ll, B, Lmax = self._audio(audios, labels, label_len, rates)
        seq = np.zeros(max(B, 1), np.int32)
        T = c_int(0)
        fz = getattr(featurizer, 'h', featurizer)
        rc = fn(self.h, fz, _fp(flat), offsets.ctypes.data_as(POINTER(c_int64)), _ip(r), _ip(labels), _ip(ll), B, Lmax,
                _ip(seq), byref(T), *tail)
        return rc, seq[:B], int(T.value)

    def upload_batch_audio(self, featurizer, audios, labels, label_len, rates=None, aug=None, wave=None):
        """A batch from audio: `featurizer` (features.Featurizer, same device) makes the MFCC features of the float32
        utterances `audios` (at `rates` Hz, None: all at its samplerate) on the device and writes them into this handle's
        batch slot; the batch is resident afterwards, as after upload_batch.  Returns (seq_len int32 [B], T).
        `aug` (BatchAug): SpecAugment masks on the normalised frames (nasr_upload_batch_audio_aug).  `wave` (WaveAug):
        reverberation and noise from the featurizer's banks on the samples, before the features are made
        (nasr_upload_batch_audio_wave)."""
        fn, tail, keep = self._with_aug('nasr_upload_batch_audio', aug, len(audios), wave)
        rc, seq, T = self._audio_call(fn, featurizer, audios, labels, label_len, rates, *tail)
        self._ck(rc)
        return seq, T

    def stage_batch_audio(self, featurizer, audios, labels, label_len, rates=None, aug=None, wave=None):
        """upload_batch_audio's staging half (stage_batch): copies and front-end kernels on the copy stream while the
        current step runs.  Returns (seq_len, T, ticket); ticket is None when no staging slot is free."""
        ticket = c_int(-1)
        fn, tail, keep = self._with_aug('nasr_stage_batch_audio', aug, len(audios), wave)
        rc, seq, T = self._audio_call(fn, featurizer, audios, labels, label_len, rates, *tail, byref(ticket))
        return seq, T, self._ticket(rc, ticket)

    def forward_resident(self, B, T, fetch=True):
        """logits [T',B,C] of the resident batch (forward() without its upload); fetch=False: the pass alone, they stay on
        the device (take_teacher_logits() reads them there) and None is returned"""
        if not fetch:
            self._ck(self.lib.nasr_forward_resident(self.h, None))
            return None
        out = np.empty((self.logit_frames(T), B, self.num_classes), np.float32)
        self._ck(self.lib.nasr_forward_resident(self.h, _fp(out)))
        return out

    def loss_resident(self, B):
        """(loss, nll [B]) of the resident batch (loss() without its upload; inference-mode pass)"""
        loss = c_float()
        nll = np.empty(B, np.float32)
        self._ck(self.lib.nasr_loss_resident(self.h, byref(loss), _fp(nll)))
        return float(loss.value), nll

    def greedy_decode_resident(self, B, T):
        Tp = self.logit_frames(T)
        ids = np.zeros((B, Tp), np.int32)
        lens = np.zeros(B, np.int32)
        self._ck(self.lib.nasr_greedy_decode_resident(self.h, _ip(ids), _ip(lens)))
        return [ids[b, :lens[b]].tolist() for b in range(B)]

    # ------------------------------------------------------------------ forced alignment
    def align(self, feats, seq_len, labels, label_len):
        """(path int32 [B,T'], score float64 [B]): every utterance's best path through the CTC lattice of its label -
        path[b][t] is the state of the extended label at logit frame t (-1 from seq_len[b] on), score[b] the path's
        log-probability.  Upload, forward and alignment, all on the device."""
        feats, seq, labels, ll, B, T, Lmax = self._batch(feats, seq_len, labels, label_len)
        path = np.empty((B, self.logit_frames(T)), np.int32)
        score = np.empty(B, np.float64)
        self._ck(self.lib.nasr_ctc_align(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, Lmax, _ip(path),
                                         score.ctypes.data_as(POINTER(c_double))))
        return path, score

    def align_resident(self, B, T):
        """align() on the resident batch and its labels (whichever upload put them there); B and T must be that batch's"""
        rb, rt = ctypes.c_int(), ctypes.c_int()
        self._ck(self.lib.nasr_resident_shape(self.h, byref(rb), byref(rt)))
        if (rb.value, rt.value) != (int(B), int(T)):
            raise ValueError('align_resident(B=%d, T=%d): the resident batch has B=%d, T=%d' % (B, T, rb.value, rt.value))
        path = np.empty((B, self.logit_frames(T)), np.int32)
        score = np.empty(B, np.float64)
        self._ck(self.lib.nasr_ctc_align_resident(self.h, _ip(path), score.ctypes.data_as(POINTER(c_double))))
        return path, score

    def align_logits(self, logits_tm, seq_len, labels, label_len):
        """The alignment kernels on the caller's logits, time-major [T',B,C] (blank = C-1; seq_len in logit frames),
        whatever this engine's model is; the resident batch is not touched."""
        logits = _f32(logits_tm)
        assert logits.ndim == 3, 'logits must be [T\',B,C]'
        Tp, B, C = logits.shape
        seq = _i32(np.asarray([int(x) for x in seq_len])).ravel()
        ll = _i32(np.asarray([int(x) for x in label_len])).ravel()
        labels = _i32(labels).reshape(B, -1)
        assert seq.size == B and ll.size == B
        path = np.empty((B, Tp), np.int32)
        score = np.empty(B, np.float64)
        self._ck(self.lib.nasr_ctc_align_logits(self.h, _fp(logits), _ip(seq), _ip(labels), _ip(ll), B, Tp, C,
                                                labels.shape[1], _ip(path), score.ctypes.data_as(POINTER(c_double))))
        return path, score

    def align_in_lds(self, F, L):
        """True when a batch with F frames and labels up to L ids keeps its back-pointers in LDS (else: global workspace)"""
        rc = int(self.lib.nasr_ctc_align_lds(int(F), int(L)))
        if rc < 0:
            raise ValueError('align_in_lds: F >= 1 and 0 <= L <= 511')
        return bool(rc)

    def commit_batch(self, ticket):
        self._ck(self.lib.nasr_commit_batch(self.h, int(ticket)))

    def discard_batch(self, ticket):
        self._ck(self.lib.nasr_discard_batch(self.h, int(ticket)))

    def compute_grads(self):
        self._ck(self.lib.nasr_compute_grads(self.h))

    def apply_adam(self, grad_scale=1.0):
        self._ck(self.lib.nasr_apply_adam(self.h, float(grad_scale)))

    def set_grad_clip(self, max_norm):
        """Global-norm clipping of every apply_adam() from here on (include/nasr.h, nasr_set_grad_clip): 0 = off, a positive
        number = tf.clip_by_global_norm's threshold, inf = measure the norm and skip non-finite gradients, never scale."""
        self._ck(self.lib.nasr_set_grad_clip(self.h, float(max_norm)))

    def set_chunking(self, chunk_frames, lookahead=0):
        """Latency-controlled training (include/nasr.h, nasr_set_chunking): from here on every whole-batch pass
        (forward, loss, gradients, train_step, greedy decode, alignment) runs each utterance as the windows of a look-ahead
        session fed chunk_frames + lookahead rows, then chunk_frames per feed.  chunk_frames = 0: off.  The library's
        refusals (unidirectional, stack_reshape, dense stages, dropout, an open stream session) raise with its reason."""
        self._ck(self.lib.nasr_set_chunking(self.h, int(chunk_frames), int(lookahead)))

    @property
    def chunking(self):
        """(chunk_frames, lookahead) as set_chunking() set them; (0, 0) = off"""
        c, r = c_int(), c_int()
        self._ck(self.lib.nasr_get_chunking(self.h, byref(c), byref(r)))
        return int(c.value), int(r.value)

    # ------------------------------------------------------------------ distillation
    def set_distill(self, weight, temperature=1.0):
        """Teacher-student distillation beside the CTC loss (include/nasr.h, nasr_set_distill): loss = (1 - weight) CTC +
        weight KD against the teacher logits of the resident batch.  weight = 0: off, the step of an engine that never
        heard of it.  The library's refusals (LAS, stack_reshape, values out of range) raise with its reason."""
        self._ck(self.lib.nasr_set_distill(self.h, float(weight), float(temperature)))

    @property
    def distill(self):
        """(weight, temperature) as set_distill() set them; weight 0.0 = off"""
        w, t = c_float(), c_float()
        self._ck(self.lib.nasr_get_distill(self.h, byref(w), byref(t)))
        return float(w.value), float(t.value)

    def set_teacher_logits(self, logits_tm):
        """teacher logits [T',B,C] (as forward() returns them) for the resident batch; the next upload drops them"""
        logits = _f32(logits_tm)
        rb, rt = ctypes.c_int(), ctypes.c_int()
        self._ck(self.lib.nasr_resident_shape(self.h, byref(rb), byref(rt)))
        if rb.value and logits.shape != (self.logit_frames(rt.value), rb.value, self.num_classes):
            raise ValueError('set_teacher_logits: logits %s, the resident batch needs %s'
                             % (logits.shape, (self.logit_frames(rt.value), rb.value, self.num_classes)))
        self._ck(self.lib.nasr_set_teacher_logits(self.h, _fp(logits)))

    def take_teacher_logits(self, teacher):
        """the same from `teacher`'s last forward pass on its own resident batch, device to device, no host wait"""
        self._ck(self.lib.nasr_take_teacher_logits(self.h, teacher.h))

    def distill_loss(self):
        """(ctc, kd) of the last loss pass: the batch-mean CTC loss and the distillation term (0.0 when it took no part)"""
        c, k = c_float(), c_float()
        self._ck(self.lib.nasr_get_distill_loss(self.h, byref(c), byref(k)))
        return float(c.value), float(k.value)

    def distill_logits(self, student_tm, teacher_tm, seq_len, weight, temperature, out=None, kd_out=None):
        """The term's kernels on the caller's logits [T',B,C] (C = this engine's num_classes; seq_len in logit frames):
        (weight * temperature * (q - p) / B as [T',B,C] float32, kd_b as [B] float64).  out / kd_out: arrays to write into
        (C-contiguous, at least that large).  The engine's state is untouched."""
        z, y = _f32(student_tm), _f32(teacher_tm)
        assert z.ndim == 3 and z.shape == y.shape and z.shape[2] == self.num_classes, 'logits must be [T\',B,num_classes]'
        Tp, B, _ = z.shape
        seq = _i32(np.asarray([int(x) for x in seq_len])).ravel()
        assert seq.size == B
        d = np.empty(z.shape, np.float32) if out is None else out
        kd = np.empty(B, np.float64) if kd_out is None else kd_out
        assert d.dtype == np.float32 and d.flags.c_contiguous and d.size >= z.size
        assert kd.dtype == np.float64 and kd.flags.c_contiguous and kd.size >= B
        self._ck(self.lib.nasr_distill_logits(self.h, _fp(z), _fp(y), _ip(seq), B, Tp, float(weight), float(temperature),
                                              _fp(d), kd.ctypes.data_as(POINTER(c_double))))
        return d, kd

    @property
    def grad_clip(self):
        """the threshold set_grad_clip() set; 0.0 = clipping is off"""
        v = c_float()
        self._ck(self.lib.nasr_get_grad_clip(self.h, byref(v)))
        return float(v.value)

    def grad_clip_stats(self, reset=False):
        """dict of last_norm, window_max_norm, last_coef, steps, clipped, skipped (nasr_clip_stats); synchronises.
        reset=True clears the window (its largest norm and the three counters) behind the read."""
        st = _lib.ClipStats()
        self._ck(self.lib.nasr_get_grad_clip_stats(self.h, byref(st), int(bool(reset))))
        return st.as_dict()

    def get_grads(self):
        g = np.empty(self.param_count, np.float32)
        self._ck(self.lib.nasr_get_grads(self.h, _fp(g), g.size))
        return g

    def set_grads(self, flat):
        flat = _f32(flat).ravel()
        self._ck(self.lib.nasr_set_grads(self.h, _fp(flat), flat.size))

    def label_error_rate(self, hyps, labels, label_len):
        """mean over the batch of edit_distance(hyp, truth)/len(truth) (networks/tfnetwork.py:66-70)."""
        B = len(hyps)
        stride = max(1, max((len(h) for h in hyps), default=1))
        ids = np.zeros((B, stride), np.int32)
        lens = np.zeros(B, np.int32)
        for b, hy in enumerate(hyps):
            lens[b] = len(hy)
            ids[b, :len(hy)] = hy
        labels = _i32(labels).reshape(B, -1)
        ll = _i32(np.asarray([int(x) for x in label_len]))
        out = c_float()
        rc = self.lib.nasr_label_error_rate(_ip(ids), _ip(lens), stride, _ip(labels), _ip(ll), labels.shape[1], B,
                                            byref(out))
        if rc != 0:
            raise _lib.NasrError(rc, 'nasr_label_error_rate: bad arguments')
        return float(out.value)

    def set_step_decode(self, on, logits=False, greedy=True):
        """Per step: loss + greedy decode copied out behind the CTC kernels (on), with logits=True the logits themselves too,
        with greedy=False (and logits) those without the greedy decode (include/nasr.h: nasr_set_step_decode)."""
        mode = 0 if not on else ((1 if greedy or not logits else 0) | (2 if logits else 0))
        self._ck(self.lib.nasr_set_step_decode(self.h, mode))

    def step_logits(self, B, T):
        """[T',B,C] logits of the step just enqueued, as soon as its forward pass + CTC are done (the backward pass runs on)."""
        out = np.empty((self.logit_frames(T), B, self.num_classes), np.float32)
        self._ck(self.lib.nasr_get_step_logits(self.h, _fp(out)))
        return out

    def get_decoded(self, B, T):
        Tp = self.logit_frames(T)
        ids = np.zeros((B, Tp), np.int32)
        lens = np.zeros(B, np.int32)
        self._ck(self.lib.nasr_get_decoded(self.h, _ip(ids), _ip(lens)))
        return [ids[b, :lens[b]].tolist() for b in range(B)]

    def beam_search(self, logits_tm, seq_len, beam_width=100, merge_repeated=True, lm=None, lm_weight=0.0, lm_bonus=0.0):
        """tf.nn.ctc_beam_search_decoder defaults (networks/tfnetwork.py:61-64) on host logits [T',B,C].
        Returns (list of id lists, log-probabilities [B]).  lm (lm.NGramLM): the search fused with that model
        (include/nasr.h: nasr_ctc_beam_search_lm); the log-probabilities are then the fused scores."""
        lg = _f32(logits_tm)
        Tp, B, C = lg.shape
        seq = _i32(np.asarray([int(x) for x in seq_len]))
        ids = np.zeros((B, Tp), np.int32)
        lens = np.zeros(B, np.int32)
        logp = np.zeros(B, np.float32)
        fn = 'nasr_ctc_beam_search' if lm is None else 'nasr_ctc_beam_search_lm'
        if lm is not None:
            if lm.num_classes != C:
                raise ValueError(f'the language model has num_classes {lm.num_classes} but the logits have {C} classes')
            rc = self.lib.nasr_ctc_beam_search_lm(_fp(lg), _ip(seq), B, Tp, C, int(beam_width), int(bool(merge_repeated)),
                                                  _fp(lm.logp), _fp(lm.eos), lm.order, lm.bos_id, float(lm_weight),
                                                  float(lm_bonus), _ip(ids), _ip(lens), _fp(logp))
        else:
            rc = self.lib.nasr_ctc_beam_search(_fp(lg), _ip(seq), B, Tp, C, int(beam_width), int(bool(merge_repeated)),
                                               _ip(ids), _ip(lens), _fp(logp))
        if rc != 0:
            raise _lib.NasrError(rc, fn + ': bad arguments')
        return [ids[b, :lens[b]].tolist() for b in range(B)], logp

    # ------------------------------------------------------------------ streaming (nasr_stream_*)
    def stream_open(self, slots=1):
        """Open the stream session: `slots` concurrent streams, each layer's (c, h) per slot kept on the device between
        feeds.  Raises the library's message for a network that cannot stream."""
        self._ck(self.lib.nasr_stream_open(self.h, int(slots)))
        self._stream_slots = int(slots)

    def stream_close(self):
        self._ck(self.lib.nasr_stream_close(self.h))

    def stream_reset(self, slots=None):
        """A new utterance starts in `slots` (None: in every slot): state and frame count zero."""
        if slots is None:
            self._ck(self.lib.nasr_stream_reset(self.h, None, 0))
        else:
            sl = _i32(np.asarray([int(x) for x in slots])).ravel()
            self._ck(self.lib.nasr_stream_reset(self.h, _ip(sl), sl.size))

    def stream_feed(self, feats, n_frames):
        """One chunk: feats [S,Tc,F], n_frames [S] in [0,Tc] (0: the slot is idle).  Returns the logits [Tc,S,C]; rows
        t >= n_frames[b] of slot b are unspecified.  Under a frame skip s the chunk's kept rows run: logits
        [ceil(Tc/s),S,C], of which slot b's first stream_keep(phase_b, n_frames[b], s)[1] are its new rows."""
        feats, n, _, _, S, Tc, _ = self._batch(feats, n_frames)
        out = np.empty((skip_frames(Tc, self.frame_skip), S, self.num_classes), np.float32)
        self._ck(self.lib.nasr_stream_feed(self.h, _fp(feats), _ip(n), Tc, _fp(out)))
        return out

    # ---- a session that takes samples
    def stream_attach_audio(self, featurizer):
        """The open session takes SAMPLES from now on: `featurizer` (features.Featurizer with normalization='causal', same
        device) turns them into the chunks' rows on the device.  It must stay open as long as the session."""
        self._ck(self.lib.nasr_stream_attach_audio(self.h, getattr(featurizer, 'h', featurizer)))
        self._stream_featurizer = featurizer
        self._stream_max_samples = int(getattr(featurizer, 'max_samples', 1 << 23))

    def _stream_slots_and_last(self, per_slot, last):
        """(S, the `last` flags as the library takes them, or None): per_slot and last must have one entry per slot"""
        S = getattr(self, '_stream_slots', 0)
        if len(per_slot) != S:
            raise ValueError('%d entries for %d slots' % (len(per_slot), S))
        if last is None:
            return S, None
        fin = np.ascontiguousarray([1 if x else 0 for x in last], dtype=np.uint8)
        if fin.size != S:
            raise ValueError('%d `last` flags for %d slots' % (fin.size, S))
        return S, fin.ctypes.data_as(POINTER(c_uint8))

    def _stream_rows_then_feed(self, rows_fn, n, last, feed=None):
        """The library's `rows_fn` on n (an int array, one count per slot): (rows int32 [S], the most of them), host only.
        With `feed`, the feed those rows size: feed(last, rows out, most out, logits out, its rows) fills logits
        [most,S,C] and must report what rows_fn said; (logits, rows) then."""
        S, fin_p = self._stream_slots_and_last(n, last)
        rows, most = np.zeros(S, np.int32), c_int(0)
        self._ck(rows_fn(self.h, n.ctypes.data_as(POINTER(np.ctypeslib.as_ctypes_type(n.dtype))), fin_p, _ip(rows), byref(most)))
        if feed is None:
            return rows, int(most.value)
        out = np.empty((most.value, S, self.num_classes), np.float32)
        got, most2 = np.zeros(S, np.int32), c_int(0)
        self._ck(feed(fin_p, _ip(got), byref(most2), _fp(out) if out.size else None, most.value))
        assert most2.value == most.value and np.array_equal(got, rows)
        return out, got

    def stream_audio_rows(self, n_samples, last=None):
        """(rows int32 [S], Tc): what a stream_feed_audio of n_samples[b] new samples per slot would emit now (host only)."""
        return self._stream_rows_then_feed(self.lib.nasr_stream_audio_rows, np.asarray([int(x) for x in n_samples], np.int64), last)

    def stream_feed_audio(self, chunks, last=None):
        """One feed of samples: chunks[b] float32 [n_b] at the featurizer's rate, or None / empty (slot b is idle, or only
        finishing); last[b] true declares slot b's utterance complete.  Returns (logits [Tc,S,C], rows int32 [S]): slot b's
        rows_b new rows are logits[:rows_b, b]; Tc = 0 when the feed emitted nothing.  At most the featurizer's
        max_samples per feed."""
        S, _ = self._stream_slots_and_last(chunks, last)
        arrs = [np.zeros(0, np.float32) if c is None else np.ascontiguousarray(c, dtype=np.float32).reshape(-1) for c in chunks]
        offsets = np.zeros(S + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([a.size for a in arrs])
        most = getattr(self, '_stream_max_samples', 1 << 23)
        if offsets[S] > most:
            raise ValueError('%d samples in one feed: the featurizer takes at most max_samples = %d' % (offsets[S], most))
        flat = np.concatenate(arrs) if offsets[S] else np.zeros(1, np.float32)
        return self._stream_rows_then_feed(
            self.lib.nasr_stream_audio_rows, np.diff(offsets), last,
            lambda fin_p, got, Tc2, out, Tc: self.lib.nasr_stream_feed_audio(
                self.h, _fp(flat), offsets.ctypes.data_as(POINTER(c_int64)), fin_p, got, Tc2, out, Tc))

    # ---- a look-ahead session on a bidirectional network
    def stream_open_lookahead(self, slots=1, lookahead=1):
        """Open a look-ahead session: `slots` concurrent streams on a bidirectional (concat) network, the forward
        direction's (c, h) carried, the backward direction restarted in every feed `lookahead` frames to the right of the
        rows the feed emits.  Raises the library's message for a network that cannot stream this way."""
        self._ck(self.lib.nasr_stream_open_lookahead(self.h, int(slots), int(lookahead)))
        self._stream_slots = int(slots)

    def stream_lookahead_rows(self, n_frames, last=None):
        """(rows int32 [S], Te): what a stream_feed_lookahead of n_frames[b] new rows per slot would emit now (host only)."""
        return self._stream_rows_then_feed(self.lib.nasr_stream_lookahead_rows, _i32(np.asarray([int(x) for x in n_frames])).ravel(), last)

    def stream_feed_lookahead(self, feats, n_frames, last=None):
        """One feed: feats [S,Tc,F] (Tc may be 0), n_frames [S] in [0,Tc], last[b] true declares slot b's utterance
        complete.  Returns (logits [Te,S,C], rows int32 [S]): slot b's rows_b emitted rows are logits[:rows_b, b]; Te = 0
        when the feed emitted nothing."""
        S, _ = self._stream_slots_and_last(n_frames, last)
        feats = _f32(feats)
        F = int(self.cfg.feature_size)
        if feats.ndim != 3 or feats.shape[0] != S or feats.shape[2] != F:
            raise ValueError('feats must be [%d, Tc, %d], not %s' % (S, F, feats.shape))
        n = _i32(np.asarray([int(x) for x in n_frames])).ravel()
        # (the library refuses negative counts too; here they must not size the output array first)
        return self._stream_rows_then_feed(
            self.lib.nasr_stream_lookahead_rows, np.clip(n, 0, None), last,
            lambda fin_p, got, Te2, out, Te: self.lib.nasr_stream_feed_lookahead(
                self.h, _fp(feats) if feats.size else None, _ip(n), fin_p, int(feats.shape[1]), got, Te2, out, Te))

    def stream_frames(self):
        out = np.zeros(getattr(self, '_stream_slots', 0), np.int64)
        self._ck(self.lib.nasr_stream_frames(self.h, out.ctypes.data_as(POINTER(c_int64))))
        return out

    def stream_state(self):
        """The session's state [L,S,2,H] float32: per layer and slot the cell's c, then its h."""
        out = np.empty((int(self.cfg.num_layers), getattr(self, '_stream_slots', 0), 2, int(self.cfg.hidden)), np.float32)
        self._ck(self.lib.nasr_stream_get_state(self.h, _fp(out), out.size))
        return out

    def set_stream_state(self, state):
        state = _f32(state)
        self._ck(self.lib.nasr_stream_set_state(self.h, _fp(state), state.size))

    def get_loss(self):
        loss = c_float()
        self._ck(self.lib.nasr_get_loss(self.h, byref(loss)))
        return float(loss.value)

    def step_void(self):
        """True when the step just applied was void on every rank (some rank's persistent recurrence aborted; Adam was
        a no-op everywhere): run it again.  Synchronises."""
        from ctypes import c_int
        v = c_int()
        self._ck(self.lib.nasr_step_void(self.h, byref(v)))
        return bool(v.value)

    def step_results(self, B, T):
        """(loss, forward_fault, hypotheses) of the step just enqueued, as soon as its forward pass + CTC are done - the
        backward pass, the exchange and Adam keep running (include/nasr.h, nasr_get_step_results)."""
        from ctypes import c_int
        Tp = self.logit_frames(T)
        ids = np.zeros((B, Tp), np.int32)
        lens = np.zeros(B, np.int32)
        loss, fault = c_float(), c_int()
        self._ck(self.lib.nasr_get_step_results(self.h, byref(loss), byref(fault), _ip(ids), _ip(lens)))
        return float(loss.value), bool(fault.value), [ids[b, :lens[b]].tolist() for b in range(B)]

    def settle_step(self, previous=False):
        """True when the latest (or, previous=True, the one-before-latest) optimiser step was void on every rank."""
        from ctypes import c_int
        v = c_int()
        self._ck(self.lib.nasr_settle_step(self.h, int(bool(previous)), byref(v)))
        return bool(v.value)

    @property
    def wgrad_overlap(self):
        """True when the upper layers' weight gradients run beside the persistent BPTT launch of the layer below."""
        return bool(self.lib.nasr_get_wgrad_overlap(self.h))

    def set_wgrad_overlap(self, on):
        self._ck(self.lib.nasr_set_wgrad_overlap(self.h, int(bool(on))))

    def diag_bucket_traffic(self, i, stream, nblocks, passes):
        """Diagnostics: a ring-all-reduce-shaped kernel over bucket i on `stream`, behind the bucket's event (include/nasr.h)."""
        from ctypes import c_void_p
        self._ck(self.lib.nasr_diag_bucket_traffic(self.h, int(i), c_void_p(int(stream)), int(nblocks), int(passes)))

    def step_token(self):
        """Sequence number of the optimiser step apply_adam() enqueued last (include/nasr.h, nasr_step_token)."""
        return int(self.lib.nasr_step_token(self.h))

    def settle_token(self, token):
        """True when optimiser step `token` was void on every rank; waits for the end of exactly that step."""
        from ctypes import c_int
        v = c_int()
        self._ck(self.lib.nasr_settle_token(self.h, int(token), byref(v)))
        return bool(v.value)

    def resident_frames(self):
        n = c_int64()
        self._ck(self.lib.nasr_resident_frames(self.h, byref(n)))
        return n.value

    def resident_rows(self):
        """Rows the operand passes and GEMMs cover for the resident batch: sum(seq_len) when the ragged batch was compacted
        (nasr.h: nasr_set_row_compaction), T x padded B otherwise."""
        n = c_int64()
        self._ck(self.lib.nasr_resident_rows(self.h, byref(n)))
        return n.value

    def set_row_compaction(self, on):
        self._ck(self.lib.nasr_set_row_compaction(self.h, int(bool(on))))

    def grad_device_ptr(self):
        return int(self.lib.nasr_grad_device_ptr(self.h)), int(self.lib.nasr_grad_device_count(self.h))

    def grad_tensor(self):
        """The flat device gradient buffer as a torch tensor ALIAS (no copy), for torch.distributed
        all-reduce over RCCL.  torch is plumbing here: it only wraps the pointer."""
        import torch
        ptr, n = self.grad_device_ptr()

        class _Ext:
            __cuda_array_interface__ = {'shape': (n,), 'typestr': '<f4', 'data': (ptr, False), 'version': 3,
                                        'strides': None}
        return torch.as_tensor(_Ext(), device='cuda')

    def grad_buckets(self):
        """[(offset, count)] in floats from grad_device_ptr(): contiguous pieces of the gradient buffer in the order
        compute_grads() completes them (include/nasr.h, "Overlapping the exchange")."""
        out = []
        n = self.lib.nasr_grad_bucket_count(self.h)
        if n < 0:
            self._ck(n)
        for i in range(n):
            o, c = c_int64(), c_int64()
            self._ck(self.lib.nasr_grad_bucket(self.h, i, byref(o), byref(c)))
            out.append((int(o.value), int(c.value)))
        return out

    # ------------------------------------------------------------------ in-library RCCL exchange (include/nasr.h nasr_comm_*)
    def comm_unique_id(self):
        """128 bytes from ncclGetUniqueId (rank 0 calls this and hands them to the other ranks)."""
        buf = ctypes.create_string_buffer(128)
        rc = self.lib.nasr_comm_unique_id(buf)
        if rc != 0:
            msg = self.lib.nasr_last_error(None)
            raise _lib.NasrError(rc, msg.decode() if msg else 'nasr_comm_unique_id failed')
        return buf.raw

    def comm_init(self, unique_id, rank, nranks):
        assert len(unique_id) == 128
        self._ck(self.lib.nasr_comm_init(self.h, ctypes.c_char_p(bytes(unique_id)), int(rank), int(nranks)))

    def comm_size(self):
        return int(self.lib.nasr_comm_size(self.h))

    def comm_allreduce_grads(self):
        self._ck(self.lib.nasr_comm_allreduce_grads(self.h))

    def comm_mean(self, values):
        v = np.ascontiguousarray(values, np.float32).copy()
        self._ck(self.lib.nasr_comm_mean(self.h, _fp(v), v.size))
        return v.tolist()

    def comm_destroy(self):
        self._ck(self.lib.nasr_comm_destroy(self.h))

    def set_bucket_defer(self, on):
        """Hold each gradient bucket's event back over the next persistent BPTT launch (include/nasr.h)."""
        self._ck(self.lib.nasr_set_bucket_defer(self.h, int(bool(on))))

    def bucket_wait(self, i, stream):
        """Makes HIP stream `stream` (raw handle) wait until the compute_grads() issued before has completed bucket i."""
        self._ck(self.lib.nasr_grad_bucket_wait(self.h, int(i), c_void_p(int(stream))))

    # ------------------------------------------------------------------ measurement
    def set_profiling(self, on):
        self._ck(self.lib.nasr_set_profiling(self.h, int(bool(on))))

    def set_graph_mode(self, on):
        self._ck(self.lib.nasr_set_graph_mode(self.h, int(bool(on))))

    def set_dropout_state(self, seed, counter):
        """Pins the keep-masks of the dense stages: forward pass number `counter` of stream `seed` (every forward pass
        uses the current counter, then increments it)."""
        self._ck(self.lib.nasr_set_dropout_state(self.h, int(seed) & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF))

    def dropout_state(self):
        s, c = c_uint32(), c_uint32()
        self._ck(self.lib.nasr_get_dropout_state(self.h, byref(s), byref(c)))
        return int(s.value), int(c.value)

    @property
    def recurrence_mode(self):
        """'persistent' (one launch per layer pass, lstm_persist.hip), 'wide-persistent' (Hp = 2048: one persistent launch per
        direction and pass, lstm_wide.hip) or 'per-step' (lstm.hip)."""
        m = int(self.lib.nasr_get_recurrence_mode(self.h))
        if m < 0:
            self._ck(m)
        return ('per-step', 'persistent', 'wide-persistent')[m]

    def persist_stats(self):
        """(aborts, re-arms) of the persistent recurrence on this handle (include/nasr.h, nasr_get_persist_stats)."""
        from ctypes import c_int
        a, r = c_int(), c_int()
        self._ck(self.lib.nasr_get_persist_stats(self.h, byref(a), byref(r)))
        return int(a.value), int(r.value)

    def set_recurrence_mode(self, persistent):
        self._ck(self.lib.nasr_set_recurrence_mode(self.h, int(bool(persistent))))

    def phase_times(self):
        pt = _lib.PhaseTimes()
        self._ck(self.lib.nasr_get_phase_times(self.h, byref(pt)))
        return pt.as_dict()


class BeamStream:
    """The CTC beam search of Engine.beam_search as a state that lives between calls (nasr_ctc_beam_open / feed / best /
    close; host only): feed() frames as they arrive, best() at any time.  Feeding an utterance in any split gives the
    ids and log-probability of the whole-utterance search bit for bit.  lm (lm.NGramLM): the fused search; its arrays
    are kept alive here, the library only borrows them.  One object per thread."""

    def __init__(self, num_classes, beam_width=100, merge_repeated=True, lm=None, lm_weight=0.0, lm_bonus=0.0):
        self.lib = _lib.load()
        self.C = int(num_classes)
        if lm is not None and lm.num_classes != self.C:
            raise ValueError(f'the language model has num_classes {lm.num_classes} but the search has {self.C} classes')
        self._args = (self.C, int(beam_width), int(bool(merge_repeated)))
        self._lm = None if lm is None else (_f32(lm.logp), _f32(lm.eos), int(lm.order), int(lm.bos_id), float(lm_weight),
                                            float(lm_bonus))
        self.h = None
        self.frames = 0
        self.reset()

    def reset(self):
        """A new search before its first frame."""
        self.close()
        h = c_void_p()
        lm = self._lm
        tail = (None, None, 1, 0, 0.0, 0.0) if lm is None else (_fp(lm[0]), _fp(lm[1])) + lm[2:]
        rc = self.lib.nasr_ctc_beam_open(*self._args, *tail, byref(h))
        if rc != 0:
            raise _lib.NasrError(rc, 'nasr_ctc_beam_open: bad arguments')
        self.h = h
        self.frames = 0

    def feed(self, logits, slot=None):
        """The next frames: logits [n,C], or column `slot` of a time-major [n,S,C] array (read in place)."""
        lg = _f32(logits)
        if lg.ndim == 3:
            n, S, C = lg.shape
            if not 0 <= int(slot) < S:
                raise ValueError(f'slot {slot} of {S}')
            offset, stride = int(slot) * C, S * C
        else:
            (n, C), offset, stride = lg.shape, 0, lg.shape[1]
        if C != self.C:
            raise ValueError(f'{C} classes fed to a search over {self.C}')
        if n:
            ptr = ctypes.cast(lg.ctypes.data + 4 * offset, POINTER(c_float))
            rc = self.lib.nasr_ctc_beam_feed(self.h, ptr, stride, n)
            if rc != 0:
                raise _lib.NasrError(rc, 'nasr_ctc_beam_feed: bad arguments')
        self.frames += n

    def best(self):
        """(ids, log-probability) of the top path of the frames fed so far; does not disturb the search."""
        ids = np.zeros(max(self.frames, 1), np.int32)
        n, logp = c_int32(), c_float()
        rc = self.lib.nasr_ctc_beam_best(self.h, _ip(ids), ids.size, byref(n), byref(logp))
        if rc != 0:
            raise _lib.NasrError(rc, 'nasr_ctc_beam_best: bad arguments')
        return ids[:n.value].tolist(), float(logp.value)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.nasr_ctc_beam_close(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WaveNetEngine(Engine):
    """An Engine over a WaveNet handle (include/nasr.h: nasr_create_wavenet): the same step, parameter, batch, decoder and
    gradient-exchange calls, plus the batch-norm state.  Only dim 128 and kernel size 7 are implemented."""

    def __init__(self, feature_size, num_classes, num_blocks=3, rates=(1, 2, 4, 8, 16), dim=128, kernel_size=7,
                 bn_epsilon=1e-3, bn_decay=0.99, learning_rate=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, device_id=0,
                 stream=None):
        self.lib = _lib.load()
        rates = tuple(int(r) for r in rates)
        if len(rates) > 8:
            raise ValueError('at most 8 dilation rates')
        cfg = _lib.WaveNetCfg(int(feature_size), int(num_classes), int(dim), int(kernel_size), int(num_blocks),
                              len(rates), (c_int32 * 8)(*(rates + (0,) * (8 - len(rates)))), float(bn_epsilon),
                              float(bn_decay), float(learning_rate), float(beta1), float(beta2), float(epsilon))
        self._open(self.lib.nasr_create_wavenet, cfg, device_id, stream)
        self.bn_count = int(self.lib.nasr_wavenet_bn_count(self.h))

    def bn_state(self):
        """(moving_mean, moving_variance, biased, updates): [S, dim] arrays in site order and the update count."""
        n = self.bn_count
        mm, mv, bs = (np.empty(n, np.float32) for _ in range(3))
        cnt = c_int64()
        self._ck(self.lib.nasr_wavenet_get_bn_state(self.h, _fp(mm), _fp(mv), _fp(bs), n, byref(cnt)))
        d = self.cfg.dim
        return mm.reshape(-1, d), mv.reshape(-1, d), bs.reshape(-1, d), cnt.value

    def set_bn_state(self, moving_mean, moving_var, biased, updates):
        mm, mv, bs = (_f32(a).ravel() for a in (moving_mean, moving_var, biased))
        self._ck(self.lib.nasr_wavenet_set_bn_state(self.h, _fp(mm), _fp(mv), _fp(bs), mm.size, int(updates)))

    def set_bn_hold(self, hold):
        self._ck(self.lib.nasr_wavenet_set_bn_hold(self.h, int(bool(hold))))

    def batch_stats(self):
        """(mean, variance of the update) of the last gradient pass, [S, dim] each."""
        n = self.bn_count
        m, v = np.empty(n, np.float32), np.empty(n, np.float32)
        self._ck(self.lib.nasr_wavenet_get_batch_stats(self.h, _fp(m), _fp(v), n))
        d = self.cfg.dim
        return m.reshape(-1, d), v.reshape(-1, d)

    def apply_bn_stats(self, means, variances):
        """Apply len(means) moving-statistics updates in order (means / variances: sequences of [S, dim] arrays)."""
        k = len(means)
        if k == 0:
            return
        m = _f32(np.stack([np.asarray(x).ravel() for x in means]))
        v = _f32(np.stack([np.asarray(x).ravel() for x in variances]))
        self._ck(self.lib.nasr_wavenet_apply_bn_stats(self.h, _fp(m), _fp(v), self.bn_count, k))


class LasEngine(Engine):
    """An Engine over a LAS handle (include/nasr.h: nasr_create_las): the common parameter, batch, gradient, Adam and
    exchange calls, plus the decoder's logits, the ids fed to its steps and the scheduled-sampling state.  Labels are
    dense [B, U]; the loss is sequence_loss."""

    def __init__(self, feature_size, num_classes, num_hidden=250, num_layers=4, sampling_probability=0.1, seed=1,
                 learning_rate=1e-4, beta1=0.9, beta2=0.999, epsilon=1e-8, device_id=0, stream=None):
        self.lib = _lib.load()
        cfg = _lib.LasCfg(int(feature_size), int(num_classes), int(num_hidden), int(num_layers),
                          float(sampling_probability), int(seed) & 0xFFFFFFFF, float(learning_rate), float(beta1),
                          float(beta2), float(epsilon))
        self._open(self.lib.nasr_create_las, cfg, device_id, stream)
        self._BU = (0, 0)

    def set_step_decode(self, on, logits=False, greedy=True):
        """The LAS step has no CTC step results: its loss and logits are read after the pass (get_loss, logits)."""

    def upload_batch(self, feats, seq_len, labels, label_len):
        feats, seq, labels, ll, B, T, U = self._batch(feats, seq_len, labels, label_len)
        self._BU = (B, U)
        self._ck(self.lib.nasr_upload_batch(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, U))

    def upload_batch_audio(self, featurizer, audios, labels, label_len, rates=None, aug=None, wave=None):
        self._BU = (len(audios), 0 if labels is None else np.asarray(labels).reshape(len(audios), -1).shape[1])
        return Engine.upload_batch_audio(self, featurizer, audios, labels, label_len, rates, aug, wave)

    def align(self, *a, **k):
        raise NotImplementedError('forced alignment walks a CTC lattice; the LAS network has none')

    align_resident = align_logits = align

    def las_forward(self, feats, seq_len, labels, label_len, sample=False):
        """logits [B, U, C] of a decoder pass (sample: scheduled sampling at the handle's probability); loss via get_loss."""
        feats, seq, labels, ll, B, T, U = self._batch(feats, seq_len, labels, label_len)
        self._BU = (B, U)
        out = np.empty((B, U, self.num_classes), np.float32)
        self._ck(self.lib.nasr_las_forward(self.h, _fp(feats), _ip(seq), _ip(labels), _ip(ll), B, T, U, int(bool(sample)),
                                           _fp(out)))
        return out

    def las_forward_resident(self, sample=False):
        """las_forward on the batch that is resident already (upload_batch, upload_batch_audio): logits [B, U, C]"""
        B, U = self._BU
        out = np.empty((B, U, self.num_classes), np.float32)
        self._ck(self.lib.nasr_las_forward_resident(self.h, int(bool(sample)), _fp(out)))
        return out

    def loss(self, feats, seq_len, labels, label_len):
        _, _, labels, _, B, _, U = self._batch(feats, seq_len, labels, label_len)
        self._BU = (B, U)
        return Engine.loss(self, feats, seq_len, labels, label_len)

    def loss_and_grads(self, feats, seq_len, labels, label_len):
        _, _, labels, _, B, _, U = self._batch(feats, seq_len, labels, label_len)
        self._BU = (B, U)
        return Engine.loss_and_grads(self, feats, seq_len, labels, label_len)

    def logits(self):
        """logits [B, U, C] of the last decoder pass"""
        B, U = self._BU
        out = np.empty((B, U, self.num_classes), np.float32)
        self._ck(self.lib.nasr_las_get_logits(self.h, _fp(out)))
        return out

    def fed_ids(self):
        """the ids the last decoder pass fed to its steps [B, U] (labels, or scheduled samples)"""
        B, U = self._BU
        out = np.empty((B, U), np.int32)
        self._ck(self.lib.nasr_las_get_fed_ids(self.h, _ip(out)))
        return out

    def sampled(self):
        """1 where the last decoder pass fed a scheduled sample instead of the label [B, U]"""
        B, U = self._BU
        out = np.empty((B, U), np.int32)
        self._ck(self.lib.nasr_las_get_sampled(self.h, _ip(out)))
        return out

    def sampling_state(self):
        p, seed, counter, tower = c_float(), c_uint32(), c_uint32(), ctypes.c_int()
        self._ck(self.lib.nasr_las_get_sampling(self.h, byref(p), byref(seed), byref(counter), byref(tower)))
        return float(p.value), int(seed.value), int(counter.value), int(tower.value)

    def set_sampling_state(self, p, seed, counter, tower=0):
        self._ck(self.lib.nasr_las_set_sampling(self.h, float(p), int(seed) & 0xFFFFFFFF, int(counter) & 0xFFFFFFFF,
                                                int(tower)))

    def beam_search(self, feats, seq_len, beam_width, max_steps, start_id, end_id, length_penalty=0.5, trace=False):
        """The reference's inference graph (include/nasr.h: nasr_las_beam_search): {'steps': T_dec, 'predicted_ids':
        gather_tree's ids [B, T_dec, W]}, and with trace also every step's 'scores', 'word_ids', 'parent_ids'
        [B, T_dec, W] and the final 'log_probs', 'lengths', 'finished' [B, W]."""
        feats, seq, _, _, B, T, _ = self._batch(feats, seq_len)
        steps = c_int32()
        self._ck(self.lib.nasr_las_beam_search(self.h, _fp(feats), _ip(seq), B, T, int(beam_width), int(max_steps),
                                               int(start_id), int(end_id), float(length_penalty), byref(steps)))
        return self._beam_results(B, int(beam_width), steps.value, trace)

    def beam_search_resident(self, beam_width, max_steps, start_id, end_id, length_penalty=0.5, trace=False):
        """beam_search over the batch that is resident already (include/nasr.h: nasr_las_beam_search_resident): no feature
        leaves the host, and the batch stays as it is for the passes that follow."""
        steps = c_int32()
        self._ck(self.lib.nasr_las_beam_search_resident(self.h, int(beam_width), int(max_steps), int(start_id),
                                                        int(end_id), float(length_penalty), byref(steps)))
        return self._beam_results(self._BU[0], int(beam_width), steps.value, trace)

    def _beam_results(self, B, W, Td, trace):
        out = {'steps': Td, 'predicted_ids': np.empty((B, Td, W), np.int32)}
        self._ck(self.lib.nasr_las_beam_get_ids(self.h, _ip(out['predicted_ids'])))
        if trace:
            out['scores'] = np.empty((B, Td, W), np.float32)
            out['word_ids'] = np.empty((B, Td, W), np.int32)
            out['parent_ids'] = np.empty((B, Td, W), np.int32)
            self._ck(self.lib.nasr_las_beam_get_trace(self.h, _fp(out['scores']), _ip(out['word_ids']),
                                                      _ip(out['parent_ids'])))
            out['log_probs'] = np.empty((B, W), np.float32)
            out['lengths'] = np.empty((B, W), np.int32)
            fin = np.empty((B, W), np.int32)
            self._ck(self.lib.nasr_las_beam_get_final(self.h, _fp(out['log_probs']), _ip(out['lengths']), _ip(fin)))
            out['finished'] = fin != 0
        return out

    def set_lm(self, lm, weight=0.0):
        """Fuse an n-gram model (lm.NGramLM, or a float32 table [K][C] with its order as (table, order)) into every later
        beam search (include/nasr.h: nasr_las_beam_set_lm); None removes it."""
        if lm is None:
            return self._ck(self.lib.nasr_las_beam_set_lm(self.h, None, 0, 0.0))
        table, order, classes = (lm.logp, lm.order, lm.num_classes) if hasattr(lm, 'logp') else (lm[0], lm[1], None)
        table = _f32(table)
        if classes is None:
            classes = table.shape[-1]
        if classes != self.num_classes or table.size != self.num_classes ** int(order):
            raise ValueError(f'an order-{order} table over {self.num_classes} classes has {self.num_classes}^{order} '
                             f'entries; got num_classes {classes} and {table.size} entries')
        self._ck(self.lib.nasr_las_beam_set_lm(self.h, _fp(table), int(order), float(weight)))

    def lm_context(self, B, W):
        """the final n-gram context index of every beam of the last search [B, W]"""
        out = np.empty((B, W), np.int32)
        self._ck(self.lib.nasr_las_beam_get_lm_context(self.h, _ip(out)))
        return out

    def beam_times(self):
        """device-timed ms of the last search's phases (it must have run with profiling on: set_profiling(True))"""
        ms = (c_float * 7)()
        self._ck(self.lib.nasr_las_beam_get_times(self.h, ms))
        names = ('encoder', 'decoder_gemm', 'decoder_cell', 'attention', 'selection', 'gather_tree', 'host_wait')
        return dict(zip(names, (float(x) for x in ms)))
