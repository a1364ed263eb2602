"""The feature front end (reference: utils.py:24-31, convert_to_mfcc): WAV reading and the GPU featurizer.

read_wav returns what librosa.load(path, sr, mono=True) returns for a file already at `sr`: float32 samples scaled the
way libsndfile scales them, channels averaged in float32; a file at another rate is an error there.  read_wav_native
returns the same samples and the file's own rate, and Featurizer resamples them on the GPU
(neuralasr_amd/csrc/resample.hip) as librosa 0.6-0.9's resample(res_type='kaiser_best') does: resampy 0.2's sinc
interpolation, then fix_length to ceil(n * sr / rate) samples.
Featurizer runs python_speech_features 0.6's mfcc(nfilt=128), include_context and the whole-utterance normalisation (or,
with normalization='causal', this project's running normalisation: DESIGN.md §16) on
the GPU (the kernels of neuralasr_amd/csrc/mfcc.hip behind the featurizer handle of csrc/nasr_fz.hip), a batch of utterances per call; with `rates`, utterances at another rate are
resampled first and the resampled samples stay on the device.  kind='logfbank' makes psf's logfbank (numcep log-mel
filterbank energies) in the place of the MFCC, and deltas=1|2 appends psf's delta(feat, 2) columns (and their deltas)
to every frame before the context stacking and the normalisation."""
import ctypes
import math
import struct

import numpy as np

from . import _lib

WAVE_FORMAT_PCM = 0x0001
WAVE_FORMAT_IEEE_FLOAT = 0x0003
WAVE_FORMAT_EXTENSIBLE = 0xFFFE


def _chunks(data):
    pos = 12
    while pos + 8 <= len(data):
        cid, size = struct.unpack_from('<4sI', data, pos)
        body = data[pos + 8:pos + 8 + size]
        yield cid, body
        pos += 8 + size + (size & 1)


def _parse(path):
    """(format tag, channels, rate, bits, data chunk) of a RIFF/WAVE file."""
    with open(path, 'rb') as fh:
        data = fh.read()
    if len(data) < 12 or data[:4] != b'RIFF' or data[8:12] != b'WAVE':
        raise ValueError('%s: not a RIFF/WAVE file' % path)
    fmt = pcm = None
    for cid, body in _chunks(data):
        if cid == b'fmt ' and fmt is None:
            if len(body) < 16:
                raise ValueError('%s: short fmt chunk' % path)
            fmt = body
        elif cid == b'data' and pcm is None:
            pcm = body
    if fmt is None or pcm is None:
        raise ValueError('%s: no fmt or data chunk' % path)
    tag, channels, rate, _, block_align, bits = struct.unpack_from('<HHIIHH', fmt, 0)
    if tag == WAVE_FORMAT_EXTENSIBLE:
        if len(fmt) < 40:
            raise ValueError('%s: short WAVE_FORMAT_EXTENSIBLE fmt chunk' % path)
        tag = struct.unpack_from('<H', fmt, 24)[0]     # the first two bytes of the subformat GUID
    return tag, channels, rate, bits, pcm


def _decode(path, tag, channels, bits, pcm):
    """float32 mono samples of a data chunk."""
    if channels < 1:
        raise ValueError('%s: no channels' % path)
    width = bits // 8
    if tag == WAVE_FORMAT_PCM and bits in (8, 16, 24, 32):
        n = len(pcm) // (width * channels) * channels
        raw = np.frombuffer(pcm, dtype=np.uint8, count=n * width)
        if bits == 8:
            y = (raw.astype(np.float32) - 128.0) / 128.0
        elif bits == 16:
            y = raw.view('<i2').astype(np.float32) / np.float32(32768.0)
        elif bits == 24:
            b = raw.reshape(-1, 3).astype(np.int32)
            v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
            v = np.where(v >= 1 << 23, v - (1 << 24), v)
            y = v.astype(np.float32) / np.float32(1 << 23)
        else:
            y = (raw.view('<i4').astype(np.float64) / 2.0 ** 31).astype(np.float32)
    elif tag == WAVE_FORMAT_IEEE_FLOAT and bits in (32, 64):
        n = len(pcm) // (width * channels) * channels
        y = np.frombuffer(pcm, dtype='<f4' if bits == 32 else '<f8', count=n).astype(np.float32)
    else:
        raise ValueError('%s: unsupported WAV encoding (format tag 0x%04x, %d bits); supported are PCM 8/16/24/32-bit '
                         'and IEEE float 32/64-bit' % (path, tag, bits))
    y = y.astype(np.float32, copy=False)
    if channels > 1:
        y = np.mean(y.reshape(-1, channels).T, axis=0)     # librosa.to_mono on float32 [channels, n]
    return np.ascontiguousarray(y, dtype=np.float32)


def read_wav(path, samplerate):
    """float32 [n] of a RIFF/WAVE file: PCM 8/16/24/32-bit, IEEE float 32/64-bit, or WAVE_FORMAT_EXTENSIBLE with a PCM
    or float subformat.  Integers are scaled as libsndfile does (x/32768, x/2^23, x/2^31, (x-128)/128); several
    channels become their float32 mean.  A file whose rate is not `samplerate` raises ValueError."""
    tag, channels, rate, bits, pcm = _parse(path)
    if rate != samplerate:
        raise ValueError('%s: sample rate %d Hz, expected %d Hz (resampling is not supported)' % (path, rate, samplerate))
    return _decode(path, tag, channels, bits, pcm)


def read_wav_native(path):
    """(float32 [n], rate): read_wav's samples of a file at its own rate, for Featurizer's `rates`."""
    tag, channels, rate, bits, pcm = _parse(path)
    return _decode(path, tag, channels, bits, pcm), int(rate)


def wav_info(path):
    """(mono samples, rate) of a RIFF/WAVE file from its chunk headers alone: what read_wav_native would return the
    length and rate of, without reading or decoding the data chunk."""
    with open(path, 'rb') as fh:
        head = fh.read(12)
        if len(head) < 12 or head[:4] != b'RIFF' or head[8:12] != b'WAVE':
            raise ValueError('%s: not a RIFF/WAVE file' % path)
        fmt = nbytes = None
        while fmt is None or nbytes is None:
            hdr = fh.read(8)
            if len(hdr) < 8:
                break
            cid, size = struct.unpack('<4sI', hdr)
            if cid == b'fmt ' and fmt is None:
                fmt = fh.read(size)
                fh.seek(size & 1, 1)
            else:
                if cid == b'data' and nbytes is None:
                    here = fh.tell()
                    fh.seek(0, 2)
                    nbytes = min(size, fh.tell() - here)          # _chunks slices a truncated data chunk the same way
                    fh.seek(here)
                fh.seek(size + (size & 1), 1)
    if fmt is None or nbytes is None or len(fmt) < 16:
        raise ValueError('%s: no fmt or data chunk' % path)
    _, channels, rate, _, _, bits = struct.unpack_from('<HHIIHH', fmt, 0)
    if channels < 1 or bits < 8:
        raise ValueError('%s: no channels' % path)
    return nbytes // (bits // 8 * channels), int(rate)


def write_wav16(path, audio, rate):
    """float samples in [-1, 1) as a mono 16-bit PCM RIFF/WAVE file (tools and tests make their corpora with it)"""
    pcm = np.round(np.asarray(audio) * 32768).astype('<i2').tobytes()
    fmt = struct.pack('<HHIIHH', WAVE_FORMAT_PCM, 1, rate, rate * 2, 2, 16)
    body = b'WAVE' + b'fmt ' + struct.pack('<I', 16) + fmt + b'data' + struct.pack('<I', len(pcm)) + pcm
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', len(body)) + body)


def resample_length(num_samples, rate, samplerate):
    """(librosa's ceil(n * ratio), resampy's int(n * ratio)) of n samples at `rate` resampled to `samplerate` (computed
    by the library, no GPU needed).  ValueError when resampy would raise: a rate <= 0 or no resampled sample."""
    lib = _lib.load()
    filtered = ctypes.c_int64()
    n = lib.nasr_resample_length(int(rate), int(samplerate), int(num_samples), ctypes.byref(filtered))
    if n < 0:
        raise ValueError('%d samples at %d Hz give no sample at %d Hz' % (num_samples, rate, samplerate))
    return int(n), int(filtered.value)


def resample_filter():
    """float64 [32769]: resampy's kaiser_best half window, as the library builds it."""
    lib = _lib.load()
    t = np.empty(32769, dtype=np.float64)
    _lib.check(lib, None, lib.nasr_resample_filter(t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), t.size))
    return t


KINDS = {'mfcc': 0, 'logfbank': 1}
NORMS = {'utterance': 0, 'causal': 1}
NORM_MIN_FRAMES = 50                                       # the default M of the causal rule: 0.5 s of frames


def _cfg(samplerate, numcep, numcontext, nfilt, nfft, kind='mfcc', deltas=0, normalization='utterance',
         norm_min_frames=None):
    if kind not in KINDS:
        raise ValueError("kind must be 'mfcc' or 'logfbank', not %r" % (kind,))
    if normalization not in NORMS:
        raise ValueError("normalization must be 'utterance' or 'causal', not %r" % (normalization,))
    if normalization == 'utterance':
        if norm_min_frames is not None:
            raise ValueError("norm_min_frames belongs to normalization='causal'")
        norm_min_frames = 0                                # not read: the struct stays what it was without the fields
    elif norm_min_frames is None:
        norm_min_frames = NORM_MIN_FRAMES
    if kind == 'logfbank':
        nfilt = numcep                                     # psf logfbank(nfilt=numcep): one column per filter
    return _lib.MfccCfg(samplerate=samplerate, numcep=numcep, numcontext=numcontext, nfilt=nfilt, nfft=nfft,
                        winlen=0.025, winstep=0.01, preemph=0.97, ceplifter=22, append_energy=1,
                        kind=KINDS[kind], deltas=int(deltas), norm=NORMS[normalization],
                        norm_min_frames=int(norm_min_frames))


def num_frames(num_samples, samplerate, numcep=13, nfilt=128, nfft=512):
    """psf's frame count of an utterance (computed by the library, no GPU needed)."""
    lib = _lib.load()
    cfg = _cfg(samplerate, numcep, 0, nfilt, nfft)
    n = lib.nasr_mfcc_frames(ctypes.byref(cfg), int(num_samples))
    if n < 0:
        raise ValueError('no frame count for %d samples at %d Hz' % (num_samples, samplerate))
    return int(n)


def filterbank(samplerate, nfilt=128, nfft=512):
    """(bins int32 [nfilt+2], weights float32 [nfilt, nfft/2+1]): the filterbank the kernels use."""
    lib = _lib.load()
    cfg = _cfg(samplerate, 1, 0, nfilt, nfft)
    bins = np.zeros(nfilt + 2, dtype=np.int32)
    w = np.zeros((nfilt, nfft // 2 + 1), dtype=np.float32)
    rc = lib.nasr_mfcc_filterbank(ctypes.byref(cfg), bins.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                  w.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
    if rc != _lib.NASR_OK:
        raise ValueError('bad filterbank configuration')
    return bins, w


class AudioBatch:
    """A batch as audio: what HipNetwork's *_audio calls and AudioDataSet hand to the step machinery in the place of the
    padded feature array.  The features are made on the device when the batch is uploaded (Engine.upload_batch_audio);
    the frame counts - seq_len and the padded length T - are the library's host-side arithmetic.  `shape` is the shape
    the padded feature array would have.  time_masks [B, nt, 2] / freq_masks [B, nf, 2] (int32, optional): the
    SpecAugment masks a TRAINING step applies to the normalised frames on the device (augment.py);
    validate / evaluate / decode / align ignore them.  rir / noise (int32 [B], -1: none), noise_off (int64 [B]) and
    snr_db (float32 [B]), all optional: the waveform augmentation of a TRAINING step (nasr_wave_aug), indices
    into the banks that the network's featurizer holds; ignored like the masks everywhere else."""

    def __init__(self, samplerate, audios, rates=None, width=0, time_masks=None, freq_masks=None, rir=None, noise=None,
                 noise_off=None, snr_db=None):
        self.samplerate = int(samplerate)
        self.audios = Featurizer._utterances(audios)
        self.rates = None if rates is None else [int(r) for r in rates]
        if self.rates is not None and len(self.rates) != len(self.audios):
            raise ValueError('%d rates for %d utterances' % (len(self.rates), len(self.audios)))
        frames = []
        for i, a in enumerate(self.audios):
            n = a.size
            if self.rates is not None and self.rates[i] != self.samplerate:
                try:
                    n = resample_length(n, self.rates[i], self.samplerate)[0]
                except ValueError as e:
                    raise ValueError('utterance %d: %s' % (i, e)) from None
            frames.append(num_frames(n, self.samplerate))
        self.seq_len = [np.asarray(t, dtype=np.int32) for t in frames]
        self.shape = (len(self.audios), max(frames), int(width))
        self.time_masks = self._masks(time_masks, 'time_masks')
        self.freq_masks = self._masks(freq_masks, 'freq_masks')
        self.rir = self._per_utt(rir, np.int32, 'rir')
        self.noise = self._per_utt(noise, np.int32, 'noise')
        self.noise_off = self._per_utt(noise_off, np.int64, 'noise_off')
        self.snr_db = self._per_utt(snr_db, np.float32, 'snr_db')
        if self.noise is not None and (self.noise_off is None or self.snr_db is None):
            raise ValueError('noise needs noise_off and snr_db')

    def _per_utt(self, a, dtype, name):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=dtype).ravel()
        if a.size != len(self.audios):
            raise ValueError('%s must hold %d values, not %d' % (name, len(self.audios), a.size))
        return a

    def _masks(self, m, name):
        if m is None:
            return None
        m = np.ascontiguousarray(m, dtype=np.int32)
        if m.ndim != 3 or m.shape[0] != len(self.audios) or m.shape[2] != 2:
            raise ValueError('%s must be [%d, n, 2], not %s' % (name, len(self.audios), m.shape))
        return m

    def aug(self, static_width):
        """the masks as the engine's upload calls take them (engine.BatchAug), or None without masks"""
        if self.time_masks is None and self.freq_masks is None:
            return None
        from .engine import BatchAug
        return BatchAug(int(static_width), self.time_masks, self.freq_masks)

    def wave(self):
        """the waveform augmentation as the engine's audio calls take it (engine.WaveAug), or None without any"""
        if self.rir is None and self.noise is None:
            return None
        from .engine import WaveAug
        return WaveAug(self.rir, self.noise, self.noise_off, self.snr_db)

    def __len__(self):
        return len(self.audios)

    def shard(self, lo, hi):
        """utterances [lo, hi) as a batch of their own, padded to ITS longest utterance"""
        def cut(a):
            return None if a is None else a[lo:hi]
        return AudioBatch(self.samplerate, self.audios[lo:hi], cut(self.rates), self.shape[2], cut(self.time_masks),
                          cut(self.freq_masks), cut(self.rir), cut(self.noise), cut(self.noise_off), cut(self.snr_db))


class Featurizer:
    """The normalised MFCC features of utils.convert_to_mfcc for a list of float32 utterances, on the GPU.  compute()
    packs consecutive utterances into calls of at most `max_samples` samples, native and resampled ones counted (a
    longer utterance goes alone).  kind='logfbank': numcep log-mel filterbank energies per frame (nfilt = numcep);
    deltas=1|2: every frame is [static | delta | delta-delta], frame_width = numcep*(1+deltas) wide.  `width` is the
    width of a row that compute() returns: (2*numcontext+1)*frame_width.  normalization='causal'  replaces
    the whole-utterance mean and std by running ones: frame u is normalised with the statistics of its first
    max(u+1, norm_min_frames) frames (default 50; at most the utterance's), context frames outside the utterance are
    exact zeros, and the (mean, std) that compute(return_stats=True) reports are those of all frames."""

    def __init__(self, samplerate, numcep, numcontext, nfilt=128, nfft=512, device_id=0, max_samples=1 << 23,
                 kind='mfcc', deltas=0, normalization='utterance', norm_min_frames=None):
        self.lib = _lib.load()
        self.samplerate, self.numcep, self.numcontext = int(samplerate), int(numcep), int(numcontext)
        self.kind, self.deltas = kind, int(deltas)
        self.max_samples = int(max_samples)
        self.cfg = _cfg(self.samplerate, self.numcep, self.numcontext, nfilt, nfft, kind, self.deltas, normalization,
                        norm_min_frames)
        self.normalization, self.norm_min_frames = normalization, int(self.cfg.norm_min_frames)
        self.frame_width = self.lib.nasr_mfcc_width(ctypes.byref(self.cfg))
        if self.frame_width < 0:                           # nasr_create_featurizer names what is wrong with the cfg
            self.frame_width = self.numcep * (1 + self.deltas)
        self.width = (2 * self.numcontext + 1) * self.frame_width
        h = ctypes.c_void_p()
        rc = self.lib.nasr_create_featurizer(ctypes.byref(self.cfg), device_id, None, ctypes.byref(h))
        _lib.check(self.lib, None, rc)
        self.h = h

    def frame_params(self):
        """(frame_len, frame_step) in samples: psf's round_half_up of winlen and winstep times the rate"""
        def half_up(x):
            return int(math.floor(x)) + (1 if x - math.floor(x) >= 0.5 else 0)
        return half_up(self.cfg.winlen * self.samplerate), max(1, half_up(self.cfg.winstep * self.samplerate))

    def frames(self, num_samples):
        n = self.lib.nasr_mfcc_frames(ctypes.byref(self.cfg), int(num_samples))
        if n < 0:
            raise ValueError('an utterance needs at least one sample')
        return int(n)

    def compute(self, audios, return_stats=False, *, rates=None):
        """list of float32 [n_i] -> list of float32 [T_i, self.width] (and [(mean, std)] if asked).
        rates: each utterance's sample rate; one at another rate than `samplerate` is resampled first (librosa.load)."""
        audios = self._utterances(audios)
        sizes = self._sizes(audios, rates)
        feats, stats = [], []
        i = 0
        while i < len(audios):
            j, total = i, 0
            while j < len(audios) and (j == i or total + sizes[j] <= self.max_samples):
                total += sizes[j]
                j += 1
            f, s = self._call(audios[i:j], None if rates is None else rates[i:j])
            feats += f
            stats += s
            i = j
        return (feats, stats) if return_stats else feats

    def resample(self, audios, rates):
        """list of float32 [n_i] at rates[i] Hz -> list of float32 [ceil(n_i * samplerate / rates[i])]: librosa's
        resample(y, rates[i], samplerate) (res_type 'kaiser_best'); an utterance at `samplerate` comes back as it is."""
        audios = self._utterances(audios)
        lens = [n for n, _ in self._lengths(audios, rates)]
        n = len(audios)
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([a.size for a in audios])
        flat = np.concatenate(audios) if n > 1 else audios[0]
        r = np.ascontiguousarray(rates, dtype=np.int32)
        out = np.empty(int(sum(lens)), dtype=np.float32)
        rc = self.lib.nasr_resample(self.h, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                    offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                    r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n,
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
        _lib.check(self.lib, self.h, rc)
        cut = np.cumsum([0] + lens)
        return [out[cut[k]:cut[k + 1]] for k in range(n)]

    def _set_bank(self, fn, arrays):
        arrays = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in arrays]
        n = len(arrays)
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([a.size for a in arrays])
        flat = np.concatenate(arrays) if n else np.zeros(1, np.float32)
        _lib.check(self.lib, self.h, fn(self.h, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                        offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n))

    def set_noise(self, clips):
        """The noise bank of the waveform augmentation: float32 clips at `samplerate`, uploaded once; an
        empty list frees it."""
        self._set_bank(self.lib.nasr_featurizer_set_noise, clips)
        self.n_clips = len(clips)

    def set_rirs(self, rirs):
        """The bank of room impulse responses, as they are convolved (augment.prepare_rir makes them): at most 8192 taps
        each; an empty list frees it."""
        self._set_bank(self.lib.nasr_featurizer_set_rirs, rirs)
        self.n_rirs = len(rirs)

    def augment_audio(self, audios, rates=None, wave=None):
        """resample() followed by the waveform augmentation `wave` (engine.WaveAug or None) on the device: the list of
        float32 waveforms at `samplerate` that the spectral kernel of an upload_batch_audio(..., wave=wave) reads."""
        audios = self._utterances(audios)
        n = len(audios)
        lens = [a.size for a in audios] if rates is None else [m for m, _ in self._lengths(audios, rates)]
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([a.size for a in audios])
        flat = np.concatenate(audios) if n > 1 else audios[0]
        r = None if rates is None else np.ascontiguousarray(rates, dtype=np.int32)
        st, keep = wave.struct(n) if wave is not None else (None, None)
        out = np.empty(int(sum(lens)), dtype=np.float32)
        rc = self.lib.nasr_augment_audio(self.h, flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),
                                         offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                         None if r is None else r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n,
                                         None if st is None else ctypes.byref(st),
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size)
        _lib.check(self.lib, self.h, rc)
        cut = np.cumsum([0] + lens)
        return [out[cut[k]:cut[k + 1]] for k in range(n)]

    @staticmethod
    def _utterances(audios):
        audios = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in audios]
        for i, a in enumerate(audios):
            if a.size == 0:
                raise ValueError('utterance %d has no samples' % i)
        return audios

    def _lengths(self, audios, rates):
        """[(resampled length, filtered length)] of every utterance; ValueError naming the first that has none."""
        if len(rates) != len(audios):
            raise ValueError('%d rates for %d utterances' % (len(rates), len(audios)))
        out = []
        for i, (a, r) in enumerate(zip(audios, rates)):
            try:
                out.append(resample_length(a.size, r, self.samplerate))
            except ValueError as e:
                raise ValueError('utterance %d: %s' % (i, e)) from None
        return out

    def _sizes(self, audios, rates):
        """the samples an utterance takes on the device: native, plus resampled when its rate is not `samplerate`."""
        if rates is None:
            return [a.size for a in audios]
        return [a.size + (n if int(r) != self.samplerate else 0)
                for a, r, (n, _) in zip(audios, rates, self._lengths(audios, rates))]

    def _call(self, audios, rates=None):
        n = len(audios)
        offsets = np.zeros(n + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([a.size for a in audios])
        flat = np.concatenate(audios) if n > 1 else audios[0]
        if rates is None:
            frames = [self.frames(a.size) for a in audios]
        else:
            frames = [self.frames(m) for m, _ in self._lengths(audios, rates)]
        rows = int(sum(frames))
        out = np.empty((rows, self.width), dtype=np.float32)
        ms = np.empty((n, 2), dtype=np.float64)
        args = (out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), rows,
                ms.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        audio_p = flat.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
        off_p = offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        if rates is None:
            rc = self.lib.nasr_featurize(self.h, audio_p, off_p, n, *args)
        else:
            r = np.ascontiguousarray(rates, dtype=np.int32)
            rc = self.lib.nasr_featurize_rates(self.h, audio_p, off_p, r.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                               n, *args)
        _lib.check(self.lib, self.h, rc)
        cut = np.cumsum([0] + frames)
        return [out[cut[k]:cut[k + 1]] for k in range(n)], [tuple(ms[k]) for k in range(n)]

    def times(self):
        """(h2d_ms, kernel_ms, d2h_ms) of the last library call."""
        t = [ctypes.c_float() for _ in range(3)]
        _lib.check(self.lib, self.h, self.lib.nasr_featurize_times(self.h, *[ctypes.byref(x) for x in t]))
        return tuple(x.value for x in t)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.nasr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
