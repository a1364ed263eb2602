"""The augmentation policy of `train --from-audio`: speed perturbation and SpecAugment's time and
frequency masks, drawn on the host in plain NumPy; the GPU applies them (the resampler takes the perturbed rate, the
kernel that stacks the context zeroes the masked frames and columns).  The reference has no counterpart: its only
augmentation is rand_shift (dataset.py:23-31), and its README lists other featurization techniques as a to-do; the rules
here are this package's own.

Every draw is a pure function of (augment_seed, counter, rank, the utterance's index in the global batch, kind, mask
index) and of nothing else - not of the order of the draws, the tower split or np.random's global state:

    Philox4x64 (np.random.Philox) with  key     = [augment_seed, kind << 32 | mask index]
                                        counter = [counter, rank, utterance index, 0]
    its first two 64-bit outputs r0, r1 (random_raw(2)); a choice among n values is r % n (the bias, n / 2^64, is
    below anything a training run could see).

kind 0 (speed): the factor is speed_perturb[r0 % len(speed_perturb)].  kind 1 (time mask k): width r0 % (wmax + 1) with
wmax = min(spec_time_width, floor(spec_time_ratio * len)), first frame r1 % (len - width + 1).  kind 2 (frequency mask
k): width r0 % (min(spec_freq_width, numcep) + 1), first column r1 % (numcep - width + 1).  The counter is the global
step the batch trains, so a resumed run draws what the uninterrupted one drew.

The waveform augmentation (nasr_wave_aug in include/nasr.h has the rules the GPU applies): with
u(r) = (r >> 11) * 2^-53, kind 3 (reverberation): applied iff u(r0) < rir_prob, with RIR r1 % n_rirs of rir_list.  kind 4
(noise): applied iff u(r0) < noise_prob, with clip r1 % n_clips of noise_list.  kind 5 (placement of the noise): the
clip's first sample is r0 % L (L its length at the config rate), the SNR noise_snr[0] + (noise_snr[1] - noise_snr[0]) *
u(r1) dB.  The banks themselves are read once (load_banks) and live on the featurizer."""
import math
import os

import numpy as np

from .features import AudioBatch, num_frames, read_wav_native, resample_length, wav_info

KIND_SPEED, KIND_TIME, KIND_FREQ, KIND_RIR, KIND_NOISE, KIND_PLACE = 0, 1, 2, 3, 4, 5
MAX_RIR_TAPS = 8192          # NASR_AUG_MAX_RIR_TAPS


def unit(r):
    """u(r): the 64-bit draw r as a float64 in [0, 1)"""
    return (r >> 11) * 2.0 ** -53


def read_list(list_file):
    """the WAV paths of a list file: one per line, blank lines and lines that start with # skipped; a relative path is
    relative to the list file's directory"""
    here = os.path.dirname(os.path.abspath(list_file))
    with open(list_file) as fh:
        lines = [ln.strip() for ln in fh]
    paths = [ln if os.path.isabs(ln) else os.path.join(here, ln) for ln in lines if ln and not ln.startswith('#')]
    if not paths:
        raise ValueError('%s lists no WAV file' % list_file)
    return paths


def clip_length(path, samplerate):
    """samples of a WAV file once it is at `samplerate` (from its header alone; load_bank's arithmetic)"""
    n, rate = wav_info(path)
    if n < 1:
        raise ValueError('%s holds no sample' % path)
    return n if rate == samplerate else resample_length(n, rate, samplerate)[0]


def prepare_rir(h):
    """A measured room impulse response as the FIR convolves it: everything before the tap of largest |h| (the direct
    path) dropped, so that the reverberated speech stays where the transcription and an alignment expect it; at most 8192
    taps; unit energy (computed in float64); float32."""
    h = np.asarray(h, dtype=np.float64).reshape(-1)
    if h.size == 0 or not np.all(np.isfinite(h)) or not np.any(h):
        raise ValueError('a room impulse response needs a finite, non-zero tap')
    h = h[int(np.argmax(np.abs(h))):][:MAX_RIR_TAPS]
    return (h / math.sqrt(float(np.sum(h * h)))).astype(np.float32)


def load_bank(list_file, featurizer):
    """float32 mono clips of the WAV files of a list file (read_wav_native: several channels become their mean) at the
    featurizer's samplerate; a file at another rate is resampled on the GPU (Featurizer.resample)"""
    out = []
    for path in read_list(list_file):
        a, rate = read_wav_native(path)
        if a.size == 0:
            raise ValueError('%s holds no sample' % path)
        out.append(a if rate == featurizer.samplerate else np.array(featurizer.resample([a], [rate])[0]))
    return out


def load_banks(config, featurizer):
    """(noise clips, prepared RIRs) of config.noise_list / config.rir_list; an empty list for a key that is off"""
    noise = load_bank(config.noise_list, featurizer) if getattr(config, 'noise_list', None) else []
    rirs = [prepare_rir(h) for h in load_bank(config.rir_list, featurizer)] if getattr(config, 'rir_list', None) else []
    return noise, rirs


class Augmenter:
    def __init__(self, config, rank=0):
        self.samplerate = int(config.samplerate)
        self.numcep = int(config.numcep)
        self.width = int(getattr(config, 'feature_size', 0))
        self.time_masks = int(getattr(config, 'spec_time_masks', 0))
        self.time_width = int(getattr(config, 'spec_time_width', 0))
        self.time_ratio = float(getattr(config, 'spec_time_ratio', 1.0))
        self.freq_masks = int(getattr(config, 'spec_freq_masks', 0))
        self.freq_width = int(getattr(config, 'spec_freq_width', 0))
        self.speeds = tuple(float(f) for f in getattr(config, 'speed_perturb', ()))
        self.seed = int(getattr(config, 'augment_seed', 0))
        self.rank = int(rank)
        self.noise_prob = float(getattr(config, 'noise_prob', 0.0)) if getattr(config, 'noise_list', None) else 0.0
        self.rir_prob = float(getattr(config, 'rir_prob', 0.0)) if getattr(config, 'rir_list', None) else 0.0
        self.snr = tuple(float(v) for v in getattr(config, 'noise_snr', (10.0, 20.0)))
        # host only: the banks' sizes from the list files and the WAV headers
        self.clip_len = [clip_length(p, self.samplerate) for p in read_list(config.noise_list)] if self.noise_prob > 0 else []
        self.n_rirs = len(read_list(config.rir_list)) if self.rir_prob > 0 else 0

    def raw(self, counter, utt, kind, k=0):
        """(r0, r1): the two 64-bit values behind the draw (counter, utt, kind, k)"""
        bg = np.random.Philox(key=np.array([self.seed, (kind << 32) | k], dtype=np.uint64),
                              counter=np.array([counter, self.rank, utt, 0], dtype=np.uint64))
        r = bg.random_raw(2)
        return int(r[0]), int(r[1])

    def frames(self, size, rate):
        """frames of `size` samples declared at `rate` Hz (AudioBatch's arithmetic)"""
        n = size if rate == self.samplerate else resample_length(size, rate, self.samplerate)[0]
        return num_frames(n, self.samplerate)

    def speed(self, counter, sizes, rates, chars):
        """(declared rates, factors) of the utterances with `sizes` samples at `rates` Hz: int(round(rate * f)), f a
        uniform choice from speed_perturb; factor 1.0 leaves the rate as it is.  An utterance that would be left with fewer
        frames than its cleaned transcription has characters (chars[i]; kept_rows' rule) keeps 1.0."""
        rates = [self.samplerate] * len(sizes) if rates is None else [int(r) for r in rates]
        if not self.speeds:
            return rates, [1.0] * len(sizes)
        out, factors = [], []
        for i, (size, rate) in enumerate(zip(sizes, rates)):
            f = self.speeds[self.raw(counter, i, KIND_SPEED)[0] % len(self.speeds)]
            new = rate if f == 1.0 else int(round(rate * f))
            if new != rate:
                try:
                    ok = self.frames(size, new) >= (chars[i] if chars is not None else 0)
                except ValueError:          # no sample left at that rate
                    ok = False
                if not ok:
                    new, f = rate, 1.0
            out.append(new)
            factors.append(f if new != rate else 1.0)
        return out, factors

    def masks(self, counter, seq_len):
        """(time_masks int32 [B, spec_time_masks, 2], freq_masks int32 [B, spec_freq_masks, 2]) of (start, width) for
        utterances of seq_len frames; None for a kind with no masks configured"""
        B = len(seq_len)
        tm = np.zeros((B, self.time_masks, 2), np.int32) if self.time_masks else None
        fm = np.zeros((B, self.freq_masks, 2), np.int32) if self.freq_masks else None
        for i in range(B):
            n = int(seq_len[i])
            wmax = min(self.time_width, int(math.floor(self.time_ratio * n)), n)
            for k in range(self.time_masks):
                r0, r1 = self.raw(counter, i, KIND_TIME, k)
                w = r0 % (wmax + 1)
                tm[i, k] = (r1 % (n - w + 1), w)
            fmax = min(self.freq_width, self.numcep)
            for k in range(self.freq_masks):
                r0, r1 = self.raw(counter, i, KIND_FREQ, k)
                w = r0 % (fmax + 1)
                fm[i, k] = (r1 % (self.numcep - w + 1), w)
        return tm, fm

    def wave(self, counter, B):
        """(rir int32 [B], noise int32 [B], noise_off int64 [B], snr_db float32 [B]) of step `counter` as nasr_wave_aug
        takes them, -1 where an utterance gets none; None in the place of the arrays of a kind that is switched off"""
        rir = np.full(B, -1, np.int32) if self.rir_prob > 0 else None
        noise = np.full(B, -1, np.int32) if self.noise_prob > 0 else None
        off = np.zeros(B, np.int64) if noise is not None else None
        snr = np.zeros(B, np.float32) if noise is not None else None
        for i in range(B):
            if rir is not None:
                r0, r1 = self.raw(counter, i, KIND_RIR)
                if unit(r0) < self.rir_prob:
                    rir[i] = r1 % self.n_rirs
            if noise is not None:
                r0, r1 = self.raw(counter, i, KIND_NOISE)
                if unit(r0) < self.noise_prob:
                    noise[i] = r1 % len(self.clip_len)
                    r0, r1 = self.raw(counter, i, KIND_PLACE)
                    off[i] = r0 % self.clip_len[noise[i]]
                    snr[i] = self.snr[0] + (self.snr[1] - self.snr[0]) * unit(r1)
        return rir, noise, off, snr

    def batch(self, counter, audios, rates, chars=None):
        """The AudioBatch of step `counter`: speed first, then the time masks from the resulting seq_len, then the
        frequency masks; the waveform augmentation's draws depend on the batch's size alone."""
        new_rates, _ = self.speed(counter, [np.asarray(a).size for a in audios], rates, chars)
        rir, noise, off, snr = self.wave(counter, len(audios))
        b = AudioBatch(self.samplerate, audios, new_rates, self.width, rir=rir, noise=noise, noise_off=off, snr_db=snr)
        b.time_masks, b.freq_masks = self.masks(counter, b.seq_len)
        return b
