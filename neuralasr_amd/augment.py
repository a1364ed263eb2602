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
step the batch trains, so a resumed run draws what the uninterrupted one drew."""
import math

import numpy as np

from .features import AudioBatch, num_frames, resample_length

KIND_SPEED, KIND_TIME, KIND_FREQ = 0, 1, 2


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

    def batch(self, counter, audios, rates, chars=None):
        """The AudioBatch of step `counter`: speed first, then the time masks from the resulting seq_len, then the
        frequency masks."""
        new_rates, _ = self.speed(counter, [np.asarray(a).size for a in audios], rates, chars)
        b = AudioBatch(self.samplerate, audios, new_rates, self.width)
        b.time_masks, b.freq_masks = self.masks(counter, b.seq_len)
        return b
