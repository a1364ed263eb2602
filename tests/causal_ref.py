"""fp64 NumPy restatement of the causal normalisation of the GPU front end (the reference has only the
whole-utterance rule of utils.py:29), on top of tests/mfcc_ref.py and tests/feat_ref.py, and a pure-NumPy simulator of a
stream session that takes samples: the sample tail, the running sums, rows_total and the ring of normalised frames.

The rule.  x[u] is un-normalised frame u of T (D columns), M = norm_min_frames, nc = numcontext:
  p1[u] = sum_k x[u][k], p2[u] = sum_k x[u][k] * x[u][k]     columns in ascending order, product rounded before the add
  S[0] = 0, S[n] = S[n-1] + p[n-1]                           strictly in frame order (numpy.cumsum)
  n_u = min(T, max(u+1, M)); N = n_u D; mean = S1[n_u] / N; var = S2[n_u] / N - mean mean; sd = sqrt(var) if var > 0 else 1
  y[u][k] = float32((x[u][k] - mean) / sd);  row t = y[t-nc .. t+nc], exact 0.0f outside the utterance.

The spectral part of a frame is computed one frame per call, offline as in the simulator, so that the two agree bit for
bit whatever a BLAS does with matrices of different heights."""
import functools

import numpy as np

import feat_ref as FR
import mfcc_ref as R

NFFT = 512


@functools.lru_cache(maxsize=None)
def _tables(samplerate, numcep, kind, nfilt):
    nf = numcep if kind == 'logfbank' else nfilt
    return R.filterbank(samplerate, NFFT, nf).T.copy(), R.dct_ortho(nf, numcep).T.copy()


def spectral(frames, samplerate, numcep, kind='mfcc', nfilt=128):
    """pre-emphasised float32 frames [n, frame_len] -> float64 [n, numcep]: mfcc_ref.mfcc / feat_ref.logfbank after
    framesig, one frame per call"""
    if kind not in FR.KINDS:
        raise ValueError('kind must be one of %r' % (FR.KINDS,))
    fb, dct = _tables(samplerate, numcep, kind, nfilt)
    out = np.empty((len(frames), numcep), dtype=np.float64)
    for i, fr in enumerate(frames):
        pspec = 1.0 / NFFT * np.square(np.absolute(np.fft.rfft(fr[None].astype(np.float64), NFFT)))
        feat = np.dot(pspec, fb)
        feat = np.log(np.where(feat == 0, R.EPS, feat))
        if kind == 'mfcc':
            energy = np.sum(pspec, 1)
            feat = R.lifter(feat @ dct, 22)
            feat[:, 0] = np.log(np.where(energy == 0, R.EPS, energy))
        out[i] = feat[0]
    return out


def raw_frames(audio, samplerate, numcep, kind='mfcc', nfilt=128):
    """float64 [T, numcep]: the un-normalised frames of an utterance (no deltas under the causal rule)"""
    sig = R.preemphasis(audio, 0.97)
    frame_len, frame_step = R.frame_params(samplerate)
    return spectral(R.framesig(sig, frame_len, frame_step), samplerate, numcep, kind, nfilt)


def frame_sums(x):
    """(p1 [T], p2 [T]): the column sums of every frame, columns in ascending order, one accumulator each"""
    p1, p2 = np.zeros(x.shape[0]), np.zeros(x.shape[0])
    for k in range(x.shape[1]):
        p1 = p1 + x[:, k]
        p2 = p2 + x[:, k] * x[:, k]
    return p1, p2


def prefix(p):
    """S [T+1]: S[0] = 0, S[n] = S[n-1] + p[n-1] (numpy.cumsum adds in order)"""
    return np.concatenate(([0.0], np.cumsum(p)))


def mean_sd(S1n, S2n, n, D):
    N = float(n * D)
    mean = S1n / N
    var = S2n / N - mean * mean
    return mean, (np.sqrt(var) if var > 0 else 1.0)


def count(u, T, M):
    """n_u: the frames whose statistics normalise frame u"""
    return min(T, max(u + 1, M))


def normalise_frames(x, M):
    """float64 [T, D] -> float32 [T, D] under the rule, and (mean, sd) of all T frames"""
    T, D = x.shape
    p1, p2 = frame_sums(x)
    S1, S2 = prefix(p1), prefix(p2)
    y = np.empty((T, D), dtype=np.float32)
    for u in range(T):
        n = count(u, T, M)
        mean, sd = mean_sd(S1[n], S2[n], n, D)
        y[u] = ((x[u] - mean) / sd).astype(np.float32)
    return y, mean_sd(S1[T], S2[T], T, D)


def stack(y, numcontext):
    """float32 [T, D] -> [T, (2 numcontext + 1) D]: include_context, exact zeros outside the utterance"""
    return R.include_context(y, numcontext) if numcontext > 0 else y


def features(audio, samplerate, numcontext, numcep, M, kind='mfcc', nfilt=128):
    """float32 [T, (2*numcontext+1)*numcep], and (mean, sd) at n = T"""
    y, ms = normalise_frames(raw_frames(audio, samplerate, numcep, kind, nfilt), M)
    return stack(y, numcontext), ms


# ------------------------------------------------------------------------------------------------- streaming
def complete_frames(n, frame_len, frame_step):
    """Fc: the frames whose every sample has arrived"""
    return 0 if n < frame_len else 1 + (n - frame_len) // frame_step


def rows_total(n, finished, samplerate, numcontext, M):
    """the rows that exist once n samples of an utterance have arrived (finished: it was declared complete)"""
    frame_len, frame_step = R.frame_params(samplerate)
    if finished:
        if n < 1:
            raise ValueError('an utterance needs at least one sample')
        return R.num_frames(n, samplerate)
    Fc = complete_frames(n, frame_len, frame_step)
    return 0 if Fc < M else max(0, Fc - numcontext)


class StreamSim:
    """One slot of a stream session fed with samples.  Its state does not grow with the utterance: the un-framed tail of the
    samples (with the one sample in front of it that pre-emphasis reads), the running sums and counts, the raw frames not
    yet normalisable (at most M) and the last 2 numcontext normalised frames."""

    def __init__(self, samplerate, numcontext, numcep, M, kind='mfcc', nfilt=128):
        self.sr, self.nc, self.numcep, self.M, self.kind, self.nfilt = samplerate, numcontext, numcep, M, kind, nfilt
        self.frame_len, self.frame_step = R.frame_params(samplerate)
        self.reset()

    def reset(self):
        self.tail = np.zeros(0, np.float32)      # samples from max(0, nframes * frame_step - 1) on
        self.n = 0                               # samples received
        self.nframes = 0                         # frames made: their sums are in S1, S2
        self.S1 = self.S2 = 0.0
        self.pending = []                        # raw frames 0 .. nframes-1 while nframes < M
        self.ring = []                           # the last 2 nc normalised frames
        self.nnorm = 0                           # frames normalised
        self.rows = 0                            # rows emitted
        self.finished = False

    def max_state(self):
        return len(self.tail), len(self.pending), len(self.ring)

    def _frame(self, f, pad):
        """pre-emphasised frame f from the tail; pad: zero-padded past the last sample"""
        t0 = f * self.frame_step
        first = max(0, self.nframes * self.frame_step - 1)            # the sample index of tail[0]
        out = np.zeros(self.frame_len, np.float32)
        hi = min(self.frame_len, self.n - t0)
        assert pad or hi == self.frame_len
        cur = self.tail[t0 - first:t0 - first + hi]
        if t0 == 0:
            out[0] = cur[0]
            out[1:hi] = cur[1:] - np.float32(0.97) * cur[:-1]
        else:
            prev = self.tail[t0 - first - 1:t0 - first - 1 + hi]
            out[:hi] = cur - np.float32(0.97) * prev
        return out

    def feed(self, samples, last=False):
        """the new samples (possibly none) -> the rows they make, float32 [k, (2 nc + 1) numcep]"""
        if self.finished:
            raise RuntimeError('the slot is finished: reset it first')
        samples = np.asarray(samples, dtype=np.float32).reshape(-1)
        if last and self.n + samples.size < 1:
            raise ValueError('an utterance needs at least one sample')
        self.tail = np.concatenate((self.tail, samples))
        self.n += samples.size
        D, M, nc = self.numcep, self.M, self.nc
        # the newly complete frames, and at `last` the zero-padded one
        want = R.num_frames(self.n, self.sr) if last else complete_frames(self.n, self.frame_len, self.frame_step)
        full = complete_frames(self.n, self.frame_len, self.frame_step)
        new = [self._frame(f, f >= full) for f in range(self.nframes, want)]
        x = spectral(new, self.sr, D, self.kind, self.nfilt) if new else np.zeros((0, D))
        p1, p2 = frame_sums(x)
        first_new = self.nframes
        S = {}                                   # (S1, S2) at the frame counts reached in this feed
        for i in range(len(new)):
            self.S1 = self.S1 + p1[i]
            self.S2 = self.S2 + p2[i]
            S[first_new + i + 1] = (self.S1, self.S2)
        S[want] = (self.S1, self.S2)
        self.nframes = want
        keep = max(0, want * self.frame_step - 1)
        self.tail = self.tail[keep - max(0, first_new * self.frame_step - 1):]
        raw = {u: r for u, r in zip(range(first_new - len(self.pending), first_new), self.pending)}
        raw.update({first_new + i: x[i] for i in range(len(new))})
        # which frames can be normalised now: all of them once M frames exist or the utterance is complete
        T = want if last else None
        upto = want if (last or want >= M) else 0
        ys = {}
        for u in range(self.nnorm, upto):
            n = max(u + 1, M) if T is None else min(T, max(u + 1, M))
            mean, sd = mean_sd(S[n][0], S[n][1], n, D)
            ys[u] = ((raw[u] - mean) / sd).astype(np.float32)
        self.pending = [] if upto else [raw[u] for u in range(want)]
        ring0 = self.nnorm - len(self.ring)
        y = {ring0 + i: r for i, r in enumerate(self.ring)}
        y.update(ys)
        self.nnorm = upto
        # the rows whose whole window exists
        total = want if last else max(0, upto - nc)
        zero = np.zeros(D, np.float32)
        out = np.empty((total - self.rows, (2 * nc + 1) * D), np.float32)
        for t in range(self.rows, total):
            out[t - self.rows] = np.concatenate([y[s] if 0 <= s < upto else zero for s in range(t - nc, t + nc + 1)])
        self.rows = total
        self.ring = [y[u] for u in range(max(0, self.nnorm - 2 * nc), self.nnorm)] if nc else []
        self.finished = bool(last)
        return out
