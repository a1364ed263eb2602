"""fp64 NumPy restatement of the front end's other features, on top of tests/mfcc_ref.py: python_speech_features 0.6's
logfbank (the log-mel filterbank energies: mfcc without the DCT, the lifter and the energy column) and its
delta(feat, N=2), then include_context and the whole-utterance normalisation on the widened frames
[static | delta | delta-delta].  Written from psf 0.6's documented procedure; psf is not installed, so neither the
procedure nor the summation order (numpy.dot's, inside psf's delta) is pinned against the package.  The kernels of
neuralasr_amd/csrc/mfcc.hip (mfcc_spectral_kernel, mfcc_delta_kernel, mfcc_norm_kernel) are checked against it."""
import numpy as np

import mfcc_ref as R

KINDS = ('mfcc', 'logfbank')


def logfbank(audio, samplerate, nfilt, nfft=512, winlen=0.025, winstep=0.01, preemph=0.97):
    """psf 0.6 logfbank(winfunc=ones) on float32 audio: float64 [T, nfilt]."""
    sig = R.preemphasis(audio, preemph)
    frame_len, frame_step = R.frame_params(samplerate, winlen, winstep)
    frames = R.framesig(sig, frame_len, frame_step)
    pspec = 1.0 / nfft * np.square(np.absolute(np.fft.rfft(frames.astype(np.float64), nfft)))
    feat = np.dot(pspec, R.filterbank(samplerate, nfft, nfilt).T)
    feat = np.where(feat == 0, R.EPS, feat)
    return np.log(feat)


def delta(feat, N=2):
    """psf 0.6 delta(feat, N): delta[t] = sum_{n=1..N} n (p[t+n] - p[t-n]) / (2 sum n^2), p = feat edge-replicated by N
    frames.  The sum runs n = 1, 2, .. in that order (the kernel's order)."""
    feat = np.asarray(feat, dtype=np.float64)
    T = feat.shape[0]
    p = np.pad(feat, ((N, N), (0, 0)), mode='edge')
    acc = np.zeros_like(feat)
    for n in range(1, N + 1):
        acc = acc + n * (p[N + n:N + n + T] - p[N - n:N - n + T])
    return acc / (2 * sum(n * n for n in range(1, N + 1)))


def with_deltas(static, deltas):
    """[T, C] -> [T, C (1 + deltas)]: [static | delta | delta of the delta]; each level pads ITS input's edges."""
    if deltas not in (0, 1, 2):
        raise ValueError('deltas must be 0, 1 or 2')
    cols = [static]
    for _ in range(deltas):
        cols.append(delta(cols[-1], 2))
    return np.concatenate(cols, axis=1) if deltas else static


def frames(audio, samplerate, numcep, kind='mfcc', deltas=0, nfilt=128):
    """float64 [T, numcep (1 + deltas)]: the un-normalised frames."""
    if kind not in KINDS:
        raise ValueError('kind must be one of %r' % (KINDS,))
    static = R.mfcc(audio, samplerate, numcep, nfilt=nfilt) if kind == 'mfcc' else logfbank(audio, samplerate, numcep)
    return with_deltas(static, deltas)


def normalise(x, numcontext):
    """include_context and (X - mean) / std over the stacked matrix, zero pads included: float32, and (mean, std)."""
    if numcontext > 0:
        x = R.include_context(x, numcontext)
    mean, std = np.mean(x), np.std(x)
    return ((x - mean) / std).astype(np.float32), (mean, std)


def features(audio, samplerate, numcontext, numcep, kind='mfcc', deltas=0, nfilt=128):
    """float32 [T, (2*numcontext+1) * numcep * (1+deltas)], and (mean, std).  kind='mfcc', deltas=0 is
    mfcc_ref.features, bit for bit."""
    return normalise(frames(audio, samplerate, numcep, kind, deltas, nfilt), numcontext)
