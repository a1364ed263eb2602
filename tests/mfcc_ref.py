"""fp64 NumPy restatement of the reference's MFCC front end (utils.py:24-31): python_speech_features 0.6's
mfcc(audio, samplerate, numcep=numcep, nfilt=128) on float32 audio, include_context and the whole-utterance
normalisation.  NumPy only (the DCT is an explicit cosine matrix): the kernels of neuralasr_amd/csrc/mfcc.hip
(launched through csrc/mfcc.h by the featurizer handle, csrc/nasr_fz.hip) are checked against it."""
import decimal
import math

import numpy as np

EPS = np.finfo(float).eps            # psf's stand-in for exact zeros before a log


def round_half_up(number):
    return int(decimal.Decimal(number).quantize(decimal.Decimal('1'), rounding=decimal.ROUND_HALF_UP))


def frame_params(samplerate, winlen=0.025, winstep=0.01):
    return round_half_up(winlen * samplerate), round_half_up(winstep * samplerate)


def num_frames(num_samples, samplerate, winlen=0.025, winstep=0.01):
    frame_len, frame_step = frame_params(samplerate, winlen, winstep)
    if num_samples <= frame_len:
        return 1
    return 1 + int(math.ceil((1.0 * num_samples - frame_len) / frame_step))


def preemphasis(x, coeff=0.97):
    """float32 in, float32 out, two roundings: s[n] = fl(x[n] - fl(coeff * x[n-1]))."""
    x = np.asarray(x, dtype=np.float32)
    return np.append(x[0], x[1:] - np.float32(coeff) * x[:-1]).astype(np.float32)


def framesig(sig, frame_len, frame_step):
    slen = len(sig)
    n = 1 if slen <= frame_len else 1 + int(math.ceil((1.0 * slen - frame_len) / frame_step))
    padlen = int((n - 1) * frame_step + frame_len)
    padded = np.concatenate((sig, np.zeros(padlen - slen, dtype=sig.dtype)))
    idx = np.arange(frame_len)[None, :] + (np.arange(n) * frame_step)[:, None]
    return padded[idx]


def hz2mel(hz):
    return 2595 * np.log10(1 + hz / 700.)


def mel2hz(mel):
    return 700 * (10 ** (mel / 2595.0) - 1)


def filterbank_bins(samplerate, nfft=512, nfilt=128):
    melpoints = np.linspace(hz2mel(0), hz2mel(samplerate / 2), nfilt + 2)
    return np.floor((nfft + 1) * mel2hz(melpoints) / samplerate)


def filterbank(samplerate, nfft=512, nfilt=128):
    bins = filterbank_bins(samplerate, nfft, nfilt)
    fb = np.zeros([nfilt, nfft // 2 + 1])
    for j in range(nfilt):
        for i in range(int(bins[j]), int(bins[j + 1])):
            fb[j, i] = (i - bins[j]) / (bins[j + 1] - bins[j])
        for i in range(int(bins[j + 1]), int(bins[j + 2])):
            fb[j, i] = (bins[j + 2] - i) / (bins[j + 2] - bins[j + 1])
    return fb


def dct_ortho(nfilt, numcep):
    """[numcep, nfilt]: the rows of a type-II DCT with norm='ortho'."""
    n = np.arange(numcep)[:, None]
    j = np.arange(nfilt)[None, :]
    m = np.cos(np.pi * n * (2 * j + 1) / (2.0 * nfilt))
    m[0] *= np.sqrt(1.0 / nfilt)
    m[1:] *= np.sqrt(2.0 / nfilt)
    return m


def lifter(cepstra, L=22):
    n = np.arange(cepstra.shape[1])
    return cepstra * (1 + (L / 2.) * np.sin(np.pi * n / L))


def mfcc(audio, samplerate, numcep, nfilt=128, nfft=512, winlen=0.025, winstep=0.01, preemph=0.97, ceplifter=22):
    """psf 0.6 mfcc(appendEnergy=True, winfunc=ones) on float32 audio; float64 [T, numcep]."""
    sig = preemphasis(audio, preemph)
    frame_len, frame_step = frame_params(samplerate, winlen, winstep)
    frames = framesig(sig, frame_len, frame_step)
    # float64 FFT, as psf got it from NumPy 1.x (NumPy 2 keeps float32 input in single precision)
    pspec = 1.0 / nfft * np.square(np.absolute(np.fft.rfft(frames.astype(np.float64), nfft)))
    energy = np.sum(pspec, 1)
    energy = np.where(energy == 0, EPS, energy)
    feat = np.dot(pspec, filterbank(samplerate, nfft, nfilt).T)
    feat = np.where(feat == 0, EPS, feat)
    feat = np.log(feat) @ dct_ortho(nfilt, numcep).T
    feat = lifter(feat, ceplifter)
    feat[:, 0] = np.log(energy)
    return feat


def include_context(feat, numcontext):
    T, C = feat.shape
    pad = np.zeros((numcontext, C), dtype=feat.dtype)
    ext = np.concatenate((pad, feat, pad))
    return np.concatenate([ext[w:w + T] for w in range(2 * numcontext + 1)], axis=1)


def features(audio, samplerate, numcontext, numcep, nfilt=128):
    """utils.convert_to_mfcc after librosa.load: float32 [T, (2*numcontext+1)*numcep], and (mean, std)."""
    x = mfcc(audio, samplerate, numcep, nfilt=nfilt)
    if numcontext > 0:
        x = include_context(x, numcontext)
    mean, std = np.mean(x), np.std(x)
    return ((x - mean) / std).astype(np.float32), (mean, std)
