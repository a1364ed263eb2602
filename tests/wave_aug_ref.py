"""The rules of the waveform augmentation (nasr_wave_aug in include/nasr.h) restated in NumPy float64:
what tests/test_gpu_wave_aug.py holds the kernels of neuralasr_amd/csrc/wave_aug.hip against.  The project's own rules,
with no counterpart in the reference."""
import numpy as np

U = 2.0 ** -24            # the unit roundoff of float32


def fir(x, h):
    """(y, bound terms): y[t] = sum_{k=0..min(K-1,t)} h[k] x[t-k] for t in [0, N), in float64 from the float32 inputs, and
    sum_k |h[k] x[t-k]| for the error bound of a float32 dot product"""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    h = np.asarray(h, dtype=np.float32).astype(np.float64)
    n = x.size
    return np.convolve(x, h)[:n], np.convolve(np.abs(x), np.abs(h))[:n]


def gamma(k):
    """the standard bound factor of a length-k float32 dot product, any order of summation"""
    return k * U / (1.0 - k * U)


def noise_track(clip, off, n):
    """n[t] = c[(o + t) mod L]"""
    clip = np.asarray(clip, dtype=np.float32)
    return clip[(int(off) + np.arange(n, dtype=np.int64)) % clip.size]


def gain64(y, n, snr_db):
    """g = sqrt(Ps / Pn) 10^(-snr_db / 20) in float64, 0 when Ps or Pn is 0"""
    ps = float(np.sum(np.asarray(y, np.float64) ** 2))
    pn = float(np.sum(np.asarray(n, np.float64) ** 2))
    if ps == 0.0 or pn == 0.0:
        return 0.0
    return float(np.sqrt(ps / pn) * 10.0 ** (-float(snr_db) / 20.0))


def mix(y, clip, off, snr_db):
    """(z, g, n): z[t] = y[t] + g n[t] in float64 with g rounded once to float32"""
    y = np.asarray(y, dtype=np.float32)
    n = noise_track(clip, off, y.size)
    g = np.float32(gain64(y, n, snr_db))
    return y.astype(np.float64) + np.float64(g) * n.astype(np.float64), g, n


def snr_db(speech, noise):
    """10 log10(Ps / Pn) of a speech and a noise track, in float64"""
    return 10.0 * np.log10(float(np.sum(np.asarray(speech, np.float64) ** 2)) / float(np.sum(np.asarray(noise, np.float64) ** 2)))
