"""fp64 NumPy restatement of librosa 0.6-0.9's resample(y, sr_orig, sr_new, res_type='kaiser_best') (resampy 0.2's
resample_f on its kaiser_best filter, then fix_length), the yardstick of the GPU resampler (csrc/resample.hip).

Vectorised over output samples; the taps run in a Python loop with masks, left wing i = 0.. then right wing k = 0..,
so every output sums its taps in resampy's order.  `acc='f32'` rounds the sum to float32 after every tap, as resampy's
float32 output array does; `acc='f64'` keeps it in float64.  The time register is resampy's sequential
`tr += 1 / ratio`, which np.cumsum reproduces bit for bit."""
import numpy as np

NUM_ZEROS = 64
NUM_TABLE = 512                     # 2 ** precision, precision 9
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
NWIN = NUM_ZEROS * NUM_TABLE + 1    # 32769


def table():
    """resampy.filters.sinc_window(64, 9, kaiser(beta), rolloff): float64 [32769]."""
    import scipy.signal
    n = NUM_TABLE * NUM_ZEROS
    sinc = ROLLOFF * np.sinc(ROLLOFF * np.linspace(0, NUM_ZEROS, num=n + 1, endpoint=True))
    return sinc * scipy.signal.windows.kaiser(2 * n + 1, BETA)[n:]


def lengths(n, sr_orig, sr_new):
    """(librosa's ceil(n * ratio), resampy's int(n * ratio)); resampy raises when the second is < 1."""
    ratio = float(sr_new) / sr_orig
    return int(np.ceil(n * ratio)), int(n * ratio)


def register(n_out, ratio):
    """resampy's time register at every output: 0, then `tr += 1 / ratio` in float64."""
    inc = 1.0 / ratio
    tr = np.full(n_out, inc, dtype=np.float64)
    tr[0] = 0.0
    return np.cumsum(tr)


def resample_f(x, sr_orig, sr_new, win=None, acc='f32'):
    """resampy.resample(x, sr_orig, sr_new, filter='kaiser_best') on float32 x: float32 [int(n * ratio)]."""
    x = np.asarray(x, dtype=np.float32)
    ratio = float(sr_new) / sr_orig
    n_out = int(x.size * ratio)
    if n_out < 1:
        raise ValueError('input signal too short to resample from %d to %d Hz' % (sr_orig, sr_new))
    win = table() if win is None else np.array(win, dtype=np.float64)
    if ratio < 1:
        win *= ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    scale = min(1.0, ratio)
    step = int(scale * NUM_TABLE)
    xd = x.astype(np.float64)
    tr = register(n_out, ratio)
    n = tr.astype(np.int64)
    y = np.zeros(n_out, dtype=np.float32 if acc == 'f32' else np.float64)

    def wing(frac, count, src):
        idx = frac * NUM_TABLE
        off = idx.astype(np.int64)
        eta = idx - off
        cnt = np.minimum(count, (NWIN - off) // step)
        for i in range(int(cnt.max()) if cnt.size else 0):
            m = i < cnt
            j = np.where(m, off + i * step, 0)
            w = win[j] + eta * delta[j]
            v = w * xd[np.where(m, src(i), 0)]
            if acc == 'f32':
                y[m] = (y[m].astype(np.float64) + v[m]).astype(np.float32)
            else:
                y[m] += v[m]

    frac = scale * (tr - n)
    wing(frac, n + 1, lambda i: n - i)
    wing(scale - frac, x.size - n - 1, lambda i: n + 1 + i)
    return y


def resample(x, sr_orig, sr_new, win=None, acc='f32'):
    """librosa.resample(x, sr_orig, sr_new) (fix=True, scale=False): resampy's output zero-padded to
    ceil(n * ratio), float32; x itself when the rates agree."""
    x = np.asarray(x, dtype=np.float32)
    if sr_orig == sr_new:
        return x
    n_samples, _ = lengths(x.size, sr_orig, sr_new)
    y = resample_f(x, sr_orig, sr_new, win, acc)
    out = np.zeros(n_samples, dtype=np.float32)
    out[:y.size] = y
    return out


def load(channels, sr_orig, sr_new, win=None):
    """librosa.load's steps after decoding: float32 [channels, n] (or [n]) -> to_mono -> resample -> fix_length."""
    y = np.asarray(channels, dtype=np.float32)
    if y.ndim > 1:
        y = np.mean(y, axis=0)
    return resample(y, sr_orig, sr_new, win)
