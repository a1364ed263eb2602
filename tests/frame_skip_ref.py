"""The numpy side of the frame-skip tests.  The batch funnel's output under a skip is a copy, so a handle
with skip s given the input X computes the bits of a handle with skip 1 given the host-made rows of the kept frames:
include_context on the utterance, rows [::s], zeros from the network length on, uploaded in the full form with the network
lengths and T' = ceil(T/s).  Everything here makes those rows, or the inputs they are made from."""
import numpy as np

from neuralasr_amd.utils import include_context


def net_len(n, s):
    """the frames the network sees of n input frames: frames 0, s, 2s, ..."""
    return len(range(0, int(n), int(s)))


def stack(utt, numcontext, numcep, pad=0.0):
    """include_context on one utterance's centre frames [len, numcep]; windows beyond its ends hold `pad` (include_context
    itself leaves zeros there: the pad value of an utterance that was not normalised)"""
    utt = np.asarray(utt, np.float32)
    out = include_context(utt, numcontext, numcep)
    if pad != 0.0:
        n, w = utt.shape[0], 2 * numcontext + 1
        src = np.arange(n)[:, None] + np.arange(w) - numcontext
        out = out.reshape(n, w, numcep).copy()
        out[(src < 0) | (src >= n)] = np.float32(pad)
        out = out.reshape(n, w * numcep)
    return out


def padded(rows, T):
    """[B, T, F] from per-utterance rows, zeros behind each"""
    out = np.zeros((len(rows), T, rows[0].shape[1]), np.float32)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out


def input_batch(utts, numcontext, numcep, T, pads=None):
    """the caller's batch in the full form: stacked rows [B, T, F] and the input lengths"""
    pads = [0.0] * len(utts) if pads is None else pads
    return padded([stack(u, numcontext, numcep, p) for u, p in zip(utts, pads)], T), [len(u) for u in utts]


def kept_batch(utts, numcontext, numcep, T, s, pads=None):
    """what the network sees of it: the kept rows [B, ceil(T/s), F] and the network lengths"""
    pads = [0.0] * len(utts) if pads is None else pads
    rows = [stack(u, numcontext, numcep, p)[::s] for u, p in zip(utts, pads)]
    assert [r.shape[0] for r in rows] == [net_len(len(u), s) for u in utts]
    return padded(rows, net_len(T, s)), [r.shape[0] for r in rows]


def masked(utts, static_width, time_masks, freq_masks):
    """SpecAugment on the centre frames: masked values are 0.  time_masks [B, nt, 2] of (first frame,
    width), freq_masks [B, nf, 2] of (first column of every static_width-wide block, width)."""
    out = []
    for b, u in enumerate(utts):
        u = np.array(u, np.float32)
        for t0, tw in time_masks[b]:
            u[t0:t0 + tw] = 0.0
        cols = np.arange(u.shape[1]) % static_width
        for f0, fw in freq_masks[b]:
            u[:, (cols >= f0) & (cols < f0 + fw)] = 0.0
        out.append(u)
    return out


def feed_kept(phase, n, s):
    """a stream slot that has had `phase` (mod s) input rows gets n more: (indices of the new rows that are kept, phase
    after) - by the rule itself, index in the utterance a multiple of s"""
    idx = [i for i in range(n) if (phase + i) % s == 0]
    return idx, (phase + n) % s
