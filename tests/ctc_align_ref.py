"""NumPy fp64 restatement of CTC forced alignment, the yardstick of the alignment tests.

For one utterance with logits x [F, C] (blank = C-1) and a label l of length L: the extended label l' has S = 2L+1 states,
blank at even s, l[(s-1)/2] at odd s.  A path pi(0..F-1) starts in {0, 1}, ends in {S-1, S-2} ({0} when L = 0) and moves by
0, 1 or 2 states per frame, 2 only onto a non-blank state that differs from the state two below.  The alignment maximises
sum_t x(t, l'_pi(t)).  Ties: among equal predecessors stay (s), then s-1, then s-2; among equal end states S-1.

    v(s, 0) = x(0, l'_s) for s < 2, -inf otherwise
    v(s, t) = x(t, l'_s) + max(v(s, t-1), v(s-1, t-1), [v(s-2, t-1)])

Before the frames t = 1, 5, 9, ... the maximum of column t-1 is subtracted from the whole column (`rescale_every` = 4; 0:
never).  That value is itself a sum / maximum of logits, so it changes no comparison in exact arithmetic, and it keeps
integer logits integer.  The score is the natural-log probability of the path, sum_t (x(t, l'_pi(t)) - logZ(t))."""
import numpy as np


def extended(label, blank):
    ext = np.full(2 * len(label) + 1, blank, np.int64)
    ext[1::2] = np.asarray(label, np.int64)
    return ext


def logz_rows(x):
    x = np.asarray(x, np.float64)
    m = x.max(axis=1)
    return m + np.log(np.exp(x - m[:, None]).sum(axis=1))


def path_score(x, label, path):
    """sum_t (x(t, l'_path(t)) - logZ(t)) in fp64"""
    x = np.asarray(x, np.float64)
    ext = extended(label, x.shape[1] - 1)
    path = np.asarray(path, np.int64)
    return float((x[np.arange(len(path)), ext[path]] - logz_rows(x)).sum())


def path_sum(x, label, path):
    """sum_t x(t, l'_path(t)) in fp64: what the alignment maximises"""
    x = np.asarray(x, np.float64)
    ext = extended(label, x.shape[1] - 1)
    path = np.asarray(path, np.int64)
    return float(x[np.arange(len(path)), ext[path]].sum())


def is_valid_path(path, label, blank):
    ext = extended(label, blank)
    S = len(ext)
    path = [int(p) for p in path]
    if not path or path[0] not in (0, 1) or path[0] >= S:
        return False
    if path[-1] not in (S - 1, S - 2) or path[-1] < 0:
        return False
    for a, b in zip(path[:-1], path[1:]):
        d = b - a
        if d not in (0, 1, 2) or b >= S:
            return False
        if d == 2 and (ext[b] == blank or ext[b] == ext[b - 2]):
            return False
    return True


def feasible(label, F):
    rep = sum(1 for i in range(1, len(label)) if label[i] == label[i - 1])
    return len(label) + rep <= F


def align(x, label, rescale_every=4):
    """(path int64 [F], score, max |v| met, smallest gap between the winner and the runner-up over every decision on the path)

    The gap is +inf where a decision had one candidate only; decisions are those of the traced path: each frame's choice
    of predecessor and the choice of the end state."""
    x = np.asarray(x, np.float64)
    F, C = x.shape
    blank = C - 1
    ext = extended(label, blank)
    S = len(ext)
    if not feasible(list(label), F):
        raise ValueError('Not enough time for target transition sequence')
    skip = np.zeros(S, bool)
    for s in range(2, S):
        skip[s] = ext[s] != blank and ext[s] != ext[s - 2]
    v = np.full(S, -np.inf)
    v[:min(2, S)] = x[0, ext[:min(2, S)]]
    bp = np.zeros((F, S), np.int64)
    gap = np.full((F, S), np.inf)
    vmax = float(np.abs(v[np.isfinite(v)]).max())
    ninf1, ninf2 = np.full(1, -np.inf), np.full(2, -np.inf)
    for t in range(1, F):
        if rescale_every and (t - 1) % rescale_every == 0:
            v = v - v.max()              # -inf stays -inf
            vmax = max(vmax, float(np.abs(v[np.isfinite(v)]).max()))
        stay = v
        one = np.concatenate([ninf1, v[:-1]])
        two = np.where(skip, np.concatenate([ninf2, v[:-2]])[:S], -np.inf)
        best, c = stay, np.zeros(S, np.int64)              # stay wins ties, then s-1, then s-2: strict > in that order
        take = one > best
        best, c = np.where(take, one, best), np.where(take, 1, c)
        take = two > best
        best, c = np.where(take, two, best), np.where(take, 2, c)
        bp[t] = c
        live = np.isfinite(best)
        second = np.sort(np.stack([stay, one, two]), axis=0)[1]
        with np.errstate(invalid='ignore'):
            gap[t] = np.where(live, best - second, np.inf)
        v = np.where(live, best + x[t, ext], -np.inf)
        vmax = max(vmax, float(np.abs(v[live]).max()))
    s = S - 1
    mingap = np.inf
    if S > 1:
        if v[S - 2] > v[S - 1]:
            s = S - 2
        mingap = abs(v[S - 1] - v[S - 2])
    path = np.zeros(F, np.int64)
    for t in range(F - 1, -1, -1):
        path[t] = s
        if t > 0:
            mingap = min(mingap, gap[t, s])
            s -= bp[t, s]
    return path, path_score(x, label, path), vmax, float(mingap)


def enumerate_paths(label, F, blank):
    """every valid path of F frames, by exhaustive search (tiny shapes only)"""
    ext = extended(label, blank)
    S = len(ext)
    out = []

    def go(path):
        if len(path) == F:
            if path[-1] in (S - 1, S - 2):
                out.append(list(path))
            return
        a = path[-1]
        for d in (0, 1, 2):
            b = a + d
            if b >= S:
                continue
            if d == 2 and (ext[b] == blank or ext[b] == ext[b - 2]):
                continue
            go(path + [b])

    for s0 in (0, 1):
        if s0 < S:
            go([s0])
    return out
