"""References, cases and the error bound of tests/test_gpu_ctc_kernels.py (the CTC kernels of csrc/ctc.hip, launch by launch).

fp64: oracle.nasr_oracle (ctc_single, log_softmax, greedy_decode).  fp32: ctc_fp32, recursion (2) of csrc/ctc.hip in NumPy
float32 with correctly rounded exp and log - the error the lattice's arithmetic alone makes; tools/ctc_fp32_model.py prints
it for the long cases of test_gpu_ctc_lattice.py.  Its `mutant=` options are wrong models of the lattice: test_ctc_ref_host.py
shows that check() rejects each of them.

The bound of one launch (check): with E_model / N_model the largest absolute error of the fp32 model's logit gradient / log p
against fp64 over the batch, every element of the kernel's gradient is within FACTOR * E_model + GRAD_ABS of fp64 and every
log p within FACTOR * N_model + 2^-22 |log p|.  Both come from the references alone."""
from collections import namedtuple

import numpy as np

from oracle import nasr_oracle as O

F32 = np.float32
NEG = F32(-1e30)

# The kernels' error in units of the fp32 model's.  The record of test_gpu_ctc_lattice.py is that both walks land at about
# twice the model; 4 is that ratio with a factor of 2 of headroom.
# Largest multiples measured on the MI355X over every case of test_gpu_ctc_kernels.py: MEASURED (the gradient's at
# instance-Lmax32-C29, engineered walk; log p's at sweep-T65..128-C29-flat, plain walk).
FACTOR = 4.0
MEASURED = {'gradient': 2.34, 'logp': 2.31}
# y = exp(x - logZ) has arguments <= 0: an argument error of |a| 2^-23 is an absolute error of at most 2^-23 / e whatever the
# logits' magnitude; a few ulp of v_exp_f32 come on top
GRAD_ABS = 1e-6
E_MODEL_CAP = 1e-3                              # a looser model would make the bound meaningless: asserted on every batch
# one rounding of the final add; a sum of at most 300 terms exp(x - m) in [0,1], each a few ulp off; log of a value in [1, C]
LOGZ_REL, LOGZ_ABS = 2.0 ** -23, 4e-6

MUTANTS = ('post_1pct', 'skip_equal', 'beta_emits', 'drop_last_group', 'ring_shift', 'blank0', 'tail_grad')


def lse3(a, b, c):
    m = np.maximum(a, np.maximum(b, c))
    return (m + np.log(np.exp(a - m) + np.exp(b - m) + np.exp(c - m))).astype(F32)


def ctc_fp32(logits, label, blank, G=4, mutant=None):
    """(nll, d nll / d logits) of one utterance, logits [T, C], as recursion (2) computes them in fp32: log domain, columns
    rescaled by their maximum every G frames, fp64 offsets.  mutant: one of MUTANTS (a wrong model), or None.
      post_1pct        the posterior of frame T // 2 is 1 % too large
      skip_equal       the skip transition is allowed between equal labels
      beta_emits       beta includes the emission at t
      drop_last_group  a last, partial group of G frames loses its last frame: the state is frozen one frame early
      ring_shift       from position 64 on, position p reads the emission of position p + 1 (a ring row handed over early)
      blank0           the blank is class 0
    (tail_grad is a mutant of the batch: model_batch.)"""
    x = np.asarray(logits, F32)
    T, C = x.shape
    if mutant == 'blank0':
        blank = 0
    mx = x.max(1, keepdims=True)
    z = (mx[:, 0] + np.log(np.exp(x - mx).sum(1))).astype(F32)
    L = len(label)
    S = 2 * L + 1
    ext = np.full(S, blank)
    ext[1::2] = label
    e = (x[:, ext] - z[:, None]).astype(F32)
    skip = np.zeros(S, bool)
    skip[2:] = (ext[2:] != blank) & (ext[2:] != ext[:-2])
    if mutant == 'skip_equal':
        skip[2:] = ext[2:] != blank
    skip_f = np.zeros(S, bool)
    skip_f[:-2] = skip[2:]
    npos = T - 1
    dead = npos - 1 if mutant == 'drop_last_group' and npos % G else -1      # the position that leaves the state alone
    shift = 1 if mutant == 'ring_shift' else 0

    def rescale(v, off):
        m = v.max()
        return np.where(v > NEG / 2, v - m, NEG).astype(F32), off + float(m)
    al, ao = np.full((T, S), NEG, F32), np.zeros(T)
    a, A = np.full(S, NEG, F32), 0.0
    a[:2] = e[0, :2]
    al[0] = a
    for t in range(1, T):
        p = t - 1
        if p % G == 0:
            a, A = rescale(a, A)
        if p != dead:
            et = e[min(t + shift, T - 1)] if p >= 64 else e[t]
            a1 = np.concatenate([[NEG], a[:-1]]).astype(F32)
            a2 = np.where(skip, np.concatenate([[NEG, NEG], a])[:S], NEG).astype(F32)
            a = (et + lse3(a, a1, a2)).astype(F32)
        al[t], ao[t] = a, A
    be, bo = np.full((T, S), NEG, F32), np.zeros(T)
    b, Bo = np.full(S, NEG, F32), 0.0
    b[max(S - 2, 0):] = 0
    be[T - 1] = b
    for t in range(T - 2, -1, -1):
        p = T - 2 - t
        if p % G == 0:
            b, Bo = rescale(b, Bo)
        if p != dead:
            et = e[max(t + 1 - shift, 0)] if p >= 64 else e[t + 1]
            bb = (b + et).astype(F32)
            b1 = np.concatenate([bb[1:], [NEG]]).astype(F32)
            b2 = np.where(skip_f, np.concatenate([bb, [NEG, NEG]])[2:], NEG).astype(F32)
            b = lse3(bb, b1, b2)
        be[t], bo[t] = b, Bo
    logp = A + float(lse3(a[S - 1], a[S - 2] if S > 1 else NEG, NEG))
    be64 = be.astype(np.float64) + (e if mutant == 'beta_emits' else 0.0)
    with np.errstate(over='ignore'):          # (a mutant's weights may overflow: check() reports the inf)
        w = np.exp(al.astype(np.float64) + be64 + (ao + bo - logp)[:, None])
    post = np.zeros((T, C))
    for s in range(S):
        post[:, ext[s]] += w[:, s]
    if mutant == 'post_1pct':
        post[T // 2] *= 1.01
    return -logp, np.exp(x.astype(np.float64) - z[:, None]) - post


# ------------------------------------------------------------------ cases
# logits [Tp][B][C] float64 holding float32 values (zeros from seq_len[b] on), labels [B][Lmax] with class 0 behind label_len
Case = namedtuple('Case', 'id C B Tp Lmax seq_len labels label_len logits')


def one_class_label(rs, L, C):
    return [int(rs.randint(0, C - 1))] * L


def pinned(rs, T, Lcap, C):
    """A label that needs every one of its T frames (L + repeats = T) where Lcap labels can (T <= 2 Lcap - 1); else Lcap
    labels with a random number of repeats."""
    if C == 2:
        return [0] * min(Lcap, (T + 1) // 2)
    if T <= 2 * Lcap - 1:
        L = min(Lcap, T - (T - 1) // 4) if T > 1 else 1       # three quarters labels, one quarter repeats ...
        L = max(L, (T + 2) // 2)                               # ... as far as L - 1 repeats reach
        return O.pinned_label(rs, L, T - L, C)
    return O.pinned_label(rs, Lcap, int(rs.randint(0, Lcap)), C)


def random_label(rs, L, C):
    return rs.randint(0, C - 1, L).tolist()


def alignment(rs, label, T, blank):
    """One path of T frames that collapses to `label`: every label at least once, a blank between equal neighbours, the
    other blanks optional."""
    L = len(label)
    ext = np.full(2 * L + 1, blank)
    ext[1::2] = label
    least = np.zeros(2 * L + 1, int)
    least[1::2] = 1
    for i in range(1, L):
        if label[i] == label[i - 1]:
            least[2 * i] = 1
    extra = T - least.sum()
    assert extra >= 0, 'infeasible label'
    return np.repeat(ext, least + rs.multinomial(extra, np.full(2 * L + 1, 1.0 / (2 * L + 1))))


def make_logits(rs, regime, seq_len, labels, label_len, Tp, C):
    """flat: randn.  sharp: a dominant class per frame along an alignment, margin 10 (even slots) and 20 (odd slots).
    sharp_improbable: the same, and up to three label frames per utterance where the label's class is 20 BELOW the rest
    (the case ctc.hip describes above its engineered walk).  mag: 30 randn, logits to about +-90.
    Rounded through fp32 before either reference sees them."""
    B = len(seq_len)
    x = np.zeros((Tp, B, C))
    for b in range(B):
        Tb = int(seq_len[b])
        v = rs.randn(Tb, C) * (30.0 if regime == 'mag' else 1.0)
        if regime in ('sharp', 'sharp_improbable'):
            path = alignment(rs, list(labels[b, :label_len[b]]), Tb, C - 1)
            v[np.arange(Tb), path] += 10.0 if b % 2 == 0 else 20.0
            at = np.flatnonzero(path != C - 1)
            if regime == 'sharp_improbable' and len(at):
                for t in rs.choice(at, min(3, len(at)), replace=False):
                    v[t] = rs.randn(C)
                    v[t, path[t]] -= 20.0
        x[:Tb, b] = v
    return x.astype(F32).astype(np.float64)


def _case(id_, rs, regime, C, Tp, Lmax, seq_len, labs):
    B = len(seq_len)
    labels = np.zeros((B, Lmax), np.int32)
    label_len = np.array([len(lab) for lab in labs], np.int32)
    for b, lab in enumerate(labs):
        labels[b, :len(lab)] = lab
    seq_len = np.asarray(seq_len, np.int32)
    return Case(id_, C, B, Tp, Lmax, seq_len, labels, label_len, make_logits(rs, regime, seq_len, labels, label_len, Tp, C))


def sweep_case(base, C, regime, n=64):
    """Slot b holds seq_len = base + b + 1: every length of a span of 64 in one launch.  Labels: random, lengths in
    [0, min(24, T // 2)], every eighth one pinned."""
    rs = np.random.RandomState(1000 * base + 10 * C + len(regime))
    seq_len = base + 1 + np.arange(n)
    labs = []
    for b, T in enumerate(seq_len):
        labs.append(pinned(rs, int(T), 24, C) if b % 8 == 7 else
                    random_label(rs, int(rs.randint(0, min(24, T // 2) + 1)), C))
    return _case(f'sweep-T{base + 1}..{base + n}-C{C}-{regime}', rs, regime, C, base + n + 5, 24, seq_len, labs)


INSTANCE_LMAX = (32, 64, 96, 128, 160, 192, 224, 256, 384, 511)       # the lower-edge width of every KS, and the widest


def states_per_lane(Lmax):
    """ctc_states_per_lane of csrc/kernels.h"""
    ks = (2 * Lmax + 1 + 63) // 64
    return 2 if ks <= 1 else ks if ks <= 8 else 12 if ks <= 12 else 16 if ks <= 16 else ks


def instance_case(Lmax, C):
    """One lattice instantiation: a full-width label, Lmax // 4, an empty label, L = 1, a pinned label and a one-class label
    of length Lmax // 2 in T = min(1100, 2 Lmax + 40) frames, ragged."""
    rs = np.random.RandomState(7 * Lmax + C)
    T = min(1100, 2 * Lmax + 40)
    Lp = Lmax // 3
    labs = [random_label(rs, Lmax, C), random_label(rs, Lmax // 4, C), [], random_label(rs, 1, C),
            O.pinned_label(rs, Lp, Lp // 4, C), one_class_label(rs, Lmax // 2, C)]
    rep0 = sum(1 for a, b in zip(labs[0][:-1], labs[0][1:]) if a == b)
    assert Lmax + rep0 <= T
    seq_len = [T, T - 3, T // 2 + 1, 7, Lp + Lp // 4, T - 1]
    return _case(f'instance-Lmax{Lmax}-C{C}', rs, 'sharp_improbable', C, T, Lmax, seq_len, labs)


CLASS_COUNTS = (2, 3, 31, 32, 33, 64, 65, 300)


def classes_case(C):
    """B 5 in T 40: a random label, a pinned one, an empty one, L = 1 and a one-class label (at C 2 every label is class 0,
    kept to T >= 2 L - 1)."""
    rs = np.random.RandomState(300 + C)
    seq_len = [40, 33, 17, 5, 39]
    labs = [random_label(rs, 12, C) if C > 2 else [0] * 9, pinned(rs, 33, 24, C), [], random_label(rs, 1, C), one_class_label(rs, 14, C)]
    return _case(f'classes-C{C}', rs, 'flat', C, 40, 24, seq_len, labs)


def small_case(C, Lmax=24, tail=4):
    """The base case of the exact tests: B 5 (Bp 16), ragged, Tp = the longest length + tail."""
    rs = np.random.RandomState(50 + C + Lmax)
    seq_len = [70, 1, 37, 66, 9]
    labs = [random_label(rs, 20, C), [], pinned(rs, 37, 24, C), random_label(rs, 1, C), one_class_label(rs, 4, C)]
    return _case(f'small-C{C}-Lmax{Lmax}', rs, 'flat', C, 70 + tail, Lmax, seq_len, labs)


def sweep_cases():
    """(case, walks): the launches of the every-length and the magnitude tests; walks = which of 'engineered' / 'plain' run it."""
    out = []
    for C, walks in ((29, ('engineered', 'plain')), (40, ('plain',))):
        for regime in ('flat', 'sharp'):
            out += [(sweep_case(base, C, regime), walks) for base in (0, 64, 128)]
        out.append((sweep_case(0, C, 'mag'), walks))
    return out


def instance_cases():
    return [instance_case(Lmax, C) for Lmax in INSTANCE_LMAX for C in (29, 40)]


def classes_cases():
    return [(classes_case(C), ('engineered', 'plain') if C <= 31 else ('plain',)) for C in CLASS_COUNTS]


def feasible(case):
    """Nothing validate_batch would refuse: what the harness accepts."""
    c = case
    ok = 1 <= c.B <= 64 and c.C >= 2 and c.Lmax >= 1 and c.labels.shape == (c.B, c.Lmax) and c.logits.shape == (c.Tp, c.B, c.C)
    for b in range(c.B):
        lab = c.labels[b, :c.label_len[b]]
        ok &= 1 <= c.seq_len[b] <= c.Tp and 0 <= c.label_len[b] <= c.Lmax
        ok &= bool(np.all((c.labels[b] >= 0) & (c.labels[b] <= c.C - 2))) and O.ctc_feasible(lab, int(c.seq_len[b]))
        ok &= not c.logits[c.seq_len[b]:, b].any()
    return bool(ok) and np.array_equal(c.logits, c.logits.astype(F32))


# ------------------------------------------------------------------ references of a case, computed once
def model_batch(case, mutant=None):
    """The fp32 model over a batch -> (gradient [Tp][B][C] of the summed nll, logp [B]).  mutant 'tail_grad': the frames
    from seq_len[b] on keep y - 0 instead of 0."""
    c = case
    g, logp = np.zeros((c.Tp, c.B, c.C)), np.zeros(c.B)
    for b in range(c.B):
        Tb = int(c.seq_len[b])
        nll, g[:Tb, b] = ctc_fp32(c.logits[:Tb, b], c.labels[b, :c.label_len[b]], c.C - 1, mutant=None if mutant == 'tail_grad' else mutant)
        logp[b] = -nll
        if mutant == 'tail_grad':
            g[Tb:, b] = np.exp(O.log_softmax(c.logits[Tb:, b]))
    return g, logp


_refs = {}


def reference(case):
    """fp64 gradient [Tp][B][C], logp [B], logz [Tp][B] (NaN where no row is computed), and the fp32 model's errors."""
    if case.id not in _refs:
        c = case
        nll, g64 = O.ctc_loss_and_grad(c.logits, c.labels, c.label_len, c.seq_len)
        logz = c.logits.max(-1) - O.log_softmax(c.logits).max(-1)
        logz[np.arange(c.Tp)[:, None] >= c.seq_len[None, :]] = np.nan
        g32, logp32 = model_batch(c)
        for a in (g64, logz):
            a.setflags(write=False)
        _refs[c.id] = dict(grad=g64, logp=-nll, logz=logz, E_model=float(np.abs(g32 - g64).max()),
                           N_model=float(np.abs(logp32 + nll).max()))
    return _refs[case.id]


def check(case, grad, logp):
    """Holds a launch's gradient [Tp][B][C] (of the summed nll: the kernel's divided by its scale) and logp [B] to the bound.
    -> (problems, the gradient's largest error in units of E_model, log p's in units of N_model)."""
    ref = reference(case)
    problems = []
    eg = np.abs(np.asarray(grad, np.float64) - ref['grad'])
    el = np.abs(np.asarray(logp, np.float64) - ref['logp'])
    if not (np.isfinite(eg).all() and np.isfinite(el).all()):
        return ['a result is not finite'], np.inf, np.inf
    bound_g = FACTOR * ref['E_model'] + GRAD_ABS
    if eg.max() > bound_g:
        t, b, k = np.unravel_index(eg.argmax(), eg.shape)
        problems.append(f'gradient of (t {t}, b {b}, class {k}; seq_len {case.seq_len[b]}, L {case.label_len[b]}) is {eg.max():.3g} '
                        f'off, bound {bound_g:.3g} (E_model {ref["E_model"]:.3g})')
    bound_l = FACTOR * ref['N_model'] + 2.0 ** -22 * np.abs(ref['logp'])
    if (el > bound_l).any():
        b = int((el - bound_l).argmax())
        problems.append(f'logp of utterance {b} (seq_len {case.seq_len[b]}, L {case.label_len[b]}) is {el[b]:.3g} off, bound {bound_l[b]:.3g}')
    return problems, eg.max() / max(ref['E_model'], 1e-300), el.max() / max(ref['N_model'], 1e-300)


def check_logz(case, logz):
    """logz [Tp][B] of the computed rows against fp64 -> problems"""
    ref = reference(case)['logz']
    v = ~np.isnan(ref)
    err = np.abs(np.asarray(logz, np.float64)[v] - ref[v])
    bad = err > LOGZ_REL * np.abs(ref[v]) + LOGZ_ABS
    return [f'logZ: {int(bad.sum())} rows beyond the bound, the worst {err.max():.3g} off'] if bad.any() or not np.isfinite(err).all() else []
