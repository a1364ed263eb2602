"""The CTC kernels of csrc/ctc.hip, launch by launch through libnasr_kt.so (tests/kernel_harness/ctc_harness.hip): logZ, the
alpha / beta walks in their plain and their engineered form, the gradient, the greedy decoder and the mean - each against
fp64 on logits the test supplies, frame by frame and element by element, and against the contract of csrc/kernels.h on
what a launch reads, ignores, writes and leaves alone.

The bound (tests/ctc_ref.py, check): every element of the gradient within FACTOR * E_model + 1e-6 of fp64, every log p within
FACTOR * N_model + 2^-22 |log p|, E_model / N_model being the error of the fp32 model of the lattice on the same batch.
FACTOR = 4.  Largest multiples measured on the MI355X over all cases of this file: 2.34 x E_model (the gradient, engineered
walk, instance-Lmax32-C29) and 2.31 x N_model (log p, plain walk, sweep-T65..128-C29-flat); the sharp regimes sit at 0.9 to
1.1, the model and the kernels sharing the rounding of x - logZ that dominates there.  Every test prints its own multiples
with the case id (pytest -s)."""
import numpy as np
import pytest

import ctc_ref as R
import kernel_harness as H
from oracle import nasr_oracle as O

pytestmark = pytest.mark.gpu

WORST = {'gradient': 0.0, 'logp': 0.0}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def pack(case, pad=0.0):
    """logits [Tp][Bp][Cp] float32 (pad everywhere outside [Tp][B][C]) and seq_len [Bp]"""
    Bp, Cp = H.rup(case.B, 16), H.rup(case.C, 32)
    x = np.full((case.Tp, Bp, Cp), pad, np.float32)
    x[:, :case.B, :case.C] = case.logits
    sq = np.zeros(Bp, np.int32)
    sq[:case.B] = case.seq_len
    return x, sq


def run(case, walk, scale=1.0, logits=None, labels=None, ws_fill=0xFF):
    x, sq = pack(case)
    return H.ctc_pass(x if logits is None else logits, sq, case.labels if labels is None else labels, case.label_len, case.C,
                      scale=scale, plain=walk == 'plain', ws_fill=ws_fill)


def valid_rows(case):
    Bp = H.rup(case.B, 16)
    v = np.zeros((case.Tp, Bp), bool)
    v[:, :case.B] = np.arange(case.Tp)[:, None] < case.seq_len[None, :]
    return v


def check_structure(case, out):
    """What the contract of kernels.h says about the places nothing is computed for."""
    v = valid_rows(case)
    assert H.untouched(out['logz'])[~v].all(), 'logZ of a row that is not computed was written'
    assert not H.untouched(out['logz'])[v].any()
    assert H.untouched(out['nll'][case.B:]).all() and (bits(out['logp'][case.B:]) == bits(np.array([H.FILL_F64]))[0]).all()
    g = bits(out['grad'])
    assert not g[~v].any(), 'the gradient of a row that is not computed is not +0'
    assert not g[:, :, case.C:].any(), 'the gradient of a padded column is not +0'
    assert np.array_equal(out['nll'][:case.B], (-out['logp'][:case.B]).astype(np.float32))


def run_and_check(case, walk):
    scale = np.float32(1.0 / case.B)                      # the library's factor
    out = run(case, walk, scale=float(scale))
    check_structure(case, out)
    grad = out['grad'][:, :case.B, :case.C].astype(np.float64) / np.float64(scale)
    problems, mg, ml = R.check(case, grad, out['logp'][:case.B])
    problems += R.check_logz(case, out['logz'][:, :case.B])
    ref = R.reference(case)
    print(f'\n{case.id} {walk}: gradient {mg:.2f} x E_model ({ref["E_model"]:.3g}), logp {ml:.2f} x N_model ({ref["N_model"]:.3g})')
    WORST['gradient'], WORST['logp'] = max(WORST['gradient'], mg), max(WORST['logp'], ml)
    print(f'largest so far: gradient {WORST["gradient"]:.2f}, logp {WORST["logp"]:.2f}')
    assert ref['E_model'] <= R.E_MODEL_CAP
    assert not problems, problems


def _ids(cases):
    return [pytest.param(c, w, id=f'{c.id}-{w}') for c, walks in cases for w in walks]


# ------------------------------------------------------------------ against fp64
@pytest.mark.parametrize('case,walk', _ids([(c, w) for c, w in R.sweep_cases() if 'mag' not in c.id]))
def test_every_length(case, walk):
    """seq_len 1 .. 192, one per slot: every residue of the walks' groups of 4, six loader chunks, the ring's reuse."""
    run_and_check(case, walk)


@pytest.mark.parametrize('case', R.instance_cases(), ids=lambda c: c.id)
def test_every_instantiation(case):
    """KS 2 .. 8, 12, 16 at the lower edge of each, and Lmax 511: the engineered walk at C 29, the plain one at C 40."""
    run_and_check(case, 'engineered' if case.C == 29 else 'plain')


@pytest.mark.parametrize('case,walk', _ids(R.classes_cases()))
def test_class_counts(case, walk):
    run_and_check(case, walk)


@pytest.mark.parametrize('case,walk', _ids([(c, w) for c, w in R.sweep_cases() if 'mag' in c.id]))
def test_magnitude(case, walk):
    """logits to +-90: exp(x - logZ) and the emissions x - logZ at arguments of 100 and more"""
    run_and_check(case, walk)


# ------------------------------------------------------------------ exact
BASES = [(29, 'engineered'), (40, 'plain'), (29, 'plain')]


def same(a, b, case):
    """logZ on the computed rows, nll, logp and the gradient, bit for bit"""
    v = valid_rows(case)
    assert np.array_equal(bits(a['logz'])[v], bits(b['logz'])[v])
    assert np.array_equal(bits(a['nll']), bits(b['nll'])) and np.array_equal(bits(a['logp']), bits(b['logp']))
    assert np.array_equal(bits(a['grad']), bits(b['grad']))


@pytest.mark.parametrize('C,walk', BASES)
@pytest.mark.parametrize('what', ['columns', 'rows', 'frames', 'labels', 'workspace'])
def test_what_is_ignored(C, walk, what):
    case = R.small_case(C)
    base = run(case, walk)
    check_structure(case, base)
    x, _ = pack(case)
    labels, ws_fill = case.labels.copy(), 0xFF
    if what == 'columns':
        x[:, :, C:] = np.nan
    elif what == 'rows':
        x[:, case.B:, :] = np.nan
    elif what == 'frames':
        for b in range(case.B):
            x[case.seq_len[b]:, b, :] = np.nan
    elif what == 'labels':
        for b in range(case.B):
            assert not labels[b, case.label_len[b]:].any()
            labels[b, case.label_len[b]:] = C - 2            # in range: nothing a gather could follow out of bounds
    else:
        ws_fill = 0x00
    out = run(case, walk, logits=x, labels=labels, ws_fill=ws_fill)
    check_structure(case, out)
    same(out, base, case)


def placed(utt, slot, B, Tp, Lmax, seed):
    """A batch of B utterances with utterance 0 of `utt` in `slot`, the others random"""
    rs = np.random.RandomState(seed)
    C, T0 = utt.C, int(utt.seq_len[0])
    seq_len = rs.randint(1, Tp + 1, B)
    labs = [R.random_label(rs, int(rs.randint(0, min(Lmax, t // 2) + 1)), C) for t in seq_len]
    seq_len[slot], labs[slot] = T0, utt.labels[0, :utt.label_len[0]].tolist()
    c = R._case(f'placed-{slot}-{B}-{Tp}-{Lmax}', rs, 'flat', C, Tp, Lmax, seq_len, labs)
    c.logits[:, slot] = 0
    c.logits[:T0, slot] = utt.logits[:T0, 0]
    return c


@pytest.mark.parametrize('C,walk', BASES)
def test_placement(C, walk):
    """One utterance gives the same bits wherever it stands: slot and batch size, T' and the label stride."""
    utt = R.small_case(C)                      # its utterance 0: 70 frames, 20 labels
    T0 = 70
    alone = placed(utt, 0, 1, T0, 24, 1)
    ref = run(alone, walk)
    for slot, B, Tp, Lmax in ((16, 17, T0, 24), (63, 64, T0, 24), (0, 1, T0 + 37, 24), (0, 1, T0, 63), (16, 17, T0 + 37, 63)):
        c = placed(utt, slot, B, Tp, Lmax, 2 + slot)
        assert R.feasible(c) and R.states_per_lane(Lmax) == 2
        out = run(c, walk)
        check_structure(c, out)
        assert np.array_equal(bits(out['grad'][:T0, slot]), bits(ref['grad'][:T0, 0])), (slot, B, Tp, Lmax)
        assert np.array_equal(bits(out['logz'][:T0, slot]), bits(ref['logz'][:T0, 0]))
        assert bits(out['nll'])[slot] == bits(ref['nll'])[0] and bits(out['logp'])[slot] == bits(ref['logp'])[0]


@pytest.mark.parametrize('C,walk', BASES)
def test_scale_and_repeatability(C, walk):
    case = R.small_case(C)
    one, again, quarter = run(case, walk), run(case, walk), run(case, walk, scale=0.25)
    for k in one:
        assert np.array_equal(bits(one[k]), bits(again[k])), k
    assert np.array_equal(bits(quarter['grad']), bits(one['grad'] * np.float32(0.25)))
    same(dict(quarter, grad=one['grad']), one, case)


# ------------------------------------------------------------------ greedy
def greedy_logits(T, C, rs):
    """Integer-valued logits [T][4][C] with planted ties, repeats and blanks across the collapse kernel's turns of 64
    frames, and rows that are partly -inf."""
    B, blank = 4, C - 1
    x = rs.randint(-5, 6, (T, B, C)).astype(np.float64)
    seq_len = np.array([T, max(T - 1, 1), max(T // 2, 1), T], np.int32)
    k1, k2 = (0, 0) if C == 2 else (int(rs.randint(0, blank)), int(rs.randint(0, blank)))
    for edge in (64, 128):
        if T > edge:
            x[edge - 1, 0, k1] = x[edge, 0, k1] = 20            # a class repeated across the turn
            x[edge - 1, 1, blank] = x[edge, 1, k2] = 20         # a blank before it
            x[edge - 1, 3, k2] = x[edge, 3, blank] = 20         # a blank behind it
    edges = (63, 64, 127, 128)
    for t in sorted(set(range(0, T, 3)) - set(edges)):
        b = t % B
        if C > 64:
            x[t, b, 0 + t % (C - 64)] = x[t, b, 64 + t % (C - 64)] = 30          # a tie inside a lane: c and c + 64
        if C > 65 and t % 2:
            x[t, b, :] = np.minimum(x[t, b, :], 29)
            x[t, b, 7] = x[t, b, 72] = 30                                        # between neighbouring lanes: c and c + 65
    for t in range(1, T, 4):
        x[t, (t + 1) % B, k1] = x[t, (t + 1) % B, blank] = 40                    # the blank against a label
    for t in sorted(set(range(2, T, 5)) - set(edges)):
        dead = rs.rand(C) < 0.7
        dead[int(rs.randint(0, C))] = False                                      # some, never all
        x[t, t % B, dead] = -np.inf
    return x, seq_len


@pytest.mark.parametrize('C', [2, 29, 64, 65, 300])
def test_greedy_is_exact(C):
    for T in (1, 63, 64, 65, 128, 129, 200):
        rs = np.random.RandomState(1000 * C + T)
        x, seq_len = greedy_logits(T, C, rs)
        want = O.greedy_decode(x, seq_len)
        xp = np.full((T, 16, H.rup(C, 32)), np.nan, np.float32)       # (what is ignored holds NaN)
        xp[:, :4, :C] = x
        for b in range(4):
            xp[seq_len[b]:, b] = np.nan
        sq = np.zeros(16, np.int32)
        sq[:4] = seq_len
        ids, lens = H.ctc_greedy(xp, sq, 4, C)
        assert lens[:4].tolist() == [len(w) for w in want], (C, T)
        assert (lens[4:] == H.FILL_I32).all()
        for b in range(4):
            assert ids[b, :lens[b]].tolist() == want[b], (C, T, b)
            assert (ids[b, lens[b]:] == H.FILL_I32).all(), 'ids behind the hypothesis were written'


# ------------------------------------------------------------------ mean
@pytest.mark.parametrize('n', [1, 3, 64])
def test_mean_is_the_left_to_right_float_sum(n):
    v = (np.random.RandomState(n).randn(n) * 10.0 ** np.random.RandomState(n + 1).randint(-3, 4, n)).astype(np.float32)
    s = np.float32(0)
    for a in v:
        s = np.float32(s + a)
    out = H.mean(v)
    assert bits(out[:1])[0] == bits(np.array([s / np.float32(n)], np.float32))[0]
    assert H.untouched(out[1:]).all()


# ------------------------------------------------------------------ refusals
def refusal_variants():
    """name -> (descriptor overrides, changes to seq_len / labels / label_len) off a valid launch of B 5, Tp 12, C 29, Lmax 6"""
    return {
        'B 0': (dict(B=0, Bp=0), {}), 'B 65': (dict(B=65, Bp=80), {}), 'Bp': (dict(Bp=32), {}), 'Cp': (dict(Cp=64), {}),
        'C 1': (dict(C=1), {}), 'Lmax 0': (dict(Lmax=0), {}), 'Lmax 512': (dict(Lmax=512), {}), 'Tp 0': (dict(Tp=0), {}),
        'seq_len 0': ({}, dict(seq=(2, 0))), 'seq_len > Tp': ({}, dict(seq=(1, 13))), 'seq_len of a padded row': ({}, dict(seq=(5, 1))),
        'label_len > Lmax': ({}, dict(ll=(0, 7))), 'label_len < 0': ({}, dict(ll=(3, -1))),
        'the blank as a label': ({}, dict(lab=(0, 1, 28))), 'a negative id': ({}, dict(lab=(0, 0, -1))),
        'an id beyond C': ({}, dict(lab=(4, 5, 29))),
        'infeasible': ({}, dict(seq=(4, 4), lab=(4, slice(0, 3), 3), ll=(4, 3))),
        '2^32 bytes of logits': (dict(Tp=4096, B=64, Bp=64, C=4096, Cp=4096), dict(allseq=1)),
        'beyond 2^32 bytes': (dict(Tp=4200, B=64, Bp=64, C=4000, Cp=4000), dict(allseq=1)),
    }


@pytest.mark.parametrize('name', sorted(refusal_variants()))
def test_refusals(name):
    """Every refusal returns -1 before a buffer is touched: nothing comes back changed."""
    over, ch = refusal_variants()[name]
    rs = np.random.RandomState(3)
    x = rs.randn(12, 16, 32).astype(np.float32)
    seq = np.array([12, 3, 7, 1, 9] + [0] * 11, np.int32)
    seq = np.concatenate([seq, np.zeros(64, np.int32)])            # (room for the descriptors that claim more rows)
    labels = rs.randint(0, 28, (5, 6)).astype(np.int32)
    labels[:, 1::2] = (labels[:, 0::2] + 1) % 28                   # no repeats
    ll = np.array([4, 1, 3, 0, 2], np.int32)
    d = H.ctc_desc(12, 5, 29, 6)
    rc, g, logz, nll, logp = H.ctc_pass_raw(d, x, seq, labels, ll)
    assert rc == 0 and not H.untouched(logz.reshape(12, 16)[0, :5]).any()          # the launch the variants depart from
    if 'seq' in ch:
        seq[ch['seq'][0]] = ch['seq'][1]
    if 'allseq' in ch:
        seq[:] = 1
    if 'lab' in ch:
        labels[ch['lab'][0], ch['lab'][1]] = ch['lab'][2]
    if 'll' in ch:
        ll[ch['ll'][0]] = ch['ll'][1]
    d = H.ctc_desc(**{**dict(Tp=12, B=5, C=29, Lmax=6), **over})
    rc, g, logz, nll, logp = H.ctc_pass_raw(d, x, seq, labels, ll)
    assert rc == -1
    assert np.array_equal(bits(g), bits(x)) and H.untouched(logz).all() and H.untouched(nll).all()
    assert (bits(logp) == bits(np.array([H.FILL_F64]))[0]).all()
    if not ({'lab', 'll'} & set(ch)) and 'Lmax' not in over:       # the greedy entry takes no labels
        rc, ids, lens = H.ctc_greedy_raw(d, x, seq)
        assert rc == -1 and (ids == H.FILL_I32).all() and (lens == H.FILL_I32).all()


def test_mean_refuses_an_empty_sum():
    out = np.full(2, H.FILL_F32, np.float32)
    v = np.zeros(1, np.float32)
    assert H.lib().kt_mean(H._f(v), 0, H._f(out), 2, H.FILL) == -1 and H.untouched(out).all()
