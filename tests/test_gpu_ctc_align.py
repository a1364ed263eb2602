"""GPU: the forced-alignment kernel of csrc/ctc.hip (4) through Engine.align_logits, against the fp64 restatement
tests/ctc_align_ref.py.

Exact cases: integer logits drawn from [-8, 8].  Every partial sum up to F = 1100 is an integer below 2^24 and the value the
kernel subtracts from a column (its maximum, every 4 frames) is one too, so fp32 is exact, ties are plentiful, and the path
must be the restatement's on every element; the score shares logZ with the loss and has the loss's tolerance.

Float cases: the kernel's fp32 sums round.  Its path must be a valid one, and its fp64 sum may fall short of the optimum by
at most F * 2^-23 * max|v|: every frame rounds one addition (and every fourth one subtraction) of a value of magnitude
<= max|v| to half an ulp, 2^-24 relative, on the winning path and on the one it beat.  Where every decision on the optimal
path was won by more than that bound, the path must be the restatement's."""
import ctypes

import numpy as np
import pytest

import ctc_align_ref as R

pytestmark = pytest.mark.gpu

SCORE_RTOL, SCORE_ATOL = 3e-5, 1e-5          # the nll tolerance of test_gpu_ctc_lattice.py


@pytest.fixture(scope='module')
def eng():
    """one small handle for the whole module: align_logits is independent of its model"""
    from neuralasr_amd.engine import Engine
    e = Engine(8, 16, 1, False, 'none', 5)
    yield e
    e.close()


def make_label(rs, L, C, runs):
    """L ids below the blank with `runs` adjacent repeats forced in (fewer when C = 2 makes every pair one)"""
    lab = rs.randint(0, C - 1, size=L)
    for i in rs.permutation(max(L - 1, 0))[:runs]:
        lab[i + 1] = lab[i]
    return lab.astype(np.int32)


def needed(lab):
    return len(lab) + sum(1 for i in range(1, len(lab)) if lab[i] == lab[i - 1])


def batch_of(rs, C, utts, slack=3, scale=None):
    """utts: [(F, label)] -> logits [T',B,C] (T' = longest F + slack), seq_len, padded labels (padding = class ids), label_len"""
    B = len(utts)
    Tp = max(F for F, _ in utts) + slack
    Lmax = max(1, max(len(l) for _, l in utts))
    if scale is None:
        logits = rs.randint(-8, 9, size=(Tp, B, C)).astype(np.float32)
    else:
        logits = (scale * rs.randn(Tp, B, C)).astype(np.float32)
    labels = rs.randint(0, C - 1, size=(B, Lmax)).astype(np.int32)
    for b, (_, l) in enumerate(utts):
        labels[b, :len(l)] = l
    return logits, [F for F, _ in utts], labels, [len(l) for _, l in utts]


def check_exact(eng, rs, C, utts, lds=None):
    logits, seq, labels, ll = batch_of(rs, C, utts)
    if lds is not None:
        assert eng.align_in_lds(max(seq), labels.shape[1]) == lds
    path, score = eng.align_logits(logits, seq, labels, ll)
    assert path.dtype == np.int32 and path.shape == (len(utts), logits.shape[0]) and score.dtype == np.float64
    for b, (F, lab) in enumerate(utts):
        want, wscore, vmax, _ = R.align(logits[:F, b], lab)
        assert vmax < 2 ** 24
        bad = np.nonzero(path[b, :F] != want)[0]
        assert bad.size == 0, 'utterance %d (F %d, L %d): %d frames differ, first at %d' % (b, F, len(lab), bad.size, bad[0])
        assert np.all(path[b, F:] == -1)
        print('utterance %d F %d L %d: score %.9g, restatement %.9g' % (b, F, len(lab), score[b], wscore))
        assert abs(score[b] - wscore) <= SCORE_ATOL + SCORE_RTOL * abs(wscore)
    return path, score


def test_short_utterances(eng):
    """F in {1, 2, 3, 4, 5, 7, 8, 9, 70}: fewer frames than a group of 4, a group exactly, one more; empty, single and
    repeated labels; every F also pinned (F = L + repeats: one path)"""
    rs = np.random.RandomState(1)
    utts = []
    for F in (1, 2, 3, 4, 5, 7, 8, 9, 70):
        utts.append((F, make_label(rs, min(F // 2, 6), 29, 1)))
    utts += [(1, make_label(rs, 1, 29, 0)), (3, np.array([4, 4], np.int32)), (5, np.array([], np.int32))]
    for L, runs in ((2, 0), (3, 1), (5, 2), (9, 0)):
        lab = make_label(rs, L, 29, runs)
        utts.append((needed(lab), lab))
    assert all(R.feasible(list(l), F) for F, l in utts)
    check_exact(eng, rs, 29, utts, lds=True)


# the lane and states-per-lane edges of S = 2L+1 (the issue's list), and one width inside every other instantiation
@pytest.mark.parametrize('L', [0, 1, 2, 31, 32, 33, 63, 64, 95, 96, 128, 160, 192, 224, 256, 511])
def test_label_length_edges(eng, L):
    """per width: a pinned label (F = L + repeats exactly), the same width with room and runs of repeats, an utterance of one
    frame beside them; L = 511 runs to F = 1100"""
    rs = np.random.RandomState(100 + L)
    pinned = make_label(rs, L, 29, L // 5)
    roomy = make_label(rs, L, 29, L // 4)
    F = 1100 if L == 511 else needed(roomy) + 37
    utts = [(max(needed(pinned), 1), pinned), (F, roomy), (1, make_label(rs, min(L, 1), 29, 0))]
    check_exact(eng, rs, 29, utts)


@pytest.mark.parametrize('B', [1, 5, 17])
def test_ragged_batches(eng, B):
    rs = np.random.RandomState(200 + B)
    utts = []
    for b in range(B):
        F = 1 if (b == B - 1 and B > 1) else int(rs.randint(20, 71))
        lab = make_label(rs, int(rs.randint(0, min(F // 2, 12) + 1)), 29, 2)
        utts.append((max(F, needed(lab)), lab))
    check_exact(eng, rs, 29, utts)


@pytest.mark.parametrize('C', [2, 29, 31, 32, 33, 300])
def test_class_counts(eng, C):
    """C = 2: one label class, every adjacent pair a repeat; 31 / 32 / 33: the edges of the loss's padded rows; 300: rows of
    several hundred classes"""
    rs = np.random.RandomState(300 + C)
    utts = [(40, make_label(rs, 7, C, 2)), (23, make_label(rs, 11, C, 3)), (9, make_label(rs, 0, C, 0))]
    utts = [(max(F, needed(l)), l) for F, l in utts]
    check_exact(eng, rs, C, utts)


@pytest.mark.parametrize('L,F,lds', [(12, 70, True), (12, 897, True), (12, 898, False), (200, 449, True), (200, 450, False),
                                     (200, 1000, False)])
def test_both_sides_of_the_backpointer_threshold(eng, L, F, lds):
    """back-pointers in LDS up to 896 (labels <= 127) / 448 (<= 255) frames after the first, in the global workspace beyond;
    exactly at the threshold and one frame past it"""
    rs = np.random.RandomState(400 + F)
    utts = [(F, make_label(rs, L, 29, L // 6)), (F - 130 if F > 400 else F - 5, make_label(rs, L // 2, 29, 3))]
    check_exact(eng, rs, 29, utts, lds=lds)


@pytest.mark.parametrize('scale', [1.0, 6.0])
@pytest.mark.parametrize('shape', [(5, 70, 12), (3, 600, 200)], ids=['B5-F70-L12', 'B3-F600-L200'])
def test_float_logits(eng, shape, scale):
    B, F, L = shape
    rs = np.random.RandomState(int(500 + F + scale))
    utts = [(F - 7 * b, make_label(rs, L - b, 29, L // 6)) for b in range(B)]
    logits, seq, labels, ll = batch_of(rs, 29, utts, scale=scale)
    path, score = eng.align_logits(logits, seq, labels, ll)
    for b, (Fb, lab) in enumerate(utts):
        x = logits[:Fb, b]
        want, wscore, vmax, gap = R.align(x, lab)
        got = path[b, :Fb]
        assert R.is_valid_path(got, lab, 28) and np.all(path[b, Fb:] == -1)
        bound = Fb * 2.0 ** -23 * vmax
        short = R.path_sum(x, lab, want) - R.path_sum(x, lab, got)
        print('scale %g utterance %d (F %d, L %d): shortfall %.3g, bound %.3g, max|v| %.4g, smallest margin %.3g, %d frames differ'
              % (scale, b, Fb, len(lab), short, bound, vmax, gap, int(np.sum(got != want))))
        assert -1e-9 <= short <= bound
        if gap > bound:
            assert np.array_equal(got, want)
        gscore = R.path_score(x, lab, got)
        assert abs(score[b] - gscore) <= SCORE_ATOL + SCORE_RTOL * abs(gscore)


def test_two_runs_give_the_same_bits(eng):
    rs = np.random.RandomState(7)
    for F, L in ((70, 12), (950, 40)):                    # LDS route, global route
        utts = [(F, make_label(rs, L, 29, 3)), (F - 9, make_label(rs, L - 2, 29, 1))]
        logits, seq, labels, ll = batch_of(rs, 29, utts, scale=3.0)
        p1, s1 = eng.align_logits(logits, seq, labels, ll)
        p2, s2 = eng.align_logits(logits, seq, labels, ll)
        assert np.array_equal(p1, p2) and np.array_equal(s1.view(np.uint64), s2.view(np.uint64))


def test_refusals(eng):
    from neuralasr_amd import _lib
    rs = np.random.RandomState(9)
    logits = rs.randn(6, 2, 5).astype(np.float32)
    # [1, 1, 1] needs 5 frames: refused by the loss's check before anything is launched - the outputs stay as they were
    labels = np.array([[1, 1, 1], [0, 2, 3]], np.int32)
    path = np.full((2, 6), -7, np.int32)
    score = np.full(2, 123.0)
    seq, ll = np.array([4, 6], np.int32), np.array([3, 3], np.int32)
    ip, fp = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    rc = eng.lib.nasr_ctc_align_logits(eng.h, logits.ctypes.data_as(fp), seq.ctypes.data_as(ip), labels.ctypes.data_as(ip),
                                       ll.ctypes.data_as(ip), 2, 6, 5, 3, path.ctypes.data_as(ip),
                                       score.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc == _lib.NASR_ERR_INFEASIBLE
    assert np.all(path == -7) and np.all(score == 123.0)
    with pytest.raises(_lib.InfeasibleLabelError) as err:
        eng.align_logits(logits, seq, labels, ll)
    assert 'Not enough time for target transition sequence (required: 5, available: 4) in sequence 0' in str(err.value)

    def refused(text, *args):
        with pytest.raises(_lib.NasrError) as e:
            eng.align_logits(*args)
        assert e.value.code == _lib.NASR_ERR_ARG and text in str(e.value), str(e.value)
    refused('label id', logits, [6, 6], np.array([[4, 0, 0], [0, 2, 3]], np.int32), [1, 3])       # the blank is no label
    refused('seq_len[1]', logits, [6, 7], labels, [1, 3])
    refused('label_len[0]', logits, [6, 6], labels, [4, 3])
    refused('nasr_ctc_align_logits', logits[:, :, :1], [6, 6], np.zeros((2, 1), np.int32), [0, 0])   # C = 1
    refused('511', rs.randn(4, 1, 5).astype(np.float32), [4], np.zeros((1, 512), np.int32), [0])
    # and the handle still aligns
    p, s = eng.align_logits(logits, [6, 6], labels, [2, 3])
    assert R.is_valid_path(p[0], [1, 1], 4) and R.is_valid_path(p[1], [0, 2, 3], 4)
