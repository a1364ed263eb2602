"""The CTC beam search fused with an n-gram table (nasr_ctc_beam_search_lm): (a) against exhaustive
enumeration of log P_ctc(y) + sum_i (weight*lm(y_i | y_<i) + bonus) + weight*eos(ctx(y)) when the beam holds every prefix,
(b) against the independent float64 restatement of tests/ctc_lm_ref.py on longer inputs and narrow beams, (c) bit for bit
against the plain decoder when the table cannot matter, and the argument checks.  Host code: runs without a GPU.

Seeds: every case's float64 gap between the best and the second-best answer exceeds 1e-3 (asserted), so the float32
decoder's rounding cannot change the winner; the first eight seeds of (a) were also picked so that the model changes the
winner of the plain search."""
import ctypes

import numpy as np
import pytest

from neuralasr_amd import _lib
from tests import ctc_lm_ref as R

FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)


def random_table(rs, C, order, scale=1.5):
    """float32 (logp [K][C], eos [K]): rows of a random distribution over the C symbols and the end"""
    K = C ** (order - 1)
    x = rs.randn(K, C + 1) * scale
    x = x - np.log(np.exp(x).sum(1, keepdims=True))
    return np.ascontiguousarray(x[:, :C], np.float32), np.ascontiguousarray(x[:, C], np.float32)


def lib_beam_lm(logits_tm, seq_len, width, merge, logp, eos, order, bos, weight, bonus, expect=0):
    lib = _lib.load()
    lg = np.ascontiguousarray(logits_tm, np.float32)
    Tp, B, C = lg.shape
    seq = np.ascontiguousarray(seq_len, np.int32)
    ids = np.zeros((B, Tp), np.int32)
    lens = np.zeros(B, np.int32)
    out = np.zeros(B, np.float32)
    rc = lib.nasr_ctc_beam_search_lm(lg.ctypes.data_as(FP), seq.ctypes.data_as(IP), B, Tp, C, width, int(merge),
                                     None if logp is None else logp.ctypes.data_as(FP),
                                     None if eos is None else eos.ctypes.data_as(FP), order, bos, weight, bonus,
                                     ids.ctypes.data_as(IP), lens.ctypes.data_as(IP), out.ctypes.data_as(FP))
    assert rc == expect
    return [ids[b, :lens[b]].tolist() for b in range(B)], out, ids, lens


def lib_beam_plain(logits_tm, seq_len, width, merge):
    lib = _lib.load()
    lg = np.ascontiguousarray(logits_tm, np.float32)
    Tp, B, C = lg.shape
    seq = np.ascontiguousarray(seq_len, np.int32)
    ids = np.zeros((B, Tp), np.int32)
    lens = np.zeros(B, np.int32)
    out = np.zeros(B, np.float32)
    assert lib.nasr_ctc_beam_search(lg.ctypes.data_as(FP), seq.ctypes.data_as(IP), B, Tp, C, width, int(merge),
                                    ids.ctypes.data_as(IP), lens.ctypes.data_as(IP), out.ctypes.data_as(FP)) == 0
    return out, ids, lens


# T, C (with blank), order, weight, bonus, bos_id, seed
EXHAUSTIVE = [(1, 3, 1, 0.7, 0.0, 0, 2), (3, 3, 2, 0.7, 0.0, 0, 3), (4, 3, 3, 1.0, 0.0, 0, 1), (5, 3, 2, 0.5, 0.8, 0, 0),
              (4, 4, 3, 0.6, -0.5, 0, 0), (5, 4, 1, 1.2, 0.4, 0, 0), (5, 4, 2, 0.8, 0.0, 0, 0), (5, 4, 3, 0.9, 1.0, 0, 0),
              (5, 4, 3, 0.9, 0.0, 2, 1), (5, 3, 2, 1.0, -0.7, 1, 4)]


@pytest.mark.parametrize('T,C,order,weight,bonus,bos,seed', EXHAUSTIVE)
def test_wide_beam_is_the_argmax_of_the_fused_score(T, C, order, weight, bonus, bos, seed):
    rs = np.random.RandomState(seed)
    logits = rs.randn(T, C) * 2.0
    logp, eos = random_table(rs, C, order)
    logits32 = logits.astype(np.float32)
    best, score, gap = R.exhaustive(logits32, logp, eos, order, bos, weight, bonus)
    assert gap > 1e-3, gap
    got, lp, _, _ = lib_beam_lm(logits32[:, None, :], [T], 1000, False, logp, eos, order, bos, weight, bonus)
    assert got[0] == best
    assert lp[0] == pytest.approx(score, abs=2e-3)
    ids_r, score_r, _ = R.beam_search_lm(logits32, 1000, False, logp, eos, order, bos, weight, bonus)
    assert ids_r == best and score_r == pytest.approx(score, abs=1e-9)


# C, order, T, seq_len, weight, bonus, bos, seed
RESTATED = [(6, 3, 30, [30, 1, 22], 0.6, 0.4, 0, 0), (6, 2, 20, [20, 13, 1], 1.0, 0.0, 3, 1),
            (29, 2, 40, [40, 1, 27], 0.5, 0.3, 0, 2), (29, 1, 25, [1, 25, 20], 0.8, -0.2, 0, 3)]


@pytest.mark.parametrize('C,order,T,seq,weight,bonus,bos,seed', RESTATED)
@pytest.mark.parametrize('width', [5, 100])
@pytest.mark.parametrize('merge', [False, True])
def test_matches_the_restatement(C, order, T, seq, weight, bonus, bos, seed, width, merge):
    rs = np.random.RandomState(1000 * seed + width)
    logits = (rs.randn(T, 3, C) * 1.5).astype(np.float32)
    logits[:, :, C - 1] += 1.0                       # blank-heavy, like a trained CTC net
    logp, eos = random_table(rs, C, order)
    assert 5 < C                                     # width 5 is the beam narrower than the class count
    got, lp, _, _ = lib_beam_lm(logits, seq, width, merge, logp, eos, order, bos, weight, bonus)
    for b in range(3):
        ids_r, score_r, gap = R.beam_search_lm(logits[:seq[b], b], width, merge, logp, eos, order, bos, weight, bonus)
        assert gap > 1e-3, (b, gap)
        assert got[b] == ids_r, (b, width, merge)
        assert lp[b] == pytest.approx(score_r, abs=2e-3)


@pytest.mark.parametrize('order', [1, 2, 3])
def test_a_table_that_cannot_matter_gives_the_plain_decoders_bits(order):
    rs = np.random.RandomState(11 + order)
    Tp, B, C = 40, 4, 9
    logits = (rs.randn(Tp, B, C) * 1.5).astype(np.float32)
    logits[:, :, C - 1] += 1.0
    seq = [40, 1, 33, 17]
    logp, eos = random_table(rs, C, order)
    for width, merge in ((100, True), (4, False)):
        plain = lib_beam_plain(logits, seq, width, merge)
        zero = lib_beam_lm(logits, seq, width, merge, logp, eos, order, 0, 0.0, 0.0)[1:]
        null = lib_beam_lm(logits, seq, width, merge, None, None, 7, -3, 0.9, 0.5)[1:]
        for other in (zero, null):
            for a, b in zip(plain, other):
                assert a.tobytes() == b.tobytes()
        fused = lib_beam_lm(logits, seq, width, merge, logp, eos, order, 0, 1.5, 0.5)[1:]
        assert fused[0].tobytes() != plain[0].tobytes()


def test_bad_arguments():
    rs = np.random.RandomState(0)
    logits = rs.randn(4, 1, 5).astype(np.float32)
    logp, eos = random_table(rs, 5, 2)
    ok = dict(logp=logp, eos=eos, order=2, bos=0, weight=0.5, bonus=0.0)

    def call(C=5, lg=logits, **kw):
        a = dict(ok, **kw)
        lib_beam_lm(lg, [lg.shape[0]], 10, True, a['logp'], a['eos'], a['order'], a['bos'], a['weight'], a['bonus'],
                    expect=_lib.NASR_ERR_ARG)

    lib_beam_lm(logits, [4], 10, True, logp, eos, 2, 0, 0.5, 0.0)
    call(order=0)
    call(order=5)
    call(bos=-1)
    call(bos=5)
    call(eos=None)
    # K*C > 2^24: 65 classes at order 4 (the table itself is never read: the check comes first)
    wide = rs.randn(2, 1, 65).astype(np.float32)
    call(lg=wide, order=4)
    big_logp, big_eos = np.zeros((64 ** 3, 64), np.float32), np.zeros(64 ** 3, np.float32)
    lg64 = rs.randn(2, 1, 64).astype(np.float32)            # 64^4 = 2^24 entries is the largest table allowed
    lib_beam_lm(lg64, [2], 4, True, big_logp, big_eos, 4, 0, 0.5, 0.0)
    lib = _lib.load()
    assert lib.nasr_ctc_beam_search_lm(None, None, 1, 1, 3, 100, 1, None, None, 1, 0, 0.0, 0.0, None, None,
                                       None) == _lib.NASR_ERR_ARG
