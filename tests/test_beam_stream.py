"""The incremental CTC beam search (nasr_ctc_beam_open / feed / best / close) against the whole-utterance
calls it shares its code with: whatever the split of the frames, the ids and the log-probability are those of
nasr_ctc_beam_search(_lm) bit for bit; `best` after every prefix is the batch search on that prefix, does not disturb
the search and can be asked twice; and the argument checks.  Host code: runs without a GPU."""
import ctypes

import numpy as np
import pytest

from neuralasr_amd import _lib
from neuralasr_amd.engine import BeamStream
from tests.test_beam_lm import lib_beam_lm, random_table

FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)


class Table:
    """what BeamStream reads of an lm.NGramLM"""

    def __init__(self, logp, eos, order, bos_id):
        self.logp, self.eos, self.order, self.bos_id, self.num_classes = logp, eos, order, bos_id, logp.shape[1]


def make_logits(kind, T, C, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(T, C) * 1.5
    x[:, C - 1] += 1.0                                    # blank-heavy, like a trained CTC net
    if kind == 'sharp':
        x *= 20.0                                         # near one-hot posteriors: most extensions underflow to -inf
    return np.ascontiguousarray(x, np.float32)


def lm_args(C, with_lm, seed):
    """(Table or None, weight, bonus): an order-2 table with a bonus and a weight, or the plain search"""
    if not with_lm:
        return None, 0.0, 0.0
    logp, eos = random_table(np.random.RandomState(100 + seed), C, 2)
    return Table(logp, eos, 2, 0), 0.7, 0.3


def batch(logits, width, merge, lm, weight, bonus):
    """(ids, logp as float32) of the whole-utterance call on logits [T, C]; T = 0: the call on one frame with seq_len 0"""
    T = logits.shape[0]
    lg = logits[:, None, :] if T else np.zeros((1, 1, logits.shape[1]), np.float32)
    if lm is None:
        got, lp, _, _ = lib_beam_lm(lg, [T], width, merge, None, None, 1, 0, 0.0, 0.0)
    else:
        got, lp, _, _ = lib_beam_lm(lg, [T], width, merge, lm.logp, lm.eos, lm.order, lm.bos_id, weight, bonus)
    return got[0], np.float32(lp[0])


def same(a, b):
    return a[0] == b[0] and np.float32(a[1]).tobytes() == np.float32(b[1]).tobytes()


CASES = [(kind, C, T) for kind in ('random', 'sharp') for C, T in ((3, 9), (6, 25), (29, 40))]


@pytest.mark.parametrize('with_lm', [False, True])
@pytest.mark.parametrize('merge', [False, True])
@pytest.mark.parametrize('width', [1, 4, 100])
@pytest.mark.parametrize('kind,C,T', CASES)
def test_any_split_gives_the_batch_searchs_bits(kind, C, T, width, merge, with_lm):
    logits = make_logits(kind, T, C, seed=C + T)
    lm, weight, bonus = lm_args(C, with_lm, C)
    want = batch(logits, width, merge, lm, weight, bonus)
    rs = np.random.RandomState(T)
    cuts = sorted(rs.choice(np.arange(1, T), size=min(4, T - 1), replace=False).tolist())
    for bounds in ([0, T], list(range(T + 1)), [0] + cuts + [T]):           # one piece, frame by frame, a random split
        s = BeamStream(C, width, merge, lm=lm, lm_weight=weight, lm_bonus=bonus)
        for a, b in zip(bounds[:-1], bounds[1:]):
            s.feed(logits[a:b])
        assert same(s.best(), want), bounds
        s.close()


@pytest.mark.parametrize('with_lm', [False, True])
@pytest.mark.parametrize('kind,C,T,width,merge', [('random', 6, 25, 4, True), ('sharp', 29, 40, 100, True),
                                                  ('random', 3, 9, 1, False), ('sharp', 6, 25, 100, False)])
def test_best_after_every_prefix_is_the_batch_search_on_it(kind, C, T, width, merge, with_lm):
    logits = make_logits(kind, T, C, seed=7 * C + T)
    lm, weight, bonus = lm_args(C, with_lm, C + 1)
    s = BeamStream(C, width, merge, lm=lm, lm_weight=weight, lm_bonus=bonus)
    first = s.best()
    assert first[0] == [] and same(first, batch(logits[:0], width, merge, lm, weight, bonus))   # t = 0: the empty hypothesis
    for t in range(1, T + 1):
        s.feed(logits[t - 1:t])
        got = s.best()
        assert same(got, s.best())                          # twice in a row: the same answer, nothing disturbed
        assert same(got, batch(logits[:t], width, merge, lm, weight, bonus)), t   # ... and the search went on correctly
    s.reset()
    assert s.best()[0] == [] and s.frames == 0


def test_a_column_of_time_major_logits_is_read_in_place():
    rs = np.random.RandomState(3)
    lg = (rs.randn(12, 3, 5) * 2).astype(np.float32)
    for b in range(3):
        s = BeamStream(5, 10, True)
        s.feed(lg[:7], slot=b)
        s.feed(lg[7:], slot=b)
        assert same(s.best(), batch(np.ascontiguousarray(lg[:, b]), 10, True, None, 0.0, 0.0))
    with pytest.raises(ValueError):
        BeamStream(5).feed(lg, slot=3)
    with pytest.raises(ValueError):
        BeamStream(4).feed(lg, slot=0)


def test_bad_arguments():
    lib = _lib.load()
    logp, eos = random_table(np.random.RandomState(0), 5, 2)
    h = ctypes.c_void_p()

    def open_(C=5, width=10, lp=None, le=None, order=1, bos=0, out=h):
        return lib.nasr_ctc_beam_open(C, width, 1, None if lp is None else lp.ctypes.data_as(FP),
                                      None if le is None else le.ctypes.data_as(FP), order, bos, 0.5, 0.0,
                                      None if out is None else ctypes.byref(out))

    assert open_(C=1) == _lib.NASR_ERR_ARG and not h.value
    assert open_(width=0) == _lib.NASR_ERR_ARG and not h.value
    assert open_(out=None) == _lib.NASR_ERR_ARG
    assert open_(lp=logp, le=None, order=2) == _lib.NASR_ERR_ARG          # the rules of nasr_ctc_beam_search_lm
    assert open_(lp=logp, le=eos, order=5) == _lib.NASR_ERR_ARG
    assert open_(lp=logp, le=eos, order=2, bos=5) == _lib.NASR_ERR_ARG
    assert open_(lp=None, le=None, order=9, bos=-3) == 0 and h.value       # no table: the LM arguments are not read
    x = (np.random.RandomState(1).randn(6, 5) * 3).astype(np.float32)
    x[:, 4] -= 5.0                                                          # little blank: a hypothesis of several ids
    n, lp = ctypes.c_int32(-1), ctypes.c_float()
    ids = np.full(8, -7, np.int32)
    assert lib.nasr_ctc_beam_feed(None, x.ctypes.data_as(FP), 5, 6) == _lib.NASR_ERR_ARG
    assert lib.nasr_ctc_beam_feed(h, None, 5, 6) == _lib.NASR_ERR_ARG
    assert lib.nasr_ctc_beam_feed(h, x.ctypes.data_as(FP), 4, 6) == _lib.NASR_ERR_ARG       # a stride below C
    assert lib.nasr_ctc_beam_feed(h, x.ctypes.data_as(FP), 5, -1) == _lib.NASR_ERR_ARG
    assert lib.nasr_ctc_beam_feed(h, None, 5, 0) == 0                                         # no frame: nothing is read
    assert lib.nasr_ctc_beam_best(h, ids.ctypes.data_as(IP), 8, ctypes.byref(n), None) == 0 and n.value == 0
    assert lib.nasr_ctc_beam_feed(h, x.ctypes.data_as(FP), 5, 6) == 0
    assert lib.nasr_ctc_beam_best(None, ids.ctypes.data_as(IP), 8, ctypes.byref(n), None) == _lib.NASR_ERR_ARG
    assert lib.nasr_ctc_beam_best(h, ids.ctypes.data_as(IP), 8, None, None) == _lib.NASR_ERR_ARG
    assert lib.nasr_ctc_beam_best(h, None, 8, ctypes.byref(n), None) == _lib.NASR_ERR_ARG
    assert lib.nasr_ctc_beam_best(h, ids.ctypes.data_as(IP), 8, ctypes.byref(n), ctypes.byref(lp)) == 0
    full, length = ids[:n.value].tolist(), n.value
    assert length >= 2 and full == batch(x, 10, True, None, 0.0, 0.0)[0]
    ids[:] = -7
    n.value = -1                                       # a short cap: NASR_ERR_ARG, the length still reported, no id written
    assert lib.nasr_ctc_beam_best(h, ids.ctypes.data_as(IP), length - 1, ctypes.byref(n), None) == _lib.NASR_ERR_ARG
    assert n.value == length and (ids == -7).all()
    assert lib.nasr_ctc_beam_best(h, None, 0, ctypes.byref(n), None) == _lib.NASR_ERR_ARG and n.value == length
    assert lib.nasr_ctc_beam_close(h) == 0
    assert lib.nasr_ctc_beam_close(None) == 0
