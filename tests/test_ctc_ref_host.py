"""CPU tests of tests/ctc_ref.py: the fp64 oracle equals brute-force enumeration on tiny lattices; the fp32 model of the
lattice follows the oracle; the case generators produce only what validate_batch accepts, on logits the model handles to
E_MODEL_CAP; the check of test_gpu_ctc_kernels.py passes the model itself on every sweep batch (not too tight) and rejects
each wrong model of MUTANTS on at least one of them (not vacuous)."""
import numpy as np
import pytest

import ctc_ref as R
from oracle import nasr_oracle as O

SWEEP = [c for c, _ in R.sweep_cases()]


# ------------------------------------------------------------------ the references
@pytest.mark.parametrize('label', [[], [0], [1, 1], [0, 2, 0], [2, 2, 2], [0, 1, 2]], ids=str)
def test_oracle_equals_brute_force_on_tiny_lattices(label):
    rs = np.random.RandomState(len(label) + 3 * sum(label))
    for T in range(max(1, len(label) + sum(a == b for a, b in zip(label[:-1], label[1:]))), 7):
        x = rs.randn(T, 4) * 2
        nll = O.ctc_single(x, label, 3)[0]
        assert nll == pytest.approx(O.ctc_brute_force(x, label, 3), rel=1e-12, abs=1e-12)
        # the fp32 model on the same lattice
        x32 = x.astype(np.float32).astype(np.float64)
        n32, g32 = R.ctc_fp32(x32, label, 3)
        n64, g64 = O.ctc_single(x32, label, 3)[:2]
        assert abs(n32 - n64) <= 1e-5 and np.abs(g32 - g64).max() <= 1e-5


def test_oracle_gradient_is_the_derivative_of_its_loss():
    rs = np.random.RandomState(5)
    x, label = rs.randn(9, 5), [1, 1, 3, 0]
    g = O.ctc_single(x, label, 4)[1]
    for t, k in ((0, 1), (4, 4), (8, 0), (5, 3)):
        d = np.zeros_like(x)
        d[t, k] = 1e-6
        num = (O.ctc_single(x + d, label, 4)[0] - O.ctc_single(x - d, label, 4)[0]) / 2e-6
        assert num == pytest.approx(g[t, k], abs=1e-8)


def test_model_rescaling_period_does_not_change_what_it_computes():
    c = R.small_case(29)
    for b in range(c.B):
        Tb, lab = c.seq_len[b], c.labels[b, :c.label_len[b]]
        n4, g4 = R.ctc_fp32(c.logits[:Tb, b], lab, 28, G=4)
        n1, g1 = R.ctc_fp32(c.logits[:Tb, b], lab, 28, G=1)
        assert abs(n4 - n1) <= 1e-4 and np.abs(g4 - g1).max() <= 1e-4


# ------------------------------------------------------------------ the generators
def all_cases():
    return SWEEP + R.instance_cases() + [c for c, _ in R.classes_cases()] + [R.small_case(29), R.small_case(40), R.small_case(29, Lmax=63)]


@pytest.mark.parametrize('case', all_cases(), ids=lambda c: c.id)
def test_cases_are_feasible_and_within_the_models_reach(case):
    assert R.feasible(case)
    ref = R.reference(case)
    print(f'{case.id}: E_model {ref["E_model"]:.3g}, N_model {ref["N_model"]:.3g}')
    assert ref['E_model'] <= R.E_MODEL_CAP
    # the unmutated model passes its own check
    problems, mg, ml = R.check(case, *R.model_batch(case))
    assert not problems and mg <= 1 and ml <= 1


def test_cases_cover_what_the_issue_lists():
    sw = R.sweep_cases()
    lens = sorted(int(t) for c, w in sw if 'flat' in c.id and c.C == 29 for t in c.seq_len)
    assert lens == list(range(1, 193))
    assert all(c.Tp == c.seq_len.max() + 5 and c.Lmax == 24 and c.B == 64 for c, _ in sw)
    assert {(c.C, w) for c, w in sw if 'mag' not in c.id} == {(29, ('engineered', 'plain')), (40, ('plain',))}
    for c, _ in sw:      # every eighth label pinned where 24 labels can pin the length
        for b in range(7, 64, 8):
            lab = c.labels[b, :c.label_len[b]]
            if c.seq_len[b] <= 47:
                assert len(lab) + int((lab[1:] == lab[:-1]).sum()) == c.seq_len[b]
    assert any(c.label_len.min() == 0 for c, _ in sw)
    assert {R.states_per_lane(L) for L in R.INSTANCE_LMAX} == {2, 3, 4, 5, 6, 7, 8, 12, 16}
    assert all(R.states_per_lane(L - 1) < R.states_per_lane(L) for L in R.INSTANCE_LMAX[1:-1])     # each the lower edge of its KS
    for c in R.instance_cases():
        assert c.B == 6 and c.Tp == min(1100, 2 * c.Lmax + 40) and len(set(c.seq_len.tolist())) == 6
        assert sorted(c.label_len.tolist()) == sorted([c.Lmax, c.Lmax // 4, 0, 1, c.Lmax // 3, c.Lmax // 2])
        one = c.labels[5, :c.label_len[5]]
        assert (one == one[0]).all()
        assert c.label_len[4] + int((c.labels[4, 1:c.label_len[4]] == c.labels[4, :c.label_len[4] - 1]).sum()) == c.seq_len[4]
    assert [c.C for c, _ in R.classes_cases()] == list(R.CLASS_COUNTS)
    assert all(('engineered' in w) == (c.C <= 31) and 'plain' in w for c, w in R.classes_cases())


def test_sharp_regimes_are_what_they_claim():
    c = next(c for c in SWEEP if c.id == 'sweep-T65..128-C29-sharp')
    y = np.exp(O.log_softmax(c.logits))
    for b, least in ((10, 0.9), (11, 0.9999)):          # margin 10 in the even slots, 20 in the odd ones
        assert y[:c.seq_len[b], b].max(-1).min() > least
    inst = R.instance_case(64, 29)
    lp = O.log_softmax(inst.logits)
    # some frame of the full-width label holds a class 15 and more below the row's best: the improbable emission
    assert (lp[:inst.seq_len[0], 0].min(-1) < -15).sum() >= 3
    mag = next(c for c in SWEEP if 'mag' in c.id)
    assert np.abs(mag.logits).max() > 80


# ------------------------------------------------------------------ has teeth
def _caught(mutant, case):
    problems, mg, ml = R.check(case, *R.model_batch(case, mutant))
    return bool(problems)


@pytest.mark.parametrize('mutant', R.MUTANTS)
def test_every_wrong_model_is_caught_on_a_sweep_batch(mutant):
    # (the ring hand-over starts at position 64: the batches of T <= 64 cannot see it)
    cases = [c for c in SWEEP if c.C == 29 and 'mag' not in c.id and (mutant != 'ring_shift' or c.seq_len.max() > 65)]
    assert any(_caught(mutant, c) for c in cases), f'{mutant} passes every sweep batch'


def test_check_holds_a_single_frame_to_the_bound():
    """What the whole-tensor norms of the network tests cannot see: one element of one frame off by 1e-4."""
    c = SWEEP[0]
    g, lp = R.model_batch(c)
    g = g.copy()
    g[c.seq_len[40] - 1, 40, 3] += 1e-4
    problems, _, _ = R.check(c, g, lp)
    assert problems and 'b 40' in problems[0]
    lz = np.array(R.reference(c)['logz'])
    assert not R.check_logz(c, lz.astype(np.float32))
    lz[0, 5] += 1e-5
    assert R.check_logz(c, lz)
