"""CPU tests of tests/rec_ref.py: the fp64 recurrence equals the oracle's LSTM layer; the error model holds an fp32
emulation of every arithmetic class on every case the GPU test runs (not too tight) and rejects each wrong model of
MUTANTS on at least one of them (not vacuous)."""
import numpy as np
import pytest

import rec_ref as R
from oracle import nasr_oracle as O

CASES = R.cases()
FWD = [c for c in CASES if not R.KINDS[c.path].bwd]
BWD = [c for c in CASES if R.KINDS[c.path].bwd]


# ------------------------------------------------------------------ the reference is the oracle's layer
@pytest.mark.parametrize('D', [1, 2])
def test_reference_equals_the_oracle_layer(D):
    rng = np.random.default_rng(11 + D)
    B, T, I, H, fb = 5, 9, 7, 6, 1.0
    ln = np.array([9, 1, 4, 9, 2])
    x = rng.standard_normal((B, T, I))
    dout = rng.standard_normal((B, T, D, H))
    pre = np.zeros((T, B, D, H, 4))
    U = np.zeros((D, H, H, 4))
    outs, caches, Ks = [], [], []
    for d in range(D):
        K = rng.uniform(-0.6, 0.6, size=(I + H, 4 * H))
        b = rng.uniform(-0.3, 0.3, size=4 * H)
        o, cache = O.lstm_dir_forward(x, ln, K, b, forget_bias=fb, reverse=d == 1)
        outs.append(o); caches.append(cache); Ks.append(K)
        pre[:, :, d] = (x @ K[:I] + b).reshape(B, T, 4, H).transpose(1, 0, 3, 2)      # oracle columns g*H + j
        U[d] = K[I:].reshape(H, 4, H).transpose(0, 2, 1)
    act, c, h = R.forward(U, pre, ln, fb)
    for d in range(D):
        assert np.max(np.abs(h[:, :, d].transpose(1, 0, 2) - outs[d])) <= 1e-12
    dG = R.backward(U, act, c, dout.transpose(1, 0, 2, 3), ln)
    for d in range(D):
        dx, dK, db = O.lstm_dir_backward(caches[d], dout[:, :, d])
        g = dG[:, :, d].transpose(1, 0, 3, 2).reshape(B, T, 4 * H)                   # [B][T][g*H + j]
        assert np.max(np.abs(g.sum((0, 1)) - db)) <= 1e-12
        assert np.max(np.abs(g @ Ks[d][:I].T - dx)) <= 1e-12
    # nothing at a frame that is not computed
    inv = ~(np.arange(T)[:, None] < ln[None, :])
    assert not h[inv].any() and not dG[inv].any()


def test_fast_activations_are_within_their_absolute_terms():
    """The emulation of tanhf_ / sigmoidf_ (correctly rounded exp2 and division) stays inside 8 u / 4 u - with the two
    1-ulp instructions' own share left over - and saturates without inf or NaN where exp overflows."""
    x = np.concatenate([np.linspace(-20, 20, 200001), [30, -30, 88, -88, 88.7, -88.7, 89, -89, 200, -200, 1e4, -1e4, 0.0]]).astype(np.float32)
    s, t = R.sigmoid_f32(x), R.tanh_f32(x)
    assert np.isfinite(s).all() and np.isfinite(t).all()
    x64 = x.astype(np.float64)
    assert np.max(np.abs(s - R._sig(x64))) <= R.SIG_ABS - 2 * R.U24
    assert np.max(np.abs(t - np.tanh(x64))) <= R.TANH_ABS - 2 * R.U24
    assert R.tanh_f32(np.float32(0)) == 0 and R.sigmoid_f32(np.float32(1e4)) == 1 and R.sigmoid_f32(np.float32(-200)) == 0
    # the design choice: the error is absolute, a tiny argument keeps none of its digits
    small = np.float32(3e-5)
    assert abs(R.tanh_f32(small) - np.tanh(np.float64(small))) <= R.TANH_ABS


def test_cases_cover_what_the_issue_lists():
    by = {}
    for c in CASES:
        by.setdefault(c.path, []).append(c)
    assert set(by) == set(R.KINDS)
    for p in ('persist_fwd32', 'persist_fwd16', 'persist_bwd'):
        assert {c.Hp for c in by[p]} >= set(range(64, 513, 64))          # every NU of the dispatch
    for p in ('step_fwd', 'step_bwd'):
        assert {c.Hp for c in by[p]} >= {64, 128, 256, 512, 576, 640}
    assert {c.B for c in CASES} >= {1, 5, 16, 17, 33, 64} and {c.D for c in CASES} == {1, 2}
    for p in set(by) - {'wide_fwd', 'wide_bwd'}:          # (the wide kernels: Hp 2048 only, T <= 6)
        assert any(c.T == 300 and c.Hp == 64 and c.B == 5 for c in by[p]), p
    assert any(c.lean and c.parts for c in by['persist_bwd']) and any(not c.parts for c in by['persist_bwd'])
    assert {c.regime for c in FWD} == {'init', 'sat', 'long', 'tiny', 'colrange', 'aligned'}
    assert {c.regime for c in by['wide_fwd']} >= {'init', 'sat', 'tiny', 'colrange'}
    assert any(c.lens == 'ragged0' for c in by['step_carry']) and any(c.lean and c.regime == 'sat' for c in by['persist_bwd'])
    assert any(c.H < c.Hp for c in CASES)


def test_regimes_are_what_they_claim():
    long_ = next(c for c in FWD if c.regime == 'long')
    inp = R.make_inputs(long_)
    _, c, h = R.forward(inp['U'], inp['pre'], inp['seq_len'], inp['fb'])
    assert np.abs(c).max() > long_.T / 2
    assert 10 < np.abs(inp['U'][0, :, :long_.H].reshape(long_.Hp, -1)).sum(0).mean() < 30
    tiny = next(c for c in FWD if c.regime == 'tiny' and c.path == 'persist_fwd16')
    inp = R.make_inputs(tiny)
    _, _, h = R.forward(inp['U'], inp['pre'], inp['seq_len'], inp['fb'])
    hv = np.abs(h[inp['valid']][:, :, :tiny.H])
    assert np.median(hv) * 2.0 ** 14 < 2.0 ** -14          # h 2^14 is an fp16 subnormal


# ------------------------------------------------------------------ not too tight
@pytest.mark.parametrize('case', FWD, ids=lambda c: c.id)
def test_forward_emulation_stays_inside_the_bound(case):
    kind = R.KINDS[case.path]
    inp = R.make_inputs(case)
    act, c, h = R.emulate_forward(kind, inp)
    r = R.check_forward(kind, inp, act, c, h)
    assert not r['problems'], r['problems']
    assert r['local'] <= 1, r
    if case.regime in ('init', 'sat'):
        assert r['running_bound'] <= R.RUNNING_LIMIT and r['running'] is not None
    assert r['running'] is None or r['running'] <= 1, r
    assert np.isfinite(act[inp['valid']]).all() and np.isfinite(h).all()


@pytest.mark.parametrize('case', BWD, ids=lambda c: c.id)
def test_backward_emulation_stays_inside_the_bound(case):
    kind = R.KINDS[case.path]
    inp = R.make_inputs(case)
    dg = R.emulate_backward(kind, inp)
    r = R.check_backward(kind, inp, dg)
    assert not r['problems'], r['problems']
    assert r['running'] <= 1, r


# ------------------------------------------------------------------ has teeth
# wrong model -> the paths it is a wrong model OF
MUTANTS = {
    'u_high_plane': ('persist_fwd16', 'wide_fwd'), 'drop_h1u2': ('persist_fwd16', 'wide_fwd'), 'drop_h2u1': ('persist_fwd16', 'wide_fwd'),
    'no_forget_bias': ('step_fwd', 'persist_fwd32', 'persist_fwd16'), 'swap_ij': ('step_fwd', 'persist_fwd32', 'persist_fwd16'),
    'bwd_reads_s': ('step_fwd', 'persist_fwd32', 'persist_fwd16'), 'stale_slice': ('step_fwd', 'persist_fwd32', 'persist_fwd16'),
    'state_not_zeroed': ('step_fwd', 'persist_fwd32', 'persist_fwd16'),
    'c_for_tanhc': ('step_bwd', 'persist_bwd', 'wide_bwd'), 'dc_dropped': ('step_bwd', 'persist_bwd', 'wide_bwd'),
}


def _caught(mutant, case):
    kind = R.KINDS[case.path]
    inp = R.make_inputs(case)
    if kind.bwd:
        dg = R.backward(inp['U'], inp['act'], inp['c'], inp['dout'], inp['seq_len'], mutant=mutant).astype(np.float32)
        r = R.check_backward(kind, inp, dg)
        return bool(r['problems']) or r['running'] > 1
    a, c, h = R.forward(inp['U'], inp['pre'], inp['seq_len'], inp['fb'], inp.get('h0'), inp.get('c0'), mutant=mutant)
    act = np.array(inp['pre'])
    v = inp['valid']
    act[v] = a[v]
    c32 = np.full(c.shape, np.nan, dtype=np.float32)
    c32[v] = c[v]
    r = R.check_forward(kind, inp, act, c32, h.astype(np.float32))
    return bool(r['problems']) or r['local'] > 1 or (r['running'] is not None and r['running'] > 1)


@pytest.mark.parametrize('mutant', sorted(MUTANTS))
def test_every_wrong_model_is_caught_on_every_path_it_applies_to(mutant):
    for path in MUTANTS[mutant]:
        small = sorted((c for c in CASES if c.path == path and c.T <= 12), key=lambda c: c.Hp * c.T * c.B)
        assert any(_caught(mutant, c) for c in small), f'{mutant} passes every {path} case'
