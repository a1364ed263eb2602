"""The LAS beam search on the GPU (nasr_las_beam_search) against the restatement of tests/las_beam_ref.py: exactly, with
all weights zero so that the logits are the projection bias; and by decision replay at random init, where the fp64 model
of tests/las_ref.py follows the GPU's trace and checks every step's scores and choice.  Plus determinism, argument and
handle checks, and that a search leaves the training state alone.  Measured errors are printed (pytest -s) and recorded
in DESIGN.md §10."""
import ctypes

import numpy as np
import pytest

from tests import las_beam_ref as ref

pytestmark = pytest.mark.gpu

F = 20


def _engine(F, C, seed=3, zero=False):
    from neuralasr_amd.engine import LasEngine
    from neuralasr_amd.networks.las import LAS
    e = LasEngine(F, C, sampling_probability=0.1, seed=5, learning_rate=1e-3)
    if zero:
        e.set_params(np.zeros(e.param_count, np.float32))
    else:
        e.set_params(LAS.__new__(LAS).initial_params(e.tensors(), seed=seed))
    return e


def _set_bias(e, bias):
    flat = e.get_params()
    off = {n: o for n, o, _, _ in e.tensors()}['projection_layer/bias']
    flat[off:off + len(bias)] = bias
    e.set_params(flat)


def _feats(B, T, F, rs):
    return rs.randn(B, T, F).astype(np.float32), np.full(B, T, np.int32)


def _bias(kind, C, end_id, rs):
    if kind == 'zero':
        return np.zeros(C, np.float32)
    # every class but the first sits >= 110 below it, in eighths: the row softmax is exactly (1, 0, ...), every log-prob
    # and every sum of them is exact in float32 on both sides; 'end' puts the first class at end_id (paths finish early)
    b = -(110 + rs.randint(0, 64, C) / 8.0)
    top = end_id if kind == 'end' else (end_id + 1) % C
    b[top] = 0
    return b.astype(np.float32)


def _gpu(e, feats, seq, W, steps, start, end, lp=0.5):
    return e.beam_search(feats, seq, W, steps, start, end, lp, trace=True)


def _tbw(a):   # [B, T, W] -> [T, B, W]
    return np.transpose(a, (1, 0, 2))


@pytest.mark.parametrize('W,C', [(1, 2), (3, 5), (3, 32), (1000, 2), (1000, 5), (1000, 32)])
@pytest.mark.parametrize('kind', ['zero', 'end', 'word'])
def test_exact_against_restatement(W, C, kind):
    rs = np.random.RandomState(W * 100 + C)
    B, T, steps, start, end = 2, 5, 12, 0, C - 1
    e = _engine(F, C, zero=True)
    bias = _bias(kind, C, end, rs)
    _set_bias(e, bias)
    feats, seq = _feats(B, T, F, rs)
    g = _gpu(e, feats, seq, W, steps, start, end)
    r = ref.beam_search(lambda t, p, ids: np.broadcast_to(bias, (B, W, C)), B, W, C, start, end, steps, 0.5)
    if kind != 'zero':
        assert (r['margin'] > 1e-4).all(), r['margin']
    print('LAS beam exact %s W=%d C=%d: T_dec %d, least margin %.3g' % (kind, W, C, r['steps'], r['margin'].min()))
    assert g['steps'] == r['steps']
    assert (_tbw(g['word_ids']) == r['word']).all()
    assert (_tbw(g['parent_ids']) == r['parent']).all()
    assert (g['lengths'] == r['lengths']).all() and (g['finished'] == r['finished']).all()
    assert (_tbw(g['predicted_ids']) == r['ids']).all()
    gs, rsc = _tbw(g['scores']), r['scores']
    assert ((gs == -np.inf) == (rsc == -np.inf)).all()
    fin = np.isfinite(rsc)
    np.testing.assert_allclose(gs[fin], rsc[fin], rtol=1e-6)
    lfin = np.isfinite(r['log_probs'])
    assert (np.isfinite(g['log_probs']) == lfin).all()
    np.testing.assert_allclose(g['log_probs'][lfin], r['log_probs'][lfin], rtol=1e-6)


def _replay_check(e, C, feats, g, W, start, end, weight=0.5, rtol=1e-5):
    """the fp64 model along the GPU's trace: (largest relative score error, steps checked)"""
    B, Td = feats.shape[0], g['steps']
    rp = ref.Replay(e.get_params(), feats.shape[2], C, feats, W)
    word, parent, scores = _tbw(g['word_ids']), _tbw(g['parent_ids']), _tbw(g['scores'])
    logp = np.full((B, W), -np.inf)
    logp[:, 0] = 0
    fin = np.ones((B, W), bool)
    fin[:, 0] = False
    lens = np.zeros((B, W), np.int64)
    is_end = np.arange(C) == end
    worst = 0.0
    for t in range(Td):
        logits = rp(t, None if t == 0 else parent[t - 1], np.full((B, W), start) if t == 0 else word[t - 1])
        lse = np.log(np.exp(logits - logits.max(-1, keepdims=True)).sum(-1, keepdims=True)) + logits.max(-1, keepdims=True)
        lp = logits - lse
        # ordinary candidates: a beam with an ordinary log-prob, live or at the end id; the FLT_LOWEST class: the rest with
        # a finite log-prob (a finished beam's other words, and every word of a beam whose log-prob came from FLT_LOWEST)
        normal = np.isfinite(logp) & (logp > -1e30)
        live = normal[..., None] & (~fin[..., None] | is_end)
        lowest = np.isfinite(logp)[..., None] & ~live
        with np.errstate(invalid='ignore'):
            total = logp[..., None] + np.where(fin[..., None], np.where(is_end, 0.0, float(ref.FLT_LOWEST)), lp)
            len_s = lens[..., None] + (~fin[..., None] & ~is_end)
            s64 = total / ((5.0 + len_s) ** weight / 6.0 ** weight)
        for b in range(B):
            chosen = parent[t, b] * C + word[t, b]
            gsc = scores[t, b].astype(np.float64)
            A = np.flatnonzero(live[b].ravel())
            inA = np.isin(chosen, A)
            sA = s64[b].ravel()
            err = np.abs(gsc[inA] - sA[chosen[inA]]) / np.maximum(np.abs(sA[chosen[inA]]), 1e-6)
            worst = max(worst, float(err.max()) if err.size else 0.0)
            assert (err <= rtol).all(), (t, b, float(err.max()))
            lo = lowest[b].ravel()[chosen]
            assert (gsc[lo] <= -1e38).all()
            dead = ~inA & ~lo
            assert (gsc[dead] == -np.inf).all()
            if A.size >= W:
                assert inA.all(), (t, b)
                rest = np.setdiff1d(A, chosen)
                if rest.size:
                    tol = rtol * max(abs(sA[chosen].min()), 1e-6)
                    assert sA[chosen].min() >= sA[rest].max() - 2 * tol, (t, b)
            else:
                assert np.isin(A, chosen).all(), (t, b)
        # the state along the GPU's choice, in fp64
        flat_total = total.reshape(B, W * C)
        sel = parent[t] * C + word[t]
        logp = np.take_along_axis(flat_total, sel, 1)
        pf = np.take_along_axis(fin, parent[t], 1)
        lens = np.take_along_axis(lens, parent[t], 1) + ~pf
        fin = pf | (word[t] == end)
    assert (lens == g['lengths']).all() and (fin == g['finished']).all()
    tree = ref.gather_tree(word, parent, g['lengths'].max(axis=1), end)
    assert (_tbw(g['predicted_ids']) == tree).all()
    return worst, Td


@pytest.mark.parametrize('B,T,W,C', [(1, 1, 4, 3), (3, 17, 64, 32), (3, 60, 4, 300), (1, 60, 1000, 32), (3, 17, 1000, 3),
                                     (1, 17, 64, 300)])
def test_decision_replay(B, T, W, C):
    rs = np.random.RandomState(B * 1000 + T * 10 + W + C)
    e = _engine(F, C, seed=B + T)
    feats, seq = _feats(B, T, F, rs)
    g = _gpu(e, feats, seq, W, 10, 1, C - 1)
    worst, Td = _replay_check(e, C, feats, g, W, 1, C - 1)
    print('LAS beam replay B=%d T=%d W=%d C=%d: %d steps, score rel err %.2e' % (B, T, W, C, Td, worst))


def test_decision_replay_reference_shape():
    """the reference's configuration: one utterance, F 840, T 400, W 1000, C 32, 100 steps"""
    Fr, C, W = 840, 32, 1000
    rs = np.random.RandomState(840)
    e = _engine(Fr, C, seed=7)
    feats, seq = _feats(1, 400, Fr, rs)
    g = _gpu(e, feats, seq, W, 100, 1, 2)
    worst, Td = _replay_check(e, C, feats, g, W, 1, 2)
    print('LAS beam replay reference shape: %d steps, score rel err %.2e' % (Td, worst))


def test_two_searches_same_bits():
    rs = np.random.RandomState(1)
    e = _engine(F, 32)
    feats, seq = _feats(2, 30, F, rs)
    a = _gpu(e, feats, seq, 1000, 20, 1, 2)
    b = _gpu(e, feats, seq, 1000, 20, 1, 2)
    for k in ('predicted_ids', 'scores', 'word_ids', 'parent_ids', 'log_probs', 'lengths', 'finished'):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a['steps'] == b['steps']


def test_arguments_and_handle_kinds():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine, WaveNetEngine
    from neuralasr_amd.features import Featurizer
    C = 8
    e = _engine(F, C)
    feats = np.zeros((1, 4, F), np.float32)
    seq = np.array([4], np.int32)
    fp = feats.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    ip = seq.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    steps = ctypes.c_int32()

    def call(h, W=4, S=5, start=1, end=2, lp=0.5):
        return e.lib.nasr_las_beam_search(h, fp, ip, 1, 4, W, S, start, end, lp, ctypes.byref(steps))

    assert call(e.h) == _lib.NASR_OK
    for kw in ({'W': 0}, {'W': 1025}, {'S': 0}, {'S': 1001}, {'start': -1}, {'start': C}, {'end': C}, {'end': -1},
               {'lp': -0.1}, {'lp': float('inf')}, {'lp': float('nan')}):
        assert call(e.h, **kw) == _lib.NASR_ERR_ARG, kw
    assert call(e.h, W=1024, S=1000) == _lib.NASR_OK
    others = [Engine(F, 16, 1, False, 'none', C), WaveNetEngine(F, C),
              Featurizer(16000, 13, 0)]
    for o in others:
        assert call(o.h) == _lib.NASR_ERR_STATE
        assert e.lib.nasr_las_beam_get_ids(o.h, ip) == _lib.NASR_ERR_STATE
    fresh = _engine(F, C)
    assert fresh.lib.nasr_las_beam_get_ids(fresh.h, ip) == _lib.NASR_ERR_STATE


def test_search_leaves_training_state_alone():
    C = 12
    rs = np.random.RandomState(4)
    feats, seq = _feats(3, 20, F, rs)
    labels = rs.randint(0, C, size=(3, 6)).astype(np.int32)
    ll = np.array([6, 3, 0], np.int32)

    def run(search):
        e = _engine(F, C)
        e.upload_batch(feats, seq, labels, ll)
        e.compute_grads()
        loss0, logits0 = e.get_loss(), e.logits()
        p0, s0, m0 = e.get_params(), e.sampling_state(), e.get_adam_state()
        g0 = e.get_grads()
        if search:
            _gpu(e, feats[:2, :15], seq[:2] - 5, 64, 8, 1, 2)
            assert e.get_params().tobytes() == p0.tobytes()
            assert e.sampling_state() == s0
            assert e.get_grads().tobytes() == g0.tobytes()
            m1 = e.get_adam_state()
            assert m1[0].tobytes() == m0[0].tobytes() and m1[1].tobytes() == m0[1].tobytes() and m1[2] == m0[2]
            assert e.get_loss() == loss0 and e.logits().tobytes() == logits0.tobytes()
        e.upload_batch(feats, seq, labels, ll)
        e.compute_grads()
        return e.get_loss(), e.get_grads(), e.logits(), e.sampling_state()

    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]
