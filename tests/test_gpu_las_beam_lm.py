"""The LAS beam search fused with an n-gram table on the GPU (nasr_las_beam_set_lm) against
tests/las_beam_lm_ref.py: exactly when all weights are zero and the table alone drives the search; on a trained-like model
by the fp64 replay along the GPU's trace and, where every step's margin is far above float32 rounding, decision by
decision against the restatement; the bits of the plain search when the table cannot matter; what a fused search leaves
alone; the error paths; and the two networks' decode / evaluate with lm_file in the config.

Seeds were chosen on the host from the restatement's own margins (asserted below); a margin of 1e-3 is two orders of
magnitude above the float32 error of a total of a dozen log-probs."""
import ctypes
import os

import numpy as np
import pytest

from tests import las_beam_lm_ref as ref
from tests.test_gpu_las_beam import F, _engine, _feats, _gpu, _tbw

pytestmark = pytest.mark.gpu

FP, IP = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
KEYS = ('predicted_ids', 'scores', 'word_ids', 'parent_ids', 'log_probs', 'lengths', 'finished')


def random_table(rs, C, order, end, boost=0.0):
    """float32 [K][C]: rows of random log-probabilities, the end id's column raised by `boost` first"""
    x = rs.randn(C ** (order - 1), C) * 1.5
    x[:, end] += boost
    return (x - np.log(np.exp(x).sum(1, keepdims=True))).astype(np.float32)


def same_bits(a, b):
    assert a['steps'] == b['steps']
    for k in KEYS:
        assert a[k].tobytes() == b[k].tobytes(), k


# C, order, W, boost of the end id, seed: with boost 2.5 every beam finishes before step 12, with 0 the search is cut there
EXACT = [(5, 1, 1, 0.0, 0), (5, 2, 3, 2.5, 0), (5, 3, 8, 2.5, 0), (5, 2, 16, 2.5, 0), (7, 1, 3, 2.5, 2), (7, 2, 8, 2.5, 3),
         (7, 3, 1, 2.5, 3), (7, 3, 16, 2.5, 1), (5, 3, 8, 0.0, 0), (5, 2, 16, 0.0, 3), (7, 3, 3, 0.0, 0)]


@pytest.mark.parametrize('C,order,W,boost,seed', EXACT)
def test_exact_when_the_table_alone_drives_the_search(C, order, W, boost, seed):
    """all weights zero: the logits are the (zero) projection bias for every row, and ids, parents, lengths and contexts
    are the restatement's; two utterances of different length see the same logits and must agree with each other too"""
    rs = np.random.RandomState(seed)
    table = random_table(rs, C, order, C - 1, boost)
    B, T, steps, start, end = 2, 6, 12, 1, C - 1
    e = _engine(F, C, zero=True)
    e.set_lm((table, order), 1.0)
    feats = rs.randn(B, T, F).astype(np.float32)
    g = _gpu(e, feats, np.array([T, 3], np.int32), W, steps, start, end)
    r = ref.beam_search_lm(lambda t, p, ids: np.zeros((B, W, C), np.float32), B, W, C, start, end, steps, 0.5, table, order,
                           1.0)
    assert r['margin'].min() > 1e-3, r['margin']
    assert (r['steps'] < steps) == (boost > 0)
    print('LAS beam LM exact C=%d order=%d W=%d: T_dec %d, least margin %.3g' % (C, order, W, r['steps'], r['margin'].min()))
    assert g['steps'] == r['steps']
    assert (_tbw(g['word_ids']) == r['word']).all()
    assert (_tbw(g['parent_ids']) == r['parent']).all()
    assert (g['lengths'] == r['lengths']).all() and (g['finished'] == r['finished']).all()
    assert (_tbw(g['predicted_ids']) == r['ids']).all()
    ctx = e.lm_context(B, W)
    assert (ctx == r['ctx']).all()
    assert (ctx == ref.contexts_along(r['word'], r['parent'], order, C, start, end)).all()
    gs, rsc = _tbw(g['scores']), r['scores']
    assert ((gs == -np.inf) == (rsc == -np.inf)).all()
    fin = np.isfinite(rsc)
    np.testing.assert_allclose(gs[fin], rsc[fin], rtol=1e-6)
    lfin = np.isfinite(r['log_probs'])
    np.testing.assert_allclose(g['log_probs'][lfin], r['log_probs'][lfin], rtol=1e-6)


def _sharp_engine(C, seed, scale):
    """random init with the projection kernel scaled up: logits that depend on the utterance as a trained model's do"""
    e = _engine(F, C, seed=seed)
    flat = e.get_params()
    for name, off, rows, cols in e.tensors():
        if name == 'projection_layer/kernel':
            flat[off:off + rows * cols] *= scale
    e.set_params(flat)
    return e


def test_an_utterance_that_finished_early_keeps_its_contexts():
    """utterance 1 has every beam finished after step 5, utterance 0 runs into the cut at 14 steps: nine more updates gather
    utterance 1's rows by parent and must carry their contexts unchanged"""
    C, W, order, T, steps, start, end, seed = 7, 3, 2, 9, 14, 1, 6, 10
    rs = np.random.RandomState(seed)
    e = _sharp_engine(C, seed, 40.0)
    feats = rs.randn(2, T, F).astype(np.float32)
    table = random_table(rs, C, order, end, 1.0)
    e.set_lm((table, order), 0.7)
    g = _gpu(e, feats, np.full(2, T, np.int32), W, steps, start, end)
    r = ref.beam_search_lm(ref.Replay(e.get_params(), F, C, feats, W), 2, W, C, start, end, steps, 0.5, table, order, 0.7)
    print('LAS beam LM early finish: done_at %s, T_dec %d, least margin %.3g' % (r['done_at'], r['steps'], r['margin'].min()))
    assert r['margin'].min() > 1e-3 and r['steps'] == steps and r['done_at'][1] + 3 <= r['done_at'][0]
    assert g['steps'] == r['steps']
    assert (_tbw(g['word_ids']) == r['word']).all() and (_tbw(g['parent_ids']) == r['parent']).all()
    assert (g['finished'] == r['finished']).all() and (g['lengths'] == r['lengths']).all()
    ctx = e.lm_context(2, W)
    assert (ctx == r['ctx']).all()
    assert (ctx == ref.contexts_along(_tbw(g['word_ids']), _tbw(g['parent_ids']), order, C, start, end)).all()
    np.testing.assert_allclose(_tbw(g['scores']), r['scores'], rtol=2e-5)


def _replay_check_lm(e, C, feats, g, W, start, end, table, order, lm_weight, weight=0.5, rtol=1e-5):
    """tests/test_gpu_las_beam.py's decision replay with the fused term: the fp64 model follows the GPU's trace; at every
    step the GPU's scores agree with fp64 within rtol and its choice is the best W up to that tolerance (so only steps
    whose margin exceeds float32 rounding can tell the two apart).  Returns (largest relative score error, steps)."""
    B, Td, K = feats.shape[0], g['steps'], C ** (order - 1)
    rp = ref.Replay(e.get_params(), feats.shape[2], C, feats, W)
    word, parent, scores = _tbw(g['word_ids']), _tbw(g['parent_ids']), _tbw(g['scores'])
    tab = np.asarray(table, np.float64).reshape(K, C)
    logp = np.full((B, W), -np.inf)
    logp[:, 0] = 0
    fin = np.ones((B, W), bool)
    fin[:, 0] = False
    lens = np.zeros((B, W), np.int64)
    ctx = np.full((B, W), ref.start_context(order, C, start), np.int64)
    is_end = np.arange(C) == end
    worst = 0.0
    for t in range(Td):
        logits = rp(t, None if t == 0 else parent[t - 1], np.full((B, W), start) if t == 0 else word[t - 1])
        mx = logits.max(-1, keepdims=True)
        lp = logits - (np.log(np.exp(logits - mx).sum(-1, keepdims=True)) + mx) + lm_weight * tab[ctx]
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
            assert (gsc[~inA & ~lo] == -np.inf).all()
            if A.size >= W:
                assert inA.all(), (t, b)
                rest = np.setdiff1d(A, chosen)
                if rest.size:
                    tol = rtol * max(abs(sA[chosen].min()), 1e-6)
                    assert sA[chosen].min() >= sA[rest].max() - 2 * tol, (t, b)
            else:
                assert np.isin(A, chosen).all(), (t, b)
        sel = parent[t] * C + word[t]
        logp = np.take_along_axis(total.reshape(B, W * C), sel, 1)
        pf = np.take_along_axis(fin, parent[t], 1)
        pc = np.take_along_axis(ctx, parent[t], 1)
        ctx = np.where(pf, pc, (pc * C + word[t]) % K)
        lens = np.take_along_axis(lens, parent[t], 1) + ~pf
        fin = pf | (word[t] == end)
    assert (lens == g['lengths']).all() and (fin == g['finished']).all()
    assert (ctx == e.lm_context(B, W)).all()
    assert (_tbw(g['predicted_ids']) == ref.gather_tree(word, parent, g['lengths'].max(axis=1), end)).all()
    return worst, Td


# C 70: the score kernel's lane-strided loop wraps and K is no power of two; C 32 at order 3: K = 1024
@pytest.mark.parametrize('B,T,W,C,order', [(3, 17, 64, 70, 2), (2, 17, 64, 32, 3), (1, 9, 1000, 32, 3)])
def test_trace_against_the_fp64_replay(B, T, W, C, order):
    rs = np.random.RandomState(B * 1000 + T * 10 + W + C)
    e = _engine(F, C, seed=B + T)
    feats, seq = _feats(B, T, F, rs)
    table = random_table(rs, C, order, C - 1)
    e.set_lm((table, order), 0.3)
    g = _gpu(e, feats, seq, W, 10, 1, C - 1)
    worst, Td = _replay_check_lm(e, C, feats, g, W, 1, C - 1, table, order, 0.3)
    print('LAS beam LM replay B=%d T=%d W=%d C=%d order=%d: %d steps, score rel err %.2e' % (B, T, W, C, order, Td, worst))
    # the table matters: the plain search of the same model takes another path
    e.set_lm(None)
    assert _gpu(e, feats, seq, W, 10, 1, C - 1)['word_ids'].tobytes() != g['word_ids'].tobytes()


@pytest.mark.parametrize('C,order,W', [(32, 3, 64), (70, 2, 7)])
def test_a_table_that_cannot_matter_gives_the_plain_searchs_bits(C, order, W):
    rs = np.random.RandomState(C)
    e = _engine(F, C)
    feats, seq = _feats(2, 21, F, rs)
    plain = _gpu(e, feats, seq, W, 12, 1, 2)
    assert (e.lm_context(2, W) == 0).all()
    e.set_lm((random_table(rs, C, order, 2), order), 0.0)
    same_bits(plain, _gpu(e, feats, seq, W, 12, 1, 2))
    e.set_lm((random_table(rs, C, order, 2), order), 0.8)
    fused = _gpu(e, feats, seq, W, 12, 1, 2)
    assert fused['scores'].tobytes() != plain['scores'].tobytes()
    e.set_lm(None)
    same_bits(plain, _gpu(e, feats, seq, W, 12, 1, 2))


def test_fused_search_leaves_training_state_alone_and_resident_agrees():
    C, order = 12, 2
    rs = np.random.RandomState(4)
    feats, seq = _feats(3, 20, F, rs)
    labels = rs.randint(0, C, size=(3, 6)).astype(np.int32)
    ll = np.array([6, 3, 0], np.int32)
    table = random_table(rs, C, order, 2)

    def run(search):
        e = _engine(F, C)
        e.upload_batch(feats, seq, labels, ll)
        e.compute_grads()
        loss0, logits0 = e.get_loss(), e.logits()
        p0, s0, m0, g0 = e.get_params(), e.sampling_state(), e.get_adam_state(), e.get_grads()
        if search:
            e.set_lm((table, order), 0.5)
            host = _gpu(e, feats, seq, 64, 8, 1, 2)
            resident = e.beam_search_resident(64, 8, 1, 2, 0.5, trace=True)
            same_bits(host, resident)                       # the resident batch is the very batch given from the host
            other = _gpu(e, feats[:2, :15], seq[:2] - 5, 64, 8, 1, 2)
            assert other['steps'] >= 1
            assert e.get_params().tobytes() == p0.tobytes() and e.sampling_state() == s0
            assert e.get_grads().tobytes() == g0.tobytes()
            m1 = e.get_adam_state()
            assert m1[0].tobytes() == m0[0].tobytes() and m1[1].tobytes() == m0[1].tobytes() and m1[2] == m0[2]
            assert e.get_loss() == loss0 and e.logits().tobytes() == logits0.tobytes()
        e.compute_grads()                                   # on the batch that is still resident
        return e.get_loss(), e.get_grads(), e.logits()

    a, b = run(False), run(True)
    assert a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()


def test_error_paths():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine, WaveNetEngine
    from neuralasr_amd.features import Featurizer
    C = 70
    e = _engine(F, C)
    lib = e.lib
    small = np.zeros(C * C, np.float32)
    p = small.ctypes.data_as(FP)
    out = np.zeros(8, np.int32)
    assert lib.nasr_las_beam_get_lm_context(e.h, out.ctypes.data_as(IP)) == _lib.NASR_ERR_STATE      # no search yet
    for order in (0, 5, -1):
        assert lib.nasr_las_beam_set_lm(e.h, p, order, 0.5) == _lib.NASR_ERR_ARG
    assert lib.nasr_las_beam_set_lm(e.h, p, 4, 0.5) == _lib.NASR_ERR_ARG          # 70^4 > 2^24: refused before it is read
    assert lib.nasr_las_beam_set_lm(e.h, p, 2, float('nan')) == _lib.NASR_ERR_ARG
    assert lib.nasr_las_beam_set_lm(e.h, p, 2, float('inf')) == _lib.NASR_ERR_ARG
    assert lib.nasr_las_beam_set_lm(None, p, 2, 0.5) == _lib.NASR_ERR_ARG
    for bad in (-np.inf, np.inf, np.nan):                                          # 0 * -inf is NaN: entries must be finite
        t = np.zeros(C * C, np.float32)
        t[C * C - 1] = bad
        assert lib.nasr_las_beam_set_lm(e.h, t.ctypes.data_as(FP), 2, 0.5) == _lib.NASR_ERR_ARG
    for o in (Engine(F, 16, 1, False, 'none', C), WaveNetEngine(F, C), Featurizer(16000, 13, 0)):
        assert lib.nasr_las_beam_set_lm(o.h, p, 2, 0.5) == _lib.NASR_ERR_STATE
        assert lib.nasr_las_beam_set_lm(o.h, None, 0, 0.0) == _lib.NASR_ERR_STATE
        assert lib.nasr_las_beam_get_lm_context(o.h, out.ctypes.data_as(IP)) == _lib.NASR_ERR_STATE
    with pytest.raises(ValueError):
        e.set_lm((np.zeros((C, C - 1), np.float32), 2), 0.5)
    # none of the refused calls set a table: the search is the plain one
    feats, seq = _feats(1, 8, F, np.random.RandomState(0))
    a = _gpu(e, feats, seq, 4, 5, 1, 2)
    assert lib.nasr_las_beam_get_lm_context(e.h, None) == _lib.NASR_ERR_ARG
    assert lib.nasr_las_beam_set_lm(e.h, p, 2, 0.5) == _lib.NASR_OK
    assert lib.nasr_las_beam_set_lm(e.h, None, 0, 0.0) == _lib.NASR_OK
    same_bits(a, _gpu(e, feats, seq, 4, 5, 1, 2))


def _toy_config(tmp_path, name, network, extra=()):
    samples = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sample_set')
    over = {'output': samples, 'model_dir': str(tmp_path / ('model_' + name)), 'num_gpus': '1', 'network': network}
    out = []
    for ln in open(os.path.join(samples, 'toy.config')).read().splitlines():
        key = ln.split('=')[0]
        out.append('%s=%s' % (key, over[key]) if key in over and '=' in ln else ln)
        if ln == '[Parameters]':
            out.extend(extra)
        if ln == '[MFCC Featurizer]':
            out.extend(['start_marker=a', 'end_marker=b'])
    p = tmp_path / (name + '.config')
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_networks_decode_with_the_configured_model(tmp_path):
    """BiLstmCTCNet.evaluate and LAS.decode with lm_file in the config return what the C entry points return for the same
    logits / batch with that model; the same config without the key returns the plain result"""
    from neuralasr_amd import lm
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    rs = np.random.RandomState(5)
    model_file = str(tmp_path / 'lm.npz')
    base = Config(_toy_config(tmp_path, 'plain_ctc', 'networks.bilstm_ctc_net.BiLstmCTCNet'), True)
    C = base.symbols.counter
    x = rs.randn(C, C + 1) * 2.0
    x = x - np.log(np.exp(x).sum(1, keepdims=True))
    model = lm.NGramLM(x[:, :C], x[:, C], 2, C, 0)
    model.save(model_file)
    keys = ['lm_file=' + model_file, 'lm_weight=1.5', 'lm_bonus=0.75']
    mfccs, labels, seq_len, labels_len = DataSet(base.train_input, base).get_next_batch()

    plain = base.load_network(fortraining=True)
    fused = Config(_toy_config(tmp_path, 'fused_ctc', 'networks.bilstm_ctc_net.BiLstmCTCNet', keys), True).load_network(True)
    fused.engine.set_params(plain.engine.get_params())
    logits = plain.engine.forward(mfccs, seq_len)
    want_plain = plain.engine.beam_search(logits, seq_len, 100, True)[0]
    want_fused = plain.engine.beam_search(logits, seq_len, 100, True, lm=model, lm_weight=1.5, lm_bonus=0.75)[0]
    assert want_plain != want_fused
    flat = lambda hyps: [i for h in hyps for i in h]                                       # noqa: E731
    assert plain.evaluate(mfccs, labels, seq_len, labels_len)[0].tolist() == flat(want_plain)
    out, _, ler = fused.evaluate(mfccs, labels, seq_len, labels_len)
    assert out.tolist() == flat(want_fused)
    assert float(ler) == pytest.approx(plain.engine.label_error_rate(want_fused, labels, labels_len))
    assert fused.decode(mfccs, seq_len).tolist() == flat(want_fused)
    # validate() is the reference's graph: no model in it
    assert fused.validate(mfccs, labels, seq_len, labels_len)[1] == plain.validate(mfccs, labels, seq_len, labels_len)[1]

    las_plain = Config(_toy_config(tmp_path, 'plain_las', 'networks.las.LAS'), True).load_network(True)
    las_fused = Config(_toy_config(tmp_path, 'fused_las', 'networks.las.LAS', keys), True).load_network(True)
    las_fused.engine.set_params(las_plain.engine.get_params())
    for net in (las_plain, las_fused):
        net.beam_width, net.max_decode_steps = 8, 6
    e = las_plain.engine
    start, end = las_plain._markers()
    want_plain = e.beam_search(mfccs, seq_len, 8, 6, start, end, 0.5)['predicted_ids'][0, :, 0]
    e.set_lm(model, 1.5)
    want_fused = e.beam_search(mfccs, seq_len, 8, 6, start, end, 0.5)['predicted_ids'][0, :, 0]
    e.set_lm(None)
    assert want_plain.tolist() != want_fused.tolist()
    assert las_plain.decode(mfccs, seq_len).tolist() == want_plain.tolist()
    assert las_fused.decode(mfccs, seq_len).tolist() == want_fused.tolist()
    assert las_fused.evaluate(mfccs, labels, seq_len, labels_len)[0][0].tolist() == want_fused.tolist()
