"""Latency-controlled training on the GPU (nasr_set_chunking) through Engine and HipNetwork, against the fp64
model of the rule in tests/lc_train_ref.py - not against the GPU's own whole-utterance pass.  Tolerances: BASELINE.md §6's,
logits 1e-4 max-abs, loss 1e-4 relative, every gradient tensor and the parameters after three Adam steps 1e-4 relative
norm-wise.  Every shape is small: T = 23 frames, so that (C, R) = (4, 3), (1, 2) and (3, 7) give several windows, with
utterances of T_b <= C + R, T_b = jC + R, T_b = jC + R + 1 and one so short that it is idle in most windows.  The fp64
result of a case is computed once and shared."""
import ctypes
import os

import numpy as np
import pytest

from oracle import nasr_oracle as O
from tests import lc_train_ref as LC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')
TOL = 1e-4
T = 23


def make_engine(spec, lr=1e-3):
    from neuralasr_amd.engine import Engine
    return Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes,
                  forget_bias=spec.forget_bias, learning_rate=lr)


def rand_params(spec, seed):
    rs = np.random.RandomState(seed)
    return [p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=seed)]     # non-zero biases too


def lengths(C, R, B):
    """T_b = T (the longest), <= C + R, = jC + R, = jC + R + 1, and 2 frames (idle in most windows); then random ones"""
    j = max(1, (T - R - 1) // C)
    lens = [T, min(C + R, T - 1), j * C + R, j * C + R + 1, 2]
    assert all(1 <= n <= T for n in lens)
    rs = np.random.RandomState(B)
    return np.asarray(lens + [int(rs.randint(1, T + 1)) for _ in range(B - len(lens))], np.int32)


def batch(spec, C, R, B, seed):
    rs = np.random.RandomState(seed)
    seq_len = lengths(C, R, B)
    feats = rs.randn(B, T, spec.feature_size).astype(np.float32)
    for b in range(B):
        feats[b, seq_len[b]:] = 0
    Lmax = 4
    labels = np.zeros((B, Lmax), np.int32)
    label_len = np.zeros(B, np.int32)
    for b in range(B):
        n = min(Lmax, max(1, int(seq_len[b]) // 3))
        lab = rs.permutation(spec.num_classes - 1)[:n]             # distinct labels: feasible with n frames
        labels[b, :n], label_len[b] = lab, n
    return feats, seq_len, labels, label_len


CASES = {
    'c4r3': (3, 20, 5, 4, 3),          # L, H, B, C, R
    'c1r2': (3, 20, 5, 1, 2),          # every window carries
    'c3r7': (3, 20, 5, 3, 7),          # R > C: windows overlap more than once
    'b17': (3, 20, 17, 4, 3),          # a second M tile
    'h70': (3, 70, 5, 4, 3),           # Hp = 128
}
_ref = {}


def case(name):
    """(spec, params, batch, C, R, fp64 (loss, nll, grads, logits)) of a case, the fp64 part computed once"""
    L, H, B, C, R = CASES[name]
    spec = O.ModelSpec(26, H, L, True, 'concat', 29)
    if name not in _ref:
        params = rand_params(spec, 11)
        bt = batch(spec, C, R, B, 5)
        ref = LC.loss_and_grads(spec, params, bt[0].astype(np.float64), bt[1], bt[2], bt[3], C, R)
        for a in ref[2]:
            a.setflags(write=False)
        _ref[name] = (spec, params, bt, C, R, ref)
    return _ref[name]


def rel(x, y):
    return float(np.linalg.norm(np.asarray(x, np.float64) - y) / max(np.linalg.norm(y), 1e-30))


def assert_grads(spec, flat, ref_grads, what=''):
    off = 0
    for (name, shp), g in zip(spec.param_shapes(), ref_grads):
        n = int(np.prod(shp))
        r = rel(flat[off:off + n].reshape(shp), g)
        print(what, name, 'rel', r)
        assert r <= TOL, (what, name, r)
        off += n
    assert off == len(flat)


# ------------------------------------------------------------------------------------------- parity with the fp64 rule
@pytest.mark.parametrize('name', sorted(CASES))
def test_logits_loss_and_every_gradient(name):
    spec, params, (feats, seq_len, labels, label_len), C, R, (rloss, rnll, rgrads, rlogits) = case(name)
    e = make_engine(spec)
    mode = e.recurrence_mode
    e.set_params(O.flatten(params))
    assert e.chunking == (0, 0)
    e.set_chunking(C, R)
    assert e.chunking == (C, R)
    logits = e.forward(feats, seq_len)
    assert logits.shape == rlogits.shape
    print(name, 'logits max-abs', np.abs(logits - rlogits).max())
    assert np.abs(logits - rlogits).max() <= TOL
    loss, nll, grads = e.loss_and_grads(feats, seq_len, labels, label_len)
    print(name, 'loss', loss, rloss)
    assert abs(loss - rloss) <= TOL * abs(rloss)
    assert np.abs(nll - rnll).max() <= TOL * np.abs(rnll).max()
    assert_grads(spec, grads, rgrads, name)
    # it is not the whole-utterance network
    e.set_chunking(0)
    whole = e.forward(feats, seq_len)
    assert np.abs(whole - rlogits).max() > 100 * TOL
    # the greedy decoder reads the chunked logits
    e.set_chunking(C, R)
    assert e.greedy_decode(feats, seq_len) == O.greedy_decode(logits.astype(np.float64), seq_len)
    assert e.recurrence_mode == mode
    e.close()


def test_one_window_is_the_handles_whole_utterance_step():
    """C + R >= T: the chunked pass against the handle's own whole-utterance pass on the per-step kernels"""
    spec, params, (feats, seq_len, labels, label_len), _, _, _ = case('c4r3')
    e = make_engine(spec)
    e.set_params(O.flatten(params))
    e.set_recurrence_mode(0)
    want_logits = e.forward(feats, seq_len)
    want_loss, want_nll, want_grads = e.loss_and_grads(feats, seq_len, labels, label_len)
    for C, R in ((20, 3), (1, 22), (4096, 1024)):
        e.set_chunking(C, R)
        logits = e.forward(feats, seq_len)
        assert np.abs(logits - want_logits).max() <= TOL
        loss, nll, grads = e.loss_and_grads(feats, seq_len, labels, label_len)
        assert abs(loss - want_loss) <= TOL * abs(want_loss)
        assert_grads(spec, grads, O.unflatten(spec, want_grads.astype(np.float64)), 'C%d' % C)
    e.close()


# ------------------------------------------------------------------------------------------- consistency with serving
@pytest.mark.parametrize('name', ['c4r3', 'c1r2', 'c3r7'])
def test_chunked_forward_is_what_a_session_of_the_handle_serves(name):
    spec, params, (feats, seq_len, _, _), C, R, _ = case(name)
    e = make_engine(spec)
    e.set_params(O.flatten(params))
    e.set_chunking(C, R)
    logits = e.forward(feats, seq_len)
    e.stream_open_lookahead(1, R)                         # sessions are not affected by the chunking
    for b, n in enumerate(int(x) for x in seq_len):
        got, pos = [], 0
        feeds = LC.session_feeds(n, C, R)
        for i, k in enumerate(feeds):
            rows = feats[b:b + 1, pos:pos + k]
            lg, emitted = e.stream_feed_lookahead(np.ascontiguousarray(rows), [k], [i == len(feeds) - 1])
            got.append(lg[:emitted[0], 0])
            pos += k
        got = np.concatenate(got)
        assert got.shape == (n, spec.num_classes)
        assert np.abs(got - logits[:n, b]).max() <= TOL, (b, n)
        e.stream_reset()
    e.stream_close()
    again = e.forward(feats, seq_len)                     # ... and the chunking not by the session
    assert again.tobytes() == logits.tobytes()
    e.close()


# ------------------------------------------------------------------------------------------- stability
def test_two_runs_give_the_same_bits():
    spec, params, bt, C, R, _ = case('c1r2')
    e = make_engine(spec)
    e.set_params(O.flatten(params))
    e.set_chunking(C, R)
    e.upload_batch(*bt)
    e.compute_grads()
    a, la = e.get_grads(), e.get_loss()
    e.compute_grads()
    b, lb = e.get_grads(), e.get_loss()
    assert a.tobytes() == b.tobytes() and np.float32(la).tobytes() == np.float32(lb).tobytes()
    assert np.abs(a).max() > 0
    e.close()


def test_three_adam_steps_and_off_again():
    """three chunked steps against fp64 Adam on the fp64 gradients; the recurrence mode stays what it was; with chunking
    off again the step has the bits it had before chunking was ever on"""
    spec, params, bt, C, R, _ = case('c4r3')
    lr = 1e-3
    e = make_engine(spec, lr)
    mode = e.recurrence_mode
    n = e.param_count
    p0 = O.flatten(params).astype(np.float32)

    def start():
        e.set_params(p0)
        e.set_adam_state(np.zeros(n, np.float32), np.zeros(n, np.float32), 0)

    start()
    before = (e.train_step(*bt), e.get_params())
    start()
    e.set_chunking(C, R)
    p = O.unflatten(spec, p0.astype(np.float64))
    m, v = [np.zeros_like(q) for q in p], [np.zeros_like(q) for q in p]
    f64 = bt[0].astype(np.float64)
    for step in range(1, 4):
        rloss, _, g, _ = LC.loss_and_grads(spec, p, f64, bt[1], bt[2], bt[3], C, R)
        loss = e.train_step(*bt)
        assert abs(loss - rloss) <= TOL * abs(rloss), step
        p, m, v = O.adam_tf(p, g, m, v, step, lr)
        assert e.recurrence_mode == mode
    got = O.unflatten(spec, e.get_params())
    for (name, _), a, b in zip(spec.param_shapes(), got, p):
        print('after 3 steps', name, rel(a, b))
        assert rel(a, b) <= TOL, name
    assert not e.step_void()
    e.set_chunking(0)
    assert e.chunking == (0, 0) and e.recurrence_mode == mode
    start()
    after = (e.train_step(*bt), e.get_params())
    assert np.float32(before[0]).tobytes() == np.float32(after[0]).tobytes()
    assert before[1].tobytes() == after[1].tobytes()
    e.close()


def test_a_change_drops_the_resident_batch():
    from neuralasr_amd import _lib
    spec, params, bt, C, R, _ = case('c4r3')
    e = make_engine(spec)
    e.set_params(O.flatten(params))
    e.upload_batch(*bt)
    e.set_chunking(C, R)
    with pytest.raises(_lib.NasrError) as err:
        e.compute_grads()
    assert err.value.code == _lib.NASR_ERR_STATE and 'no resident batch' in str(err.value)
    e.upload_batch(*bt)
    e.compute_grads()
    e.set_chunking(C, R)                  # no change: the batch stays
    e.compute_grads()
    e.close()


# ------------------------------------------------------------------------------------------- gradient buckets
def test_gradient_read_bucket_by_bucket():
    """every bucket cloned on a side stream behind nasr_grad_bucket_wait, put back into a cleared buffer: nasr_get_grads
    then returns what it returned for the whole buffer"""
    import torch
    spec, params, bt, C, R, _ = case('c4r3')
    e = make_engine(spec)
    e.set_params(O.flatten(params))
    e.set_chunking(C, R)
    e.upload_batch(*bt)
    e.compute_grads()
    want = e.get_grads()
    gt = e.grad_tensor()
    buckets = e.grad_buckets()
    assert len(buckets) == spec.num_layers and sum(c for _, c in buckets) == gt.numel()
    e.compute_grads()
    side = torch.cuda.Stream()
    parts = []
    with torch.cuda.stream(side):
        for i, (off, cnt) in enumerate(buckets):
            e.bucket_wait(i, side.cuda_stream)
            parts.append(gt[off:off + cnt].clone())
    torch.cuda.synchronize()
    e.synchronize()
    gt.zero_()
    torch.cuda.synchronize()
    assert not e.get_grads().any()
    for (off, cnt), part in zip(buckets, parts):
        gt[off:off + cnt].copy_(part)
    torch.cuda.synchronize()
    assert e.get_grads().tobytes() == want.tobytes()
    e.close()


# ------------------------------------------------------------------------------------------- clipping
def test_clipping_uses_the_norm_of_the_chunked_gradient():
    spec, params, bt, C, R, (_, _, rgrads, _) = case('c4r3')
    norm = float(np.linalg.norm(O.flatten(rgrads)))
    e = make_engine(spec)
    e.set_params(O.flatten(params))
    e.set_chunking(C, R)
    e.set_grad_clip(norm / 3)
    e.train_step(*bt)
    st = e.grad_clip_stats()
    print('norm', st['last_norm'], norm, 'coef', st['last_coef'])
    assert abs(st['last_norm'] - norm) <= TOL * norm
    assert st['clipped'] == 1 and st['skipped'] == 0 and abs(st['last_coef'] - 1 / 3) <= 1e-3
    # the whole-utterance gradient has another norm
    e.set_chunking(0)
    e.set_params(O.flatten(params))
    e.train_step(*bt)
    assert abs(e.grad_clip_stats()['last_norm'] - norm) > 10 * TOL * norm
    e.close()


# ------------------------------------------------------------------------------------------- refusals
def refused(call, code, *words):
    from neuralasr_amd import _lib
    with pytest.raises(_lib.NasrError) as err:
        call()
    assert err.value.code == code, str(err.value)
    for w in words:
        assert w in str(err.value), str(err.value)


def test_refusals():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import Engine, LasEngine, WaveNetEngine
    from neuralasr_amd.features import Featurizer
    STATE, ARG = _lib.NASR_ERR_STATE, _lib.NASR_ERR_ARG
    e = Engine(8, 16, 1, False, 'none', 5)
    refused(lambda: e.set_chunking(4, 3), STATE, 'nasr_set_chunking', 'unidirectional', 'causal already')
    e.set_chunking(0)                                      # off is no change
    assert e.chunking == (0, 0)
    e.close()
    e = Engine(8, 16, 1, True, 'stack_reshape', 5)
    refused(lambda: e.set_chunking(4, 3), STATE, 'nasr_set_chunking', 'NASR_MERGE_STACK_RESHAPE', 'point in time')
    assert e.chunking == (0, 0)
    e.close()
    e = Engine(8, 16, 1, True, 'concat', 5, pre=(12,), post=0, relu_clip=2.0, dropout=(0.0,))
    refused(lambda: e.set_chunking(4, 3), STATE, 'nasr_set_chunking', 'dense stages')
    assert e.chunking == (0, 0)
    e.close()
    e = Engine(8, 16, 1, True, 'concat', 5, pre=(12,), post=0, relu_clip=2.0, dropout=(0.1,))
    refused(lambda: e.set_chunking(4, 3), STATE, 'nasr_set_chunking', 'dropout[0]', 'cannot stream')
    e.close()
    for e in (WaveNetEngine(39, 29), LasEngine(39, 29)):
        refused(lambda: e._ck(e.lib.nasr_set_chunking(e.h, 4, 3)), STATE, 'nasr_set_chunking', 'WaveNet or LAS')
        e.close()
    f = Featurizer(16000, 13, 2)
    assert f.lib.nasr_set_chunking(f.h, 4, 3) == STATE
    msg = f.lib.nasr_last_error(f.h).decode()
    assert 'nasr_set_chunking' in msg and 'featurizer handle has no model' in msg
    c, r = ctypes.c_int(7), ctypes.c_int(7)
    assert f.lib.nasr_get_chunking(f.h, ctypes.byref(c), ctypes.byref(r)) == STATE
    f.close()
    e = Engine(8, 16, 2, True, 'concat', 5)
    for C, R, word in ((-1, 3, '[1,4096]'), (4097, 3, '[1,4096]'), (4, 0, '[1,1024]'), (4, 1025, '[1,1024]')):
        refused(lambda: e.set_chunking(C, R), ARG, 'nasr_set_chunking', word)
        assert e.chunking == (0, 0)
    e.set_chunking(4, 3)
    refused(lambda: e.set_chunking(4, 0), ARG, '[1,1024]')
    assert e.chunking == (4, 3)
    e.stream_open_lookahead(1, 3)
    refused(lambda: e.set_chunking(5, 3), STATE, 'nasr_set_chunking', 'stream session is open')
    refused(lambda: e.set_chunking(0), STATE, 'stream session is open')
    assert e.chunking == (4, 3)
    e.stream_close()
    e.set_chunking(0, 99)
    assert e.chunking == (0, 0)
    e.close()


# ------------------------------------------------------------------------------------------- the sample set, from a config
def config_with(tmp_path, network, **extra):
    out = []
    for ln in open(os.path.join(SAMPLES, 'toy.config')).read().splitlines():
        if ln.startswith('output='):
            ln = 'output=' + SAMPLES
        elif ln.startswith('model_dir='):
            ln = 'model_dir=' + str(tmp_path / 'model')
        elif ln.startswith('network='):
            ln = 'network=networks.' + network
        out.append(ln)
        if ln.strip() == '[Parameters]':
            out += ['%s=%s' % kv for kv in extra.items()]
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_network_from_config_trains_and_evaluates_in_windows(tmp_path, monkeypatch):
    from neuralasr_amd import _lib
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    from neuralasr_amd.networks.bilstm_ctc_net import BiLstm3x500CTCNet
    monkeypatch.setattr(BiLstm3x500CTCNet, 'num_hidden', 24)
    cfg = Config(config_with(tmp_path, 'bilstm_ctc_net.BiLstm3x500CTCNet', chunk_frames=2, stream_lookahead=1), True)
    net = cfg.load_network(fortraining=True)
    assert net.engine.chunking == (2, 1)        # the toy utterances have 5 to 9 frames: three windows and more
    ds = DataSet(cfg.train_input, cfg)
    for _ in range(2):
        if not ds.has_more_batches():
            ds.reset_epoch()
        loss, _ = net.train(*ds.get_next_batch())
        assert np.isfinite(loss)
    ds.reset_epoch()
    bt = ds.get_next_batch()
    vloss, vler = net.validate(*bt)
    ids, eloss, eler = net.evaluate(*bt)
    assert np.isfinite(vloss) and np.isfinite(eloss) and 0 <= vler and 0 <= eler
    spans = net.align(*bt)
    assert len(spans) == len(bt[2]) and all(np.isfinite(s[0]) for s in spans)
    # the loss validate() reports is the chunked graph's: with chunking off it is another number
    net.engine.set_chunking(0)
    wloss, _ = net.validate(*bt)
    assert wloss != vloss
    assert np.isfinite(net.engine.get_params()).all()
    net.engine.close()
    # without the keys nothing is set; a network the library refuses says why at construction
    off = Config(config_with(tmp_path, 'bilstm_ctc_net.BiLstm3x500CTCNet'), True).load_network(fortraining=True)
    assert off.engine.chunking == (0, 0)
    off.engine.close()
    bad = Config(config_with(tmp_path, 'bilstm_ctc_net.BiLstmCTCNet', chunk_frames=2, stream_lookahead=1), True)
    with pytest.raises(_lib.NasrError, match='NASR_MERGE_STACK_RESHAPE'):
        bad.load_network(fortraining=True)
